"""What the host does in train mode (nefes_amd/train.py), on the CPU: tools/make_golden_train_routes.py replays every case of its list
-- the four autograd Functions over the tuned shapes on both pipes, the layered dX chain, a reduced embedding, a supplied encoding,
the generic kernels at five (width, depth) pairs, frozen parameters, ray gradients, and the refusals -- against a recording library
whose weight-gradient launch fills its partials with a counter.  Each outcome (every C call with its arguments and every timer key
in order, the digest of all parameter gradients, or the exception's class) must equal the one recorded in
tests/golden/train_routes.json, case by case."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import make_golden_train_routes as G      # noqa: E402


def test_train_routes_match_the_recorded_ones():
    with open(os.path.join(ROOT, "tests", "golden", "train_routes.json")) as f:
        rec = json.load(f)
    wrong, ids = [], []
    with G.patched():
        for k, (cid, thunk) in enumerate(G.cases()):
            ids.append(cid)
            got = thunk()
            want = [rec["events"][i] for i in rec["cases"][k]] if k < rec["n"] else ["<no such case in the fixture>"]
            if got != want:
                at = next((j for j, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
                wrong.append(f"{cid}\n    first difference at event {at} of {len(want)} recorded / {len(got)} now\n"
                             f"    recorded: {want[at] if at < len(want) else '<end>'}\n    now:      {got[at] if at < len(got) else '<end>'}")
    assert len(ids) == rec["n"] == len(rec["cases"])
    assert hashlib.sha256("\n".join(ids).encode()).hexdigest() == rec["ids_sha256"], "the case list differs from the recorded one"
    assert not wrong, f"{len(wrong)} of {len(ids)} cases changed:\n" + "\n".join(wrong[:40])


def test_patches_are_undone():
    from nefes_amd import lib as L
    from nefes_amd import ops
    from nefes_amd import train as T
    state = lambda: (L.load, ops._chk, ops._stream, ops._timed, T._generic_buffers_fit, ops.SPLIT, ops.GENERIC_TRAIN, ops.GENERIC_TRAIN_EXT,
                     ops.TAP, T.FUSED_DX, T.DEBUG)
    before = state()
    with G.patched():
        G.set_switches({"SPLIT": "f32", "GENERIC_TRAIN": True, "FUSED_DX": False, "DEBUG": {}})
    assert state() == before


def test_field_train_any_picks_the_function_render_picked():
    """train.field_train_any, the dispatcher render() calls: a tuned pack goes to field_train / field_train_encoded whatever the
    switches say; a generic pack goes to field_train_generic only with GENERIC_TRAIN, behind an xyz encoder to
    field_train_generic_encoded only with GENERIC_TRAIN_EXT (GENERIC_TRAIN does not reach it), and is refused otherwise.  "Goes to" =
    the same C calls, timer keys and parameter gradients as the function called directly."""
    import itertools
    from nefes_amd import train as T
    direct = {(False, False): lambda net, mode, grid, *r: T.field_train(net, mode, *r), (False, True): T.field_train_encoded,
              (True, False): lambda net, mode, grid, *r: T.field_train_generic(net, mode, *r), (True, True): T.field_train_generic_encoded}
    with G.patched():
        for generic, behind_grid, gt, gte in itertools.product((False, True), repeat=4):
            shape = dict(D=6, W=64) if generic else dict(W=256)
            net = lambda: G.prepare(G.network(shape["W"], 16, 1, D=shape.get("D", 8), xyz=32 if behind_grid else 63))

            def through(f, pack):
                def call(n, mode):
                    pk = () if not pack else ((n.packed_generic() if generic else n.packed()),)
                    return f(n, *pk, mode, G._Grid() if behind_grid else None, *G.rays()), ()
                return call
            got = G.run(through(T.field_train_any, True), net(), G.FULL, T.param_names, {"GENERIC_TRAIN": gt, "GENERIC_TRAIN_EXT": gte})
            served = not generic or (gte if behind_grid else gt)
            if not served:
                assert got == ["!NotImplementedError"], (generic, behind_grid, gt, gte, got)
                continue
            want = G.run(through(direct[(generic, behind_grid)], False), net(), G.FULL, T.param_names, {"GENERIC_TRAIN": True, "GENERIC_TRAIN_EXT": True})
            assert got == want and got[-1].startswith("grads:"), (generic, behind_grid, gt, gte, got[-3:], want[-3:])


def test_backward_route_follows_its_forward():
    """A backward runs the dX step its forward prepared for, whatever train.FUSED_DX says by then: the fused fp16 launch and its timer
    key after a fused fp16 forward, the layered chain under the plain key after a layered one."""
    import torch
    from nefes_amd import train as T
    with G.patched():
        for at_forward, entry, key in ((True, "nefes_field_bwd_train_h3(", "t:field_bwd_train[h3]"), (False, "nefes_train_dx(", "t:field_bwd_train")):
            G.set_switches({"FUSED_DX": at_forward})
            del G.EVENTS[:]
            raw = T.field_train(G.prepare(G.network(256, 16, 1)), G.FULL, *G.rays())
            T.FUSED_DX = not at_forward
            raw.backward(torch.ones_like(raw))
            back = G.EVENTS[G.EVENTS.index(key):]
            assert any(e.startswith(entry) for e in back) and not any(e.startswith("t:field_bwd_train") for e in back[1:]), back[:4]
            assert any(e.startswith("nefes_train_dx(") for e in back) == (not at_forward)

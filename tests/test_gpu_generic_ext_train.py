"""Training the MLP behind a hash grid at any --netwidth / --netdepth: the generic field kernels' train-mode instances on a SUPPLIED
32-feature encoding (nefes_amd/csrc/field_generic.hip gen_fwd_kernel / gen_bwd_kernel<NCB, GenArgsExtTrain>,
nefes_field_{fwd,bwd}_train_generic_ext, train.field_train_generic_encoded, opt-in: ops.GENERIC_TRAIN_EXT).

Ground truth: oracle/ref_cpu.py (+ oracle/hashgrid_ref.py through the grid) in float64, the fp32 oracle next to it.  Bounds, the
project's own: raw outputs three-way e_hip <= max(1e-4, 1.5 e_ref), raw_t against float64 under 2e-5, every parameter gradient under
1e-4 of float64 on the kernels' own ReLU branches (audited as tests/test_gpu_generic_train.py audits them), d encoding and d viewdirs
by tests/generic_util.py pinned_gradients_generic, the table gradient a flat 1e-4 of float64 autograd.  Inputs: 5 rays x 33 samples,
M = 165 = 128 + 37, so that the second 128-sample train tile is part covered and the 64- and 32-sample tiles end ragged."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from oracle import hashgrid_ref as HG
from oracle import ref_cpu as O
from tests import branch as B
from tests import generic_util as G
from tests import parity_log as P
from tests import test_generic_ext_train as CPU
from tests import test_gpu_generic_ext as X
from tests import test_gpu_hashgrid_train as HT
from tests.test_gpu_generic_ext import FAR, FOCAL_AT_854, NEAR, _oracle_render, _render_kwargs
from tests.test_gpu_generic_train import _nets, _oracle_params
from tests.test_gpu_hashgrid_train import _loss

pytestmark = pytest.mark.gpu
DEV = "cuda"
N_RAYS, N_S = 5, 33
FWD_KEY, BWD_KEY = "field_fwd_train[generic,ext]", "field_bwd_train[generic,ext]"


def test_cpu_file_restates_the_ext_shapes():
    assert CPU.SHAPES == [s[:3] for s in X.SHAPES]


def _inputs(C_, fine, seed=2, N=N_RAYS, S=N_S):
    """An encoding random in +-0.4 (tests/test_gpu_generic_ext.py _inputs), unit view directions, a cotangent for raw_t."""
    g = torch.Generator().manual_seed(seed)
    enc = (torch.rand(N, S, 32, generator=g) * 2 - 1) * 0.4
    v = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    return enc, v, torch.randn(N, (9 if fine else 4) + C_, S, generator=g)


def _run(net, mode, enc, v, Gr):
    """One train-mode forward + backward of the autograd Function -> raw_t, the leaves, debug buffers, tap."""
    from nefes_amd import train as TR
    enc_h, v_h = enc.to(DEV).requires_grad_(), v.to(DEV).requires_grad_()
    sd = dict(net.named_parameters())
    TR.DEBUG = {}
    try:
        with B.tapped() as tap:
            raw_t = TR.FieldTrainGenericEncoded.apply(enc_h, v_h, net, mode, *[sd[n] for n in TR.param_names_generic(net, mode)])
            (raw_t * Gr.to(DEV)).sum().backward()
        dbg = dict(TR.DEBUG)
    finally:
        TR.DEBUG = None
    return types.SimpleNamespace(raw_t=raw_t, enc_h=enc_h, v_h=v_h, dbg=dbg, tap=dict(tap))


def _oracle(net, names, D, fine, enc, v, dt, act=None, G_up=None):
    """The oracle's field on a supplied encoding -> raw [N, S, R]; with G_up [N, R, S] also the gradients of sum(raw G_up) w.r.t. the
    parameters `names`, the encoding and the view directions."""
    N, S = enc.shape[:2]
    p = _oracle_params(net, names if G_up is not None else (), dt)
    e = enc.reshape(-1, 32).to(dt).clone().requires_grad_(G_up is not None)
    vv = v.to(dt).clone().requires_grad_(G_up is not None)
    ed = O.freq_encode(vv[:, None].expand(N, S, 3).reshape(-1, 3), 4)
    a = None if act is None else (lambda tag, pre: act(tag, pre, 0))
    raw = O.field_forward(p, torch.cat([e, ed], 1), output_transient=fine, in_xyz=32, D=D, skip=4, act=a).reshape(N, S, -1)
    if G_up is None:
        return raw.detach()
    (raw * G_up.permute(0, 2, 1).to(dt)).sum().backward()
    out = {n: p[n].grad for n in names}
    out.update({"d enc": e.grad.reshape(N, S, 32), "d viewdirs": vv.grad, "__raw__": raw.detach()})
    return out


def _check_gradients(tag, net, names, D, fine, enc, v, Gr, r, tol=1e-4):
    """raw_t against float64 on the kernels' branches (2e-5), every parameter gradient under `tol` of float64 [branch-pinned], d enc and
    d viewdirs under pinned_gradients_generic's rule, which also audits the branches.  -> the worst parameter-gradient error."""
    keep = {}

    def oracle_run(dt, act, _):
        keep[dt] = _oracle(net, names, D, fine, enc, v, dt, act=act, G_up=Gr)
        return keep[dt]

    out = G.pinned_gradients_generic(tag, {"d enc": r.enc_h.grad, "d viewdirs": r.v_h.grad}, r.tap, oracle_run)
    e_raw = B.rel(r.raw_t.permute(0, 2, 1), keep[torch.float64]["__raw__"])
    print(f"[{tag}] raw_t vs float64 on the kernels' branches: {e_raw:.2e}")
    assert e_raw < 2e-5
    sd = dict(net.named_parameters())
    worst = ("", 0.)
    for n in names:
        assert sd[n].grad is not None and sd[n].grad.shape == sd[n].shape, n
        worst = max(worst, (n, B.rel(sd[n].grad, keep[torch.float64][n])), key=lambda t: t[1])
    print(f"[{tag}] worst parameter gradient vs float64 [branch-pinned]: {worst[1]:.2e} ({worst[0]})")
    P.record(tag, "worst parameter gradient [branch-pinned]", e_hip=worst[1], e_ref=None, bound=tol)
    assert worst[1] < tol, worst
    return worst[1], out["d enc"][0]


# (W, D, C, net): STATIC + the skip layer; the same fine; the reference's default; depth 1 (layer 1 reads E and takes the density's
# rank-1 term); no skip; the 32-sample tile
CASES = [(64, 6, 16, "coarse"), (64, 6, 16, "fine"), (128, 8, 128, "fine"), (32, 1, 16, "fine"), (128, 4, 30, "coarse"),
         (320, 7, 29, "fine")]


@pytest.mark.parametrize("Wd,D,C_,typ", CASES)
def test_field_train_generic_ext_weight_grads(Wd, D, C_, typ, monkeypatch):
    from nefes_amd import lib as L
    from nefes_amd import ops
    from nefes_amd import train as TR
    monkeypatch.setattr(ops, "TIMERS", {})
    fine = typ == "fine"
    mode = L.FIELD_FULL if fine else L.FIELD_STATIC
    net = _nets(Wd, D, C_, typ, in_xyz=32)
    enc, v, Gr = _inputs(C_, fine)
    N, S, M = N_RAYS, N_S, N_RAYS * N_S
    r = _run(net, mode, enc, v, Gr)
    assert set(ops.TIMERS) - {"ray_grad_reduce"} == {FWD_KEY, BWD_KEY}, set(ops.TIMERS)
    acts, off = r.dbg["acts"], r.dbg["off"]
    tag = f"generic_ext_train[{Wd},{D},{C_},{typ}]"
    names = TR.param_names_generic(net, mode)
    assert r.raw_t.shape == (N, (9 if fine else 4) + C_, S)
    block = lambda b, n: acts[:, off[b]:off[b] + n, :].permute(0, 2, 1).reshape(-1, n)[:M].cpu()
    # ---- the E block is the supplied encoding, bit for bit, in natural order; the ext row map ----
    assert off[L.TB_E] == 0 and off[L.TB_DV] == 32 and off[L.TB_L1] == 64
    assert torch.equal(block(L.TB_E, 32), enc.reshape(M, 32))
    # ---- the saved outputs: trunk, DV, FINAL, DIR, T0..T2 with their zero padding rows, three-way ----
    skip = 4 if D > 4 else -1
    Hp = (Wd // 2 + 31) // 32 * 32
    saved = {}
    for dt in (torch.float64, torch.float32):
        p = _oracle_params(net, (), dt)
        lin = lambda name, x: torch.nn.functional.linear(x, p[name + ".weight"], p[name + ".bias"])
        e = enc.reshape(M, 32).to(dt)
        h, out = e, {}
        for l in range(1, D + 1):
            if l - 1 == skip:
                h = torch.cat([e, h], 1)
            h = torch.relu(lin(f"xyz_encoding_{l}.0", h))
            out[L.TB_L1 + l - 1] = h
        dv = O.freq_encode(v.to(dt), 4)[:, None, :].expand(N, S, 27).reshape(M, 27)
        fin = lin("xyz_encoding_final", h)
        x = torch.cat([fin, dv], 1)
        out.update({L.TB_DV: dv, L.TB_FINAL: fin, L.TB_DIR: torch.relu(lin("dir_encoding.0", x))})
        if fine:
            out[L.TB_T0] = torch.relu(lin("transient_encoding.0", x))
            out[L.TB_T1] = torch.relu(lin("transient_encoding.2", out[L.TB_T0]))
            out[L.TB_T2] = torch.relu(lin("transient_encoding.4", out[L.TB_T1]))
        saved[dt] = out
    for b, ref64 in saved[torch.float64].items():
        n, rows = ref64.shape[1], off[b + 1] - off[b]
        assert rows == (32 if b == L.TB_DV else (Hp if b >= L.TB_DIR else Wd)), (b, rows)
        blk = block(b, rows)
        B.three_way(tag, f"saved output of block {b}", blk[:, :n], saved[torch.float32][b], ref64)
        assert bool((blk[:, n:] == 0).all()), b
    for b in range(L.TB_L1 + D, L.TB_FINAL):                                # layers above the depth: empty blocks
        assert off[b + 1] == off[b]
    # ---- raw outputs three-way (the oracles on their own branches), then everything on the kernels' branches ----
    B.three_way(tag, "raw", r.raw_t.permute(0, 2, 1), _oracle(net, (), D, fine, enc, v, torch.float32),
                _oracle(net, (), D, fine, enc, v, torch.float64))
    _check_gradients(tag, net, names, D, fine, enc, v, Gr, r)


def _sentinel_launch(pk, mode, N, S, enc, v, g_raw, guard=64):
    """The two C entry points on buffers with `guard` sentinel words behind raw_t, the masks, g_xyz_enc, g_viewdirs_s, acts and dacts
    (memory of the test's own, inside its allocations) -> acts, dacts in (row, sample) order."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    from nefes_amd import train as TR
    lib = L.load()
    M, R = N * S, pk.n_raw(mode)
    rows, _ = pk.train_rows()
    tiles = (M + 127) // 128
    SENT, ISENT = 12345.5, 0x5a5a5a5a
    full = lambda n: torch.full((n + guard,), SENT, device=DEV)
    raw, g_enc, g_vs, acts, dacts = full(N * R * S), full(M * 32), full(M * 3), full(tiles * rows * 128), full(tiles * rows * 128)
    masks = torch.full((pk.mask_bytes(M) // 4 + guard,), ISENT, dtype=torch.int32, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    L.check(lib.nefes_field_fwd_train_generic_ext(pk.desc, p(pk.blob), mode, N, S, p(enc), p(v), p(raw), p(acts), p(masks), ops._stream()),
            "fwd")
    L.check(lib.nefes_field_bwd_train_generic_ext(pk.desc, p(pk.blob), mode, N, S, p(v), p(raw), p(g_raw), p(masks), p(dacts), p(g_enc),
                                                  p(g_vs), ops._stream()), "bwd")
    torch.cuda.synchronize()
    for name, t in (("raw_t", raw), ("g_xyz_enc", g_enc), ("g_viewdirs_s", g_vs), ("acts", acts), ("dacts", dacts)):
        assert bool((t[t.numel() - guard:] == SENT).all()), f"{name}: written behind its end"
        assert bool(t[:t.numel() - guard].isfinite().all()) or name in ("acts", "dacts"), name
    assert bool((masks[masks.numel() - guard:] == ISENT).all()), "masks: written behind their end"
    assert not bool((raw[:N * R * S] == SENT).any()) and not bool((g_enc[:M * 32] == SENT).any()) and not bool((g_vs[:M * 3] == SENT).any())
    view = lambda t: TR.rows_view(t[:tiles * rows * 128].view(tiles, rows, 128)).permute(1, 0, 2).reshape(rows, -1)
    return view(acts), view(dacts)


def test_padding_rows_dead_samples_and_unwritten_memory(monkeypatch):
    """(96, 5, 128, fine): W / 2 = 48 in 64 rows, the 131-row head in 160, SIG 1 of 32, TH 5 of 32; M = 165 of 256 buffer columns, so the
    launch has a 64-sample tile no sample reaches: it writes zeros and touches neither the masks nor raw_t nor the encoding's gradient."""
    from nefes_amd import lib as L
    from nefes_amd import train as TR
    Wd, D, C_ = 96, 5, 128
    net = _nets(Wd, D, C_, "fine", in_xyz=32)
    enc, v, Gr = _inputs(C_, True)
    M = N_RAYS * N_S
    r = _run(net, L.FIELD_FULL, enc, v, Gr)
    dacts, off, rows = r.dbg["dacts"], r.dbg["off"], r.dbg["rows"]
    flat = dacts.permute(1, 0, 2).reshape(rows, -1)                      # [rows, 256 buffer columns]
    assert flat.shape[1] == 256
    g_rows = slice(off[L.TB_L1], rows)
    assert bool((flat[g_rows, M:] == 0).all())                           # dead samples of a tile AND the tile no sample reaches
    assert bool(flat[g_rows, :M].isfinite().all())
    real = {L.TB_DIR: 48, L.TB_T0: 48, L.TB_T1: 48, L.TB_T2: 48, L.TB_RGB: 3 + C_, L.TB_SIG: 1, L.TB_TH: 5}
    for b, n in real.items():
        assert off[b + 1] - off[b] > n
        assert bool((flat[off[b] + n:off[b + 1]] == 0).all()), b
        assert float(flat[off[b]:off[b] + n, :M].abs().max()) > 0, b
    acts = r.dbg["acts"].permute(1, 0, 2).reshape(rows, -1)
    assert bool(acts[:off[L.TB_RGB]].isfinite().all())                   # every X operand column is written (0 * NaN would poison dW)
    assert bool((acts[:off[L.TB_RGB], 192:] == 0).all())                 # the 64-sample tile past the last sample: zeros, not a forward
    grads = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
    g_in = (r.enc_h.grad.clone(), r.v_h.grad.clone())
    # the same step on buffers that start as NaN / -1 instead of whatever torch.empty returns: bit-identical gradients
    real_torch = torch

    class Poisoned:
        def __getattr__(self, k):
            return getattr(real_torch, k)

        @staticmethod
        def empty(*a, **kw):
            t = real_torch.empty(*a, **kw)
            return t.fill_(float("nan") if t.is_floating_point() else -1)

        @staticmethod
        def empty_like(x, **kw):
            t = real_torch.empty_like(x, **kw)
            return t.fill_(float("nan") if t.is_floating_point() else -1)

    monkeypatch.setattr(TR, "torch", Poisoned())
    for p in net.parameters():
        p.grad = None
    r2 = _run(net, L.FIELD_FULL, enc, v, Gr)
    monkeypatch.undo()
    for n, p in net.named_parameters():
        if n in grads:
            assert bool(p.grad.isfinite().all()), n
            assert torch.equal(p.grad, grads[n]), n
    assert torch.equal(r2.enc_h.grad, g_in[0]) and torch.equal(r2.v_h.grad, g_in[1]) and torch.equal(r2.raw_t, r.raw_t)
    # the two C entry points between sentinels: nothing behind any buffer, the same buffers as the Function's
    pk = net.packed_generic()
    a2, d2 = _sentinel_launch(pk, L.FIELD_FULL, N_RAYS, N_S, enc.reshape(M, 32).to(DEV).contiguous(), v.to(DEV).contiguous(),
                              Gr.to(DEV).contiguous())
    assert torch.equal(a2[:off[L.TB_RGB]], acts[:off[L.TB_RGB]]) and torch.equal(d2[g_rows], flat[g_rows])


@pytest.mark.parametrize("Wd,D,C_,typ", [(64, 6, 16, "fine"), (96, 5, 128, "coarse")])
def test_device_repack_of_an_ext_description(Wd, D, C_, typ, monkeypatch):
    """nefes_generic_pack_device on a NEFES_XYZ_EXTERNAL32 description: same blob pointer, generation + 1, no host packer, and the bytes
    of a fresh host pack of the same values."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    net = _nets(Wd, D, C_, typ, in_xyz=32)
    pk = net.packed_generic()
    assert pk.xyz_encoding == L.XYZ_EXTERNAL32
    ptr, gen0 = pk.blob.data_ptr(), pk.generation
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for n, p in net.named_parameters():
            p.add_(torch.randn(p.shape, generator=g).to(DEV) * 0.01)
    host_calls = []
    lib = ops.L.load()

    class Counting:
        def __getattr__(self, k):
            if k == "nefes_generic_pack":
                host_calls.append(k)
            return getattr(lib, k)

    monkeypatch.setattr(ops.L, "load", lambda: Counting())
    pk2 = net.packed_generic()
    assert pk2 is pk and pk.blob.data_ptr() == ptr and pk.generation == gen0 + 1 and not host_calls
    monkeypatch.undo()
    net._pk_gen = None
    fresh = net.packed_generic()                                         # the host packer on the same values
    assert fresh is not pk and fresh.blob.numel() == pk.blob.numel() and torch.equal(fresh.blob, pk.blob)


def test_against_the_tuned_train_path_on_the_same_weights():
    """A (256, 8, C = 16) fine network: FieldTrainEncoded on packed() and the generic Function on packed_generic(), each on its own
    forward's branches: every parameter gradient and d enc under 1e-4 of float64.  The ratio of the two errors is recorded, not bounded."""
    from nefes_amd import lib as L
    from nefes_amd import train as TR
    Wd, D, C_ = 256, 8, 16
    net = _nets(Wd, D, C_, "fine", in_xyz=32)
    assert not net.uses_generic()
    enc, v, Gr = _inputs(C_, True, seed=4)
    names = TR.param_names_generic(net, L.FIELD_FULL)
    assert names == TR.param_names(net, L.FIELD_FULL)
    sd = dict(net.named_parameters())
    errs = {}
    for which, fn in (("generic", TR.FieldTrainGenericEncoded), ("tuned", TR.FieldTrainEncoded)):
        for p in net.parameters():
            p.grad = None
        enc_h, v_h = enc.to(DEV).requires_grad_(), v.to(DEV).requires_grad_()
        with B.tapped() as tap:
            raw_t = fn.apply(enc_h, v_h, net, L.FIELD_FULL, *[sd[n] for n in names])
            (raw_t * Gr.to(DEV)).sum().backward()
        pin = G.GenericPinned(tap) if which == "generic" else B.Pinned(tap, Wd)
        g64 = _oracle(net, names, D, True, enc, v, torch.float64, act=pin.act(True), G_up=Gr)
        flips, units, worst_pre = pin.summary()
        assert worst_pre < 2e-5 and flips <= max(8, units // 100000), (which, flips, units, worst_pre)
        errs[which] = {"weights": max(B.rel(sd[n].grad, g64[n]) for n in names), "d enc": B.rel(enc_h.grad, g64["d enc"])}
    print(f"[generic_ext_train_vs_tuned] worst gradient errors vs float64: {errs}")
    for k in errs["generic"]:
        P.record("generic_ext_train_vs_tuned[256,8,16]", f"{k}: generic error / tuned error [branch-pinned]", e_hip=errs["generic"][k],
                 e_ref=errs["tuned"][k], ratio=errs["generic"][k] / max(errs["tuned"][k], 1e-30), bound=1e-4)
        assert errs["generic"][k] < 1e-4 and errs["tuned"][k] < 1e-4, (k, errs)


# ---- through render() --------------------------------------------------------------------------------------------------------------
def _pair(Wd, D, C_, trainable_table):
    from nefes_amd import ops
    coarse, fine = _nets(Wd, D, C_, "coarse", in_xyz=32), _nets(Wd, D, C_, "fine", in_xyz=32)
    grid = ops.HashGrid(X.BOUND, table=HG.make_table(0) * X.TABLE_GAIN)
    grid.table.requires_grad_(trainable_table)
    return coarse, fine, grid


@pytest.mark.parametrize("Wd,D,C_,H,W,case,far", [(64, 6, 16, 12, 16, "weights", 1.), (64, 6, 16, 12, 16, "joint", 1.),
                                                  (128, 8, 128, 6, 8, "joint", FAR)])
def test_render_trains_the_weights_behind_a_grid(Wd, D, C_, H, W, case, far, monkeypatch):
    """render() of a coarse / fine pair sharing one grid, 16 + 16 samples, bound 25, test_time False, one loss.backward():
    `weights` = the MLPs alone, `joint` = MLPs + table + pose.  Loss within 1e-5 of the fp32 oracle's; weight gradients under 1e-4 of the
    float64 oracle on the kernels' branches and depths, the table gradient a flat 1e-4, the pose gradient three-way.

    The far plane.  Nothing in front of the grid is float64 in the kernels or in the fp32 oracle, so both sit about 2e-5 from the
    float64 oracle on every weight (fp32 cell arithmetic of a grid of bound 25), and a gradient that is a cancelling sum multiplies
    that.  The coarse static_sigma gradients are such a sum, of d loss / d sigma over all samples.  With the far plane at 6, the other
    hash-grid tests' choice, the untrained (64, 6) pair renders opaque rays of nearly constant colour: the terms have both signs and
    sum |g| / |sum g| is 8.6; the fp32 oracle on float64's branches and depths is then 1.9e-4 from float64 on static_sigma.0.bias itself
    (CPU), and the kernels measured 1.82e-4 next to it -- no room under a flat 1e-4 for either.  With the far plane at 1 the rays stay
    translucent, the ratio is 1.75 and that fp32 oracle is 1.3e-5 away (every other weight under 7e-6): the (64, 6, 16) cases use it.
    At (128, 8, 128) the same fp32 oracle is 2.7e-5 away at far 6, which stays.  Each far plane was chosen from the fp32 oracle's own
    distance alone; the weight assertion is the last one, so that every other check of a case runs first, and e_ref is printed next
    to e_hip."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    from nefes_amd import train as TR
    from nefes_amd.render import render
    monkeypatch.setattr(ops, "GENERIC_TRAIN_EXT", True)
    NC = NI = 16
    joint = case == "joint"
    coarse, fine, grid = _pair(Wd, D, C_, joint)
    focal = FOCAL_AT_854 * W / 854.
    pose = O.se3_exp_pose(*X.POSE)
    c2w = pose.to(DEV).requires_grad_(joint)
    ops.TIMERS = timers = {}
    try:
        with B.tapped() as tap:
            rgb, disp, acc, ex = render(H, W, focal, c2w=c2w, near=NEAR, far=far, **_render_kwargs(coarse, fine, grid, NC, NI, False))
            loss = _loss(rgb, ex)
            loss.backward()
    finally:
        ops.TIMERS = None
    assert {FWD_KEY, BWD_KEY, "hashgrid_fwd"} <= set(timers), sorted(timers)
    assert ("hashgrid_bwd_table" in timers) == joint
    assert not [k for k in timers if "h3" in k or k.startswith(("field_fwd[", "field_bwd["))], sorted(timers)
    assert len(tap["masks_generic"]) == 2
    tag = f"generic_ext_train_render[{Wd},{D},{C_},{case}]"
    names_c, names_f = TR.param_names_generic(coarse, L.FIELD_STATIC), TR.param_names_generic(fine, L.FIELD_FULL)
    pin_c, pin_f = G.GenericPinned(tap, index=0), G.GenericPinned(tap)

    def oracle_run(dt, record, want_table):
        pc, pf = _oracle_params(coarse, names_c, dt), _oracle_params(fine, names_f, dt)
        tab = grid.table.detach().cpu().to(dt).requires_grad_(want_table)
        p_ = pose.to(dt).clone().requires_grad_(joint)
        acts = (pin_c.act(record), pin_f.act(record), pin_f.z_fine)
        with G.oracle_depth(D):
            if far == FAR:                                                  # tests/test_gpu_hashgrid_c128.py's composition: any frame, far 6
                _, l_ = _oracle_render(H, W, NC, NI, p_, pc, pf, tab, dt, False, *acts)
            else:                                                           # tests/test_gpu_hashgrid_train.py's: this frame, any far plane
                assert (H, W, NC, NI) == (HT.H, HT.W, HT.NC, HT.NI)
                _, l_ = HT._oracle_train_render(p_, pc, pf, tab, dt, False, far, *acts)
        l_.backward()
        return float(l_.detach()), pc, pf, tab.grad, p_.grad

    loss64, pc, pf, g_tab, g_pose64 = oracle_run(torch.float64, True, joint)
    loss32, pc32, pf32, _, g_pose32 = oracle_run(torch.float32, False, False)
    for name, pin in (("coarse", pin_c), ("fine", pin_f)):
        flips, units, worst = pin.summary()
        P.record(tag, f"{name}: relu branch flips vs float64", flips=flips, units=units, worst_preact_rel=worst)
        assert worst < B.AUDIT_CLASSES["same_inputs"] and flips <= max(8, units // 100000), (name, flips, units, worst)
    print(f"[{tag}] loss {float(loss.detach())}, fp32 oracle {loss32}, float64 oracle {loss64}")
    assert abs(float(loss.detach()) - loss32) < 1e-5 * abs(loss32)
    errs = []
    for net, p64, p32, names, which in ((coarse, pc, pc32, names_c, "coarse"), (fine, pf, pf32, names_f, "fine")):
        sd = dict(net.named_parameters())
        for n in names:
            assert sd[n].grad is not None, (which, n)
            if float(p64[n].grad.abs().max()) == 0.:                        # transient_beta: beta is not in this loss
                assert float(sd[n].grad.abs().max()) == 0., (which, n)
                continue
            errs.append((B.rel(sd[n].grad, p64[n].grad), B.rel(p32[n].grad, p64[n].grad), f"{which} {n}"))
    errs.sort(reverse=True)
    worst = errs[0]
    print(f"[{tag}] worst weight gradients vs float64 [branch-pinned] (e_hip, fp32 oracle's e_ref, name): "
          + ", ".join(f"({a:.2e}, {b:.2e}, {n})" for a, b, n in errs[:4]))
    P.record(tag, "worst weight gradient [branch-pinned]", e_hip=worst[0], e_ref=worst[1], bound=1e-4)
    if joint:
        assert grid.table.grad is not None and float(grid.table.grad.abs().max()) > 0
        e = B.rel(grid.table.grad, g_tab)
        print(f"[{tag}] d table vs float64 autograd [branch-pinned]: {e:.2e}")
        P.record(tag, "d table [branch-pinned, flat bound]", e_hip=e, e_ref=None, bound=1e-4)
        assert e < 1e-4, e
        assert c2w.grad is not None and float(c2w.grad.abs().max()) > 0
        B.three_way(tag, "d c2w [branch-pinned]", c2w.grad, g_pose32, g_pose64)
    else:
        assert grid.table.grad is None
    assert worst[0] < 1e-4, worst


def test_the_switch(monkeypatch):
    """Off (the default): the refusal tests/test_gpu_generic_ext.py pins, whatever ops.GENERIC_TRAIN says.  On alone: it trains."""
    from nefes_amd import ops
    from nefes_amd.render import render
    assert ops.GENERIC_TRAIN_EXT is False and ops.GENERIC_TRAIN is False
    coarse, fine, grid = _pair(64, 6, 16, False)
    coarse.requires_grad_(False)
    run = lambda: render(2, 3, FOCAL_AT_854 * 3 / 854., c2w=O.se3_exp_pose(*X.POSE).to(DEV), near=NEAR, far=FAR,
                         **_render_kwargs(coarse, fine, grid, 16, 16, False))
    for generic_train in (False, True):
        monkeypatch.setattr(ops, "GENERIC_TRAIN", generic_train)
        with pytest.raises(NotImplementedError, match="train mode.*D=6.*W=64.*in_channels_xyz=32.*NEFES_GENERIC_TRAIN_EXT"):
            run()
    monkeypatch.setattr(ops, "GENERIC_TRAIN", False)
    monkeypatch.setattr(ops, "GENERIC_TRAIN_EXT", True)
    ops.TIMERS = timers = {}
    try:
        rgb, _, _, ex = run()
        _loss(rgb, ex).backward()
    finally:
        ops.TIMERS = None
    assert {FWD_KEY, BWD_KEY} <= set(timers) and "field_fwd[static,generic,ext]" in timers, sorted(timers)      # (the frozen coarse network)
    grads = [p.grad for n, p in fine.named_parameters() if not n.startswith(("fusion_net", "exposure_embedding"))]
    assert all(g_ is not None and torch.isfinite(g_).all() for g_ in grads) and max(float(g_.abs().max()) for g_ in grads) > 0


def test_training_moves_the_loss(monkeypatch):
    """Six Adam steps on the weights and the table of a (64, 6, 16) pair: the last loss is below the first, every step after the first
    re-packs on the device (no host packer call), and a backward held across a step raises the generation error."""
    from nefes_amd import ops
    from nefes_amd.render import render
    monkeypatch.setattr(ops, "GENERIC_TRAIN_EXT", True)
    H, W, NC, NI, C_ = 8, 8, 16, 16, 16
    coarse, fine, grid = _pair(64, 6, C_, True)
    kw = _render_kwargs(coarse, fine, grid, NC, NI, False)
    focal = FOCAL_AT_854 * W / 854.
    pose = O.se3_exp_pose(*X.POSE).to(DEV)
    gen = torch.Generator().manual_seed(1)
    t_rgb, t_feat = torch.rand(H * W, 3, generator=gen).to(DEV), torch.randn(H * W, C_, generator=gen).to(DEV)
    loss_of = lambda rgb, ex: ((rgb - t_rgb) ** 2).mean() + ((ex["feat_map"] - t_feat) ** 2).mean() + ((ex["rgb0"] - t_rgb) ** 2).mean()
    prm = [p for net in (coarse, fine) for n, p in net.named_parameters() if not n.startswith(("fusion_net", "exposure_embedding"))]
    opt = torch.optim.Adam([{"params": prm, "lr": 5e-4}, {"params": grid.parameters(), "lr": 1e-2}])
    pk_c, pk_f = coarse.packed_generic(), fine.packed_generic()         # packed on the host once, here
    gen0 = (pk_c.generation, pk_f.generation)
    host_calls = []
    lib = ops.L.load()

    class Counting:
        def __getattr__(self, k):
            if k == "nefes_generic_pack":
                host_calls.append(k)
            return getattr(lib, k)

    monkeypatch.setattr(ops.L, "load", lambda: Counting())
    losses = []
    for _ in range(6):
        rgb, _, _, ex = render(H, W, focal, c2w=pose, near=NEAR, far=FAR, **kw)
        loss = loss_of(rgb, ex)
        opt.zero_grad()
        loss.backward()
        assert torch.isfinite(grid.table.grad).all() and float(grid.table.grad.abs().max()) > 0
        opt.step()
        losses.append(float(loss.detach()))
    print(f"[generic_ext_train_steps] losses {losses}")
    assert not host_calls
    assert coarse.packed_generic() is pk_c and fine.packed_generic() is pk_f
    assert (pk_c.generation, pk_f.generation) == (gen0[0] + 6, gen0[1] + 6)      # five renders after a step, and the two calls above
    assert losses[-1] < losses[0], losses
    rgb, _, _, ex = render(H, W, focal, c2w=pose, near=NEAR, far=FAR, **kw)
    loss = loss_of(rgb, ex)
    opt.zero_grad()
    with torch.no_grad():
        for p in prm:
            p.add_(1e-3)
    coarse.packed_generic(), fine.packed_generic()
    with pytest.raises(RuntimeError, match="re-packed"):
        loss.backward()


@pytest.mark.parametrize("tag", CPU.GOLDEN_TAGS)
def test_generic_ext_train_vs_reference_golden(golden, tag):
    """One forward + backward on the inputs of tests/golden/generic_ext_train.npz, tensors the reference itself produced
    (tools/make_golden_generic_ext_train.py): raw outputs three-way with the reference in the fp32 seat; gradients under the rules of
    test_generic_train_vs_reference_golden -- each within 1e-3 of the reference's with cosine > 0.9995, the worst within
    P.bound(e_ref, tol=1e-3) of the float64 oracle on its own branches.  The reference's d x covers d enc and, through the direction
    embedding's chain, the reduced d viewdirs."""
    from nefes_amd import lib as L
    from nefes_amd import train as TR
    g = golden("generic_ext_train")
    net, (Wd, D, C_, fine, N, S), enc, v, G_up, ref = CPU.golden_case(g, tag, device=DEV)
    mode = L.FIELD_FULL if fine else L.FIELD_STATIC
    names = TR.param_names_generic(net, mode)
    r = _run(net, mode, enc, v, G_up)
    raw64, g64, ge64, gv64 = CPU.oracle_on_case(net, D, fine, enc, v, G_up, torch.float64)
    t = f"generic_ext_train_golden[{tag}]"
    B.three_way(t, "raw vs the reference", r.raw_t.permute(0, 2, 1).reshape(N * S, -1), torch.from_numpy(ref["raw"]), raw64)
    ref_ge, ref_gv = CPU.reference_input_grads(ref, v, N, S)
    sd = dict(net.named_parameters())
    triples = [(n, sd[n].grad, torch.from_numpy(ref["grad." + n]), g64[n]) for n in names]
    triples += [("d enc", r.enc_h.grad.reshape(N * S, 32), ref_ge, ge64), ("d viewdirs", r.v_h.grad, ref_gv, gv64)]
    worst = {"e_hip": 0., "e_ref": 0., "direct": 0.}
    for name, got, b, t64 in triples:
        assert got is not None and tuple(got.shape) == tuple(b.shape), name
        a, b, t64 = got.detach().cpu().double().reshape(-1), b.double().reshape(-1), t64.double().reshape(-1)
        assert float(b.abs().max()) > 0, name
        direct = float((a - b).abs().max() / b.abs().max())
        cos = float(torch.dot(a, b) / (a.norm() * b.norm()).clamp_min(1e-30))
        sc = t64.abs().max()
        worst = {"e_hip": max(worst["e_hip"], float((a - t64).abs().max() / sc)), "e_ref": max(worst["e_ref"], float((b - t64).abs().max() / sc)),
                 "direct": max(worst["direct"], direct)}
        assert direct < 1e-3 and cos > 0.9995, (name, direct, cos)
    bound = P.bound(worst["e_ref"], tol=1e-3)
    print(f"[{t}] worst gradient: {worst}, bound {bound}, {len(triples)} gradients compared")
    P.record(t, "worst gradient, UNPINNED: hip / reference fp32 vs float64 on its own branches", bound=bound, **worst)
    assert worst["e_hip"] <= bound, worst
    assert len(triples) == 2 * (D + (10 if fine else 4)) + 2

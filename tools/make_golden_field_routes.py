#!/usr/bin/env python3
"""Fixture of the field kernels' ROUTING: which C entry points and timer keys serve a given pack, mode, direction, input kind and
sample count under given switches -- tests/golden/field_routes.json, replayed by tests/test_field_routes.py.

Runs on the CPU without the library: L.load() hands out an object whose every attribute records its own name and returns 0,
ops._chk / ops._stream return None, ops._timed records its key, packs are SimpleNamespace objects and tensors live on the meta
device.  Only names that callers outside nefes_amd/ops.py use are called, so the same generator replays on any later revision.

Per case the outcome is the sequence of entry points ("c:") and timer keys ("t:") in launch order, a predicate's value ("="), and
the class name of the exception that ended it ("!").

Usage:  python tools/make_golden_field_routes.py            (writes the fixture from the tree it is run in)
"""
import contextlib
import hashlib
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from nefes_amd import lib as L          # noqa: E402
from nefes_amd import ops               # noqa: E402
from nefes_amd import train as T        # noqa: E402
from nefes_amd import field as F        # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "field_routes.json")

SHAPES = [(256, 16), (128, 128), (256, 128), (128, 16), (256, 200), (64, 16)]
SMALL, BIG = (4, 64), (1 << 21, 1 << 10)          # M = 256, and M = 2^31: at (above) the fp16 kernels' sample bound
SPLITS = [(s, x) for s in ("h3", "x6", "f32") for x in (True, False)]
# switch sets beyond SPLIT x USE_X6, on the packs of EXTRA_PACKS only: an invalid SPLIT, and the fused paths switched off
EXTRA = [{"SPLIT": "bogus", "USE_X6": True}, {"SPLIT": "bogus", "USE_X6": False},
         {"SPLIT": "h3", "USE_X6": True, "FUSED_COARSE": False}, {"SPLIT": "h3", "USE_X6": True, "FUSED_HASHGRID": False}]
SWITCH_NAMES = ("SPLIT", "USE_X6", "FOLD_FINAL", "FIELD_GENERIC", "FUSED_HASHGRID", "FUSED_COARSE", "REPACK_H3", "FACTORED_HEAD")

EVENTS = []


class _Lib:
    def __getattr__(self, name):
        def fn(*args):
            EVENTS.append("c:" + name)
            return 0
        return fn


class _Timed:
    def __init__(self, name):
        EVENTS.append("t:" + name)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


@contextlib.contextmanager
def patched():
    """The replacements of the module docstring, undone on exit (the test suite shares the process)."""
    saved = (L.load, ops._chk, ops._stream, ops._timed, {k: getattr(ops, k) for k in SWITCH_NAMES})
    lib = _Lib()
    L.load, ops._chk, ops._stream, ops._timed = (lambda: lib), (lambda *a, **k: None), (lambda: None), _Timed
    try:
        yield
    finally:
        L.load, ops._chk, ops._stream, ops._timed = saved[:4]
        for k, v in saved[4].items():
            setattr(ops, k, v)


def set_switches(sw):
    defaults = {"SPLIT": "h3", "USE_X6": True, "FOLD_FINAL": True, "FIELD_GENERIC": False, "FUSED_HASHGRID": True, "FUSED_COARSE": True,
                "REPACK_H3": True, "FACTORED_HEAD": True}
    for k in SWITCH_NAMES:
        setattr(ops, k, sw.get(k, defaults[k]))


def switch_id(sw):
    return ",".join(f"{k}={sw[k]}" for k in sorted(sw))


# ------------------------------------------------------------------------------------------------------------------------------
# packs
# ------------------------------------------------------------------------------------------------------------------------------
def _check_generation(gen):
    if gen != 0:
        raise RuntimeError("re-packed")


def tuned_pack(width, feat_dim, xyz_encoding, has_transient, h3_valid, fold):
    pk = types.SimpleNamespace(width=width, feat_dim=feat_dim, xyz_encoding=xyz_encoding, has_transient=has_transient, h3_valid=h3_valid,
                               fold=fold, generic=False, desc=None, blob=torch.empty(16, dtype=torch.uint8, device="meta"), generation=0,
                               mask_bytes=lambda M: 4 * ((M + 127) // 128) * 8, check_generation=_check_generation)
    pk.n_raw = types.MethodType(ops.PackedField.n_raw, pk)
    return pk


def generic_pack(width, feat_dim, has_transient):
    pk = types.SimpleNamespace(width=width, depth=8, skip=4, feat_dim=feat_dim, xyz_encoding=L.XYZ_FREQ10, has_transient=has_transient,
                               h3_valid=False, fold=False, generic=True, desc=None, blob=torch.empty(16, dtype=torch.uint8, device="meta"),
                               generation=0, mask_bytes=lambda M: 4 * ((M + 127) // 128) * 8, check_generation=_check_generation)
    pk.n_raw = types.MethodType(ops.PackedGeneric.n_raw, pk)
    return pk


def packs():
    """[(pack id, kind, constructor arguments)]"""
    out = []
    for (w, c) in SHAPES:
        for enc in (L.XYZ_FREQ10, L.XYZ_EXTERNAL32):
            for tr in (True, False):
                for valid in (True, False):
                    for fold in (False, True):
                        out.append((f"tuned,W={w},C={c},enc={enc},transient={int(tr)},h3_valid={int(valid)},fold={int(fold)}", "tuned",
                                    (w, c, enc, tr, valid, fold)))
        for tr in (True, False):
            out.append((f"generic,W={w},C={c},transient={int(tr)}", "generic", (w, c, tr)))
    return out


def switch_sets(pack_id):
    sets = [{"SPLIT": s, "USE_X6": x} for s, x in SPLITS]
    if pack_id.endswith("h3_valid=1,fold=0") or pack_id.startswith("generic"):
        sets += EXTRA
    return sets


# ------------------------------------------------------------------------------------------------------------------------------
# calls
# ------------------------------------------------------------------------------------------------------------------------------
def t(*shape, grad=False, dtype=torch.float32):
    return torch.empty(*shape, device="meta", dtype=dtype, requires_grad=grad)


def hash_grid():
    g = object.__new__(ops.HashGrid)
    g.desc = types.SimpleNamespace(n_levels=16, n_features=2)
    g.n_out = 32
    g.table = t(1024, 2)
    return g


def _back(out, *more):
    outs = [o for o in (out,) + more if o is not None and o.requires_grad]
    torch.autograd.backward(outs, [torch.empty_like(o) for o in outs])


def _mode_name(mode):
    return ("sigma", "static", "full")[mode]


def tuned_calls():
    """[(call id, function of the pack, under the first switch set only)] -- the same list for every tuned pack."""
    calls = []
    grid = hash_grid()

    def add(name, fn, small_only=False, once=False):
        """small_only: not at the sample bound (a duplicate of a call that is); once: under the first switch set only (no routing)."""
        if not (small_only and name.startswith("big")):
            calls.append((name, fn, once))

    for tag, (N, S) in (("small", SMALL), ("big", BIG)):
        M = N * S
        rays = lambda g=False, N=N, S=S: (t(N, 3, grad=g), t(N, 3, grad=g), t(N, 3, grad=g), t(N, S))
        for mode in (L.FIELD_SIGMA, L.FIELD_STATIC, L.FIELD_FULL):
            m = _mode_name(mode)
            dup = mode == L.FIELD_SIGMA          # (the sigma-only pass refuses its backward after the same forward)
            add(f"{tag},{m},FieldFromRays", lambda pk, mode=mode, rays=rays: ops.FieldFromRays.apply(*rays(), pk, mode))
            add(f"{tag},{m},field_from_rays", lambda pk, mode=mode, rays=rays: ops.field_from_rays(*rays(), pk, mode), True)
            add(f"{tag},{m},FieldFromPoints", lambda pk, mode=mode, N=N, S=S: ops.FieldFromPoints.apply(t(N, S, 3), t(N, 3), pk, mode))
            add(f"{tag},{m},FieldFromPoints,no viewdirs", lambda pk, mode=mode, N=N, S=S: ops.FieldFromPoints.apply(t(N, S, 3), None, pk, mode), True)
            add(f"{tag},{m},field_from_points", lambda pk, mode=mode, N=N, S=S: ops.field_from_points(t(N, S, 3), t(N, 3), pk, mode), True)
            add(f"{tag},{m},FieldFromEncoding", lambda pk, mode=mode, N=N, S=S: ops.FieldFromEncoding.apply(t(N, S, 32), t(N, 3), pk, mode))
            add(f"{tag},{m},FieldFromRaysHashGrid", lambda pk, mode=mode, rays=rays: ops.FieldFromRaysHashGrid.apply(*rays(), pk, mode, grid))
            add(f"{tag},{m},field_fwd", lambda pk, mode=mode, N=N, S=S: ops.field_fwd(pk, mode, N, S, rays_o=t(N, 3), rays_d=t(N, 3), z=t(N, S),
                                                                                  viewdirs=t(N, 3), want_masks=True))
            add(f"{tag},{m},field_fwd,enc", lambda pk, mode=mode, N=N, S=S, M=M: ops.field_fwd(pk, mode, N, S, xyz_enc=t(M, 32), viewdirs=t(N, 3)), True)
            add(f"{tag},{m},field_fwd_x6", lambda pk, mode=mode, N=N, S=S: ops.field_fwd_x6(pk, mode, N, S, t(N, 3), t(N, 3), t(N, S),
                                                                                        viewdirs=t(N, 3), want_masks=True))
            add(f"{tag},{m},field_fwd_x6,pts", lambda pk, mode=mode, N=N, S=S, M=M: ops.field_fwd_x6(pk, mode, N, S, pts=t(M, 3), viewdirs=t(N, 3)), True)
            add(f"{tag},{m},field_fwd_x6,enc", lambda pk, mode=mode, N=N, S=S, M=M: ops.field_fwd_x6(pk, mode, N, S, xyz_enc=t(M, 32), viewdirs=t(N, 3)), True)
            # backward through .apply (the sigma-only pass refuses)
            add(f"{tag},{m},FieldFromRays,backward", lambda pk, mode=mode, rays=rays: _back(ops.FieldFromRays.apply(*rays(True), pk, mode)), dup)
            add(f"{tag},{m},field_from_rays,backward", lambda pk, mode=mode, rays=rays: _back(ops.field_from_rays(*rays(True), pk, mode)), True)
            add(f"{tag},{m},FieldFromPoints,backward",
                lambda pk, mode=mode, N=N, S=S: _back(ops.FieldFromPoints.apply(t(N, S, 3, grad=True), t(N, 3, grad=True), pk, mode)), dup)
            add(f"{tag},{m},field_from_points,backward",
                lambda pk, mode=mode, N=N, S=S: _back(ops.field_from_points(t(N, S, 3, grad=True), t(N, 3, grad=True), pk, mode)), True)
            add(f"{tag},{m},FieldFromEncoding,backward",
                lambda pk, mode=mode, N=N, S=S: _back(ops.FieldFromEncoding.apply(t(N, S, 32, grad=True), t(N, 3, grad=True), pk, mode)), dup)
            add(f"{tag},{m},FieldFromRaysHashGrid,backward",
                lambda pk, mode=mode, rays=rays: _back(ops.FieldFromRaysHashGrid.apply(*rays(True), pk, mode, grid)), dup)
            if mode != L.FIELD_SIGMA:
                add(f"{tag},{m},field_bwd", lambda pk, mode=mode, N=N, S=S: ops.field_bwd(
                    pk, N, S, t(N, pk.n_raw(mode), S), t(N, pk.n_raw(mode), S), t(8, dtype=torch.int32), rays_o=t(N, 3), rays_d=t(N, 3),
                    z=t(N, S), viewdirs=t(N, 3), mode=mode))
                add(f"{tag},{m},field_bwd,pts", lambda pk, mode=mode, N=N, S=S, M=M: ops.field_bwd(
                    pk, N, S, t(N, pk.n_raw(mode), S), t(N, pk.n_raw(mode), S), t(8, dtype=torch.int32), pts=t(M, 3), viewdirs=t(N, 3), mode=mode), True)
        add(f"{tag},full,field_bwd,default mode", lambda pk, N=N, S=S: ops.field_bwd(
            pk, N, S, t(N, pk.n_raw(2), S), t(N, pk.n_raw(2), S), t(8, dtype=torch.int32), viewdirs=t(N, 3)))
        add(f"{tag},field_sigma_row", lambda pk, N=N, S=S: ops.field_sigma_row(pk, t(N, 3), t(N, 3), t(S)))
        add(f"{tag},field_sigma_row,grid", lambda pk, N=N, S=S: ops.field_sigma_row(pk, t(N, 3), t(N, 3), t(S), grid))
        # the factored head (pk stands for the pack without its feature rows)
        fh = lambda pk, C=128: (t(C, pk.width // 2), t(pk.width // 2, C), t(C))
        add(f"{tag},FieldFromRaysFH", lambda pk, rays=rays: ops.FieldFromRaysFH.apply(*rays(), pk), once=True)
        add(f"{tag},FieldFromRaysFH,backward", lambda pk, rays=rays: _back(ops.FieldFromRaysFH.apply(*rays(True), pk)), once=True)
        add(f"{tag},RenderFineFH", lambda pk, rays=rays: ops.RenderFineFH.apply(*rays(), pk, *fh(pk), L.COMP_TRANSIENT, 0.1), once=True)
        add(f"{tag},RenderFineFH,backward", lambda pk, rays=rays: _back(*ops.RenderFineFH.apply(*rays(True), pk, *fh(pk), L.COMP_TRANSIENT, 0.1)[:2]), True, True)
        add(f"{tag},RenderFineFH,gmap,backward",
            lambda pk, rays=rays: _back(*ops.RenderFineFH.apply(*rays(True), pk, *fh(pk), L.COMP_TRANSIENT, 0.1, True)[:2]), once=True)
    calls += predicate_calls(grid)
    return calls


def predicate_calls(grid):
    calls = []
    add = lambda name, fn: calls.append((name, fn, False))
    add("static_h3", ops.static_h3)
    add("canonical_shape", ops.canonical_shape)
    add("h3_shape", ops.h3_shape)
    add("head_class", lambda pk: ops.head_class(pk.feat_dim))
    for mode in (L.FIELD_SIGMA, L.FIELD_STATIC, L.FIELD_FULL):
        add(f"x6_supported,{_mode_name(mode)}", lambda pk, mode=mode: ops.x6_supported(pk, mode))
    add("require_instance", lambda pk: ops.require_instance(pk, "a test"))
    add("hashgrid_fused_ok", lambda pk: ops.hashgrid_fused_ok(pk, grid))
    add("hashgrid_fused_ok,no grid", lambda pk: ops.hashgrid_fused_ok(pk, None))
    for Nc, Ni, N in ((64, 64, 4), (128, 128, 4), (256, 256, 4), (256, 257, 4), (96, 64, 4), (64, 0, 4), (64, 64, 1 << 25)):
        add(f"fused_coarse_pass_ok,{Nc},{Ni},{N}", lambda pk, a=(Nc, Ni, N): ops.fused_coarse_pass_ok(pk, *a))
        add(f"fused_coarse_pass_ok,{Nc},{Ni},{N},grid", lambda pk, a=(Nc, Ni, N): ops.fused_coarse_pass_ok(pk, *a, grid))
    add("train.fp16_pipe", T.fp16_pipe)
    add("train.ext_pipe", T.ext_pipe)
    return calls


def generic_calls():
    calls = []
    grid = hash_grid()
    add = lambda name, fn: calls.append((name, fn, False))
    for tag, (N, S) in (("small", SMALL), ("big", BIG)):
        M = N * S
        rays = lambda g=False, N=N, S=S: (t(N, 3, grad=g), t(N, 3, grad=g), t(N, 3, grad=g), t(N, S))
        for mode in (L.FIELD_SIGMA, L.FIELD_STATIC, L.FIELD_FULL):
            m = _mode_name(mode)
            add(f"{tag},{m},field_from_rays", lambda pk, mode=mode, rays=rays: ops.field_from_rays(*rays(), pk, mode))
            add(f"{tag},{m},field_from_points", lambda pk, mode=mode, N=N, S=S: ops.field_from_points(t(N, S, 3), t(N, 3), pk, mode))
            add(f"{tag},{m},field_from_points,no viewdirs", lambda pk, mode=mode, N=N, S=S: ops.field_from_points(t(N, S, 3), None, pk, mode))
            add(f"{tag},{m},field_from_rays,backward", lambda pk, mode=mode, rays=rays: _back(ops.field_from_rays(*rays(True), pk, mode)))
            add(f"{tag},{m},field_from_points,backward",
                lambda pk, mode=mode, N=N, S=S: _back(ops.field_from_points(t(N, S, 3, grad=True), t(N, 3, grad=True), pk, mode)))
            add(f"{tag},{m},field_fwd_generic", lambda pk, mode=mode, N=N, S=S: ops.field_fwd_generic(
                pk, mode, N, S, rays_o=t(N, 3), rays_d=t(N, 3), z=t(N, S), viewdirs=t(N, 3), want_masks=True))
            add(f"{tag},{m},field_fwd_generic,pts", lambda pk, mode=mode, N=N, S=S, M=M: ops.field_fwd_generic(pk, mode, N, S, pts=t(M, 3), viewdirs=t(N, 3)))
            add(f"{tag},{m},field_bwd_generic", lambda pk, mode=mode, N=N, S=S: ops.field_bwd_generic(
                pk, mode, N, S, t(N, pk.n_raw(mode), S), t(N, pk.n_raw(mode), S), t(8, dtype=torch.int32), rays_o=t(N, 3), rays_d=t(N, 3),
                z=t(N, S), viewdirs=t(N, 3)))
    add("is_generic", ops.is_generic)
    add("canonical_shape", ops.canonical_shape)
    add("h3_shape", ops.h3_shape)
    add("hashgrid_fused_ok", lambda pk: ops.hashgrid_fused_ok(pk, grid))
    add("fused_coarse_pass_ok", lambda pk: ops.fused_coarse_pass_ok(pk, 64, 64, 4))
    add("fused_coarse_pass_ok,grid", lambda pk: ops.fused_coarse_pass_ok(pk, 64, 64, 4, grid))
    return calls


def outcome(fn, *args):
    del EVENTS[:]
    try:
        r = fn(*args)
        if r is None or isinstance(r, (bool, int)):
            EVENTS.append(f"={r}")
    except Exception as e:       # noqa: BLE001  (the class name is the record)
        EVENTS.append("!" + type(e).__name__)
    return " ".join(EVENTS)


# ------------------------------------------------------------------------------------------------------------------------------
# the module-level predicates (nefes_amd/field.py), on CPU modules
# ------------------------------------------------------------------------------------------------------------------------------
MODULES = [("fine,W=256,C=16", dict(typ="fine", W=256, f_dim=16, encode_transient=True)),
           ("fine,W=256,C=128", dict(typ="fine", W=256, f_dim=128, encode_transient=True)),
           ("fine,W=128,C=128", dict(typ="fine", W=128, f_dim=128, encode_transient=True)),
           ("fine,W=128,C=16", dict(typ="fine", W=128, f_dim=16, encode_transient=True)),
           ("fine,W=128,C=128,no transient", dict(typ="fine", W=128, f_dim=128)),
           ("coarse,W=256,C=16", dict(typ="coarse", W=256, f_dim=16)),
           ("fine,W=256,C=16,ext", dict(typ="fine", W=256, f_dim=16, encode_transient=True, in_channels_xyz=32)),
           ("fine,W=128,C=128,reduced", dict(typ="fine", W=128, f_dim=128, encode_transient=True, in_channels_xyz=33, in_channels_dir=15)),
           ("fine,W=64,D=2,C=16", dict(typ="fine", W=64, D=2, f_dim=16, encode_transient=True)),
           ("fine,W=256,D=6,C=16", dict(typ="fine", W=256, D=6, f_dim=16, encode_transient=True)),
           ("fine,W=256,C=200", dict(typ="fine", W=256, f_dim=200, encode_transient=True))]
MODULE_SWITCHES = [{"SPLIT": s, "USE_X6": x, "FIELD_GENERIC": g, "FOLD_FINAL": f, "FACTORED_HEAD": h}
                   for s, x in SPLITS for g in (False, True) for f, h in ((True, True), (False, True), (True, False))]
MODULE_CALLS = [("fold_ok", lambda net: bool(net.fold_ok())), ("factored_head_ok", lambda net: bool(net.factored_head_ok())),
                ("uses_generic", lambda net: bool(net.uses_generic()))]


def modules():
    out = []
    for name, kw in MODULES:
        for frozen in (True, False):
            net = F.NeRFH_NFF(**kw)
            net.requires_grad_(not frozen)
            out.append((f"{name},{'frozen' if frozen else 'trainable'}", net))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
def cases():
    """Every case as (case id, thunk -> outcome string); run inside patched()."""
    lists = {"tuned": tuned_calls(), "generic": generic_calls()}
    make = {"tuned": tuned_pack, "generic": generic_pack}
    for pid, kind, args in packs():
        pk = make[kind](*args)
        for k, sw in enumerate(switch_sets(pid)):
            for cid, fn, once in lists[kind]:
                if once and k:
                    continue

                def thunk(pk=pk, sw=sw, fn=fn):
                    set_switches(sw)
                    return outcome(fn, pk)
                yield f"{pid} | {switch_id(sw)} | {cid}", thunk
    for mid, net in modules():
        for sw in MODULE_SWITCHES:
            for cid, fn in MODULE_CALLS:
                def thunk(net=net, sw=sw, fn=fn):
                    set_switches(sw)
                    return outcome(fn, net)
                yield f"{mid} | {switch_id(sw)} | {cid}", thunk


def record():
    """-> {"outcomes": [distinct outcome strings], "cases": [index into outcomes per case, in cases() order], "n": count,
    "ids_sha256": digest of the case ids in that order}, [case ids]"""
    table, idx, ids = {}, [], []
    with patched():
        for cid, thunk in cases():
            o = thunk()
            idx.append(table.setdefault(o, len(table)))
            ids.append(cid)
    return {"outcomes": list(table), "cases": idx, "n": len(idx), "ids_sha256": hashlib.sha256("\n".join(ids).encode()).hexdigest()}, ids


def main():
    rec, ids = record()
    with open(OUT, "w") as f:
        json.dump(rec, f, separators=(",", ":"))
        f.write("\n")
    print(f"{OUT}: {rec['n']} cases, {len(rec['outcomes'])} distinct outcomes, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()

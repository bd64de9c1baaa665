"""Hash-grid fields of any --netwidth / --netdepth: the generic field kernels on a SUPPLIED 32-feature encoding
(nefes_amd/csrc/field_generic.hip gen_fwd_kernel / gen_bwd_kernel<NCB, GenArgsExt>, nefes_field_fwd_generic_ext / nefes_field_bwd_generic_ext).

Ground truth: oracle/ref_cpu.py (+ oracle/hashgrid_ref.py through the grid) in float64, the fp32 oracle next to it.  Bounds, the
project's (tests/branch.py, tests/parity_log.py): outputs and gradients e_hip <= max(1e-4, 1.5 e_ref), gradients on the kernels' own
ReLU branches (tests/generic_util.py decodes the generic mask words); the table gradient a flat 1e-4 of float64 autograd, as
tests/test_gpu_hashgrid_train.py has it.  Before these instances existed every case below raised ("no field kernel serves" / "not
built for the generic field kernels")."""
import ctypes as C
import functools
import types

import pytest
import torch

from oracle import hashgrid_ref as HG
from oracle import ref_cpu as O
from tests import branch as B
from tests import generic_util as G
from tests import parity_log as P
from tests.test_gpu_hashgrid_c128 import BOUND, FAR, FOCAL_AT_854, NEAR, POSE, TABLE_GAIN, _oracle_render, _render_kwargs

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (W, D, C, N, S): skip layer + a ragged last tile; the reference's default width with its 128-channel head; no skip (gE from layer 1
# alone); depth 1 (layer 1 also takes the static density's rank-1 term); the 32-sample tile above width 256, twice; S = 1
SHAPES = [(64, 6, 16, 7, 33), (128, 8, 128, 5, 24), (128, 4, 30, 11, 17), (32, 1, 16, 2, 65), (320, 7, 29, 4, 50), (512, 8, 16, 3, 40),
          (96, 5, 141, 5, 1)]
KEYS = {f"field_{d}[{m},generic,ext]" for d, m in (("fwd", "full"), ("bwd", "full"), ("fwd", "static"), ("bwd", "static"), ("fwd", "sigma"))}


def _inputs(C, N, S, seed):
    g = torch.Generator().manual_seed(seed)
    enc = (torch.rand(N, S, 32, generator=g) * 2 - 1) * 0.4
    v = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    return enc, v, torch.randn(N, 9 + C, S, generator=g)


def _oracle(net, D, enc, v, dt, transient=True, sigma=False, act=None, G_up=None):
    """The oracle's field on a supplied encoding -> raw [N, S, R]; with G_up [N, R, S] also d sum(raw G_up) / d (enc, viewdirs)."""
    N, S = enc.shape[:2]
    e = enc.reshape(-1, 32).detach().clone().to(dt).requires_grad_(G_up is not None)
    vv = v.detach().clone().to(dt).requires_grad_(G_up is not None)
    p = G.oracle_params(net, dt)
    a = None if act is None else (lambda tag, pre: act(tag, pre, 0))
    if sigma:
        return O.field_forward(p, e, sigma_only=True, in_xyz=32, D=D, skip=4).reshape(N, S, 1).detach()
    ed = O.freq_encode(vv[:, None].expand(N, S, 3).reshape(-1, 3), 4)
    raw = O.field_forward(p, torch.cat([e, ed], 1), output_transient=transient, in_xyz=32, D=D, skip=4, act=a).reshape(N, S, -1)
    if G_up is None:
        return raw.detach()
    ge, gv = torch.autograd.grad((raw * G_up.permute(0, 2, 1).to(dt)).sum(), (e, vv))
    return {"d enc": ge.reshape(N, S, 32), "d viewdirs": gv}


@functools.lru_cache(maxsize=None)
def _case(Wd, D, C, N, S):
    """One FULL forward of FieldFromEncoding on the generic pack, its masks and graph: computed once, shared, never modified."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    coarse, fine = G.modules(Wd, D, C, in_xyz=32, device=DEV)
    assert fine.uses_generic() and coarse.uses_generic() and fine.packed_any().xyz_encoding == L.XYZ_EXTERNAL32
    enc, v, G_up = _inputs(C, N, S, 100 + Wd + N)
    enc_h, v_h = enc.to(DEV).requires_grad_(), v.to(DEV).requires_grad_()
    ops.TIMERS = timers = {}
    try:
        with B.tapped() as tap:
            raw_t = ops.FieldFromEncoding.apply(enc_h, v_h, fine.packed_any(), L.FIELD_FULL)
    finally:
        ops.TIMERS = None
    return types.SimpleNamespace(coarse=coarse, fine=fine, enc=enc, v=v, G=G_up, enc_h=enc_h, v_h=v_h, raw_t=raw_t, tap=dict(tap),
                                 timers=set(timers))


@pytest.mark.parametrize("Wd,D,C,N,S", SHAPES)
def test_field_on_a_supplied_encoding(Wd, D, C, N, S):
    """FULL, STATIC (the coarse network) and SIGMA through FieldFromEncoding on packed_any(): raw outputs three-way; d enc and
    d viewdirs of FULL and of STATIC on the kernels' own branches."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    c = _case(Wd, D, C, N, S)
    tag = f"generic_ext[{Wd},{D},{C},{N},{S}]"
    assert c.timers == {"field_fwd[full,generic,ext]"}, c.timers
    assert c.raw_t.shape == (N, 9 + C, S) and torch.isfinite(c.raw_t).all()
    B.three_way(tag, "raw full", c.raw_t.permute(0, 2, 1), _oracle(c.fine, D, c.enc, c.v, torch.float32), _oracle(c.fine, D, c.enc, c.v, torch.float64))
    ops.TIMERS = timers = {}
    try:
        ge, gv = torch.autograd.grad((c.raw_t * c.G.to(DEV)).sum(), (c.enc_h, c.v_h), retain_graph=True)
        assert ge.shape == (N, S, 32) and torch.isfinite(ge).all() and float(ge.abs().max()) > 0
        G.pinned_gradients_generic(tag, {"d enc": ge, "d viewdirs": gv}, c.tap,
                                   lambda dt, act, _: _oracle(c.fine, D, c.enc, c.v, dt, act=act, G_up=c.G))
        # the static head of the coarse network (a render with test_time False), forward and backward
        Gs = c.G[:, :4 + C].contiguous()
        enc_h, v_h = c.enc.to(DEV).requires_grad_(), c.v.to(DEV).requires_grad_()
        with B.tapped() as tap:
            raw_s = ops.FieldFromEncoding.apply(enc_h, v_h, c.coarse.packed_any(), L.FIELD_STATIC)
        assert raw_s.shape == (N, 4 + C, S)
        ge, gv = torch.autograd.grad((raw_s * Gs.to(DEV)).sum(), (enc_h, v_h))
        assert ge.shape == (N, S, 32) and torch.isfinite(ge).all() and float(ge.abs().max()) > 0
        B.three_way(tag, "raw static", raw_s.permute(0, 2, 1), _oracle(c.coarse, D, c.enc, c.v, torch.float32, transient=False),
                    _oracle(c.coarse, D, c.enc, c.v, torch.float64, transient=False))
        G.pinned_gradients_generic(tag + " static", {"d enc": ge, "d viewdirs": gv}, tap,
                                   lambda dt, act, _: _oracle(c.coarse, D, c.enc, c.v, dt, transient=False, act=act, G_up=Gs))
        with torch.no_grad():
            sig = ops.FieldFromEncoding.apply(c.enc.to(DEV), None, c.coarse.packed_any(), L.FIELD_SIGMA)
        B.three_way(tag, "raw sigma", sig.permute(0, 2, 1), _oracle(c.coarse, D, c.enc, c.v, torch.float32, sigma=True),
                    _oracle(c.coarse, D, c.enc, c.v, torch.float64, sigma=True))
    finally:
        ops.TIMERS = None
    assert set(timers) == (KEYS - {"field_fwd[full,generic,ext]"}) | {"ray_grad_reduce"}, sorted(timers)


@pytest.mark.parametrize("Wd,D,C,N,S", SHAPES[:2])
def test_backward_one_upstream_channel_at_a_time(Wd, D, C, N, S):
    """A gradient that enters through ONE channel: the first colour channel, the first and the last feature channel, the static density
    and each transient channel.  Branch-pinned, max(1e-4, 1.5 e_ref) each."""
    c = _case(Wd, D, C, N, S)
    chans = {"rgb0": 0, "feat_first": 3, "feat_last": 2 + C, "sigma_s": 3 + C, "rgb_t0": 4 + C, "rgb_t1": 5 + C, "rgb_t2": 6 + C,
             "sigma_t": 7 + C, "beta": 8 + C}
    pin = G.GenericPinned(c.tap)
    for name, ch in chans.items():
        G_up = torch.zeros(N, 9 + C, S)
        G_up[:, ch] = c.G[:, ch]
        ge, gv = torch.autograd.grad((c.raw_t * G_up.to(DEV)).sum(), (c.enc_h, c.v_h), retain_graph=True)
        g64 = _oracle(c.fine, D, c.enc, c.v, torch.float64, act=pin.act(False), G_up=G_up)
        g32 = _oracle(c.fine, D, c.enc, c.v, torch.float32, act=pin.act(False), G_up=G_up)
        for what, got in (("d enc", ge), ("d viewdirs", gv)):
            if not g64[what].any():                                 # (static sigma does not see the view direction)
                assert not got.any(), (name, what)
                continue
            B.three_way(f"generic_ext_one_channel[{Wd},{D},{C}]", f"{name}: {what} [branch-pinned]", got, g32[what], g64[what])


def _launch(pk, mode, N, S, enc, v, g_up, guard):
    """The two C entry points on buffers with `guard` sentinel floats behind raw_t, the masks, g_xyz_enc and g_viewdirs_s (memory of
    the test's own, inside its allocations) -> the buffers."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    lib = L.load()
    M, R = N * S, pk.n_raw(mode)
    SENT, ISENT = 12345.5, 0x5a5a5a5a
    raw = torch.full((N * R * S + guard,), SENT, device=DEV)
    masks = torch.full((pk.mask_bytes(M) // 4 + guard,), ISENT, dtype=torch.int32, device=DEV)
    g_enc = torch.full((M * 32 + guard,), SENT, device=DEV)
    g_vs = torch.full((M * 3 + guard,), SENT, device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    L.check(lib.nefes_field_fwd_generic_ext(pk.desc, p(pk.blob), mode, N, S, p(enc), p(v), p(raw), p(masks), ops._stream()), "fwd")
    g_raw = torch.zeros(N, R, S, device=DEV)
    g_raw[:g_up.shape[0]] = g_up
    L.check(lib.nefes_field_bwd_generic_ext(pk.desc, p(pk.blob), mode, N, S, p(v), p(raw), p(g_raw), p(masks), p(g_enc), p(g_vs),
                                            ops._stream()), "bwd")
    torch.cuda.synchronize()
    for name, t in (("raw_t", raw), ("g_xyz_enc", g_enc), ("g_viewdirs_s", g_vs)):
        assert bool((t[t.numel() - guard:] == SENT).all()), f"{name}: written behind its end"
    assert bool((masks[masks.numel() - guard:] == ISENT).all()), "masks: written behind their end"
    return raw[:N * R * S].view(N, R, S), g_enc[:M * 32].view(M, 32), g_vs[:M * 3].view(M, 3)


@pytest.mark.parametrize("Wd,D,C,N,S,N_up", [(64, 6, 16, 7, 33, 64), (320, 7, 29, 4, 50, 16)])
def test_dead_columns_write_nothing_and_contribute_nothing(Wd, D, C, N, S, N_up):
    """N S is no multiple of the tile (64 / 32 samples): nothing is written behind raw_t, the mask words, g_xyz_enc or g_viewdirs_s, and
    the live rows are bit-identical to those of a launch whose samples fill whole tiles (more rays, zero upstream gradient there)."""
    from nefes_amd import lib as L
    _, fine = G.modules(Wd, D, C, in_xyz=32, device=DEV)
    pk = fine.packed_generic()
    assert (N * S) % pk.tile and not (N_up * S) % pk.tile
    enc, v, G_up = (t.to(DEV).contiguous() for t in _inputs(C, N_up, S, 7))
    G_up[N:] = 0
    ragged = _launch(pk, L.FIELD_FULL, N, S, enc[:N].contiguous(), v[:N].contiguous(), G_up[:N], 64)
    whole = _launch(pk, L.FIELD_FULL, N_up, S, enc, v, G_up[:N], 64)
    M = N * S
    assert torch.isfinite(ragged[0]).all() and float(ragged[1].abs().max()) > 0
    assert torch.equal(ragged[0], whole[0][:N])
    assert torch.equal(ragged[1], whole[1][:M]) and torch.equal(ragged[2], whole[2][:M])


@pytest.mark.parametrize("C", [16, 128])
def test_generic_against_tuned_on_the_same_weights(C):
    """packed_generic() and packed() of one (256, 8) network through FieldFromEncoding: each within the rules above of float64, forward
    and backward (each backward on its own forward's branches).  The ratio of the two errors is recorded, not bounded."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    Wd, D, N, S = 256, 8, 7, 33
    _, fine = G.modules(Wd, D, C, in_xyz=32, device=DEV)
    assert not fine.uses_generic()
    enc, v, G_up = _inputs(C, N, S, 11 + C)
    tag = f"generic_ext_vs_tuned[{C}]"
    r32, r64 = _oracle(fine, D, enc, v, torch.float32), _oracle(fine, D, enc, v, torch.float64)
    run = lambda dt, act, _: _oracle(fine, D, enc, v, dt, act=act, G_up=G_up)
    errs = {}
    for kind, pk in (("generic", fine.packed_generic()), ("tuned", fine.packed())):
        enc_h, v_h = enc.to(DEV).requires_grad_(), v.to(DEV).requires_grad_()
        ops.TIMERS = timers = {}
        try:
            with B.tapped() as tap:
                raw_t = ops.FieldFromEncoding.apply(enc_h, v_h, pk, L.FIELD_FULL)
            ge, gv = torch.autograd.grad((raw_t * G_up.to(DEV)).sum(), (enc_h, v_h))
        finally:
            ops.TIMERS = None
        assert ("field_fwd[full,generic,ext]" in timers) == (kind == "generic") and ("field_fwd[full,h3]" in timers) == (kind == "tuned")
        errs[kind] = {"raw": B.three_way(tag, f"{kind}: raw full", raw_t.permute(0, 2, 1), r32, r64)[0]}
        hip = {"d enc": ge, "d viewdirs": gv}
        out = G.pinned_gradients_generic(f"{tag} {kind}", hip, tap, run) if kind == "generic" else B.pinned_gradients(f"{tag} {kind}", hip, tap, Wd, run)
        errs[kind].update({k: e[0] for k, e in out.items()})
    for k in errs["generic"]:
        P.record(tag, f"{k}: generic error / tuned error", e_hip=errs["generic"][k], e_ref=errs["tuned"][k],
                 ratio=errs["generic"][k] / max(errs["tuned"][k], 1e-30), bound=None)


def _pair(Wd, D, C):
    from nefes_amd import ops
    coarse, fine = G.modules(Wd, D, C, in_xyz=32, device=DEV)
    return coarse, fine, ops.HashGrid(BOUND, table=HG.make_table(0) * TABLE_GAIN)


def _p(net, dt):
    return G.oracle_params(net, dt)


@pytest.mark.parametrize("Wd,D,C", [(128, 8, 128), (64, 6, 16)])
def test_render_through_the_grid_at_test_time(Wd, D, C):
    """render() of a coarse + fine pair behind a hash grid, 4 x 6 rays, 16 + 16 samples: maps three-way against the oracle composed as
    tests/test_gpu_cam.py composes it; d c2w on the kernels' branches and depths."""
    from nefes_amd import ops
    from nefes_amd.render import render
    NC, NI, H, W = 16, 16, 4, 6
    coarse, fine, grid = _pair(Wd, D, C)
    table = grid.table.detach().cpu()
    focal = FOCAL_AT_854 * W / 854.
    pose = O.se3_exp_pose(*POSE)
    c2w = pose.to(DEV).requires_grad_()
    ops.TIMERS = timers = {}
    try:
        with B.tapped() as tap:
            rgb, disp, acc, ex = render(H, W, focal, c2w=c2w, near=NEAR, far=FAR, **_render_kwargs(coarse, fine, grid, NC, NI))
        feat = ex["feat_map"]
        (gh,) = torch.autograd.grad(O.bench_loss(rgb, feat), c2w)
    finally:
        ops.TIMERS = None
    assert {"hashgrid_fwd", "hashgrid_bwd_x", "field_fwd[sigma,generic,ext]", "field_fwd[full,generic,ext]", "field_bwd[full,generic,ext]"} <= set(timers), \
        sorted(timers)
    assert not [k for k in timers if "h3" in k or "hashgrid]" in k], sorted(timers)
    assert rgb.shape == (H * W, 3) and feat.shape == (H * W, C)
    tag = f"generic_ext_render[{Wd},{D},{C}]"

    def run(dt, act, zf, p_):
        with G.oracle_depth(D):
            return _oracle_render(H, W, NC, NI, p_, _p(coarse, dt), _p(fine, dt), table.to(dt), dt, True, None, act, zf)

    outs = {dt: run(dt, None, None, pose.to(dt))[0] for dt in (torch.float32, torch.float64)}
    for name, got in (("rgb", rgb), ("feat", feat), ("disp", disp), ("acc", acc)):
        B.three_way(tag, name, got, getattr(outs[torch.float32], name), getattr(outs[torch.float64], name))

    def oracle_run(dt, act, zf):
        c = pose.to(dt).requires_grad_()
        return {"d c2w": torch.autograd.grad(run(dt, act, zf, c)[1], c)[0]}

    assert torch.isfinite(gh).all() and float(gh.abs().max()) > 0
    G.pinned_gradients_generic(tag, {"d c2w": gh}, tap, oracle_run)


@pytest.mark.parametrize("Wd,D,C", [(128, 8, 128), (64, 6, 16)])
def test_trainable_table_behind_frozen_generic_networks(Wd, D, C):
    """test_time False, grid.table.requires_grad_(True), frozen networks: the coarse pass is the STATIC forward + backward of the generic
    kernels, the fine pass the FULL ones; d table within a flat 1e-4 of float64 autograd on the kernels' branches and depths."""
    from nefes_amd import ops
    from nefes_amd.render import render
    NC, NI, H, W = 16, 16, 4, 6
    coarse, fine, grid = _pair(Wd, D, C)
    grid.table.requires_grad_(True)
    focal = FOCAL_AT_854 * W / 854.
    pose = O.se3_exp_pose(*POSE)
    ops.TIMERS = timers = {}
    try:
        with B.tapped() as tap:
            rgb, disp, acc, ex = render(H, W, focal, c2w=pose.to(DEV), near=NEAR, far=FAR, **_render_kwargs(coarse, fine, grid, NC, NI, False))
            (O.bench_loss(rgb, ex["feat_map"]) + O.bench_loss(ex["rgb0"], ex["feat0"])).backward()
    finally:
        ops.TIMERS = None
    assert {"field_fwd[static,generic,ext]", "field_bwd[static,generic,ext]", "field_fwd[full,generic,ext]", "field_bwd[full,generic,ext]",
            "hashgrid_bwd_table"} <= set(timers), sorted(timers)
    assert not [k for k in timers if "train" in k or "h3" in k], sorted(timers)
    g_tab = grid.table.grad
    assert g_tab is not None and torch.isfinite(g_tab).all() and float(g_tab.abs().max()) > 0
    assert len(tap["masks_generic"]) == 2
    coarse_pin = G.GenericPinned(tap, index=0)
    tag = f"generic_ext_table[{Wd},{D},{C}]"

    # float64 autograd on the kernels' branches (coarse and fine) and depths.  One oracle run, not the usual fp32 + float64 pair: the
    # bound is flat, so the fp32 oracle's own error does not enter it, and d loss / d table through the oracle's dense table is the
    # slow part of this test.
    fine_pin = G.GenericPinned(tap)
    dt = torch.float64
    tab = grid.table.detach().cpu().to(dt).requires_grad_()
    with G.oracle_depth(D):
        _, loss = _oracle_render(H, W, NC, NI, pose.to(dt), _p(coarse, dt), _p(fine, dt), tab, dt, False, coarse_pin.act(True),
                                 fine_pin.act(True), fine_pin.z_fine)
    (g64,) = torch.autograd.grad(loss, tab)
    for name, pin in (("coarse", coarse_pin), ("fine", fine_pin)):
        flips, units, worst = pin.summary()
        print(f"[{tag}] {name} ReLU branch pattern vs float64: {flips} of {units} units differ, worst {worst:.1e}")
        P.record(tag, f"{name}: relu branch flips vs float64", flips=flips, units=units, worst_preact_rel=worst)
        assert worst < B.AUDIT_CLASSES["same_inputs"] and flips <= max(8, units // 100000), (name, flips, units, worst)
    e = B.rel(g_tab, g64)
    print(f"[{tag}] d table vs float64 autograd [branch-pinned]: {e:.2e}")
    P.record(tag, "d table [branch-pinned, flat bound]", e_hip=e, e_ref=None, bound=1e-4)
    assert e < 1e-4, e


@pytest.mark.parametrize("generic_train", [False, True])
def test_trainable_weights_behind_an_encoder_stay_refused(generic_train, monkeypatch):
    from nefes_amd import ops
    from nefes_amd.render import render
    monkeypatch.setattr(ops, "GENERIC_TRAIN", generic_train)
    coarse, fine, grid = _pair(64, 6, 16)
    fine.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="train mode.*D=6.*W=64.*in_channels_xyz=32"):
        render(2, 3, FOCAL_AT_854 * 3 / 854., c2w=O.se3_exp_pose(*POSE).to(DEV), near=NEAR, far=FAR,
               **_render_kwargs(coarse, fine, grid, 16, 16, False))


@pytest.mark.parametrize("Wd,D", [(48, 8), (64, 9)])
def test_unsupported_shapes_on_32_inputs_raise_naming_the_shape(Wd, D):
    from nefes_amd.render import render
    coarse, fine, grid = _pair(Wd, D, 16)
    with pytest.raises(RuntimeError, match=f"D={D}.*W={Wd}.*in_channels_xyz=32"):
        render(2, 3, FOCAL_AT_854 * 3 / 854., c2w=O.se3_exp_pose(*POSE).to(DEV), near=NEAR, far=FAR, **_render_kwargs(coarse, fine, grid, 16, 16))


def test_two_streams_give_identical_results():
    """Forward + backward of (64, 6, 16, 7, 33) alone, and the same launches while a second stream runs the tuned fp16 forward."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    Wd, D, C, N, S = SHAPES[0]
    _, fine = G.modules(Wd, D, C, in_xyz=32, device=DEV)
    pk = fine.packed_generic()
    enc, v, G_up = (t.to(DEV) for t in _inputs(C, N, S, 3))
    _, tuned = G.modules(256, 8, 16, device=DEV)
    pk_t = tuned.packed()
    g = torch.Generator().manual_seed(4)
    o, d = (torch.rand(2048, 3, generator=g) - .5).to(DEV), torch.randn(2048, 3, generator=g).to(DEV)
    z = torch.sort(torch.rand(2048, 96, generator=g) * 4, -1)[0].to(DEV)
    vt = torch.nn.functional.normalize(d, dim=-1)

    def run():
        e, vv = enc.clone().requires_grad_(), v.clone().requires_grad_()
        raw = ops.FieldFromEncoding.apply(e, vv, pk, L.FIELD_FULL)
        raw.backward(G_up)
        return raw.detach().clone(), e.grad.clone(), vv.grad.clone()

    base = run()
    with torch.no_grad():
        ops.field_from_rays(o, d, vt, z, pk_t, L.FIELD_FULL)           # (first-launch work of the tuned kernel, outside the overlap)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(device=DEV), torch.cuda.Stream(device=DEV)
    for s in (s1, s2):
        s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s2), torch.no_grad():
        for _ in range(3):
            ops.field_from_rays(o, d, vt, z, pk_t, L.FIELD_FULL)
    with torch.cuda.stream(s1):
        out = run()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(base, out))

"""Hash-grid fields with the reference's 128-channel feature head: width 256, NEFES_XYZ_EXTERNAL32, head class 1 (30 <= C <= 141).

The instances under test (csrc/field_h3_instances.h, the <..., EXTERNAL32, 256, 5, ...> / <256, 9, EXTERNAL32, ...> rows): the full pass on a supplied encoding, its
backward-to-inputs, and the train-mode pair; the sigma-only instances are the class-0 ones, reached for class 1 too.  No instance of
this class gathers the hash grid itself (the backward did not keep the accumulator tiles in place), so renders take
HashGridEncode + FieldFromEncoding -- the routing is asserted, and the composition is checked against the oracle through the grid.

Ground truth: oracle/hashgrid_ref.py + oracle/ref_cpu.py in float64, the fp32 oracle next to it.  Bounds, as tests/test_gpu_cam.py and
tests/test_gpu_hashgrid_train.py apply them to C = 16 (tests/branch.py, tests/parity_log.py):
    raw outputs against float64                      max(3e-6, 3 e_ref), worst channel, relative to that channel's maximum
    gradients on the kernels' own ReLU branches      max(1e-4, 1.5 e_ref)
    weight / table gradients against float64         a flat 1e-4, branch-pinned
e_ref = the fp32 oracle's own distance from float64.  Sample points stay on the positive side of -bound (the oracle's int64 dense index
does not wrap like the kernels' uint32 for negative cells) and the render cases use far 6 (tests/test_gpu_hashgrid_train.py's note on
the coarse static_sigma weight gradient at far 20)."""
import functools
import types

import pytest
import torch

from oracle import hashgrid_ref as HG
from oracle import ref_cpu as O
from tests import branch as B
from tests import parity_log as P
from tests.test_gpu_train import _oracle_params

pytestmark = pytest.mark.gpu
DEV = "cuda"
WD = 256
BOUND, NEAR, FAR, FOCAL_AT_854 = 25.0, 0., 6., 744.
TABLE_GAIN = 3e3                 # as tests/test_gpu_cam.py: O(0.3) features, so that the MLP sees the position
# (C, N, S): 7 x 33 = 231 samples = one full tile + a tile of three full waves and a wave of 7; 41 x 24 = 984 = seven tiles + 88
SHAPES = [(30, 7, 33), (128, 41, 24), (141, 7, 33), (128, 7, 33)]


def _net(typ, C, trainable=False):
    from nefes_amd.field import NeRFH_NFF
    if typ == "coarse":
        net = NeRFH_NFF('coarse', W=WD, f_dim=C, in_channels_xyz=32)
    else:
        net = NeRFH_NFF('fine', W=WD, f_dim=C, in_channels_xyz=32, encode_appearance=True, encode_transient=True)
    return net.requires_grad_(trainable).to(DEV)


def _grid(seed=0, trainable=False):
    from nefes_amd import ops
    grid = ops.HashGrid(BOUND, table=HG.make_table(seed) * TABLE_GAIN)
    if trainable:
        grid.table.requires_grad_(True)
    return grid


def _per_channel_err(got_nrs, ref_nsr):
    sc = ref_nsr.abs().amax((0, 1)).clamp_min(1e-30)
    return float(((got_nrs.permute(0, 2, 1).cpu().double() - ref_nsr.double()).abs().amax((0, 1)) / sc).max())


def _p(net, dt):
    return {k: v.detach().cpu().to(dt) for k, v in net.named_parameters() if not k.startswith(("fusion_net", "exposure_embedding"))}


@functools.lru_cache(maxsize=None)
def _encoded_case(C, N, S):
    """One forward of the class-1 full pass on a supplied encoding (FieldFromEncoding), its masks, and the oracles' outputs: computed
    once, shared by the tests below, never modified."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    net, coarse = _net("fine", C), _net("coarse", C)
    g = torch.Generator().manual_seed(100 + C + N)
    enc = (torch.rand(N, S, 32, generator=g) * 2 - 1) * 0.4
    v = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    G = torch.randn(N, 9 + C, S, generator=g)
    enc_h, v_h = enc.to(DEV).requires_grad_(), v.to(DEV).requires_grad_()
    ops.TIMERS = timers = {}
    try:
        with B.tapped() as tap:
            raw_t = ops.FieldFromEncoding.apply(enc_h, v_h, net.packed(), L.FIELD_FULL)
        with torch.no_grad():
            sig_t = ops.FieldFromEncoding.apply(enc_h.detach(), None, coarse.packed(), L.FIELD_SIGMA)
    finally:
        ops.TIMERS = None
    ed = lambda dt: O.freq_encode(v.to(dt)[:, None].expand(N, S, 3).reshape(-1, 3), 4)
    ref = {dt: O.field_forward(_p(net, dt), torch.cat([enc.reshape(-1, 32).to(dt), ed(dt)], 1), output_transient=True, in_xyz=32).reshape(N, S, -1)
           for dt in (torch.float32, torch.float64)}
    sig = {dt: O.field_forward(_p(coarse, dt), enc.reshape(-1, 32).to(dt), sigma_only=True, in_xyz=32).reshape(N, S, 1)
           for dt in (torch.float32, torch.float64)}
    return types.SimpleNamespace(net=net, coarse=coarse, enc=enc, v=v, G=G, enc_h=enc_h, v_h=v_h, raw_t=raw_t, sig_t=sig_t, tap=dict(tap),
                                 timers=set(timers), ref=ref, sig=sig, ed=ed)


def _oracle_input_grads(c, C, N, S, G, dt, act):
    """d sum(raw * G) / d (enc, viewdirs) of the oracle's field on a given ReLU branch pattern."""
    e = c.enc.reshape(-1, 32).to(dt).requires_grad_()
    v = c.v.to(dt).requires_grad_()
    ed = O.freq_encode(v[:, None].expand(N, S, 3).reshape(-1, 3), 4)
    raw = O.field_forward(_p(c.net, dt), torch.cat([e, ed], 1), output_transient=True, in_xyz=32,
                          act=lambda tag, pre: act(tag, pre, 0)).reshape(N, S, -1)
    ge, gv = torch.autograd.grad((raw * G.permute(0, 2, 1).to(dt)).sum(), (e, v))
    return {"d enc": ge.reshape(N, S, 32), "d viewdirs": gv}


@pytest.mark.parametrize("C,N,S", SHAPES)
def test_full_and_sigma_forward_on_a_supplied_encoding(C, N, S):
    """FULL through FieldFromEncoding and sigma-only (the class-0 instance, reached for class 1) against the float64 oracle; the fp32
    oracle itself is inside the bound's floor regime it is compared with (checked on the CPU values)."""
    c = _encoded_case(C, N, S)
    assert c.timers == {"field_fwd[full,h3]", "field_fwd[sigma,h3]"}, c.timers
    assert c.raw_t.shape == (N, 9 + C, S) and torch.isfinite(c.raw_t).all()
    e_ref = _per_channel_err(c.ref[torch.float32].permute(0, 2, 1), c.ref[torch.float64])
    e_hip = _per_channel_err(c.raw_t.detach(), c.ref[torch.float64])
    assert e_ref < 3e-6, e_ref                                      # the fp32 oracle on these inputs: the rule is not vacuous
    print(f"[hashgrid_c128] C={C} {N}x{S}: raw vs float64 (worst channel) hip {e_hip:.2e}  fp32 oracle {e_ref:.2e}")
    P.record(f"hashgrid_c128_full[{C},{N},{S}]", "raw (worst channel)", e_hip=e_hip, e_ref=e_ref, bound=max(3e-6, 3 * e_ref))
    assert e_hip <= max(3e-6, 3 * e_ref), (e_hip, e_ref)
    s_ref = _per_channel_err(c.sig[torch.float32].permute(0, 2, 1), c.sig[torch.float64])
    s_hip = _per_channel_err(c.sig_t, c.sig[torch.float64])
    P.record(f"hashgrid_c128_sigma[{C},{N},{S}]", "sigma", e_hip=s_hip, e_ref=s_ref, bound=max(3e-6, 3 * s_ref))
    assert s_ref < 3e-6 and s_hip <= max(3e-6, 3 * s_ref), (s_hip, s_ref)


@pytest.mark.parametrize("C,N,S", SHAPES)
def test_backward_to_the_encoding_on_the_forward_masks(C, N, S):
    """The class-1 backward fed the class-1 forward's masks: d encoding / d viewdirs of a dense upstream gradient, branch-pinned."""
    c = _encoded_case(C, N, S)
    ge, gv = torch.autograd.grad((c.raw_t * c.G.to(DEV)).sum(), (c.enc_h, c.v_h), retain_graph=True)
    assert ge.shape == (N, S, 32) and torch.isfinite(ge).all() and float(ge.abs().max()) > 0
    B.pinned_gradients(f"hashgrid_c128_bwd[{C},{N},{S}]", {"d enc": ge, "d viewdirs": gv}, c.tap, WD,
                       lambda dt, act, zf: _oracle_input_grads(c, C, N, S, c.G, dt, act))


@pytest.mark.parametrize("C", [30, 128, 141])
def test_backward_one_upstream_channel_at_a_time(C):
    """A gradient that enters through ONE channel: the first, a middle and the last real feature channel (the last one sits in the
    head class's partial group of sixteen k-values for C = 30 and C = 141; the k-values behind it are padding), the first colour
    channel, and each of the six sigma / transient channels.  Branch-pinned, max(1e-4, 1.5 e_ref) each."""
    N, S = 7, 33
    c = _encoded_case(C, N, S)
    R = 9 + C
    chans = {"rgb0": 0, "feat_first": 3, "feat_mid": 3 + C // 2, "feat_last": 2 + C, "sigma_s": 3 + C, "rgb_t0": 4 + C, "rgb_t1": 5 + C,
             "rgb_t2": 6 + C, "sigma_t": 7 + C, "beta": 8 + C}
    pin = B.Pinned(c.tap, WD)
    for name, ch in chans.items():
        G = torch.zeros(N, R, S)
        G[:, ch] = c.G[:, ch]
        ge, gv = torch.autograd.grad((c.raw_t * G.to(DEV)).sum(), (c.enc_h, c.v_h), retain_graph=True)
        g64 = _oracle_input_grads(c, C, N, S, G, torch.float64, pin.act(False))
        g32 = _oracle_input_grads(c, C, N, S, G, torch.float32, pin.act(False))
        for what, got in (("d enc", ge), ("d viewdirs", gv)):
            if not g64[what].any():                                 # (static sigma does not see the view direction)
                assert not got.any(), (name, what)
                continue
            B.three_way(f"hashgrid_c128_one_channel[{C}]", f"{name}: {what} [branch-pinned]", got, g32[what], g64[what])


@pytest.mark.parametrize("C", [30, 128, 141])
@pytest.mark.parametrize("typ", ["coarse", "fine"])
def test_field_train_on_the_external_encoding_class1(typ, C, monkeypatch):
    """tests/test_gpu_hashgrid_train.py::test_field_train_on_the_external_encoding at head class 1, with its bounds: FieldTrainEncoded
    (STATIC for the coarse network, FULL for the fine one) on an N x S grid ragged against the 128-sample tiles, against the float64
    oracle on the kernels' own ReLU branch pattern -- saved pre-activations (and the E block = the encoding, natural order) within
    5e-6, raw outputs within 2e-5, every parameter gradient and d encoding / d viewdirs within a flat 1e-4 of their max-norm."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    from nefes_amd import train as TR
    from tests.test_gpu_train import _relerr
    monkeypatch.setattr(ops, "TIMERS", {})
    N, S = 37, 24                                                   # 888 samples: 7 tiles, the last one ragged
    mode = L.FIELD_STATIC if typ == "coarse" else L.FIELD_FULL
    net = _net(typ, C, True)
    g = torch.Generator().manual_seed(2 + C)
    enc = (torch.rand(N, S, 32, generator=g) * 2 - 1) * 0.4
    v = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    enc_h, v_h = enc.to(DEV).requires_grad_(), v.to(DEV).requires_grad_()
    names = TR.param_names(net, mode)
    sd = dict(net.named_parameters())
    TR.DEBUG = {}
    try:
        with B.tapped() as tap:
            raw_t = TR.FieldTrainEncoded.apply(enc_h, v_h, net, mode, *[sd[n] for n in names])
        acts, off = TR.DEBUG["acts"], TR.DEBUG["off"]
    finally:
        TR.DEBUG = None
    R, M = raw_t.shape[1], N * S
    assert R == 3 + C + (1 if typ == "coarse" else 6)
    p = _oracle_params(net, names)
    e = enc.reshape(-1, 32).double()
    got_e = acts[:, off[L.TB_E]:off[L.TB_E] + 32, :].permute(0, 2, 1).reshape(-1, 32)[:M].cpu().double()
    assert torch.equal(got_e, e.float().double())                   # the encoding itself, natural order
    h = e
    for l in range(1, 9):
        if l == 5:
            h = torch.cat([e, h], 1)
        pre = torch.nn.functional.linear(h, p[f"xyz_encoding_{l}.0.weight"].detach(), p[f"xyz_encoding_{l}.0.bias"].detach())
        got = acts[:, off[L.TB_L1 + l - 1]:off[L.TB_L1 + l - 1] + WD, :].permute(0, 2, 1).reshape(-1, WD)[:M].cpu().double()
        assert float((got - pre).abs().max()) < 5e-6, l
        h = torch.relu(pre)
    G = torch.randn(N, R, S, generator=g)
    (raw_t * G.to(DEV)).sum().backward()
    assert set(ops.TIMERS) == {"field_fwd_train[h3,ext]", "field_bwd_train[h3,ext]", "ray_grad_reduce"}, set(ops.TIMERS)
    pin = B.Pinned(tap, WD)
    e64 = e.clone().requires_grad_()
    v64 = v.double().requires_grad_()
    ed = O.freq_encode(v64[:, None].expand(N, S, 3).reshape(-1, 3), 4)
    raw = O.field_forward(p, torch.cat([e64, ed], 1), output_transient=typ == "fine", in_xyz=32,
                          act=lambda tag, pre: pin.act(True)(tag, pre, 0)).reshape(N, S, -1)
    flips, units, worst_pre = pin.summary()
    P.record(f"train_field_ext_c128[{typ},{C}]", "relu branch flips vs float64", flips=flips, units=units, worst_preact_rel=worst_pre)
    assert worst_pre < 2e-5 and flips <= max(8, units // 100000), (flips, units, worst_pre)
    assert _relerr(raw_t.permute(0, 2, 1), raw) < 2e-5
    (raw * G.permute(0, 2, 1).double()).sum().backward()
    worst = ("", 0.)
    for n in names:
        assert sd[n].grad is not None, n
        worst = max(worst, (n, _relerr(sd[n].grad, p[n].grad)), key=lambda t: t[1])
    for n, a_, b_ in (("d enc", enc_h.grad, e64.grad.reshape(N, S, 32)), ("d viewdirs", v_h.grad, v64.grad)):
        worst = max(worst, (n, _relerr(a_, b_)), key=lambda t: t[1])
    print(f"[train_field_ext_c128] {typ} C={C}: worst gradient {worst[0]} {worst[1]:.2e}")
    P.record(f"train_field_ext_c128[{typ},{C}]", "worst gradient [branch-pinned]", e_hip=worst[1], e_ref=None, bound=1e-4)
    assert worst[1] < 1e-4, worst


def _ray_inputs(N, S, seed):
    g = torch.Generator().manual_seed(seed)
    o = (torch.rand(N, 3, generator=g) - .5) * 8
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1)
    v = d.clone()
    d = d * (0.5 + torch.rand(N, 1, generator=g))
    z = torch.sort(torch.rand(N, S, generator=g) * FAR, -1)[0]
    return o, d, v, z, g


@pytest.mark.parametrize("C,N,S", [(30, 7, 33), (128, 41, 24), (141, 7, 33)])
def test_class1_takes_the_separate_launches_and_is_correct(C, N, S):
    """No fused-gather instance of head class 1 is built (csrc/field_h3_instances.h, the note at the backward's <256, 9, EXTERNAL32> row): hashgrid_fused_ok and
    fused_coarse_pass_ok say no, the fused entry point refuses the full pass loudly, and rays -> HashGridEncode -> FieldFromEncoding
    gives raw outputs within max(3e-6, 3 e_ref) of the float64 oracle and ray gradients branch-pinned within max(1e-4, 1.5 e_ref).
    The sigma-only gather instance has no rgb head and serves either class: bit-identical to the separate launches, also on one shared
    row of depths."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    coarse, fine = _net("coarse", C), _net("fine", C)
    table = HG.make_table(0) * TABLE_GAIN
    grid = ops.HashGrid(BOUND, table=table)
    o, d, v, z, g = _ray_inputs(N, S, 5 + C)
    assert float((o[:, None] + d[:, None] * z[..., None]).min()) > -BOUND          # positive side of the bound only
    G = torch.randn(N, 9 + C, S, generator=g)
    oh, dh, vh = (t.to(DEV).requires_grad_() for t in (o, d, v))
    zh, Gh = z.to(DEV), G.to(DEV)
    pk_c, pk_f = coarse.packed(), fine.packed()
    assert not ops.hashgrid_fused_ok(pk_f, grid) and not ops.hashgrid_fused_ok(pk_c, grid)
    assert not ops.fused_coarse_pass_ok(pk_c, 64, 64, N, grid)
    with pytest.raises(RuntimeError, match="Compiled: fp16 two-part instances"):
        ops.FieldFromRaysHashGrid.apply(oh, dh, vh, zh, pk_f, L.FIELD_FULL, grid)

    def separate(pk, mode):
        pts = oh[:, None, :] + dh[:, None, :] * zh[..., None]
        return ops.FieldFromEncoding.apply(grid(pts), vh, pk, mode)

    ops.TIMERS = timers = {}
    try:
        with B.tapped() as tap:
            raw_s = separate(pk_f, L.FIELD_FULL)
            gs = torch.autograd.grad((raw_s * Gh).sum(), (oh, dh, vh))
        sig_s = separate(pk_c, L.FIELD_SIGMA)
    finally:
        ops.TIMERS = None
    assert {"hashgrid_fwd", "field_fwd[full,h3]", "field_bwd[h3]", "hashgrid_bwd_x", "field_fwd[sigma,h3]"} <= set(timers), sorted(timers)
    assert not [k for k in timers if "hashgrid]" in k], sorted(timers)
    names = ("d rays_o", "d rays_d", "d viewdirs")

    def oracle_run(dt, act, zf, want_raw=False):
        o_, d_, v_ = (t.to(dt).requires_grad_() for t in (o, d, v))
        pts = o_[:, None] + d_[:, None] * z.to(dt)[..., None]
        e = HG.encode(pts.reshape(-1, 3), table.to(dt), BOUND)
        ed = O.freq_encode(v_[:, None].expand(N, S, 3).reshape(-1, 3), 4)
        a = None if act is None else (lambda tag, pre: act(tag, pre, 0))
        raw = O.field_forward(_p(fine, dt), torch.cat([e, ed], 1), output_transient=True, in_xyz=32, act=a).reshape(N, S, -1)
        if want_raw:
            return raw.detach()
        return dict(zip(names, torch.autograd.grad((raw * G.permute(0, 2, 1).to(dt)).sum(), (o_, d_, v_))))

    r32, r64 = oracle_run(torch.float32, None, None, True), oracle_run(torch.float64, None, None, True)
    e_ref, e_hip = _per_channel_err(r32.permute(0, 2, 1), r64), _per_channel_err(raw_s.detach(), r64)
    P.record(f"hashgrid_c128_rays[{C},{N},{S}]", "raw (worst channel)", e_hip=e_hip, e_ref=e_ref, bound=max(3e-6, 3 * e_ref))
    assert e_hip <= max(3e-6, 3 * e_ref), (e_hip, e_ref)
    B.pinned_gradients(f"hashgrid_c128_rays[{C},{N},{S}]", dict(zip(names, gs)), tap, WD, oracle_run)
    # the sigma-only pass with the gather inside the kernel: the class-0 instance, no rgb head
    sig_f = ops.FieldFromRaysHashGrid.apply(oh.detach(), dh.detach(), vh.detach(), zh, pk_c, L.FIELD_SIGMA, grid)
    assert torch.equal(sig_f, sig_s)
    z_row = ops.coarse_depth_row(64, NEAR, FAR, False, torch.device(DEV))
    sig_row = ops.field_sigma_row(pk_c, oh.detach(), dh.detach(), z_row, grid)
    pts = oh.detach()[:, None, :] + dh.detach()[:, None, :] * z_row[None, :, None]
    assert torch.equal(sig_row, ops.FieldFromEncoding.apply(grid(pts), None, pk_c, L.FIELD_SIGMA))


# ---- render() end to end ---------------------------------------------------------------------------------------------------------
def _render_kwargs(coarse, fine, grid, nc, ni, test_time=True):
    args = types.SimpleNamespace(nerfh_nff=True, use_fine_only=False, NeRFW=True, transient_at_test=True, netchunk=1 << 21)
    return dict(network_query_fn=None, perturb=False, N_importance=ni, N_samples=nc, network_fn=coarse, network_fine=fine,
                use_viewdirs=True, white_bkgd=False, raw_noise_std=0., test_time=test_time, args=args, ndc=False, lindisp=False,
                xyz_encoder=grid)


def _oracle_render(H, W, nc, ni, pose, pc, pf, tab, dt, test_time, coarse_act=None, fine_act=None, z_fine=None):
    """rendering.py:88-180 with the hash grid in front of both networks, composed from the oracle's stages as tests/test_gpu_cam.py and
    tests/test_gpu_hashgrid_train.py do; the coarse / fine passes on GIVEN ReLU branch patterns and fine depths."""
    focal = FOCAL_AT_854 * W / 854.
    o, d = O.ray_bundle(H, W, focal, pose)
    o, d = o.reshape(-1, 3), d.reshape(-1, 3)
    v = d / torch.norm(d, dim=-1, keepdim=True)
    n = o.shape[0]
    near, far = torch.full((n, 1), NEAR, dtype=dt), torch.full((n, 1), FAR, dtype=dt)
    z = O.coarse_depths(near, far, nc, False)

    def field(p, zz, sigma_only, act, transient):
        pts = o[:, None] + d[:, None] * zz[..., None]
        e = HG.encode(pts.reshape(-1, 3), tab, BOUND)
        a = None if act is None else (lambda tag, pre: act(tag, pre, 0))
        if sigma_only:
            return O.field_forward(p, e, sigma_only=True, in_xyz=32).reshape(n, zz.shape[1], 1)
        ed = O.freq_encode(v[:, None].expand(pts.shape).reshape(-1, 3), 4)
        return O.field_forward(p, torch.cat([e, ed], 1), output_transient=transient, in_xyz=32, act=a).reshape(n, zz.shape[1], -1)

    if test_time:
        c0 = O.composite(field(pc, z, True, None, False), z, test_time=True, typ="coarse")
    else:
        c0 = O.composite(field(pc, z, False, coarse_act, False), z, test_time=False, typ="coarse")
    zs = O.inverse_cdf_samples(.5 * (z[..., 1:] + z[..., :-1]), c0.weights[..., 1:-1].detach(), ni, det=True).detach()
    zf = torch.sort(torch.cat([z, zs], -1), -1)[0] if z_fine is None else z_fine.to(dt)
    c = O.composite(field(pf, zf, False, fine_act, True), zf, output_transient=True, test_time=test_time, typ="fine",
                    transient_at_test=True)
    loss = O.bench_loss(c.rgb, c.feat)
    if not test_time:
        loss = loss + O.bench_loss(c0.rgb, c0.feat)
    return c, loss


POSE = ((0.4, -0.9, 0.15), (3.0, -2.0, 4.5))


def _render_timer_keys(C):
    """Timer keys of one frozen render + backward-to-pose of a (256, C, hash grid) pair: which launches ran."""
    from nefes_amd import ops
    from nefes_amd.render import render
    coarse, fine = _net("coarse", C), _net("fine", C)
    grid = _grid(0)
    H, W = 2, 3
    c2w = O.se3_exp_pose(*POSE).to(DEV).requires_grad_()
    ops.TIMERS = timers = {}
    try:
        rgb, _, _, ex = render(H, W, FOCAL_AT_854 * W / 854., c2w=c2w, near=NEAR, far=FAR, **_render_kwargs(coarse, fine, grid, 64, 64))
        O.bench_loss(rgb, ex["feat_map"]).backward()
    finally:
        ops.TIMERS = None
    return set(timers)


# what a frozen (256, 16, hash grid) render + backward launched before the class-1 instances existed
C16_RENDER_LAUNCHES = {"field_fwd[sigma,h3,hashgrid]", "coarse_sample", "field_fwd[full,h3,hashgrid]", "composite_fwd", "composite_bwd",
                       "field_bwd[h3,hashgrid]", "ray_grad_reduce"}


def test_class0_hashgrid_render_launches_what_it_launched_before():
    """Unchanged routing: the (256, 16, ext) render takes the fused two-launch coarse pass and the fused-gather fine pass, nothing else
    and nothing generic; the C = 128 render takes the separate launches -- no kernel that gathers the grid itself."""
    k16 = _render_timer_keys(16)
    print("[hashgrid_c128] launches of the (256, 16, hash grid) render:", sorted(k16))
    assert k16 == C16_RENDER_LAUNCHES, sorted(k16)
    k128 = _render_timer_keys(128)
    assert not [k for k in k128 if "hashgrid]" in k or "generic" in k], sorted(k128)
    assert {"hashgrid_fwd", "hashgrid_bwd_x", "field_fwd[sigma,h3]", "field_fwd[full,h3]", "field_bwd[h3]"} <= k128, sorted(k128)


def test_render_cam_geometry_c128():
    """40 rays at the Cambridge camera geometry (bound 25), C = 128, 64 + 64 samples, far 6: maps three-way, d c2w branch-pinned."""
    from nefes_amd import ops
    from nefes_amd.render import render
    C, NC, NI, H, W = 128, 64, 64, 5, 8
    coarse, fine = _net("coarse", C), _net("fine", C)
    assert not coarse.uses_generic() and not fine.uses_generic()
    grid = _grid(0)
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
    assert {"hashgrid_fwd", "field_fwd[full,h3]", "field_bwd[h3]", "hashgrid_bwd_x"} <= set(timers), sorted(timers)     # the separate launches
    assert rgb.shape == (H * W, 3) and feat.shape == (H * W, C)
    tag = "hashgrid_c128_render[bound 25, far 6]"
    run = lambda dt, act, zf, p_: _oracle_render(H, W, NC, NI, p_, _p(coarse, dt), _p(fine, dt), table.to(dt), dt, True, None, act, zf)
    outs = {dt: run(dt, None, None, pose.to(dt))[0] for dt in (torch.float32, torch.float64)}
    for name, got in (("rgb", rgb), ("feat", feat), ("disp", disp), ("acc", acc)):
        B.three_way(tag, name, got, getattr(outs[torch.float32], name), getattr(outs[torch.float64], name))

    def oracle_run(dt, act, zf):
        c = pose.to(dt).requires_grad_()
        return {"d c2w": torch.autograd.grad(run(dt, act, zf, c)[1], c)[0]}

    assert torch.isfinite(gh).all() and float(gh.abs().max()) > 0
    B.pinned_gradients(tag, {"d c2w": gh}, tap, WD, oracle_run)


def test_train_step_c128_and_device_repack():
    """One train-mode step (test_time False) with a trainable table and trainable coarse + fine networks at C = 128, 7 x 9 = 63 rays,
    64 + 64 samples: every parameter gradient, the table gradient and d c2w against float64 autograd on the kernels' branches and
    depths; then an Adam step, after which the device re-pack of both networks is bit-identical to a host re-pack.
    Bounds: d c2w max(1e-4, 1.5 e_ref); the table gradient and every weight / bias gradient a flat 1e-4 of float64 autograd; maps
    three-way.  The ray grid was picked on the CPU so that the fp32 ORACLE's own ReLU branches are inside the branch audit's bound
    against float64 (2e-5, tests/branch.py "same_inputs"; 1.3e-5 here, 2.3e-5 at 8 x 8): asserted below on the two oracle runs."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    from nefes_amd import train as TR
    from nefes_amd.render import render
    C, NC, NI, H, W = 128, 64, 64, 7, 9
    coarse, fine = _net("coarse", C, True), _net("fine", C, True)
    grid = _grid(0, trainable=True)
    focal = FOCAL_AT_854 * W / 854.
    pose = O.se3_exp_pose(*POSE)
    c2w = pose.to(DEV).requires_grad_()
    pks = (coarse.packed(), fine.packed())
    ops.TIMERS = timers = {}
    try:
        with B.tapped() as tap:
            rgb, disp, acc, ex = render(H, W, focal, c2w=c2w, near=NEAR, far=FAR, **_render_kwargs(coarse, fine, grid, NC, NI, False))
            (O.bench_loss(rgb, ex["feat_map"]) + O.bench_loss(ex["rgb0"], ex["feat0"])).backward()
    finally:
        ops.TIMERS = None
    assert {"field_fwd_train[h3,ext]", "field_bwd_train[h3,ext]", "hashgrid_bwd_table"} <= set(timers), sorted(timers)
    names_c, names_f = TR.param_names(coarse, L.FIELD_STATIC), TR.param_names(fine, L.FIELD_FULL)
    sd_c, sd_f = dict(coarse.named_parameters()), dict(fine.named_parameters())
    hip = {"d table": grid.table.grad, "d c2w": c2w.grad}
    hip.update({"coarse " + n: sd_c[n].grad for n in names_c})
    hip.update({"fine " + n: sd_f[n].grad for n in names_f})
    assert all(v is not None and torch.isfinite(v).all() for v in hip.values())
    coarse_pin = B.Pinned(tap, WD, index=0)
    tag = "hashgrid_c128_train"

    def oracle_run(dt, act, zf):
        pc, pf = _oracle_params(coarse, names_c, dt), _oracle_params(fine, names_f, dt)
        tab = grid.table.detach().cpu().to(dt).requires_grad_()
        p_ = pose.detach().clone().to(dt).requires_grad_()
        seen = pres.setdefault(dt, [])

        def rec(tag, pre, row0):                                    # the fine pass's pre-activations of this precision
            seen.append((tag, pre.detach()))
            return act(tag, pre, row0)

        c, loss = _oracle_render(H, W, NC, NI, p_, pc, pf, tab, dt, False, coarse_pin.act(False), rec, zf)
        loss.backward()
        maps[dt] = c                                                # (the maps of the same two oracle runs: one per precision)
        out = {"d table": tab.grad, "d c2w": p_.grad}
        out.update({"coarse " + n: pc[n].grad for n in names_c})
        out.update({"fine " + n: pf[n].grad for n in names_f})
        return out

    maps, pres = {}, {}
    errs = B.pinned_gradients(tag, hip, tap, WD, oracle_run)
    # weight and table gradients: a flat 1e-4 of float64 autograd (d c2w keeps the shared rule applied above)
    worst = max(((n, e[0]) for n, e in errs.items() if n != "d c2w"), key=lambda t: t[1])
    P.record(tag, "worst weight / table gradient [branch-pinned, flat bound]", e_hip=worst[1], e_ref=None, bound=1e-4)
    assert worst[1] < 1e-4, worst
    # the fp32 oracle itself on these inputs: its ReLU branches against float64's (same branch pattern and depths upstream of each layer)
    o_flips, o_units, o_worst = 0, 0, 0.
    for (t64, p64), (t32, p32) in zip(pres[torch.float64], pres[torch.float32]):
        assert t64 == t32
        f = (p64 < 0) != (p32 < 0)
        o_units, o_flips = o_units + f.numel(), o_flips + int(f.sum())
        if f.any():
            o_worst = max(o_worst, float(p64[f].abs().max() / p64.abs().max()))
    print(f"[{tag}] fp32 oracle's own ReLU branches vs float64: {o_flips} of {o_units} units differ, worst {o_worst:.1e}")
    P.record(tag, "fp32 oracle: relu branch flips vs float64", flips=o_flips, units=o_units, worst_preact_rel=o_worst)
    assert o_worst < B.AUDIT_CLASSES["same_inputs"], (o_flips, o_units, o_worst)
    for name, got in (("rgb", rgb), ("feat", ex["feat_map"]), ("disp", disp), ("acc", acc)):
        B.three_way(tag, name, got.detach(), getattr(maps[torch.float32], name).detach(), getattr(maps[torch.float64], name).detach())
    # an optimizer step, then the device re-pack against the host packer
    params = [p for n, p in list(coarse.named_parameters()) + list(fine.named_parameters()) if not n.startswith(("fusion_net", "exposure_embedding"))]
    torch.optim.Adam(params, lr=5e-4).step()
    for net, pk in zip((coarse, fine), pks):
        blob0 = pk.blob.clone()
        assert net.packed() is pk and pk.generation == 1 and pk.h3_valid        # re-packed in place, on the device, fp16 streams included
        assert not torch.equal(pk.blob, blob0)
        host = ops.PackedField(dict(net.named_parameters()), net.W, net.W_features, net.encode_transient, DEV, pk.xyz_encoding)
        assert torch.equal(pk.blob, host.blob), int((pk.blob != host.blob).sum())
        assert len(pk.h3_byte_ranges()) == (10 if net is fine else 6)

"""Depth on the GPU: the depth-loss kernels (csrc/depth_loss.hip) and nefes_sample_px_nearest against tests/depth_ref.py,
render(depth_map=True) on every path against the oracle's Composite.depth, the factored head's fifth output and its g_depth, and
PoseRefiner(depth_weight=) in every form of the loop.  The CPU twins are tests/test_depth_ref.py and tests/test_depth_args.py."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from tests import branch as B
from tests import depth_ref as D
from tests import parity_log as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = lambda a: torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def ops():
    from nefes_amd import ops as _ops
    return _ops


# ---- the loss kernels -------------------------------------------------------------------------------------------------------------
DELTA, WEIGHT, G_LOSS = 0.07, 1.7, -0.75


def loss_case(G, P, seed):
    """disp, target [G, P] float32 with residuals of both signs on both sides of DELTA."""
    rng = np.random.default_rng(seed)
    target = rng.uniform(0.5, 3.5, (G, P)).astype(np.float32)
    e = rng.uniform(-3 * DELTA, 3 * DELTA, (G, P))
    return (1.0 / (target + e)).astype(np.float32), target


def run_kernels(ops, disp, target, mask=None, base=None):
    """-> (value float32, per-group float64 [G], g_disp float32 [G, P]) of ops.depth_loss at upstream gradient G_LOSS."""
    d = T(disp).to(DEV).requires_grad_()
    mk = None if mask is None else T(mask).to(DEV)
    out = None if base is None else torch.full((), float(base), device=DEV)
    loss, groups = ops.depth_loss(d, T(target).to(DEV), mk, delta=DELTA, weight=WEIGHT, out=out, accumulate=base is not None,
                                  return_groups=True)
    (g,) = torch.autograd.grad(loss, d, grad_outputs=torch.full((), G_LOSS, device=DEV))
    if out is not None:
        assert loss.data_ptr() == out.data_ptr()
    return loss.detach().cpu().numpy(), groups.cpu().numpy().copy(), g.cpu().numpy()


def check_case(ops, tag, disp, target, mask=None, base=None):
    """Value, per-group values and every gradient element within one float32 rounding of the float64 restatement (all per-pixel
    arithmetic of the kernels is double, each output rounded once: |got - ref| <= 2^-23 |ref|); invalid pixels' gradients == 0."""
    val, groups, grad = run_kernels(ops, disp, target, mask, base)
    rv, rg, rgrad = D.depth_loss(disp, target, mask, DELTA, WEIGHT, g_loss=G_LOSS, base=base)
    ev = abs(float(val) - rv) / max(abs(rv), 1e-300)
    eg = float(np.max(np.abs(grad - rgrad) / np.maximum(np.abs(rgrad), 1e-300)))
    print(f"[depth_loss {tag}] value {float(val):.9g} (float64 {rv:.17g}), relative error {ev:.2e}; worst gradient element {eg:.2e} (bound {2.0 ** -23:.2e})")
    assert D.within_one_ulp(val, rv), (tag, val, rv)
    np.testing.assert_allclose(groups, rg, rtol=1e-13, atol=0)             # (doubles: the summation order is all that differs)
    assert D.within_one_ulp(grad, rgrad), (tag, eg)
    inv = ~D.valid(disp, target, mask)
    assert not grad[inv].any() and np.all(grad[inv] == 0)
    return val, groups, grad


@pytest.mark.parametrize("P_", [1, 63, 64, 65, 255, 256, 257, 4800])
@pytest.mark.parametrize("G", [1, 3])
def test_depth_loss_kernels_match_float64(ops, G, P_):
    tag = f"G={G},P={P_}"
    disp, target = loss_case(G, P_, 100 * G + P_)
    e = 1.0 / disp.astype(np.float64) - target
    if P_ >= 63:                                                            # both branches of rho, both signs
        assert (np.abs(e) < DELTA).any() and (e > DELTA).any() and (e < -DELTA).any()
    check_case(ops, tag + " all valid", disp, target)
    # accumulate on top of a known value: what the buffer held, widened, plus the term, rounded once
    plain = check_case(ops, tag + " accumulate", disp, target, base=np.float32(0.3))
    # holes and bad disparities, spread over the row where it has room
    d2, t2 = disp.copy(), target.copy()
    idx = np.unique(np.linspace(0, P_ - 1, 9).astype(int))
    holes = [0.0, np.inf, np.nan, -1.0]
    bad_disp = [np.nan, 0.0, -0.3, np.inf]
    if P_ >= 63:
        for k in range(4):
            t2[0, idx[k]] = holes[k]
            d2[0, idx[4 + k]] = bad_disp[k]
    if G > 1:
        t2[1, :] = 0.0                                                      # a group without a valid pixel: value 0, gradient exactly 0
    val, groups, grad = check_case(ops, tag + " holes", d2, t2)
    if G > 1:
        assert groups[1] == 0 and not grad[1].any()
    # Inf / NaN at invalid pixels change no bit of the result
    t3, d3 = t2.copy(), d2.copy()
    inv = ~D.valid(d2, t2)
    t3[inv] = np.where(np.arange(inv.sum()) % 2 == 0, np.nan, -np.inf)
    val3, groups3, grad3 = run_kernels(ops, d3, t3)
    assert val3.tobytes() == val.tobytes() and groups3.tobytes() == groups.tobytes() and grad3.tobytes() == grad.tobytes()
    # a mask; an all-ones mask gives the bits of NULL
    mask = (np.random.default_rng(7 + P_).random((G, P_)) > 0.4).astype(np.uint8)
    if not mask.any():
        mask[0, 0] = 1
    check_case(ops, tag + " mask", d2, t2, mask)
    ones = run_kernels(ops, d2, t2, np.ones_like(mask))
    assert ones[0].tobytes() == val.tobytes() and ones[1].tobytes() == groups.tobytes() and ones[2].tobytes() == grad.tobytes()


def test_depth_loss_with_a_residual_of_exactly_delta(ops):
    disp = np.array([[0.5, 0.25, 0.5]], np.float32)
    target = np.array([[1.75, 4.25, 2.0]], np.float32)
    d = T(disp).to(DEV).requires_grad_()
    loss = ops.depth_loss(d, T(target).to(DEV), delta=0.25, weight=1.0)
    loss.backward()
    rv, _, rgrad = D.depth_loss(disp, target, None, 0.25, 1.0)
    assert D.within_one_ulp(loss.detach().cpu().numpy(), rv) and np.array_equal(d.grad.cpu().numpy(), rgrad.astype(np.float32))


# ---- nearest sampling -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 257])
@pytest.mark.parametrize("Cc", [1, 3])
def test_nearest_sampling(ops, Cc, n):
    H, W = 11, 13
    gen = torch.Generator().manual_seed(10 * Cc + n)
    m = torch.randn(Cc, H, W, generator=gen)
    m[:, 3:6, 4:9] = 0.0                                                    # a hole, as a depth frame has them
    grid = torch.stack([torch.randint(0, W, (n,), generator=gen), torch.randint(0, H, (n,), generator=gen)], -1).float()
    a = ops.sample_pixels(m.to(DEV), grid.to(DEV))
    b = ops.sample_pixels(m.to(DEV), grid.to(DEV), nearest=True)
    assert torch.equal(a, b) and torch.equal(b.cpu(), m[:, grid[:, 1].long(), grid[:, 0].long()])      # integer coordinates: bit for bit
    px = torch.rand(n, 2, generator=gen) * torch.tensor([W - 1., H - 1.])                                # sub-pixel
    special = torch.tensor([[2.5, 3.5], [-3.5, H + 2.25], [W - 0.5, -0.5], [0.49999997, 0.5], [W - 1.5, H - 1.5], [1e9, -1e9], [6.5, 0.0]])
    k = min(n, len(special))
    px[:k] = special[:k]                                                    # half-way and out-of-frame points
    got = ops.sample_pixels(m.to(DEV), px.to(DEV), nearest=True)
    assert got.shape == (Cc, n) and np.array_equal(got.cpu().numpy(), D.sample_nearest(m.numpy(), px.numpy()))
    out = torch.full((Cc, n), 7.0, device=DEV)
    assert ops.sample_pixels(m.to(DEV), px.to(DEV), out=out, nearest=True) is out and torch.equal(out, got)


# ---- render(depth_map=True) -------------------------------------------------------------------------------------------------------
def e2e_scene(g, tag):
    from tests.test_gpu_parity import _dropin, _kwargs, _modules
    Wd, C, Ni, tat, sscale, H, W, focal = g[f"{tag}.cfg"]
    R, M = _dropin()
    coarse, fine = _modules(int(Wd), int(C), float(sscale))
    kw = dict(_kwargs(M, coarse, fine, int(Ni), bool(tat)), N_samples=64)
    return R, kw, (int(Wd), int(C), int(Ni), bool(tat), float(sscale)), (int(H), int(W), float(focal))


def oracle_depth(g, tag, dt, cfgs, hwf, c2w=None, act=None, zf=None):
    """(disp, acc, depth) of the oracle's fine Composite on the fixture's scene: raw2outputs on the oracle's own fine-pass samples."""
    Wd, C, Ni, tat, sscale = cfgs
    pc, pf = O.make_field_params("coarse", Wd, C, dtype=dt), O.make_field_params("fine", Wd, C, dtype=dt)
    for p in (pc, pf):
        p["static_sigma.0.weight"] = p["static_sigma.0.weight"] * sscale
        p["static_sigma.0.bias"] = p["static_sigma.0.bias"] * sscale
    cfg = O.RenderCfg(N_samples=64, N_importance=Ni, transient_at_test=tat)
    dbg = {}
    c = T(g[f"{tag}.c2w"]).to(dt) if c2w is None else c2w
    O.render(*hwf, pc, pf, cfg, c2w=c, near=0., far=4., debug=dbg, fine_act=act, z_fine=zf)
    comp = O.composite(dbg["raw_fine"], dbg["z_fine"], cfg.raw_noise_std, output_transient=cfg.NeRFW, beta_min=0.1, white_bkgd=cfg.white_bkgd,
                       test_time=cfg.test_time, typ="fine", transient_at_test=cfg.transient_at_test)
    return comp.disp, comp.acc, comp.depth


@pytest.mark.parametrize("tag", ["metric", "metric_B", "ref_default", "ref_default_B"])
def test_render_depth_map(golden, tag, monkeypatch):
    """Variants A (transient_at_test) and B (static only), plain path (width 256) and factored head (width 128 / 128 channels): depth_map
    against the oracle's Composite.depth by the end-to-end test's bound on the maps (tests/parity_log.py NORTH_STAR_TOL, three-way);
    chunked = one chunk; render_poses = two renders; pixels= = the frame's rows; without the keyword nothing changes.  Every ray of
    these scenes hits something (tests/test_depth_ref.py checks the fixture on the CPU): none is excluded from a comparison."""
    import nefes_amd.render as NR
    from nefes_amd.render import render_poses
    g = golden("end_to_end")
    R, kw, cfgs, (H, W, focal) = e2e_scene(g, tag)
    pose = T(g[f"{tag}.c2w"]).to(DEV)
    hist = torch.full((1, 10), 10.)
    render = lambda c, **more: R.render(H, W, focal, chunk=32768, c2w=c, near=0., far=4., img_idx=hist, **dict(kw, **more))
    c_plain, c_depth = pose.clone().requires_grad_(), pose.clone().requires_grad_()
    plain = render(c_plain)
    with_d = render(c_depth, depth_map=True)
    assert "depth_map" not in plain[3] and with_d[3]["depth_map"].shape == (H * W,) and with_d[3]["depth_map"].grad_fn is not None
    O.bench_loss(plain[0], plain[3]["feat_map"]).backward()
    O.bench_loss(with_d[0], with_d[3]["feat_map"]).backward()
    for a, b in zip(plain[:3] + [plain[3]["feat_map"], c_plain.grad], with_d[:3] + [with_d[3]["feat_map"], c_depth.grad]):
        assert torch.equal(a, b)                                            # asking for the depth changes no other bit
    depth = with_d[3]["depth_map"].detach()
    d32, d64 = (oracle_depth(g, tag, dt, cfgs, (H, W, focal)) for dt in (torch.float32, torch.float64))
    assert bool(torch.isfinite(d64[0]).all()) and bool(torch.isfinite(with_d[1]).all())
    B.three_way(f"depth_map[{tag}]", "depth_map vs the oracle's Composite.depth", depth, d32[2], d64[2], tol=P.NORTH_STAR_TOL)
    B.three_way(f"depth_map[{tag}]", "1 / disp_map vs the oracle's 1 / disp", 1.0 / with_d[1].detach(), 1.0 / d32[0], 1.0 / d64[0], tol=P.NORTH_STAR_TOL)
    # render_poses with two poses = two renders
    other = O.se3_exp_pose((0.05, 0.15, -0.1), (0.2, 0.1, 0.25)).to(DEV)
    both = render_poses(H, W, focal, torch.stack([pose[:3, :4], other]), near=0., far=4., **dict(kw, depth_map=True))
    assert both[3]["depth_map"].shape == (2, H * W) and torch.equal(both[3]["depth_map"][0], depth)
    assert torch.equal(both[3]["depth_map"][1], render(other, depth_map=True)[3]["depth_map"])
    # render(pixels=subset) = the full render's rows
    rows = torch.tensor([0, 7, H * W - 1, 13, 13, 20])
    px = torch.stack([rows % W, rows // W], -1).float().to(DEV)
    sub = R.render(H, W, focal, chunk=32768, c2w=pose, near=0., far=4., img_idx=hist, pixels=px, **dict(kw, depth_map=True))
    assert torch.equal(sub[3]["depth_map"], depth[rows.to(DEV)])
    # render(row_range=) = those rows
    part = R.render(H, W, focal, chunk=32768, c2w=pose, near=0., far=4., img_idx=hist, row_range=(1, 2), **dict(kw, depth_map=True))
    assert torch.equal(part[3]["depth_map"], depth[W:3 * W])
    # chunked: 20 rays per launch sequence over the frame's rays = one chunk, bit for bit (and the plan counts the map's 4 bytes)
    cfg = NR._cfg(dict(kw, depth_map=True))
    NR.rays_per_launch(cfg, kw["network_fn"], kw["network_fine"], torch.device(DEV))
    per_ray = {k: v for k, v in NR._PER_RAY.items() if k[:2] == (cfgs[0], cfgs[1])}
    with_key = [v for k, v in per_ray.items() if k[-1] is True and len(k) == 8]
    without = [v for k, v in per_ray.items() if len(k) == 7 and k[4] is False]
    assert with_key and without and with_key[0] == without[0] + 4
    monkeypatch.setattr(NR, "rays_per_launch", lambda *a, **k: 20)
    monkeypatch.setattr(NR, "_clamp_to_free_memory", lambda step, *a, **k: step)
    chunked = render(pose, depth_map=True)
    assert chunked[3]["depth_map"].shape == (H * W,) and torch.equal(chunked[3]["depth_map"], depth) and torch.equal(chunked[0], plain[0])


def test_render_sharded_hands_the_keyword_through(golden):
    from nefes_amd import dist
    g = golden("end_to_end")
    R, kw, _, (H, W, focal) = e2e_scene(g, "metric_B")
    pose = T(g["metric_B.c2w"]).to(DEV)
    full = R.render(H, W, focal, c2w=pose, near=0., far=4., **dict(kw, depth_map=True))[3]["depth_map"]
    parts = [dist.render_sharded(R.render, H, W, focal, pose, rank=r, world=H + 1, near=0., far=4., **dict(kw, depth_map=True)) for r in range(H + 1)]
    assert torch.equal(torch.cat([p[3]["depth_map"] for p in parts]), full)
    empty = [p for p in parts if p[0].shape[0] == 0]
    assert empty and all(p[3]["depth_map"].shape == (0,) for p in empty)
    none = dist.render_sharded(R.render, H, W, focal, pose, rank=H, world=H + 1, near=0., far=4., **kw)
    assert "depth_map" not in none[3]


# ---- the factored head ------------------------------------------------------------------------------------------------------------
FH_VS_PLAIN = 2e-6         # tests/test_gpu_fh.py: the maps of the factored head against the plain kernels (its bound on disp and acc)


def test_factored_head_depth_map_and_its_pose_gradient():
    """The width-128 / 128-channel frozen network of tests/test_gpu_fh.py.  depth_map with the factored head on against off within
    that file's FH-vs-plain bound; the pose gradient of L = sum_i c_i depth_map_i (fixed random c) is not zero and, on the kernels' own
    ReLU branches and depths (tests/branch.py), within max(1e-4, 1.5 x the fp32 oracle's own distance) of the float64 oracle -- on both
    head paths.  Before depth_map existed the factored-head node dropped the compositor's depth and passed no g_depth."""
    from nefes_amd import ops
    from tests.test_gpu_surface import dropin, kwargs, nets, params
    R, M, _ = dropin()
    Wd, C, Ni = 128, 128, 64
    coarse, fine = nets(Wd, C)
    kw = dict(kwargs(M, coarse, fine, Ni, tat=True), use_viewdirs=True, ndc=False, depth_map=True)
    H, W, focal = 6, 8, 7.0
    pose = O.bench_pose()
    coef = torch.randn(H * W, generator=torch.Generator().manual_seed(21))
    assert fine.factored_head_ok()
    cfg = O.RenderCfg(N_samples=64, N_importance=Ni)
    cfg.transient_at_test = True

    def oracle_run(dt, act, zf):
        c = pose.to(dt).requires_grad_()
        dbg = {}
        O.render(H, W, focal, *params(Wd, C, dt), cfg, c2w=c, near=0., far=4., debug=dbg, fine_act=act, z_fine=zf)
        comp = O.composite(dbg["raw_fine"], dbg["z_fine"], cfg.raw_noise_std, output_transient=cfg.NeRFW, beta_min=0.1,
                           white_bkgd=cfg.white_bkgd, test_time=cfg.test_time, typ="fine", transient_at_test=cfg.transient_at_test)
        return {"d c2w of sum c depth_map": torch.autograd.grad((comp.depth * coef.to(dt)).sum(), c)[0]}
    outs = {}
    for fh in (True, False):
        ops.FACTORED_HEAD = fh
        ops.TIMERS = timers = {}
        try:
            c2w = pose.to(DEV).requires_grad_()
            with B.tapped() as tap:
                rgb, disp, acc, ex = R.render(H, W, focal, c2w=c2w, near=0., far=4., **kw)
            (gd,) = torch.autograd.grad((ex["depth_map"] * coef.to(DEV)).sum(), c2w)
        finally:
            ops.FACTORED_HEAD = True
            ops.TIMERS = None
        assert ("field_fwd[full,h3,fh]" in timers) == fh, sorted(timers)
        assert float(gd.abs().max()) > 0
        outs[fh] = (ex["depth_map"].detach(), gd)
        B.pinned_gradients(f"depth_map_fh[fh={int(fh)}]", {"d c2w of sum c depth_map": gd}, tap, Wd, oracle_run)
    e = B.rel(outs[True][0], outs[False][0])
    P.record("depth_map_fh", "depth_map: factored head vs plain kernels", direct=e, bound=FH_VS_PLAIN)
    print(f"[depth_map_fh] depth_map, factored head vs plain kernels: {e:.2e}; d c2w {B.rel(outs[True][1], outs[False][1]):.2e}")
    assert e < FH_VS_PLAIN, e


def test_factored_head_node_without_want_depth_is_unchanged():
    """Four outputs, the same bits and ray gradients as the five-output node's first four; the fifth output's gradient reaches the rays."""
    from nefes_amd import lib as L
    from nefes_amd import ops
    from tests.test_gpu_surface import nets
    _, fine = nets(128, 128)
    pk, w_f, w_f_t, b_f = fine.packed_fh()
    g = torch.Generator().manual_seed(9)
    N, S = 53, 128
    o = (torch.randn(N, 3, generator=g) * 0.3).to(DEV)
    d = torch.nn.functional.normalize(torch.randn(N, 3, generator=g), dim=-1).to(DEV)
    z = torch.sort(torch.rand(N, S, generator=g) * 4, -1)[0].to(DEV)
    G_rgb, G_feat = torch.randn(N, 3, generator=g).to(DEV), torch.randn(N, 128, generator=g).to(DEV)
    G_dep = torch.randn(N, generator=g).to(DEV)
    res = []
    for want in (None, False, True):
        oo, dd, vv = (t.clone().requires_grad_() for t in (o, d, d))
        outs = ops.RenderFineFH.apply(oo, dd, vv, z, pk, w_f, w_f_t, b_f, L.COMP_TRANSIENT, 0.1, *(() if want is None else (False, want)))
        assert len(outs) == (5 if want else 4)
        ((outs[0] * G_rgb).sum() + (outs[1] * G_feat).sum()).backward(retain_graph=True)
        res.append([t.detach() for t in outs[:4]] + [oo.grad.clone(), dd.grad.clone(), vv.grad.clone()])
        if want:
            raw = ops.FieldFromRaysFH.apply(oo, dd, vv, z, pk)
            chain = ops.Composite.apply(raw, z, 65, L.COMP_TRANSIENT, 0.1)
            assert torch.equal(outs[4], chain[4])                           # the compositor's own depth
            gs = torch.autograd.grad((outs[4] * G_dep).sum(), [oo, dd])
            gc = torch.autograd.grad((chain[4] * G_dep).sum(), [oo, dd])
            assert all(float(a.abs().max()) > 0 for a in gs)
            for a, b_, name in zip(gs, gc, ("d rays_o", "d rays_d")):
                err = B.rel(a, b_)
                P.record("factored_head_depth_node", f"{name} of sum c depth: one node vs the three-node chain", direct=err, bound=FH_VS_PLAIN)
                assert err < FH_VS_PLAIN, (name, err)
    for r in res[1:]:
        assert all(torch.equal(a, b_) for a, b_ in zip(r, res[0]))


# ---- PoseRefiner(depth_weight=) ---------------------------------------------------------------------------------------------------
LAMBDA, HUBER = 0.5, 0.05


def depth_frame(g, refiner_of):
    """The scene's own 1 / disp_map at the true pose [h, w], with a 10 x 10 block of zeros (sensor holes)."""
    from nefes_amd.render import render
    probe = refiner_of(g, False)
    with torch.no_grad():
        probe._reset(T(g["true_c2w"]).to(DEV), T(g["target"]).to(DEV), T(g["hist"]).to(DEV))
        c2w = probe._composed_pose()
        _, disp, _, _ = render(probe.h, probe.w, probe.focal, c2w=c2w.reshape(3, 4), near=probe.near, far=probe.far, img_idx=probe.hist, **probe.kw)
    frame = (1.0 / disp).reshape(probe.h, probe.w).clone()
    frame[1:11, 3:13] = 0.0
    return frame


def state(r):
    return torch.cat([r.model.r.grad.reshape(-1), r.model.t.grad.reshape(-1)]).clone()


@pytest.mark.parametrize("per_pixel", [False, True])
@pytest.mark.parametrize("sparse", [None, 40])
def test_refiner_iteration_is_the_chain_called_by_hand(golden, ops, sparse, per_pixel):
    """refiner.loss and the (r, t) gradient are torch.equal to: the refiner's own feature term (whose kernel leaves its value in the
    loss buffer), then ops.depth_loss(disp_map, depth, weight=lambda, out=that buffer, accumulate=True), the two differentiated together;
    refiner.depth_loss is the term alone (lambda not applied); the total is one rounding of feature + lambda * term."""
    from tests.test_gpu_intrinsics import refiner
    g = golden("refine")
    frame = depth_frame(g, refiner)
    more = dict(depth_weight=LAMBDA, depth_huber=HUBER, per_pixel=per_pixel, **({} if sparse is None else dict(sparse=sparse)))
    init, target, hist = T(g["init_c2w"]).to(DEV), T(g["target"]).to(DEV), T(g["hist"]).to(DEV)
    px = None
    if sparse is not None:
        gen = torch.Generator().manual_seed(5)
        px = (torch.rand(sparse, 2, generator=gen) * torch.tensor([15., 11.])).to(DEV)       # sub-pixel points of the 12 x 16 frame
        px[:8] = px[:8].round()
        px[0], px[1] = torch.tensor([5., 4.], device=DEV), torch.tensor([12.4, 9.6], device=DEV)         # inside the block of holes
    r = refiner(g, False, **more)
    r._reset(init, target, hist, None, px, frame)
    total = r.loss_and_grad().clone()
    grads, term = state(r), r.depth_loss.clone()
    # by hand
    h = refiner(g, False, **more)
    h._reset(init, target, hist, None, px, frame)
    depth_target = frame.reshape(1, -1) if sparse is None else ops.sample_pixels(frame[None], px, nearest=True)
    assert torch.equal(h.depth_target, depth_target)
    if sparse is not None:
        assert np.array_equal(depth_target.cpu().numpy(), D.sample_nearest(frame[None].cpu().numpy(), px.cpu().numpy()))
        assert float(depth_target[0, 0]) == 0 and float(depth_target[0, 1]) == 0 and int((depth_target > 0).sum()) > 8
    feat_loss, _ = h._feature_term()
    assert feat_loss.data_ptr() == h.loss.data_ptr()
    feat_value = h.loss.clone()
    disp = h._disp.reshape(1, -1)
    alone, groups = ops.depth_loss(disp.detach(), depth_target, delta=HUBER, weight=1.0, return_groups=True)
    by_hand = ops.depth_loss(disp, depth_target, delta=HUBER, weight=LAMBDA, out=h.loss, accumulate=True)
    one = torch.ones((), device=DEV)
    torch.autograd.grad([feat_loss, by_hand], [h.model.r, h.model.t], grad_outputs=[one, one])
    assert torch.equal(total, h.loss) and torch.equal(grads, state(h))
    assert torch.equal(term, groups.reshape(())) and float(term) > 0
    rv, rg, _ = D.depth_loss(disp.detach().cpu().numpy(), depth_target.cpu().numpy(), None, HUBER, LAMBDA, base=feat_value.cpu().numpy())
    assert D.within_one_ulp(total.cpu().numpy(), rv) and abs(float(term) - rg[0]) <= 1e-13 * rg[0]
    assert D.within_one_ulp(alone.cpu().numpy(), rg[0])
    print(f"[refiner_depth sparse={sparse} per_pixel={per_pixel}] feature {float(feat_value):.6f} + {LAMBDA} x depth {float(term):.6f} = {float(total):.6f}")
    # the depth term moves the gradient: a refiner without it walks elsewhere
    plain = refiner(g, False, per_pixel=per_pixel, **({} if sparse is None else dict(sparse=sparse)))
    plain._reset(init, target, hist, None, px)
    assert torch.equal(plain.loss_and_grad(), feat_value) and not torch.equal(state(plain), grads)


@pytest.mark.parametrize("sparse", [None, 40])
def test_refiner_graph_equals_eager(golden, sparse):
    from tests.test_gpu_intrinsics import job, refiner
    g = golden("refine")
    frame = depth_frame(g, refiner)
    more = dict(depth_weight=LAMBDA, depth_huber=HUBER, **({} if sparse is None else dict(sparse=sparse, seed=3)))
    res = []
    for graph in (False, True):
        r = refiner(g, graph, **more)
        pose, losses = r.refine(*job(g), 5, depth=frame)
        assert (r.graph is not None) == graph
        res.append((pose.clone(), losses.clone(), r.depth_loss.clone(), r.loss.clone()))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert torch.equal(res[1][1][-1], res[1][3]) and float(res[1][2]) > 0
    # the captured refiner takes the next image's depth in place: the same image again gives the same trajectory, another frame another
    same_px = {} if sparse is None else dict(pixels=r.pixels.clone())        # (a sparse refiner would draw the next image's pixels)
    again = r.refine(*job(g), 5, depth=frame, **same_px)
    assert torch.equal(again[0], res[1][0]) and torch.equal(again[1], res[1][1])
    shifted = torch.where(frame > 0, frame + 0.2, frame)
    assert not torch.equal(r.refine(*job(g), 5, depth=shifted, **same_px)[1], res[1][1])


def test_refiner_batch_of_two_walks_the_solo_trajectories(golden):
    """images=2, one group per image: each image's total is its own.  The batched convolutions are another fp32 rounding of the loop, so
    the rule is the one the suite holds a batch to against its images alone (tests/test_gpu_refine_masked.py: losses within 2e-4 over
    four iterations, poses within 2e-3) -- and the two depth frames are not interchangeable at that tolerance."""
    from tests.test_gpu_intrinsics import refiner
    g = golden("refine")
    frame = depth_frame(g, refiner)
    n = 4
    init, target, hist = T(g["init_c2w"]), T(g["target"]), T(g["hist"])
    inits = torch.stack([init, T(g["true_c2w"])])
    frames = torch.stack([frame, torch.where(frame > 0, frame + 0.3, frame).roll(3, 1)])
    mk = lambda images: refiner(g, True, depth_weight=LAMBDA, depth_huber=HUBER, images=images)
    single, batch = mk(1), mk(2)
    alone = [[t.clone() for t in single.refine(inits[b], target, hist, n, depth=frames[b])] + [single.depth_loss.clone()] for b in range(2)]
    swapped = single.refine(inits[0], target, hist, n, depth=frames[1])[1].clone()
    poses, losses = batch.refine(inits, torch.stack([target, target]), hist.repeat(2, 1), n, depth=frames)
    assert poses.shape == (2, 4, 4) and losses.shape == (n, 2) and batch.depth_loss.shape == (2,)
    for b in range(2):
        p1, l1, t1 = alone[b]
        e_l, e_p = B.rel(losses[:, b], l1), float((poses[b] - p1).abs().max())
        P.record("refiner_depth_batch", f"image {b}: losses / poses, batch of two vs alone", direct=e_l, e_ref=e_p, bound=2e-4)
        assert e_l < 2e-4 and e_p < 2e-3, (b, e_l, e_p)
        assert abs(float(batch.depth_loss[b]) - float(t1)) <= 2e-4 * max(float(t1), 1e-3)
    assert B.rel(losses[:, 0], swapped) > 2e-3


def test_redrawn_refiner_resamples_the_depth_inside_the_captured_iteration(golden, ops):
    """sparse=40, redraw=2: after a redraw the replayed depth term is the eager term of a fresh refiner at the NEW pixels (same state),
    and not the first draw's."""
    from tests.test_gpu_intrinsics import job, refiner
    g = golden("refine")
    frame = depth_frame(g, refiner)
    more = dict(depth_weight=LAMBDA, depth_huber=HUBER, sparse=40)
    r = refiner(g, True, redraw=2, seed=11, **more)
    r.refine(*job(g), 0, depth=frame)                                       # state, capture, state again; no iteration yet
    assert r.graph is not None
    seen = []
    for i in range(3):                                                      # iterations 0, 1 share a draw; iteration 2 redraws
        before = (r.model.r.detach().clone(), r.model.t.detach().clone())
        r.replay()
        seen.append((r.pixels.clone(), r.depth_target.clone(), r.depth_loss.clone(), r.loss.clone(), before))
    assert torch.equal(seen[0][0], seen[1][0]) and not torch.equal(seen[1][0], seen[2][0])
    for px, dt, term, total, (r0, t0) in (seen[0], seen[2]):
        assert torch.equal(dt, ops.sample_pixels(frame[None], px, nearest=True))
        fresh = refiner(g, False, **more)
        fresh._reset(*job(g), None, px, frame)
        with torch.no_grad():
            fresh.model.r.copy_(r0)
            fresh.model.t.copy_(t0)
        assert torch.equal(fresh.loss_and_grad(), total) and torch.equal(fresh.depth_loss, term)
    first_pixels = refiner(g, False, **more)
    first_pixels._reset(*job(g), None, seen[0][0], frame)
    with torch.no_grad():
        first_pixels.model.r.copy_(seen[2][4][0])
        first_pixels.model.t.copy_(seen[2][4][1])
    first_pixels.loss_and_grad()
    assert not torch.equal(first_pixels.depth_loss, seen[2][2])


def test_descent_with_the_depth_term(golden):
    """From the fixture's start, 20 iterations, sparse with 96 points and the depth term on: the total ends below where it began."""
    from tests.test_gpu_intrinsics import job, refiner
    g = golden("refine")
    frame = depth_frame(g, refiner)
    r = refiner(g, True, depth_weight=LAMBDA, depth_huber=HUBER, sparse=96, seed=1)
    pose, losses = r.refine(*job(g), 20, depth=frame)
    first, last = float(losses[0]), float(losses[-1])
    true = T(g["true_c2w"]).to(DEV)
    err0, err1 = float((T(g["init_c2w"]).to(DEV)[:3, 3] - true[:3, 3]).norm()), float((pose[:3, 3] - true[:3, 3]).norm())
    print(f"[depth_descent] total loss {first:.6f} -> {last:.6f} over 20 iterations (depth term at the end {float(r.depth_loss):.6f}); "
          f"translation error {err0:.4f} -> {err1:.4f}")
    P.record("depth_descent", "total loss: first, last (sparse=96, 20 iterations)", direct=first, e_ref=last, bound=None)
    P.record("depth_descent", "translation error: start, end", direct=err0, e_ref=err1, bound=None)
    assert last < first

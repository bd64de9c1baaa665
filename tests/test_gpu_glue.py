"""The small kernels between the large ones, each against a plain float64 statement of the same operation (tests/glue_ref.py), per
element, at the smallest shapes that take every path of the kernel: csrc/refine.hip fusion_input / feat_head / adam and csrc/rays.hip
ray_grad_reduce / coarse_depths / ndc / raygen_bwd.  The inputs, the bounds and where they come from are in tests/glue_ref.py;
tests/test_glue_ref.py checks them on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from tests import glue_ref as R
from tests import parity_log as P

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ops():
    from nefes_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def L():
    from nefes_amd import lib as _L
    _L.load()
    return _L


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- fusion_input ------------------------------------------------------------------------------------------------------------------
def run_fusion(ops, case, shape, affine, need=(True, True), images=None):
    """-> (x, g_rgb or None, g_feat or None) on the GPU; `images` = a slice of the batch to run alone."""
    B, H, W, Cf = shape
    sl = slice(0, B) if images is None else images
    px = slice(sl.start * H * W, sl.stop * H * W)
    rgb, feat = case["rgb"][px].to(DEV).requires_grad_(need[0]), case["feat"][px].to(DEV).requires_grad_(need[1])
    x = ops.fusion_input(rgb, feat, None if affine is None else affine[sl].contiguous().to(DEV), sl.stop - sl.start, H, W, R.MEAN, R.STD)
    x.backward(case["g_x"][sl].to(DEV))
    return x.detach(), rgb.grad, feat.grad


@pytest.mark.parametrize("with_affine", [False, True], ids=["plain", "affine"])
@pytest.mark.parametrize("shape", R.FUSION_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fusion_input(ops, shape, with_affine):
    B, H, W, Cf = shape
    case = R.fusion_case(*shape)
    affine = case["affine"] if with_affine else None
    tag = f"fusion_input[{B}x{H}x{W}x{Cf},{'affine' if with_affine else 'plain'}]"
    x64, g64 = R.fusion_eval(case, shape, with_affine, torch.float64)
    x32, g32 = R.fusion_eval(case, shape, with_affine, torch.float32)
    feat_t = case["feat"].reshape(B, H * W, Cf).permute(0, 2, 1).reshape(B, Cf, H, W)
    g_feat_want = case["g_x"][:, 3:].reshape(B, Cf, H * W).permute(0, 2, 1).reshape(B * H * W, Cf)
    runs = {need: run_fusion(ops, case, shape, affine, need) for need in ((True, True), (True, False), (False, True))}
    for need, (x, g_rgb, g_feat) in runs.items():
        what = {(True, True): "both", (True, False): "rgb only", (False, True): "feat only"}[need]
        assert x.shape == (B, 3 + Cf, H, W)
        assert torch.equal(x[:, 3:].cpu(), feat_t), (tag, what)                                  # pure copies
        P.check(tag, f"x colours ({what})", R.rel_max(x[:, :3], x64), R.rel_max(x32, x64), R.rel_max(x[:, :3], x32), tol=R.TOL_FP32)
        assert (g_rgb is not None) == need[0] and (g_feat is not None) == need[1]
        if need[1]:
            assert torch.equal(g_feat.cpu(), g_feat_want), (tag, what)
        if need[0]:
            P.check(tag, f"g_rgb ({what})", R.rel_max(g_rgb, g64), R.rel_max(g32, g64), R.rel_max(g_rgb, g32), tol=R.TOL_FP32)
    # the three backward forms agree bit for bit where they overlap
    assert torch.equal(runs[(True, True)][1], runs[(True, False)][1]) and torch.equal(runs[(True, True)][2], runs[(False, True)][2])
    # image b of the batch is the image run alone with its own affine
    x, g_rgb, g_feat = runs[(True, True)]
    for b in range(B if B > 1 else 0):
        xa, ra, fa = run_fusion(ops, case, shape, affine, images=slice(b, b + 1))
        px = slice(b * H * W, (b + 1) * H * W)
        assert torch.equal(xa[0], x[b]) and torch.equal(ra, g_rgb[px]) and torch.equal(fa, g_feat[px]), (tag, b)


# ---- feat_head ---------------------------------------------------------------------------------------------------------------------
def run_head(ops, case, rows=None):
    sl = slice(None) if rows is None else rows
    w, b = case["w"].to(DEV), case["b"].to(DEV)
    gmap = case["gmap"][sl].contiguous().to(DEV).requires_grad_()
    feat = ops.FeatHead.apply(gmap, w, w.t().contiguous(), b)
    feat.backward(case["g_feat"][sl].contiguous().to(DEV))
    return feat.detach(), gmap.grad


@pytest.mark.parametrize("shape", R.HEAD_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_feat_head(ops, shape):
    N, Cc, F = shape
    case = R.head_case(*shape)
    d = {k: v.double() for k, v in case.items()}
    b_fwd, b_bwd = R.head_bounds(case)
    feat, g_gmap = run_head(ops, case)
    assert feat.shape == (N, Cc) and g_gmap.shape == (N, F + 1)
    r_f = R.ratio(feat, R.feat_head(d["gmap"], d["w"], d["b"]), b_fwd)
    r_b = R.ratio(g_gmap, R.feat_head_bwd(d["g_feat"], d["w"], d["b"]), b_bwd)
    tag = f"feat_head[{N}x{Cc}x{F}]"
    P.record(tag, "forward / ((F+2) u sum|terms|)", ratio=r_f, bound=1.0)
    P.record(tag, "backward / ((C+1) u sum|terms|)", ratio=r_b, bound=1.0)
    print(f"{tag}: error / bound forward {r_f:.3f}, backward {r_b:.3f}")
    assert r_f <= 1 and r_b <= 1, (tag, r_f, r_b)
    # a ray's result does not depend on which other rays are in the batch
    for i in range(N):
        f1, g1 = run_head(ops, case, slice(i, i + 1))
        assert torch.equal(f1[0], feat[i]) and torch.equal(g1[0], g_gmap[i]), (tag, i)
    if N > 2:
        rows = torch.arange(N - 1, 0, -2)
        f2, g2 = run_head(ops, case, rows)
        assert torch.equal(f2, feat[rows.to(DEV)]) and torch.equal(g2, g_gmap[rows.to(DEV)]), tag


@pytest.mark.parametrize("N,Cc,F", [(2, 257, 16), (2, 16, 256), (2, 16, 0), (0, 16, 16)])
def test_feat_head_refuses(L, N, Cc, F):
    """Outside the ABI's range (C <= 256, 0 < F < 256, N > 0) both entries answer with a bad argument, on buffers large enough for any."""
    buf = [torch.zeros(4 * 300 * 300, device=DEV) for _ in range(4)]
    with pytest.raises(RuntimeError, match="bad argument"):
        L.check(L.load().nefes_feat_head_fwd(N, Cc, F, *map(ptr, buf), stream()), "nefes_feat_head_fwd")
    with pytest.raises(RuntimeError, match="bad argument"):
        L.check(L.load().nefes_feat_head_bwd(N, Cc, F, *map(ptr, buf), stream()), "nefes_feat_head_bwd")
    torch.cuda.synchronize()


# ---- FusedAdam ---------------------------------------------------------------------------------------------------------------------
def make_adam(ops, n):
    case = R.adam_case(n)
    params = [t.to(DEV).requires_grad_() for t in R.split(case["p0"], n)]
    return ops.FusedAdam(list(zip(params, R.adam_lrs(n)))), params


def adam_run(opt, grads, steps, snap=()):
    out = {}
    for t in range(1, steps + 1):
        opt.grad.copy_(grads[t - 1])
        opt.step()
        if t in snap:
            out[t] = (opt.flat.clone(), opt.m.clone(), opt.v.clone())
    return out


@pytest.mark.parametrize("n", list(R.ADAM_SIZES))
def test_fused_adam(ops, n):
    case, truth, ref32 = R.adam_case(n), R.adam_truth(n), R.torch_adam(n, torch.float32)
    grads = case["grads"].to(DEV)
    opt, params = make_adam(ops, n)
    assert torch.equal(opt.lr.cpu(), case["lr"]) and torch.equal(opt.flat.cpu(), case["p0"])
    got = adam_run(opt, grads, R.ADAM_STEPS, R.ADAM_CHECK)
    assert float(opt.step_t) == R.ADAM_STEPS
    assert torch.equal(torch.cat([p.detach().reshape(-1) for p in params]), opt.flat)            # the parameters are views of the flat buffer
    for t in R.ADAM_CHECK:
        for name, a, b32, b64 in zip("pmv", got[t], ref32[t], truth[t]):
            P.check(f"fused_adam[n={n}]", f"{name} after step {t}", R.rel_elem(a, b64), R.rel_elem(b32, b64), R.rel_elem(a, b32), tol=R.TOL_FP32)
    if n >= 3:
        assert torch.equal(opt.flat[R.ADAM_ZERO].cpu(), case["p0"][R.ADAM_ZERO])         # zero gradient: 0 / eps, the element never moves
    # zero_state + the same parameters + the same gradients = the same trajectory, bit for bit
    p_end = opt.flat.clone()
    opt.zero_state()
    assert float(opt.step_t) == 0 and not bool(opt.m.any()) and not bool(opt.v.any()) and not bool(opt.grad.any())
    opt.flat.copy_(case["p0"])
    again = adam_run(opt, grads, R.ADAM_STEPS, (1, R.ADAM_STEPS))
    assert torch.equal(again[1][0], got[1][0]) and torch.equal(again[R.ADAM_STEPS][0], p_end)
    assert float(opt.step_t) == R.ADAM_STEPS


def test_fused_adam_replays_equal_eager_steps(ops):
    """K replays of one captured step = K eager steps, with the gradients refreshed in place and one learning rate changed in place on the
    device between replays: the step counter, the learning rates and the gradients are all read from device memory when the kernel runs."""
    n, K = 7, 6
    case = R.adam_case(n)
    grads = case["grads"].to(DEV)

    def between(opt, t):
        opt.grad.copy_(grads[t])
        if t == 3:
            opt.lr[4:5].fill_(3e-3)

    eager, _ = make_adam(ops, n)
    for t in range(K):
        between(eager, t)
        eager.step()
    opt, _ = make_adam(ops, n)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up outside the capture, then back to the start
        opt.step()
    torch.cuda.current_stream().wait_stream(side)
    opt.zero_state()
    opt.flat.copy_(case["p0"])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    for t in range(K):
        between(opt, t)
        graph.replay()
    torch.cuda.synchronize()
    assert float(opt.step_t) == K == float(eager.step_t)
    assert not torch.equal(opt.flat.cpu(), case["p0"])
    for a, b in ((opt.flat, eager.flat), (opt.m, eager.m), (opt.v, eager.v)):
        assert torch.equal(a, b)


def test_fused_adam_refuses_1025(ops):
    opt = ops.FusedAdam([(torch.zeros(1000, device=DEV, requires_grad=True), 1e-3), (torch.zeros(25, device=DEV, requires_grad=True), 1e-4)])
    with pytest.raises(RuntimeError, match="bad argument"):
        opt.step()
    torch.cuda.synchronize()
    assert float(opt.step_t) == 0


# ---- ray_grad_reduce ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_vs", [True, False], ids=["g_vs", "no_g_vs"])
@pytest.mark.parametrize("N,S", R.REDUCE_SHAPES)
def test_ray_grad_reduce(ops, N, S, with_vs):
    case = R.reduce_case(N, S)
    z, g_pts, g_vs = case["z"], case["g_pts"], case["g_vs"] if with_vs else None
    ref = R.ray_reduce(z.double(), g_pts.double(), None if g_vs is None else g_vs.double())
    dev = lambda t, sl=slice(None): None if t is None else t[sl].contiguous().to(DEV)
    got = ops.ray_grad_reduce(N, S, dev(z), dev(g_pts), dev(g_vs))
    tag = f"ray_grad_reduce[{N}x{S},{'g_vs' if with_vs else 'no g_vs'}]"
    ratios = {}
    for name, a, s, mag, k in zip(("g_o", "g_d", "g_v"), got, ref[:3], ref[3:], (2, 3, 2)):
        assert a.shape == (N, 3)
        ratios[name] = R.ratio(a, s, k * R.U * mag)
        P.record(tag, f"{name} / ({k} u sum|terms|)", ratio=ratios[name], bound=1.0)
    print(f"{tag}: error / bound {ratios}")
    assert all(r <= 1 for r in ratios.values()), (tag, ratios)
    if not with_vs:
        assert torch.equal(got[2].cpu(), torch.zeros(N, 3))
    for i in range(N):                                                                  # rows do not depend on the batch
        one = ops.ray_grad_reduce(1, S, dev(z, slice(i, i + 1)), dev(g_pts, slice(i, i + 1)), dev(g_vs, slice(i, i + 1)))
        assert all(torch.equal(a[0], b[i]) for a, b in zip(one, got)), (tag, i)


# ---- coarse depths -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("jitter", [False, True], ids=["det", "jitter"])
@pytest.mark.parametrize("lindisp", [False, True], ids=["lin", "lindisp"])
@pytest.mark.parametrize("Nc", R.DEPTH_NC)
def test_coarse_depths(ops, Nc, lindisp, jitter):
    case = R.depth_case(Nc)
    N = R.DEPTH_N
    batch = case["batch"].to(DEV)
    t_rand = case["t_rand"].to(DEV) if jitter else None
    for per_ray in (False, True):
        z64, _, _ = R.depth_ref(Nc, lindisp, jitter, per_ray, torch.float64)
        z32, near, far = R.depth_ref(Nc, lindisp, jitter, per_ray, torch.float32)
        if per_ray:
            bounds = batch[:, 6:8]
            assert bounds.stride(0) == 21
            z = ops.coarse_depths(N, Nc, -1., -1., lindisp, t_rand, device=DEV, bounds=bounds)
        else:
            z = ops.coarse_depths(N, Nc, R.DEPTH_NEAR, R.DEPTH_FAR, lindisp, t_rand, device=DEV)
            const = torch.tensor([R.DEPTH_NEAR, R.DEPTH_FAR, -7.0], device=DEV).repeat(N, 1)          # row stride 3
            assert torch.equal(ops.coarse_depths(N, Nc, -1., -1., lindisp, t_rand, device=DEV, bounds=const[:, :2]), z)
        assert z.shape == (N, Nc)
        tag = f"coarse_depths[Nc={Nc},{'lindisp' if lindisp else 'lin'},{'jitter' if jitter else 'det'},{'per ray' if per_ray else 'scalar'}]"
        P.check(tag, "z per element", R.rel_elem(z, z64), R.rel_elem(z32, z64), R.rel_elem(z, z32), tol=R.TOL_DEPTH)
        if not lindisp and not jitter:
            assert np.array_equal(z.cpu().numpy(), z32.numpy()), tag
        assert R.depth_rows_ok(z.cpu(), near, far), tag


# ---- NDC ---------------------------------------------------------------------------------------------------------------------------
def ndc_library(L, geom, o, d, g_oo, g_od):
    """The library entries with the call form of ops.NdcRays (forward, then backward with either upstream possibly null)."""
    H, W, focal, near = geom
    n = o.shape[0]
    oo, od, go, gd = (torch.empty_like(o) for _ in range(4))
    L.check(L.load().nefes_ndc_fwd(H, W, float(focal), float(near), n, ptr(o), ptr(d), ptr(oo), ptr(od), stream()), "nefes_ndc_fwd")
    L.check(L.load().nefes_ndc_bwd(H, W, float(focal), float(near), n, ptr(o), ptr(d), ptr(g_oo), ptr(g_od), ptr(go), ptr(gd), stream()),
            "nefes_ndc_bwd")
    return oo, od, go, gd


@pytest.mark.parametrize("geom", R.NDC_GEOM, ids=lambda g: f"{g[0]}x{g[1]},f={g[2]},near={g[3]}")
@pytest.mark.parametrize("n", R.NDC_N)
def test_ndc(L, n, geom):
    case = {k: v.to(DEV) for k, v in R.ndc_case(n, geom[3]).items()}
    for which in ("both", "o", "d"):
        got = ndc_library(L, geom, case["o"], case["d"], case["g_o"] if which != "d" else None, case["g_d"] if which != "o" else None)
        r64, r32 = R.ndc_eval(n, geom, torch.float64, which), R.ndc_eval(n, geom, torch.float32, which)
        tag = f"ndc[n={n},{geom[0]}x{geom[1]},near={geom[3]},upstream={which}]"
        for name, a, b32, b64 in zip(("out_o", "out_d", "g_rays_o", "g_rays_d"), got, r32, r64):
            assert a.shape == (n, 3)
            P.check(tag, name, R.rel_max(a, b64), R.rel_max(b32, b64), R.rel_max(a, b32), tol=R.TOL_NDC)


# ---- raygen, focal path ------------------------------------------------------------------------------------------------------------
def test_raygen_bwd_above_the_block_cap(ops):
    """513 x 512 rays = 1026 blocks' worth, above the 1024-block cap: the grid-stride loop of the focal kernel takes a second trip."""
    H, W, f = 513, 512, 400.0
    c2w = O.bench_pose()
    gen = torch.Generator().manual_seed(3)
    go, gd, gv = (torch.randn(H * W, 3, generator=gen) for _ in range(3))
    c = c2w.clone().double().requires_grad_()
    o, d = O.ray_bundle(H, W, f, c)
    v = d / torch.norm(d, dim=-1, keepdim=True)
    ((o.reshape(-1, 3) * go.double()).sum() + (d.reshape(-1, 3) * gd.double()).sum() + (v.reshape(-1, 3) * gv.double()).sum()).backward()
    g = ops.raygen_bwd(H, W, f, c2w.to(DEV), 0, H, go.to(DEV), gd.to(DEV), gv.to(DEV))
    K = torch.tensor([f, f, float(W * .5), float(H * .5)], dtype=torch.float32, device=DEV)
    gk, _ = ops.raygen_k_bwd(H, W, K, c2w.to(DEV), 0, H, go.to(DEV), gd.to(DEV), gv.to(DEV))
    assert torch.equal(g, gk)
    e = R.rel_max(g, c.grad)
    P.record("raygen_bwd[513x512]", "d c2w vs float64", e_hip=e, e_ref=None, direct=None, bound=1e-5)
    assert e < 1e-5, e

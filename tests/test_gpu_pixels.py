"""Rendering and refining at chosen pixels on the GPU: the raygen_px kernels against raygen_k (bit for bit on an integer grid) and against
float64 (sub-pixel, shuffled, repeated and out-of-frame points), the target sampler, render(pixels=) / render_poses(pixels=) against the
full frame and the oracle, and PoseRefiner(sparse=K).  The float64 helpers are tests/pixels_ref.py; scene, cameras and the refiner
factory are those of tests/test_gpu_intrinsics.py; the CPU twin is tests/test_pixels_args.py."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from tests import branch as B
from tests import parity_log as P
from tests import pixels_ref as R
from tests.test_gpu_intrinsics import (C, DEV, FOCAL, Nc, Ni, OFF, RH, RW, T, Wd, centred, dev, job, maps_of, off_centre, refiner, rel,
                                       rendered_centred, scene, upstream)       # noqa: F401  (scene: a fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from nefes_amd import ops as _ops
    return _ops


def subpixel_list(n, H, W, seed):
    """n points (x, y): uniform over the frame at sub-pixel positions, with a repeated point and two points outside the frame
    (x = -3.5, y = H + 2.25) where n has room for them, shuffled."""
    gen = torch.Generator().manual_seed(seed)
    px = torch.rand(n, 2, generator=gen) * torch.tensor([W - 1., H - 1.])
    if n == 1:
        return torch.tensor([[-3.5, H + 2.25]])
    if n >= 4:
        px[1] = px[0]
        px[2, 0], px[3, 1] = -3.5, H + 2.25
    if n >= 16:
        px[n // 2:n // 2 + 4] = px[4:8]
    return px[torch.randperm(n, generator=gen)].contiguous()


# ---- ray kernels ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,f,shards", [(6, 8, 7.3, [(0, 6)]), (10, 7, 9.1, [(0, 3), (3, 3), (6, 4)]), (33, 65, 58.0, [(11, 1)])])
def test_integer_grid_is_raygen_k_bit_for_bit(ops, H, W, f, shards):
    c2w, K = O.bench_pose().to(DEV), off_centre(H, W, f).to(DEV)
    go, gd, gv = upstream(H * W)
    for row0, n in shards:
        sl = slice(row0 * W, (row0 + n) * W)
        px = R.grid_pixels(W, row0, n).to(DEV)
        a, b = ops.raygen_k_fwd(H, W, K, c2w, row0, n), ops.raygen_px_fwd(px, K, c2w)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), (row0, n)
        for present in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
            g = [dev(t[sl]) if p else None for t, p in zip((go, gd, gv), present)]
            k12, k4 = ops.raygen_k_bwd(H, W, K, c2w, row0, n, *g)
            p12, p4 = ops.raygen_px_bwd(px, K, c2w, *g)
            assert torch.equal(k12, p12) and torch.equal(k4, p4), (row0, n, present)
            q12, none = ops.raygen_px_bwd(px, K, c2w, *g, want_intr=False)       # g_intr null
            assert none is None and torch.equal(q12, k12), (row0, n, present)


@pytest.mark.parametrize("n", [1, 15, 257, 2305, 1024 * 256 + 5])
def test_subpixel_lists_match_float64(ops, n):
    """One ray; part of one wave; two blocks; nine full blocks and one lane; the grid-stride loop.  Forward within the raygen bound
    (rtol 3e-7, atol 1e-7), the 12 + 2 + 2 gradient numbers within 1e-5 of float64 autograd through rays_at -- the bounds
    tests/test_gpu_intrinsics.py holds the same arithmetic to."""
    H, W, f, tag = 33, 65, 58.0, f"raygen_px[{n}]"
    c2w, K, px = O.bench_pose(), off_centre(H, W, f), subpixel_list(n, H, W, seed=n)
    go, gd, gv = upstream(n)
    c, k = c2w.double().requires_grad_(), K.double().requires_grad_()
    o64, d64, v64 = R.rays_at(px, k, c)
    sum((x * t.double()).sum() for x, t in zip((o64, d64, v64), (go, gd, gv))).backward()
    o, d, v = ops.raygen_px_fwd(px.to(DEV), K.to(DEV), c2w.to(DEV))
    assert torch.equal(o.cpu(), c2w[:3, 3].expand(n, 3))
    for name, got, want in (("rays_d", d, d64), ("viewdirs", v, v64)):
        print(f"[{tag}] {name}: max abs err {float((got.cpu().double() - want.detach()).abs().max()):.2e}")
        np.testing.assert_allclose(got.cpu().numpy(), want.detach().numpy(), rtol=3e-7, atol=1e-7)
    g_c2w, g_k = ops.raygen_px_bwd(px.to(DEV), K.to(DEV), c2w.to(DEV), dev(go), dev(gd), dev(gv))
    errs = {"d c2w": rel(g_c2w, c.grad), "d (fx, fy)": rel(g_k[:2], k.grad[:2]), "d (cx, cy)": rel(g_k[2:], k.grad[2:])}
    for name, e in errs.items():
        print(f"[{tag}] {name}: {e:.2e}")
        P.record(tag, name + " vs float64", e_hip=e, e_ref=None, direct=None, bound=1e-5)
    assert all(e < 1e-5 for e in errs.values()), errs


# ---- target sampler ---------------------------------------------------------------------------------------------------------------
def test_sampler_returns_the_map_at_integer_coordinates(ops):
    Cc, H, W = 3, 5, 7
    m = torch.randn(Cc, H, W, generator=torch.Generator().manual_seed(1))
    px = torch.cat([torch.tensor([[0., 0.], [W - 1., H - 1.], [W - 1., 0.], [0., H - 1.]]), R.grid_pixels(W, 0, H)])
    got = ops.sample_pixels(m.to(DEV), px.to(DEV)).cpu()
    assert torch.equal(got, m[:, px[:, 1].long(), px[:, 0].long()])


@pytest.mark.parametrize("Cc", [1, 19])
@pytest.mark.parametrize("n", [1, 65, 1000])
def test_sampler_matches_float64_bilinear(ops, n, Cc):
    """Fractional and out-of-frame points within 1e-6 max|map| of the float64 helper: six fp32 roundings (three per a + f (b - a), two
    levels deep), each at most 2^-24 of the largest tap -- 1e-6 leaves a factor of 2.8."""
    H, W = 5, 7
    m = torch.randn(Cc, H, W, generator=torch.Generator().manual_seed(Cc))
    px = subpixel_list(n, H, W, seed=100 + n)
    if n >= 8:
        px[4:8] = torch.tensor([[W - 1., 1.5], [2.25, H - 1.], [W + 4., -1.], [W - 1., H - 1.]])
    got = ops.sample_pixels(m.to(DEV), px.to(DEV)).cpu()
    assert tuple(got.shape) == (Cc, n)
    err = float((got.double() - R.bilinear(m, px)).abs().max() / m.abs().max())
    print(f"[sample_px n={n} C={Cc}] max err / max|map| {err:.2e}")
    P.record(f"sample_px[{n},{Cc}]", "bilinear vs float64", e_hip=err, e_ref=None, direct=None, bound=1e-6)
    assert err < 1e-6


# ---- render -----------------------------------------------------------------------------------------------------------------------
def render_at(scene, px=None, K=None, idx=None, seed=5):
    """(maps, c2w.grad, K.grad) of the 4 x 6 scene at the bench pose: the full frame (px None) or the pixel list.  Loss: O.bench_loss,
    or with idx (full frame) / seed an upstream that is zero off the rows idx of the frame."""
    from nefes_amd.render import render
    c2w = O.bench_pose().to(DEV).requires_grad_()
    k = None if K is None else K.clone().to(DEV).requires_grad_()
    kw = dict(scene, **({} if k is None else {"intrinsics": k}), **({} if px is None else {"pixels": px}))
    out = render(RH, RW, FOCAL, c2w=c2w, near=0., far=4., **kw)
    m = maps_of(out)
    if idx is None and seed is None:
        O.bench_loss(m["rgb"], m["feat"]).backward()
    else:
        gen = torch.Generator().manual_seed(seed)
        rows = RH * RW if idx is None else len(idx)
        g_rgb, g_feat = torch.randn(rows, 3, generator=gen).to(DEV), torch.randn(rows, C, generator=gen).to(DEV)
        pick = (lambda t: t) if idx is None or px is not None else (lambda t: t[idx])
        ((pick(m["rgb"]) * g_rgb).sum() + (pick(m["feat"]) * g_feat).sum()).backward()
    return m, c2w.grad, None if k is None else k.grad


@pytest.mark.parametrize("camera", [False, True])
def test_render_at_the_full_integer_grid_is_render(scene, camera):
    K = off_centre(RH, RW, FOCAL) if camera else None
    full = render_at(scene, None, K, seed=None)
    grid = render_at(scene, R.grid_pixels(RW, 0, RH).to(DEV), K, seed=None)
    assert all(torch.equal(grid[0][k], full[0][k]) for k in full[0])
    assert torch.equal(grid[1], full[1]) and (K is None or torch.equal(grid[2], full[2]))
    host = render_at(scene, R.grid_pixels(RW, 0, RH).long().tolist(), K, seed=None)        # host integers: converted, the same rays
    assert all(torch.equal(host[0][k], full[0][k]) for k in full[0]) and torch.equal(host[1], full[1])


def test_render_of_a_subset_is_the_full_renders_rows(scene):
    """A ray's maps do not depend on its neighbours: a shuffled 11-pixel subset within 1e-6 (the project's map bound) of the full render's
    rows; its pose gradient within 1e-6 relative of the full render's under an upstream that is zero off the subset (they differ in the
    order of float64 sums and one fp32 rounding)."""
    idx = torch.randperm(RH * RW, generator=torch.Generator().manual_seed(8))[:11]
    px = R.grid_pixels(RW, 0, RH)[idx].contiguous().to(DEV)
    full, g_full, _ = render_at(scene, None, None, idx=idx.to(DEV))
    sub, g_sub, _ = render_at(scene, px, None, idx=idx.to(DEV))
    errs = {k: rel(sub[k], full[k][idx.to(DEV)]) for k in full}
    errs["d c2w"] = rel(g_sub, g_full)
    print("[render_pixels subset]", {k: f"{v:.2e}" for k, v in errs.items()})
    for k, e in errs.items():
        P.record("render_pixels_subset", k, e_hip=None, e_ref=None, direct=e, bound=1e-6)
    assert tuple(sub["rgb"].shape) == (11, 3) and tuple(sub["feat"].shape) == (11, C) and tuple(sub["disp"].shape) == (11,)
    assert all(e < 1e-6 for e in errs.values()), errs


def test_render_at_subpixel_points_maps_and_gradients(scene):
    """24 sub-pixel points at the off-centre camera: maps within 1e-4 of the fp32 oracle on rays_at's rays; d c2w, d (fx, fy), d (cx, cy)
    against float64 on the kernels' own ReLU branch pattern and sample depths (tests/branch.py), as
    test_render_off_centre_camera_maps_and_gradients does for the frame."""
    from nefes_amd.render import render
    K0, px0 = off_centre(RH, RW, FOCAL), subpixel_list(RH * RW, RH, RW, seed=24)
    c2w, K = O.bench_pose().to(DEV).requires_grad_(), K0.to(DEV).requires_grad_()
    with B.tapped() as tap:
        out = render(RH, RW, FOCAL, c2w=c2w, near=0., far=4., intrinsics=K, pixels=px0.to(DEV), **scene)
    O.bench_loss(out[0], out[3]["feat_map"]).backward()
    cfg = O.RenderCfg(N_samples=Nc, N_importance=Ni)

    def oracle(dt, act=None, zf=None):
        c, k = O.bench_pose(dt).requires_grad_(), K0.to(dt).requires_grad_()
        o, d, _ = R.rays_at(px0, k, c)
        r = O.render(RH, RW, FOCAL, O.make_field_params("coarse", Wd, C, dtype=dt), O.make_field_params("fine", Wd, C, dtype=dt), cfg,
                     rays=(o, d), near=0., far=4., fine_act=act, z_fine=zf)
        gc, gk = torch.autograd.grad(O.bench_loss(r[0], r[3]["feat_map"]), [c, k])
        return maps_of(r), {"d c2w": gc, "d (fx, fy)": gk[:2], "d (cx, cy)": gk[2:]}
    ref = oracle(torch.float32)[0]
    errs = {k: B.rel(v, ref[k]) for k, v in maps_of(out).items()}
    print("[render_pixels] maps vs the fp32 oracle:", {k: f"{v:.2e}" for k, v in errs.items()})
    for k, e in errs.items():
        P.record("render_pixels", k + " map", e_hip=None, e_ref=None, direct=e, bound=1e-4)
    assert all(e < 1e-4 for e in errs.values()), errs
    hip = {"d c2w": c2w.grad, "d (fx, fy)": K.grad[:2], "d (cx, cy)": K.grad[2:]}
    B.pinned_gradients("render_pixels", hip, tap, Wd, lambda dt, act, zf: oracle(dt, act, zf)[1])


def test_render_poses_with_one_pixel_set_per_pose_is_two_renders(scene):
    from nefes_amd.render import render, render_poses
    n = 9
    gen = torch.Generator().manual_seed(12)
    g_rgb, g_feat = torch.randn(2, n, 3, generator=gen).to(DEV), torch.randn(2, n, C, generator=gen).to(DEV)
    poses0 = torch.stack([O.bench_pose(), O.se3_exp_pose((0.05, 0.15, -0.1), (0.2, 0.1, 0.25))])
    px2 = torch.stack([subpixel_list(n, RH, RW, seed=1), subpixel_list(n, RH, RW, seed=2)]).to(DEV)
    K0 = off_centre(RH, RW, FOCAL)
    poses, K = poses0.to(DEV).requires_grad_(), K0.to(DEV).requires_grad_()
    out = render_poses(RH, RW, FOCAL, poses, near=0., far=4., intrinsics=K, pixels=px2, **scene)
    assert tuple(out[0].shape) == (2, n, 3) and tuple(out[3]["feat_map"].shape) == (2, n, C)
    ((out[0] * g_rgb).sum() + (out[3]["feat_map"] * g_feat).sum()).backward()
    k_sum = torch.zeros(4, device=DEV)
    for b in range(2):
        c, k = poses0[b].to(DEV).requires_grad_(), K0.to(DEV).requires_grad_()
        one = render(RH, RW, FOCAL, c2w=c, near=0., far=4., intrinsics=k, pixels=px2[b], **scene)
        ((one[0] * g_rgb[b]).sum() + (one[3]["feat_map"] * g_feat[b]).sum()).backward()
        m, mb = maps_of(one), maps_of(out)
        assert all(torch.equal(m[key], mb[key][b]) for key in m), b
        assert torch.equal(c.grad, poses.grad[b]), b
        k_sum += k.grad
    assert torch.equal(K.grad, k_sum)                                         # the shared camera: the sum of the two renders' gradients
    shared = render_poses(RH, RW, FOCAL, poses0.to(DEV), near=0., far=4., intrinsics=K0.to(DEV), pixels=px2[0], **scene)
    twice = render_poses(RH, RW, FOCAL, poses0.to(DEV), near=0., far=4., intrinsics=K0.to(DEV), pixels=torch.stack([px2[0], px2[0]]), **scene)
    assert all(torch.equal(a, b) for a, b in zip(maps_of(shared).values(), maps_of(twice).values()))
    assert torch.equal(shared[0][0], out[0][0]) and not torch.equal(shared[0][1], out[0][1])


# ---- refinement -------------------------------------------------------------------------------------------------------------------
KP = 40


def frame_points(g, n, seed):
    H, W, _ = g["hwf"].tolist()
    ts = int(g["tinyscale"])
    return subpixel_list(n, int(H // ts), int(W // ts), seed).to(DEV)


def frame_mask(g):
    H, W, _ = g["hwf"].tolist()
    ts = int(g["tinyscale"])
    return (torch.rand(int(H // ts), int(W // ts), generator=torch.Generator().manual_seed(6)) > 0.35).to(torch.uint8)


def by_hand(r, target, px, per_pixel=False, mask=None, K=None):
    """The sparse iteration's chain called by hand at the refiner's state: (loss, d r, d t, d K)."""
    from nefes_amd import ops
    from nefes_amd.render import render
    rr, tt = r.model.r.detach().clone().requires_grad_(), r.model.t.detach().clone().requires_grad_()
    ws = r.world_setup
    c2w = ops.pose_compose(rr, tt, r.model.init_c2w, ws["pose_scale"], ws["move_all_cam_vec"], ws["pose_scale2"])
    out = render(r.h, r.w, r.focal, c2w=c2w.reshape(3, 4), near=r.near, far=r.far, img_idx=r.hist, pixels=px,
                 **r.kw, **({} if K is None else {"intrinsics": K}))
    feat = out[3]["feat_map"].t()
    m = None
    if mask is not None:
        xi, yi = px[:, 0].round().clamp(0, r.w - 1).long(), px[:, 1].round().clamp(0, r.h - 1).long()
        m = (mask.to(DEV)[yi, xi] > 0).to(torch.uint8).reshape(1, -1).contiguous()
    op = ops.pixel_cosine_loss if per_pixel else ops.cosine_feature_loss
    loss = op(feat, ops.sample_pixels(target, px), mask=m)
    loss.backward()
    return loss.detach(), rr.grad, tt.grad, None if K is None else K.grad


@pytest.mark.parametrize("per_pixel,masked", [(False, False), (True, False), (False, True), (True, True)])
def test_sparse_iteration_is_the_chain_called_by_hand(golden, per_pixel, masked):
    g = golden("refine")
    init, target, hist = job(g)
    px, mask = frame_points(g, KP, seed=3), frame_mask(g) if masked else None
    r = refiner(g, False, sparse=KP, per_pixel=per_pixel, masked=masked)
    r._reset(init, target, hist, mask, px)
    assert torch.equal(r.pixels, px) and tuple(r.target.shape) == (int(g["C"]), KP)
    if masked:
        assert 0 < int(r.mask.sum()) < KP                                     # the mask does drop some of the points
    loss = r.loss_and_grad().clone()
    want = by_hand(r, target, px, per_pixel, mask)
    print(f"[sparse wiring per_pixel={per_pixel} masked={masked}] loss {float(loss):.6f}  by hand {float(want[0]):.6f}")
    assert torch.isfinite(loss) and float(r.model.r.grad.abs().max()) > 0
    assert torch.equal(loss, want[0]) and torch.equal(r.model.r.grad, want[1]) and torch.equal(r.model.t.grad, want[2])


def test_sparse_loop_graph_equals_eager(golden):
    g = golden("refine")
    px = frame_points(g, KP, seed=3)
    eager = refiner(g, False, sparse=KP).refine(*job(g), 5, pixels=px)
    graph = refiner(g, True, sparse=KP).refine(*job(g), 5, pixels=px)
    print("[sparse graph vs eager] losses", [f"{float(v):.6f}" for v in eager[1]])
    assert torch.equal(eager[0], graph[0]) and torch.equal(eager[1], graph[1])
    drawn = [refiner(g, gr, sparse=KP, seed=s) for gr, s in ((False, 1), (True, 1), (False, 2))]      # pixels=None: K distinct integer pixels, by the seed
    for r in drawn:
        r.refine(*job(g), 0)
    a, b, c = (r.pixels.cpu() for r in drawn)
    assert torch.equal(a, b) and not torch.equal(a, c) and torch.equal(a, a.round()) and len({tuple(p) for p in a.tolist()}) == KP
    assert float(a[:, 0].min()) >= 0 and float(a[:, 0].max()) <= drawn[0].w - 1 and float(a[:, 1].min()) >= 0 and float(a[:, 1].max()) <= drawn[0].h - 1


def test_captured_iteration_reads_the_pixels_from_memory(golden):
    """Replay, set_pixels(other), replay: the second loss is the eager loss of a fresh refiner on `other`, bit for bit, and not the first
    replay's.  Pixels passed to the kernels by value, or a target that was not re-sampled, would replay the first."""
    g = golden("refine")
    init, target, hist = job(g)
    px, other = frame_points(g, KP, seed=3), frame_points(g, KP, seed=4)
    r = refiner(g, True, sparse=KP)
    r.refine(init, target, hist, 0, pixels=px)                                # state, capture, state again; no iteration yet
    assert r.graph is not None
    r.replay()
    first = r.loss.clone()
    r._reset(init, target, hist, None, px)
    r.set_pixels(other)
    r.replay()
    second = r.loss.clone()
    losses = []
    for p in (px, other):
        fresh = refiner(g, False, sparse=KP)
        fresh._reset(init, target, hist, None, p)
        losses.append(fresh.loss_and_grad().clone())
    print(f"[graph_reads_pixels] first {float(first):.6f}  after set_pixels {float(second):.6f}  eager {float(losses[1]):.6f}")
    assert torch.equal(first, losses[0])
    assert torch.equal(second, losses[1]) and not torch.equal(second, first)


def pose_error(pose, true):
    """(translation distance, rotation angle in degrees) between two 4 x 4 (or 3 x 4) poses."""
    a, b = pose.detach().cpu().double()[:3], true.detach().cpu().double()[:3]
    cos = ((a[:, :3].T @ b[:, :3]).trace() - 1) / 2
    return float((a[:, 3] - b[:, 3]).norm()), float(torch.rad2deg(torch.acos(cos.clamp(-1, 1))))


def test_sparse_refinement_descends(golden):
    """Target: the library's own feat_map at the true pose, at 96 sub-pixel points; 20 iterations from the fixture's perturbed start.
    The loss falls and the pose error -- translation distance and rotation angle, each -- ends below the start's.  No rate is asserted:
    nobody has measured one."""
    g = golden("refine")
    init, frame, hist = job(g)
    true = T(g["true_c2w"]).float().to(DEV)
    px = frame_points(g, 96, seed=9)
    r = refiner(g, False, sparse=96)
    r._reset(true, frame, hist, None, px)
    target = r.features()                                                     # [C, 96] at r = t = 0 on the true pose
    r._reset(init, frame, hist, None, px)
    with torch.no_grad():
        r.target.copy_(target)
    start = pose_error(r._refined_pose(), true)
    losses = []
    for _ in range(20):
        r._iteration()
        losses.append(float(r.loss))
    end = pose_error(r._refined_pose(), true)
    print(f"[sparse descent] loss {losses[0]:.4e} -> {losses[-1]:.4e}; |dt| {start[0]:.4f} -> {end[0]:.4f}; angle {start[1]:.3f} -> {end[1]:.3f} deg")
    P.record("sparse_refine", "20 iterations at 96 sub-pixel points", loss_first=losses[0], loss_last=losses[-1], dt_first=start[0],
             dt_last=end[0], deg_first=start[1], deg_last=end[1])
    assert losses[-1] < losses[0]
    assert end[0] < start[0] and end[1] < start[1]


def test_sparse_learn_focal_gradient_is_the_cameras(golden):
    """learn_focal with sparse=: d loss / d log_f is finite, non-zero and K.grad[:2] . (fx, fy) of the chain called by hand."""
    g = golden("refine")
    init, target, hist = job(g)
    px = frame_points(g, KP, seed=3)
    r = refiner(g, False, sparse=KP, learn_focal=True)
    r._reset(init, target, hist, None, px)
    loss = r.loss_and_grad().clone()
    K = rendered_centred(g).to(DEV).requires_grad_()
    want = by_hand(r, target, px, K=K)
    got, by_k = r.log_f.grad.clone(), (want[3][0] * K.detach()[0] + want[3][1] * K.detach()[1]).reshape(1)
    print(f"[sparse learn_focal] d loss / d log_f {float(got):.6e}  K.grad[:2] . (fx, fy) {float(by_k):.6e}")
    assert torch.equal(loss, want[0]) and bool(torch.isfinite(got).all()) and float(got) != 0.
    assert torch.equal(got, by_k)

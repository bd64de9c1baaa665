"""Pinhole intrinsics (fx, fy, cx, cy) on the GPU: the raygen_k kernels against the focal kernels (bit for bit at a centred camera) and
against float64 (off-centre, anisotropic), render() / render_poses() with `intrinsics=`, and PoseRefiner(intrinsics=, learn_focal=).
The float64 rays are the three lines of `rays_of` below, differentiable w.r.t. the pose and the camera; the CPU twin is
tests/test_intrinsics_args.py."""
import types

import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from tests import branch as B
from tests import parity_log as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = lambda a: torch.from_numpy(np.asarray(a))
OFF = (1.07, 0.95, 1.1, 0.9)        # centred (f, f, W/2, H/2) -> fx = 1.07 f, fy = 0.95 f, cx = 0.55 W, cy = 0.45 H


def rays_of(H, W, K, c2w, row0=0, nrows=None):
    """get_rays for the camera K = (fx, fy, cx, cy) in K's dtype: (rays_o, rays_d, viewdirs), each [nrows*W, 3]."""
    ii, jj = torch.meshgrid(torch.arange(W, dtype=K.dtype), torch.arange(row0, row0 + (H - row0 if nrows is None else nrows), dtype=K.dtype), indexing="xy")
    d = torch.sum(torch.stack([(ii - K[2]) / K[0], -(jj - K[3]) / K[1], -torch.ones_like(ii)], -1)[..., None, :] * c2w[:3, :3], -1).reshape(-1, 3)
    return c2w[:3, 3].expand(d.shape), d, d / torch.norm(d, dim=-1, keepdim=True)


def centred(H, W, f):
    return torch.tensor([f, f, float(W * .5), float(H * .5)], dtype=torch.float32)


def off_centre(H, W, f):
    return centred(H, W, f) * torch.tensor(OFF, dtype=torch.float32)


def upstream(n, seed=3):
    gen = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(n, 3, generator=gen) for _ in range(3))


def rel(a, b):
    return B.rel(a, b)


@pytest.fixture(scope="module")
def ops():
    from nefes_amd import ops as _ops
    return _ops


def dev(t):
    return None if t is None else t.to(DEV)


# ---- kernels ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,f,shards", [(6, 8, 7.3, [(0, 6)]), (5, 7, 6.1, [(0, 5)]), (10, 7, 9.1, [(0, 3), (3, 3), (6, 4)])])
def test_centred_camera_is_the_focal_path_bit_for_bit(golden, ops, H, W, f, shards):
    c2w = (T(golden("raygen")["c2w0"]).float()[:3, :4].contiguous() if (H, W) == (6, 8) else O.bench_pose()).to(DEV)
    K = centred(H, W, f).to(DEV)
    go, gd, gv = upstream(H * W)
    for row0, n in shards:
        sl = slice(row0 * W, (row0 + n) * W)
        a, b = ops.raygen_fwd(H, W, f, c2w, row0, n), ops.raygen_k_fwd(H, W, K, c2w, row0, n)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), (row0, n)
        for present in ((1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)):
            g = [dev(t[sl]) if p else None for t, p in zip((go, gd, gv), present)]
            g12 = ops.raygen_bwd(H, W, f, c2w, row0, n, *g)
            k12, k4 = ops.raygen_k_bwd(H, W, K, c2w, row0, n, *g)
            assert torch.equal(g12, k12) and bool(torch.isfinite(k4).all()), (row0, n, present)
            assert torch.equal(ops.raygen_k_bwd(H, W, K, c2w, row0, n, *g, want_intr=False)[0], g12)


def check_against_float64(ops, H, W, f, tag, present=(1, 1, 1), shards=None):
    """Forward within the raygen bound (rtol 3e-7, atol 1e-7), the 12 + 2 + 2 gradient numbers within 1e-5 of float64 autograd --
    (fx, fy) and (cx, cy) as separate records: their scales differ by the focal."""
    c2w, K = O.bench_pose(), off_centre(H, W, f)
    go, gd, gv = (t if p else None for t, p in zip(upstream(H * W), present))
    c, k = c2w.double().requires_grad_(), K.double().requires_grad_()
    o64, d64, v64 = rays_of(H, W, k, c)
    sum(((x * t.double()).sum() for x, t in zip((o64, d64, v64), (go, gd, gv)) if t is not None)).backward()
    o, d, v = ops.raygen_k_fwd(H, W, K.to(DEV), c2w.to(DEV))
    assert torch.equal(o.cpu(), c2w[:3, 3].expand(H * W, 3))
    for name, got, want in (("rays_d", d, d64), ("viewdirs", v, v64)):
        print(f"[{tag}] {name}: max abs err {float((got.cpu().double() - want.detach()).abs().max()):.2e}")
        np.testing.assert_allclose(got.cpu().numpy(), want.detach().numpy(), rtol=3e-7, atol=1e-7)
    g_c2w, g_k = ops.raygen_k_bwd(H, W, K.to(DEV), c2w.to(DEV), 0, H, dev(go), dev(gd), dev(gv))
    kg = k.grad if k.grad is not None else torch.zeros(4, dtype=torch.float64)
    errs = {"d c2w": rel(g_c2w, c.grad)}
    if gd is not None or gv is not None:
        errs.update({"d (fx, fy)": rel(g_k[:2], kg[:2]), "d (cx, cy)": rel(g_k[2:], kg[2:])})
    else:                                                                     # only rays_o has an upstream gradient: the camera's is exactly zero
        assert torch.equal(g_k.cpu(), torch.zeros(4))
    for name, e in errs.items():
        print(f"[{tag}] {name}: {e:.2e}")
        P.record(tag, name + " vs float64", e_hip=e, e_ref=None, direct=None, bound=1e-5)
    assert all(e < 1e-5 for e in errs.values()), errs
    if shards:                                                                # row shards sum to the unsharded 16 numbers, forward rows are the frame's
        acc = torch.zeros(16, dtype=torch.float64)
        for row0, n in shards:
            sl = slice(row0 * W, (row0 + n) * W)
            a, b = ops.raygen_k_bwd(H, W, K.to(DEV), c2w.to(DEV), row0, n, *(dev(t[sl]) if t is not None else None for t in (go, gd, gv)))
            acc += torch.cat([a.reshape(-1), b]).cpu().double()
            assert all(torch.equal(x, y[sl]) for x, y in zip(ops.raygen_k_fwd(H, W, K.to(DEV), c2w.to(DEV), row0, n), (o, d, v)))
        assert rel(acc[:12], c.grad.reshape(-1)) < 1e-5 and rel(acc[12:14], kg[:2]) < 1e-5 and rel(acc[14:], kg[2:]) < 1e-5


@pytest.mark.parametrize("present", [(1, 1, 1), (1, 0, 0), (0, 1, 0), (0, 0, 1)])
def test_off_centre_camera_matches_float64(ops, present):
    check_against_float64(ops, 10, 7, 9.1, f"raygen_k[10x7,{present}]", present, shards=[(0, 3), (3, 3), (6, 4)] if all(present) else None)


@pytest.mark.parametrize("H,W,f,shards", [(3, 5, 4.2, None), (33, 65, 58.0, [(0, 11), (11, 1), (12, 21)]), (513, 512, 400.0, None)])
def test_reduction_shapes(ops, H, W, f, shards):
    """One partly filled wave; nine blocks, the last partly filled; more than 1024 blocks' worth of rays (the grid-stride loop)."""
    check_against_float64(ops, H, W, f, f"raygen_k[{H}x{W}]", shards=shards)


# ---- render -----------------------------------------------------------------------------------------------------------------------
Wd, C, Ni, Nc, RH, RW = 256, 16, 128, 64, 4, 6
FOCAL = 525.505 * RW / 640.


@pytest.fixture(scope="module")
def scene():
    """smoke()'s scene: 4 x 6, width 256, 16 feature channels, 64 + 128 samples."""
    from nefes_amd.field import NeRFH_NFF
    coarse = NeRFH_NFF('coarse', W=Wd, f_dim=C).requires_grad_(False).to(DEV)
    fine = NeRFH_NFF('fine', W=Wd, f_dim=C, encode_appearance=True, encode_transient=True).requires_grad_(False).to(DEV)
    args = types.SimpleNamespace(nerfh_nff=True, use_fine_only=False, NeRFW=True, transient_at_test=True, netchunk=1 << 21)
    return dict(network_query_fn=None, perturb=False, N_importance=Ni, N_samples=Nc, network_fn=coarse, network_fine=fine,
                use_viewdirs=True, white_bkgd=False, raw_noise_std=0., test_time=True, args=args, ndc=False, lindisp=False)


def maps_of(out):
    return {"rgb": out[0], "disp": out[1], "acc": out[2], "feat": out[3]["feat_map"]}


def test_render_with_the_centred_camera_is_render(scene):
    from nefes_amd.render import render
    res = []
    for K in (None, centred(RH, RW, FOCAL).to(DEV), tuple(centred(RH, RW, FOCAL).tolist())):
        c2w = O.bench_pose().to(DEV).requires_grad_()
        out = render(RH, RW, FOCAL, c2w=c2w, near=0., far=4., **(scene if K is None else dict(scene, intrinsics=K)))   # (from inside the kwargs)
        O.bench_loss(out[0], out[3]["feat_map"]).backward()
        res.append((maps_of(out), c2w.grad))
    for m, g in res[1:]:
        assert all(torch.equal(m[k], res[0][0][k]) for k in m) and torch.equal(g, res[0][1])


def test_render_off_centre_camera_maps_and_gradients(scene):
    """Maps within 1e-4 of the fp32 oracle on the same rays; d c2w, d (fx, fy), d (cx, cy) against float64 on the kernels' own ReLU
    branch pattern and sample depths under the suite's rule e_hip <= max(1e-4, 1.5 e_ref) (tests/branch.py, audit class same_inputs)."""
    from nefes_amd.render import render
    K0 = off_centre(RH, RW, FOCAL)
    c2w, K = O.bench_pose().to(DEV).requires_grad_(), K0.to(DEV).requires_grad_()
    with B.tapped() as tap:
        out = render(RH, RW, FOCAL, c2w=c2w, near=0., far=4., intrinsics=K, **scene)
    O.bench_loss(out[0], out[3]["feat_map"]).backward()
    assert K.grad is not None and tuple(K.grad.shape) == (4,)
    cfg = O.RenderCfg(N_samples=Nc, N_importance=Ni)

    def oracle(dt, act=None, zf=None):
        c, k = O.bench_pose(dt).requires_grad_(), K0.to(dt).requires_grad_()
        o, d, _ = rays_of(RH, RW, k, c)
        r = O.render(RH, RW, FOCAL, O.make_field_params("coarse", Wd, C, dtype=dt), O.make_field_params("fine", Wd, C, dtype=dt), cfg,
                     rays=(o, d), near=0., far=4., fine_act=act, z_fine=zf)
        gc, gk = torch.autograd.grad(O.bench_loss(r[0], r[3]["feat_map"]), [c, k])
        return maps_of(r), {"d c2w": gc, "d (fx, fy)": gk[:2], "d (cx, cy)": gk[2:]}
    ref = oracle(torch.float32)[0]
    errs = {k: B.rel(v, ref[k]) for k, v in maps_of(out).items()}
    print("[render_intrinsics] maps vs the fp32 oracle:", {k: f"{v:.2e}" for k, v in errs.items()})
    for k, e in errs.items():
        P.record("render_intrinsics", k + " map", e_hip=None, e_ref=None, direct=e, bound=1e-4)
    assert all(e < 1e-4 for e in errs.values()), errs
    hip = {"d c2w": c2w.grad, "d (fx, fy)": K.grad[:2], "d (cx, cy)": K.grad[2:]}
    B.pinned_gradients("render_intrinsics", hip, tap, Wd, lambda dt, act, zf: oracle(dt, act, zf)[1])


def test_render_poses_with_one_camera_per_pose_is_two_renders(scene):
    from nefes_amd.render import render, render_poses
    n = RH * RW
    gen = torch.Generator().manual_seed(11)
    g_rgb, g_feat = torch.randn(2, n, 3, generator=gen).to(DEV), torch.randn(2, n, C, generator=gen).to(DEV)
    poses0 = torch.stack([O.bench_pose(), O.se3_exp_pose((0.05, 0.15, -0.1), (0.2, 0.1, 0.25))])
    K0 = torch.stack([off_centre(RH, RW, FOCAL), centred(RH, RW, 1.1 * FOCAL)])
    poses, K2 = poses0.to(DEV).requires_grad_(), K0.to(DEV).requires_grad_()
    out = render_poses(RH, RW, FOCAL, poses, near=0., far=4., intrinsics=K2, **scene)
    ((out[0] * g_rgb).sum() + (out[3]["feat_map"] * g_feat).sum()).backward()
    for b in range(2):
        c, k = poses0[b].to(DEV).requires_grad_(), K0[b].to(DEV).requires_grad_()
        one = render(RH, RW, FOCAL, c2w=c, near=0., far=4., intrinsics=k, **scene)
        ((one[0] * g_rgb[b]).sum() + (one[3]["feat_map"] * g_feat[b]).sum()).backward()
        m, mb = maps_of(one), maps_of(out)
        assert all(torch.equal(m[key], mb[key][b]) for key in m), b
        assert torch.equal(c.grad, poses.grad[b]) and torch.equal(k.grad, K2.grad[b]), b
    shared = render_poses(RH, RW, FOCAL, poses0.to(DEV), near=0., far=4., intrinsics=K0[0].to(DEV), **scene)       # one camera for all poses
    assert torch.equal(shared[0][0], out[0][0]) and not torch.equal(shared[0][1], out[0][1])


# ---- refinement -------------------------------------------------------------------------------------------------------------------
def refiner(g, graph, **more):
    """tests/test_gpu_refine.py::refiner with PoseRefiner's further keywords."""
    from nefes_amd.field import NeRFH_NFF
    from nefes_amd.refine import PoseRefiner
    wd, c = int(g["Wd"]), int(g["C"])
    coarse = NeRFH_NFF('coarse', W=wd, f_dim=c).requires_grad_(False).to(DEV)
    fine = NeRFH_NFF('fine', W=wd, f_dim=c, encode_appearance=True, encode_transient=True).requires_grad_(False).to(DEV)
    with torch.no_grad():
        coarse.exposure_embedding.params.copy_(T(g["exposure_params"]))
    args = types.SimpleNamespace(nerfh_nff=True, use_fine_only=False, NeRFW=True, transient_at_test=True, encode_hist=True)
    kw = dict(network_query_fn=None, perturb=0., N_importance=int(g["Ni"]), N_samples=int(g["Nc"]), network_fn=coarse,
              network_fine=fine, use_viewdirs=True, white_bkgd=False, raw_noise_std=0., test_time=True, args=args, ndc=False,
              lindisp=False)
    world = dict(pose_scale=float(g["pose_scale"]), pose_scale2=float(g["pose_scale2"]), move_all_cam_vec=g["move_all_cam_vec"].tolist())
    H, W, focal = g["hwf"].tolist()
    more.setdefault("lr_r", float(g["lr"][0]))
    more.setdefault("lr_t", float(g["lr"][1]))
    return PoseRefiner(kw, args, (H, W, focal), float(g["near"]), float(g["far"]), tinyscale=int(g["tinyscale"]), world_setup=world,
                       graph=graph, device=DEV, **more)


def rendered_centred(g):
    """The centred camera of the RENDERED frame (h, w, focal / ts) of the refine.npz scene."""
    H, W, focal = g["hwf"].tolist()
    ts = int(g["tinyscale"])
    return centred(int(H // ts), int(W // ts), float(focal) / ts)


def job(g):
    return T(g["init_c2w"]).to(DEV), T(g["target"]).to(DEV), T(g["hist"]).to(DEV)


@pytest.mark.parametrize("graph", [False, True])
def test_refiner_with_the_centred_camera_walks_the_same_trajectory(golden, graph):
    g = golden("refine")
    plain = refiner(g, graph).refine(*job(g), 5)
    for K in (rendered_centred(g).to(DEV), tuple(rendered_centred(g).tolist())):
        pose, losses = refiner(g, graph, intrinsics=K).refine(*job(g), 5)
        assert torch.equal(pose, plain[0]) and torch.equal(losses, plain[1])
    assert float(plain[1][-1]) < float(plain[1][0])


def test_captured_iteration_reads_the_camera_from_memory(golden):
    """Replay, move refiner.intrinsics in place to the off-centre camera, replay: the second loss is the eager loss of a fresh refiner
    built with that camera, bit for bit, and not the first replay's.  A camera passed to the kernels by value would replay the first."""
    g = golden("refine")
    r = refiner(g, True, intrinsics=rendered_centred(g).to(DEV))
    r.refine(*job(g), 0)                                                      # state, capture, state again; no iteration yet
    assert r.graph is not None
    r.replay()
    first = r.loss.clone()
    r._reset(*job(g))
    r.intrinsics.mul_(torch.tensor(OFF, device=DEV))
    r.replay()
    second = r.loss.clone()
    fresh = refiner(g, False, intrinsics=r.intrinsics.clone())
    fresh._reset(*job(g))
    eager = fresh.loss_and_grad().clone()
    centre = refiner(g, False)
    centre._reset(*job(g))
    assert torch.equal(first, centre.loss_and_grad())                         # (the first replay was the centred camera's loss)
    print(f"[graph_reads_camera] centred {float(first):.6f}  off-centre replayed {float(second):.6f}  eager {float(eager):.6f}")
    assert torch.equal(second, eager) and not torch.equal(second, first)


def test_learn_focal_moves_towards_the_true_focal(golden):
    """Target: the library's own fused features at the true pose with log_f* = 0.02; start at log_f = 0 with the pose frozen
    (lr_r = lr_t = 0), 20 iterations at the default lr_f.  No convergence rate is asserted: nobody has measured one."""
    g = golden("refine")
    init, _, hist = job(g)
    true_log_f, out = 0.02, {}
    for graph in (False, True):
        r = refiner(g, graph, learn_focal=True, lr_r=0., lr_t=0.)
        r._reset(init, torch.zeros_like(r.target), hist)
        with torch.no_grad():
            r.log_f.fill_(true_log_f)
        target = r.features()[0]
        if not graph:
            r._reset(init, target, hist)
            r.loss_and_grad()
            grad0 = float(r.log_f.grad)
        pose, losses, log_f = r.refine(init, target, hist, 20)
        assert torch.equal(pose[:3, :4], init[:3, :4])                        # the pose did not move
        out[graph] = (target, losses, log_f)
    assert all(torch.equal(a, b) for a, b in zip(out[False], out[True]))      # graph and eager agree bit for bit
    _, losses, log_f = out[True]
    first, last, end = float(losses[0]), float(losses[-1]), float(log_f)
    print(f"[learn_focal] d loss / d log_f at 0: {grad0:.3e}; log_f after 20 iterations {end:.5f} (true {true_log_f}); loss {first:.3e} -> {last:.3e}")
    P.record("learn_focal", "log_f after 20 iterations from 0 (true 0.02)", log_f=end, grad_first=grad0, loss_first=first, loss_last=last)
    assert grad0 < 0                                                          # descent raises log_f, towards log_f* > 0
    assert abs(end - true_log_f) < abs(0. - true_log_f)
    assert last < first

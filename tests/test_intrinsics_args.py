"""What a CPU can check of the pinhole intrinsics (fx, fy, cx, cy): the three raygen_k exports, every refusal of the entry points
(they return before any HIP call: the pointers are dummies that are never dereferenced), ops.as_intrinsics, the refusals of render() /
render_poses() / PoseRefiner, refine.resized_intrinsics against float64 rays, and the second gradient all-reduce of
dist.render_sharded on two gloo ranks.  The GPU twin is tests/test_gpu_intrinsics.py."""
import ctypes as C
import os
import socket
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from nefes_amd import lib as L

BADARG = -1
PTR = C.c_void_p(4096)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nefes_raygen_k_fwd", "nefes_raygen_k_bwd_workspace", "nefes_raygen_k_bwd")


def test_names_are_declared_and_exported():
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "nefes_hip.h")).read()
    for name in NAMES:
        assert name in L.SIGNATURES and hasattr(lib, name) and name + "(" in hdr, name
    assert lib.nefes_version() == L.ABI_VERSION == 20
    assert "#define NEFES_ABI_VERSION 20" in hdr


def test_workspace_holds_sixteen_sums_per_block():
    q, q12 = L.load().nefes_raygen_k_bwd_workspace, L.load().nefes_raygen_bwd_workspace
    for n, blocks in ((1, 1), (256, 1), (257, 2), (33 * 65, 9), (262144, 1024), (262656, 1024), (1 << 24, 1024)):
        assert q(n) == blocks * 16 * 8 and q12(n) == blocks * 12 * 8, n


def test_refusals():
    lib = L.load()

    def fwd(H=6, W=8, intr=PTR, c2w=PTR, row0=0, nrows=6, o=PTR, d=PTR, v=PTR):
        return lib.nefes_raygen_k_fwd(H, W, intr, c2w, row0, nrows, o, d, v, None)

    def bwd(H=6, W=8, intr=PTR, c2w=PTR, row0=0, nrows=6, go=PTR, gd=PTR, gv=PTR, ws=PTR, g=PTR, gk=PTR):
        return lib.nefes_raygen_k_bwd(H, W, intr, c2w, row0, nrows, go, gd, gv, ws, g, gk, None)
    sizes = (dict(H=0), dict(H=-3), dict(W=0), dict(W=-1), dict(nrows=0), dict(nrows=-2), dict(row0=-1), dict(row0=1), dict(row0=5, nrows=2),
             dict(row0=6, nrows=1), dict(nrows=7))
    for call in (fwd, bwd):
        for kw in sizes + (dict(intr=None), dict(c2w=None)):
            assert call(**kw) == BADARG, (call.__name__, kw)
    for kw in (dict(o=None), dict(d=None)):
        assert fwd(**kw) == BADARG, kw
    for kw in (dict(ws=None), dict(g=None)):
        assert bwd(**kw) == BADARG, kw


def test_as_intrinsics_forms_and_refusals():
    from nefes_amd import ops
    t = torch.tensor([5., 6., 2., 3.])
    assert ops.as_intrinsics(t, "cpu") is t                                  # a float32 [4] tensor on the device: used as is
    for form in ((5, 6., 2, 3.), [5., 6., 2., 3.], np.array([5, 6, 2, 3]), torch.tensor([5., 6., 2., 3.], dtype=torch.float64),
                 [[5, 0, 2], [0, 6, 3], [0, 0, 1]], np.array([[5., 0, 2], [0, 6, 3], [0, 0, 1]]), torch.tensor([[5., 0, 2], [0, 6, 3], [0, 0, 1]])):
        k = ops.as_intrinsics(form, "cpu")
        assert k.dtype == torch.float32 and torch.equal(k, t), form
    bad = {"skew": [[5, 0.25, 2], [0, 6, 3], [0, 0, 1]], r"K\[1\]\[0\]": [[5, 0, 2], [1e-3, 6, 3], [0, 0, 1]],
           r"K\[2\]\[2\]": [[5, 0, 2], [0, 6, 3], [0, 0, 2]], r"K\[2\]\[0\]": [[5, 0, 2], [0, 6, 3], [0.5, 0, 1]],
           "fx = 0.0": (0, 6, 2, 3), "fy = -6.0": (5, -6, 2, 3), "fx = nan": (float("nan"), 6, 2, 3), "cy = inf": (5, 6, 2, float("inf")),
           "fy = inf": (5, float("inf"), 2, 3), "shape": (5, 6, 2), "fx = -1.0": [[-1, 0, 2], [0, 6, 3], [0, 0, 1]]}
    for match, form in bad.items():
        with pytest.raises(ValueError, match=match):
            ops.as_intrinsics(form, "cpu")
    with pytest.raises(ValueError, match="0.25"):                            # the offending value is named
        ops.as_intrinsics(bad["skew"], "cpu")


def test_render_refuses_ndc_and_caller_rays_before_touching_the_device():
    """Both raise on a machine without a GPU: nothing was allocated or launched before them."""
    from nefes_amd.render import render, render_poses
    kw = dict(N_samples=4, N_importance=4, network_fn=None, network_fine=None, use_viewdirs=True, near=0., far=4.)
    K = (7., 8., 3., 2.)
    rays = (torch.zeros(24, 3), torch.ones(24, 3))
    with pytest.raises(NotImplementedError, match="ndc"):
        render(4, 6, 7.0, c2w=torch.eye(4)[:3], intrinsics=K, ndc=True, **kw)
    with pytest.raises(NotImplementedError, match="ndc"):                     # ... and from inside the render kwargs, as the reference's loop calls it
        render(4, 6, 7.0, c2w=torch.eye(4)[:3], **dict(kw, intrinsics=K, ndc=True))
    with pytest.raises(ValueError, match="rays="):
        render(4, 6, 7.0, rays=rays, intrinsics=K, ndc=False, **kw)
    with pytest.raises(NotImplementedError, match="ndc"):
        render_poses(4, 6, 7.0, torch.eye(4)[None, :3], intrinsics=K, ndc=True, **kw)


def test_refiner_arguments():
    """Construction only, on the CPU device: it allocates buffers and launches nothing."""
    from nefes_amd.field import NeRFH_NFF
    from nefes_amd.refine import PoseRefiner
    coarse = NeRFH_NFF('coarse', W=128, f_dim=16).requires_grad_(False)
    args = types.SimpleNamespace(nerfh_nff=True, use_fine_only=False, NeRFW=True, transient_at_test=True, encode_hist=True)
    kw = dict(network_fn=coarse, network_fine=None, args=args)
    make = lambda **more: PoseRefiner(kw, args, (40, 60, 50.0), 0., 4., graph=False, device="cpu", **more)
    K = (13., 12., 7., 5.5)
    plain = make()
    assert plain.intrinsics is None and plain.log_f is None and plain._camera() == {} and plain.opt.flat.numel() == 6
    r = make(intrinsics=K)
    assert r.intrinsics.dtype == torch.float32 and r.intrinsics.tolist() == list(K) and r._camera()["intrinsics"] is r.intrinsics
    assert r.opt.flat.numel() == 6                                            # no new parameter without learn_focal
    own = torch.tensor(K)
    assert make(intrinsics=own).intrinsics.data_ptr() == own.data_ptr()       # the caller's tensor, not a copy
    assert tuple(make(images=2, intrinsics=[K, K]).intrinsics.shape) == (2, 4) and tuple(make(images=2, intrinsics=K).intrinsics.shape) == (4,)
    assert make(pose_model=torch.nn.Linear(12, 12), intrinsics=K).intrinsics.tolist() == list(K)
    with pytest.raises(ValueError):
        make(images=2, intrinsics=[K, K, K])
    with pytest.raises(ValueError, match="fx"):
        make(intrinsics=(0., 12., 7., 5.5))
    with pytest.raises(NotImplementedError, match="fused_glue"):
        make(intrinsics=K, fused_glue=False)
    f = make(learn_focal=True, lr_f=0.25)
    assert f.intrinsics.tolist() == [12.5, 12.5, 7.5, 5.0]                    # the centred camera of the rendered 10 x 15 frame
    assert f.log_f.shape == (1,) and float(f.log_f.detach()) == 0. and f.opt.flat.numel() == 7 and f.opt.lr.tolist() == [0.01] * 3 + [0.1] * 3 + [0.25]
    assert f.log_f.data_ptr() == f.opt.flat[6:].data_ptr() and f.log_f.grad.data_ptr() == f.opt.grad[6:].data_ptr()
    with torch.no_grad():
        f.log_f.fill_(0.5)
    k = f._camera()["intrinsics"]
    assert k.requires_grad and torch.equal(k[2:], f.intrinsics[2:])
    assert torch.allclose(k[:2].detach(), f.intrinsics[:2] * float(np.exp(0.5)), rtol=1e-6)
    f._reset(torch.eye(4), torch.zeros(16, 10, 15), torch.zeros(10))
    assert float(f.log_f) == 0.
    for more in (dict(images=2), dict(pose_model=torch.nn.Linear(12, 12)), dict(fused_glue=False), dict(lietorch=True)):
        with pytest.raises(NotImplementedError):
            make(learn_focal=True, **more)


def _rays64(h, w, K, cols=None, rows=None):
    """Camera-frame directions [(col - cx)/fx, -(row - cy)/fy, -1] in float64 at the given (possibly fractional) pixel positions."""
    fx, fy, cx, cy = (torch.as_tensor(v, dtype=torch.float64) for v in K)
    cols = torch.arange(w, dtype=torch.float64) if cols is None else cols
    rows = torch.arange(h, dtype=torch.float64) if rows is None else rows
    ii, jj = cols[None, :].expand(len(rows), len(cols)), rows[:, None].expand(len(rows), len(cols))
    return torch.stack([(ii - cx) / fx, -(jj - cy) / fy, -torch.ones_like(ii)], -1)


@pytest.mark.parametrize("full,small,K", [((240, 427), (60, 106), (372., 372., 213.5, 120.)),
                                          ((480, 640), (120, 160), (585., 590., 330.25, 236.5))])
def test_resized_intrinsics_keeps_every_pixels_ray(full, small, K):
    """The ray through pixel x of the resized image is the full-resolution ray at (x + 0.5) W / w - 0.5 (align_corners=False)."""
    from nefes_amd.refine import resized_intrinsics
    (H, W), (h, w) = full, small
    k = resized_intrinsics(K, full, small)
    K33 = [[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]]
    assert resized_intrinsics(K33, full, small) == k and resized_intrinsics(torch.tensor(K, dtype=torch.float64), full, small) == k
    cols = (torch.arange(w, dtype=torch.float64) + 0.5) * W / w - 0.5
    rows = (torch.arange(h, dtype=torch.float64) + 0.5) * H / h - 0.5
    assert float((_rays64(h, w, k) - _rays64(H, W, K, cols, rows)).abs().max()) < 1e-13
    if (H, W) == (480, 640):                                                  # an integer factor: division by 4 plus the half-pixel shift
        assert k == (K[0] / 4, K[1] / 4, (K[2] + 0.5) / 4 - 0.5, (K[3] + 0.5) / 4 - 0.5)
    else:                                                                     # the Cambridge numbers of INTEGRATION.md
        assert abs(k[0] - 372 * 106 / 427) < 1e-12 and k[1] == 93.0 and abs(k[2] - (214.0 * 106 / 427 - 0.5)) < 1e-12 and k[3] == 29.625
        assert abs(w / (2 * k[0]) - 427 / (2 * 372.)) < 1e-15                 # the query image's horizontal field of view, not 106 / (2 * 93)


# ---- dist.render_sharded(intrinsics=K): the camera's gradient is all-reduced like the pose's --------------------------------------
def _stand_in_render(H, W, focal, c2w=None, row_range=None, intrinsics=None, **kw):
    """A torch stand-in with render()'s call surface: rgb = a smooth function of this rank's rays."""
    row0, n = row_range
    d = torch.sum(_rays64(H, W, intrinsics)[row0:row0 + n, :, None, :] * c2w[:3, :3], -1).reshape(-1, 3)
    o = c2w[:3, 3].expand(d.shape)
    rgb = torch.sin(3. * d) + torch.cos(o * d.flip(-1))
    return [rgb, rgb[:, 0], rgb[:, 1], {"feat_map": rgb.repeat(1, 2)}]


def _problem():
    from oracle import ref_cpu as O
    return 7, 5, O.bench_pose(torch.float64).requires_grad_(), torch.tensor([6.1, 5.3, 2.9, 3.2], dtype=torch.float64, requires_grad=True)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    from nefes_amd import dist as D
    H, W, c2w, K = _problem()
    rgb, _, _, ex = D.render_sharded(_stand_in_render, H, W, 1.0, c2w, intrinsics=K)
    ((rgb ** 2).sum() / (H * W * 3) + (ex["feat_map"] ** 2).sum() / (H * W * 6)).backward()       # two all-reduces: 12 floats, 4 floats
    q.put((rank, c2w.grad.numpy().copy(), K.grad.numpy().copy(), rgb.shape[0]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_rank_intrinsics_gradient_equals_unsharded():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=240) for _ in procs], key=lambda t: t[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    H, W, c2w, K = _problem()
    rgb, _, _, ex = _stand_in_render(H, W, 1.0, c2w=c2w, row_range=(0, H), intrinsics=K)
    ((rgb ** 2).mean() + (ex["feat_map"] ** 2).mean()).backward()
    assert float(K.grad.abs().min()) > 0
    for rank, g_pose, g_k, n in got:
        assert n == (4, 3)[rank] * W
        assert torch.allclose(torch.from_numpy(g_k), K.grad, rtol=1e-12, atol=0), (rank, g_k, K.grad)         # identical on every rank
        assert torch.allclose(torch.from_numpy(g_pose), c2w.grad, rtol=1e-12, atol=1e-15), (rank, g_pose, c2w.grad)


def test_render_sharded_without_intrinsics_passes_no_keyword():
    from nefes_amd import dist as D
    seen = {}

    def fn(H, W, focal, **kw):
        seen.update(kw)
        return "out"
    assert D.render_sharded(fn, 6, 4, 3.5, torch.eye(4)[:3], rank=1, world=2, near=0.) == "out"
    assert "intrinsics" not in seen and seen["row_range"] == (3, 3) and seen["near"] == 0.
    K = torch.tensor([1., 2., 3., 4.])
    D.render_sharded(fn, 6, 4, 3.5, torch.eye(4)[:3], rank=0, world=2, intrinsics=K)
    assert seen["intrinsics"] is K                                            # no gradient asked for: passed through untouched

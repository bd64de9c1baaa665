"""What a CPU can check of rendering and refining at chosen pixels: the four exports (raygen_px forward / workspace / backward, sample_px),
every refusal of the entry points (they return before any HIP call: the pointers are dummies that are never dereferenced),
ops.as_pixels, the refusals of render(pixels=) / render_poses(pixels=) / PoseRefiner(sparse=), and the two float64 helpers of
tests/pixels_ref.py against rays_of and torch's grid_sample.  The GPU twin is tests/test_gpu_pixels.py."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from nefes_amd import lib as L
from tests import pixels_ref as R

BADARG = -1
PTR = C.c_void_p(4096)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nefes_raygen_px_fwd", "nefes_raygen_px_bwd_workspace", "nefes_raygen_px_bwd", "nefes_sample_px")


def test_names_are_declared_and_exported():
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "nefes_hip.h")).read()
    for name in NAMES:
        assert name in L.SIGNATURES and hasattr(lib, name) and name + "(" in hdr, name


def test_workspace_is_raygen_ks():
    q, qk = L.load().nefes_raygen_px_bwd_workspace, L.load().nefes_raygen_k_bwd_workspace
    for n, blocks in ((1, 1), (15, 1), (256, 1), (257, 2), (2305, 10), (262144, 1024), (1024 * 256 + 5, 1024), (1 << 24, 1024)):
        assert q(n) == qk(n) == blocks * 16 * 8, n


def test_refusals():
    lib = L.load()

    def fwd(n=48, px=PTR, intr=PTR, c2w=PTR, o=PTR, d=PTR, v=PTR):
        return lib.nefes_raygen_px_fwd(n, px, intr, c2w, o, d, v, None)

    def bwd(n=48, px=PTR, intr=PTR, c2w=PTR, go=PTR, gd=PTR, gv=PTR, ws=PTR, g=PTR, gk=PTR):
        return lib.nefes_raygen_px_bwd(n, px, intr, c2w, go, gd, gv, ws, g, gk, None)

    def smp(Cc=3, H=5, W=7, m=PTR, n=9, px=PTR, out=PTR):
        return lib.nefes_sample_px(Cc, H, W, m, n, px, out, None)
    for call in (fwd, bwd):
        for kw in (dict(n=0), dict(n=-4), dict(px=None), dict(intr=None), dict(c2w=None)):
            assert call(**kw) == BADARG, (call.__name__, kw)
    for kw in (dict(o=None), dict(d=None)):
        assert fwd(**kw) == BADARG, kw
    for kw in (dict(ws=None), dict(g=None)):
        assert bwd(**kw) == BADARG, kw
    for kw in (dict(Cc=0), dict(Cc=-1), dict(H=0), dict(W=0), dict(W=-2), dict(n=0), dict(n=-1), dict(m=None), dict(px=None), dict(out=None)):
        assert smp(**kw) == BADARG, kw


def test_as_pixels_forms_and_refusals():
    from nefes_amd import ops
    t = torch.tensor([[0., 0.], [2.5, 1.], [-3.5, 7.25]])
    assert ops.as_pixels(t, "cpu") is t                                      # a contiguous float32 [K, 2] tensor on the device: used as is
    for form in ([[0, 0], [2.5, 1], [-3.5, 7.25]], ((0., 0.), (2.5, 1.), (-3.5, 7.25)), t.numpy(), t.double(), t.half(),
                 t.t().contiguous().t()):
        p = ops.as_pixels(form, "cpu")
        assert p.dtype == torch.float32 and p.is_contiguous() and torch.equal(p, t), form
    ints = torch.tensor([[0, 0], [5, 3], [7, 2]])
    for form in (ints, ints.int(), ints.to(torch.uint8), ints.numpy(), ints.tolist()):
        p = ops.as_pixels(form, "cpu")
        assert p.dtype == torch.float32 and torch.equal(p, ints.float())
    for match, form in {"shape": [1., 2.], r"\(3, 3\)": np.zeros((3, 3)), r"\(2, 2, 2\)": torch.zeros(2, 2, 2), r"\(0, 2\)": torch.zeros(0, 2),
                        "pixel 1": [[0., 0.], [float("nan"), 1.]], "not finite": [[float("inf"), 1.]]}.items():
        with pytest.raises(ValueError, match=match):
            ops.as_pixels(form, "cpu")
    # on a device other than the host nothing is read back: anything but float32 (or integer) [K, 2] is refused, by dtype, shape and device
    for bad, match in ((torch.zeros(4, 2, dtype=torch.float64, device="meta"), "float64"), (torch.zeros(4, 3, device="meta"), r"\(4, 3\)"),
                       (torch.zeros(4, 2, dtype=torch.float16, device="meta"), "meta")):
        with pytest.raises(ValueError, match=match):
            ops.as_pixels(bad, "cpu")


def test_render_refuses_rays_row_range_and_ndc_before_touching_the_device():
    """All raise on a machine without a GPU: nothing was allocated or launched before them."""
    from nefes_amd.render import render, render_poses
    kw = dict(N_samples=4, N_importance=4, network_fn=None, network_fine=None, use_viewdirs=True, near=0., far=4.)
    px = [[0., 0.], [2.5, 1.], [5., 3.]]
    rays = (torch.zeros(3, 3), torch.ones(3, 3))
    with pytest.raises(ValueError, match="rays="):
        render(4, 6, 7.0, rays=rays, pixels=px, ndc=False, **kw)
    with pytest.raises(ValueError, match="row_range"):
        render(4, 6, 7.0, c2w=torch.eye(4)[:3], pixels=px, row_range=(0, 2), ndc=False, **kw)
    with pytest.raises(NotImplementedError, match="ndc"):
        render(4, 6, 7.0, c2w=torch.eye(4)[:3], pixels=px, ndc=True, **kw)
    with pytest.raises(NotImplementedError, match="ndc"):                     # ... and from inside the render kwargs, as the reference's loop calls it
        render(4, 6, 7.0, c2w=torch.eye(4)[:3], **dict(kw, pixels=px, ndc=True))
    with pytest.raises(NotImplementedError, match="ndc"):
        render_poses(4, 6, 7.0, torch.eye(4)[None, :3], pixels=px, ndc=True, **kw)


def test_sparse_refiner_arguments():
    """Construction only, on the CPU device: it allocates buffers and launches nothing."""
    from nefes_amd.field import NeRFH_NFF
    from nefes_amd.refine import PoseRefiner
    coarse = NeRFH_NFF('coarse', W=128, f_dim=16).requires_grad_(False)
    args = types.SimpleNamespace(nerfh_nff=True, use_fine_only=False, NeRFW=True, transient_at_test=True, encode_hist=True)
    kw = dict(network_fn=coarse, network_fine=None, args=args)
    make = lambda **more: PoseRefiner(kw, args, (40, 60, 50.0), 0., 4., graph=False, device="cpu", **more)
    plain = make()
    assert plain.sparse is None and not hasattr(plain, "pixels") and tuple(plain.target.shape) == (16, 10, 15)      # without sparse= nothing changes
    r = make(sparse=7)
    assert r.sparse == 7 and tuple(r.pixels.shape) == (7, 2) and r.pixels.dtype == torch.float32
    assert tuple(r.target.shape) == (16, 7) and r.mask is None
    assert r.intrinsics.tolist() == [12.5, 12.5, 7.5, 5.0] and r._camera()["intrinsics"] is r.intrinsics          # the centred camera of the 10 x 15 frame
    assert r.opt.flat.numel() == 6
    m = make(sparse=7, masked=True, per_pixel=True)
    assert tuple(m.mask.shape) == (1, 7) and m.mask.dtype == torch.uint8 and bool(m.mask.all())
    K = (13., 12., 7., 5.5)
    assert make(sparse=7, intrinsics=K).intrinsics.tolist() == list(K)
    f = make(sparse=7, learn_focal=True)
    assert f.opt.flat.numel() == 7 and f._camera()["intrinsics"].requires_grad
    for more in (dict(pose_model=torch.nn.Linear(12, 12)), dict(images=2), dict(upsample=True), dict(fused_glue=False), dict(lietorch=True)):
        with pytest.raises(NotImplementedError, match="sparse"):
            make(sparse=7, **more)
    with pytest.raises(ValueError):
        make(sparse=0)
    with pytest.raises(RuntimeError, match="sparse"):
        plain.set_pixels([[0., 0.]])
    with pytest.raises(ValueError, match="sparse"):
        plain.refine(torch.eye(4), torch.zeros(16, 10, 15), torch.zeros(10), 0, pixels=[[0., 0.]])
    with pytest.raises(RuntimeError, match="image"):                          # no image yet: nothing to sample the target from
        r.set_pixels(torch.zeros(7, 2))


def test_rays_at_is_rays_of_on_an_integer_grid():
    from tests.test_gpu_intrinsics import rays_of
    H, W = 5, 7
    K = torch.tensor([6.5, 5.8, 3.85, 2.25], dtype=torch.float64)
    c2w = torch.tensor([[0.8, -0.36, 0.48, 0.3], [0.6, 0.48, -0.64, -0.2], [0., 0.8, 0.6, 1.1]], dtype=torch.float64)
    for row0, n in ((0, H), (2, 1), (1, 3)):
        a, b = rays_of(H, W, K, c2w, row0, n), R.rays_at(R.grid_pixels(W, row0, n), K, c2w)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), (row0, n)


def test_bilinear_is_grid_sample_with_aligned_corners_and_border_padding():
    gen = torch.Generator().manual_seed(2)
    Cc, H, W = 3, 5, 7
    m = torch.randn(Cc, H, W, generator=gen, dtype=torch.float64)
    px = torch.cat([torch.rand(40, 2, generator=gen) * torch.tensor([W - 1., H - 1.]), R.grid_pixels(W, 0, H),
                    torch.tensor([[W - 1., H - 1.], [0., 0.], [W - 1., 1.5], [2.25, H - 1.]])])
    p = px.double()
    grid = torch.stack([2 * p[:, 0] / (W - 1) - 1, 2 * p[:, 1] / (H - 1) - 1], -1)[None, None]
    want = torch.nn.functional.grid_sample(m[None], grid, mode="bilinear", padding_mode="border", align_corners=True)[0, :, 0]
    got = R.bilinear(m, px)
    assert float((got - want).abs().max()) < 1e-13
    ints = R.grid_pixels(W, 0, H)
    assert torch.equal(R.bilinear(m, ints), m.reshape(Cc, -1))                # an integer coordinate: the map's own value
    out = torch.tensor([[-3.5, 2.], [W + 4., -1.], [3., H + 2.25]])           # out of frame: the border's value
    assert torch.equal(R.bilinear(m, out), torch.stack([m[:, 2, 0], m[:, 0, W - 1], m[:, H - 1, 3]], -1))

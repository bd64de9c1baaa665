"""What a CPU can check of the depth term (csrc/depth_loss.hip, nefes_sample_px_nearest; ops.depth_loss, PoseRefiner(depth_weight=)): the
exports, every refusal of the two new entry families (they return before any HIP call: the pointers are dummies that are never
dereferenced), the checks of ops.depth_loss that run before anything is launched, PoseRefiner's refusals (lambda <= 0, delta <= 0, a depth
frame of the wrong shape) and refine.resized_depth.  The GPU twin is tests/test_gpu_depth.py."""
import ctypes as C
import os
import types

import pytest
import torch

from nefes_amd import lib as L

BADARG, UNSUPPORTED = -1, -2
PTR = C.c_void_p(4096)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nefes_depth_loss_scratch_doubles", "nefes_depth_loss_fwd", "nefes_depth_loss_bwd", "nefes_sample_px_nearest")


def test_names_are_declared_and_exported():
    lib = L.load()
    hdr = open(os.path.join(ROOT, "include", "nefes_hip.h")).read()
    for name in NAMES:
        assert name in L.SIGNATURES and hasattr(lib, name) and name + "(" in hdr, name
    assert lib.nefes_version() == L.ABI_VERSION             # calls were added: the version stays
    assert L.SIGNATURES["nefes_sample_px_nearest"] == L.SIGNATURES["nefes_sample_px"]


def test_scratch_query():
    q = L.load().nefes_depth_loss_scratch_doubles
    assert q(0) == 0 and q(-3) == 0 and [q(G) for G in (1, 2, 3, 8, 65535)] == [2, 4, 6, 16, 131070]


def test_loss_refusals_come_before_any_hip_call():
    lib = L.load()

    def fwd(G=1, P=100, d=PTR, t=PTR, m=None, delta=0.1, weight=1.0, acc=0, s=PTR, l=PTR):
        return lib.nefes_depth_loss_fwd(G, P, d, t, m, delta, weight, acc, s, l, None)

    def bwd(G=1, P=100, d=PTR, t=PTR, m=None, delta=0.1, weight=1.0, s=PTR, g=PTR, o=PTR):
        return lib.nefes_depth_loss_bwd(G, P, d, t, m, delta, weight, s, g, o, None)
    nan, inf = float("nan"), float("inf")
    for call in (fwd, bwd):
        for kw in (dict(G=0), dict(G=-1), dict(G=65536), dict(P=0), dict(P=-7), dict(d=None), dict(t=None), dict(s=None), dict(delta=0.0),
                   dict(delta=-0.1), dict(delta=nan), dict(delta=inf), dict(weight=nan), dict(weight=inf), dict(weight=-inf)):
            assert call(**kw) == BADARG, kw
        for m in (None, PTR):                                  # the grid limit: one thread per pixel, 256 per block, 2^31 - 1 blocks
            assert call(G=1, P=(2 ** 31 - 1) * 256 + 1, m=m) == UNSUPPORTED
            assert call(G=3, P=((2 ** 31 - 1) * 256) // 3 + 1, m=m) == UNSUPPORTED
    assert fwd(l=None) == BADARG and fwd(l=None, acc=1) == BADARG
    assert bwd(g=None) == BADARG and bwd(o=None) == BADARG


def test_nearest_sampling_refusals_are_sample_pxs():
    lib = L.load()
    for fn in (lib.nefes_sample_px_nearest, lib.nefes_sample_px):
        call = lambda Cc=1, H=6, W=8, m=PTR, n=5, px=PTR, out=PTR: fn(Cc, H, W, m, n, px, out, None)
        for kw in (dict(Cc=0), dict(H=0), dict(W=-1), dict(n=0), dict(n=-2), dict(m=None), dict(px=None), dict(out=None)):
            assert call(**kw) == BADARG, kw


def test_ops_depth_loss_checks_run_before_anything_is_launched():
    from nefes_amd import ops
    disp, target = torch.rand(2, 50) + 0.2, torch.rand(2, 50) + 1.0
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="delta"):
            ops.depth_loss(disp, target, delta=bad)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="weight"):
            ops.depth_loss(disp, target, weight=bad)
    with pytest.raises(ValueError, match="`target`"):
        ops.depth_loss(disp, target[:, :49])
    with pytest.raises(ValueError, match="`target`"):
        ops.depth_loss(disp, target.double())
    with pytest.raises(ValueError, match="mask"):
        ops.depth_loss(disp, target, mask=torch.ones(2, 50))            # not uint8
    with pytest.raises(ValueError, match="mask"):
        ops.depth_loss(disp, target, mask=torch.ones(2, 49, dtype=torch.uint8))
    for bad in (torch.zeros(1), torch.zeros((), dtype=torch.float64), torch.zeros(()).requires_grad_(), 1.0):
        with pytest.raises(ValueError, match="`out`"):
            ops.depth_loss(disp, target, out=bad)
    with pytest.raises(ValueError, match="accumulate"):
        ops.depth_loss(disp, target, accumulate=True)
    with pytest.raises(RuntimeError, match="no CPU path"):                # good arguments get as far as the device check: no fall-back
        ops.depth_loss(disp, target, out=torch.zeros(()), accumulate=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.sample_pixels(torch.zeros(1, 6, 8), torch.zeros(3, 2), nearest=True)


def _make(**more):
    from nefes_amd.field import NeRFH_NFF
    from nefes_amd.refine import PoseRefiner
    coarse = NeRFH_NFF('coarse', W=128, f_dim=16).requires_grad_(False)
    args = types.SimpleNamespace(nerfh_nff=True, use_fine_only=False, NeRFW=True, transient_at_test=True, encode_hist=True)
    kw = dict(network_fn=coarse, network_fine=None, args=args)
    return PoseRefiner(kw, args, (40, 60, 50.0), 0., 4., graph=False, device="cpu", **more)


def test_refiner_validates_the_depth_term():
    """Construction only, on the CPU device: it allocates buffers and launches nothing."""
    plain = _make()
    assert plain.depth_weight is None and plain.depth_huber is None and plain.depth_loss is None and not hasattr(plain, "depth_target")
    r = _make(depth_weight=0.5, depth_huber=0.05)
    assert (r.depth_weight, r.depth_huber) == (0.5, 0.05) and tuple(r.depth_target.shape) == (1, 10 * 15)
    assert r.depth_loss.dtype == torch.float64 and r.depth_loss.shape == ()
    assert _make(depth_weight=1).depth_huber == 0.1
    assert tuple(_make(depth_weight=1., images=2).depth_target.shape) == (2, 150) and _make(depth_weight=1., images=2).depth_loss.shape == (2,)
    s = _make(depth_weight=1., sparse=40)
    assert tuple(s.depth_target.shape) == (1, 40) and tuple(s._depth_frame.shape) == (1, 10, 15)
    for bad in (0, 0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="depth_weight"):
            _make(depth_weight=bad)
        with pytest.raises(ValueError, match="depth_huber"):
            _make(depth_weight=1.0, depth_huber=bad)
    with pytest.raises(ValueError, match="depth_huber"):
        _make(depth_huber=0.1)                                            # a threshold without a term
    with pytest.raises(NotImplementedError, match="fused_glue"):
        _make(depth_weight=1.0, fused_glue=False)


def test_refiner_refuses_a_wrong_depth_frame():
    eye, tgt, hist = torch.eye(4), torch.zeros(16, 10, 15), torch.zeros(10)
    r = _make(depth_weight=1.0)
    for shape in ((40, 60), (15, 10), (2, 10, 15), (150,)):
        with pytest.raises(ValueError, match=r"shape \(" + ", ".join(str(v) for v in shape) + r",?\).*\(10, 15\)"):
            r.refine(eye, tgt, hist, iters=1, depth=torch.ones(shape))
        with pytest.raises(ValueError, match=r"\(10, 15\)"):
            r._reset(eye, tgt, hist, None, None, torch.ones(shape))
    with pytest.raises(ValueError, match="depth="):
        r.refine(eye, tgt, hist, iters=1)                                 # built with the term, no frame given
    for holes in (torch.zeros(10, 15), torch.full((10, 15), float("nan")), torch.full((10, 15), float("inf")), -torch.ones(10, 15)):
        with pytest.raises(ValueError, match="no valid pixel"):
            r._reset(eye, tgt, hist, None, None, holes)
    b = _make(depth_weight=1.0, images=2)
    with pytest.raises(ValueError, match=r"\[2, 10, 15\]"):
        b.refine(eye[None].repeat(2, 1, 1), tgt[None].repeat(2, 1, 1, 1), hist[None].repeat(2, 1), iters=1, depth=torch.ones(10, 15))
    one_empty = torch.ones(2, 10, 15)
    one_empty[1] = 0
    with pytest.raises(ValueError, match=r"image\(s\) \[1\]"):
        b._reset(eye[None].repeat(2, 1, 1), tgt[None].repeat(2, 1, 1, 1), hist[None].repeat(2, 1), None, None, one_empty)
    with pytest.raises(ValueError, match="depth_weight"):
        _make().refine(eye, tgt, hist, iters=1, depth=torch.ones(10, 15))  # a frame for a refiner without the term


def test_resized_depth_takes_the_nearest_source_pixel_to_each_centre():
    from nefes_amd.refine import resized_depth, resized_intrinsics
    H, W, h, w = 480, 640, 60, 80
    D = torch.arange(H * W, dtype=torch.float32).reshape(H, W)
    d = resized_depth(D, (H, W), (h, w))
    assert d.shape == (h, w)
    for y, x in ((0, 0), (59, 79), (17, 33)):                            # the centre of (x, y) lies at ((x + .5) W / w, (y + .5) H / h)
        assert d[y, x] == D[int((y + 0.5) * H / h), int((x + 0.5) * W / w)]
    # resized_intrinsics' convention: rendered pixel x looks where source coordinate (x + 0.5) W / w - 0.5 does: the nearest pixel to it
    fx, fy, cx, cy = resized_intrinsics((500., 500., 319.5, 239.5), (H, W), (h, w))
    for x in (0, 33, 79):
        src = (x + 0.5) * W / w - 0.5
        assert abs(float(d[0, x] - D[int((0 + 0.5) * H / h), 0]) - src) <= 0.5
    assert torch.equal(resized_depth(D, (H, W), (H, W)), D)             # same size: the frame itself
    odd = resized_depth(D[:7, :5], (7, 5), (3, 2))                       # no multiple: rows floor((2y+1) 7 / 6), columns floor((2x+1) 5 / 4)
    assert torch.equal(odd, D[:7, :5][[1, 3, 5]][:, [1, 3]])
    assert resized_depth(torch.zeros(2, 7, 5), (7, 5), (3, 2)).shape == (2, 3, 2)
    with pytest.raises(ValueError, match="from_hw"):
        resized_depth(D, (H, W + 1), (h, w))

"""Ray generation on the GPU, all three forms of the one kernel body (csrc/rays.hip): the focal, intrinsics and pixel-list entry points
bit for bit against the independent numpy float32 forward of tests/rays_ref.py (held to float64 by tests/test_rays_ref.py) -- rays_o and
rays_d whole, viewdirs per ray up to the one float the hardware's square root leaves open (`same` below) -- and the one autograd Function
behind ops.rays against the direct backward calls.  The focal-vs-intrinsics and grid-vs-list comparisons of
tests/test_gpu_intrinsics.py and tests/test_gpu_pixels.py compare instances of that body with each other; this file anchors the body."""
import pytest
import torch

from oracle import ref_cpu as O
from tests import pixels_ref as R
from tests import rays_ref as N
from tests.test_gpu_intrinsics import DEV, centred, dev, off_centre, upstream
from tests.test_gpu_pixels import subpixel_list

pytestmark = pytest.mark.gpu
T = torch.from_numpy


@pytest.fixture(scope="module")
def ops():
    from nefes_amd import ops as _ops
    return _ops


def same(got, want, what):
    """rays_o and rays_d equal the reference's; every ray's viewdirs equal one of the reference's three candidates for it (the norm is
    the hardware's square root, one of three neighbouring floats: tests/rays_ref.py)."""
    for name, g, w in zip(("rays_o", "rays_d"), got, want):
        assert torch.equal(g.cpu(), T(w)), (what, name)
    hit = (got[2].cpu()[None] == T(N.viewdirs_candidates(want[1]))).all(-1)
    print(f"[raygen {what}] rays whose norm is below / at / above the correctly rounded root: {hit.sum(1).tolist()} of {hit.shape[1]}")
    assert bool(hit.any(0).all()), (what, "viewdirs", int((~hit.any(0)).sum()))


# ---- the forward against the numpy float32 reference, bit for bit -------------------------------------------------------------------
@pytest.mark.parametrize("H,W,f,shards", [(6, 8, 7.3, [(0, 6)]), (10, 7, 9.1, [(0, 3), (3, 3), (6, 4)]), (33, 65, 58.0, [(11, 1)])])
def test_grids_are_the_float32_reference_bit_for_bit(ops, H, W, f, shards):
    c2w = O.bench_pose()
    for row0, n in shards:
        x, y = N.grid_xy(W, row0, n)
        px = R.grid_pixels(W, row0, n).to(DEV)
        want = N.rays(x, y, N.centred(H, W, f), c2w.numpy())
        same(ops.raygen_fwd(H, W, f, c2w.to(DEV), row0, n), want, ("focal", row0, n))
        for name, K in (("centred", centred(H, W, f)), ("off-centre", off_centre(H, W, f))):
            want = N.rays(x, y, K.numpy(), c2w.numpy())
            same(ops.raygen_k_fwd(H, W, K.to(DEV), c2w.to(DEV), row0, n), want, ("intrinsics", name, row0, n))
            same(ops.raygen_px_fwd(px, K.to(DEV), c2w.to(DEV)), want, ("list", name, row0, n))


@pytest.mark.parametrize("n", [1, 15, 257])
def test_subpixel_lists_are_the_float32_reference_bit_for_bit(ops, n):
    H, W, f = 33, 65, 58.0
    c2w, K, px = O.bench_pose(), off_centre(H, W, f), subpixel_list(n, H, W, seed=n)
    want = N.rays(px[:, 0].numpy(), px[:, 1].numpy(), K.numpy(), c2w.numpy())
    same(ops.raygen_px_fwd(px.to(DEV), K.to(DEV), c2w.to(DEV)), want, n)


# ---- the one Function -------------------------------------------------------------------------------------------------------------
H, W, FOCAL = 10, 7, 9.1


def leaf(t):
    return t.to(DEV).requires_grad_()


def through(ops, c2w, g, **camera_and_pixels):
    torch.autograd.backward(ops.rays(c2w, H, W, **camera_and_pixels), [dev(t) for t in g])


def test_focal_gradient_is_raygen_bwd(ops):
    c2w, g = leaf(O.bench_pose()), upstream(H * W)
    through(ops, c2w, g, focal=FOCAL)
    assert torch.equal(c2w.grad, ops.raygen_bwd(H, W, FOCAL, c2w.detach(), 0, H, *map(dev, g)))


def test_intrinsics_gradients_are_raygen_k_bwd(ops):
    c2w, K, g = leaf(O.bench_pose()), leaf(off_centre(H, W, FOCAL)), upstream(H * W)
    through(ops, c2w, g, intr=K)
    g12, g4 = ops.raygen_k_bwd(H, W, K.detach(), c2w.detach(), 0, H, *map(dev, g))
    assert torch.equal(c2w.grad, g12) and torch.equal(K.grad, g4)


def test_list_gradients_are_raygen_px_bwd_and_the_pixels_get_none(ops):
    n = 15
    c2w, K, px, g = leaf(O.bench_pose()), leaf(off_centre(33, 65, 58.0)), leaf(subpixel_list(n, 33, 65, seed=n)), upstream(n)
    through(ops, c2w, g, intr=K, px=px)
    g12, g4 = ops.raygen_px_bwd(px.detach(), K.detach(), c2w.detach(), *map(dev, g))
    assert torch.equal(c2w.grad, g12) and torch.equal(K.grad, g4)
    assert px.grad is None


@pytest.mark.parametrize("form", ["focal", "intrinsics", "list"])
def test_a_4x4_float64_pose_gets_a_gradient_of_its_own_kind(ops, form):
    n = 15
    K, px = off_centre(H, W, FOCAL).to(DEV), subpixel_list(n, H, W, seed=n).to(DEV)
    kw = {"focal": dict(focal=FOCAL), "intrinsics": dict(intr=K), "list": dict(intr=K, px=px)}[form]
    g = upstream(n if form == "list" else H * W)
    pose = torch.eye(4, dtype=torch.float64)
    pose[:3, :4] = O.bench_pose()
    c34, c44 = leaf(O.bench_pose()), leaf(pose)
    through(ops, c34, g, **kw)
    through(ops, c44, g, **kw)
    assert c44.grad.dtype == torch.float64 and tuple(c44.grad.shape) == (4, 4)
    assert torch.equal(c44.grad[:3], c34.grad.double()) and torch.equal(c44.grad[3], torch.zeros(4, dtype=torch.float64, device=DEV))


@pytest.mark.parametrize("form", ["intrinsics", "list"])
def test_a_camera_that_asks_for_no_gradient_gets_none(ops, form):
    n = 15
    K, px = off_centre(H, W, FOCAL).to(DEV), subpixel_list(n, H, W, seed=n).to(DEV)
    c2w, g = leaf(O.bench_pose()), upstream(n if form == "list" else H * W)
    through(ops, c2w, g, intr=K, **(dict(px=px) if form == "list" else {}))
    if form == "list":
        g12, none = ops.raygen_px_bwd(px, K, c2w.detach(), *map(dev, g), want_intr=False)
    else:
        g12, none = ops.raygen_k_bwd(H, W, K, c2w.detach(), 0, H, *map(dev, g), want_intr=False)
    assert K.grad is None and none is None and torch.equal(c2w.grad, g12)


def test_a_focal_length_with_a_pixel_list_is_refused(ops):
    c2w, px = leaf(O.bench_pose()), subpixel_list(15, H, W, seed=15).to(DEV)
    with pytest.raises(ValueError, match="as_intrinsics"):
        ops.rays(c2w, H, W, focal=FOCAL, px=px)

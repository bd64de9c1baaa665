"""The numpy float32 forward of tests/rays_ref.py against the float64 rays (rays_of on a grid, pixels_ref.rays_at on a list) within the
project's ray bound, rtol 3e-7, atol 1e-7 -- the reference tests/test_gpu_rays.py holds the kernels to bit for bit is itself held to
float64 here, without a GPU -- and the one refusal of ops.rays that needs no device."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from tests import pixels_ref as R
from tests import rays_ref as N
from tests.test_gpu_intrinsics import centred, off_centre, rays_of
from tests.test_gpu_pixels import subpixel_list

GRIDS = [(6, 8, 7.3, (0, 6)), (10, 7, 9.1, (0, 3)), (10, 7, 9.1, (3, 3)), (10, 7, 9.1, (6, 4)), (33, 65, 58.0, (11, 1)), (33, 65, 58.0, (0, 33))]


def close(got, want):
    for g, w in zip(got, want):
        assert g.dtype == np.float32
        np.testing.assert_allclose(g, w.numpy(), rtol=3e-7, atol=1e-7)


def test_centred_is_the_torch_float32_camera():
    for H, W, f in ((6, 8, 7.3), (5, 7, 6.1), (33, 65, 58.0)):
        assert np.array_equal(N.centred(H, W, f), centred(H, W, f).numpy())


@pytest.mark.parametrize("camera", [centred, off_centre])
@pytest.mark.parametrize("H,W,f,rows", GRIDS)
def test_grid_matches_float64(H, W, f, rows, camera):
    c2w, K = O.bench_pose(), camera(H, W, f)
    x, y = N.grid_xy(W, *rows)
    assert np.array_equal(np.stack([x, y], -1), R.grid_pixels(W, *rows).numpy())
    close(N.rays(x, y, K.numpy(), c2w.numpy()), rays_of(H, W, K.double(), c2w.double(), *rows))


@pytest.mark.parametrize("n", [1, 15, 257, 2305])
def test_subpixel_lists_match_float64(n):
    H, W, f = 33, 65, 58.0
    c2w, K, px = O.bench_pose(), off_centre(H, W, f), subpixel_list(n, H, W, seed=n)
    close(N.rays(px[:, 0].numpy(), px[:, 1].numpy(), K.numpy(), c2w.numpy()), R.rays_at(px, K.double(), c2w.double()))


def test_a_focal_length_with_a_pixel_list_is_refused():
    """Before anything touches a device: the tensors are the host's."""
    from nefes_amd import ops
    with pytest.raises(ValueError, match="as_intrinsics"):
        ops.rays(O.bench_pose(), 33, 65, focal=58.0, px=subpixel_list(15, 33, 65, seed=15))
    with pytest.raises(ValueError, match="as_intrinsics"):
        ops.raygen_px_fwd(subpixel_list(15, 33, 65, seed=15), 58.0, O.bench_pose())
    with pytest.raises(ValueError, match="focal= or intr="):
        ops.rays(O.bench_pose(), 33, 65)

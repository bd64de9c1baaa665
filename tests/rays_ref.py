"""The forward of ray generation (csrc/rays.hip, raygen_fwd_kernel) restated in numpy float32, one IEEE operation per step and in the
kernel's order, so that the kernels can be held to it bit for bit: numpy's elementwise float32 -, /, *, + and sqrt are correctly
rounded and never fused.  Independent of the kernels and of torch; tests/test_rays_ref.py holds it to the float64 rays, tests/test_gpu_rays.py
holds the three forms of the kernel to it.

One operation of the kernel is not IEEE's: __fsqrt_rn compiles to the hardware's v_sqrt_f32 (the header maps it to the native square
root; the kernel's disassembly shows the bare instruction), which is specified to 1 ulp, not correctly rounded, and which no host can
restate.  So rays_o and rays_d are held to `rays` bit for bit, and viewdirs to `viewdirs_candidates`: per ray, the three correctly
rounded quotients d / nrm for ONE of the three floats the instruction may return -- the correctly rounded root and its two neighbours."""
import numpy as np

F = np.float32


def centred(H, W, focal):
    """The camera of the focal entry points: (focal, focal, W/2, H/2), each half a double product converted once."""
    return np.array([focal, focal, W * .5, H * .5], dtype=F)


def grid_xy(W, row0, nrows):
    """(x, y) = (column, row) of the row-major pixels of rows [row0, row0 + nrows): the integers the grid kernels convert."""
    idx = np.arange(nrows * W)
    return (idx % W).astype(F), (row0 + idx // W).astype(F)


def rays(x, y, K, c2w):
    """x, y float32 [n]; K = (fx, fy, cx, cy); c2w [3, 4] -> (rays_o, rays_d, viewdirs), float32 [n, 3] each."""
    x, y, K, c2w = (np.ascontiguousarray(a, dtype=F) for a in (x, y, K, c2w))
    fx, fy, cx, cy = K
    dc0 = (x - cx) / fx                                       # subtract, divide
    dc1 = -((y - cy) / fy)                                    # subtract, divide, negate
    dc2 = np.full_like(x, -1)
    d = []
    for a in range(3):                                        # three products and two adds per axis
        p0, p1, p2 = dc0 * c2w[a, 0], dc1 * c2w[a, 1], dc2 * c2w[a, 2]
        d.append((p0 + p1) + p2)
    nrm = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])  # squares, two adds, sqrt
    rays_d = np.stack(d, -1)
    viewdirs = np.stack([c / nrm for c in d], -1)             # divide
    assert rays_d.dtype == F and viewdirs.dtype == F
    return np.broadcast_to(c2w[:, 3], rays_d.shape).copy(), rays_d, viewdirs


def viewdirs_candidates(rays_d):
    """float32 [3, n, 3]: rays_d / nrm, each quotient correctly rounded, for nrm = the lower neighbour of the correctly rounded root of
    (d0 d0 + d1 d1) + d2 d2, that root, and its upper neighbour.  A kernel's viewdirs must equal one of the three, whole rays at a time."""
    d = np.ascontiguousarray(rays_d, dtype=F)
    nrm = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    return np.stack([d / r[:, None] for r in (np.nextafter(nrm, F(0)), nrm, np.nextafter(nrm, F(np.inf)))])

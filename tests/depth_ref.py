"""numpy float64 restatement of the depth loss (csrc/depth_loss.hip) and of nearest sampling (nefes_sample_px_nearest), for the tests.
tests/test_depth_ref.py pins it against torch float64 autograd (SmoothL1Loss(beta=delta) on 1/disp - target over the valid set); the GPU
tests compare the kernels with it."""
import numpy as np


def valid(disp, target, mask=None):
    """A pixel is valid iff target is finite and > 0, disp is finite and > 0, and its mask byte (if any) is != 0."""
    with np.errstate(invalid="ignore"):
        v = np.isfinite(target) & (target > 0) & np.isfinite(disp) & (disp > 0)
    return v if mask is None else v & (np.asarray(mask) != 0)


def depth_loss(disp, target, mask=None, delta=0.1, weight=1.0, g_loss=1.0, base=None):
    """disp, target [G, P] float32 (mask uint8 [G, P] or None) -> (value, per-group values L_g [G], g_disp [G, P]), all float64.
    value = weight * sum_g L_g (+ base, the float32 number an accumulating call finds); g_disp = g_loss * d value / d disp."""
    disp32, target32 = np.asarray(disp, np.float32), np.asarray(target, np.float32)
    G, P = disp32.shape
    v = valid(disp32, target32, mask)
    d, t = disp32.astype(np.float64), target32.astype(np.float64)
    groups, grad = np.zeros(G), np.zeros((G, P))
    for g in range(G):
        idx = np.nonzero(v[g])[0]
        if idx.size == 0:
            continue
        e = 1.0 / d[g, idx] - t[g, idx]
        quad = np.abs(e) <= delta
        rho = np.where(quad, e * e / (2.0 * delta), np.abs(e) - 0.5 * delta)
        groups[g] = rho.sum() / idx.size
        drho = np.where(quad, e / delta, np.sign(e))
        grad[g, idx] = float(g_loss) * weight * drho / idx.size * (-1.0 / (d[g, idx] * d[g, idx]))
    value = weight * groups.sum()
    if base is not None:
        value = float(np.float32(base)) + value
    return value, groups, grad


def sample_nearest(m, px):
    """m [C, H, W], px [n, 2] float32 rows of (x, y) -> [C, n]: the tap (clamp(floor(x + 0.5), 0, W-1), clamp(floor(y + 0.5), 0, H-1)),
    the sum in float64 (exact for a float32 coordinate); a NaN coordinate reads column / row 0."""
    m, px = np.asarray(m), np.asarray(px, np.float32).astype(np.float64)
    C, H, W = m.shape

    def tap(c, n):
        with np.errstate(invalid="ignore"):
            f = np.floor(c + 0.5)
        f = np.where(np.isnan(f), 0.0, f)
        return np.clip(f, 0, n - 1).astype(np.int64)
    return m[:, tap(px[:, 1], H), tap(px[:, 0], W)]


def within_one_ulp(got, ref64):
    """|got - ref| <= 2^-23 |ref| elementwise: float32 `got` against the float64 result -- one rounding of double arithmetic."""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    return bool(np.all(np.abs(got - ref64) <= 2.0 ** -23 * np.abs(ref64)))

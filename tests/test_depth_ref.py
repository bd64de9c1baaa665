"""tests/depth_ref.py (the float64 restatement the GPU tests of the depth loss compare with) pinned against torch float64 autograd:
torch.nn.SmoothL1Loss(beta=delta, reduction='mean') on 1/disp - target over the valid set, per group; and nearest sampling against a
direct loop.  No GPU."""
import numpy as np
import pytest
import torch

from tests import depth_ref as D


def torch_loss(disp, target, mask, delta, weight):
    """-> (value, per-group values, d value / d disp) by autograd over the compacted valid set (float64)."""
    d = torch.from_numpy(np.asarray(disp, np.float32)).double().requires_grad_()
    t = torch.from_numpy(np.asarray(target, np.float32)).double()
    v = torch.isfinite(t) & (t > 0) & torch.isfinite(d.detach()) & (d.detach() > 0)
    if mask is not None:
        v = v & (torch.from_numpy(np.asarray(mask)) != 0)
    crit = torch.nn.SmoothL1Loss(beta=delta, reduction="mean")
    groups = []
    for g in range(d.shape[0]):
        idx = v[g].nonzero().flatten()
        groups.append(crit(1.0 / d[g, idx], t[g, idx]) if idx.numel() else d[g, idx].sum())      # (no valid pixel: 0, zero gradient)
    total = weight * torch.stack(groups).sum()
    (grad,) = torch.autograd.grad(total, d)
    return float(total.detach()), torch.stack(groups).detach().numpy(), grad.numpy()


def case(G, P, seed, delta):
    rng = np.random.default_rng(seed)
    target = rng.uniform(0.5, 3.5, (G, P)).astype(np.float32)
    # residuals on both sides of delta, both signs
    e = rng.uniform(-3 * delta, 3 * delta, (G, P))
    disp = (1.0 / (target + e)).astype(np.float32)
    return disp, target


@pytest.mark.parametrize("G,P", [(1, 1), (1, 65), (3, 257)])
def test_both_branches_against_autograd(G, P):
    delta, weight = 0.07, 1.7
    disp, target = case(G, P, 11 + P, delta)
    e = 1.0 / disp.astype(np.float64) - target
    if P > 1:
        assert (np.abs(e) < delta).any() and (np.abs(e) > delta).any() and (e > delta).any() and (e < -delta).any()
    val, groups, grad = D.depth_loss(disp, target, None, delta, weight)
    tv, tg, tgrad = torch_loss(disp, target, None, delta, weight)
    assert abs(val - tv) <= 1e-13 * abs(tv)
    np.testing.assert_allclose(groups, tg, rtol=1e-13, atol=0)
    np.testing.assert_allclose(grad, tgrad, rtol=1e-12, atol=0)


def test_residual_exactly_delta():
    """|e| = delta exactly (binary fractions: 1/disp, target and delta are exact): both branches give delta / 2 and slope +-1."""
    disp = np.array([[0.5, 0.25, 0.5]], np.float32)            # depths 2, 4, 2
    target = np.array([[1.75, 4.25, 2.0]], np.float32)         # e = 0.25, -0.25, 0
    val, groups, grad = D.depth_loss(disp, target, None, 0.25, 1.0)
    assert groups[0] == (0.125 + 0.125 + 0.0) / 3 and val == groups[0]
    np.testing.assert_array_equal(grad[0], np.array([1.0, -1.0, 0.0]) / 3 * (-1.0 / disp[0].astype(np.float64) ** 2))
    tv, tg, tgrad = torch_loss(disp, target, None, 0.25, 1.0)
    assert val == tv and np.array_equal(grad, tgrad)


def test_holes_nan_disp_and_mask():
    delta, weight = 0.1, 0.5
    disp, target = case(3, 130, 5, delta)
    target[0, [0, 7, 64]] = (0.0, np.inf, np.nan)              # sensor holes
    target[0, 9] = -1.0
    disp[0, [3, 65]] = (np.nan, 0.0)                           # a ray without density; a non-positive disparity
    disp[0, 66] = -0.3
    disp[0, 67] = np.inf
    target[1, :] = 0.0                                         # a group without a valid pixel
    mask = (np.random.default_rng(3).random((3, 130)) > 0.4).astype(np.uint8)
    for mk in (None, mask):
        val, groups, grad = D.depth_loss(disp, target, mk, delta, weight)
        tv, tg, tgrad = torch_loss(disp, target, mk, delta, weight)
        assert np.isfinite(val) and abs(val - tv) <= 1e-13 * abs(tv)
        np.testing.assert_allclose(groups, tg, rtol=1e-13, atol=0)
        np.testing.assert_allclose(grad, tgrad, rtol=1e-12, atol=0)
        assert groups[1] == 0 and not grad[1].any()
        inv = ~D.valid(disp, target, mk)
        assert inv[0, [0, 7, 64, 9, 3, 65, 66, 67]].all() and not grad[inv].any()
    # an all-ones mask is no mask; the value at an invalid pixel is never combined
    a = D.depth_loss(disp, target, np.ones_like(mask), delta, weight)
    b = D.depth_loss(disp, target, None, delta, weight)
    assert a[0] == b[0] and np.array_equal(a[2], b[2])
    t2 = target.copy()
    t2[0, 0], t2[0, 7] = np.nan, -np.inf
    c = D.depth_loss(disp, t2, None, delta, weight)
    assert c[0] == b[0] and np.array_equal(c[2], b[2])


def test_g_loss_and_accumulate():
    disp, target = case(2, 70, 2, 0.1)
    v1, _, g1 = D.depth_loss(disp, target, None, 0.1, 2.0)
    v2, _, g2 = D.depth_loss(disp, target, None, 0.1, 2.0, g_loss=-0.75, base=np.float32(0.3))
    assert v2 == float(np.float32(0.3)) + v1
    np.testing.assert_allclose(g2, -0.75 * g1, rtol=1e-15, atol=0)      # (the same products in another order)


@pytest.mark.parametrize("tag", ["metric", "metric_B", "ref_default", "ref_default_B"])
def test_every_ray_of_the_end_to_end_fixture_hits_something(golden, tag):
    """The reference's disp of tests/golden/end_to_end.npz is finite with acc = 1 +- 2e-7 on every ray: tests/test_gpu_depth.py excludes
    no ray from its depth comparisons on these scenes."""
    g = golden("end_to_end")
    assert np.isfinite(g[f"{tag}.disp"]).all() and (g[f"{tag}.disp"] > 0).all() and np.abs(g[f"{tag}.acc"] - 1).max() <= 2e-7


def test_nearest_sampling():
    rng = np.random.default_rng(0)
    m = rng.standard_normal((3, 5, 7)).astype(np.float32)
    px = np.array([[0, 0], [6, 4], [2.4, 1.6], [2.5, 1.5], [3.5, 2.5], [-0.5, -0.51], [-3, 9], [6.49, 4.49], [6.5, 4.5], [1e9, -1e9],
                   [np.nan, 2], [0.49999997, 0.5]], np.float32)
    want = [(0, 0), (6, 4), (2, 2), (3, 2), (4, 3), (0, 0), (0, 4), (6, 4), (6, 4), (6, 0), (0, 2), (0, 1)]
    got = D.sample_nearest(m, px)
    assert got.shape == (3, len(px))
    for i, (x, y) in enumerate(want):
        assert np.array_equal(got[:, i], m[:, y, x]), (i, px[i])

"""refine.masked_feature_loss -- the select form of the reference's masked_feature_loss (dm/DFM_pose_refine.py:257-288, `--semantic`) that
the refinement loop can replay, and what the masked kernels are compared with -- against tests/golden/masked_loss.npz: the REFERENCE's
own function (torch.nonzero, then CosineSimilarity over the compacted maps) on two shapes x three masks x both forms
(tools/make_golden_masked_loss.py).  Bounds: 1e-6 on the float32 evaluation (a number below 1: a few ulp of summation order between the
compacted and the select form), 1e-12 on the float64 re-evaluation."""
import numpy as np
import pytest
import torch

from nefes_amd.refine import feature_loss, masked_feature_loss

T32, T64 = 1e-6, 1e-12


def cases(golden):
    g = golden("masked_loss")
    for ci, (C, H, W) in enumerate(g["cases"].tolist()):
        key = f"{C}x{H}x{W}"
        a = torch.from_numpy(g[f"a_{key}"].astype(np.float32)) / float(g["scale"])
        b = torch.from_numpy(g[f"b_{key}"].astype(np.float32)) / float(g["scale"])
        for mi, kind in enumerate(g["masks"].tolist()):
            m = torch.from_numpy(g[f"mask_{kind}_{key}"])
            for pp in (False, True):
                yield f"{key} {kind} {'pixel' if pp else 'channel'}", a, b, m, pp, float(g["ref32"][ci, mi, int(pp)]), float(g["ref64"][ci, mi, int(pp)])


def test_fixture_is_what_the_issue_describes(golden):
    g = golden("masked_loss")
    assert g["cases"].tolist() == [[5, 6, 7], [16, 15, 20]] and g["masks"].tolist() == ["random", "single", "ones"]
    for C, H, W in g["cases"].tolist():
        key = f"{C}x{H}x{W}"
        frac = float(g[f"mask_random_{key}"].mean())
        assert 0.5 < frac < 0.7 and int(g[f"mask_single_{key}"].sum()) == 1 and bool(g[f"mask_ones_{key}"].all()), (key, frac)
        assert g[f"mask_random_{key}"].shape == (1, H, W) and g[f"mask_random_{key}"].dtype == np.uint8


def test_select_form_equals_the_reference(golden):
    n = 0
    for tag, a, b, m, pp, ref32, ref64 in cases(golden):
        l32 = float(masked_feature_loss(a, b, m, per_pixel=pp))
        l64 = float(masked_feature_loss(a.double(), b.double(), m, per_pixel=pp))
        print(f"{tag:30s} fp32 {abs(l32 - ref32):.2e}  float64 {abs(l64 - ref64):.2e}")
        assert abs(l32 - ref32) <= T32 and abs(l64 - ref64) <= T64, (tag, l32, ref32, l64, ref64)
        # any mask dtype and the [H,W] / flat shapes give the same number
        for mm in (m.bool(), m.float() * 0.25, m[0], m.reshape(-1).double()):
            assert float(masked_feature_loss(a, b, mm, per_pixel=pp)) == l32, tag
        n += 1
    assert n == 12


def test_all_ones_is_the_unmasked_loss(golden):
    for tag, a, b, m, pp, ref32, ref64 in cases(golden):
        if " ones " in tag:
            assert abs(float(feature_loss(a.double(), b.double(), per_pixel=pp)) - ref64) <= T64, tag


def test_a_mean_over_all_pixels_is_caught(golden):
    """The inputs discriminate: the deliberately wrong per-pixel variant -- sum of the valid cosines over ALL pixels instead of over the
    valid ones -- lands at least 10x over the bound wherever the mask is not all ones."""
    seen = 0
    for tag, a, b, m, pp, ref32, ref64 in cases(golden):
        if not pp or " ones " in tag:
            continue
        v = m.reshape(-1) > 0
        cos = torch.nn.CosineSimilarity(dim=0, eps=1e-6)(a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1))
        wrong = float(1 - (cos * v).sum() / v.numel())
        assert abs(wrong - ref32) >= 10 * T32, (tag, wrong, ref32)
        seen += 1
    assert seen == 4


def _rand_case(seed, C=7, H=9, W=11):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(C, H, W, generator=g, dtype=torch.float64)
    b = torch.randn(C, H, W, generator=g, dtype=torch.float64) + 0.6 * a
    m = (torch.rand(1, H, W, generator=g) < 0.6)
    return a, b, m


def test_identities_in_float64():
    """Binary m, float64: the channel-wise masked loss is the unmasked loss of (m a, m b); the per-pixel masked loss is the m-weighted
    mean of the per-pixel cosines."""
    for seed in range(3):
        a, b, m = _rand_case(seed)
        lc = float(masked_feature_loss(a, b, m))
        assert abs(lc - float(feature_loss(a * m, b * m))) <= T64
        cos = torch.nn.CosineSimilarity(dim=0, eps=1e-6)(a.reshape(7, -1), b.reshape(7, -1))
        w = m.reshape(-1).double()
        assert abs(float(masked_feature_loss(a, b, m, per_pixel=True)) - float(1 - (w * cos).sum() / w.sum())) <= T64


def test_empty_mask_values():
    a, b, m = _rand_case(5)
    none = torch.zeros_like(m)
    assert float(masked_feature_loss(a, b, none)) == 1.0
    assert np.isnan(float(masked_feature_loss(a, b, none, per_pixel=True)))
    assert float(masked_feature_loss(a.float(), b.float(), none)) == 1.0


@pytest.mark.parametrize("per_pixel", [False, True])
def test_values_at_masked_out_pixels_are_never_used(per_pixel):
    """A select, not a product with 0: Inf, NaN and 1e30 at masked-out pixels of either map leave the loss and the gradient alone,
    bit for bit, and the gradient is exactly 0 there."""
    a, b, m = _rand_case(9)
    a, b = a.float(), b.float()

    def run(a_, b_):
        x = a_.clone().requires_grad_()
        loss = masked_feature_loss(x, b_, m, per_pixel=per_pixel)
        (3.0 * loss).backward()
        return loss.detach(), x.grad

    l0, g0 = run(a, b)
    out = ~m[0]
    for junk in (float("nan"), float("inf"), 1e30):
        aj, bj = a.clone(), b.clone()
        aj[:, out] = junk
        bj[:, out] = -junk
        l1, g1 = run(aj, bj)
        assert torch.equal(l0, l1) and torch.equal(g0, g1) and torch.isfinite(g1).all()
    assert float(g0[:, out].abs().max()) == 0.0 and float(g0[:, m[0]].abs().min()) > 0.0


def test_full_resolution_mask():
    from nefes_amd.refine import full_resolution_mask
    low = torch.zeros(15, 20)
    low[4:9, 5:12] = 1
    full = full_resolution_mask(low, (60, 80), crop=10)
    assert full.dtype == torch.uint8 and tuple(full.shape) == (40, 60) and full.is_contiguous()
    expect = low.repeat_interleave(4, 0).repeat_interleave(4, 1)[10:-10, 10:-10]         # nearest neighbour at an integer scale
    assert torch.equal(full, expect.to(torch.uint8))
    assert tuple(full_resolution_mask(low[None].bool(), (60, 80), crop=0).shape) == (1, 60, 80)
    assert tuple(full_resolution_mask(torch.ones(2, 15, 20), (61, 83), crop=3).shape) == (2, 55, 77)

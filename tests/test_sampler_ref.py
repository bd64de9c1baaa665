"""tests/sampler_ref.py, the exact reference the sampler kernels are held to (tests/test_gpu_sampler.py), checked on the CPU:
it reproduces the golden vectors of the reference project bit for bit, and the inputs the GPU tests feed SEE each rule of the
sampler -- the helper with one rule deliberately changed (the changed copies live here) gives another answer on them."""
import numpy as np
import pytest
import torch

from tests import sampler_ref as R

T = lambda a: torch.from_numpy(np.asarray(a))
SHAPES = sorted(set(R.MERGE_SHAPES + R.FUSED_SHAPES))


def batch(Nc, Ni, per_ray, N=37):
    """(sigma, z [N, Nc], kinds, weights, cdf) of one shape of the GPU matrix, with the CPU oracle's fp32 weights."""
    sigma, z, kinds = R.rays(Nc, N, 1000 * Nc + Ni, per_ray)
    w = R.coarse_weights(sigma, z)
    z = z if z.dim() == 2 else z[None].expand(N, Nc).contiguous()
    return sigma, z, kinds, w, R.cdf_from_weights(w)


def changed_invert(bins, cdf, u, right=True, denom_rule=True, below_min=0, above_off=0):
    """oracle/ref_cpu.py invert_cdf (rendering.py:49-64) with one rule changed per argument."""
    inds = torch.searchsorted(cdf, u.contiguous(), right=right)
    below = torch.clamp(inds - 1, min=below_min)
    above = torch.clamp(inds, max=cdf.shape[-1] - 1 - above_off)
    c_lo, c_hi = torch.gather(cdf, 1, below), torch.gather(cdf, 1, above)
    b_lo, b_hi = torch.gather(bins, 1, below), torch.gather(bins, 1, above)
    denom = c_hi - c_lo
    if denom_rule:
        denom = torch.where(denom < 1e-5, torch.ones_like(denom), denom)
    return b_lo + (u - c_lo) / denom * (b_hi - b_lo), inds


def same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=-7., posinf=-8., neginf=-9.), torch.nan_to_num(b, nan=-7., posinf=-8., neginf=-9.))


@pytest.mark.parametrize("tag,det,Ni", [("det128", True, 128), ("det64", True, 64), ("rand128", False, 128)])
def test_helper_reproduces_the_golden_cases(golden, tag, det, Ni):
    g = golden("sample_pdf")
    z, w = T(g[f"{tag}.z"]), T(g["w"])
    u = None if det else T(g[f"{tag}.u"])
    cdf, inds, samples, z_fine = R.reference(z, w, u, Ni, cdf=T(g[f"{tag}.cdf"]))
    assert np.array_equal(inds.numpy(), g[f"{tag}.inds"])
    assert np.array_equal(samples.numpy(), g[f"{tag}.samples"])
    assert np.array_equal(z_fine.numpy(), g[f"{tag}.merged"])
    # its own CDF: torch's cascade sum is not reproducible, one ulp of 1.0 each way is (tests/test_gpu_parity.py, the same bound)
    own = R.cdf_from_weights(w)
    assert float(np.abs(own.numpy() - g[f"{tag}.cdf"]).max()) <= 2.4e-7
    assert bool((own.diff(dim=-1) >= 0).all()) and bool((own[:, 0] == 0).all())
    # the reference's call surface (bins, weights[..., 1:-1]) is the same computation
    mid = .5 * (z[..., 1:] + z[..., :-1])
    c1, i1, s1, none = R.reference(mid, w[..., 1:-1], u, Ni, layout=1)
    c0, i0, s0, _ = R.reference(z, w, u, Ni)
    assert none is None and torch.equal(c1, c0) and torch.equal(i1, i0) and torch.equal(s1, s0)


def test_the_cdf_check_fires_on_sums_that_depend_on_their_order():
    """cdf_from_weights asserts that its float64 sums are exact.  Weights far outside [0, 1] break that, and it says so."""
    w = torch.rand(4, 64, generator=torch.Generator().manual_seed(0))
    R.cdf_from_weights(w)
    w[:, 7] = 3e12
    with pytest.raises(AssertionError, match="order of summation|inexact"):
        R.cdf_from_weights(w)


@pytest.mark.parametrize("Nc,Ni", SHAPES)
@pytest.mark.parametrize("per_ray", [True, False])
def test_every_shape_gives_ordered_rows_and_enough_ties(Nc, Ni, per_ray):
    N = 37 if (Nc, Ni) in R.FUSED_SHAPES else 9
    sigma, z, kinds, w, cdf = batch(Nc, Ni, per_ray, N)
    assert bool((cdf.diff(dim=-1) >= 0).all()), [kinds[r] for r in range(N) if not bool((cdf[r].diff() >= 0).all())]
    assert bool(torch.isfinite(w).all()) and bool((z.diff(dim=-1) >= 0).all())
    us = R.u_rows(Ni, cdf[0], 7, N=N)
    assert set(us) == {"linspace", "per_ray", "uneven", "shuffled", "ties"}
    assert bool((us["uneven"].diff() >= 0).all()) and bool((us["ties"].diff() >= 0).all())
    assert Ni == 1 or not bool((us["shuffled"].diff() >= 0).all())
    assert Ni == 1 or not torch.equal(us["uneven"], torch.linspace(0., 1., Ni))
    assert float(us["per_ray"][0, 0]) == (0. if Ni > 1 else 1.) and float(us["per_ray"][0, Ni - 1]) == 1.
    assert R.count_ties(us["ties"], cdf[0]) >= R.ties_required(Nc, Ni)
    for name, u in us.items():
        _, inds, samples, z_fine = R.reference(z, w, u, Ni)
        assert z_fine.shape == (N, Nc + Ni) and bool(torch.isfinite(z_fine).all()), name
        bad = [kinds[r] for r in range(N) if not bool((z_fine[r].diff() >= 0).all())]
        assert not bad, (name, bad)
        assert int(inds.min()) >= 1 and int(inds.max()) <= Nc - 1, name


@pytest.mark.parametrize("Nc,Ni", [s for s in SHAPES if s[0] >= 4])
def test_ties_see_the_side_of_searchsorted(Nc, Ni):
    """right=False moves the index of every exact tie u == cdf[k]: the tie row changes `inds` of ray 0 at each of them."""
    _, z, kinds, w, cdf = batch(Nc, Ni, True)
    u = R.expand_u(R.tie_row(Ni, cdf[0]), z.shape[0], Ni)
    bins = .5 * (z[..., 1:] + z[..., :-1])
    _, inds = changed_invert(bins, cdf, u)
    assert torch.equal(inds, R.reference(z, w, u, Ni)[1])                     # the unchanged copy is the helper
    _, left = changed_invert(bins, cdf, u, right=False)
    # away from the two ends (0 and 1 are the only ties of the linspace): u == cdf[k], 1 <= k <= Nc - 3, has inds = k + 1
    ks = inds[0][left[0] != inds[0]]
    assert int(((ks >= 2) & (ks <= Nc - 2)).sum()) >= R.ties_required(Nc, Ni) >= 1


@pytest.mark.parametrize("Nc,Ni", R.FUSED_SHAPES)
def test_flat_cdf_rays_see_the_denominator_rule(Nc, Ni):
    """Without denom < 1e-5 -> 1 a flat stretch of the CDF divides by (nearly) zero: the one-hot rays (a spike in the middle, the
    golden file's one-hot row) change samples wherever u falls on the flat part, the saturated ray where u = 1 meets cdf[-1]."""
    _, z, kinds, w, cdf = batch(Nc, Ni, True)
    bins = .5 * (z[..., 1:] + z[..., :-1])
    for name in ("linspace", "uneven"):
        u = R.expand_u(R.u_rows(Ni, None, 7, N=z.shape[0])[name], z.shape[0], Ni)
        s, _ = changed_invert(bins, cdf, u)
        assert torch.equal(s, R.reference(z, w, u, Ni)[2])
        s_bad, _ = changed_invert(bins, cdf, u, denom_rule=False)
        if Ni == 1 and name == "linspace":                                  # (u = 0 only: t = 0 whatever the denominator is)
            continue
        r = kinds.index("spike_mid")
        assert not same(s_bad[r], s[r]), (name, "spike_mid")
        r = kinds.index("saturated")
        assert float(u[r, -1]) == 1. and float(cdf[r, -1]) <= 1.
        assert not same(s_bad[r], s[r]), (name, "saturated")


def test_the_golden_one_hot_and_both_ends_rows_see_the_denominator_rule(golden):
    g = golden("sample_pdf")
    z, w = T(g["det128.z"])[[2, 5]], T(g["w"])[[2, 5]]
    assert int((w[0] > 0).sum()) == 1 and float(w[1, 1]) == .5 and float(w[1, -2]) == .5
    cdf = R.cdf_from_weights(w)
    bins = .5 * (z[..., 1:] + z[..., :-1])
    u = R.expand_u(None, 2, 128)
    s, _ = changed_invert(bins, cdf, u)
    s_bad, _ = changed_invert(bins, cdf, u, denom_rule=False)
    assert torch.equal(s, R.reference(z, w, None, 128)[2])
    assert not same(s_bad[0], s[0]) and not same(s_bad[1], s[1])


@pytest.mark.parametrize("Nc,Ni", [s for s in SHAPES if s[0] >= 4])
def test_the_end_samples_see_the_clamps(Nc, Ni):
    """below = max(inds - 1, 0) and above = min(inds, Nc - 2): one off moves the first sample / those of the last interval."""
    _, z, kinds, w, cdf = batch(Nc, Ni, True)
    bins = .5 * (z[..., 1:] + z[..., :-1])
    u = R.expand_u(R.u_rows(Ni, None, 7, N=z.shape[0])["uneven"] if Ni == 1 else None, z.shape[0], Ni)
    s, _ = changed_invert(bins, cdf, u)
    if Ni > 1:
        s_lo, _ = changed_invert(bins, cdf, u, below_min=1)
        rows = bins[:, 0] != bins[:, 1]                                        # u = 0 -> bins[0]: on every ray but the one whose
        assert int(rows.sum()) == len(kinds) - kinds.count("dup_front")        # first three depths are equal
        assert bool((s_lo[rows, 0] != s[rows, 0]).all())
    # above: u = 1 itself lands on bins[-1] either way (its t is an ulp), the samples of the LAST CDF interval are what moves -- and
    # only they.  The zero-density ray has a uniform pdf: a linspace finer than 1 / (Nc - 2) has an entry inside that interval.
    s_hi, _ = changed_invert(bins, cdf, u, above_off=1)
    inds = R.reference(z, w, u, Ni)[1]
    moved = s_hi != s
    assert not bool((moved & (inds != Nc - 2)).any())
    if Ni - 1 > Nc - 2:
        assert bool(moved[kinds.index("zero")].any())


@pytest.mark.parametrize("Nc,Ni", [s for s in SHAPES if s[0] >= 9])
def test_equal_depths_meet_equal_samples(Nc, Ni):
    """The rays with runs of equal coarse depths have samples EQUAL to a coarse depth (both bins around them are that depth): the
    merge has to rank ties between the two halves.  The three equal depths in front catch u = 0 on every shape; the run of five
    holds 3 / (Nc - 2) of a near-uniform pdf, which a linspace of spacing 1 / (Ni - 1) cannot step over once that is smaller."""
    _, z, kinds, w, cdf = batch(Nc, Ni, True)
    _, _, samples, z_fine = R.reference(z, w, None, Ni)
    r = kinds.index("dup_front")
    assert float(samples[r, 0]) == float(z[r, 0]) == float(z[r, 2])
    if 3. * (Ni - 1) >= 1.05 * (Nc - 2):
        r = kinds.index("dup_mid")
        hit = samples[r] == z[r, Nc // 2]
        assert int(hit.sum()) >= 1 and float(z[r, Nc // 2 - 2]) == float(z[r, Nc // 2 + 2])
        # a merge that kept one of each equal pair would lose them
        assert torch.unique(z_fine[r]).numel() <= Nc + Ni - 4 - int(hit.sum())

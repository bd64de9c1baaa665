"""The two kernels of csrc/sample_pdf.hip against tests/sampler_ref.py, an independent and exact reference (numpy CDF + the CPU
oracle's invert_cdf + torch.sort), bit for bit at every fast path: the lane-strided loops and both searches of
sample_pdf_merge_kernel at coarse counts from 3 to 256, both layouts, a supplied CDF; the inverted search of coarse_sample_kernel
(guess, walk, histogram) in its vectorised and scalar forms at RW = 1, 2, 4, its paired binary search, both merges and both row
stores -- on rays that are empty, saturated, one-hot at either end or in the middle, carry runs of equal depths, and on u rows
that are evenly spaced, uneven, unordered, per ray, or made of exact ties u == cdf[k].  Every comparison is an equality; the
composited weights alone are held to the float64 oracle at the compositing tests' own bound."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from tests import parity_log as P
from tests import sampler_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = lambda a: torch.from_numpy(np.asarray(a))


@pytest.fixture(scope="module")
def ops():
    from nefes_amd import lib, ops as _ops
    lib.load()
    return _ops


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


def differs(what, got, want, kinds):
    """None if `got` == `want` bit for bit, else where it first differs: (what, ray kind, ray, column, got, want)."""
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(got, want):
        return None
    r, c = (got != want).nonzero()[0].tolist()
    return (what, kinds[r], r, c, got[r, c].item(), want[r, c].item(), f"{int((got != want).sum())} of {got.numel()} differ")


def report(kernel, Nc, Ni, N, mode, uname, bad):
    print(f"sampler_ref: {kernel} Nc={Nc} Ni={Ni} N={N} {mode} u={uname}: {'MISMATCH ' + repr(bad) if bad else 'match'}")


def test_the_device_linspace_is_the_host_linspace(ops):
    """u = None is torch.linspace(0, 1, Ni) made on the device (ops._linspace01) for the kernels and on the host for the reference:
    the same bits at every Ni used below -- were they not, the failures below would be about this row and not about a kernel."""
    for Ni in sorted({s[1] for s in R.MERGE_SHAPES + R.FUSED_SHAPES}):
        assert torch.equal(ops._linspace01(Ni, DEV).cpu(), torch.linspace(0., 1., steps=Ni)), Ni


# ---- sample_pdf_merge_kernel ------------------------------------------------------------------------------------------------
def merge_case(ops, Nc, Ni, N):
    sigma, z, kinds = R.rays(Nc, N, 1000 * Nc + Ni, True)
    w = R.coarse_weights(sigma, z)
    cdf_ref = R.cdf_from_weights(w)
    us = R.u_rows(Ni, cdf_ref[0], 7, N=N)
    assert R.count_ties(us["ties"], cdf_ref[0]) >= R.ties_required(Nc, Ni)
    failures = []
    for uname, u in us.items():
        z_fine, z_samples, inds, cdf = ops.sample_pdf_merge(dev(z), dev(w), Ni, u=dev(u), want_debug=True)
        bad = [differs("cdf", cdf, cdf_ref, kinds)]
        # everything behind the CDF against the reference on the kernel's OWN cdf: an ulp there is reported as a CDF failure, above,
        # and not as a cascade of index failures
        _, i_ref, s_ref, f_ref = R.reference(z, w, u, Ni, cdf=cdf.cpu())
        bad += [differs("inds", inds.long(), i_ref, kinds), differs("z_samples", z_samples, s_ref, kinds), differs("z_fine", z_fine, f_ref, kinds)]
        bad = [b for b in bad if b]
        report("merge", Nc, Ni, N, "per-ray depths", uname, bad)
        failures += [(uname, b) for b in bad]
    assert not failures, failures


@pytest.mark.parametrize("Nc,Ni", R.MERGE_SHAPES)
def test_merge_kernel_equals_the_reference(ops, Nc, Ni):
    """N = 9 fills neither a workgroup of four rays nor a whole number of them."""
    merge_case(ops, Nc, Ni, 9)


def test_merge_kernel_equals_the_reference_on_one_ray(ops):
    merge_case(ops, 64, 128, 1)


@pytest.mark.parametrize("Ni", [128, 200, 448])
def test_merge_kernel_on_the_golden_one_hot_and_both_ends_rows(ops, golden, Ni):
    """The two degenerate weight rows of the golden file (all of the mass on one sample; half on each end of the pdf)."""
    g = golden("sample_pdf")
    z, w = T(g["det128.z"])[[2, 5]].contiguous(), T(g["w"])[[2, 5]].contiguous()
    kinds = ["one_hot", "both_ends"]
    cdf_ref = R.cdf_from_weights(w)
    failures = []
    for uname, u in R.u_rows(Ni, cdf_ref[1], 7, N=2).items():
        z_fine, z_samples, inds, cdf = ops.sample_pdf_merge(dev(z), dev(w), Ni, u=dev(u), want_debug=True)
        _, i_ref, s_ref, f_ref = R.reference(z, w, u, Ni, cdf=cdf.cpu())
        bad = [b for b in (differs("cdf", cdf, cdf_ref, kinds), differs("inds", inds.long(), i_ref, kinds),
                           differs("z_samples", z_samples, s_ref, kinds), differs("z_fine", z_fine, f_ref, kinds)) if b]
        report("merge", 64, Ni, 2, "golden rows", uname, bad)
        failures += [(uname, b) for b in bad]
    assert not failures, failures


@pytest.mark.parametrize("Nc,Ni", [(65, 63), (200, 130)])
def test_merge_kernel_bins_layout_equals_the_reference(ops, Nc, Ni):
    """The reference's call surface sample_pdf(bins, weights[..., 1:-1]): layout 1 of the kernel."""
    sigma, z, kinds = R.rays(Nc, 9, 1000 * Nc + Ni, True)
    w = R.coarse_weights(sigma, z)
    mid = (.5 * (z[..., 1:] + z[..., :-1])).contiguous()
    w_mid = w[..., 1:-1].contiguous()
    cdf_ref = R.cdf_from_weights(w)
    failures = []
    for uname, u in R.u_rows(Ni, cdf_ref[0], 7, N=9).items():
        none, z_samples, inds, cdf = ops.sample_pdf_merge(dev(mid), dev(w_mid), Ni, u=dev(u), want_debug=True, bins_layout=True)
        assert none is None
        c_ref, i_ref, s_ref, _ = R.reference(mid, w_mid, u, Ni, layout=1)
        assert torch.equal(c_ref, cdf_ref)
        _, _, s0, _ = R.reference(z, w, u, Ni)
        assert torch.equal(s_ref, s0)                                # the two call surfaces of the reference agree
        bad = [b for b in (differs("cdf", cdf, c_ref, kinds), differs("inds", inds.long(), i_ref, kinds), differs("z_samples", z_samples, s_ref, kinds)) if b]
        report("merge", Nc, Ni, 9, "bins layout", uname, bad)
        failures += [(uname, b) for b in bad]
    assert not failures, failures


@pytest.mark.parametrize("Nc,Ni", [(16, 24), (64, 200), (200, 130)])
def test_merge_kernel_counts_on_a_cdf_that_is_not_sorted(ops, Nc, Ni):
    """A caller-supplied CDF with two interior entries swapped takes the linear count: inds = #{k : cdf[k] <= u}, as the kernel's
    comment says (torch.searchsorted is undefined on such a row, so the plain count is the reference)."""
    sigma, z, kinds = R.rays(Nc, 9, 1000 * Nc + Ni, True)
    w = R.coarse_weights(sigma, z)
    cdf = R.cdf_from_weights(w).clone()
    a, b = Nc // 3, Nc // 3 + 2
    cdf[:, [a, b]] = cdf[:, [b, a]]
    assert bool((cdf[:, a] > cdf[:, a + 1]).all())
    failures = []
    for uname, u in R.u_rows(Ni, None, 7, N=9).items():
        _, _, inds, cdf_out = ops.sample_pdf_merge(dev(z), dev(w), Ni, u=dev(u), cdf=dev(cdf), want_debug=True)
        assert torch.equal(cdf_out.cpu(), cdf)
        uu = R.expand_u(u, 9, Ni).numpy()
        count = (cdf.numpy()[:, None, :] <= uu[:, :, None]).sum(-1)
        bad = differs("inds", inds.long(), torch.from_numpy(count).long(), kinds)
        report("merge", Nc, Ni, 9, "unsorted cdf", uname, bad)
        if bad:
            failures.append((uname, bad))
    assert not failures, failures


# ---- coarse_sample_kernel ---------------------------------------------------------------------------------------------------
def fused_case(ops, Nc, Ni, N, zmode):
    if zmode == "per-ray depths":
        sigma, z, kinds = R.rays(Nc, N, 1000 * Nc + Ni, True)
        z_full = z
    else:
        z_row = ops.coarse_depth_row(Nc, R.NEAR, R.FAR, zmode == "shared lindisp row", DEV).cpu()
        assert bool((z_row.diff() > 0).all())
        sigma, z, kinds = R.rays(Nc, N, 1000 * Nc + Ni, False, z_row=z_row)
        z_full = z[None].expand(N, Nc).contiguous()
    sg = dev(sigma.reshape(N, 1, Nc))
    # first call: the weights, held to the float64 oracle beside the fp32 one (tests/test_gpu_parity.py
    # test_composite_four_samples_per_lane_matches_oracle: the same rule and bound)
    _, _, w_dev = ops.coarse_sample(sg, dev(z), Ni, want_weights=True)
    w = w_dev.cpu()
    w64 = R.coarse_weights(sigma, z, torch.float64)
    w32 = R.coarse_weights(sigma, z, torch.float32).double()
    relm = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
    P.check(f"sampler_ref[fused,Nc={Nc},Ni={Ni},N={N},{zmode}]", "weights", relm(w.double(), w64), relm(w32, w64), tol=2e-6)
    # second round: every u variant, the row of exact ties of ray 0's own CDF among them
    cdf_ref = R.cdf_from_weights(w)
    us = R.u_rows(Ni, cdf_ref[0], 7, N=N)
    assert R.count_ties(us["ties"], cdf_ref[0]) >= R.ties_required(Nc, Ni)
    failures = []
    for uname, u in us.items():
        _, _, s_ref, f_ref = R.reference(z_full, w, u, Ni)
        z_fine, z_samples, w2 = ops.coarse_sample(sg, dev(z), Ni, u=dev(u), want_weights=True)
        m_fine, m_samples = ops.sample_pdf_merge(dev(z_full), w_dev, Ni, u=dev(u))
        for kernel, got_s, got_f in (("fused", z_samples, z_fine), ("merge", m_samples, m_fine)):
            bad = [b for b in (differs("z_samples", got_s, s_ref, kinds), differs("z_fine", got_f, f_ref, kinds)) if b]
            report(kernel, Nc, Ni, N, zmode, uname, bad)
            failures += [(kernel, uname, b) for b in bad]
        if not torch.equal(w2, w_dev):
            failures.append(("fused", uname, "the weights depend on u"))
    assert not failures, failures


@pytest.mark.parametrize("zmode", ["per-ray depths", "shared row", "shared lindisp row"])
@pytest.mark.parametrize("Nc,Ni", R.FUSED_SHAPES)
def test_fused_kernel_equals_the_reference(ops, Nc, Ni, zmode):
    """N = 37 fills neither the last wave nor the last workgroup at any RW."""
    fused_case(ops, Nc, Ni, 37, zmode)


@pytest.mark.parametrize("zmode", ["per-ray depths", "shared row"])
@pytest.mark.parametrize("Nc,Ni", [(64, 128), (256, 256)])
def test_fused_kernel_equals_the_reference_on_one_ray(ops, Nc, Ni, zmode):
    fused_case(ops, Nc, Ni, 1, zmode)


# ---- sizes the kernels do not take: an error before any launch -------------------------------------------------------------------
def test_sampler_sizes_out_of_range_fail_loudly(ops):
    zeros = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(RuntimeError, match="nefes_sample_pdf_merge failed: bad argument"):
        ops.sample_pdf_merge(zeros(2, 2), zeros(2, 2), 4)                          # Nc = 2
    with pytest.raises(RuntimeError, match="nefes_sample_pdf_merge failed: unsupported configuration"):
        ops.sample_pdf_merge(zeros(2, 257), zeros(2, 257), 4)                      # Nc = 257
    with pytest.raises(RuntimeError, match="nefes_sample_pdf_merge failed: unsupported configuration"):
        ops.sample_pdf_merge(zeros(2, 64), zeros(2, 64), 449)                      # Nc + Ni = 513
    with pytest.raises(RuntimeError, match="nefes_coarse_sample failed: unsupported configuration"):
        ops.coarse_sample(zeros(2, 1, 65), zeros(2, 65), 4)                        # Nc = 65
    with pytest.raises(RuntimeError, match="nefes_coarse_sample failed: unsupported configuration"):
        ops.coarse_sample(zeros(2, 1, 64), zeros(2, 64), 449)                      # Nc + Ni = 513

"""An independent, exact reference of the hierarchical sampler (csrc/sample_pdf.hip), for tests/test_sampler_ref.py (CPU) and
tests/test_gpu_sampler.py (GPU).  Nothing here touches the GPU or the code under test.

The sampler is  bins = z_mid  ->  cdf = [0, cumsum((w[1:-1] + 1e-5) / sum)]  ->  searchsorted(cdf, u, right=True) + linear
interpolation  ->  sort(cat[z, samples])  (rendering.py:23-66,132-141).  Every stage after the CDF is plain fp32 torch on the CPU
(oracle/ref_cpu.py invert_cdf, torch.sort), which reproduces the golden vectors bit for bit.  The CDF is the arithmetic the kernels
document -- the total of fl32(w + 1e-5) accumulated in float64 and rounded once, pdf = fl32(ww / total), a float64 running sum
rounded per element -- restated in numpy.  Both float64 sums are exact for weights in [0, 1] (every term is an fp32 number of at
least ~4e-8 and the sums stay below 2^9: 53 bits hold every partial sum), so their order does not matter and the kernels' result
is fully determined: `cdf_from_weights` asserts that per input instead of assuming it."""
import numpy as np
import torch

from oracle import ref_cpu as O

NEAR, FAR = 0.25, 5.0

# the shapes of tests/test_gpu_sampler.py (here so that the CPU test walks the same matrix)
MERGE_SHAPES = [(3, 1), (4, 5), (16, 24), (64, 128), (65, 63), (64, 200), (200, 130), (256, 256), (64, 448)]
FUSED_SHAPES = [(64, 1), (64, 37), (64, 64), (64, 100), (64, 448), (128, 64), (128, 100), (128, 128), (128, 384), (256, 64), (256, 100),
                (256, 256)]


def _seq_sum(a):
    """Sum along the last axis strictly left to right in float64 (np.sum is pairwise)."""
    return np.cumsum(a, axis=-1, dtype=np.float64)[..., -1]


def cdf_from_weights(w):
    """fp32 weights [N, Nc] -> fp32 cdf [N, Nc - 1] = [0, cumsum(pdf)], pdf over w[:, 1:-1] (rendering.py:26-29, :134)."""
    w = np.ascontiguousarray(w.detach().cpu().numpy() if torch.is_tensor(w) else w)
    assert w.dtype == np.float32 and w.ndim == 2 and w.shape[1] >= 3, (w.dtype, w.shape)
    ww = (w[:, 1:-1] + np.float32(1e-5)).astype(np.float32)
    n = ww.shape[1]
    perm = np.random.default_rng(n).permutation(n)
    ww64 = ww.astype(np.float64)
    total64 = _seq_sum(ww64)
    assert np.array_equal(total64, _seq_sum(ww64[:, perm])), "the float64 total of w + 1e-5 depends on the order of summation"
    total = total64.astype(np.float32)
    pdf = (ww / total[:, None]).astype(np.float32)
    pdf64 = pdf.astype(np.float64)
    run = np.cumsum(pdf64, axis=-1)
    assert np.array_equal(run[:, -1], _seq_sum(pdf64[:, perm])), "the float64 running sum of the pdf depends on the order of summation"
    # ... and so does no prefix: each one and the sum of the terms behind it (added back to front) make up the same total
    back = np.cumsum(pdf64[:, ::-1], axis=-1)[:, ::-1]
    assert np.array_equal(run[:, :-1] + back[:, 1:], np.broadcast_to(run[:, -1:], run[:, :-1].shape)), "a prefix of the pdf sum is inexact"
    cdf = np.concatenate([np.zeros((w.shape[0], 1), np.float32), run.astype(np.float32)], -1)
    return torch.from_numpy(cdf)


def expand_u(u, N, Ni):
    """None (the deterministic linspace, rendering.py:33), [Ni] or [N, Ni] -> contiguous fp32 [N, Ni]."""
    if u is None:
        u = torch.linspace(0., 1., steps=Ni)
    u = u.detach().cpu().to(torch.float32)
    assert u.shape[-1] == Ni
    return (u[None].expand(N, Ni) if u.dim() == 1 else u).contiguous()


def reference(z, w, u, Ni, layout=0, cdf=None):
    """-> (cdf [N, Nc-1], inds [N, Ni] int64, samples [N, Ni], z_fine [N, Nc+Ni]) in fp32 on the CPU.
    layout 0: z = the coarse depths [N, Nc], w = their weights [N, Nc].  layout 1: the reference's call surface
    sample_pdf(bins, weights[..., 1:-1]): z = bins [N, Nc-1], w = [N, Nc-2]; there is nothing to merge and z_fine is None."""
    z, w = z.detach().cpu().to(torch.float32), w.detach().cpu().to(torch.float32)
    if layout == 0:
        bins = .5 * (z[..., 1:] + z[..., :-1])                              # rendering.py:132
    else:
        bins = z
        w = torch.cat([torch.zeros_like(w[:, :1]), w, torch.zeros_like(w[:, :1])], -1)      # (the two end weights are never read)
    cdf = cdf_from_weights(w) if cdf is None else cdf.detach().cpu().to(torch.float32)
    assert cdf.shape == bins.shape
    samples, inds = O.invert_cdf(bins, cdf, expand_u(u, z.shape[0], Ni))
    z_fine = torch.sort(torch.cat([z, samples], -1), -1)[0] if layout == 0 else None     # rendering.py:141
    return cdf, inds, samples, z_fine


def depth_row(Nc, lindisp=False):
    """The shared row of coarse depths (rendering.py:96-100) as the CPU oracle builds it."""
    return O.coarse_depths(torch.full((1, 1), NEAR), torch.full((1, 1), FAR), Nc, lindisp)[0].contiguous()


def rays(Nc, N, seed, per_ray_depths, z_row=None):
    """-> (sigma [N, Nc], z, kinds).  z = [N, Nc] jittered, sorted rows when per_ray_depths, else the one shared row [Nc] (`z_row`,
    by default the CPU oracle's row between 0.25 and 5.0).  kinds[r] names row r: row 0 is generic, one row of each special kind
    follows (as far as N and Nc allow), generic rows fill the rest."""
    gen = torch.Generator().manual_seed(seed)
    sigma = torch.nn.functional.softplus(3 * torch.randn(N, Nc, generator=gen)) * 0.5
    z_row = depth_row(Nc) if z_row is None else z_row.detach().cpu().to(torch.float32)
    kinds = ["generic"] * N
    mid = Nc // 2

    def zero(r): sigma[r] = 0.

    def saturated(r): sigma[r] = 3000.

    def spike_mid(r):
        sigma[r] = 0.
        sigma[r, mid:mid + 3] = 5000.

    def tiny(r): sigma[r] = 1e-12

    def spike_first(r):
        sigma[r] = 0.
        sigma[r, 0] = 5000.

    def spike_last_two(r):
        sigma[r] = 0.
        sigma[r, -2:] = 5000.

    special = [("zero", zero), ("saturated", saturated), ("spike_mid", spike_mid), ("tiny", tiny), ("spike_first", spike_first),
               ("spike_last_two", spike_last_two)]
    z = z_row
    if per_ray_depths:
        z = torch.sort(z_row[None] + (torch.rand(N, Nc, generator=gen) - .5) * 0.02, -1)[0].contiguous()
        if Nc >= 9:
            # Equal depths have alpha = 0, so the bins between them weigh 1e-5 / total whatever sigma is: a density far below 1e-5
            # keeps the pdf of these two rows near uniform, so that samples do fall between -- and therefore ON -- the equal depths
            def dup_mid(r):
                sigma[r] *= 1e-6
                z[r, mid - 2:mid + 3] = z[r, mid]

            def dup_front(r):
                sigma[r] *= 1e-6
                z[r, :3] = z[r, 2]

            special += [("dup_mid", dup_mid), ("dup_front", dup_front)]
    for r, (name, fn) in enumerate(special, start=1):
        if r < N:
            fn(r)
            kinds[r] = name
    return sigma, z, kinds


def coarse_weights(sigma, z, dtype=torch.float32):
    """Compositing variant D of the CPU oracle: the weights of the sigma-only coarse pass."""
    z = z if z.dim() == 2 else z[None].expand(sigma.shape[0], -1)
    return O.composite(sigma.to(dtype)[..., None], z.to(dtype), typ="coarse", test_time=True).weights


def tie_row(Ni, cdf_row):
    """A shared ascending u row of exact ties: the interior entries of `cdf_row` [Nc-1], each with its two fp32 neighbours, padded
    with a linspace or trimmed to Ni entries (the entries themselves go last)."""
    c = np.asarray(cdf_row.detach().cpu().numpy() if torch.is_tensor(cdf_row) else cdf_row, np.float32)[1:-1]
    if len(c) > Ni:
        c = c[np.round(np.linspace(0, len(c) - 1, Ni)).astype(np.int64)]
    room = Ni - len(c)
    near = np.stack([np.nextafter(c, np.float32(-np.inf), dtype=np.float32), np.nextafter(c, np.float32(np.inf), dtype=np.float32)], -1).reshape(-1)
    near = near[:room]
    pad = np.linspace(0., 1., room - len(near), dtype=np.float32) if room > len(near) else np.zeros(0, np.float32)
    u = np.sort(np.concatenate([c, near, pad]).astype(np.float32))
    assert u.shape == (Ni,)
    return torch.from_numpy(u)


def count_ties(u_row, cdf_row):
    """How many entries of the shared row `u_row` equal an interior entry of `cdf_row` exactly."""
    return int(np.isin(u_row.detach().cpu().numpy(), cdf_row.detach().cpu().numpy()[1:-1]).sum())


def ties_required(Nc, Ni):
    return min(Ni, Nc - 3)


def u_rows(Ni, cdf_row, seed, N=1):
    """-> {name: u}: None; a per-ray draw [N, Ni] holding an exact 0 and an exact 1; a shared ascending, unevenly spaced row with a
    value repeated three times; the same row shuffled; and, given the CDF of ray 0, the row of exact ties (tie_row)."""
    gen = torch.Generator().manual_seed(seed)
    per_ray = torch.rand(N, Ni, generator=gen)
    per_ray[0, 0] = 0.
    per_ray[0, Ni - 1] = 1.
    uneven = torch.sort(torch.rand(Ni, generator=gen) ** 3)[0]
    if Ni >= 5:
        uneven[Ni // 2 - 1:Ni // 2 + 2] = uneven[Ni // 2]
    uneven[0] = 0.
    uneven[Ni - 1] = 1.
    shuffled = uneven[torch.randperm(Ni, generator=gen)]
    if Ni > 1 and bool((shuffled.diff() >= 0).all()):
        shuffled = uneven.flip(0)
    out = {"linspace": None, "per_ray": per_ray, "uneven": uneven.contiguous(), "shuffled": shuffled.contiguous()}
    if cdf_row is not None:
        out["ties"] = tie_row(Ni, cdf_row)
    return out

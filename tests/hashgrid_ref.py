"""Float64 statement of the multiresolution hash-grid encoding at ANY geometry, its two gradients, seeded inputs on both sides of the
bound, and per-element error budgets derived from the reference's own derivatives.  tests/test_gpu_hashgrid.py holds the kernels of
csrc/hashgrid.hip (and, through them, the device functions of csrc/hashgrid.h that the fp16 field kernels call) to it per element;
tests/test_hashgrid_ref.py checks this file on the CPU.

Written from the kernels' comments, not from oracle/hashgrid_ref.py (which is one geometry, positive side only); the two are compared
where both are defined.  The index rule is stated as the CONTRACT the kernels implement:

    corner coordinate   c_k = (floor(pos_k) + d_k) mod 2^32                         (the kernels' (uint32_t)(int)floorf(pos))
    dense level         i = (c_x + c_y res + c_z res^2) mod 2^32, then mod entries   (uint32 arithmetic, then hg_index's reduction)
    hashed level        i = (c_x ^ c_y * 2654435761 ^ c_z * 805459861) mod 2^32, then mod entries

so a position below -bound (negative cell) lands where the kernels' uint32 wrap puts it.  That pins the kernels' OWN behaviour there;
parity with tiny-cuda-nn stays unpinned.

Positions are fp32 (what the kernels read); everything after them is float64.

Budgets (u = 2^-24, the unit roundoff of fp32; every figure is a first-order bound on |kernel - float64| per element).  The kernel's
only LARGE error is the fp32 rounding of hg_cell's  pos = x01 * scale + 0.5,  x01 = (x + bound) / (2 bound):
    rounding of x + bound        u |x + bound|, carried through / (2 bound) and * scale:   u |x01| scale
    rounding of the division     u |x01|, carried through * scale:                          u |x01| scale
    rounding of the product      u |x01 scale|   (absent when the compiler fuses the multiply-add)
    rounding of the sum          u |pos|
  = u (3 |x01| scale + |pos|) <= u (2 |x01| scale + 2 |pos| + 1/2)  because |x01| scale = |pos - 1/2| <= |pos| + 1/2;
    E_POS = u (2 |x01| scale + 2 |pos| + 1)  keeps the other half unit for w = pos - floor(pos) (exact in fp32, Sterbenz / same binade).
The cell itself is the same in fp32 and float64 because the inputs are drawn away from the cell faces (ambiguous()).  The error of pos
then reaches a result through that result's derivative with respect to the blend weight w_k; the remaining terms count the roundings of
the arithmetic after hg_cell and are written beside the lines that compute them."""
import functools
import math

import numpy as np
import torch

U = 2.0 ** -24
PRIMES = (1, 2654435761, 805459861)
MS = (1, 3, 63, 64, 65, 257, 1000)
SETS = ("inside", "both_sides", "rays", "repeats")
NEGATIVE_SETS = ("both_sides", "rays", "repeats")          # sets with coordinates below -bound
REPEATS = (1, 2, 63, 64, 65)                               # run lengths of the `repeats` set, cycled
K_DENSE = 9
# (n_levels, log2_hashmap_size, base_resolution, max_resolution, bound)
GEOMETRIES = {
    "default": (16, 19, 16, 2048, 25.0),       # the shipped one: 5 dense levels
    "small": (5, 10, 4, 64, 2.0),              # n_levels no multiple of 4; 2 dense levels
    "all_dense": (16, 24, 2, 24, 1.5),         # no hashed level: everything through the fp64 workspace
    "all_hashed": (16, 8, 16, 2048, 8.0),      # n_dense == 0: no workspace, no flush
    "three": (3, 12, 3, 11, 0.75),             # the fourth wave of the merged table-gradient kernel has no level
    "one": (1, 8, 5, 5, 1.0),                  # a single (dense) level: scale = base_resolution - 1
}


class Geometry:
    """hg_geometry restated.  `mutation` in {"scale_no_minus1", "no_round8", "offsets"} builds a deliberately wrong one (the CPU
    tests measure that the budgets tell it apart)."""

    def __init__(self, n_levels, log2_hashmap_size, base_resolution, max_resolution, bound, mutation=None):
        self.n_levels, self.log2, self.base, self.max_res, self.bound = n_levels, log2_hashmap_size, base_resolution, max_resolution, float(bound)
        # a single level has no growth factor: scale = base_resolution - 1 (ops.HashGrid passes 1.0 as well)
        growth = math.exp(math.log(max_resolution / base_resolution) / (n_levels - 1)) if n_levels > 1 else 1.0
        self.per_level_scale = float(np.float32(growth))                # the C ABI carries it as fp32
        self.levels, off = [], 0
        for l in range(n_levels):
            # the level scale is evaluated in float64 and rounded once
            scale = float(np.float32(base_resolution * self.per_level_scale ** l - 1.0))
            res = int(math.ceil(scale)) + 1
            entries = min(res ** 3 if mutation == "no_round8" else (res ** 3 + 7) // 8 * 8, 1 << log2_hashmap_size)
            if mutation == "scale_no_minus1":
                scale = float(np.float32(base_resolution * self.per_level_scale ** l))
            self.levels.append(dict(scale=scale, res=res, entries=entries, offset=off, hashed=res ** 3 > entries))
            off += entries
        self.total = off
        self.n_dense = 0                                                # entries of the dense levels: a prefix of the table
        for L in self.levels:
            if L["hashed"]:
                break
            self.n_dense = L["offset"] + L["entries"]
        if mutation == "offsets":                                       # every level reads the next level's block (the last: the first's)
            offs = [L["offset"] for L in self.levels]
            for l, L in enumerate(self.levels):
                L["offset"] = offs[(l + 1) % n_levels]

    def desc(self):
        from nefes_amd import lib as L
        return L.NefesHashGridDesc(self.n_levels, 2, self.log2, self.base, self.per_level_scale, self.bound)


@functools.lru_cache(maxsize=None)
def geometry(name, mutation=None):
    return Geometry(*GEOMETRIES[name], mutation=mutation)


def make_table(geo, seed=0, dtype=torch.float32):
    """U(-1, 1): neighbouring entries differ by O(1), so a wrong corner is far outside every budget (the 1e-4 initialisation is not)."""
    g = torch.Generator().manual_seed(1000 + seed)
    return (torch.rand(geo.total, 2, generator=g, dtype=torch.float32) * 2 - 1).to(dtype)


# ---- the cell, the blend weights and the eight corner indices of every sample at one level -----------------------------------------
CORNERS = [((c & 1), (c >> 1) & 1, c >> 2) for c in range(8)]          # corner c adds (dx, dy, dz) = its bits 0, 1, 2


def level_index(L, cell, mutation=None):
    """[M, 8] int64 table rows (level offset included) of the eight corners of integer cells `cell` [M, 3] (int64, may be negative)."""
    M32 = np.uint64(0xFFFFFFFF)
    out = np.empty((cell.shape[0], 8), np.int64)
    for c, d in enumerate(CORNERS):
        if mutation == "swap_xz":
            d = (d[2], d[1], d[0])
        if mutation == "no_wrap" and not L["hashed"]:
            cc = [cell[:, k] + d[k] for k in range(3)]
            i = (cc[0] + cc[1] * L["res"] + cc[2] * L["res"] ** 2) % L["entries"]        # python's non-negative remainder of a signed index
            out[:, c] = L["offset"] + i
            continue
        cc = [(cell[:, k] + d[k]).astype(np.uint64) & M32 for k in range(3)]             # two's complement, low 32 bits
        if L["hashed"]:
            p = PRIMES if mutation != "primes" else (PRIMES[0], PRIMES[2], PRIMES[1])
            i = (cc[0] * np.uint64(p[0]) & M32) ^ (cc[1] * np.uint64(p[1]) & M32) ^ (cc[2] * np.uint64(p[2]) & M32)      # (uint64 products wrap mod 2^64: low 32 bits right)
        else:
            i = (cc[0] + cc[1] * np.uint64(L["res"]) + cc[2] * np.uint64(L["res"] ** 2)) & M32
        out[:, c] = L["offset"] + (i % np.uint64(L["entries"])).astype(np.int64)
    return out


def level_pos(geo, L, x, mutation=None):
    """float64 x01 and pos of fp32 positions x [M, 3] (x may require grad as float64)."""
    x01 = (x.double() + geo.bound) / (2 * geo.bound)
    pos = x01 * L["scale"] + (0.0 if mutation == "pos_no_half" else 0.5)
    return x01, pos


def level_terms(geo, l, x, mutation=None):
    """Everything one level contributes: pos, e_pos [M, 3]; the per-axis blend factors a [M, 8, 3] (w_k or 1 - w_k of each corner) and
    their signs sg [8, 3] (d a / d w_k); the corner rows idx [M, 8]."""
    L = geo.levels[l]
    x01, pos = level_pos(geo, L, x, mutation)
    cell = torch.floor(pos).detach()
    w = pos - cell
    e_pos = U * (2 * x01.abs() * L["scale"] + 2 * pos.abs() + 1)        # module docstring
    if mutation == "flip_w":
        w = torch.stack([w[:, 0], 1 - w[:, 1], w[:, 2]], 1)
    d = torch.tensor(CORNERS, dtype=torch.float64)                       # [8, 3]
    a = torch.where(d[None] > 0, w[:, None, :], 1 - w[:, None, :])       # [M, 8, 3]
    sg = 2 * d - 1
    idx = torch.from_numpy(level_index(L, cell.numpy().astype(np.int64), mutation))
    return dict(pos=pos, e_pos=e_pos.detach(), a=a, sg=sg, idx=idx, s=L["scale"] / (2 * geo.bound))


def _others(a, k):
    """product of the blend factors of the two axes other than k: [M, 8]"""
    j, i = [(1, 2), (0, 2), (0, 1)][k]
    return a[:, :, j] * a[:, :, i]


def _third(a, k, j):
    return a[:, :, 3 - k - j]


def encode(geo, x, table, mutation=None, want_budget=False):
    """x [M, 3] -> enc [M, 2 n_levels] in float64 (differentiable w.r.t. a float64 x); with want_budget also its budget, per element:
        sum_k e_pos_k |d enc / d w_k|  +  16 u sum_corners |w_c f_c|
    16: hg_level_fwd forms w_c with up to 5 roundings (three 1 - w, two products) and adds eight corners with one fma rounding each
    (each bounded by u times the sum of the |w_c f_c|): 13, rounded up."""
    table = table.double()
    geo_m = geometry_of(geo, mutation)
    outs, buds = [], []
    for l in range(geo.n_levels):
        t = level_terms(geo_m, l, x, mutation)
        f = table[t["idx"]]                                               # [M, 8, 2]
        wc = t["a"].prod(-1)                                              # [M, 8]
        outs.append((wc[..., None] * f).sum(1))
        if want_budget:
            b = 16 * U * (wc[..., None] * f).abs().sum(1)
            for k in range(3):
                dk = ((t["sg"][None, :, k] * _others(t["a"], k))[..., None] * f).sum(1)       # d enc / d w_k  [M, 2]
                b = b + t["e_pos"][:, k, None] * dk.abs()
            buds.append(b.detach())
    enc = torch.cat(outs, 1)
    return (enc, torch.cat(buds, 1)) if want_budget else enc


def geometry_of(geo, mutation):
    if mutation in ("scale_no_minus1", "no_round8", "offsets"):
        return Geometry(geo.n_levels, geo.log2, geo.base, geo.max_res, geo.bound, mutation=mutation)
    return geo


def grad_x(geo, x, table, g_enc, mutation=None):
    """d sum(g_enc * encode(x)) / d x [M, 3] in float64 and its budget.  Per level l, with F = sum_c w_c v_c, v_c = f_c . g_l (the two
    features of the level) and s_l = scale_l / (2 bound) = d pos / d x:
        g_x[k] = sum_l s_l dF/dw_k,     dF/dw_k = sum_c (+-) v_c (product of the other two axes' blend factors)
        budget = sum_l  s_l ( sum_{j != k} e_pos_j |d^2 F / dw_k dw_j|  +  16 u sum_c |v|_c (other two factors) )  +  8 u |g_l|
    (F is linear in each w_k, so the error of pos_k itself does not reach dF/dw_k.)
    16: hg_level_bwd_x forms v_c with 3 roundings (two products, one sum), the other two factors with 2 (1 - w) and 2 (products), and adds
    eight corners with one rounding each: 15, rounded up.  |v|_c = |f_c0 g_0| + |f_c1 g_1|, not |v_c|: v_c's own roundings are relative to its
    two products, which may cancel.
    8, on |g_l| = |s_l dF/dw_k|: s = scale * inv_range (inv_range rounded, the product: 2), g * s (1), and the four shuffle steps that add
    the sixteen lanes of a sample (4, each bounded by u times sum_l |g_l|): 7, rounded up."""
    table, g_enc = table.double(), g_enc.double()
    geo_m = geometry_of(geo, mutation)
    gx = torch.zeros(x.shape[0], 3, dtype=torch.float64)
    bud = torch.zeros_like(gx)
    for l in range(geo.n_levels):
        t = level_terms(geo_m, l, x, mutation if mutation != "drop_s" else None)
        f, a, sg = table[t["idx"]], t["a"], t["sg"]
        g = g_enc[:, 2 * l:2 * l + 2]
        v = (f * g[:, None, :]).sum(-1)                                   # [M, 8]
        va = (f * g[:, None, :]).abs().sum(-1)
        s = 1.0 if (mutation == "drop_s" and l == 0) else t["s"]
        for k in range(3):
            gl = s * (sg[None, :, k] * _others(a, k) * v).sum(1)
            b = 16 * U * (va * _others(a, k)).sum(1)
            for j in range(3):
                if j != k:
                    d2 = (sg[None, :, k] * sg[None, :, j] * _third(a, k, j) * v).sum(1)
                    b = b + t["e_pos"][:, j] * d2.abs()
            gx[:, k] += gl
            bud[:, k] += t["s"] * b + 8 * U * gl.abs()
    return gx, bud


def grad_table(geo, x, g_enc, mutation=None, calls=1):
    """d sum(g_enc * encode(x)) / d table as a float64 index_add, sparse: (rows [K] sorted unique, value [K, 2], budget [K, 2],
    n_terms [K]) over the rows any sample touches; every other row of the gradient is exactly zero.  calls=2: what two calls into the
    same buffer leave (the same terms twice).  Per entry and feature, over the terms t = w_c g that land on it:
        budget = sum_terms ( sum_k e_pos_k |d w_c / d w_k| |g|  +  4 u |t| )  +  k u sum_terms |t|
    4 u |t|: the corner weight hg_corner_weight forms (two products and the 1 - w subtractions, which are exact for w >= 1/2 and carry
    2^-25 / (1 - w) otherwise: at most 5 u at corner 000 with all three w just below 1/2; the unit above 4 is inside k, below).
    k, hashed entries (fp32 atomics land in any order; the merged form first adds the terms of a run in the wave: fewer roundings):
        the product w_c g (1), then n_terms - 1 additions whose partial sums are bounded by sum |t| (the first lands on 0.0 exactly):
        n_terms, of k = n_terms + 2.
    k, dense entries (fp64 workspace, rounded once by the flush kernel): K_DENSE = 9 =
        the product w_c g (1)
        the merged form's segmented scan: six shuffle steps, one fp32 addition each on the path of a term (6; the plain-atomic form has none)
        the fp64 atomics: 2^-53 per term, nothing at this scale
        the flush kernel's (float)dense[j] (1), and its += into the caller's buffer (1; exact on a zeroed buffer, where this unit
        pays for the fifth rounding of the corner weight).
    With calls=2 both formulas are evaluated on the doubled list of terms (k = 2 n_terms + 2, resp. 2 x 9: the second flush adds
    a value of magnitude |r| into one of magnitude |r| and rounds at |2 r|, two units of sum |t| -- and the first call's += was exact)."""
    g_enc = g_enc.double()
    rows, vals, buds = [], [], []
    geo_m = geometry_of(geo, mutation)
    dropped = None
    for l in range(geo.n_levels):
        t = level_terms(geo_m, l, x, mutation if mutation != "drop_run_tail" else None)
        a, sg = t["a"], t["sg"]
        g = g_enc[:, 2 * l:2 * l + 2]
        term = a.prod(-1)[..., None] * g[:, None, :]                      # [M, 8, 2]
        dw = sum(t["e_pos"][:, None, k] * _others(a, k) for k in range(3))       # sum_k e_pos_k |d w_c / d w_k|  [M, 8]
        b = dw[..., None] * g.abs()[:, None, :] + 4 * U * term.abs()
        keep = torch.ones(x.shape[0], 8, dtype=torch.bool)
        if mutation == "drop_run_tail":                                   # the last sample of a run at level 0 adds nothing, at any level
            dropped = run_tail(t["idx"][:, 0]) if l == 0 else dropped
            keep[dropped] = False
        rows.append(t["idx"][keep])
        vals.append(term[keep])
        buds.append(b[keep])
    rows, vals, buds = torch.cat(rows), torch.cat(vals), torch.cat(buds)
    uniq, inv = torch.unique(rows, return_inverse=True)
    K = uniq.shape[0]
    value = torch.zeros(K, 2, dtype=torch.float64).index_add_(0, inv, vals) * calls
    budget = torch.zeros(K, 2, dtype=torch.float64).index_add_(0, inv, buds) * calls
    mag = torch.zeros(K, 2, dtype=torch.float64).index_add_(0, inv, vals.abs()) * calls
    n_terms = torch.zeros(K, dtype=torch.float64).index_add_(0, inv, torch.ones(rows.shape[0], dtype=torch.float64)) * calls
    k = torch.where(uniq < geo.n_dense, torch.full_like(n_terms, K_DENSE * calls), n_terms + 2)
    return uniq, value, budget + k[:, None] * U * mag, n_terms.long()


def run_tail(idx):
    """last sample of the longest run of consecutive samples that share the row idx[m] (the first such run on a tie)"""
    idx = idx.tolist()
    best, start = (0, 0), 0
    for m in range(1, len(idx) + 1):
        if m == len(idx) or idx[m] != idx[start]:
            if m - start > best[0]:
                best = (m - start, m - 1)
            start = m
    return best[1]


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def ambiguous(geo, x):
    """[M] bool: at some level and axis pos lies within 4 ulp (fp32) of |pos| + 1 from an integer.  E_POS < 4 u (|pos| + 1) <= that
    distance, so outside it the kernel's fp32 floor(pos) is the float64 one: the trilinear value is continuous across a cell face, but
    the x-gradient is not and the table gradient changes destination."""
    bad = torch.zeros(x.shape[0], dtype=torch.bool)
    for L in geo.levels:
        _, pos = level_pos(geo, L, x)
        ulp = torch.from_numpy(np.spacing((pos.abs() + 1).numpy().astype(np.float32)).astype(np.float64))
        bad |= ((pos - torch.round(pos)).abs() <= 4 * ulp).any(1)
    return bad


class Draw:
    """Rejection sampling that counts what it discards."""

    def __init__(self, geo, seed):
        self.geo, self.g, self.drawn, self.kept = geo, torch.Generator().manual_seed(seed), 0, 0

    def take(self, n, candidates):
        """the first n unambiguous positions among candidates(count) -> [count, 3] fp32, in the candidates' order"""
        out, have = [], 0
        while have < n:
            c = candidates(n - have + 8).float()
            ok = ~ambiguous(self.geo, c)
            # only what is consumed counts: the candidates up to the last one kept
            c_ok = c[ok][:n - have]
            used = int(ok.nonzero()[c_ok.shape[0] - 1]) + 1 if c_ok.shape[0] else c.shape[0]
            self.drawn += used
            self.kept += c_ok.shape[0]
            out.append(c_ok)
            have += c_ok.shape[0]
        return torch.cat(out)

    def uniform(self, n, half_width):
        return self.take(n, lambda k: (torch.rand(k, 3, generator=self.g, dtype=torch.float64) * 2 - 1) * half_width)

    @property
    def discarded(self):
        return 1 - self.kept / max(1, self.drawn)


def positions(geo_name, kind, M, seed=0, want_draw=False):
    """[M, 3] fp32, |x| <= 4 bound (so that (int)floorf(pos) is defined), no sample within ambiguous() of a cell face.
      inside      uniform in +-0.999 bound
      both_sides  uniform in +-2.2 bound: about 60 % of the samples have a coordinate below -bound (negative cells)
      rays        sorted depths along rays that start outside the bound, cross it and leave: runs of consecutive samples share entries at
                  the coarse levels
      repeats     one position 1, 2, 63, 64, 65 times in a row (cycled, each run a new position in +-1.5 bound): runs that end inside a
                  wave, fill one exactly, and cross into the next workgroup of the merged table-gradient kernel"""
    geo = geometry(geo_name)
    dr = Draw(geo, 7919 * (list(GEOMETRIES).index(geo_name) + 1) + 101 * SETS.index(kind) + M + 100003 * seed)
    b = geo.bound
    if kind == "inside":
        x = dr.uniform(M, 0.999 * b)
    elif kind == "both_sides":
        x = dr.uniform(M, 2.2 * b)
    elif kind == "rays":
        S = min(M, 96)
        rows = []
        for r in range(-(-M // S)):
            o = torch.nn.functional.normalize(torch.randn(3, generator=dr.g, dtype=torch.float64), dim=0) * 1.8 * b
            aim = (torch.rand(3, generator=dr.g, dtype=torch.float64) * 2 - 1) * 0.5 * b
            d = torch.nn.functional.normalize(aim - o, dim=0)
            rows.append(dr.take(S, lambda k: o + d * torch.sort(torch.rand(k, generator=dr.g, dtype=torch.float64) * 3.6 * b)[0][:, None]))
            # (the kept depths of one ray are sorted; a second batch of candidates, drawn only if 8 spares did not suffice, starts over)
        x = torch.cat(rows)[:M]
    elif kind == "repeats":
        runs, n = [], 0
        while n < M:
            runs.append(REPEATS[len(runs) % len(REPEATS)])
            n += runs[-1]
        p = dr.uniform(len(runs), 1.5 * b)
        x = torch.cat([p[i:i + 1].expand(r, 3) for i, r in enumerate(runs)])[:M]
    else:
        raise KeyError(kind)
    x = x.float().contiguous()
    assert x.shape == (M, 3) and float(x.abs().max()) <= 4 * b and not bool(ambiguous(geo, x).any())
    return (x, dr) if want_draw else x


def upstream(geo, M, seed=0, only_level=None):
    """g_enc ~ N(0, 1) [M, 2 n_levels] fp32; only_level: zero on every other level."""
    g = torch.Generator().manual_seed(2000 + seed + M)
    ge = torch.randn(M, 2 * geo.n_levels, generator=g)
    if only_level is not None:
        keep = torch.zeros(2 * geo.n_levels)
        keep[2 * only_level:2 * only_level + 2] = 1
        ge = ge * keep
    return ge.contiguous()


def ratio(err, budget):
    """largest err / budget over the elements (0 / 0 counts as 0: an exact result under a zero budget)"""
    r = torch.where(err == 0, torch.zeros_like(err), err / budget)
    return float(r.max()) if r.numel() else 0.0


# ---- the kernels' arithmetic restated in fp32 on the CPU (tests/test_hashgrid_ref.py: it stays inside 0.75 x budget) ------------------
def _f32(a):
    return np.asarray(a, np.float32)


def fp32_restatement(geo, x, table, g_enc, fma):
    """hg_cell / hg_level_fwd / hg_level_bwd_x / the table scatter as the kernels order them, in numpy fp32.  fma: the pos line as one
    fused multiply-add (evaluated exactly in float64, rounded once) or as a rounded product and a rounded sum.
    -> enc [M, 2 L], g_x [M, 3], g_table [entries, 2] (fp32 arrays)."""
    x, table, g_enc = _f32(x.numpy()), _f32(table.numpy()), _f32(g_enc.numpy())
    M = x.shape[0]
    b = np.float32(geo.bound)
    one = np.float32(1)
    enc = np.zeros((M, 2 * geo.n_levels), np.float32)
    lanes = np.zeros((M, 16, 3), np.float32)
    g_table = np.zeros((geo.total, 2), np.float32)
    dense = np.zeros((geo.n_dense, 2), np.float64)
    inv_range = one / (np.float32(2) * b)
    for l, L in enumerate(geo.levels):
        sc = np.float32(L["scale"])
        x01 = (x + b) / (np.float32(2) * b)
        pos = _f32(x01.astype(np.float64) * np.float64(sc) + 0.5) if fma else x01 * sc + np.float32(0.5)
        fl = np.floor(pos)
        w = pos - fl
        idx = level_index(L, fl.astype(np.int64))
        f = table[idx]                                                   # [M, 8, 2]
        ge = g_enc[:, 2 * l:2 * l + 2]
        acc = np.zeros((M, 2), np.float32)
        g = np.zeros((M, 3), np.float32)
        for c, (dx, dy, dz) in enumerate(CORNERS):
            wx, wy, wz = (w[:, 0] if dx else one - w[:, 0]), (w[:, 1] if dy else one - w[:, 1]), (w[:, 2] if dz else one - w[:, 2])
            wc = wx * wy * wz
            acc = _f32(wc[:, None].astype(np.float64) * f[:, c] + acc)   # fmaf(wc, f, acc)
            v = f[:, c, 0] * ge[:, 0] + f[:, c, 1] * ge[:, 1]
            g[:, 0] += (v if dx else -v) * wy * wz
            g[:, 1] += (v if dy else -v) * wx * wz
            g[:, 2] += (v if dz else -v) * wx * wy
            t = wc[:, None] * ge
            if L["hashed"]:
                np.add.at(g_table, idx[:, c], t)                         # fp32, one addition per term, in sample order
            else:
                np.add.at(dense, idx[:, c], t.astype(np.float64))
        enc[:, 2 * l:2 * l + 2] = acc
        lanes[:, l] = g * (sc * inv_range)
    for o in (8, 4, 2, 1):                                               # the xor-shuffle tree over the sixteen lanes of a sample
        lanes = lanes + lanes[:, np.arange(16) ^ o]
    g_table[:geo.n_dense] += dense.astype(np.float32)
    return torch.from_numpy(enc), torch.from_numpy(lanes[:, 0].copy()), torch.from_numpy(g_table)

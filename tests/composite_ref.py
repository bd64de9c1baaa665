"""Inputs, float64 truth, per-ray scales and the acceptance bound that the compositing kernels (csrc/composite.hip) are held to by
tests/test_gpu_composite.py, and that tests/test_composite_ref.py checks on the CPU (no GPU needed here).

The truth is oracle/ref_cpu.py `composite` in float64; the same oracle in fp32 gives the noise floor of fp32 arithmetic (e_ref).
Every error is scaled PER RAY and PER GROUP by float64 quantities only, never by anything a kernel returned:

  maps, colour / feature / beta rows of d raw:   max |float64 value| over that ray's entries of the group
  the two sigma rows of d raw:                   max(that, cancel(ray) * U(ray))

The sigma gradient is a difference of terms that cancel: in exact arithmetic d acc / d sigma_j = delta_j T_final, which is ~0 on a
saturated ray although each of the two terms is delta_j T_{j+1} large.  cancel = max_j delta_j T_{j+1} is the size of those terms
(variant B: the larger of the combined and the static chain), U the sum over the upstreams present of |upstream| times the largest
multiplier it meets on its way to a weight (table in `sigma_terms`).

bound(e_ref, E) = max(4 E, 1.5 e_ref).  E (E_MAPS, E_GRADS) is the fp32 oracle's largest error over the whole case list, measured on
the CPU and pinned by tests/test_composite_ref.py to [E/2, E].  1.5 is the project's REF_FACTOR (tests/parity_log.py).  The 4 is
derived: every quantity here inherits the rounding of 1 - expf(-x); the CPU's exp is correctly rounded (0.5 ulp), a device expf may
be off by 2 ulp, i.e. four times as far."""
import functools

import torch

from oracle import ref_cpu as O
from tests import parity_log as P

# largest per-ray-scaled error of the fp32 oracle against the float64 oracle over all_runs() (tests/test_composite_ref.py recomputes
# them and holds them to [E/2, E]).  torch's fp32 sums and exp differ a little between CPUs, hence the head-room above the measured
# values (maps: `map feat`; gradient rows: `d rgb rows`, ray 5 of variant B at S = 2).
E_MAPS = 8.0e-6
E_GRADS = 6.0e-6

UPSTREAMS = ("rgb", "feat", "disp", "acc", "depth", "weights", "beta")
FLAGS = {"A": 1, "B": 1 | 2, "C": 0, "D": 4}
WHITE_BKGD = 8
NAN_RAY = 8          # zero density: disp = 1 / (0 / 0) is NaN in the reference itself
CLAMP_RAY = 7        # z == 0: depth / sum_w = 0 <= 1e-10, disp = 1e10


def bound(e_ref, E):
    return max(4 * E, P.REF_FACTOR * e_ref)


def n_rows(tag, C):
    return 1 if tag == "D" else 3 + C + (6 if tag in ("A", "B") else 1)


@functools.lru_cache(maxsize=None)
def make_case(tag, S, N, C, seed, white_bkgd=False):
    """raw [N,S,R], z [N,S] and the seven upstreams.  Rays 3, 5, 6, 7, 8 (where N has them) have fixed roles, see below."""
    g = torch.Generator().manual_seed(seed)
    R = n_rows(tag, C)
    trans = tag in ("A", "B")
    raw = torch.randn(N, S, R, generator=g)
    i_s = 0 if tag == "D" else 3 + C
    dens = torch.nn.functional.softplus(3 * torch.randn(N, S, generator=g))
    tdens = torch.nn.functional.softplus(torch.randn(N, S, generator=g) - 1)
    z = torch.sort(0.05 + 4 * torch.rand(N, S, generator=g), -1)[0]
    if N > 3:
        dens[3] *= 40.                                    # alpha saturates to exactly 1 early
        tdens[3] *= 40.
    if N > 5:
        dens[5, S // 2:] = 0.                             # empty second half
        tdens[5, S // 2:] = 0.
    if N > 6:
        sparse = 0.05 * max(1., S / 256.)                 # the sparse ray.  No sparser: 1 - exp(-x) loses its digits in fp32, and x is
        dens[6] *= sparse                                 # delta * sigma -- past S = 256 the steps shrink, so the density grows with S
        tdens[6] *= sparse
        if S > 256 and tag != "D":                        # ... and its 300 to 500 near-equal weights meet colours and features of one sign:
            raw[6, :, :3 + C] = raw[6, :, :3 + C].abs()   # a signed sum of that many terms cancels to where fp32 itself is 1e-5 off
    if N > CLAMP_RAY:
        z[CLAMP_RAY] = 0.                                 # depth / sum_w = 0: the clamp branch of disp
    if N > NAN_RAY:
        dens[NAN_RAY] = 0.                                # no density at all: disp is NaN
        tdens[NAN_RAY] = 0.
    raw[..., i_s] = dens
    if trans:
        raw[..., i_s + 4] = tdens
        raw[..., i_s + 1:i_s + 4] = torch.sigmoid(raw[..., i_s + 1:i_s + 4])
        raw[..., i_s + 5] = torch.nn.functional.softplus(raw[..., i_s + 5])     # beta is a softplus in the model: a sum without cancellation
    ups = {k: torch.randn(N, *sh, generator=g) for k, sh in
           (("rgb", (3,)), ("feat", (C,)), ("disp", ()), ("acc", ()), ("depth", ()), ("weights", (S,)), ("beta", ()))}
    return dict(tag=tag, S=S, N=N, C=C, seed=seed, white=bool(white_bkgd), raw=raw, z=z, ups=ups,
                key=(tag, S, N, C, seed, bool(white_bkgd)))


def maps_of(case):
    return ("acc", "weights") if case["tag"] == "D" else UPSTREAMS


def disp_rays(case):
    """The rays whose disp takes part in the loss and in the comparison: all but NAN_RAY."""
    return torch.tensor([n for n in range(case["N"]) if n != NAN_RAY], dtype=torch.long)


def loss_of(case, maps, ups, only=None):
    """sum(map * upstream) over all maps, or over the single map `only`; NAN_RAY is indexed out of the disp term."""
    loss = 0.
    for k in maps_of(case):
        if only is not None and k != only:
            continue
        t = maps[k] * ups[k]
        loss = loss + (t[disp_rays(case).to(t.device)].sum() if k == "disp" else t.sum())
    return loss


def oracle_forward(case, raw, z):
    tag = case["tag"]
    o = O.composite(raw, z, output_transient=tag in ("A", "B"), test_time=tag in ("B", "D"), typ="coarse" if tag == "D" else "fine",
                    transient_at_test=tag == "A", white_bkgd=case["white"])
    return {k: getattr(o, k) for k in maps_of(case)}


def run_forward(case, dtype, only, forward):
    """(maps, d raw) of `forward(case, raw, z) -> maps` under the shared loss; float64 tensors."""
    raw = case["raw"].detach().clone().to(dtype).requires_grad_()
    maps = forward(case, raw, case["z"].to(dtype))
    loss = loss_of(case, maps, {k: v.to(dtype) for k, v in case["ups"].items()}, only)
    if torch.is_tensor(loss) and loss.requires_grad:
        loss.backward()
    g = raw.grad if raw.grad is not None else torch.zeros_like(raw)      # e.g. beta alone in variants B / C: a constant
    return {k: v.detach().double() for k, v in maps.items()}, g.double()


@functools.lru_cache(maxsize=None)
def _oracle_cached(key, dtype, only):
    return run_forward(make_case(*key), dtype, only, oracle_forward)


def run_oracle(case, dtype, only=None):
    """(maps, d raw [N,S,R]) of oracle/ref_cpu.py composite in `dtype`, as float64 tensors.  Cached: treat as read-only."""
    return _oracle_cached(case["key"], dtype, only)


def present(case, only=None):
    return tuple(k for k in maps_of(case) if only is None or k == only)


def grad_groups(case, g):
    """d raw [N,S,R] cut into the groups that are compared separately."""
    if case["tag"] == "D":
        return {"d sigma": g[..., 0]}
    C3 = 3 + case["C"]
    out = {"d rgb rows": g[..., :3], "d feat rows": g[..., 3:C3], "d sigma": g[..., C3]}
    if case["tag"] in ("A", "B"):
        out.update({"d t_rgb rows": g[..., C3 + 1:C3 + 4], "d t_sigma": g[..., C3 + 4], "d beta row": g[..., C3 + 5]})
    return out


# No scale is smaller than this: fp32 carries no relative precision below its smallest normal number (a weight behind exp(-300)
# is 1e-130 in float64 and 0 in fp32, in the reference too), so an absolute error of 2^-126 counts as one of 2^-24, not as 100 %.
SCALE_FLOOR = 2.0 ** -126 / 2.0 ** -24


def _per_ray_max(t):
    return torch.nan_to_num(t.double(), nan=0.).abs().reshape(t.shape[0], -1).amax(1).clamp_min(SCALE_FLOOR)


def sigma_terms(case, only=None):
    """cancel(ray) * U(ray) in float64, from the inputs alone.

    upstream   multiplier
    acc        1
    weights    1                                   (largest |g_weights| of the ray)
    depth      max z
    rgb        max_j sum_c |g_rgb_c colour_jc|     (+ the same over the transient colours in variant A)
    beta       max |t_beta|                        (variant A)
    disp       |g_disp| disp^2 max z / sum_w       (0 on the clamp branch; NAN_RAY takes no part)
    feat       --                                  (the weights are detached there)"""
    tag, C = case["tag"], case["C"]
    raw, z, ups = case["raw"].double(), case["z"].double(), {k: v.double() for k, v in case["ups"].items()}
    N = case["N"]
    i_s = 0 if tag == "D" else 3 + C
    trans = tag in ("A", "B")
    delta = torch.cat([z[:, 1:] - z[:, :-1], torch.full((N, 1), 1e2, dtype=torch.float64)], -1)
    s_sig = raw[..., i_s]
    t_sig = raw[..., i_s + 4] if trans else torch.zeros_like(s_sig)
    T_next = torch.cumprod(torch.exp(-delta * (s_sig + t_sig)), -1)             # T_{j+1}
    cancel = (delta * T_next).amax(1)
    if tag == "B":
        cancel = torch.maximum(cancel, (delta * torch.cumprod(torch.exp(-delta * s_sig), -1)).amax(1))
    have = present(case, only)
    zmax = z.abs().amax(1)
    U = torch.zeros(N, dtype=torch.float64)
    if "acc" in have:
        U += ups["acc"].abs()
    if "weights" in have:
        U += ups["weights"].abs().amax(1)
    if "depth" in have:
        U += ups["depth"].abs() * zmax
    if "rgb" in have:
        U += (ups["rgb"][:, None, :] * raw[..., :3]).abs().sum(-1).amax(1)
        if tag == "A":
            U += (ups["rgb"][:, None, :] * raw[..., i_s + 1:i_s + 4]).abs().sum(-1).amax(1)
    if "beta" in have and tag == "A":
        U += ups["beta"].abs() * raw[..., i_s + 5].abs().amax(1)
    if "disp" in have:
        m64, _ = run_oracle(case, torch.float64, only)
        sum_w = m64["weights"].sum(1)
        d = m64["disp"]
        t = ups["disp"].abs() * d * d * zmax / sum_w
        t = torch.where(m64["depth"] / sum_w > 1e-10, t, torch.zeros_like(t))    # clamp branch: no gradient; NaN compares false
        U += torch.nan_to_num(t, nan=0., posinf=0.)
    return cancel * U


@functools.lru_cache(maxsize=None)
def _scales_cached(key, only):
    case = make_case(*key)
    m64, g64 = run_oracle(case, torch.float64, only)
    sc = {"map " + k: _per_ray_max(v) for k, v in m64.items()}
    gg = grad_groups(case, g64)
    sc.update({k: _per_ray_max(v) for k, v in gg.items()})
    cu = sigma_terms(case, only)
    for k in ("d sigma", "d t_sigma"):
        if k in sc:
            sc[k] = torch.maximum(sc[k], cu)
    if case["C"] >= 64:                                    # the feature split: every channel against its own rows
        fr = gg["d feat rows"]
        sc["d feat rows/ch"] = torch.nan_to_num(fr, nan=0.).abs().amax(1).clamp_min(SCALE_FLOOR)      # [N, C]
    return sc


def scales(case, only=None):
    """group -> per-ray scale [N] (the per-channel group of the feature-split cases: [N, C]); float64 quantities only."""
    return _scales_cached(case["key"], only)


def quantities(case, maps, g_raw):
    """group -> tensor [N, ...] (float64, on the CPU) of one run, named like `scales`."""
    out = {"map " + k: maps[k].detach().cpu().double() for k in maps_of(case)}
    gg = grad_groups(case, g_raw.detach().cpu().double())
    out.update(gg)
    if case["C"] >= 64:
        out["d feat rows/ch"] = gg["d feat rows"]
    return out


def ray_errors(case, maps, g_raw, only=None):
    """group -> (e [N], where [N]): per ray, the largest |value - float64| / scale and its flat index in the ray.  An entry that is
    NaN in float64 must be NaN in `maps` / `g_raw` too and the other way round (AssertionError otherwise); it takes no part in any
    maximum.  That is disp of NAN_RAY and, in every run whose loss has a disp term, that ray's two sigma rows (0 x NaN in the
    backward of the division, in the reference too): the sigma rows of the zero-density ray are compared in MAGNITUDE only in the
    single-upstream runs without disp, everywhere else only their NaN pattern is."""
    m64, g64 = run_oracle(case, torch.float64, only)
    want, got, sc = quantities(case, m64, g64), quantities(case, maps, g_raw), scales(case, only)
    out = {}
    for k, w in want.items():
        v, s = got[k], sc[k]
        assert v.shape == w.shape, (k, v.shape, w.shape)
        assert torch.equal(torch.isnan(v), torch.isnan(w)), (case["key"], only, k, "NaN where float64 has none, or none where it has")
        if s.dim() == 2:                                   # per (ray, channel): [N,S,C] against [N,C]
            e = (v - w).abs() / s[:, None, :]
        else:
            e = (v - w).abs().reshape(w.shape[0], -1) / s[:, None]
        e = torch.nan_to_num(e, nan=0.).reshape(w.shape[0], -1)
        if e.shape[1] == 0:
            out[k] = (torch.zeros(w.shape[0], dtype=torch.float64), torch.zeros(w.shape[0], dtype=torch.long))
        else:
            out[k] = e.max(1)
    return out


def errors(case, maps, g_raw, only=None):
    """group -> (largest error over the rays, (ray, flat index in the ray) where); see ray_errors."""
    out = {}
    for k, (e, where) in ray_errors(case, maps, g_raw, only).items():
        n = int(e.argmax())
        out[k] = (float(e[n]), (n, int(where[n])))
    return out


ROLE_RAYS = (3, 5, 6, CLAMP_RAY, NAN_RAY)          # every other ray is an ordinary one


def is_map(group):
    return group.startswith("map ")


# ---- the case list: exactly what tests/test_gpu_composite.py runs, and what E_MAPS / E_GRADS are measured over ----------------
RAGGED_S = (2, 63, 65, 127, 130, 191, 250)
RAGGED_VARIANTS = (("A", False), ("A", True), ("B", False), ("C", False), ("D", False))
FOUR_S = (64, 128, 192, 256)
FOUR_N = (1, 3, 5, 37)
ALONE_S = (130, 192)
SPLIT_C = (64, 65, 97, 128, 131)
SPLIT_S = (64, 192, 100)
MISALIGNED = tuple((tag, S) for S in (64, 128) for tag in ("A", "D"))
DEEP_S = (300, 380, 440, 500)       # composite_fwd/bwd_kernel<OnePerLane<5>>, <6>, <7>, <8>: five to eight passes
DEEP_ALONE_S = (320, 500)
DEEP_VARIANTS = ("A", "B", "C")


def _seed(kind, tag, S, N, C, white=False):
    return 1000003 * kind + 10007 * S + 101 * N + 13 * C + 7 * ord(tag) + (1 if white else 0)


def ragged_case(tag, white, S):
    return make_case(tag, S, 11, 5, _seed(1, tag, S, 11, 5, white), white)


def four_case(tag, S, N):
    return make_case(tag, S, N, 5, _seed(2, tag, S, N, 5))


def alone_case(tag, S):
    return make_case(tag, S, 11, 5, _seed(3, tag, S, 11, 5))


def alone_upstreams(tag):
    return ("acc", "weights") if tag == "D" else UPSTREAMS


def split_case(C, S):
    return make_case("A", S, 9, C, _seed(4, "A", S, 9, C))


def misaligned_case(tag, S):
    return make_case(tag, S, 11, 5, _seed(5, tag, S, 11, 5))


def all_runs():
    """Every (case, only) whose VALUES the GPU file compares with the oracle.  (test_clamp_and_nan_rays also runs (alone_case, None),
    of which it compares the NaN pattern and nothing else.)"""
    runs = [(ragged_case(tag, white, S), None) for S in RAGGED_S for tag, white in RAGGED_VARIANTS]
    runs += [(four_case(tag, S, N), None) for S in FOUR_S for tag in ("A", "B", "C") for N in FOUR_N]
    runs += [(alone_case(tag, S), only) for S in ALONE_S for tag in ("A", "B", "C", "D") for only in alone_upstreams(tag)]
    runs += [(split_case(C, S), None) for C in SPLIT_C for S in SPLIT_S]
    runs += [(misaligned_case(tag, S), None) for tag, S in MISALIGNED]
    runs += [(ragged_case(tag, False, S), None) for S in DEEP_S for tag in DEEP_VARIANTS]
    runs += [(alone_case(tag, S), only) for S in DEEP_ALONE_S for tag in DEEP_VARIANTS for only in alone_upstreams(tag)]
    return runs

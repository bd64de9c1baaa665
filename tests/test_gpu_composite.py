"""The compositing kernels (csrc/composite.hip: composite_fwd/bwd_kernel<OnePerLane<1..8>> and <FourPerLane<1..4>>) against the float64
oracle, PER RAY and PER GROUP (each map; of d raw the static colour rows, the feature rows, static sigma, the transient colour rows,
transient sigma and the beta row), with the fp32 oracle's own error beside every number and tests/composite_ref.py's
bound = max(4 E, 1.5 e_ref) as the limit.  Inputs, scales, constants and the case list live in tests/composite_ref.py, which
tests/test_composite_ref.py checks on the CPU.  Sizes stay at N <= 37 and C <= 131; S <= 256 except for the five-to-eight-pass
cases (S = 300 .. 500), which are what reaches composite_fwd/bwd_kernel<OnePerLane<5..8>>.

What each test is for: ragged S (one sample per lane, Q = 1..4, every variant, disp included), the same at Q = 5..8 for variants
A, B and C, four samples per lane with disp and ray counts that leave segments, waves and blocks partly idle, every upstream
gradient ALONE at Q = 3, 5, 8 and four per lane (the null-pointer branches of the backward, the zero-fill of the feature rows),
the feature-channel split over blockIdx.y, pointers that are not 16-byte aligned, the clamp and NaN branches of disp, writes past
ray N, and run-to-run repeatability.  With a disp upstream the zero-density ray's two sigma rows are NaN in the reference itself
(tests/composite_ref.py ray_errors): there the NaN pattern is compared, the values only in the single-upstream runs without disp."""
import ctypes

import pytest
import torch

from tests import composite_ref as R
from tests import parity_log as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F64 = torch.float32, torch.float64


@pytest.fixture(scope="module")
def ops():
    from nefes_amd import ops as _ops
    return _ops


def flags_of(case):
    return R.FLAGS[case["tag"]] | (R.WHITE_BKGD if case["white"] else 0)


def offset_view(t, requires_grad=False):
    """`t` as a contiguous view 4 bytes into a larger buffer: (buffer, view).  The view's pointer is not 16-byte aligned."""
    n = t.numel()
    buf = torch.zeros(n + 8, device=DEV)
    buf[1:1 + n] = t.reshape(-1).to(DEV)
    buf.requires_grad_(requires_grad)
    v = buf[1:1 + n].view(t.shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return buf, v


def run_hip(ops, case, only=None, misalign=()):
    """(maps, d raw [N,S,R]) of ops.Composite under tests/composite_ref.py's loss, on the CPU."""
    N, S, C = case["N"], case["S"], case["C"]
    src = case["raw"].permute(0, 2, 1).contiguous()                  # raw_t [N,R,S]
    if "raw_t" in misalign:
        leaf, raw_t = offset_view(src, requires_grad=True)
    else:
        leaf = raw_t = src.to(DEV).requires_grad_()
    z = offset_view(case["z"])[1] if "z" in misalign else case["z"].to(DEV)
    outs = ops.Composite.apply(raw_t, z, C, flags_of(case), 0.1)
    maps = {k: v for k, v in zip(R.UPSTREAMS, outs) if k in R.maps_of(case)}
    loss = R.loss_of(case, maps, {k: v.to(DEV) for k, v in case["ups"].items()}, only)
    loss.backward()
    g = leaf.grad[1:1 + src.numel()].view(src.shape) if "raw_t" in misalign else leaf.grad      # arrives in the buffer's .grad
    return {k: v.detach().cpu() for k, v in maps.items()}, g.permute(0, 2, 1).contiguous().cpu()


def compare(test, case, maps, g, only=None):
    """Every group through parity_log.check; a group over its bound is reported with the ray and the place in the ray."""
    e_hip = R.errors(case, maps, g, only)
    e_ref = R.errors(case, *R.run_oracle(case, F32, only), only)
    over = []
    for k, (e, loc) in e_hip.items():
        E = R.E_MAPS if R.is_map(k) else R.E_GRADS
        try:
            P.check(test, k, e, e_ref[k][0], tol=4 * E, factor=P.REF_FACTOR)
        except AssertionError:
            over.append((k, f"e_hip {e:.3e}", f"e_ref {e_ref[k][0]:.3e}", f"bound {R.bound(e_ref[k][0], E):.3e}", "ray, index in ray", loc))
    assert not over, (test, over)


def name(kind, case, only=None, extra=""):
    tag = case["tag"] + ("w" if case["white"] else "")
    return f"composite.{kind}[{tag},S={case['S']},N={case['N']},C={case['C']}{',' + only if only else ''}{extra}]"


# ---- one sample per lane, Q = 1..4 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", R.RAGGED_S)
@pytest.mark.parametrize("tag,white", R.RAGGED_VARIANTS)
def test_ragged_sample_counts(ops, tag, white, S):
    case = R.ragged_case(tag, white, S)
    compare(name("ragged", case), case, *run_hip(ops, case))


# ---- one sample per lane, Q = 5..8 (S > 256): variants A, B, C with disp and every upstream ----------------------------------------
@pytest.mark.parametrize("S", R.DEEP_S)
@pytest.mark.parametrize("tag", R.DEEP_VARIANTS)
def test_five_to_eight_passes(ops, tag, S):
    case = R.ragged_case(tag, False, S)
    compare(name("deep", case), case, *run_hip(ops, case))


# ---- four samples per lane, disp compared and differentiated -----------------------------------------------------------------
@pytest.mark.parametrize("N", R.FOUR_N)
@pytest.mark.parametrize("S", R.FOUR_S)
@pytest.mark.parametrize("tag", ["A", "B", "C"])
def test_four_per_lane_with_disp(ops, tag, S, N):
    case = R.four_case(tag, S, N)
    compare(name("four", case), case, *run_hip(ops, case))


# ---- every upstream alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,S", [(tag, S) for tag in ("A", "B", "C", "D") for S in R.ALONE_S] +
                         [(tag, S) for tag in R.DEEP_VARIANTS for S in R.DEEP_ALONE_S])
def test_each_upstream_alone(ops, tag, S):
    case = R.alone_case(tag, S)
    C = case["C"]
    for only in R.alone_upstreams(tag):
        maps, g = run_hip(ops, case, only)
        compare(name("alone", case, only), case, maps, g, only)
        if tag == "D":
            continue
        if only != "feat":
            assert not bool(g[..., 3:3 + C].any()), (tag, S, only, "feature rows of d raw are not exactly 0 without a feat upstream")
        else:
            rest = torch.cat([g[..., :3], g[..., 3 + C:]], -1)
            _, g64 = R.run_oracle(case, F64, only)
            assert not bool(torch.cat([g64[..., :3], g64[..., 3 + C:]], -1).any())        # detached weights: the oracle's are zero
            assert not bool(rest.any()), (tag, S, "feat alone reaches rows other than the feature rows")


# ---- feature channels split over blockIdx.y ----------------------------------------------------------------------------------
@pytest.mark.parametrize("S", R.SPLIT_S)
@pytest.mark.parametrize("C", R.SPLIT_C)
def test_feature_split(ops, C, S):
    case = R.split_case(C, S)
    maps, g = run_hip(ops, case)
    test = name("split", case)
    compare(test, case, maps, g)                                   # all maps and groups; d raw's feature rows per (ray, channel) too
    # feat channel by channel (per-ray scale: one channel of one ray is a single sum, with cancellation)
    m64, _ = R.run_oracle(case, F64)
    m32, _ = R.run_oracle(case, F32)
    sc = R.scales(case)["map feat"][:, None]
    e_hip = ((maps["feat"].double() - m64["feat"]).abs() / sc).amax(0)
    e_ref = ((m32["feat"] - m64["feat"]).abs() / sc).amax(0)
    lim = torch.tensor([R.bound(float(e), R.E_MAPS) for e in e_ref], dtype=F64)
    c = int((e_hip / lim).argmax())
    P.check(test, f"map feat, worst channel ({c})", float(e_hip[c]), float(e_ref[c]), tol=4 * R.E_MAPS, factor=P.REF_FACTOR)
    assert bool((e_hip <= lim).all()), (test, "channels over their bound", (e_hip > lim).nonzero().flatten().tolist())


# ---- pointers that are not 16-byte aligned: S % 64 == 0 falls back to one sample per lane ---------------------------------------
# This shows that the RESULTS on such pointers are right.  It is no proof of the dispatch: it cannot see which kernel the launcher
# chose, and would not fail if the aligned16() guards were gone and the hardware served the unaligned 16-byte accesses anyway.
@pytest.mark.parametrize("misalign", [("raw_t",), ("z",), ("raw_t", "z")])
@pytest.mark.parametrize("tag,S", R.MISALIGNED)
def test_misaligned_fallback(ops, tag, S, misalign):
    case = R.misaligned_case(tag, S)
    compare(name("misaligned", case, extra="," + "+".join(misalign)), case, *run_hip(ops, case, misalign=misalign))


# ---- the clamp and NaN branches of disp ------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", R.ALONE_S)
@pytest.mark.parametrize("tag", ["A", "B", "C"])
def test_clamp_and_nan_rays(ops, tag, S):
    case = R.alone_case(tag, S)
    C3 = 3 + case["C"]
    for only in ("disp", None):
        maps, g = run_hip(ops, case, only)                         # (the NaN pattern must be the float64 oracle's: R.errors)
        R.errors(case, maps, g, only)
        assert float(maps["disp"][R.CLAMP_RAY]) == 1e10
        assert bool(torch.isnan(maps["disp"][R.NAN_RAY]))
        for k, v in maps.items():
            keep = torch.ones(case["N"], dtype=torch.bool)
            keep[R.NAN_RAY] = k != "disp"
            assert bool(torch.isfinite(v[keep]).all()), (tag, S, only, k)
        # a disp upstream meets 0 x NaN on the zero-density ray, in the reference too: its two sigma rows, nothing else
        sig = torch.zeros_like(g, dtype=torch.bool)
        sig[R.NAN_RAY, :, C3] = True
        if tag in ("A", "B"):
            sig[R.NAN_RAY, :, C3 + 4] = True
        assert bool(torch.isfinite(g[~sig]).all()), (tag, S, only)
        if only == "disp":
            assert not bool(g[R.CLAMP_RAY].any()), (tag, S, "the clamp branch passes no gradient")


# ---- nothing is written past ray N -------------------------------------------------------------------------------------------
SENTINEL = -71993.5


@pytest.mark.parametrize("N", [1, 5, 17])
@pytest.mark.parametrize("S", [64, 128, 192, 100])
@pytest.mark.parametrize("tag", ["A", "D"])
def test_no_write_past_n(ops, tag, S, N):
    from nefes_amd import lib as L
    lib, C, PAD = L.load(), 5, 8
    case = R.make_case(tag, S, N, C, 600000 + 1000 * S + N)
    Rr = R.n_rows(tag, C)
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    raw_t = case["raw"].permute(0, 2, 1).contiguous().to(DEV)
    z = case["z"].to(DEV)
    ups = {k: v.contiguous().to(DEV) for k, v in case["ups"].items()}
    assert raw_t.shape == (N, Rr, S) and z.shape == (N, S)
    full = lambda *sh: torch.full((N + PAD, *sh), SENTINEL, device=DEV)
    outs = {"acc": full(), "weights": full(S)}
    if tag != "D":
        outs.update(rgb=full(3), feat=full(C), disp=full(), depth=full(), beta=full())
    g_raw_t = full(Rr, S)
    o = lambda k: ptr(outs.get(k))
    u = lambda k: ptr(ups[k]) if k in R.maps_of(case) else None
    L.check(lib.nefes_composite_fwd(N, S, C, R.FLAGS[tag], 0.1, ptr(raw_t), ptr(z), o("rgb"), o("feat"), o("disp"), o("acc"), o("depth"),
                                    o("weights"), o("beta"), ops._stream()), "nefes_composite_fwd")
    L.check(lib.nefes_composite_bwd(N, S, C, R.FLAGS[tag], ptr(raw_t), ptr(z), u("rgb"), u("feat"), u("disp"), u("acc"), u("depth"),
                                    u("weights"), u("beta"), ptr(g_raw_t), ops._stream()), "nefes_composite_bwd")
    torch.cuda.synchronize()
    outs["d raw_t"] = g_raw_t
    for k, v in outs.items():
        v = v.cpu()
        assert bool((v[N:] == SENTINEL).all()), (tag, S, N, k, "written past ray N")
        assert not bool((v[:N] == SENTINEL).any()), (tag, S, N, k, "entries of rays below N left unwritten")


# ---- the same inputs give the same bits ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [130, 192])          # composite_fwd/bwd_kernel<OnePerLane<3>>; <FourPerLane<3>>
def test_repeatable(ops, S):
    case = R.alone_case("A", S)
    bits = lambda t: t.contiguous().view(torch.int32)
    m1, g1 = run_hip(ops, case)
    m2, g2 = run_hip(ops, case)
    assert all(torch.equal(bits(m1[k]), bits(m2[k])) for k in m1) and torch.equal(bits(g1), bits(g2))

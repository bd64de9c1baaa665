"""Float64 statements, seeded inputs and acceptance bounds for the small kernels between the large ones (csrc/refine.hip fusion_input /
feat_head / adam, csrc/rays.hip ray_grad_reduce / coarse_depths / ndc / raygen_bwd).  tests/test_gpu_glue.py holds the kernels to them
per element; tests/test_glue_ref.py checks them on the CPU (no GPU needed here).

Every reference is a few lines of plain torch written from the kernels' comments and the reference's formulas, evaluated in the dtype of
its inputs: float64 is the truth, the same lines in fp32 give the noise floor of fp32 arithmetic (e_ref).  NDC and the coarse depths are
oracle/ref_cpu.py `ndc_warp` / `coarse_depths` and are not restated.  Two kinds of bound:

  three-way (tests/parity_log.py check): e_hip <= max(tol, 1.5 e_ref), tol one of the project's existing figures
      TOL_FP32 = 2e-6   a single fp32 operation chain (test_bicubic_upsample_matches_torch, the prepared-loss tests)
      TOL_DEPTH = 2e-7  test_ndc_and_depths' rtol for the depths
      TOL_NDC = 1e-4    the north star
  derived (sums): |hip - float64| <= k u sum|terms| per element, u = 2^-24, k the number of roundings on the longest path from a term
      to the stored result in ANY summation order (feat_head: F + 1 terms and the output, F + 2; its backward C terms and the output,
      C + 1; ray_grad_reduce: the one rounding of a float64-accumulated sum, doubled; its g_d: the fp32 product as well, 3)."""
import functools
import math

import torch

from oracle import ref_cpu as O
from tests import parity_log as P

U = 2.0 ** -24
TOL_FP32 = 2e-6
TOL_DEPTH = 2e-7
TOL_NDC = P.NORTH_STAR_TOL
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)        # FusionNet's colour normalisation


def rel_max(a, ref):
    """|a - ref| over the tensor, divided by the tensor's largest float64 magnitude."""
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-30))


def rel_elem(a, ref, floor=1e-30):
    """Largest per-element relative distance, each element's magnitude floored at `floor`."""
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    return float(((a - ref).abs() / ref.abs().clamp_min(floor)).max())


def ratio(a, ref, bound):
    """Largest |a - ref| / bound over the elements (0 / 0 counts as 0: an exact result under a zero bound)."""
    err = (a.detach().cpu().double() - ref.detach().cpu().double()).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max())


# ---- fusion_input ------------------------------------------------------------------------------------------------------------------
FUSION_SHAPES = [(1, 5, 13, 1), (2, 7, 9, 64), (3, 8, 8, 65), (2, 3, 43, 130), (1, 60, 80, 128)]      # (B, H, W, C)
LIN_MAX = 4.0            # |K rgb + b| <= 4: sigmoid stays in (0.018, 0.982)


def fusion_input(rgb, feat, affine, B, H, W, mean, std):
    """y = sigmoid(rgb K^T + b) per image (affine [B, 12] = K row-major, then b), (y - mean) / std, cat with feat -> [B, 3+C, H, W]."""
    y = rgb.reshape(B, H * W, 3)
    if affine is not None:
        K, b = affine[:, :9].reshape(B, 3, 3), affine[:, 9:]
        y = torch.sigmoid(y @ K.transpose(1, 2) + b[:, None, :])
    y = (y - torch.tensor(mean, dtype=rgb.dtype)) / torch.tensor(std, dtype=rgb.dtype)
    x = torch.cat([y, feat.reshape(B, H * W, -1)], -1)
    return x.permute(0, 2, 1).reshape(B, -1, H, W)


@functools.lru_cache(maxsize=None)
def fusion_case(B, H, W, C):
    """fp32 rgb in [0, 1], feat, an affine per image with |K rgb + b| <= LIN_MAX on the whole colour cube, and an upstream g_x."""
    g = torch.Generator().manual_seed(1000 * B + 100 * H + 10 * W + C)
    N = B * H * W
    rgb, feat = torch.rand(N, 3, generator=g), torch.randn(N, C, generator=g)
    affine = torch.randn(B, 12, generator=g)
    k, b = affine[:, :9].reshape(B, 3, 3), affine[:, 9:]
    affine = affine * (0.999 * LIN_MAX / (k.abs().sum(-1) + b.abs()).max(-1).values)[:, None]       # rows of |K| 1 + |b| bound |lin|
    return dict(rgb=rgb, feat=feat, affine=affine.contiguous(), g_x=torch.randn(B, 3 + C, H, W, generator=g))


def fusion_eval(case, shape, with_affine, dtype):
    """-> (x[:, :3], g_rgb) of the reference in `dtype`."""
    B, H, W, _ = shape
    rgb = case["rgb"].to(dtype).clone().requires_grad_()
    x = fusion_input(rgb, case["feat"].to(dtype), case["affine"].to(dtype) if with_affine else None, B, H, W, MEAN, STD)
    g_rgb, = torch.autograd.grad(x, rgb, case["g_x"].to(dtype))
    return x[:, :3].detach(), g_rgb


# ---- feat_head ---------------------------------------------------------------------------------------------------------------------
HEAD_SHAPES = [(1, 1, 1), (3, 17, 15), (5, 128, 64), (2, 129, 16), (2, 16, 128), (2, 130, 127), (4, 256, 255)]     # (N, C, F)


def feat_head(gmap, w, b):
    F = w.shape[1]
    return gmap[:, :F] @ w.T + gmap[:, F:] * b


def feat_head_abs(gmap, w, b):
    """sum_f |g_f w_cf| + |g_F b_c|: the size of the terms of feat_head's sum."""
    return feat_head(gmap.abs(), w.abs(), b.abs())


def feat_head_bwd(g_feat, w, b):
    """d / d gmap of (feat_head * g_feat).sum(): [N, F + 1], column F the bias column."""
    return g_feat @ torch.cat([w, b[:, None]], 1)


def feat_head_bwd_abs(g_feat, w, b):
    return feat_head_bwd(g_feat.abs(), w.abs(), b.abs())


@functools.lru_cache(maxsize=None)
def head_case(N, C, F):
    g = torch.Generator().manual_seed(7 + 100000 * N + 300 * C + F)
    return dict(gmap=torch.randn(N, F + 1, generator=g), w=torch.randn(C, F, generator=g) / math.sqrt(F), b=torch.randn(C, generator=g),
                g_feat=torch.randn(N, C, generator=g))


def head_bounds(case):
    """(forward bound [N, C], backward bound [N, F + 1]) from float64 magnitudes of the fp32 inputs."""
    d = {k: v.double() for k, v in case.items()}
    C, F = d["w"].shape
    return (F + 2) * U * feat_head_abs(d["gmap"], d["w"], d["b"]), (C + 1) * U * feat_head_bwd_abs(d["g_feat"], d["w"], d["b"])


# ---- Adam --------------------------------------------------------------------------------------------------------------------------
ADAM_SIZES = {1: [(1,)], 6: [(1,), (2,), (3,)], 7: [(3,), (2, 2)], 1024: [(1000,), (17,), (7,)]}      # total n -> parameter shapes
ADAM_STEPS, ADAM_CHECK = 60, (1, 2, 10, 60)
ADAM_ZERO, ADAM_TINY, ADAM_HUGE = 0, 1, 2            # flat indices (where n has them) of the three special elements
BETAS, EPS = (0.9, 0.999), 1e-8


def adam(p, grads, lrs, steps, betas=BETAS, eps=EPS):
    """torch.optim.Adam's single-tensor update (no weight decay, no amsgrad) on the flat `p` with a learning rate per element, in p's
    dtype: grads [steps, n] -> [(p, m, v) after step 1, 2, ...]."""
    b1, b2 = betas
    p, m, v, out = p.clone(), torch.zeros_like(p), torch.zeros_like(p), []
    for t in range(1, steps + 1):
        g = grads[t - 1]
        m = m + (1 - b1) * (g - m)
        v = b2 * v + (1 - b2) * g * g
        denom = v.sqrt() / math.sqrt(1 - b2 ** t) + eps
        p = p - lrs / (1 - b1 ** t) * (m / denom)
        out.append((p, m, v))
    return out


def adam_lrs(n):
    """One learning rate per parameter of ADAM_SIZES[n], log-spaced over [1e-5, 1e-2] (one parameter: 1e-3)."""
    k = len(ADAM_SIZES[n])
    return [1e-3] if k == 1 else [10.0 ** (-5 + 3 * i / (k - 1)) for i in range(k)]


@functools.lru_cache(maxsize=None)
def adam_case(n):
    """p0 [n] with 1 <= |p| < 2, grads [steps, n], lr per element (float64).  Every element's gradient keeps its sign and stays within a
    factor 3 of its own scale (1e-3 .. 10, log-uniform), so that m never cancels and per-element relative errors mean something; element
    ADAM_ZERO's is exactly 0 from the first step, ADAM_TINY's ~1e-12, ADAM_HUGE's ~1e6 (where n >= 3)."""
    g = torch.Generator().manual_seed(4242 + n)
    sign = lambda: torch.randint(0, 2, (n,), generator=g).float() * 2 - 1
    p0 = sign() * (1 + torch.rand(n, generator=g))
    scale = sign() * 10.0 ** (torch.rand(n, generator=g) * 4 - 3)
    if n >= 3:
        scale[ADAM_ZERO], scale[ADAM_TINY], scale[ADAM_HUGE] = 0.0, 1e-12, -1e6
    grads = scale * (0.5 + torch.rand(ADAM_STEPS, n, generator=g))
    lr = torch.cat([torch.full((math.prod(s),), lr, dtype=torch.float64) for s, lr in zip(ADAM_SIZES[n], adam_lrs(n))])
    return dict(p0=p0, grads=grads, lr=lr)


def split(flat, n):
    """The flat [n] tensor as the parameters of ADAM_SIZES[n] (copies)."""
    out, off = [], 0
    for s in ADAM_SIZES[n]:
        k = math.prod(s)
        out.append(flat[off:off + k].reshape(s).clone())
        off += k
    return out


def torch_adam(n, dtype):
    """torch.optim.Adam on the CPU in `dtype`, one parameter group per parameter -> {step: (p, m, v) flat} for ADAM_CHECK."""
    case = adam_case(n)
    params = [t.to(dtype).requires_grad_() for t in split(case["p0"], n)]
    opt = torch.optim.Adam([dict(params=[p], lr=lr) for p, lr in zip(params, adam_lrs(n))], betas=BETAS, eps=EPS, foreach=False)
    out = {}
    for t in range(1, ADAM_STEPS + 1):
        for p, gr in zip(params, split(case["grads"][t - 1], n)):
            p.grad = gr.to(dtype)
        opt.step()
        if t in ADAM_CHECK:
            flat = lambda f: torch.cat([f(p).detach().reshape(-1).clone() for p in params])
            out[t] = (flat(lambda p: p), flat(lambda p: opt.state[p]["exp_avg"]), flat(lambda p: opt.state[p]["exp_avg_sq"]))
    return out


@functools.lru_cache(maxsize=None)
def adam_truth(n):
    """{step: (p, m, v)} of `adam` in float64 on the fp32 inputs, for ADAM_CHECK."""
    case = adam_case(n)
    res = adam(case["p0"].double(), case["grads"].double(), case["lr"], ADAM_STEPS)
    return {t: res[t - 1] for t in ADAM_CHECK}


# ---- ray_grad_reduce ---------------------------------------------------------------------------------------------------------------
REDUCE_SHAPES = [(1, 1), (3, 5), (5, 21), (4, 22), (7, 64), (6, 65), (9, 192), (2, 257)]        # (N, S)


def ray_reduce(z, g_pts, g_vs):
    """pts = o + d z (per sample), so g_o = sum_s g_pts, g_d = sum_s g_pts z, and g_v = sum_s g_vs; then the same sums over absolute
    values: (g_o, g_d, g_v, a_o, a_d, a_v), each [N, 3] (g_v, a_v zero without g_vs)."""
    gz = g_pts * z[..., None]
    gv = g_vs if g_vs is not None else torch.zeros_like(g_pts)
    return g_pts.sum(1), gz.sum(1), gv.sum(1), g_pts.abs().sum(1), gz.abs().sum(1), gv.abs().sum(1)


@functools.lru_cache(maxsize=None)
def reduce_case(N, S):
    g = torch.Generator().manual_seed(31 * N + S)
    return dict(z=0.5 + 5.5 * torch.rand(N, S, generator=g).sort(-1).values, g_pts=torch.randn(N, S, 3, generator=g),
                g_vs=torch.randn(N, S, 3, generator=g))


# ---- coarse depths -----------------------------------------------------------------------------------------------------------------
DEPTH_N, DEPTH_NC = 9, (1, 2, 37, 64)
DEPTH_NEAR, DEPTH_FAR = 0.5, 6.0                     # the scalar entry's bounds


def _round_trips(x):
    return 1 / (1 / x) == x


@functools.lru_cache(maxsize=None)
def depth_case(Nc):
    """batch [N, 21] with (near, far) per ray in columns 6:8 (near >= 0.25, far >= near + 1) and garbage elsewhere; jitter [N, Nc].
    near and far are drawn among the fp32 numbers with 1 / (1 / x) == x: at t = 0 and t = 1 the lindisp formula IS that round trip, and
    from any other number the reference's own fp32 result leaves [near, far] by an ulp (a third of all draws)."""
    g = torch.Generator().manual_seed(77 + Nc)
    batch = torch.randn(DEPTH_N, 21, generator=g) * 100
    near = 0.25 + 1.5 * torch.rand(8 * DEPTH_N, generator=g)
    far = near + 1 + 4 * torch.rand(8 * DEPTH_N, generator=g)
    keep = (_round_trips(near) & _round_trips(far)).nonzero().flatten()[:DEPTH_N]
    batch[:, 6], batch[:, 7] = near[keep], far[keep]
    return dict(batch=batch, t_rand=torch.rand(DEPTH_N, Nc, generator=g))


def depth_ref(Nc, lindisp, jitter, per_ray, dtype):
    case = depth_case(Nc)
    if per_ray:
        near, far = case["batch"][:, 6:7].to(dtype), case["batch"][:, 7:8].to(dtype)
    else:
        near, far = torch.full((DEPTH_N, 1), DEPTH_NEAR, dtype=dtype), torch.full((DEPTH_N, 1), DEPTH_FAR, dtype=dtype)
    return O.coarse_depths(near, far, Nc, lindisp, case["t_rand"].to(dtype) if jitter else None), near, far


def depth_rows_ok(z, near, far):
    """Every row non-decreasing and inside [near, far] (z, near, far in one dtype)."""
    return bool((z[:, 1:] >= z[:, :-1]).all()) and bool((z >= near).all()) and bool((z <= far).all())


# ---- NDC ---------------------------------------------------------------------------------------------------------------------------
NDC_N = (1, 255, 256, 257, 1000)
NDC_GEOM = [(6, 8, 7.3, 1.0), (9, 5, 4.1, 0.5)]      # (H, W, focal, near)
NDC_MIN_Z = 0.2


@functools.lru_cache(maxsize=None)
def ndc_case(n, near):
    """Forward-facing rays away from the warp's two poles: |d_z| >= 0.2 and |o_z + t d_z| = near >= 0.2 hold by construction
    (d_z in [-1.5, -0.2], the shifted origin lies on the near plane z = -near); o_z in [-0.3, 0.5] keeps t of order one."""
    g = torch.Generator().manual_seed(500 + n + int(near * 10))
    o = torch.cat([torch.randn(n, 2, generator=g), torch.rand(n, 1, generator=g) * 0.8 - 0.3], 1)
    d = torch.cat([torch.randn(n, 2, generator=g) * 0.5, -(NDC_MIN_Z + 1.3 * torch.rand(n, 1, generator=g))], 1)
    return dict(o=o, d=d, g_o=torch.randn(n, 3, generator=g), g_d=torch.randn(n, 3, generator=g))


def ndc_eval(n, geom, dtype, which="both"):
    """-> (out_o, out_d, g_rays_o, g_rays_d) of O.ndc_warp in `dtype`; `which` = 'both' | 'o' | 'd' upstream gradients present."""
    H, W, focal, near = geom
    case = ndc_case(n, near)
    o, d = case["o"].to(dtype).clone().requires_grad_(), case["d"].to(dtype).clone().requires_grad_()
    oo, od = O.ndc_warp(H, W, focal, near, o, d)
    loss = sum((x * case[k].to(dtype)).sum() for x, k, on in ((oo, "g_o", which != "d"), (od, "g_d", which != "o")) if on)
    go, gd = torch.autograd.grad(loss, (o, d))
    return oo.detach(), od.detach(), go, gd

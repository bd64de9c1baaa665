// The training step's losses (script/models/losses.py:4-173: ColorLoss, ColorFeatureLoss, ColorFeatureFusionLoss, NerfWLoss,
// ColorFeatureFusionNerfWLoss), forward and backward.  In torch every term is a chain of sub / pow / div / log / mean / mul / add
// launches plus autograd's backward of each: several dozen launches of 5-10 us around 6144 rays.  Here: two launches forward (per-block
// partial sums, one finalising block), one launch backward, whatever the class and its switches.
//
//   colour, plain   coef (mean((rgb_fine - t)^2) [+ mean((rgb_coarse - t)^2)])
//   colour, NeRF-W  c_l = 1/2 mean((rgb_coarse - t)^2);  f_l = 1/2 mean((rgb_fine - t)^2), or with beta mean((rgb_fine - t)^2 / (2 beta^2)),
//                   b_l = 3 + mean(log beta), s_l = lambda_u mean(transient_sigmas);  each times coef, the loss is their sum
//   features        per tensor mean((a - b)^2), mean(|a - b|), or 1 - mean_n cos(a_n, b_n) over the channels (each norm clamped at 1e-8);
//                   loss_f = fine [+ coarse], loss_fusion = fusion
//
// Arithmetic: every element is widened to fp64 first, every sum is fp64 in a fixed order -- a thread's elements in ascending order, the
// wave's lanes by wave_sum's tree, the block's four waves in order, the blocks' partials by the same scheme in the finalising block --
// and each output is rounded to fp32 once.  No atomics: two calls on the same inputs return the same bits.
// A block owns NEFES_TRAIN_LOSS_ROWS consecutive rays in both directions.  transient_sigmas is read through its row stride (render()'s
// raw_f[:, ch, :] is a view with row stride R S); its gradient is ONE number, g coef lambda_u / (N S), which the caller expands.
#include <hip/hip_runtime.h>

#include "../../include/nefes_hip.h"
#include "wave.h"

namespace {

constexpr int kRows = NEFES_TRAIN_LOSS_ROWS, kThreads = 256, kWaves = kThreads / 64;
constexpr int kSlots = 8;                       // doubles per block in the scratch: c, f, b, s, feat fine, feat coarse, feat fusion, spare
constexpr int kSums = 7;
constexpr double kCosEps = 1e-8;                // torch.nn.CosineSimilarity's default eps
constexpr int kMaxInner = 1 << 20;              // C and S: kRows * C stays far inside an int

struct LossIn {
    const float *rgb_fine, *rgb_coarse, *rgb_target, *beta, *sigmas, *feat_fine, *feat_coarse, *feat_fusion, *feat_target;
};
struct LossGrad {
    float *rgb_fine, *rgb_coarse, *beta, *sigma, *feat_fine, *feat_coarse, *feat_fusion;
};

// sum over this block's rows [r0, r0 + nr) of one feature tensor's per-element (MSE, L1) or per-row (COS) term; a partial per thread
__device__ __forceinline__ double feat_partial(int kind, const float* __restrict__ a, const float* __restrict__ b, int r0, int nr, int C) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double acc = 0.0;
    if (kind == NEFES_LOSS_FEAT_COS) {
        for (int r = wave; r < nr; r += kWaves) {                 // wave-uniform: every lane reaches the wave sums
            const float* ra = a + (long)(r0 + r) * C;
            const float* rb = b + (long)(r0 + r) * C;
            double dot = 0.0, aa = 0.0, bb = 0.0;
            for (int c = lane; c < C; c += 64) {
                const double x = (double)ra[c], y = (double)rb[c];
                dot += x * y;
                aa += x * x;
                bb += y * y;
            }
            dot = wave_sum(dot);
            aa = wave_sum(aa);
            bb = wave_sum(bb);
            const double na = sqrt(aa), nb = sqrt(bb);
            if (lane == 0) acc += dot / ((na > kCosEps ? na : kCosEps) * (nb > kCosEps ? nb : kCosEps));
        }
        return acc;
    }
    const long base = (long)r0 * C;
    const int n = nr * C;
    for (int e = tid; e < n; e += kThreads) {
        const double dd = (double)a[base + e] - (double)b[base + e];
        acc += kind == NEFES_LOSS_FEAT_L1 ? fabs(dd) : dd * dd;
    }
    return acc;
}

// the block's kSums sums from its threads' partials, fixed order; valid on threads 0..kSums-1 after the call
__device__ __forceinline__ double block_sums(double (&acc)[kSums], double (*red)[kSlots]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < kSums; ++k) {
        const double v = wave_sum(acc[k]);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    return tid < kSums ? ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid] : 0.0;
}

__global__ __launch_bounds__(kThreads) void train_loss_partial_kernel(NefesTrainLossDesc d, LossIn p, double* __restrict__ part) {
    __shared__ double red[kWaves][kSlots];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r0 = (int)blockIdx.x * kRows, nr = d.N - r0 < kRows ? d.N - r0 : kRows;
    const bool fine = d.present & NEFES_LOSS_HAS_RGB_FINE, coarse = d.present & NEFES_LOSS_HAS_RGB_COARSE;
    const bool beta = d.present & NEFES_LOSS_HAS_BETA;
    double acc[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int e = tid; e < nr * 3; e += kThreads) {
        const long i = (long)r0 * 3 + e;
        const double t = (double)p.rgb_target[i];
        if (coarse) {
            const double dd = (double)p.rgb_coarse[i] - t;
            acc[0] += dd * dd;
        }
        if (fine) {
            const double dd = (double)p.rgb_fine[i] - t;
            double q = dd * dd;
            if (beta) {
                const double bt = (double)p.beta[r0 + e / 3];
                q = q / (2.0 * (bt * bt));
            }
            acc[1] += q;
        }
    }
    if (beta) {
        for (int e = tid; e < nr; e += kThreads) acc[2] += log((double)p.beta[r0 + e]);
        for (int r = wave; r < nr; r += kWaves) {
            const float* row = p.sigmas + (long)(r0 + r) * d.sigma_row_stride;
            for (int c = lane; c < d.S; c += 64) acc[3] += (double)row[c];
        }
    }
    if (d.present & NEFES_LOSS_HAS_FEAT_FINE) acc[4] = feat_partial(d.feat_kind, p.feat_fine, p.feat_target, r0, nr, d.C);
    if (d.present & NEFES_LOSS_HAS_FEAT_COARSE) acc[5] = feat_partial(d.feat_kind, p.feat_coarse, p.feat_target, r0, nr, d.C);
    if (d.present & NEFES_LOSS_HAS_FEAT_FUSION) acc[6] = feat_partial(d.feat_kind, p.feat_fusion, p.feat_target, r0, nr, d.C);
    const double s = block_sums(acc, red);
    if (tid < kSums) part[(long)blockIdx.x * kSlots + tid] = s;
}

__device__ __forceinline__ double feat_term(int kind, double sum, double N, double C) {
    return kind == NEFES_LOSS_FEAT_COS ? 1.0 - sum / N : sum / (N * C);
}

__global__ __launch_bounds__(kThreads) void train_loss_final_kernel(NefesTrainLossDesc d, int n_blocks, const double* __restrict__ part,
                                                                    float* __restrict__ terms, float* __restrict__ losses) {
    __shared__ double red[kWaves][kSlots];
    __shared__ double tot[kSlots];
    const int tid = threadIdx.x;
    double acc[kSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = tid; b < n_blocks; b += kThreads) {
#pragma unroll
        for (int k = 0; k < kSums; ++k) acc[k] += part[(long)b * kSlots + k];
    }
    const double s = block_sums(acc, red);
    if (tid < kSums) tot[tid] = s;
    __syncthreads();
    if (tid != 0) return;
    const bool fine = d.present & NEFES_LOSS_HAS_RGB_FINE, coarse = d.present & NEFES_LOSS_HAS_RGB_COARSE;
    const bool beta = d.present & NEFES_LOSS_HAS_BETA, nerfw = d.present & NEFES_LOSS_NERFW;
    const double N = (double)d.N, coef = (double)d.coef;
    double t[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const double half = nerfw ? 0.5 : 1.0;
    if (coarse) t[0] = coef * (half * (tot[0] / (3.0 * N)));
    if (fine) t[1] = coef * ((beta ? 1.0 : half) * (tot[1] / (3.0 * N)));
    if (beta) {
        t[2] = coef * (3.0 + tot[2] / N);
        t[3] = coef * ((double)d.lambda_u * (tot[3] / (N * (double)d.S)));
    }
    if (d.present & NEFES_LOSS_HAS_FEAT_FINE) t[4] = feat_term(d.feat_kind, tot[4], N, (double)d.C);
    if (d.present & NEFES_LOSS_HAS_FEAT_COARSE) t[5] = feat_term(d.feat_kind, tot[5], N, (double)d.C);
    if (d.present & NEFES_LOSS_HAS_FEAT_FUSION) t[6] = feat_term(d.feat_kind, tot[6], N, (double)d.C);
#pragma unroll
    for (int k = 0; k < 8; ++k) terms[k] = (float)t[k];
    losses[0] = (float)(nerfw ? ((t[0] + t[1]) + t[2]) + t[3] : t[1] + t[0]);
    losses[1] = (float)(t[4] + t[5]);
    losses[2] = (float)t[6];
}

// d (k * term) / d a for this block's rows of one feature tensor; k = upstream gradient of the term
__device__ __forceinline__ void feat_grad(int kind, double k, const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ g,
                                          int r0, int nr, int C, double N) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (kind == NEFES_LOSS_FEAT_COS) {
        // cos = a.b / (max(|a|, eps) max(|b|, eps)):  d cos / d a = b / (|a||b|) - (a.b) a / (|a|^3 |b|); a clamped norm is a constant, so
        // below eps the second term drops and the first keeps eps in |a|'s place -- large (1 / eps) but finite, where autograd through
        // torch's norm returns 1e8-sized or NaN values.  Rows with norms under 1e-3 are outside what the tests pin.
        const double kk = -k / N;
        for (int r = wave; r < nr; r += kWaves) {
            const long off = (long)(r0 + r) * C;
            double dot = 0.0, aa = 0.0, bb = 0.0;
            for (int c = lane; c < C; c += 64) {
                const double x = (double)a[off + c], y = (double)b[off + c];
                dot += x * y;
                aa += x * x;
                bb += y * y;
            }
            dot = wave_sum(dot);
            aa = wave_sum(aa);
            bb = wave_sum(bb);
            const double na = sqrt(aa), nb = sqrt(bb), nbc = nb > kCosEps ? nb : kCosEps;
            const double k1 = na > kCosEps ? kk / (na * nbc) : kk / (kCosEps * nbc);
            const double k2 = na > kCosEps ? kk * dot / (na * na * na * nbc) : 0.0;
            for (int c = lane; c < C; c += 64) g[off + c] = (float)(k1 * (double)b[off + c] - k2 * (double)a[off + c]);
        }
        return;
    }
    const long base = (long)r0 * C;
    const int n = nr * C;
    const double kk = k / (N * (double)C);
    for (int e = tid; e < n; e += kThreads) {
        const double dd = (double)a[base + e] - (double)b[base + e];
        // L1: sign(0) = 0, as torch's
        g[base + e] = (float)(kind == NEFES_LOSS_FEAT_L1 ? (dd > 0.0 ? kk : (dd < 0.0 ? -kk : 0.0)) : 2.0 * kk * dd);
    }
}

__global__ __launch_bounds__(kThreads) void train_loss_bwd_kernel(NefesTrainLossDesc d, LossIn p, const float* __restrict__ g_color,
                                                                  const float* __restrict__ g_f, const float* __restrict__ g_fusion, LossGrad o) {
    const int tid = threadIdx.x;
    const int r0 = (int)blockIdx.x * kRows, nr = d.N - r0 < kRows ? d.N - r0 : kRows;
    const bool beta = d.present & NEFES_LOSS_HAS_BETA, nerfw = d.present & NEFES_LOSS_NERFW;
    const double N = (double)d.N, coef = (double)d.coef;
    const double gc = g_color ? (double)g_color[0] : 0.0, gf = g_f ? (double)g_f[0] : 0.0, gu = g_fusion ? (double)g_fusion[0] : 0.0;
    const double kc = gc * coef * (nerfw ? 1.0 : 2.0) / (3.0 * N);           // d (coef [1/2] mean(dd^2)) / d x = kc dd
    if (o.rgb_fine || o.rgb_coarse) {
        for (int e = tid; e < nr * 3; e += kThreads) {
            const long i = (long)r0 * 3 + e;
            const double t = (double)p.rgb_target[i];
            if (o.rgb_coarse) o.rgb_coarse[i] = (float)(kc * ((double)p.rgb_coarse[i] - t));
            if (o.rgb_fine) {
                double v = kc * ((double)p.rgb_fine[i] - t);
                if (beta) {
                    const double bt = (double)p.beta[r0 + e / 3];
                    v = v / (bt * bt);                                       // d (dd^2 / (2 beta^2)) / d x = dd / beta^2
                }
                o.rgb_fine[i] = (float)v;
            }
        }
    }
    if (o.beta) {
        for (int e = tid; e < nr; e += kThreads) {
            const long i = (long)(r0 + e) * 3;
            const double bt = (double)p.beta[r0 + e];
            double ss = 0.0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double dd = (double)p.rgb_fine[i + c] - (double)p.rgb_target[i + c];
                ss += dd * dd;
            }
            // f_l: -sum_c dd^2 / beta^3 / (3 N);  b_l: 1 / (beta N)
            o.beta[r0 + e] = (float)(gc * coef * (1.0 / (bt * N) - ss / (bt * bt * bt) / (3.0 * N)));
        }
    }
    if (o.sigma && blockIdx.x == 0 && tid == 0) o.sigma[0] = (float)(gc * coef * (double)d.lambda_u / (N * (double)d.S));
    if (o.feat_fine) feat_grad(d.feat_kind, gf, p.feat_fine, p.feat_target, o.feat_fine, r0, nr, d.C, N);
    if (o.feat_coarse) feat_grad(d.feat_kind, gf, p.feat_coarse, p.feat_target, o.feat_coarse, r0, nr, d.C, N);
    if (o.feat_fusion) feat_grad(d.feat_kind, gu, p.feat_fusion, p.feat_target, o.feat_fusion, r0, nr, d.C, N);
}

// 0, or the refusal: everything here is decided before any HIP call
int check_desc(const NefesTrainLossDesc* d, const LossIn& p) {
    if (!d || d->N <= 0 || !p.rgb_target) return NEFES_E_BADARG;
    const unsigned m = d->present;
    if (m & ~(unsigned)NEFES_LOSS_PRESENT_ALL) return NEFES_E_BADARG;
    const bool nerfw = m & NEFES_LOSS_NERFW;
    if (nerfw ? !(m & NEFES_LOSS_HAS_RGB_COARSE) : !(m & NEFES_LOSS_HAS_RGB_FINE)) return NEFES_E_BADARG;      // the class's required colour
    if ((m & NEFES_LOSS_HAS_RGB_FINE) && !p.rgb_fine) return NEFES_E_BADARG;
    if ((m & NEFES_LOSS_HAS_RGB_COARSE) && !p.rgb_coarse) return NEFES_E_BADARG;
    if (m & NEFES_LOSS_HAS_BETA) {
        if (!nerfw || !(m & NEFES_LOSS_HAS_RGB_FINE) || !p.beta || !p.sigmas || d->S <= 0 || d->sigma_row_stride < d->S) return NEFES_E_BADARG;
        if (d->S > kMaxInner) return NEFES_E_UNSUPPORTED;
    }
    if (m & (NEFES_LOSS_HAS_FEAT_FINE | NEFES_LOSS_HAS_FEAT_COARSE | NEFES_LOSS_HAS_FEAT_FUSION)) {
        if (d->feat_kind != NEFES_LOSS_FEAT_MSE && d->feat_kind != NEFES_LOSS_FEAT_L1 && d->feat_kind != NEFES_LOSS_FEAT_COS) return NEFES_E_BADARG;
        if (d->C <= 0 || !p.feat_target) return NEFES_E_BADARG;
        if ((m & NEFES_LOSS_HAS_FEAT_FINE) && !p.feat_fine) return NEFES_E_BADARG;
        if ((m & NEFES_LOSS_HAS_FEAT_COARSE) && !p.feat_coarse) return NEFES_E_BADARG;
        if ((m & NEFES_LOSS_HAS_FEAT_FUSION) && !p.feat_fusion) return NEFES_E_BADARG;
        if (d->C > kMaxInner) return NEFES_E_UNSUPPORTED;
    }
    return 0;
}

inline int n_blocks_of(int N) { return (N + kRows - 1) / kRows; }

}  // namespace

extern "C" size_t nefes_train_loss_scratch_doubles(int N) { return N > 0 ? (size_t)n_blocks_of(N) * kSlots : 0; }

extern "C" int nefes_train_loss_fwd(const NefesTrainLossDesc* desc, const float* rgb_fine, const float* rgb_coarse, const float* rgb_target,
                                    const float* beta, const float* transient_sigmas, const float* feat_fine, const float* feat_coarse,
                                    const float* feat_fusion, const float* feat_target, double* scratch, float* terms, float* losses,
                                    void* stream) {
    const LossIn p{rgb_fine, rgb_coarse, rgb_target, beta, transient_sigmas, feat_fine, feat_coarse, feat_fusion, feat_target};
    if (const int rc = check_desc(desc, p)) return rc;
    if (!scratch || !terms || !losses) return NEFES_E_BADARG;
    const int nb = n_blocks_of(desc->N);
    hipLaunchKernelGGL(train_loss_partial_kernel, dim3((unsigned)nb), dim3(kThreads), 0, (hipStream_t)stream, *desc, p, scratch);
    hipLaunchKernelGGL(train_loss_final_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, *desc, nb, (const double*)scratch, terms, losses);
    return (int)hipGetLastError();
}

extern "C" int nefes_train_loss_bwd(const NefesTrainLossDesc* desc, const float* g_color, const float* g_loss_f, const float* g_loss_fusion,
                                    const float* rgb_fine, const float* rgb_coarse, const float* rgb_target, const float* beta,
                                    const float* transient_sigmas, const float* feat_fine, const float* feat_coarse, const float* feat_fusion,
                                    const float* feat_target, float* g_rgb_fine, float* g_rgb_coarse, float* g_beta, float* g_sigma,
                                    float* g_feat_fine, float* g_feat_coarse, float* g_feat_fusion, void* stream) {
    const LossIn p{rgb_fine, rgb_coarse, rgb_target, beta, transient_sigmas, feat_fine, feat_coarse, feat_fusion, feat_target};
    if (const int rc = check_desc(desc, p)) return rc;
    const unsigned m = desc->present;
    // a gradient is written only for an input that is there
    if ((g_rgb_fine && !(m & NEFES_LOSS_HAS_RGB_FINE)) || (g_rgb_coarse && !(m & NEFES_LOSS_HAS_RGB_COARSE)) ||
        ((g_beta || g_sigma) && !(m & NEFES_LOSS_HAS_BETA)) || (g_feat_fine && !(m & NEFES_LOSS_HAS_FEAT_FINE)) ||
        (g_feat_coarse && !(m & NEFES_LOSS_HAS_FEAT_COARSE)) || (g_feat_fusion && !(m & NEFES_LOSS_HAS_FEAT_FUSION)))
        return NEFES_E_BADARG;
    if (!g_rgb_fine && !g_rgb_coarse && !g_beta && !g_sigma && !g_feat_fine && !g_feat_coarse && !g_feat_fusion) return NEFES_E_BADARG;
    const LossGrad o{g_rgb_fine, g_rgb_coarse, g_beta, g_sigma, g_feat_fine, g_feat_coarse, g_feat_fusion};
    hipLaunchKernelGGL(train_loss_bwd_kernel, dim3((unsigned)n_blocks_of(desc->N)), dim3(kThreads), 0, (hipStream_t)stream, *desc, p, g_color,
                       g_loss_f, g_loss_fusion, o);
    return (int)hipGetLastError();
}

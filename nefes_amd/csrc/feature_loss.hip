// The refinement loop's feature losses as kernels: in torch the loss on the up-sampled 128 x 220 x 300
// maps is ~35 elementwise passes over 34 MB each -- a fifth of an 80x60 refinement iteration.
//
//   cosine            feature_loss (script/dm/DFM_pose_refine.py:211-233, per_pixel=False): 1 - mean_c cos(a_c, b_c) over the
//                     pixels of [C, P] maps, torch.nn.CosineSimilarity(dim=1, eps=1e-6) semantics (each norm clamped at eps),
//                     float64 accumulation; backward d loss / d a in one pass.
//   upcos             the same ON the bicubically up-sampled, cropped map, without the up-sampled map;
//                     for a fixed target also through the Gram matrices of the up-sampling (nefes_upcos_prepare, nefes_upcos_gram_*).
//   pixcos, uppixcos  per_pixel=True: the cosine over the channels of each pixel, low resolution and up-sampled.
// Each form unmasked and MASKED (masked_feature_loss, :257-288), one kernel template and one launcher template per form and direction.
// One return code differs from the entry points' earlier, written-out form: nefes_cosine_loss_fwd / _bwd now refuse a grid beyond
// 2^31 - 1 blocks with NEFES_E_UNSUPPORTED, as their masked twins do (cosine_loss_fwd / cosine_loss_bwd below).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>

#include "../../include/nefes_hip.h"
#include "bicubic.h"

namespace {
// ---- cosine feature loss -------------------------------------------------------------------------------------------------
constexpr int kParts = 8;      // blocks per channel

// o[0..3) = the three sums over the workgroup's 256 threads, added in a fixed tree order; every thread of the workgroup calls
__device__ __forceinline__ void block_sum3(double dab, double daa, double dbb, double* __restrict__ o) {
    __shared__ double sh[3][256];
    sh[0][threadIdx.x] = dab; sh[1][threadIdx.x] = daa; sh[2][threadIdx.x] = dbb;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + s];
            sh[1][threadIdx.x] += sh[1][threadIdx.x + s];
            sh[2][threadIdx.x] += sh[2][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        o[0] = sh[0][0]; o[1] = sh[1][0]; o[2] = sh[2][0];
    }
}

// MASKED (the reference's masked_feature_loss, dm/DFM_pose_refine.py:257-288; `--semantic`): one uint8 per pixel and GROUP (image) of Cg
// channels, valid iff != 0.  A masked-out pixel is never READ (a select, not a product with 0: Inf / NaN there leave every result
// alone), the sums run over the valid pixels in the order the unmasked instance walks them -- an all-ones mask gives its bits -- and
// d loss / d a is exactly 0 there.  The unmasked instances ignore `mask` and `Cg`.
template <bool MASKED>
__global__ __launch_bounds__(256) void cosine_partial_kernel(int C, long P, const float* __restrict__ a, const float* __restrict__ b,
                                                             const uint8_t* __restrict__ mask, int Cg,
                                                             double* __restrict__ part) {      // part [C][kParts][3]
    const int c = blockIdx.x / kParts, q = blockIdx.x % kParts;
    const long per = (P + kParts - 1) / kParts, lo = q * per, hi = lo + per < P ? lo + per : P;
    const float* pa = a + (long)c * P;
    const float* pb = b + (long)c * P;
    const uint8_t* pm = MASKED ? mask + (long)(c / Cg) * P : nullptr;
    double dab = 0, daa = 0, dbb = 0;
    for (long i = lo + threadIdx.x; i < hi; i += 256) {
        if (MASKED && !pm[i]) continue;
        const double x = pa[i], y = pb[i];
        dab += x * y;
        daa += x * x;
        dbb += y * y;
    }
    block_sum3(dab, daa, dbb, part + ((long)c * kParts + q) * 3);
}

// stats [C][4] = (dot, |a|, |b|, cos) of the C = G * Cg channels; loss = sum_g (1 - mean of the group's Cg cosines).  The unmasked
// forms launch it with one group of all channels: 0 + (1 - s / C) is the double 1 - s / C, their 1 - mean cos.  A
// channel without a valid pixel has all three sums 0: cos = 0 (both norms clamped at eps), as the reference's expression gives.
__global__ __launch_bounds__(256) void cosine_final_groups_kernel(int G, int Cg, double eps, const double* __restrict__ part,
                                                                  double* __restrict__ stats, float* __restrict__ loss) {
    __shared__ double sh[256];
    double total = 0;
    for (int g = 0; g < G; ++g) {
        double acc = 0;
        for (int cc = threadIdx.x; cc < Cg; cc += 256) {
            const long c = (long)g * Cg + cc;
            double dab = 0, daa = 0, dbb = 0;
            for (int q = 0; q < kParts; ++q) {
                const double* o = part + (c * kParts + q) * 3;
                dab += o[0]; daa += o[1]; dbb += o[2];
            }
            const double na = sqrt(daa), nb = sqrt(dbb);
            const double cs = dab / ((na > eps ? na : eps) * (nb > eps ? nb : eps));
            stats[c * 4 + 0] = dab; stats[c * 4 + 1] = na; stats[c * 4 + 2] = nb; stats[c * 4 + 3] = cs;
            acc += cs;
        }
        sh[threadIdx.x] = acc;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
            __syncthreads();
        }
        total += 1.0 - sh[0] / Cg;
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)total;
}

// g_a[c][p] = -g_loss / C * d cos_c / d a[c][p]   (MASKED: C planes in groups of Cg, the mean over the group's Cg; 0 where masked out)
template <bool MASKED>
__global__ __launch_bounds__(256) void cosine_bwd_kernel(int C, long P, double eps, const float* __restrict__ a, const float* __restrict__ b,
                                                         const uint8_t* __restrict__ mask, int Cg, const double* __restrict__ stats,
                                                         const float* __restrict__ g_loss, float* __restrict__ g_a) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)C * P) return;
    const int c = (int)(idx / P);
    if (MASKED) {
        if (!mask[(long)(c / Cg) * P + idx % P]) {
            g_a[idx] = 0.f;
            return;
        }
        C = Cg;
    }
    const double dab = stats[c * 4 + 0], na = stats[c * 4 + 1], nb = stats[c * 4 + 2];
    const double nbc = nb > eps ? nb : eps;
    const double k = -(double)g_loss[0] / C;
    double v;
    if (na > eps) v = (double)b[idx] / (na * nbc) - dab * (double)a[idx] / (na * na * na * nbc);
    else v = (double)b[idx] / (eps * nbc);                                   // the clamped norm is a constant there
    g_a[idx] = (float)(k * v);
}

// ---- feature loss ON the up-sampled image, without the up-sampled image (DFM_APR_refine.py:114-131): the loop up-samples the
// fused [C,h,w] features bicubically to (H, W), crops 10 px and takes the cosine loss against the query image's features.  As
// separate kernels that is 34 MB written and read again each way (up-sampled features; their gradient) around 2.4 MB of data.
// Here every up-sampled value is interpolated where it is consumed -- same expression, same order as bicubic_up_fwd_kernel -- from
// the channel's low-resolution plane (forward: staged in LDS) or its four source rows (backward), and the target is the only
// large tensor that moves.
struct UpCosArgs {
    int C, h, w, OH, OW, o0, CH, CW;
    float sy, sx;
    const float* x;        // [C, h, w]
    const float* target;   // [C, CH, CW]
};

// One up-sampled value from the four source rows rr of its output row (rows ty.base - 1 .. + 2, clamped to the plane, in LDS or in
// memory) and the clamped source columns xs of tx: x first, then y -- the expression and order of bicubic_up_fwd_kernel
// (upsample.hip), bit for bit.
__device__ __forceinline__ float up_value(const float* const (&rr)[4], const int (&xs)[4], const nefes_bicubic::Taps& tx,
                                          const nefes_bicubic::Taps& ty) {
    float rows[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) rows[i] = rr[i][xs[0]] * tx.w[0] + rr[i][xs[1]] * tx.w[1] + rr[i][xs[2]] * tx.w[2] + rr[i][xs[3]] * tx.w[3];
    return rows[0] * ty.w[0] + rows[1] * ty.w[1] + rows[2] * ty.w[2] + rows[3] * ty.w[3];
}

template <bool MASKED>      // mask [C / Cg][CH][CW]: see cosine_partial_kernel
__global__ __launch_bounds__(256) void upcos_partial_kernel(UpCosArgs a, const uint8_t* __restrict__ mask, int Cg,
                                                            double* __restrict__ part) {      // part [C][kParts][3]
    using namespace nefes_bicubic;
    extern __shared__ float plane[];
    const int c = blockIdx.x / kParts, q = blockIdx.x % kParts;
    const float* src = a.x + (long)c * a.h * a.w;
    for (int i = threadIdx.x; i < a.h * a.w; i += 256) plane[i] = src[i];
    __syncthreads();
    // part q = a band of up-sampled rows; a thread owns columns (its x taps and clamped source columns are computed once)
    const int per = (a.CH + kParts - 1) / kParts, r_lo = q * per, r_hi = r_lo + per < a.CH ? r_lo + per : a.CH;
    double dab = 0, daa = 0, dbb = 0;
    for (int j = threadIdx.x; j < a.CW; j += 256) {
        const Taps tx = taps_of(a.sx, j + a.o0);
        int xs[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) xs[m] = clampi(tx.base - 1 + m, a.w);
        const float* pb = a.target + (long)c * a.CH * a.CW + j;
        const uint8_t* pm = MASKED ? mask + (long)(c / Cg) * a.CH * a.CW + j : nullptr;
        for (int r = r_lo; r < r_hi; ++r) {
            if (MASKED && !pm[(long)r * a.CW]) continue;
            const Taps ty = taps_of(a.sy, r + a.o0);
            const float* rr[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) rr[i] = plane + clampi(ty.base - 1 + i, a.h) * a.w;
            const double xv = up_value(rr, xs, tx, ty);
            const double yv = pb[(long)r * a.CW];
            dab += xv * yv;
            daa += xv * xv;
            dbb += yv * yv;
        }
    }
    block_sum3(dab, daa, dbb, part + ((long)c * kParts + q) * 3);
}

__global__ __launch_bounds__(256) void upcos_gather_rows_kernel(long outer, int n_in, int n_win, long inner, nefes_bicubic::GatherTable gy,
                                                                const float* __restrict__ src, float* __restrict__ dst) {
    using namespace nefes_bicubic;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= outer * n_in * inner) return;
    const long q = idx % inner;
    const int y = (int)((idx / inner) % n_in);
    const long p = idx / (inner * n_in);
    dst[idx] = gather_axis_table(gy, y, src + p * n_win * inner + q, inner);
}

// ---- per-pixel feature loss (`--per_pixel`, dm/options.py:73; DFM_pose_refine.py:227-233 with dim = channels) ----------------------
// For maps a, b [G, C, P] (G groups = images, each with its own mean):
//     cos_p = a_p.b_p / (max(|a_p|, eps) max(|b_p|, eps)),   loss = sum over groups of (1 - mean_p cos_p)
//     d loss / d a[c,p] = -(g / P) (b[c,p] / (na' nb') - [|a_p| > eps] (a_p.b_p) a[c,p] / (|a_p|^3 nb'))     (a clamped norm is a constant)
// The normalisation is per pixel, so all C values of a pixel are needed at once: there is no Gram form and NO PREPARED-TARGET FORM of
// this loss (<up, t> = <X, Uy^T t Ux> needs ONE factor per channel in front of the sum over pixels; here every pixel has its own).
// Forward: a workgroup owns kPixCols consecutive pixels (loads coalesced along P) and splits the channels into kPixSlices
// contiguous slices, one wave each -- 66 000 pixels are only ~1 000 waves, and a wave that walks all 128 channels alone waits
// out 128 memory latencies one after the other (measured at the loop's shape: 257 us; this form 106 us, profiles/per_pixel_loss).  A
// thread walks its slice's c in ascending order with (a.b, |a|^2, |b|^2) in float64; slice 0 adds the four slices in order, leaves
// stats [G][3][P] = (a.b, |a|, |b|) planes for the backward, and the workgroup's float64 sum of cos_p goes to part [G][nb]; a
// finalising launch adds the partials in a fixed order: mean [G] (float64) and the float32 loss.  Backward: one launch from the
// pixel's three numbers.  No atomics, fixed summation order: a step repeats bit for bit and can be captured.
// scratch (doubles) = mean [G] | stats [G][3][P] | part [G][nb]
constexpr int kPixCols = 64, kPixSlices = 4, kPixBlock = kPixCols * kPixSlices;      // (8 slices: the same time; 16: slower)

// sh[0] = sum of sh[0 .. n) in a fixed tree order; n <= 512, every thread of the block calls
__device__ __forceinline__ void pix_block_sum(double* sh, int n) {
    __syncthreads();
    for (int s = 256; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s && (int)threadIdx.x + s < n) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
}

__device__ __forceinline__ double pix_cos(double dab, double na, double nb, double eps) {
    return dab / ((na > eps ? na : eps) * (nb > eps ? nb : eps));
}

// the slices' sums of one pixel added in slice order by slice 0's thread -> stats planes, cos_p; then the workgroup's sum of cos_p
// (fixed tree) in sh[0][0][0].  Every thread of the workgroup calls.
__device__ __forceinline__ void pix_finish(double (*sh)[kPixSlices][kPixCols], double dab, double daa, double dbb, bool live, double eps,
                                           double* st, long P) {
    const int col = threadIdx.x % kPixCols, sl = threadIdx.x / kPixCols;
    sh[0][sl][col] = dab; sh[1][sl][col] = daa; sh[2][sl][col] = dbb;
    __syncthreads();
    double cs = 0;
    if (sl == 0 && live) {
        double t[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            t[k] = sh[k][0][col];
#pragma unroll
            for (int q = 1; q < kPixSlices; ++q) t[k] += sh[k][q][col];
        }
        const double na = sqrt(t[1]), nb = sqrt(t[2]);
        st[0] = t[0]; st[P] = na; st[2 * P] = nb;
        cs = pix_cos(t[0], na, nb, eps);
    }
    __syncthreads();
    double* red = &sh[0][0][0];
    if (sl == 0) red[col] = cs;
    pix_block_sum(red, kPixCols);
}

// MASKED (mask [G][P] uint8, see cosine_partial_kernel): a masked-out pixel is not read, leaves no stats (the backward does not read them
// either) and adds nothing to the workgroup's sum; the workgroup's count of valid pixels goes to cnt [G][nb] beside part, and the mean
// is over the group's valid pixels (none: 0 / 0 = NaN, what the reference's mean of an empty tensor gives).
template <bool MASKED>
__global__ __launch_bounds__(kPixBlock) void pixcos_fwd_kernel(int C, long P, double eps, const float* __restrict__ a, const float* __restrict__ b,
                                                               const uint8_t* __restrict__ mask, double* __restrict__ stats,
                                                               double* __restrict__ part, double* __restrict__ cnt) {
    __shared__ double sh[3][kPixSlices][kPixCols];
    const int g = blockIdx.y, sl = threadIdx.x / kPixCols;
    const long p = (long)blockIdx.x * kPixCols + threadIdx.x % kPixCols;
    const int per = (C + kPixSlices - 1) / kPixSlices, c0 = sl * per, c1 = c0 + per < C ? c0 + per : C;
    double dab = 0, daa = 0, dbb = 0;
    bool live = p < P;
    if (MASKED) {
        live = live && mask[(long)g * P + p] != 0;
        const int n = __syncthreads_count(live && sl == 0);
        if (threadIdx.x == 0) cnt[(long)g * gridDim.x + blockIdx.x] = (double)n;
    }
    if (live) {
        const float* pa = a + (long)g * C * P + p;
        const float* pb = b + (long)g * C * P + p;
#pragma unroll 4
        for (int c = c0; c < c1; ++c) {
            const double x = pa[(long)c * P], y = pb[(long)c * P];
            dab += x * y;
            daa += x * x;
            dbb += y * y;
        }
    }
    pix_finish(sh, dab, daa, dbb, live, eps, stats + (long)g * 3 * P + p, P);
    if (threadIdx.x == 0) part[(long)g * gridDim.x + blockIdx.x] = sh[0][0][0];
}

// mean[g] = (sum of the group's nb partials) / P;  loss = sum_g (1 - mean[g])
// MASKED: P is the group's count of valid pixels, the sum of its nb entries of cnt (whole numbers: exact in any order), kept in
// count[g] for the backward.
template <bool MASKED>
__global__ __launch_bounds__(256) void pixcos_final_kernel(int G, int nb, double P, const double* __restrict__ part, const double* __restrict__ cnt,
                                                           double* __restrict__ mean, double* __restrict__ count, float* __restrict__ loss) {
    __shared__ double sh[256];
    double total = 0;
    for (int g = 0; g < G; ++g) {
        if (MASKED) {
            double n = 0;
            for (int i = threadIdx.x; i < nb; i += 256) n += cnt[(long)g * nb + i];
            sh[threadIdx.x] = n;
            pix_block_sum(sh, 256);
            P = sh[0];
            __syncthreads();
            if (threadIdx.x == 0) count[g] = P;
        }
        double acc = 0;
        for (int i = threadIdx.x; i < nb; i += 256) acc += part[(long)g * nb + i];
        sh[threadIdx.x] = acc;
        pix_block_sum(sh, 256);
        const double m = sh[0] / P;
        __syncthreads();
        if (threadIdx.x == 0) mean[g] = m;
        total += 1.0 - m;
    }
    if (threadIdx.x == 0) *loss = (float)total;
}

// the two factors of the gradient at one pixel: g_a = k1 b - k2 a
struct PixK {
    double k1, k2;
};
__device__ __forceinline__ PixK pix_factors(double k, double dab, double na, double nb, double eps) {
    const double nbc = nb > eps ? nb : eps;
    PixK r;
    r.k1 = na > eps ? k / (na * nbc) : k / (eps * nbc);
    r.k2 = na > eps ? k * dab / (na * na * na * nbc) : 0.0;
    return r;
}

template <bool MASKED>      // count [G]: the groups' valid pixels (pixcos_final_kernel)
__global__ __launch_bounds__(256) void pixcos_bwd_kernel(long n, int C, long P, double eps, const float* __restrict__ a, const float* __restrict__ b,
                                                         const uint8_t* __restrict__ mask, const double* __restrict__ count,
                                                         const double* __restrict__ stats, const float* __restrict__ g_loss,
                                                         float* __restrict__ g_a) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const long p = idx % P, g = idx / (P * C);
    if (MASKED && !mask[g * P + p]) {
        g_a[idx] = 0.f;
        return;
    }
    const double* st = stats + g * 3 * P + p;
    const PixK f = pix_factors(-(double)g_loss[0] / (MASKED ? count[g] : (double)P), st[0], st[P], st[2 * P], eps);
    g_a[idx] = (float)(f.k1 * (double)b[idx] - f.k2 * (double)a[idx]);
}

// The same loss ON the up-sampled, cropped map without the up-sampled map: the per-pixel twin of upcos_partial_kernel /
// upcos_bwd_rows_kernel.  x [G*C, h, w], target [G*C, CH, CW] (UpCosArgs with C = G*C planes), Cg channels per group.
// Forward: one workgroup per (group, window row r, segment of kPixCols columns), the channels in kPixSlices slices as above.  A thread
// computes its x taps and clamped source columns once and interpolates every channel's value with up_value's expression and order
// (x first, then y: the value bicubic_up_fwd_kernel would have written, bit for bit) from the channel's four source rows in x (2.4 MB
// at the loop's shape: L2) -- the target row is the only HBM read.  part [G][CH][segments].
template <bool MASKED>      // mask [G][CH][CW], cnt beside part: see pixcos_fwd_kernel
__global__ __launch_bounds__(kPixBlock) void uppixcos_fwd_kernel(UpCosArgs a, int Cg, double eps, const uint8_t* __restrict__ mask,
                                                                 double* __restrict__ stats, double* __restrict__ part,
                                                                 double* __restrict__ cnt) {
    using namespace nefes_bicubic;
    __shared__ double sh[3][kPixSlices][kPixCols];
    const int r = blockIdx.x, seg = blockIdx.y, g = blockIdx.z, sl = threadIdx.x / kPixCols;
    const int j = seg * kPixCols + threadIdx.x % kPixCols;
    const long P = (long)a.CH * a.CW, plane = (long)a.h * a.w;
    const int per = (Cg + kPixSlices - 1) / kPixSlices, c0 = sl * per, c1 = c0 + per < Cg ? c0 + per : Cg;
    double dab = 0, daa = 0, dbb = 0;
    bool live = j < a.CW;
    if (MASKED) {
        live = live && mask[(long)g * P + (long)r * a.CW + j] != 0;
        const int n = __syncthreads_count(live && sl == 0);
        if (threadIdx.x == 0) cnt[((long)g * a.CH + r) * gridDim.y + seg] = (double)n;
    }
    if (live) {
        const Taps ty = taps_of(a.sy, r + a.o0), tx = taps_of(a.sx, j + a.o0);
        long ro[4];
        int xs[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ro[i] = (long)clampi(ty.base - 1 + i, a.h) * a.w;
            xs[i] = clampi(tx.base - 1 + i, a.w);
        }
        const float* src = a.x + (long)g * Cg * plane;
        const float* tg = a.target + (long)g * Cg * P + (long)r * a.CW + j;
#pragma unroll 4
        for (int c = c0; c < c1; ++c) {
            // (up_value's expression written out: through the helper this kernel came out 2 VGPRs larger and 5 us slower at the loop's
            // shape, profiles/feature_loss_one_body/README.md)
            const float* pl = src + c * plane;
            float rows[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float* rr = pl + ro[i];
                rows[i] = rr[xs[0]] * tx.w[0] + rr[xs[1]] * tx.w[1] + rr[xs[2]] * tx.w[2] + rr[xs[3]] * tx.w[3];
            }
            const double xv = rows[0] * ty.w[0] + rows[1] * ty.w[1] + rows[2] * ty.w[2] + rows[3] * ty.w[3];
            const double yv = tg[c * P];
            dab += xv * yv;
            daa += xv * xv;
            dbb += yv * yv;
        }
    }
    pix_finish(sh, dab, daa, dbb, live, eps, stats + (long)g * 3 * P + (long)r * a.CW + j, P);
    if (threadIdx.x == 0) part[((long)g * a.CH + r) * gridDim.y + seg] = sh[0][0][0];
}

// Backward of both up-sampled losses.  One workgroup per (plane c = group * Cg + channel, up-sampled row of the window): the row's
// gradient d loss / d up[c][oy][:] = k1 target - k2 up (pix_factors; d cos / d a = b / (|a||b|) - (a.b) a / (|a|^3 |b|), a clamped
// norm is a constant) is formed in LDS from the interpolated values and the target row, and gathered along x onto the w source
// columns: tmp[c][oy - o0][0..w).  upcos_gather_rows_kernel finishes along y.
//   PER_PIXEL = false   stats [C][4] of cosine_final_groups_kernel: the two factors are the channel's, formed once; the mean is
//                       over the C channels (MASKED: the group's Cg)
//   PER_PIXEL = true    stats [G][3][P] of uppixcos_fwd_kernel: the two factors are the pixel's; the mean is over the P pixels
//                       (MASKED: count [G], the groups' valid pixels)
// MASKED: a masked-out up-sampled pixel contributes nothing to the gather: its gs is 0, its stats and target are not read.
template <bool MASKED, bool PER_PIXEL>
__global__ __launch_bounds__(128) void upcos_bwd_rows_kernel(UpCosArgs a, int Cg, double eps, const double* __restrict__ stats,
                                                             const float* __restrict__ g_loss, nefes_bicubic::GatherTable gx,
                                                             const uint8_t* __restrict__ mask, const double* __restrict__ count,
                                                             float* __restrict__ tmp) {
    using namespace nefes_bicubic;
    extern __shared__ float lds[];
    float* rows = lds;                 // [4][w] the four source rows of this up-sampled row
    float* gs = lds + 4 * a.w;         // [CW]
    const int c = blockIdx.x / a.CH, r = blockIdx.x % a.CH, oy = r + a.o0;
    const Taps ty = taps_of(a.sy, oy);
    const float* src = a.x + (long)c * a.h * a.w;
    for (int i = threadIdx.x; i < 4 * a.w; i += 128) rows[i] = src[(long)clampi(ty.base - 1 + i / a.w, a.h) * a.w + i % a.w];
    __syncthreads();
    const long P = (long)a.CH * a.CW;
    const double k = PER_PIXEL ? -(double)g_loss[0] / (MASKED ? count[c / Cg] : (double)P) : -(double)g_loss[0] / (MASKED ? Cg : a.C);
    const double* st = PER_PIXEL ? stats + (long)(c / Cg) * 3 * P + (long)r * a.CW : stats + c * 4;
    PixK f;
    if (!PER_PIXEL) f = pix_factors(k, st[0], st[1], st[2], eps);
    const float* pb = a.target + ((long)c * a.CH + r) * a.CW;
    const uint8_t* pm = MASKED ? mask + ((long)(c / Cg) * a.CH + r) * a.CW : nullptr;
    const float* const rr[4] = {rows, rows + a.w, rows + 2 * a.w, rows + 3 * a.w};
    for (int j = threadIdx.x; j < a.CW; j += 128) {
        if (MASKED && !pm[j]) {
            gs[j] = 0.f;
            continue;
        }
        const Taps tx = taps_of(a.sx, j + a.o0);
        int xs[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) xs[m] = clampi(tx.base - 1 + m, a.w);
        const double av = up_value(rr, xs, tx, ty);
        if (PER_PIXEL) f = pix_factors(k, st[j], st[P + j], st[2 * P + j], eps);
        gs[j] = (float)(f.k1 * (double)pb[j] - f.k2 * av);
    }
    __syncthreads();
    float* out = tmp + ((long)c * a.CH + r) * a.w;
    for (int xi = threadIdx.x; xi < a.w; xi += 128) out[xi] = gather_axis_table(gx, xi, gs, 1);
}

// ---- the same loss for a FIXED target, through the Gram matrices of the up-sampling (round 5) ---------------------------------
// Per channel the up-sampled, cropped image is  up = Uy X Ux^T  (Uy [CH, h], Ux [CW, w]: the bicubic taps of the window's rows and
// columns, clamped at the borders).  The refinement loop holds the target for all iterations of an image (DFM_APR_refine.py:
// 100-131: the query image's features are extracted once, the pose is optimised opt_iter times against them), so
//     <up, target> = <X, Uy^T target Ux> = <X, Tt>            Tt [C, h, w]: once per image (upcos_prep_* below)
//     |up|^2       = <X, Gy X Gx>                             Gy = Uy^T Uy [h, h], Gx = Ux^T Ux [w, w]: once per geometry, banded
//     |target|^2                                              once per image
//     d loss / d X = -g / C (k1 Tt - k2 Gy X Gx)              (k1, k2 of upcos_bwd_rows_kernel)
// and an iteration touches the 2.4 MB of X, Tt and P = Gy X Gx instead of the 34 MB target twice: 30 + 47 + 14 us -> three small
// launches.  Everything in float64 from the float32 tap weights (those of taps_of: what ATen's kernel uses), so the result is the
// float64 value of the loss on the float32 taps -- the one-pass kernels above round every up-sampled value to float32 first.
__global__ void bicubic_gram_kernel(int n_in, int o0, int n_win, float scale, double* __restrict__ G) {
    using namespace nefes_bicubic;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_in * n_in) return;
    const int ya = idx / n_in, yb = idx % n_in;
    double acc = 0;
    for (int o = o0; o < o0 + n_win; ++o) {
        const Taps t = taps_of(scale, o);
        double wa = 0, wb = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int y = clampi(t.base - 1 + k, n_in);
            if (y == ya) wa += (double)t.w[k];
            if (y == yb) wb += (double)t.w[k];
        }
        acc += wa * wb;
    }
    G[idx] = acc;
}

// tmp[c][r][x] = sum_ox Wx(ox -> x) target[c][r][ox]
__global__ __launch_bounds__(256) void upcos_prep_rows_kernel(long n, int CW, int w, nefes_bicubic::GatherTable gx,
                                                              const float* __restrict__ target, double* __restrict__ tmp) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int x = (int)(idx % w);
    const long row = idx / w;                                    // c * CH + r
    const int f = gx.first[x], cnt = gx.count[x];
    const float* wt = gx.wt + (long)x * gx.T;
    const float* s = target + row * CW + f;
    double acc = 0;
    for (int i = 0; i < cnt; ++i) acc += (double)wt[i] * (double)s[i];
    tmp[idx] = acc;
}

// tt[c][y][x] = sum_r Wy(r -> y) tmp[c][r][x]
__global__ __launch_bounds__(256) void upcos_prep_cols_kernel(long n, int h, int CH, int w, nefes_bicubic::GatherTable gy,
                                                              const double* __restrict__ tmp, double* __restrict__ tt) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int x = (int)(idx % w), y = (int)((idx / w) % h);
    const long c = idx / ((long)w * h);
    const int f = gy.first[y], cnt = gy.count[y];
    const float* wt = gy.wt + (long)y * gy.T;
    const double* s = tmp + (c * CH + f) * w + x;
    double acc = 0;
    for (int i = 0; i < cnt; ++i) acc += (double)wt[i] * s[(long)i * w];
    tt[idx] = acc;
}

// dbb[c] = |target[c]|^2
__global__ __launch_bounds__(256) void upcos_prep_norm_kernel(long P, const float* __restrict__ target, double* __restrict__ dbb) {
    const float* pb = target + (long)blockIdx.x * P;
    double acc = 0;
    for (long i = threadIdx.x; i < P; i += 256) {
        const double v = pb[i];
        acc += v * v;
    }
    __shared__ double sh[256];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) dbb[blockIdx.x] = sh[0];
}

// One workgroup per (channel, band of source rows): Q = X Gx on the band's rows and R more on either side (LDS), P = Gy Q on the
// band, partial <X, Tt> and <X, P> in the layout cosine_final_groups_kernel sums (|target|^2 rides in part 0).  Fixed order: deterministic.
__global__ __launch_bounds__(256) void upcos_gram_fwd_kernel(int h, int w, int R, const float* __restrict__ x, const double* __restrict__ tt,
                                                             const double* __restrict__ dbb, const double* __restrict__ Gx,
                                                             const double* __restrict__ Gy, double* __restrict__ part,
                                                             double* __restrict__ pmat) {
    extern __shared__ double lds_d[];
    const int c = blockIdx.x / kParts, q = blockIdx.x % kParts;
    const int per = (h + kParts - 1) / kParts, r_lo = q * per < h ? q * per : h, r_hi = r_lo + per < h ? r_lo + per : h;
    const int y_lo = r_lo - R > 0 ? r_lo - R : 0, y_hi = r_hi + R < h ? r_hi + R : h, nrow = r_hi > r_lo ? y_hi - y_lo : 0;
    const int B = 2 * R + 1;
    double* Q = lds_d;                                  // [nrow][w]
    double* gxb = Q + (per + 2 * R) * w;                // [w][B]: column xx of Gx, rows xx - R .. xx + R (zero outside the matrix)
    double* gyb = gxb + w * B;                          // [per][B]: row y of Gy, columns y - R .. y + R
    float* X = (float*)(gyb + per * B);                 // [nrow][w]
    const float* src = x + ((long)c * h + y_lo) * w;
    // everything that comes from memory in ONE round: the rows of X, the band of Gx, this part's rows of Gy's band
    for (int i = threadIdx.x; i < nrow * w; i += 256) X[i] = src[i];
    for (int i = threadIdx.x; i < w * B; i += 256) {
        const int xx = i / B, a = xx - R + i % B;
        gxb[i] = a >= 0 && a < w ? Gx[(long)a * w + xx] : 0.0;
    }
    for (int i = threadIdx.x; i < (r_hi - r_lo) * B; i += 256) {
        const int y = r_lo + i / B, b = y - R + i % B;
        gyb[i] = b >= 0 && b < h ? Gy[(long)y * h + b] : 0.0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nrow * w; i += 256) {
        const int xx = i % w, yy = i / w;
        const int a0 = xx - R > 0 ? xx - R : 0, a1 = xx + R < w - 1 ? xx + R : w - 1;
        double acc = 0;
        for (int a = a0; a <= a1; ++a) acc += (double)X[yy * w + a] * gxb[xx * B + a - xx + R];
        Q[i] = acc;
    }
    __syncthreads();
    double dab = 0, daa = 0;
    for (int i = threadIdx.x; i < (r_hi - r_lo) * w; i += 256) {
        const int xx = i % w, y = r_lo + i / w;
        const int b0 = y - R > 0 ? y - R : 0, b1 = y + R < h - 1 ? y + R : h - 1;
        const long o = ((long)c * h + y) * w + xx;
        const double tv = tt[o];
        double p = 0;
        for (int b = b0; b <= b1; ++b) p += gyb[(y - r_lo) * B + b - y + R] * Q[(b - y_lo) * w + xx];
        const double xv = X[(y - y_lo) * w + xx];
        dab += xv * tv;
        daa += xv * p;
        pmat[o] = p;
    }
    __shared__ double sh[2][256];
    sh[0][threadIdx.x] = dab; sh[1][threadIdx.x] = daa;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            sh[0][threadIdx.x] += sh[0][threadIdx.x + s];
            sh[1][threadIdx.x] += sh[1][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double* o = part + ((long)c * kParts + q) * 3;
        o[0] = sh[0][0]; o[1] = sh[1][0]; o[2] = q == 0 ? dbb[c] : 0.0;
    }
}

// g_x = -g / C (k1 Tt - k2 P): the factors of upcos_bwd_rows_kernel
__global__ __launch_bounds__(256) void upcos_gram_bwd_kernel(int C, long P, double eps, const double* __restrict__ tt, const double* __restrict__ pmat,
                                                             const double* __restrict__ stats, const float* __restrict__ g_loss,
                                                             float* __restrict__ g_x) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)C * P) return;
    const int c = (int)(idx / P);
    const double dab = stats[c * 4 + 0], na = stats[c * 4 + 1], nb = stats[c * 4 + 2];
    const double nbc = nb > eps ? nb : eps;
    const double k = -(double)g_loss[0] / C;
    const double k1 = na > eps ? k / (na * nbc) : k / (eps * nbc), k2 = na > eps ? k * dab / (na * na * na * nbc) : 0.0;
    g_x[idx] = (float)(k1 * tt[idx] - k2 * pmat[idx]);
}

}  // namespace


// The channel-wise losses, unmasked (G = 1, Cg = C, mask = null) and masked (C = G * Cg planes): one body per entry-point pair
template <bool MASKED>
static int upcos_loss_fwd(int G, int Cg, int h, int w, int OH, int OW, int crop, const float* x, const float* target, const uint8_t* mask,
                          double* scratch, float* loss, void* stream) {
    const int CH = OH - 2 * crop, CW = OW - 2 * crop;
    if (G <= 0 || Cg <= 0 || h <= 0 || w <= 0 || crop < 0 || CH <= 0 || CW <= 0 || !x || !target || !scratch || !loss || (MASKED && !mask))
        return NEFES_E_BADARG;
    if ((size_t)h * w * 4 > 96 * 1024) return NEFES_E_UNSUPPORTED;           // the channel's plane is staged in LDS
    if ((long)G * Cg * kParts > 0x7fffffffl) return NEFES_E_UNSUPPORTED;
    const int C = G * Cg;
    UpCosArgs a{C, h, w, OH, OW, crop, CH, CW, (float)h / OH, (float)w / OW, x, target};
    double* part = scratch + (size_t)C * 4;
    const size_t lds = (size_t)h * w * 4;
    hipError_t e = hipFuncSetAttribute((const void*)upcos_partial_kernel<MASKED>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(upcos_partial_kernel<MASKED>, dim3(C * kParts), dim3(256), lds, (hipStream_t)stream, a, mask, Cg, part);
    hipLaunchKernelGGL(cosine_final_groups_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, G, Cg, 1e-6, (const double*)part, scratch, loss);
    return (int)hipGetLastError();
}
extern "C" int nefes_upcos_loss_fwd(int C, int h, int w, int OH, int OW, int crop, const float* x, const float* target, double* scratch,
                                    float* loss, void* stream) {
    return upcos_loss_fwd<false>(1, C, h, w, OH, OW, crop, x, target, nullptr, scratch, loss, stream);
}
extern "C" int nefes_upcos_loss_masked_fwd(int G, int Cg, int h, int w, int OH, int OW, int crop, const float* x, const float* target,
                                           const uint8_t* mask, double* scratch, float* loss, void* stream) {
    return upcos_loss_fwd<true>(G, Cg, h, w, OH, OW, crop, x, target, mask, scratch, loss, stream);
}

template <bool MASKED>
static int upcos_loss_bwd(int G, int Cg, int h, int w, int OH, int OW, int crop, const float* x, const float* target, const uint8_t* mask,
                          const double* scratch, const float* g_loss, const int* tx_first, const int* tx_count, const float* tx_wt,
                          const int* ty_first, const int* ty_count, const float* ty_wt, int T, float* tmp, float* g_x, void* stream) {
    const int CH = OH - 2 * crop, CW = OW - 2 * crop;
    if (G <= 0 || Cg <= 0 || h <= 0 || w <= 0 || crop < 0 || CH <= 0 || CW <= 0 || !x || !target || !scratch || !g_loss || !tmp || !g_x ||
        (MASKED && !mask))
        return NEFES_E_BADARG;
    if (!tx_first || !tx_count || !tx_wt || !ty_first || !ty_count || !ty_wt || T <= 0) return NEFES_E_BADARG;
    if ((long)G * Cg * CH > 0x7fffffffl) return NEFES_E_UNSUPPORTED;
    const int C = G * Cg;
    const nefes_bicubic::GatherTable gx{tx_first, tx_count, tx_wt, T}, gy{ty_first, ty_count, ty_wt, T};
    UpCosArgs a{C, h, w, OH, OW, crop, CH, CW, (float)h / OH, (float)w / OW, x, target};
    const size_t lds = (size_t)(4 * w + CW) * 4;
    if (lds > 96 * 1024) return NEFES_E_UNSUPPORTED;
    hipError_t e = hipFuncSetAttribute((const void*)upcos_bwd_rows_kernel<MASKED, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((upcos_bwd_rows_kernel<MASKED, false>), dim3((unsigned)((long)C * CH)), dim3(128), lds, (hipStream_t)stream, a, Cg, 1e-6,
                       scratch, g_loss, gx, mask, (const double*)nullptr, tmp);
    const long n = (long)C * h * w;                    // g_x[c][y][x] = sum over the window's rows oy of Wy(oy -> y) tmp[c][oy - o0][x]
    hipLaunchKernelGGL(upcos_gather_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (long)C, h, CH, (long)w, gy,
                       (const float*)tmp, g_x);
    return (int)hipGetLastError();
}
extern "C" int nefes_upcos_loss_bwd(int C, int h, int w, int OH, int OW, int crop, const float* x, const float* target, const double* scratch,
                                    const float* g_loss, const int* tx_first, const int* tx_count, const float* tx_wt, const int* ty_first,
                                    const int* ty_count, const float* ty_wt, int T, float* tmp, float* g_x, void* stream) {
    return upcos_loss_bwd<false>(1, C, h, w, OH, OW, crop, x, target, nullptr, scratch, g_loss, tx_first, tx_count, tx_wt, ty_first, ty_count,
                                 ty_wt, T, tmp, g_x, stream);
}
extern "C" int nefes_upcos_loss_masked_bwd(int G, int Cg, int h, int w, int OH, int OW, int crop, const float* x, const float* target,
                                           const uint8_t* mask, const double* scratch, const float* g_loss, const int* tx_first,
                                           const int* tx_count, const float* tx_wt, const int* ty_first, const int* ty_count, const float* ty_wt,
                                           int T, float* tmp, float* g_x, void* stream) {
    return upcos_loss_bwd<true>(G, Cg, h, w, OH, OW, crop, x, target, mask, scratch, g_loss, tx_first, tx_count, tx_wt, ty_first, ty_count, ty_wt,
                                T, tmp, g_x, stream);
}

// scratch of the per-pixel loss (doubles): mean [G] | stats [G][3][P] | one partial per forward workgroup
extern "C" size_t nefes_pixcos_scratch_doubles(int G, int64_t P) {
    return G > 0 && P > 0 ? (size_t)G * (1 + 3 * (size_t)P + (size_t)((P + kPixCols - 1) / kPixCols)) : 0;
}
extern "C" size_t nefes_uppixcos_scratch_doubles(int G, int OH, int OW, int crop) {
    const int CH = OH - 2 * crop, CW = OW - 2 * crop;
    return G > 0 && crop >= 0 && CH > 0 && CW > 0 ? (size_t)G * (1 + 3 * (size_t)CH * CW + (size_t)CH * ((CW + kPixCols - 1) / kPixCols)) : 0;
}
// masked: the unmasked layout | the workgroups' counts of valid pixels (one per partial) | count [G]
extern "C" size_t nefes_pixcos_masked_scratch_doubles(int G, int64_t P) {
    return G > 0 && P > 0 ? nefes_pixcos_scratch_doubles(G, P) + (size_t)G * (1 + (size_t)((P + kPixCols - 1) / kPixCols)) : 0;
}
extern "C" size_t nefes_uppixcos_masked_scratch_doubles(int G, int OH, int OW, int crop) {
    const int CH = OH - 2 * crop, CW = OW - 2 * crop;
    return G > 0 && crop >= 0 && CH > 0 && CW > 0
               ? nefes_uppixcos_scratch_doubles(G, OH, OW, crop) + (size_t)G * (1 + (size_t)CH * ((CW + kPixCols - 1) / kPixCols))
               : 0;
}

// The per-pixel losses, unmasked (mask = null) and masked: one body per entry-point pair
template <bool MASKED>
static int pixcos_loss_fwd(int G, int C, int64_t P, const float* a, const float* b, const uint8_t* mask, double* scratch, float* loss,
                           void* stream) {
    if (G <= 0 || G > 65535 || C <= 0 || P <= 0 || !a || !b || !scratch || !loss || (MASKED && !mask)) return NEFES_E_BADARG;
    const int64_t nb = (P + kPixCols - 1) / kPixCols;
    if (nb > 0x7fffffffl) return NEFES_E_UNSUPPORTED;
    double* stats = scratch + G;
    double* part = stats + (size_t)G * 3 * P;
    double* cnt = MASKED ? part + (size_t)G * nb : nullptr;
    double* count = MASKED ? cnt + (size_t)G * nb : nullptr;
    hipLaunchKernelGGL(pixcos_fwd_kernel<MASKED>, dim3((unsigned)nb, (unsigned)G), dim3(kPixBlock), 0, (hipStream_t)stream, C, (long)P, 1e-6, a, b,
                       mask, stats, part, cnt);
    hipLaunchKernelGGL(pixcos_final_kernel<MASKED>, dim3(1), dim3(256), 0, (hipStream_t)stream, G, (int)nb, (double)P, (const double*)part,
                       (const double*)cnt, scratch, count, loss);
    return (int)hipGetLastError();
}
extern "C" int nefes_pixcos_loss_fwd(int G, int C, int64_t P, const float* a, const float* b, double* scratch, float* loss, void* stream) {
    return pixcos_loss_fwd<false>(G, C, P, a, b, nullptr, scratch, loss, stream);
}
extern "C" int nefes_pixcos_loss_masked_fwd(int G, int C, int64_t P, const float* a, const float* b, const uint8_t* mask, double* scratch,
                                            float* loss, void* stream) {
    return pixcos_loss_fwd<true>(G, C, P, a, b, mask, scratch, loss, stream);
}

template <bool MASKED>
static int pixcos_loss_bwd(int G, int C, int64_t P, const float* a, const float* b, const uint8_t* mask, const double* scratch,
                           const float* g_loss, float* g_a, void* stream) {
    if (G <= 0 || G > 65535 || C <= 0 || P <= 0 || !a || !b || !scratch || !g_loss || !g_a || (MASKED && !mask)) return NEFES_E_BADARG;
    const long n = (long)G * C * P;
    if ((n + 255) / 256 > 0x7fffffffl) return NEFES_E_UNSUPPORTED;
    const int64_t nb = (P + kPixCols - 1) / kPixCols;
    const double* count = MASKED ? scratch + (size_t)G * (1 + 3 * (size_t)P + 2 * (size_t)nb) : nullptr;
    hipLaunchKernelGGL(pixcos_bwd_kernel<MASKED>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, C, (long)P, 1e-6, a, b,
                       mask, count, scratch + G, g_loss, g_a);
    return (int)hipGetLastError();
}
extern "C" int nefes_pixcos_loss_bwd(int G, int C, int64_t P, const float* a, const float* b, const double* scratch, const float* g_loss,
                                     float* g_a, void* stream) {
    return pixcos_loss_bwd<false>(G, C, P, a, b, nullptr, scratch, g_loss, g_a, stream);
}
extern "C" int nefes_pixcos_loss_masked_bwd(int G, int C, int64_t P, const float* a, const float* b, const uint8_t* mask, const double* scratch,
                                            const float* g_loss, float* g_a, void* stream) {
    return pixcos_loss_bwd<true>(G, C, P, a, b, mask, scratch, g_loss, g_a, stream);
}

template <bool MASKED>
static int uppixcos_loss_fwd(int G, int C, int h, int w, int OH, int OW, int crop, const float* x, const float* target, const uint8_t* mask,
                             double* scratch, float* loss, void* stream) {
    const int CH = OH - 2 * crop, CW = OW - 2 * crop;
    if (G <= 0 || G > 65535 || C <= 0 || h <= 0 || w <= 0 || crop < 0 || CH <= 0 || CW <= 0 || !x || !target || !scratch || !loss ||
        (MASKED && !mask))
        return NEFES_E_BADARG;
    if ((long)G * C > 0x7fffffffl) return NEFES_E_UNSUPPORTED;
    UpCosArgs a{G * C, h, w, OH, OW, crop, CH, CW, (float)h / OH, (float)w / OW, x, target};
    double* stats = scratch + G;
    double* part = stats + (size_t)G * 3 * CH * CW;
    const int nseg = (CW + kPixCols - 1) / kPixCols;
    if (nseg > 65535 || (long)CH * nseg > 0x7fffffffl) return NEFES_E_UNSUPPORTED;
    double* cnt = MASKED ? part + (size_t)G * CH * nseg : nullptr;
    double* count = MASKED ? cnt + (size_t)G * CH * nseg : nullptr;
    hipLaunchKernelGGL(uppixcos_fwd_kernel<MASKED>, dim3((unsigned)CH, (unsigned)nseg, (unsigned)G), dim3(kPixBlock), 0, (hipStream_t)stream, a, C,
                       1e-6, mask, stats, part, cnt);
    hipLaunchKernelGGL(pixcos_final_kernel<MASKED>, dim3(1), dim3(256), 0, (hipStream_t)stream, G, CH * nseg, (double)CH * CW, (const double*)part,
                       (const double*)cnt, scratch, count, loss);
    return (int)hipGetLastError();
}
extern "C" int nefes_uppixcos_loss_fwd(int G, int C, int h, int w, int OH, int OW, int crop, const float* x, const float* target,
                                       double* scratch, float* loss, void* stream) {
    return uppixcos_loss_fwd<false>(G, C, h, w, OH, OW, crop, x, target, nullptr, scratch, loss, stream);
}
extern "C" int nefes_uppixcos_loss_masked_fwd(int G, int C, int h, int w, int OH, int OW, int crop, const float* x, const float* target,
                                              const uint8_t* mask, double* scratch, float* loss, void* stream) {
    return uppixcos_loss_fwd<true>(G, C, h, w, OH, OW, crop, x, target, mask, scratch, loss, stream);
}

template <bool MASKED>
static int uppixcos_loss_bwd(int G, int C, int h, int w, int OH, int OW, int crop, const float* x, const float* target, const uint8_t* mask,
                             const double* scratch, const float* g_loss, const int* tx_first, const int* tx_count, const float* tx_wt,
                             const int* ty_first, const int* ty_count, const float* ty_wt, int T, float* tmp, float* g_x, void* stream) {
    const int CH = OH - 2 * crop, CW = OW - 2 * crop;
    if (G <= 0 || G > 65535 || C <= 0 || h <= 0 || w <= 0 || crop < 0 || CH <= 0 || CW <= 0 || !x || !target || !scratch || !g_loss || !tmp || !g_x ||
        (MASKED && !mask))
        return NEFES_E_BADARG;
    if (!tx_first || !tx_count || !tx_wt || !ty_first || !ty_count || !ty_wt || T <= 0) return NEFES_E_BADARG;
    const long planes = (long)G * C, n = planes * h * w;
    if (planes * CH > 0x7fffffffl || (n + 255) / 256 > 0x7fffffffl) return NEFES_E_UNSUPPORTED;
    const nefes_bicubic::GatherTable gx{tx_first, tx_count, tx_wt, T}, gy{ty_first, ty_count, ty_wt, T};
    UpCosArgs a{(int)planes, h, w, OH, OW, crop, CH, CW, (float)h / OH, (float)w / OW, x, target};
    const size_t lds = (size_t)(4 * w + CW) * 4;
    if (lds > 96 * 1024) return NEFES_E_UNSUPPORTED;
    hipError_t e = hipFuncSetAttribute((const void*)upcos_bwd_rows_kernel<MASKED, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    const size_t nparts = (size_t)CH * ((CW + kPixCols - 1) / kPixCols);
    const double* count = MASKED ? scratch + (size_t)G * (1 + 3 * (size_t)CH * CW + 2 * nparts) : nullptr;
    hipLaunchKernelGGL((upcos_bwd_rows_kernel<MASKED, true>), dim3((unsigned)(planes * CH)), dim3(128), lds, (hipStream_t)stream, a, C, 1e-6,
                       scratch + G, g_loss, gx, mask, count, tmp);
    hipLaunchKernelGGL(upcos_gather_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, planes, h, CH, (long)w, gy,
                       (const float*)tmp, g_x);
    return (int)hipGetLastError();
}
extern "C" int nefes_uppixcos_loss_bwd(int G, int C, int h, int w, int OH, int OW, int crop, const float* x, const float* target,
                                       const double* scratch, const float* g_loss, const int* tx_first, const int* tx_count, const float* tx_wt,
                                       const int* ty_first, const int* ty_count, const float* ty_wt, int T, float* tmp, float* g_x, void* stream) {
    return uppixcos_loss_bwd<false>(G, C, h, w, OH, OW, crop, x, target, nullptr, scratch, g_loss, tx_first, tx_count, tx_wt, ty_first, ty_count,
                                    ty_wt, T, tmp, g_x, stream);
}
extern "C" int nefes_uppixcos_loss_masked_bwd(int G, int C, int h, int w, int OH, int OW, int crop, const float* x, const float* target,
                                              const uint8_t* mask, const double* scratch, const float* g_loss, const int* tx_first,
                                              const int* tx_count, const float* tx_wt, const int* ty_first, const int* ty_count,
                                              const float* ty_wt, int T, float* tmp, float* g_x, void* stream) {
    return uppixcos_loss_bwd<true>(G, C, h, w, OH, OW, crop, x, target, mask, scratch, g_loss, tx_first, tx_count, tx_wt, ty_first, ty_count, ty_wt,
                                   T, tmp, g_x, stream);
}

extern "C" int nefes_bicubic_gram(int n_in, int n_out, int o0, int n_win, double* G, void* stream) {
    if (n_in <= 0 || n_out <= 0 || o0 < 0 || n_win <= 0 || o0 + n_win > n_out || !G) return NEFES_E_BADARG;
    if ((long)n_in * n_in > (1 << 24)) return NEFES_E_UNSUPPORTED;
    hipLaunchKernelGGL(bicubic_gram_kernel, dim3((unsigned)((n_in * n_in + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_in, o0, n_win,
                       (float)n_in / n_out, G);
    return (int)hipGetLastError();
}

extern "C" int nefes_upcos_prepare(int C, int h, int w, int OH, int OW, int crop, const float* target, const int* tx_first, const int* tx_count,
                                   const float* tx_wt, const int* ty_first, const int* ty_count, const float* ty_wt, int T, double* tmp,
                                   double* tt, double* dbb, void* stream) {
    const int CH = OH - 2 * crop, CW = OW - 2 * crop;
    if (C <= 0 || h <= 0 || w <= 0 || crop < 0 || CH <= 0 || CW <= 0 || !target || !tmp || !tt || !dbb) return NEFES_E_BADARG;
    if (!tx_first || !tx_count || !tx_wt || !ty_first || !ty_count || !ty_wt || T <= 0) return NEFES_E_BADARG;
    const nefes_bicubic::GatherTable gx{tx_first, tx_count, tx_wt, T}, gy{ty_first, ty_count, ty_wt, T};
    const long n1 = (long)C * CH * w, n2 = (long)C * h * w;
    if ((n1 + 255) / 256 > 0x7fffffffl) return NEFES_E_UNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(upcos_prep_rows_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, st, n1, CW, w, gx, target, tmp);
    hipLaunchKernelGGL(upcos_prep_cols_kernel, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, st, n2, h, CH, w, gy, (const double*)tmp, tt);
    hipLaunchKernelGGL(upcos_prep_norm_kernel, dim3((unsigned)C), dim3(256), 0, st, (long)CH * CW, target, dbb);
    return (int)hipGetLastError();
}

// LDS bytes of one upcos_gram_fwd_kernel workgroup (a band of rows of one channel: Q = X Gx and the two Gram bands); the launch needs
// it within NEFES_UPCOS_GRAM_LDS_MAX.  Callers ask BEFORE they commit to the prepared-target form (ops.UpcosTarget.fits): the one-pass
// kernels (nefes_upcos_loss_fwd / _bwd) take any geometry.
#define NEFES_UPCOS_GRAM_LDS_MAX (96 * 1024)
extern "C" size_t nefes_upcos_gram_lds_bytes(int h, int w, int band) {
    if (h <= 0 || w <= 0 || band < 0) return 0;
    const int per = (h + kParts - 1) / kParts;
    return (size_t)(per + 2 * band) * w * 12 + (size_t)(w + per) * (2 * band + 1) * 8;
}

extern "C" int nefes_upcos_gram_fwd(int C, int h, int w, const float* x, const double* tt, const double* dbb, const double* gram_x,
                                    const double* gram_y, int band, double* scratch, double* pmat, float* loss, void* stream) {
    if (C <= 0 || h <= 0 || w <= 0 || band < 0 || !x || !tt || !dbb || !gram_x || !gram_y || !scratch || !pmat || !loss) return NEFES_E_BADARG;
    const size_t lds = nefes_upcos_gram_lds_bytes(h, w, band);
    if (lds > NEFES_UPCOS_GRAM_LDS_MAX) return NEFES_E_UNSUPPORTED;
    // the kernel's dynamic-LDS ceiling, once per device of this process (a constant: not state a caller could observe)
    static std::atomic<unsigned long long> attr_set{0};
    int dev = 0;
    (void)hipGetDevice(&dev);
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(attr_set.load(std::memory_order_relaxed) & bit)) {
        hipError_t e = hipFuncSetAttribute((const void*)upcos_gram_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, NEFES_UPCOS_GRAM_LDS_MAX);
        if (e != hipSuccess) return (int)e;
        attr_set.fetch_or(bit, std::memory_order_relaxed);
    }
    double* part = scratch + (size_t)C * 4;
    hipLaunchKernelGGL(upcos_gram_fwd_kernel, dim3((unsigned)(C * kParts)), dim3(256), lds, (hipStream_t)stream, h, w, band, x, tt, dbb, gram_x,
                       gram_y, part, pmat);
    hipLaunchKernelGGL(cosine_final_groups_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, 1, C, 1e-6, (const double*)part, scratch, loss);
    return (int)hipGetLastError();
}

extern "C" int nefes_upcos_gram_bwd(int C, int h, int w, const double* tt, const double* pmat, const double* scratch, const float* g_loss,
                                    float* g_x, void* stream) {
    if (C <= 0 || h <= 0 || w <= 0 || !tt || !pmat || !scratch || !g_loss || !g_x) return NEFES_E_BADARG;
    const long n = (long)C * h * w;
    hipLaunchKernelGGL(upcos_gram_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, C, (long)h * w, 1e-6, tt, pmat,
                       scratch, g_loss, g_x);
    return (int)hipGetLastError();
}


extern "C" size_t nefes_cosine_loss_scratch_doubles(int C) { return C > 0 ? (size_t)C * (kParts * 3 + 4) : 0; }

// a, b [G, Cg, P], mask [G, P]; loss = sum_g (1 - mean of the group's Cg cosines over its valid pixels).  The unmasked entry points are
// one group of C channels; since they share this body they refuse a grid beyond 2^31 - 1 blocks (NEFES_E_UNSUPPORTED) as the masked
// ones always did, where they used to launch it.
template <bool MASKED>
static int cosine_loss_fwd(int G, int Cg, int64_t P, const float* a, const float* b, const uint8_t* mask, double* scratch, float* loss,
                           void* stream) {
    if (G <= 0 || Cg <= 0 || P <= 0 || !a || !b || (MASKED && !mask) || !scratch || !loss) return NEFES_E_BADARG;
    if ((long)G * Cg * kParts > 0x7fffffffl) return NEFES_E_UNSUPPORTED;
    const int C = G * Cg;
    double* part = scratch + (size_t)C * 4;
    hipLaunchKernelGGL(cosine_partial_kernel<MASKED>, dim3(C * kParts), dim3(256), 0, (hipStream_t)stream, C, (long)P, a, b, mask, Cg, part);
    hipLaunchKernelGGL(cosine_final_groups_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, G, Cg, 1e-6, (const double*)part, scratch, loss);
    return (int)hipGetLastError();
}
extern "C" int nefes_cosine_loss_fwd(int C, int64_t P, const float* a, const float* b, double* scratch, float* loss, void* stream) {
    return cosine_loss_fwd<false>(1, C, P, a, b, nullptr, scratch, loss, stream);
}
extern "C" int nefes_cosine_loss_masked_fwd(int G, int Cg, int64_t P, const float* a, const float* b, const uint8_t* mask, double* scratch,
                                            float* loss, void* stream) {
    return cosine_loss_fwd<true>(G, Cg, P, a, b, mask, scratch, loss, stream);
}

template <bool MASKED>
static int cosine_loss_bwd(int G, int Cg, int64_t P, const float* a, const float* b, const uint8_t* mask, const double* scratch,
                           const float* g_loss, float* g_a, void* stream) {
    if (G <= 0 || Cg <= 0 || P <= 0 || !a || !b || (MASKED && !mask) || !scratch || !g_loss || !g_a) return NEFES_E_BADARG;
    const long n = (long)G * Cg * P;
    if ((long)G * Cg > 0x7fffffffl || (n + 255) / 256 > 0x7fffffffl) return NEFES_E_UNSUPPORTED;
    hipLaunchKernelGGL(cosine_bwd_kernel<MASKED>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, G * Cg, (long)P, 1e-6, a, b,
                       mask, Cg, scratch, g_loss, g_a);
    return (int)hipGetLastError();
}
extern "C" int nefes_cosine_loss_bwd(int C, int64_t P, const float* a, const float* b, const double* scratch, const float* g_loss,
                                     float* g_a, void* stream) {
    return cosine_loss_bwd<false>(1, C, P, a, b, nullptr, scratch, g_loss, g_a, stream);
}
extern "C" int nefes_cosine_loss_masked_bwd(int G, int Cg, int64_t P, const float* a, const float* b, const uint8_t* mask, const double* scratch,
                                            const float* g_loss, float* g_a, void* stream) {
    return cosine_loss_bwd<true>(G, Cg, P, a, b, mask, scratch, g_loss, g_a, stream);
}


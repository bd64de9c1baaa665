// The geometric term of an RGB-D pose refinement: a Huber loss between normalised rendered depth and a measured depth map.
//
//   d = 1 / disp            the compositor writes disp = 1 / max(1e-10, depth / sum_s w_s) with the weights each variant normalises by
//                           (nerfh_nff.py:113-118, :164-166), so 1 / disp is the normalised z-depth of the ray in all of them --
//                           rays_d is unnormalised with camera z = -1: the ray parameter IS z-depth, what a Kinect frame holds;
//   e = d - target;         rho(e) = e^2 / (2 delta) for |e| <= delta, |e| - delta / 2 beyond (torch.nn.SmoothL1Loss(beta = delta));
//   L_g = mean of rho over the VALID pixels of group (image) g;   value = weight * sum_g L_g.
// Valid: target finite and > 0 (a sensor hole is 0, Inf or NaN), disp finite and > 0 (a ray that met no density has disp = NaN), the
// mask byte != 0 where there is a mask.  A select, as in the masked feature losses (feature_loss.hip): an invalid pixel's values enter
// no arithmetic, its gradient is exactly 0, a group without a valid pixel is worth 0 with a zero gradient.  Per-pixel arithmetic in
// double from the float32 inputs, sums in double in a fixed order, no atomics, every output rounded to float32 once.
// The gradient goes to disp -- g_disp is what both compositor backward paths already take.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/nefes_hip.h"
#include "wave.h"

namespace {
constexpr int kDepthBlock = 1024;      // the forward's ONE workgroup: 16 waves walk the pixels of every group in turn

// the pixel's residual e = 1 / disp - target; false: not valid (nothing was computed)
__device__ __forceinline__ bool depth_residual(const float* __restrict__ disp, const float* __restrict__ target,
                                               const uint8_t* __restrict__ mask, long i, double* e) {
    if (mask && !mask[i]) return false;
    const float t = target[i], d = disp[i];
    if (!(t > 0.f && t <= 3.402823466e+38f) || !(d > 0.f && d <= 3.402823466e+38f)) return false;      // (NaN fails every comparison)
    *e = 1.0 / (double)d - (double)t;
    return true;
}

// sum over the workgroup's threads, on every thread: the lanes of a wave on wave_sum (wave.h), the waves' sums added in wave order
__device__ __forceinline__ double depth_block_sum(double v, double* __restrict__ sh) {
    v = wave_sum(v);
    __syncthreads();                                   // (the previous sum's readers are done with sh)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = sh[0];
#pragma unroll
    for (int w = 1; w < kDepthBlock / 64; ++w) t += sh[w];
    return t;
}

// One launch, one workgroup: group after group, thread t adds the pixels t, t + 1024, ... in ascending order, then the block sum.
// scratch: L_g [G] (weight not applied) | the valid counts [G]
__global__ __launch_bounds__(kDepthBlock) void depth_loss_fwd_kernel(int G, long P, const float* __restrict__ disp,
                                                                     const float* __restrict__ target, const uint8_t* __restrict__ mask,
                                                                     double delta, double weight, int accumulate,
                                                                     double* __restrict__ scratch, float* loss) {
    __shared__ double sh[kDepthBlock / 64];
    double total = 0;
    for (int g = 0; g < G; ++g) {
        double s = 0, n = 0;
        for (long p = threadIdx.x; p < P; p += kDepthBlock) {
            double e;
            if (depth_residual(disp, target, mask, (long)g * P + p, &e)) {
                const double a = fabs(e);
                s += a <= delta ? e * e / (2.0 * delta) : a - 0.5 * delta;
                n += 1.0;
            }
        }
        s = depth_block_sum(s, sh);
        n = depth_block_sum(n, sh);                    // (whole numbers: exact in any order)
        const double Lg = n > 0 ? s / n : 0.0;
        if (threadIdx.x == 0) {
            scratch[g] = Lg;
            scratch[G + g] = n;
        }
        total += Lg;
    }
    if (threadIdx.x == 0) {
        const double v = weight * total;
        loss[0] = (float)(accumulate ? (double)loss[0] + v : v);
    }
}

// one thread per pixel: g_disp = g_loss weight rho'(e) / n_g * (-1 / disp^2), exactly 0 at an invalid pixel
__global__ __launch_bounds__(256) void depth_loss_bwd_kernel(long n, int G, long P, const float* __restrict__ disp,
                                                             const float* __restrict__ target, const uint8_t* __restrict__ mask, double delta,
                                                             double weight, const double* __restrict__ scratch,
                                                             const float* __restrict__ g_loss, float* __restrict__ g_disp) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double e;
    if (!depth_residual(disp, target, mask, i, &e)) {
        g_disp[i] = 0.f;
        return;
    }
    const double d = (double)disp[i], a = fabs(e);
    const double dr = a <= delta ? e / delta : (e > 0 ? 1.0 : -1.0);
    g_disp[i] = (float)((double)g_loss[0] * weight * dr / scratch[G + i / P] * (-1.0 / (d * d)));
}

bool depth_args_ok(int G, int64_t P, const void* disp, const void* target, double delta, double weight) {
    return G > 0 && G <= 65535 && P > 0 && disp && target && delta > 0 && isfinite(delta) && isfinite(weight);
}
}  // namespace

extern "C" size_t nefes_depth_loss_scratch_doubles(int G) { return G > 0 ? 2 * (size_t)G : 0; }

extern "C" int nefes_depth_loss_fwd(int G, int64_t P, const float* disp, const float* target, const uint8_t* mask, double delta,
                                    double weight, int accumulate, double* scratch, float* loss, void* stream) {
    if (!depth_args_ok(G, P, disp, target, delta, weight) || !scratch || !loss) return NEFES_E_BADARG;
    if (P > (0x7fffffffl * 256) / G) return NEFES_E_UNSUPPORTED;       // (the backward could not follow)
    hipLaunchKernelGGL(depth_loss_fwd_kernel, dim3(1), dim3(kDepthBlock), 0, (hipStream_t)stream, G, (long)P, disp, target, mask, delta,
                       weight, accumulate, scratch, loss);
    return (int)hipGetLastError();
}

extern "C" int nefes_depth_loss_bwd(int G, int64_t P, const float* disp, const float* target, const uint8_t* mask, double delta,
                                    double weight, const double* scratch, const float* g_loss, float* g_disp, void* stream) {
    if (!depth_args_ok(G, P, disp, target, delta, weight) || !scratch || !g_loss || !g_disp) return NEFES_E_BADARG;
    if (P > (0x7fffffffl * 256) / G) return NEFES_E_UNSUPPORTED;
    const long n = (long)G * P;
    hipLaunchKernelGGL(depth_loss_bwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, G, (long)P, disp,
                       target, mask, delta, weight, scratch, g_loss, g_disp);
    return (int)hipGetLastError();
}

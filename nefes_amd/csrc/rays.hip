// Ray generation / NDC warp / coarse depths and the pose-gradient reductions.
// Restates script/models/ray_utils.py:5-16 (get_rays), :27-44 (ndc_rays), rendering.py:96-112 (z_vals),
// :217 (viewdirs) and the autograd backward of those ops down to the 3x4 camera-to-world pose.
// All HBM-bound and tiny next to the MLP (36 B written per ray forward, 36 B read per ray backward).
#include "../../include/nefes_hip.h"
#include "wave.h"

// ---- get_rays + viewdirs, forward and backward: one kernel body over two small functors ----------------------------------------
// Where ray idx's pixel (x, y) = (column, row) comes from:
//   GridPixels: the frame's rows from row0 on, row-major (raygen, raygen_k);
//   ListPixels: a float32 [n, 2] list in device memory, read when the kernel runs like the device camera (raygen_px).  Any value is
//               legal: an integer coordinate is that pixel (no half-pixel offset), fractions and points outside the frame are rays too.
// Where the camera (fx, fy, cx, cy) comes from:
//   ValueCamera:  four launch arguments (raygen: fx = fy = focal, cx = (float)(W*.5), cy = (float)(H*.5), formed by the host).  The
//                 backward forms the twelve pose sums (kSums = 12).
//   DeviceCamera: intr[4] READ FROM DEVICE MEMORY when the kernel runs, never passed by value (raygen_k, raygen_px): a captured
//                 iteration follows a camera that is updated in place between replays, and the backward can hand a gradient to it --
//                 four more sums, d L / d (fx, fy, cx, cy) (kSums = 16).
// Both cameras feed the same operations in the same order, so at intr = (focal, focal, (float)(W*.5), (float)(H*.5)) the rays and the
// twelve pose sums of the two are equal bit for bit, as are a grid's and the list of its row-major integer pixels.  Three pairs are
// instantiated: (grid, value), (grid, device), (list, device).  A kernel takes its camera as Camera::Arg and builds the functor from it.
struct GridPixels {
    int W, row0;
    __device__ __forceinline__ void operator()(int idx, float& x, float& y) const {
        x = (float)(idx % W);
        y = (float)(row0 + idx / W);
    }
};
struct ListPixels {
    const float* px;
    __device__ __forceinline__ void operator()(int idx, float& x, float& y) const {
        x = px[(size_t)idx * 2];
        y = px[(size_t)idx * 2 + 1];
    }
};
struct ValueCamera {
    using Arg = ValueCamera;
    static constexpr int kSums = 12;
    float fx_, fy_, cx_, cy_;
    __device__ __forceinline__ float fx() const { return fx_; }
    __device__ __forceinline__ float fy() const { return fy_; }
    __device__ __forceinline__ float cx() const { return cx_; }
    __device__ __forceinline__ float cy() const { return cy_; }
};
struct DeviceCamera {
    using Arg = const float* __restrict__;   // (restrict has to stand on the kernel's own argument to reach the compiler)
    static constexpr int kSums = 16;
    const float* intr;
    __device__ __forceinline__ float fx() const { return intr[0]; }
    __device__ __forceinline__ float fy() const { return intr[1]; }
    __device__ __forceinline__ float cx() const { return intr[2]; }
    __device__ __forceinline__ float cy() const { return intr[3]; }
};

template <class Camera>
__device__ __forceinline__ void pixel_dir(const Camera& cam, float x, float y, float (&dc)[3]) {
    // dirs = [(x - cx)/fx, -(y - cy)/fy, -1]   (ray_utils.py:10; no half-pixel offset)
    dc[0] = __fdiv_rn(__fsub_rn(x, cam.cx()), cam.fx());
    dc[1] = -__fdiv_rn(__fsub_rn(y, cam.cy()), cam.fy());
    dc[2] = -1.f;
}

template <class Pixels, class Camera>
__global__ __launch_bounds__(256) void raygen_fwd_kernel(Pixels pixel, typename Camera::Arg arg, const float* __restrict__ c2w, int n,
                                                         float* rays_o, float* rays_d, float* viewdirs) {
    const Camera cam{arg};
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    float x, y;
    pixel(idx, x, y);
    float dc[3];
    pixel_dir(cam, x, y, dc);
    float d[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {   // rays_d[a] = sum_b dirs[b] * c2w[a][b]  (:13)
        const float p0 = __fmul_rn(dc[0], c2w[a * 4 + 0]), p1 = __fmul_rn(dc[1], c2w[a * 4 + 1]),
                    p2 = __fmul_rn(dc[2], c2w[a * 4 + 2]);
        d[a] = __fadd_rn(__fadd_rn(p0, p1), p2);
    }
    const float nrm = __fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(d[0], d[0]), __fmul_rn(d[1], d[1])), __fmul_rn(d[2], d[2])));
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        rays_o[(size_t)idx * 3 + a] = c2w[a * 4 + 3];                    // :15
        rays_d[(size_t)idx * 3 + a] = d[a];
        if (viewdirs) viewdirs[(size_t)idx * 3 + a] = __fdiv_rn(d[a], nrm);   // rendering.py:217
    }
}

// stage 1: per-block partial of the kSums sums (f64) -- the 12 pose-gradient sums, then, for a device camera, d L/d (fx, fy, cx, cy);
// stage 2: fixed-order final sum.  With gd the gradient reaching rays_d and R_a column a of the rotation:
//     d dirs_0 / d fx = -(x - cx)/fx^2 = -dirs_0/fx     d dirs_0 / d cx = -1/fx
//     d dirs_1 / d fy = +(y - cy)/fy^2 = -dirs_1/fy     d dirs_1 / d cy = +1/fy
template <class Pixels, class Camera>
__global__ __launch_bounds__(256) void raygen_bwd_kernel(Pixels pixel, typename Camera::Arg arg, const float* __restrict__ c2w, int n,
                                                         const float* g_o, const float* g_d, const float* g_v, double* partial) {
    constexpr int K = Camera::kSums;
    const Camera cam{arg};
    __shared__ double red[4][K];
    double s[K];
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = 0.0;
    float ifx = 0.f, ify = 0.f;
    if constexpr (K == 16) {
        ifx = __fdiv_rn(1.f, cam.fx());
        ify = __fdiv_rn(1.f, cam.fy());
    }
    for (int idx = blockIdx.x * 256 + threadIdx.x; idx < n; idx += gridDim.x * 256) {
        float x, y;
        pixel(idx, x, y);
        float dc[3];
        pixel_dir(cam, x, y, dc);
        float gd[3] = {0.f, 0.f, 0.f};
        if (g_d)
#pragma unroll
            for (int a = 0; a < 3; ++a) gd[a] = g_d[(size_t)idx * 3 + a];
        if (g_v) {   // v = d/|d|  =>  d L/d d += (g - v (v.g)) / |d|
            float d[3];
#pragma unroll
            for (int a = 0; a < 3; ++a)
                d[a] = __fadd_rn(__fadd_rn(__fmul_rn(dc[0], c2w[a * 4]), __fmul_rn(dc[1], c2w[a * 4 + 1])), __fmul_rn(dc[2], c2w[a * 4 + 2]));
            const float nrm = __fsqrt_rn(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            const float gv0 = g_v[(size_t)idx * 3], gv1 = g_v[(size_t)idx * 3 + 1], gv2 = g_v[(size_t)idx * 3 + 2];
            const float v0 = d[0] / nrm, v1 = d[1] / nrm, v2 = d[2] / nrm;
            const float dot = v0 * gv0 + v1 * gv1 + v2 * gv2;
            gd[0] += (gv0 - v0 * dot) / nrm;
            gd[1] += (gv1 - v1 * dot) / nrm;
            gd[2] += (gv2 - v2 * dot) / nrm;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int b = 0; b < 3; ++b) s[a * 4 + b] += (double)gd[a] * (double)dc[b];
            if (g_o) s[a * 4 + 3] += (double)g_o[(size_t)idx * 3 + a];
        }
        if constexpr (K == 16) {   // gd . R_0 and gd . R_1 in fp32, the camera's factor in fp32, the product and the sum in f64
            const float r0 = __fadd_rn(__fadd_rn(__fmul_rn(gd[0], c2w[0]), __fmul_rn(gd[1], c2w[4])), __fmul_rn(gd[2], c2w[8]));
            const float r1 = __fadd_rn(__fadd_rn(__fmul_rn(gd[0], c2w[1]), __fmul_rn(gd[1], c2w[5])), __fmul_rn(gd[2], c2w[9]));
            s[12] += (double)(-__fmul_rn(dc[0], ifx)) * (double)r0;   // fx
            s[13] += (double)(-__fmul_rn(dc[1], ify)) * (double)r1;   // fy
            s[14] += (double)(-ifx) * (double)r0;                     // cx
            s[15] += (double)ify * (double)r1;                        // cy
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double v = wave_sum(s[k]);
        if (lane == 0) red[wave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < K) partial[(size_t)blockIdx.x * K + threadIdx.x] =
        ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}
__global__ void raygen_bwd_final(const double* partial, int nblocks, int nsums, float* g_c2w, float* g_intr) {
    const int k = threadIdx.x;
    if (k >= nsums) return;
    double s = 0.0;
    for (int b = 0; b < nblocks; ++b) s += partial[(size_t)b * nsums + k];
    if (k < 12) g_c2w[k] = (float)s;
    else if (g_intr) g_intr[k - 12] = (float)s;
}

static int raygen_blocks(int n) {
    int b = (n + 255) / 256;
    return b > 1024 ? 1024 : (b < 1 ? 1 : b);
}

template <class Pixels, class Camera>
static int raygen_fwd_launch(Pixels pixel, typename Camera::Arg cam, const float* c2w, int n, float* rays_o, float* rays_d, float* viewdirs,
                             void* stream) {
    raygen_fwd_kernel<Pixels, Camera><<<dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream>>>(pixel, cam, c2w, n, rays_o, rays_d,
                                                                                                  viewdirs);
    return (int)hipGetLastError();
}
template <class Pixels, class Camera>
static int raygen_bwd_launch(Pixels pixel, typename Camera::Arg cam, const float* c2w, int n, const float* g_rays_o, const float* g_rays_d,
                             const float* g_viewdirs, void* workspace, float* g_c2w, float* g_intr, void* stream) {
    const int nb = raygen_blocks(n);
    hipStream_t st = (hipStream_t)stream;
    raygen_bwd_kernel<Pixels, Camera><<<dim3(nb), dim3(256), 0, st>>>(pixel, cam, c2w, n, g_rays_o, g_rays_d, g_viewdirs,
                                                                     (double*)workspace);
    raygen_bwd_final<<<dim3(1), dim3(64), 0, st>>>((const double*)workspace, nb, Camera::kSums, g_c2w, g_intr);
    return (int)hipGetLastError();
}
static size_t raygen_workspace(int n_rays, int sums) { return (size_t)raygen_blocks(n_rays) * sums * sizeof(double); }
// the focal camera, centred: the double product and the one conversion the focal kernels made per ray, made once
static ValueCamera focal_camera(int H, int W, float focal) { return ValueCamera{focal, focal, (float)(W * .5), (float)(H * .5)}; }

extern "C" int nefes_raygen_fwd(int H, int W, float focal, const float* c2w, int row0, int nrows, float* rays_o,
                                float* rays_d, float* viewdirs, void* stream) {
    if (!c2w || !rays_o || !rays_d || H <= 0 || W <= 0 || nrows <= 0 || row0 < 0 || row0 + nrows > H) return NEFES_E_BADARG;
    return raygen_fwd_launch<GridPixels, ValueCamera>(GridPixels{W, row0}, focal_camera(H, W, focal), c2w, nrows * W, rays_o, rays_d,
                                                      viewdirs, stream);
}
extern "C" size_t nefes_raygen_bwd_workspace(int n_rays) { return raygen_workspace(n_rays, ValueCamera::kSums); }
extern "C" int nefes_raygen_bwd(int H, int W, float focal, const float* c2w, int row0, int nrows, const float* g_rays_o,
                                const float* g_rays_d, const float* g_viewdirs, void* workspace, float* g_c2w,
                                void* stream) {
    if (!c2w || !workspace || !g_c2w || H <= 0 || W <= 0 || nrows <= 0 || row0 < 0 || row0 + nrows > H) return NEFES_E_BADARG;
    return raygen_bwd_launch<GridPixels, ValueCamera>(GridPixels{W, row0}, focal_camera(H, W, focal), c2w, nrows * W, g_rays_o, g_rays_d,
                                                      g_viewdirs, workspace, g_c2w, nullptr, stream);
}

// pinhole intrinsics intr[4] = (fx, fy, cx, cy) in device memory (DeviceCamera)
extern "C" int nefes_raygen_k_fwd(int H, int W, const float* intr, const float* c2w, int row0, int nrows, float* rays_o,
                                  float* rays_d, float* viewdirs, void* stream) {
    if (!intr || !c2w || !rays_o || !rays_d || H <= 0 || W <= 0 || nrows <= 0 || row0 < 0 || row0 + nrows > H)
        return NEFES_E_BADARG;
    return raygen_fwd_launch<GridPixels, DeviceCamera>(GridPixels{W, row0}, intr, c2w, nrows * W, rays_o, rays_d, viewdirs, stream);
}
extern "C" size_t nefes_raygen_k_bwd_workspace(int n_rays) { return raygen_workspace(n_rays, DeviceCamera::kSums); }
extern "C" int nefes_raygen_k_bwd(int H, int W, const float* intr, const float* c2w, int row0, int nrows, const float* g_rays_o,
                                  const float* g_rays_d, const float* g_viewdirs, void* workspace, float* g_c2w, float* g_intr,
                                  void* stream) {
    if (!intr || !c2w || !workspace || !g_c2w || H <= 0 || W <= 0 || nrows <= 0 || row0 < 0 || row0 + nrows > H)
        return NEFES_E_BADARG;
    return raygen_bwd_launch<GridPixels, DeviceCamera>(GridPixels{W, row0}, intr, c2w, nrows * W, g_rays_o, g_rays_d, g_viewdirs, workspace,
                                                       g_c2w, g_intr, stream);
}

// the same rays and sums at a list of pixels px [n, 2] = (x, y) in device memory (ListPixels)
extern "C" int nefes_raygen_px_fwd(int n, const float* px, const float* intr, const float* c2w, float* rays_o, float* rays_d,
                                   float* viewdirs, void* stream) {
    if (!px || !intr || !c2w || !rays_o || !rays_d || n <= 0) return NEFES_E_BADARG;
    return raygen_fwd_launch<ListPixels, DeviceCamera>(ListPixels{px}, intr, c2w, n, rays_o, rays_d, viewdirs, stream);
}
extern "C" size_t nefes_raygen_px_bwd_workspace(int n) { return nefes_raygen_k_bwd_workspace(n); }
extern "C" int nefes_raygen_px_bwd(int n, const float* px, const float* intr, const float* c2w, const float* g_rays_o,
                                   const float* g_rays_d, const float* g_viewdirs, void* workspace, float* g_c2w, float* g_intr,
                                   void* stream) {
    if (!px || !intr || !c2w || !workspace || !g_c2w || n <= 0) return NEFES_E_BADARG;
    return raygen_bwd_launch<ListPixels, DeviceCamera>(ListPixels{px}, intr, c2w, n, g_rays_o, g_rays_d, g_viewdirs, workspace, g_c2w, g_intr,
                                                       stream);
}

// ---- bilinear sample of a [C, H, W] map at a pixel list (the targets of a sparse feature loss) ----------------------------------
// out[c, i] = map[c] at px[i] = (x, y), channel-major as the loss kernels read it.  (x, y) is clamped to the frame first, then split
// into cell and fraction; the second tap's index is clamped to the last column / row, so x = W-1 reads nothing past the row.  Each
// interpolation is a + f (b - a): at an integer coordinate f = 0 and the value is the map's own, exactly.  A NaN coordinate clamps
// to 0 (fmaxf returns the other operand): no index leaves the map for any input.
// NEAREST (nefes_sample_px_nearest): the one tap at column clamp(floor(x + 0.5), 0, W-1), row clamp(floor(y + 0.5), 0, H-1) instead -- the
// sum in double, exact for every float32 coordinate; NaN clamps to 0 as above.  For maps that must not be blended (a depth frame with
// holes); at an integer coordinate both instances return the map's own value.
template <bool NEAREST>
__global__ __launch_bounds__(256) void sample_px_kernel(int C, int H, int W, const float* __restrict__ map, int n,
                                                        const float* __restrict__ px, float* out) {
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)C * n) return;
    const int i = (int)(t % n);
    const size_t c = t / n;
    if (NEAREST) {
        const int xn = (int)fmin(fmax(floor((double)px[(size_t)i * 2] + 0.5), 0.0), (double)(W - 1));
        const int yn = (int)fmin(fmax(floor((double)px[(size_t)i * 2 + 1] + 0.5), 0.0), (double)(H - 1));
        out[t] = map[c * (size_t)H * W + (size_t)yn * W + xn];
        return;
    }
    const float x = fminf(fmaxf(px[(size_t)i * 2], 0.f), (float)(W - 1));
    const float y = fminf(fmaxf(px[(size_t)i * 2 + 1], 0.f), (float)(H - 1));
    const int x0 = (int)x, y0 = (int)y;                      // x, y >= 0: truncation is the floor
    const int x1 = x0 + 1 < W ? x0 + 1 : W - 1, y1 = y0 + 1 < H ? y0 + 1 : H - 1;
    const float fx = __fsub_rn(x, (float)x0), fy = __fsub_rn(y, (float)y0);
    const float* m = map + c * (size_t)H * W;
    const float m00 = m[(size_t)y0 * W + x0], m01 = m[(size_t)y0 * W + x1], m10 = m[(size_t)y1 * W + x0], m11 = m[(size_t)y1 * W + x1];
    const float top = __fadd_rn(m00, __fmul_rn(fx, __fsub_rn(m01, m00)));
    const float bot = __fadd_rn(m10, __fmul_rn(fx, __fsub_rn(m11, m10)));
    out[t] = __fadd_rn(top, __fmul_rn(fy, __fsub_rn(bot, top)));
}
template <bool NEAREST>
static int sample_px_launch(int C, int H, int W, const float* map, int n, const float* px, float* out, void* stream) {
    if (!map || !px || !out || C <= 0 || H <= 0 || W <= 0 || n <= 0) return NEFES_E_BADARG;
    const size_t total = (size_t)C * n;
    hipLaunchKernelGGL(sample_px_kernel<NEAREST>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, C, H, W, map, n,
                       px, out);
    return (int)hipGetLastError();
}
extern "C" int nefes_sample_px(int C, int H, int W, const float* map, int n, const float* px, float* out, void* stream) {
    return sample_px_launch<false>(C, H, W, map, n, px, out, stream);
}
extern "C" int nefes_sample_px_nearest(int C, int H, int W, const float* map, int n, const float* px, float* out, void* stream) {
    return sample_px_launch<true>(C, H, W, map, n, px, out, stream);
}

// ---- ndc_rays (ray_utils.py:27-44) ------------------------------------------------------------
struct Ndc {
    float t, ox, oy, oz, kx, ky;
};
__device__ __forceinline__ Ndc ndc_common(int H, int W, float focal, float near, const float* o, const float* d) {
    Ndc r;
    r.t = -(near + o[2]) / d[2];
    r.ox = o[0] + r.t * d[0];
    r.oy = o[1] + r.t * d[1];
    r.oz = o[2] + r.t * d[2];
    r.kx = (float)(-1. / (W / (2. * (double)focal)));
    r.ky = (float)(-1. / (H / (2. * (double)focal)));
    return r;
}
__global__ __launch_bounds__(256) void ndc_fwd_kernel(int H, int W, float focal, float near, int n, const float* ro,
                                                      const float* rd, float* oo, float* od) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* o = ro + (size_t)i * 3;
    const float* d = rd + (size_t)i * 3;
    const Ndc r = ndc_common(H, W, focal, near, o, d);
    oo[(size_t)i * 3 + 0] = r.kx * r.ox / r.oz;
    oo[(size_t)i * 3 + 1] = r.ky * r.oy / r.oz;
    oo[(size_t)i * 3 + 2] = 1.f + 2.f * near / r.oz;
    od[(size_t)i * 3 + 0] = r.kx * (d[0] / d[2] - r.ox / r.oz);
    od[(size_t)i * 3 + 1] = r.ky * (d[1] / d[2] - r.oy / r.oz);
    od[(size_t)i * 3 + 2] = -2.f * near / r.oz;
}
__global__ __launch_bounds__(256) void ndc_bwd_kernel(int H, int W, float focal, float near, int n, const float* ro,
                                                      const float* rd, const float* goo, const float* god, float* gro,
                                                      float* grd) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* o = ro + (size_t)i * 3;
    const float* d = rd + (size_t)i * 3;
    const Ndc r = ndc_common(H, W, focal, near, o, d);
    float go[3] = {0, 0, 0}, gd[3] = {0, 0, 0};
    if (goo) { go[0] = goo[(size_t)i * 3]; go[1] = goo[(size_t)i * 3 + 1]; go[2] = goo[(size_t)i * 3 + 2]; }
    if (god) { gd[0] = god[(size_t)i * 3]; gd[1] = god[(size_t)i * 3 + 1]; gd[2] = god[(size_t)i * 3 + 2]; }
    const float iz = 1.f / r.oz, idz = 1.f / d[2];
    // gradients w.r.t. the shifted origin (ox,oy,oz) and the direction terms d0/d2, d1/d2
    const float g_ox = (go[0] - gd[0]) * r.kx * iz;
    const float g_oy = (go[1] - gd[1]) * r.ky * iz;
    const float g_oz = -(go[0] - gd[0]) * r.kx * r.ox * iz * iz - (go[1] - gd[1]) * r.ky * r.oy * iz * iz
                       - (go[2] - gd[2]) * 2.f * near * iz * iz;
    float g_d0 = gd[0] * r.kx * idz, g_d1 = gd[1] * r.ky * idz;
    float g_d2 = -gd[0] * r.kx * d[0] * idz * idz - gd[1] * r.ky * d[1] * idz * idz;
    // shifted origin = o + t d, t = -(near + o2)/d2
    const float g_t = g_ox * d[0] + g_oy * d[1] + g_oz * d[2];
    g_d0 += g_ox * r.t; g_d1 += g_oy * r.t; g_d2 += g_oz * r.t;
    const float g_o2 = g_oz + g_t * (-idz);
    g_d2 += g_t * ((near + o[2]) * idz * idz);
    gro[(size_t)i * 3 + 0] = g_ox; gro[(size_t)i * 3 + 1] = g_oy; gro[(size_t)i * 3 + 2] = g_o2;
    grd[(size_t)i * 3 + 0] = g_d0; grd[(size_t)i * 3 + 1] = g_d1; grd[(size_t)i * 3 + 2] = g_d2;
}
extern "C" int nefes_ndc_fwd(int H, int W, float focal, float near, int n, const float* rays_o, const float* rays_d,
                             float* out_o, float* out_d, void* stream) {
    if (!rays_o || !rays_d || !out_o || !out_d || n <= 0) return NEFES_E_BADARG;
    hipLaunchKernelGGL(ndc_fwd_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, H, W, focal, near, n, rays_o,
                       rays_d, out_o, out_d);
    return (int)hipGetLastError();
}
extern "C" int nefes_ndc_bwd(int H, int W, float focal, float near, int n, const float* rays_o, const float* rays_d,
                             const float* g_out_o, const float* g_out_d, float* g_rays_o, float* g_rays_d, void* stream) {
    if (!rays_o || !rays_d || !g_rays_o || !g_rays_d || n <= 0) return NEFES_E_BADARG;
    hipLaunchKernelGGL(ndc_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, H, W, focal, near, n, rays_o,
                       rays_d, g_out_o, g_out_d, g_rays_o, g_rays_d);
    return (int)hipGetLastError();
}

// ---- coarse depths (rendering.py:96-112) ---------------------------------------------------------
// bounds != null: near/far are read per ray from bounds[ray*stride + 0/1] (the [n,21] ray batch of rendering.py:227-235,
// columns 6:8), as render_rays does (:90-100); otherwise the scalars apply to every ray.
__global__ __launch_bounds__(256) void coarse_depths_kernel(int N, int Nc, float near, float far, const float* __restrict__ bounds,
                                                            int stride, int lindisp, const float* __restrict__ t,
                                                            const float* t_rand, float* z) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)N * Nc) return;
    const int k = (int)(i % Nc);
    if (bounds) {
        const size_t ray = i / Nc;
        near = bounds[ray * stride];
        far = bounds[ray * stride + 1];
    }
    auto zk = [&](int kk) {
        const float tt = t[kk];
        if (!lindisp) return __fadd_rn(__fmul_rn(near, __fsub_rn(1.f, tt)), __fmul_rn(far, tt));
        return __fdiv_rn(1.f, __fadd_rn(__fmul_rn(__fdiv_rn(1.f, near), __fsub_rn(1.f, tt)), __fmul_rn(__fdiv_rn(1.f, far), tt)));
    };
    float v = zk(k);
    if (t_rand) {   // stratified jitter inside [lower, upper] (:104-112)
        const float lo = k == 0 ? v : __fmul_rn(.5f, __fadd_rn(v, zk(k - 1)));
        const float hi = k == Nc - 1 ? v : __fmul_rn(.5f, __fadd_rn(zk(k + 1), v));
        v = __fadd_rn(lo, __fmul_rn(__fsub_rn(hi, lo), t_rand[i]));
    }
    z[i] = v;
}
extern "C" int nefes_coarse_depths(int N, int Nc, float near, float far, int lindisp, const float* t, const float* t_rand,
                                   float* z, void* stream) {
    if (!t || !z || N <= 0 || Nc <= 0) return NEFES_E_BADARG;
    const size_t n = (size_t)N * Nc;
    hipLaunchKernelGGL(coarse_depths_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, N, Nc, near,
                       far, (const float*)nullptr, 0, lindisp, t, t_rand, z);
    return (int)hipGetLastError();
}
extern "C" int nefes_coarse_depths_rays(int N, int Nc, const float* bounds, int stride, int lindisp, const float* t,
                                        const float* t_rand, float* z, void* stream) {
    if (!t || !z || !bounds || stride < 2 || N <= 0 || Nc <= 0) return NEFES_E_BADARG;
    const size_t n = (size_t)N * Nc;
    hipLaunchKernelGGL(coarse_depths_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, N, Nc, 0.f,
                       0.f, bounds, stride, lindisp, t, t_rand, z);
    return (int)hipGetLastError();
}

// ---- per-ray reduction of the field backward (autograd of pts = o + d*z, rendering.py:142) ----------
__global__ __launch_bounds__(256) void ray_grad_reduce_kernel(int N, int S, const float* __restrict__ z,
                                                              const float* __restrict__ g_pts, const float* __restrict__ g_vs,
                                                              float* g_o, float* g_d, float* g_v) {
    const int lane = threadIdx.x & 63;
    const int ray = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (ray >= N) return;
    const float* gp = g_pts + (size_t)ray * S * 3;
    const float* gv = g_vs ? g_vs + (size_t)ray * S * 3 : nullptr;
    const float* zr = z + (size_t)ray * S;
    double so[3] = {0, 0, 0}, sd[3] = {0, 0, 0}, sv[3] = {0, 0, 0};
    for (int i = lane; i < 3 * S; i += 64) {
        const int s = i / 3, c = i - 3 * s;
        const float g = gp[i];
        const double gz = (double)(g * zr[s]);
        const float v = gv ? gv[i] : 0.f;
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (c == k) { so[k] += g; sd[k] += gz; sv[k] += v; }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double a = wave_sum(so[k]), b = wave_sum(sd[k]), c = wave_sum(sv[k]);
        if (lane == 0) {
            g_o[(size_t)ray * 3 + k] = (float)a;
            g_d[(size_t)ray * 3 + k] = (float)b;
            if (g_v) g_v[(size_t)ray * 3 + k] = (float)c;
        }
    }
}
extern "C" int nefes_ray_grad_reduce(int N, int S, const float* z, const float* g_pts, const float* g_viewdirs_s,
                                     float* g_rays_o, float* g_rays_d, float* g_viewdirs, void* stream) {
    if (!z || !g_pts || !g_rays_o || !g_rays_d || N <= 0 || S <= 0) return NEFES_E_BADARG;
    hipLaunchKernelGGL(ray_grad_reduce_kernel, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, N, S, z, g_pts,
                       g_viewdirs_s, g_rays_o, g_rays_d, g_viewdirs);
    return (int)hipGetLastError();
}

// Multiresolution hash-grid positional encoding (BASELINE config 4) and its backward to x.
// The reference only configures this encoding (script/models/nerfh_tcnn.py:60-75, input normalisation :151-156);
// the arithmetic is tiny-cuda-nn's published algorithm, restated in oracle/hashgrid_ref.py (PARITY UNPINNED:
// tiny-cuda-nn is neither vendored nor version-pinned by the reference, and the model is orphaned there).
//
// Roofline: gather-bound.  Per sample: 16 levels x 8 corners x 8 B (fp32 x2) = 1 KiB of table reads, 12 B in, 128 B out.
// The 48.8 MB table stays in the 256 MiB Infinity Cache.  One thread per (sample, level): a wave covers 4 samples,
// writes 512 contiguous bytes, and the backward reduces the 16 levels of a sample with 4 xor-shuffles.
#include <stdlib.h>

#include "hashgrid.h"

__global__ __launch_bounds__(256) void hashgrid_fwd_kernel(HgGeom g, const float2* __restrict__ table, long long M,
                                                           const float* __restrict__ x, float2* __restrict__ enc) {
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long m = tid / g.n_levels;
    const int l = (int)(tid - m * g.n_levels);
    if (m >= M) return;
    const HgLevel L = g.lv[l];
    const float xs[3] = {x[m * 3 + 0], x[m * 3 + 1], x[m * 3 + 2]};
    const float2 acc = hg_level_fwd(L, g.bound, table, xs);
    // the embedding is written once and read once by the field kernel: a non-temporal store, so that 10 GB of output per fine pass
    // do not push the table (the data with reuse: 67 MB, four times the L2s) out of the caches on its way
    __builtin_nontemporal_store(acc.x, &enc[tid].x);     // enc[m][2l .. 2l+1]
    __builtin_nontemporal_store(acc.y, &enc[tid].y);
}

__global__ __launch_bounds__(256) void hashgrid_bwd_x_kernel(HgGeom g, const float2* __restrict__ table, long long M,
                                                             const float* __restrict__ x, const float2* __restrict__ g_enc,
                                                             float* __restrict__ g_x) {
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x;
    long long m = tid / 16;                 // 16 lanes per sample (levels beyond n_levels contribute zero)
    const int l = (int)(tid & 15);
    const bool live = m < M && l < g.n_levels;
    if (m >= M) m = M - 1;
    float gx[3] = {0.f, 0.f, 0.f};
    if (live) {
        const HgLevel L = g.lv[l];
        const float xs[3] = {x[m * 3 + 0], x[m * 3 + 1], x[m * 3 + 2]};
        const float* gep = (const float*)&g_enc[m * g.n_levels + l];                       // (read once: non-temporal)
        const float2 ge = make_float2(__builtin_nontemporal_load(gep), __builtin_nontemporal_load(gep + 1));
        hg_level_bwd_x(L, g.bound, g.inv_range, table, xs, ge, gx);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) gx[k] += __shfl_xor(gx[k], o);
    if (l == 0 && tid / 16 < M) {
        g_x[m * 3 + 0] = gx[0]; g_x[m * 3 + 1] = gx[1]; g_x[m * 3 + 2] = gx[2];
    }
}

extern "C" size_t nefes_hashgrid_table_entries(const NefesHashGridDesc* desc) {
    HgGeom g;
    uint64_t total = 0;
    if (hg_geometry(desc, &g, &total)) return 0;
    return (size_t)total;
}

extern "C" int nefes_hashgrid_fwd(const NefesHashGridDesc* desc, const float* table, int64_t M, const float* x, float* enc,
                                  void* stream) {
    if (!table || !x || !enc || M <= 0) return NEFES_E_BADARG;
    HgGeom g;
    int rc = hg_geometry(desc, &g, nullptr);
    if (rc) return rc;
    const long long n = (long long)M * g.n_levels;
    hipLaunchKernelGGL(hashgrid_fwd_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g,
                       (const float2*)table, (long long)M, x, (float2*)enc);
    return (int)hipGetLastError();
}

extern "C" int nefes_hashgrid_bwd_x(const NefesHashGridDesc* desc, const float* table, int64_t M, const float* x,
                                    const float* g_enc, float* g_x, void* stream) {
    if (!table || !x || !g_enc || !g_x || M <= 0) return NEFES_E_BADARG;
    HgGeom g;
    int rc = hg_geometry(desc, &g, nullptr);
    if (rc) return rc;
    const long long n = (long long)M * 16;
    hipLaunchKernelGGL(hashgrid_bwd_x_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g,
                       (const float2*)table, (long long)M, x, (const float2*)g_enc, g_x);
    return (int)hipGetLastError();
}

// ---- gradient w.r.t. the table (training the grid) -------------------------------------------------------------------------------
// g_table[i] += sum over (sample, level, corner) landing on entry i of w_corner * g_enc[sample][level]: a scatter-add of
// 16 levels x 8 corners x 2 floats = 1 KiB per sample into the 48.8 MB table, with the cell / weight / corner-order / index rules
// of hg_level_fwd (wrapped indices of positions outside the bound included).  No packed half-precision atomics.
//
// Reproducibility.  The atomics run at the memory side, so the ORDER of the adds to one entry is the hardware's.  The dense levels
// (the coarse ones: 331 k entries at the default geometry) are where that matters: consecutive samples of every ray share their
// entries, one entry collects up to ~1e5 terms per step, and fp32 sums of that length in two orders differed by 8e-6 of the
// gradient's max-norm.  Those levels therefore accumulate into an fp64 workspace (global_atomic_add_f64), which is rounded ONCE into
// the fp32 gradient by a flush kernel: two launches then agree to the last fp32 bit except where an fp64 sum sits within ~1e-16 of a
// rounding boundary.  The hashed levels (few terms per entry: collisions of unrelated samples) add in fp32 directly; their reordering
// moves an entry by an ulp of itself.  Reproducible to rounding, not bitwise.
//
// Two scatter forms (nefes_hashgrid_bwd_table; NEFES_HG_TABLE_ATOMIC=1 selects the first, for A/B runs and as the correctness baseline):
//   plain  : one thread per (sample, level) as hashgrid_fwd_kernel, one atomic per feature per corner -- the 64 lanes of a wave
//            add to 64 unrelated rows (4 samples x 16 levels);
//   merged : one lane per sample, one level per wave pass (lanes = 64 consecutive samples, i.e. a third of a 192-sample ray).  Along
//            a ray the samples are sorted by depth, so runs of consecutive lanes share a corner entry: a segmented scan across the
//            lanes of each run (ballot of the run heads, then shuffles that never cross a run's first lane) leaves the run's sum in
//            its last lane, and only that lane issues the atomic.  A wave whose 64 entries are all distinct skips the scan.
__device__ __forceinline__ float hg_corner_weight(const float (&w)[3], int corner) {
    const int dx = corner & 1, dy = (corner >> 1) & 1, dz = corner >> 2;
    return (dx ? w[0] : 1.f - w[0]) * (dy ? w[1] : 1.f - w[1]) * (dz ? w[2] : 1.f - w[2]);     // (hg_level_fwd's product order)
}

// entry i's two sums: the fp64 workspace for the dense levels (entries [0, n_dense) of the table), the fp32 gradient otherwise
__device__ __forceinline__ void hg_table_add(float* __restrict__ g_table, double* __restrict__ dense, uint32_t n_dense, uint32_t i,
                                             float vx, float vy) {
    if (i < n_dense) {
        unsafeAtomicAdd(&dense[2 * (size_t)i], (double)vx);
        unsafeAtomicAdd(&dense[2 * (size_t)i + 1], (double)vy);
    } else {
        unsafeAtomicAdd(&g_table[2 * (size_t)i], vx);
        unsafeAtomicAdd(&g_table[2 * (size_t)i + 1], vy);
    }
}

__global__ __launch_bounds__(256) void hashgrid_bwd_table_atomic_kernel(HgGeom g, long long M, const float* __restrict__ x,
                                                                        const float2* __restrict__ g_enc, float* __restrict__ g_table,
                                                                        double* __restrict__ dense, uint32_t n_dense) {
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long m = tid / g.n_levels;
    const int l = (int)(tid - m * g.n_levels);
    if (m >= M) return;
    const HgLevel L = g.lv[l];
    const float xs[3] = {x[m * 3 + 0], x[m * 3 + 1], x[m * 3 + 2]};
    const float2 ge = g_enc[tid];                        // enc[m][2l .. 2l+1]
    float w[3];
    uint32_t c[3];
    hg_cell(L, g.bound, xs, c, w);
#pragma unroll
    for (int corner = 0; corner < 8; ++corner) {
        const uint32_t i = hg_index(L, c[0] + (corner & 1), c[1] + ((corner >> 1) & 1), c[2] + (corner >> 2));
        const float wc = hg_corner_weight(w, corner);
        hg_table_add(g_table, dense, n_dense, i, wc * ge.x, wc * ge.y);
    }
}

// merged form: a workgroup = 64 consecutive samples (one per lane) x all levels, wave w takes levels w, w + 4, w + 8, w + 12 -- the
// block's 8 KiB of g_enc is read by its four waves out of the same lines
__global__ __launch_bounds__(256) void hashgrid_bwd_table_merged_kernel(HgGeom g, long long M, const float* __restrict__ x,
                                                                        const float2* __restrict__ g_enc, float* __restrict__ g_table,
                                                                        double* __restrict__ dense, uint32_t n_dense) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const long long m_raw = (long long)blockIdx.x * 64 + lane;
    const bool live = m_raw < M;
    const long long m = live ? m_raw : M - 1;
    const float xs[3] = {x[m * 3 + 0], x[m * 3 + 1], x[m * 3 + 2]};
    const uint64_t below = (lane == 63) ? ~0ull : ((2ull << lane) - 1ull);     // lanes 0 .. lane
#pragma unroll 1
    for (int l = wave; l < g.n_levels; l += 4) {
        const HgLevel L = g.lv[l];
        float2 ge = g_enc[m * g.n_levels + l];
        if (!live) ge = make_float2(0.f, 0.f);
        float w[3];
        uint32_t c[3];
        hg_cell(L, g.bound, xs, c, w);
#pragma unroll
        for (int corner = 0; corner < 8; ++corner) {
            const uint32_t i = hg_index(L, c[0] + (corner & 1), c[1] + ((corner >> 1) & 1), c[2] + (corner >> 2));
            const float wc = hg_corner_weight(w, corner);
            float vx = wc * ge.x, vy = wc * ge.y;
            // run heads: lane 0 and every lane whose entry differs from the previous lane's (dead lanes repeat sample M-1 with a
            // zero gradient and merge into its run)
            const uint32_t prev = (uint32_t)__shfl_up((int)i, 1);
            const uint64_t heads = __ballot(lane == 0 || prev != i);
            bool tail = true;
            if (heads != ~0ull) {
                const int start = 63 - __builtin_clzll(heads & below);            // first lane of my run
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const float ux = __shfl_up(vx, off), uy = __shfl_up(vy, off);
                    if (lane - off >= start) { vx += ux; vy += uy; }
                }
                tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
            }
            if (tail) hg_table_add(g_table, dense, n_dense, i, vx, vy);
        }
    }
}

// g_table[j] += (float)dense[j] over the dense levels' 2 n_dense floats: each entry rounded once
__global__ __launch_bounds__(256) void hashgrid_bwd_table_flush_kernel(long long n, const double* __restrict__ dense,
                                                                       float* __restrict__ g_table) {
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j < n) g_table[j] += (float)dense[j];
}

// entries of the dense levels: a prefix of the table (the resolution grows with the level, so once res^3 exceeds the hash-map size
// every later level is hashed)
static uint32_t hg_dense_entries(const HgGeom& g) {
    uint32_t n = 0;
    for (int l = 0; l < g.n_levels && !g.lv[l].hashed; ++l) n = g.lv[l].offset + g.lv[l].entries;
    return n;
}

extern "C" size_t nefes_hashgrid_bwd_table_workspace(const NefesHashGridDesc* desc) {
    HgGeom g;
    if (hg_geometry(desc, &g, nullptr)) return 0;
    return (size_t)hg_dense_entries(g) * 2 * sizeof(double);
}

extern "C" int nefes_hashgrid_bwd_table(const NefesHashGridDesc* desc, int64_t M, const float* x, const float* g_enc, float* g_table,
                                        void* workspace, void* stream) {
    if (!x || !g_enc || !g_table || M <= 0) return NEFES_E_BADARG;
    HgGeom g;
    int rc = hg_geometry(desc, &g, nullptr);
    if (rc) return rc;
    const uint32_t n_dense = hg_dense_entries(g);
    if (n_dense && !workspace) return NEFES_E_BADARG;
    double* dense = (double*)workspace;
    hipStream_t st = (hipStream_t)stream;
    if (n_dense) {
        hipError_t e = hipMemsetAsync(dense, 0, (size_t)n_dense * 2 * sizeof(double), st);
        if (e != hipSuccess) return (int)e;
    }
    const char* form = getenv("NEFES_HG_TABLE_ATOMIC");
    if (form && form[0] == '1') {
        const long long n = (long long)M * g.n_levels;
        hipLaunchKernelGGL(hashgrid_bwd_table_atomic_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, g, (long long)M, x,
                           (const float2*)g_enc, g_table, dense, n_dense);
    } else {
        hipLaunchKernelGGL(hashgrid_bwd_table_merged_kernel, dim3((unsigned)((M + 63) / 64)), dim3(256), 0, st, g, (long long)M, x,
                           (const float2*)g_enc, g_table, dense, n_dense);
    }
    if (n_dense) {
        const long long n = (long long)n_dense * 2;
        hipLaunchKernelGGL(hashgrid_bwd_table_flush_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, (const double*)dense,
                           g_table);
    }
    return (int)hipGetLastError();
}

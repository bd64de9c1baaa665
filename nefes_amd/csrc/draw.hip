// Device-side draw of K distinct pixels per image, uniform among the valid pixels of a mask (nefes_draw_pixels): the batch of a
// sparse refinement iteration or of a training step, without np.random.choice / torch.nonzero on the host (run_nefes.py:47-62).
//
// Contract (include/nefes_hip.h; tests/draw_ref.py restates it in numpy): pixel i = y*W + x of image b has the 64-bit sort key
// (o0 << 32) | o1 of Philox-4x32-10 at counter (i, b, epoch lo, epoch hi), key (seed lo, seed hi), epoch = tick / period with
// {seed, tick} READ FROM DEVICE MEMORY when the kernels run; the draw is the K valid pixels with the smallest (key, i), written in
// ascending i.  A function of (seed, epoch, b, mask[b]) alone: what the atomics below decide is the ORDER in which a histogram bin
// is counted and a candidate is appended, and both are consumed as sets.
//
// Four launches, ordered by the stream; no block reads what another block of the SAME launch wrote:
//   zero   histograms and candidate counters of this call;
//   hash   grid (chunks of 2048 pixels, images): the keys [B, n] and, per image, a histogram of the valid keys' top 12 bits (LDS
//          histogram per block, its non-empty bins added to the image's).  The only reader of `state`;
//   mark   same grid: every block finds, from the image's histogram, want = min(K, n_valid) and the bin T that holds the want-th
//          smallest key (K << n: keys are uniform, T is one of the first bins); valid pixels of bins below T are in the draw -- one
//          64-bit ballot per wave is one word of the image's bitmap -- and those of bin T are appended to the candidate list
//          (about n_valid / 4096 of them);
//   write  one block per image: ranks the candidates by (key, i), sets the bits of the first want - (pixels below T), then turns the
//          bitmap into the list: a popcount per thread over its run of words, a block scan, the pixels in ascending order.  Fewer than
//          K valid pixels: want = n_valid selects them all, and the rows behind repeat them cyclically; none: rows of (0, 0).
//          Thread 0 of block 0 advances the tick: every key was formed two launches earlier.
#include "../../include/nefes_hip.h"
#include <hip/hip_runtime.h>

namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr int kThreads = 256;
constexpr int kChunk = kThreads * 8;       // pixels per block of the hash and mark kernels
constexpr int kBins = 4096;                // histogram of the keys' top 12 bits: 16 KiB of LDS
constexpr int kBinShift = 52;

// Philox-4x32-10 (Salmon et al., SC'11): the first two output words as one 64-bit key
__device__ __forceinline__ u64 philox_key(u32 c0, u32 c1, u32 c2, u32 c3, u32 k0, u32 k1) {
    constexpr u32 M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const u32 hi0 = __umulhi(M0, c0), lo0 = M0 * c0, hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += W0;
        k1 += W1;
    }
    return ((u64)c0 << 32) | c1;
}

// the workspace of one call: all of it is written by the call before it is read
struct DrawWs {
    u64* keys;      // [B, n]
    u64* bitmap;    // [B, ceil(n / 64)]: bit i = pixel i is in the draw
    u32* hist;      // [B, kBins], then n_cand [B]: zeroed together
    u32* n_cand;
    u32* cand;      // [B, n]: indices of the pixels of bin T, in order of arrival (capacity n: a pixel is appended once)
};
struct DrawLayout {
    size_t keys, bitmap, hist, cand, total, zero_words;
};
__host__ DrawLayout draw_layout(int B, int H, int W) {
    const size_t n = (size_t)H * W, nw = (n + 63) / 64, b = (size_t)B;
    DrawLayout l;
    l.keys = 0;
    l.bitmap = l.keys + b * n * 8;
    l.hist = l.bitmap + b * nw * 8;
    l.zero_words = (b * (kBins + 1) + 3) / 4 * 4;
    l.cand = l.hist + l.zero_words * 4;
    l.total = l.cand + b * n * 4;
    return l;
}

__global__ __launch_bounds__(kThreads) void draw_zero_kernel(u32* words, size_t count) {
    const size_t t = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (t < count) words[t] = 0u;
}

__global__ __launch_bounds__(kThreads) void draw_hash_kernel(int B, int n, const uint8_t* __restrict__ mask, int period,
                                                             const u64* state, DrawWs ws) {
    __shared__ u32 bins[kBins];
    const u64 seed = state[0], epoch = state[1] / (u64)period;
    const u32 k0 = (u32)seed, k1 = (u32)(seed >> 32), e0 = (u32)epoch, e1 = (u32)(epoch >> 32);
    const int base = blockIdx.x * kChunk;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        for (int k = threadIdx.x; k < kBins; k += kThreads) bins[k] = 0u;
        __syncthreads();
        const size_t img = (size_t)b * n;
#pragma unroll
        for (int j = 0; j < kChunk / kThreads; ++j) {
            const int i = base + j * kThreads + threadIdx.x;
            if (i < n) {
                const u64 key = philox_key((u32)i, (u32)b, e0, e1, k0, k1);
                ws.keys[img + i] = key;
                if (!mask || mask[img + i] != 0) atomicAdd(&bins[(u32)(key >> kBinShift)], 1u);
            }
        }
        __syncthreads();
        for (int k = threadIdx.x; k < kBins; k += kThreads) {
            const u32 c = bins[k];
            if (c) atomicAdd(&ws.hist[(size_t)b * kBins + k], c);
        }
        __syncthreads();
    }
}

// inclusive scan of one value per thread over the block's 256 threads; `total` on every thread.  sh: 4 words.
__device__ __forceinline__ u32 block_incl_scan(u32 v, u32* sh, u32& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u32 u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    __syncthreads();                       // (sh may still be read from the previous use)
    if (lane == 63) sh[wave] = v;
    __syncthreads();
    u32 before = 0u;
    for (int w = 0; w < wave; ++w) before += sh[w];
    total = (sh[0] + sh[1]) + (sh[2] + sh[3]);
    return v + before;
}

// What an image's histogram says about its draw: n_valid; want = min(K, n_valid) pixels to select; the bin T of the want-th smallest
// key; take = how many of bin T's m pixels belong to the draw (1 <= take <= m; every pixel of a bin below T does).  want = 0: the
// rest is unset.  Called by all threads of a 256-thread block; sh: 8 words.
struct DrawBin {
    u32 n_valid, want, T, take, m;
};
__device__ __forceinline__ DrawBin draw_find_bin(const u32* __restrict__ hist, int K, u32* sh) {
    constexpr int PER = kBins / kThreads;
    u32 c[PER], sum = 0u;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        c[k] = hist[threadIdx.x * PER + k];
        sum += c[k];
    }
    DrawBin r;
    const u32 incl = block_incl_scan(sum, sh, r.n_valid);
    r.want = r.n_valid < (u32)K ? r.n_valid : (u32)K;
    u32 run = incl - sum;
    if (r.want > 0u && run < r.want && r.want <= incl) {       // exactly one thread: incl is non-decreasing over the threads
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            if (run < r.want && r.want <= run + c[k]) {
                sh[4] = threadIdx.x * PER + k;
                sh[5] = r.want - run;
                sh[6] = c[k];
            }
            run += c[k];
        }
    }
    __syncthreads();
    r.T = sh[4];
    r.take = sh[5];
    r.m = sh[6];
    return r;
}

__global__ __launch_bounds__(kThreads) void draw_mark_kernel(int B, int n, const uint8_t* __restrict__ mask, int K, DrawWs ws) {
    __shared__ u32 sh[8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int base = blockIdx.x * kChunk;
    const size_t nw = ((size_t)n + 63) / 64;
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const DrawBin d = draw_find_bin(ws.hist + (size_t)b * kBins, K, sh);
        const size_t img = (size_t)b * n;
#pragma unroll
        for (int j = 0; j < kChunk / kThreads; ++j) {
            const int i = base + j * kThreads + threadIdx.x;
            bool below = false;
            if (i < n && d.want > 0u && (!mask || mask[img + i] != 0)) {
                const u32 bin = (u32)(ws.keys[img + i] >> kBinShift);
                below = bin < d.T;
                if (bin == d.T) ws.cand[img + atomicAdd(&ws.n_cand[b], 1u)] = (u32)i;     // (< m <= n appended per image)
            }
            const u64 word = __ballot(below);                 // the wave's 64 consecutive pixels: one word of the bitmap
            const size_t w = (size_t)(base + j * kThreads) / 64 + wave;
            if (lane == 0 && w < nw) ws.bitmap[(size_t)b * nw + w] = word;
        }
        __syncthreads();                                      // (sh is rewritten for the next image)
    }
}

__global__ __launch_bounds__(kThreads) void draw_write_kernel(int H, int W, int K, DrawWs ws, u64* state, int advance, float* px,
                                                              int32_t* n_valid) {
    __shared__ u32 sh[8];
    __shared__ u64 tile_key[kThreads];
    __shared__ u32 tile_idx[kThreads];
    const int b = blockIdx.x, n = H * W;
    const size_t nw = ((size_t)n + 63) / 64;
    const DrawBin d = draw_find_bin(ws.hist + (size_t)b * kBins, K, sh);
    const u64* keys = ws.keys + (size_t)b * n;
    const u32* cand = ws.cand + (size_t)b * n;
    u64* bitmap = ws.bitmap + (size_t)b * nw;
    if (b == 0 && threadIdx.x == 0 && advance) state[1] = state[1] + 1ull;
    // bin T: candidate c is in the draw iff fewer than `take` candidates precede it in (key, i).  Tiles of 256 candidates in LDS.
    // (m is bin T's count and the number of candidates appended; the smaller of the two, so that a mask written to between the two
    // launches -- the caller's race -- cannot make an index of an entry nobody wrote)
    const u32 m = d.want > 0u ? (d.m < ws.n_cand[b] ? d.m : ws.n_cand[b]) : 0u;
    for (u32 q0 = 0; q0 < m; q0 += kThreads) {
        const u32 c = q0 + threadIdx.x;
        const bool mine = c < m;
        const u32 ic = mine ? cand[c] : 0u;
        const u64 kc = mine ? keys[ic] : 0ull;
        u32 rank = 0u;
        for (u32 t0 = 0; t0 < m; t0 += kThreads) {
            __syncthreads();
            const u32 e = t0 + threadIdx.x;
            const u32 ie = e < m ? cand[e] : 0xffffffffu;
            tile_idx[threadIdx.x] = ie;
            tile_key[threadIdx.x] = e < m ? keys[ie] : ~0ull;          // (never precedes a candidate: its index is larger)
            __syncthreads();
            const u32 cnt = m - t0 < (u32)kThreads ? m - t0 : (u32)kThreads;
            for (u32 k = 0; k < cnt; ++k) {
                const u64 k2 = tile_key[k];
                rank += (k2 < kc || (k2 == kc && tile_idx[k] < ic)) ? 1u : 0u;
            }
        }
        if (mine && rank < d.take) atomicOr(&bitmap[ic >> 6], 1ull << (ic & 63u));
    }
    __syncthreads();
    // the bitmap as a list: thread t owns words [w0, w1).  Its words are read as device-scope atomic loads: some were just updated
    // by this block's atomics, which do not pass through the L1 a plain load may hit.
    const size_t per = (nw + kThreads - 1) / kThreads;
    const size_t w0 = threadIdx.x * per < nw ? threadIdx.x * per : nw, w1 = w0 + per < nw ? w0 + per : nw;
    u32 count = 0u;
    for (size_t w = w0; w < w1; ++w) count += (u32)__popcll(__hip_atomic_load(&bitmap[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    u32 total;
    u32 at = block_incl_scan(count, sh, total) - count;       // total == want
    float* out = px + (size_t)b * K * 2;
    for (size_t w = w0; w < w1; ++w) {
        u64 word = __hip_atomic_load(&bitmap[w], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        while (word && at < (u32)K) {                         // (at < K always: total = want <= K; the bound guards the store)
            const int i = (int)(w * 64) + (__ffsll((long long)word) - 1);
            word &= word - 1;
            out[(size_t)at * 2] = (float)(i % W);
            out[(size_t)at * 2 + 1] = (float)(i / W);
            ++at;
        }
    }
    __syncthreads();
    // fewer than K valid pixels: rows want.. repeat rows 0..want-1 cyclically; none: (0, 0)
    for (u32 j = d.want + threadIdx.x; j < (u32)K; j += kThreads) {
        const u32 src = d.want ? j % d.want : 0u;
        out[(size_t)j * 2] = d.want ? out[(size_t)src * 2] : 0.f;
        out[(size_t)j * 2 + 1] = d.want ? out[(size_t)src * 2 + 1] : 0.f;
    }
    if (n_valid && threadIdx.x == 0) n_valid[b] = (int32_t)d.n_valid;
}

bool draw_bad_shape(int B, int H, int W) { return B <= 0 || H <= 0 || W <= 0 || (long long)H * W > (1ll << 24); }

}   // namespace

extern "C" size_t nefes_draw_pixels_workspace(int B, int H, int W) {
    if (draw_bad_shape(B, H, W)) return 0;
    return draw_layout(B, H, W).total;
}

extern "C" int nefes_draw_pixels(int B, int H, int W, const uint8_t* mask, int K, int period, uint64_t* state, int advance, float* px,
                                 int32_t* n_valid, void* workspace, void* stream) {
    if (draw_bad_shape(B, H, W) || K <= 0 || period <= 0 || (long long)K > (long long)H * W || !state || !px || !workspace)
        return NEFES_E_BADARG;
    const int n = H * W;
    const DrawLayout l = draw_layout(B, H, W);
    char* p = (char*)workspace;
    DrawWs ws;
    ws.keys = (u64*)(p + l.keys);
    ws.bitmap = (u64*)(p + l.bitmap);
    ws.hist = (u32*)(p + l.hist);
    ws.n_cand = ws.hist + (size_t)B * kBins;
    ws.cand = (u32*)(p + l.cand);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((n + kChunk - 1) / kChunk), (unsigned)(B < 65535 ? B : 65535));
    draw_zero_kernel<<<dim3((unsigned)((l.zero_words + kThreads - 1) / kThreads)), dim3(kThreads), 0, st>>>(ws.hist, l.zero_words);
    draw_hash_kernel<<<grid, dim3(kThreads), 0, st>>>(B, n, mask, period, (const u64*)state, ws);
    draw_mark_kernel<<<grid, dim3(kThreads), 0, st>>>(B, n, mask, K, ws);
    draw_write_kernel<<<dim3((unsigned)B), dim3(kThreads), 0, st>>>(H, W, K, ws, (u64*)state, advance, px, n_valid);
    return (int)hipGetLastError();
}

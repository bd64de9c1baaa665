// Generic field kernels: NeRFH_NFF of ANY width (multiple of 32, 32..512) and depth (1..8, optional skip layer) as run-time
// arguments -- script/models/nerfh_nff.py:452-478,525-576 with --netwidth / --netdepth free.  Not tuned: strict fp32 on
// v_mfma_f32_32x32x2_f32 through the compiler builtin, no asm schedule, no split products, no scale tables.  A network the tuned
// instances serve (field_fwd_h3.hip ...) never comes here unless the caller asks (NEFES_FIELD_GENERIC=1, nefes_amd/ops.py).
//
// One workgroup of four waves per tile of TS = 64 samples (32 above width 256: LDS).  Activations live in LDS as [feature][sample]
// and ping-pong between two buffers; the embeddings have regions of their own, so the skip layer and the heads read two K-segments
// instead of a concatenation.  A product is D[feature][sample] += W[feature][k] act[k][sample]: wave w owns the 32-feature row blocks
// w, w + 4, ... and both 32-sample column blocks, so one A fragment (weights, from global / L2) feeds two MFMAs.
//
// Weight blob (nefes_generic_pack): per layer the matrix TWICE in plain fp32 -- wt[Kp][Mp] (k-major: the forward's A fragment is
// two 128-byte rows) and wb[Mp][Kp] (m-major: the same for the transposed product of the backward) -- and bias[Mp].  Mp = outputs
// rounded up to 32 (zero rows), Kp = the layer's input with each embedding padded to its LDS region (63 -> 64, 27 -> 32; zero
// columns).  Layers: L1..LD, FINAL, SIGMA, DIR, RGB (rgb + features) [, T0, T1, T2, TH = transient rgb(3) | sigma | beta].
//
// ReLU masks: one word per (tile, hidden layer, row block, lane): bit 16 c + r = accumulator r of column block c was > 0.  The
// backward's transposed product leaves the gradient of a layer's output in exactly the accumulator that produced it, so it tests the
// same bit -- no recomputation of the forward (which would double the backward's matrix work) and 1 bit per activation of traffic.
//
// One kernel template per direction, gen_fwd_kernel<NCB, Args> / gen_bwd_kernel<NCB, Args>: NCB = TS / 32, Args = one of four
// argument structs whose two constants select what the body compiles in (eight entry points, sixteen instances):
//   GenArgs          nefes_field_{fwd,bwd}_generic             the frequency embedding of the position, inference
//   GenArgsExt       nefes_field_{fwd,bwd}_generic_ext         ext
//   GenArgsTrain     nefes_field_{fwd,bwd}_train_generic       train
//   GenArgsExtTrain  nefes_field_{fwd,bwd}_train_generic_ext   ext and train
// ext (NEFES_XYZ_EXTERNAL32): the E region is the caller's 32 features per sample (a hash grid's, gathered by the launches of
// hashgrid.hip) instead of the 63-feature frequency embedding: 32 rows, no padding row, Kp = 32 for layer 1 and 32 + W for the skip
// layer; the backward stores d loss / d encoding where the other instances apply the embedding's chain rule (gen_embed's overload,
// gen_input_grads_ext).
// train: the kernels also copy, from the LDS buffers they sit in anyway, every weight-gradient operand to the train-layout buffers
// of csrc/train.hip (layout.h nefes_train_off): the forward the embeddings and every hidden layer's OUTPUT (after ReLU) to `acts`,
// the backward the gradient with respect to every layer's pre-activation to `dacts`.  nefes_train_dw_bias then forms dW = G X^T
// unchanged; the block -> first-row map is gen_train_map (nefes_generic_train_row_offset).  With ext the E block of `acts` is the
// caller's 32 features in natural order, so every later block starts 32 rows earlier (nefes_generic_train_row_offset_ext).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nefes_hip.h"
#include "layout.h"

#include <string.h>

#define GEN_MAX_LAYERS 16
#define GEN_E_ROWS 64      /* xyz embedding: 63 features + a zero row */
#define GEN_X_ROWS 32      /* ... of a NEFES_XYZ_EXTERNAL32 network: the supplied features, unpadded */
#define GEN_DV_ROWS 32     /* direction embedding: 27 features + zero rows */
#define GEN_HEAD_ROWS 160  /* rgb + features: 3 + 141 rounded up to 32 */

typedef float f32x16 __attribute__((ext_vector_type(16)));

// torch.nn.Softplus(beta=1, threshold=20), torch.sigmoid
__device__ __forceinline__ float softplus_ref(float x) { return x > 20.f ? x : log1pf(expf(x)); }
__device__ __forceinline__ float sigmoid_ref(float x) { return 1.f / (1.f + expf(-x)); }
__device__ __forceinline__ float mul_rn(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float add_rn(float a, float b) { return __fadd_rn(a, b); }

// sin / cos of x 2^k as the tuned kernels evaluate them (field_common.h: exact argument reduction in turns, one odd polynomial on
// [-1/4, 1/4] turns, 1.7e-7 absolute): t = x / (2 pi) in f64, its fraction as 64-bit fixed point hi.lo, frac(t 2^k) = a shift.
__device__ __forceinline__ void turns_fixed(float x, uint32_t& hi, uint32_t& lo) {
    const double t = (double)x * 0.15915494309189533577;
    const double s = (t - __builtin_floor(t)) * 4294967296.0;
    hi = (uint32_t)s;
    lo = (uint32_t)((s - (double)hi) * 4294967296.0);
}
__device__ __forceinline__ float sin_phase(uint32_t top) {         // sin(2 pi top / 2^32)
    const float r = (float)(int32_t)top * 2.3283064365386963e-10f;
    const float a = fabsf(r);
    const float rr = __builtin_copysignf(fminf(a, 0.5f - a), r);
    const float z = rr * rr;
    float p = 39.53672409057617f;
    p = __builtin_fmaf(p, z, -76.5497817993164f);
    p = __builtin_fmaf(p, z, 81.60100555419922f);
    p = __builtin_fmaf(p, z, -41.34165573120117f);
    p = __builtin_fmaf(p, z, 6.283185005187988f);
    return rr * p;
}
__device__ __forceinline__ uint32_t phase_of(uint32_t hi, uint32_t lo, int k) {   // top 32 bits of frac(t 2^k), k < 32
    return k ? (hi << k) | (lo >> (32 - k)) : hi;
}

struct GenLayer {
    int M, Mp, Kp;
    long long wt, wb, bias;      // float offsets into the blob
};
struct GenLayout {
    int W, D, skip, C, fine;
    int n_layers;
    int iFINAL, iSIGMA, iDIR, iRGB, iT0, iT1, iT2, iTH;
    GenLayer L[GEN_MAX_LAYERS];
    long long total_floats;
    int mask_words;              // words per lane and tile
    int slot_off[12];            // first row block of hidden layer slot (L1..LD, DIR, T0, T1, T2) in a tile's mask words
    int e_rows;                  // rows of the E region: GEN_E_ROWS or GEN_X_ROWS (host side only; it sits in the struct's tail padding)
};

static bool gen_desc_ok(const NefesGenericNetDesc* d) {
    if (!d) return false;
    if (d->width < 32 || d->width > 512 || d->width % 32) return false;
    if (d->depth < 1 || d->depth > 8) return false;
    if (d->skip != -1 && (d->skip < 1 || d->skip >= d->depth)) return false;
    if (d->feat_dim < 1 || d->feat_dim > 141) return false;
    if (d->xyz_encoding != NEFES_XYZ_FREQ10 && d->xyz_encoding != NEFES_XYZ_EXTERNAL32) return false;
    return d->has_transient == 0 || d->has_transient == 1;
}

static int gen_layout(const NefesGenericNetDesc* d, GenLayout* g) {
    if (!gen_desc_ok(d)) return NEFES_E_UNSUPPORTED;
    memset(g, 0, sizeof(*g));
    const int W = d->width, D = d->depth, H = W / 2;
    g->W = W; g->D = D; g->skip = d->skip; g->C = d->feat_dim; g->fine = d->has_transient;
    const int ER = g->e_rows = d->xyz_encoding == NEFES_XYZ_EXTERNAL32 ? GEN_X_ROWS : GEN_E_ROWS;
    int n = 0;
    long long off = 0;
    auto add = [&](int M, int Kp) {
        GenLayer& l = g->L[n];
        l.M = M; l.Mp = (M + 31) / 32 * 32; l.Kp = Kp;
        l.wt = off; off += (long long)Kp * l.Mp;
        l.wb = off; off += (long long)Kp * l.Mp;
        l.bias = off; off += l.Mp;
        return n++;
    };
    for (int i = 0; i < D; ++i) add(W, i == 0 ? ER : (i == d->skip ? ER + W : W));
    g->iFINAL = add(W, W);
    g->iSIGMA = add(1, W);
    g->iDIR = add(H, W + GEN_DV_ROWS);
    g->iRGB = add(3 + d->feat_dim, H);
    if (d->has_transient) {
        g->iT0 = add(H, W + GEN_DV_ROWS);
        g->iT1 = add(H, H);
        g->iT2 = add(H, H);
        g->iTH = add(5, H);
    }
    g->n_layers = n;
    g->total_floats = off + 64;          // slack behind the last matrix
    int rb = 0;
    for (int i = 0; i < D; ++i) { g->slot_off[i] = rb; rb += W / 32; }
    for (int i = 0; i < 4; ++i) { g->slot_off[D + i] = rb; rb += (H + 31) / 32; }
    g->mask_words = rb;
    return 0;
}

static int gen_tile(int W) { return W <= 256 ? 64 : 32; }

extern "C" size_t nefes_generic_blob_bytes(const NefesGenericNetDesc* desc) {
    GenLayout g;
    if (gen_layout(desc, &g)) return 0;
    return (size_t)g.total_floats * 4;
}

extern "C" size_t nefes_generic_mask_bytes(const NefesGenericNetDesc* desc, int64_t M) {
    GenLayout g;
    if (M <= 0 || gen_layout(desc, &g)) return 0;
    const int TS = gen_tile(g.W);
    return (size_t)((M + TS - 1) / TS) * g.mask_words * 64 * 4;
}

// The packers' table: tensor pair t (weight, bias; torch layout [rows][src_cols]) fills rows [m0, m0 + rows) of layer li; source
// columns [emb_at, emb_at + emb) are an embedding padded to emb_pad in the kernels' K order, so column c -> k = gen_put_k.
struct GenPut { int li, m0, rows, t, src_cols, emb, emb_at, emb_pad; };
__host__ __device__ static inline int gen_put_k(const GenPut& p, int c) { return c < p.emb_at + p.emb ? c : c + (p.emb_pad - p.emb); }
template <class F>
static void gen_for_each_put(const GenLayout& g, F f) {
    const int W = g.W, D = g.D, H = W / 2;
    const bool ext = g.e_rows == GEN_X_ROWS;      // the supplied encoding: 32 source columns, 32 rows, nothing to pad
    const int e_src = ext ? GEN_X_ROWS : 63, e_emb = ext ? 0 : 63, e_pad = ext ? 0 : GEN_E_ROWS;
    int t = 0;
    for (int i = 0; i < D; ++i, t += 2) {
        if (i == 0) f(GenPut{i, 0, W, t, e_src, e_emb, 0, e_pad});
        else if (i == g.skip) f(GenPut{i, 0, W, t, e_src + W, e_emb, 0, e_pad});
        else f(GenPut{i, 0, W, t, W, 0, 0, 0});
    }
    f(GenPut{g.iFINAL, 0, W, t, W, 0, 0, 0}); t += 2;
    f(GenPut{g.iDIR, 0, H, t, W + 27, 27, W, GEN_DV_ROWS}); t += 2;
    f(GenPut{g.iSIGMA, 0, 1, t, W, 0, 0, 0}); t += 2;
    f(GenPut{g.iRGB, 0, 3 + g.C, t, H, 0, 0, 0}); t += 2;
    if (g.fine) {
        f(GenPut{g.iT0, 0, H, t, W + 27, 27, W, GEN_DV_ROWS}); t += 2;
        f(GenPut{g.iT1, 0, H, t, H, 0, 0, 0}); t += 2;
        f(GenPut{g.iT2, 0, H, t, H, 0, 0, 0}); t += 2;
        f(GenPut{g.iTH, 3, 1, t, H, 0, 0, 0}); t += 2;      // transient sigma
        f(GenPut{g.iTH, 0, 3, t, H, 0, 0, 0}); t += 2;      // transient rgb
        f(GenPut{g.iTH, 4, 1, t, H, 0, 0, 0}); t += 2;      // transient beta
    }
}

// tensors: (weight, bias) per layer: xyz_encoding_1..D, xyz_encoding_final, dir_encoding.0, static_sigma.0, static_rgb.0
// [, transient_encoding.0/.2/.4, transient_sigma.0, transient_rgb.0, transient_beta.0]; torch layout [out, in], embeddings at their
// full 63 / 27 features (NEFES_XYZ_EXTERNAL32: 32 in the place of the 63).
extern "C" int nefes_generic_pack(const NefesGenericNetDesc* desc, const float* const* tensors, int n_tensors, void* blob,
                                  size_t blob_bytes) {
    GenLayout g;
    int rc = gen_layout(desc, &g);
    if (rc) return rc;
    if (!tensors || !blob) return NEFES_E_BADARG;
    if (n_tensors != 2 * (g.D + (g.fine ? 10 : 4)) || blob_bytes < (size_t)g.total_floats * 4) return NEFES_E_BADARG;
    for (int i = 0; i < n_tensors; ++i)
        if (!tensors[i]) return NEFES_E_BADARG;
    float* out = (float*)blob;
    memset(out, 0, (size_t)g.total_floats * 4);
    gen_for_each_put(g, [&](const GenPut& p) {
        const GenLayer& l = g.L[p.li];
        const float *w = tensors[p.t], *b = tensors[p.t + 1];
        for (int m = 0; m < p.rows; ++m) {
            for (int c = 0; c < p.src_cols; ++c) {
                const int k = gen_put_k(p, c);
                const float v = w[(size_t)m * p.src_cols + c];
                out[l.wt + (long long)k * l.Mp + (p.m0 + m)] = v;
                out[l.wb + (long long)(p.m0 + m) * l.Kp + k] = v;
            }
            out[l.bias + p.m0 + m] = b[m];
        }
    });
    return 0;
}

// The same scatter on the device (a trainable network after an optimiser step): one launch per tensor pair, plain stores, the blob's
// padding (zeroed once at allocation) is never touched.
__global__ __launch_bounds__(256) void gen_pack_kernel(float* __restrict__ out, long long wt, long long wb, long long bias, int Mp,
                                                       int Kp, GenPut p, const float* __restrict__ w, const float* __restrict__ b) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.rows * p.src_cols) return;
    const int m = idx / p.src_cols, c = idx - m * p.src_cols;
    const int k = gen_put_k(p, c);
    const float v = w[idx];
    out[wt + (long long)k * Mp + (p.m0 + m)] = v;
    out[wb + (long long)(p.m0 + m) * Kp + k] = v;
    if (c == 0) out[bias + p.m0 + m] = b[m];
}

extern "C" int nefes_generic_pack_device(const NefesGenericNetDesc* desc, const float* const* tensors, int n_tensors, void* blob,
                                         size_t blob_bytes, void* stream) {
    GenLayout g;
    int rc = gen_layout(desc, &g);
    if (rc) return rc;
    if (!tensors || !blob) return NEFES_E_BADARG;
    if (n_tensors != 2 * (g.D + (g.fine ? 10 : 4)) || blob_bytes < (size_t)g.total_floats * 4) return NEFES_E_BADARG;
    for (int i = 0; i < n_tensors; ++i)
        if (!tensors[i]) return NEFES_E_BADARG;
    int err = 0;
    gen_for_each_put(g, [&](const GenPut& p) {
        if (err) return;
        const GenLayer& l = g.L[p.li];
        const int n = p.rows * p.src_cols;
        hipLaunchKernelGGL(gen_pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (float*)blob, l.wt,
                           l.wb, l.bias, l.Mp, l.Kp, p, tensors[p.t], tensors[p.t + 1]);
        err = (int)hipGetLastError();
    });
    return err;
}

// ---- train-mode row map: first row of block NEFES_TB_* (layout.h: E, DV, L1..L8, FINAL, DIR, T0..T2, RGB, SIG, TH, END) in a tile of
// the `acts` / `dacts` buffers of this network.  Blocks the network does not have (layers above its depth, the transient blocks of a
// network without that head) are empty; every block is a multiple of 32 rows.
// The E block is the kernels' E region: GEN_E_ROWS of the frequency embedding, GEN_X_ROWS of a supplied encoding.
struct GenTrainMap { int off[NEFES_TB_END + 1]; };
static int gen_train_map(const NefesGenericNetDesc* d, int xyz_encoding, GenTrainMap* m) {
    if (!gen_desc_ok(d) || d->xyz_encoding != xyz_encoding) return NEFES_E_UNSUPPORTED;      // each entry point serves one encoding
    const int W = d->width, Hp = (W / 2 + 31) / 32 * 32, fine = d->has_transient;
    int r = 0;
    for (int b = 0; b <= NEFES_TB_END; ++b) {
        m->off[b] = r;
        if (b == NEFES_TB_E) r += xyz_encoding == NEFES_XYZ_EXTERNAL32 ? GEN_X_ROWS : GEN_E_ROWS;
        else if (b == NEFES_TB_DV) r += GEN_DV_ROWS;
        else if (b >= NEFES_TB_L1 && b < NEFES_TB_FINAL) r += b - NEFES_TB_L1 < d->depth ? W : 0;
        else if (b == NEFES_TB_FINAL) r += W;
        else if (b == NEFES_TB_DIR) r += Hp;
        else if (b >= NEFES_TB_T0 && b <= NEFES_TB_T2) r += fine ? Hp : 0;
        else if (b == NEFES_TB_RGB) r += (3 + d->feat_dim + 31) / 32 * 32;
        else if (b == NEFES_TB_SIG) r += 32;
        else if (b == NEFES_TB_TH) r += fine ? 32 : 0;
    }
    return 0;
}

static size_t gen_train_rows(const NefesGenericNetDesc* desc, int xyz_encoding) {
    GenTrainMap m;
    return gen_train_map(desc, xyz_encoding, &m) ? 0 : (size_t)m.off[NEFES_TB_END];
}

static int gen_train_row_offset(const NefesGenericNetDesc* desc, int xyz_encoding, int block) {
    GenTrainMap m;
    if (block < 0 || block > NEFES_TB_END) return NEFES_E_BADARG;
    const int rc = gen_train_map(desc, xyz_encoding, &m);
    return rc ? rc : m.off[block];
}

extern "C" size_t nefes_generic_train_rows(const NefesGenericNetDesc* desc) { return gen_train_rows(desc, NEFES_XYZ_FREQ10); }
extern "C" int nefes_generic_train_row_offset(const NefesGenericNetDesc* desc, int block) {
    return gen_train_row_offset(desc, NEFES_XYZ_FREQ10, block);
}
extern "C" size_t nefes_generic_train_rows_ext(const NefesGenericNetDesc* desc) { return gen_train_rows(desc, NEFES_XYZ_EXTERNAL32); }
extern "C" int nefes_generic_train_row_offset_ext(const NefesGenericNetDesc* desc, int block) {
    return gen_train_row_offset(desc, NEFES_XYZ_EXTERNAL32, block);
}

// ---------------------------------------------------------------------------------------------------------------------------
struct GenArgs {
    static constexpr bool train = false;
    static constexpr bool ext = false;
    GenLayout g;
    const float* blob;
    const float *rays_o, *rays_d, *z, *pts, *viewdirs;
    float* raw_t;
    uint32_t* masks;
    const float *raw_in, *g_raw_t;     // backward
    float *g_pts, *g_vs;
    long long M;
    int S, R, mode;
};

__device__ __forceinline__ int gen_rho(int half, int r) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// acc[c] += A(32 x K) B(K x 32 c): a -> this lane's weight column (already at row block + lane % 32, + half * lda), b -> its LDS
// column (already at lane % 32, + half * TS); K a multiple of 8.
template <int NCB>
__device__ __forceinline__ void gen_mma(f32x16 (&acc)[NCB], const float* __restrict__ a, long long lda, const float* b, int K) {
    constexpr int TS = 32 * NCB;
    for (int k0 = 0; k0 < K; k0 += 8) {          // every K here is a multiple of 16: four k-steps per trip, loads ahead of the MFMAs
        float av[4], bv[4][NCB];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            av[u] = a[(long long)(k0 + 2 * u) * lda];
#pragma unroll
            for (int c = 0; c < NCB; ++c) bv[u][c] = b[(k0 + 2 * u) * TS + 32 * c];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int c = 0; c < NCB; ++c) acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[u], bv[u][c], acc[c], 0, 0, 0);
    }
}

// One layer: out rows [0, MB * 32) = bias + seg0 + seg1; w0 / w1 = first k-row of the segment in a [k][ld] matrix whose columns are
// the output rows (forward: wt, ld = Mp; backward: wb + column offset, ld = Kp); n_cols = valid columns (the lane's is clamped).
template <int NCB, class Epi>
__device__ __forceinline__ void gen_layer(const float* __restrict__ w0, const float* in0, int K0, const float* __restrict__ w1,
                                          const float* in1, int K1, long long ld, int n_cols, int MB, const float* __restrict__ bias,
                                          Epi epi) {
    constexpr int TS = 32 * NCB;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, l31 = lane & 31;
    for (int rb = wave; rb < MB; rb += 4) {
        f32x16 acc[NCB];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float bv = bias ? bias[rb * 32 + gen_rho(half, r)] : 0.f;
#pragma unroll
            for (int c = 0; c < NCB; ++c) acc[c][r] = bv;
        }
        int col = rb * 32 + l31;
        col = col < n_cols ? col : n_cols - 1;
        gen_mma<NCB>(acc, w0 + half * ld + col, ld, in0 + half * TS + l31, K0);
        if (K1 > 0) gen_mma<NCB>(acc, w1 + half * ld + col, ld, in1 + half * TS + l31, K1);
        epi(rb, acc);
    }
}

// position of sample m on its ray batch: pts = o + d z as the reference rounds it (rendering.py:114,142), or the caller's point
__device__ __forceinline__ float gen_coord(const GenArgs& a, long long m, int axis) {
    if (m >= a.M) return 0.f;
    if (a.pts) return a.pts[m * 3 + axis];
    const long long n = m / a.S;
    return add_rn(a.rays_o[n * 3 + axis], mul_rn(a.rays_d[n * 3 + axis], a.z[m]));
}

// The direction embedding alone, for the instances on a supplied encoding: the second half of gen_embed and the second half of the
// frequency backward's last loop (gen_dir_grad).  Those two keep their own copies.  Calling these from them gives the same bits
// (same operations, same order, -ffp-contract=off) and the same register counts, but the compiler then lays out all eight backward
// kernels differently from their first instructions on, and their times move: -15 % on the frequency embedding at (256, 8), +19 %
// on a supplied encoding (profiles/generic_one_template/README.md).  Merge them together with a tuning of these kernels, not before.
template <int NCB>
__device__ __forceinline__ void gen_embed_dir(const GenArgs& a, long long m0, float* DV) {
    constexpr int TS = 32 * NCB;
    const int tid = threadIdx.x;
    if (a.viewdirs) {
        for (int i = tid; i < 3 * TS; i += 256) {
            const int s = i % TS, axis = i / TS;
            const long long m = m0 + s;
            const float x = m < a.M ? a.viewdirs[(m / a.S) * 3 + axis] : 0.f;
            uint32_t hi, lo;
            turns_fixed(x, hi, lo);
            DV[axis * TS + s] = x;
            for (int k = 0; k < 4; ++k) {
                const uint32_t ph = phase_of(hi, lo, k);
                DV[(3 + 6 * k + axis) * TS + s] = sin_phase(ph);
                DV[(6 + 6 * k + axis) * TS + s] = sin_phase(ph + 0x40000000u);
            }
        }
        for (int i = tid; i < 5 * TS; i += 256) DV[27 * TS + i] = 0.f;
    }
}

// rows of the frequency embedding in the reference's order (nerfh_nff.py:252-270): x (3), then per octave sin (3), cos (3)
template <int NCB>
__device__ __forceinline__ void gen_embed(const GenArgs& a, long long m0, float* E, float* DV) {
    constexpr int TS = 32 * NCB;
    const int tid = threadIdx.x;
    for (int i = tid; i < 3 * TS; i += 256) {
        const int s = i % TS, axis = i / TS;
        const float x = gen_coord(a, m0 + s, axis);
        uint32_t hi, lo;
        turns_fixed(x, hi, lo);
        E[axis * TS + s] = x;
        for (int k = 0; k < 10; ++k) {
            const uint32_t ph = phase_of(hi, lo, k);
            E[(3 + 6 * k + axis) * TS + s] = sin_phase(ph);
            E[(6 + 6 * k + axis) * TS + s] = sin_phase(ph + 0x40000000u);
        }
    }
    for (int i = tid; i < TS; i += 256) E[63 * TS + i] = 0.f;
    if (a.viewdirs) {
        for (int i = tid; i < 3 * TS; i += 256) {
            const int s = i % TS, axis = i / TS;
            const long long m = m0 + s;
            const float x = m < a.M ? a.viewdirs[(m / a.S) * 3 + axis] : 0.f;
            uint32_t hi, lo;
            turns_fixed(x, hi, lo);
            DV[axis * TS + s] = x;
            for (int k = 0; k < 4; ++k) {
                const uint32_t ph = phase_of(hi, lo, k);
                DV[(3 + 6 * k + axis) * TS + s] = sin_phase(ph);
                DV[(6 + 6 * k + axis) * TS + s] = sin_phase(ph + 0x40000000u);
            }
        }
        for (int i = tid; i < 5 * TS; i += 256) DV[27 * TS + i] = 0.f;
    }
}

// through the direction embedding: d sin(f x) = f cos(f x), d cos(f x) = -f sin(f x)
template <int TS>
__device__ __forceinline__ float gen_dir_grad(const GenArgs& a, long long m, int axis, int s, const float* gDV) {
    const float x = a.viewdirs[(m / a.S) * 3 + axis];
    uint32_t hi, lo;
    turns_fixed(x, hi, lo);
    float gx = gDV[axis * TS + s];
    for (int k = 0; k < 4; ++k) {
        const uint32_t ph = phase_of(hi, lo, k);
        const float f = (float)(1 << k);
        gx += gDV[(3 + 6 * k + axis) * TS + s] * (f * sin_phase(ph + 0x40000000u));
        gx += gDV[(6 + 6 * k + axis) * TS + s] * (f * sin_phase(ph + 0x80000000u));
    }
    return gx;
}

// ---- a supplied 32-feature encoding in the place of the position (NEFES_XYZ_EXTERNAL32) -------------------------------------------
struct GenArgsExt : GenArgs {
    static constexpr bool ext = true;
    const float* xyz_enc;      // [M][32]
    float* g_enc;              // [M][32], backward
};

// E[f][s] = xyz_enc[m0 + s][f], columns of samples >= M as zeros.  A sample's 128 bytes go to eight consecutive lanes as 16-byte
// loads (a wave reads 1 KiB of consecutive memory); the transpose is four scalar LDS stores per lane (the eight lanes of a sample
// share a bank: an 8-way conflict on 4 TS / 32 stores per thread of a kernel that then runs D + 3 matrix products).
template <int NCB>
__device__ __forceinline__ void gen_embed(const GenArgsExt& a, long long m0, float* E, float* DV) {
    constexpr int TS = 32 * NCB;
    for (int i = threadIdx.x; i < TS * (GEN_X_ROWS / 4); i += 256) {
        const int s = i / (GEN_X_ROWS / 4), q = i % (GEN_X_ROWS / 4);
        const long long m = m0 + s;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m < a.M) v = *(const float4*)(a.xyz_enc + m * GEN_X_ROWS + 4 * q);
        E[(4 * q + 0) * TS + s] = v.x;
        E[(4 * q + 1) * TS + s] = v.y;
        E[(4 * q + 2) * TS + s] = v.z;
        E[(4 * q + 3) * TS + s] = v.w;
    }
    gen_embed_dir<NCB>(a, m0, DV);
}

// the backward's last step: g_enc[m][f] = gE[f][s] of the live samples (the same lane <-> address map), d loss / d viewdirs per sample
template <int NCB>
__device__ __forceinline__ void gen_input_grads_ext(const GenArgsExt& a, long long m0, const float* gE, const float* gDV) {
    constexpr int TS = 32 * NCB;
    for (int i = threadIdx.x; i < TS * (GEN_X_ROWS / 4); i += 256) {
        const int s = i / (GEN_X_ROWS / 4), q = i % (GEN_X_ROWS / 4);
        const long long m = m0 + s;
        if (m >= a.M) continue;
        *(float4*)(a.g_enc + m * GEN_X_ROWS + 4 * q) = make_float4(gE[(4 * q + 0) * TS + s], gE[(4 * q + 1) * TS + s],
                                                                    gE[(4 * q + 2) * TS + s], gE[(4 * q + 3) * TS + s]);
    }
    for (int i = threadIdx.x; i < 3 * TS; i += 256) {
        const int s = i % TS, axis = i / TS;
        const long long m = m0 + s;
        if (m >= a.M) continue;
        a.g_vs[m * 3 + axis] = gen_dir_grad<TS>(a, m, axis, s, gDV);
    }
}

// Train mode: where a kernel's operands go.  buf = `acts` (forward) or `dacts` (backward), [tile128][rows][128] in the train layout.
struct GenTrain {
    float* buf;
    int rows;
    GenTrainMap map;
};

// rows [0, rows_p) x the tile's TS samples of block `block`: LDS [row][TS] -> the train buffer, rows >= rows_real as zeros.  Sixteen
// bytes per lane: a row's TS / 4 quads go to consecutive lanes (one conflict-free LDS row per 16 / 8 lanes) and four consecutive rows
// of a 16-sample group are 256 contiguous bytes of the buffer (layout.h nefes_train_off).  rows_p is a multiple of 32.
template <int TS>
__device__ __forceinline__ void gen_train_store(const GenTrain& t, long long m0, int block, const float* src, int rows_real, int rows_p) {
    float* dst = t.buf + (size_t)(m0 >> 7) * t.rows * 128;
    const int s0 = (int)(m0 & 127), row0 = t.map.off[block];
    for (int i = threadIdx.x; i < rows_p * (TS / 4); i += 256) {
        const int q = i % (TS / 4), r = i / (TS / 4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < rows_real) v = *(const float4*)(src + r * TS + 4 * q);
        *(float4*)(dst + nefes_train_off(row0 + r, s0 + 4 * q)) = v;
    }
}

// a tile past the last sample (the launch covers whole 128-sample train tiles): rows [row_lo, row_hi) of its columns are zeros, so
// that the weight-gradient sums over the whole buffer read no unwritten memory
template <int TS>
__device__ __forceinline__ void gen_train_zero(const GenTrain& t, long long m0, int row_lo, int row_hi) {
    float* dst = t.buf + (size_t)(m0 >> 7) * t.rows * 128;
    const int s0 = (int)(m0 & 127);
    for (int i = threadIdx.x; i < (row_hi - row_lo) * (TS / 4); i += 256) {
        const int q = i % (TS / 4), r = row_lo + i / (TS / 4);
        *(float4*)(dst + nefes_train_off(r, s0 + 4 * q)) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

struct GenArgsTrain : GenArgs {
    static constexpr bool train = true;
    GenTrain t;
};
struct GenArgsExtTrain : GenArgsExt {
    static constexpr bool train = true;
    GenTrain t;
};
template <class Args>
__device__ __forceinline__ const GenTrain* gen_train_of(const Args& a) {
    if constexpr (Args::train) return &a.t;
    else return nullptr;
}

// The forward kernel, one instance per argument struct and tile size.  Args::train: the same code plus the copies to the train
// buffer; Args::ext: a supplied 32-feature encoding in the E region (ER = 32 rows, gen_embed's other overload).
template <int NCB, class Args>
__global__ __launch_bounds__(256, 1) void gen_fwd_kernel(Args a) {
    constexpr int TS = 32 * NCB;
    constexpr bool TRAIN = Args::train;
    constexpr int ER = Args::ext ? GEN_X_ROWS : GEN_E_ROWS;      // rows of the E region
    const GenTrain* const tr = gen_train_of(a);
    extern __shared__ __attribute__((aligned(16))) float gen_smem[];
    const GenLayout& g = a.g;
    const int W = g.W, D = g.D, H = W / 2;
    float* E = gen_smem;
    float* DV = E + ER * TS;
    float* X = DV + GEN_DV_ROWS * TS;
    float* Y = X + W * TS;
    const long long tile = blockIdx.x, m0 = tile * TS;
    const int lane = threadIdx.x & 63, half = lane >> 5, l31 = lane & 31;
    const float* blob = a.blob;
    uint32_t* mk = a.masks ? a.masks + (tile * g.mask_words) * 64 + lane : nullptr;
    if constexpr (TRAIN) {
        if (m0 >= a.M) {      // (no mask words, no raw_t: neither buffer has room for this tile)
            gen_train_zero<TS>(*tr, m0, 0, tr->map.off[NEFES_TB_RGB]);
            return;
        }
    }

    gen_embed<NCB>(a, m0, E, DV);
    __syncthreads();
    if constexpr (TRAIN) {
        gen_train_store<TS>(*tr, m0, NEFES_TB_E, E, ER, ER);
        gen_train_store<TS>(*tr, m0, NEFES_TB_DV, DV, GEN_DV_ROWS, GEN_DV_ROWS);
    }

    // hidden layer: ReLU, mask word, activations to LDS (rows beyond m_real are zero rows of the blob: relu(0) = 0)
    auto hidden = [&](float* out, int slot) {
        const int so = g.slot_off[slot];
        return [=](int rb, f32x16(&acc)[NCB]) {
            uint32_t bits = 0u;
#pragma unroll
            for (int c = 0; c < NCB; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const float v = acc[c][r];
                    bits |= (v > 0.f ? 1u : 0u) << (16 * c + r);
                    out[(rb * 32 + gen_rho(half, r)) * TS + 32 * c + l31] = v > 0.f ? v : 0.f;
                }
            if (mk) mk[(so + rb) * 64] = bits;
        };
    };
    auto linear = [&](float* out) {
        return [=](int rb, f32x16(&acc)[NCB]) {
#pragma unroll
            for (int c = 0; c < NCB; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) out[(rb * 32 + gen_rho(half, r)) * TS + 32 * c + l31] = acc[c][r];
        };
    };
    // raw_t[n][ch][s] of this lane's samples
    long long base[NCB];
    bool live[NCB];
#pragma unroll
    for (int c = 0; c < NCB; ++c) {
        const long long m = m0 + 32 * c + l31;
        live[c] = m < a.M;
        base[c] = live[c] ? (m / a.S) * a.R * a.S + m % a.S : 0;
    }
    // head: kind 0 identity, 1 softplus, 2 transient (rows 0..2 sigmoid, 3..4 softplus)
    float* const raw = a.raw_t;
    const long long S64 = a.S;
    auto head = [&](int ch0, int m_real, int kind) {
        return [=](int rb, f32x16(&acc)[NCB]) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rb * 32 + gen_rho(half, r);
                if (row >= m_real) continue;
#pragma unroll
                for (int c = 0; c < NCB; ++c) {
                    if (!live[c]) continue;
                    float v = acc[c][r];
                    if (kind == 1 || (kind == 2 && row >= 3)) v = softplus_ref(v);
                    else if (kind == 2) v = sigmoid_ref(v);
                    raw[base[c] + (long long)(ch0 + row) * S64] = v;
                }
            }
        };
    };

    float *cur = X, *oth = Y;
    {
        const GenLayer& l = g.L[0];
        gen_layer<NCB>(blob + l.wt, E, ER, nullptr, nullptr, 0, l.Mp, l.Mp, W / 32, blob + l.bias, hidden(cur, 0));
    }
    __syncthreads();
    // TRAIN: a layer's output is complete behind its barrier and its buffer is next written behind the following barrier: copy it out here
    if constexpr (TRAIN) gen_train_store<TS>(*tr, m0, NEFES_TB_L1, cur, W, W);
    for (int i = 1; i < D; ++i) {
        const GenLayer& l = g.L[i];
        if (i == g.skip)
            gen_layer<NCB>(blob + l.wt, E, ER, blob + l.wt + (long long)ER * l.Mp, cur, W, l.Mp, l.Mp, W / 32,
                           blob + l.bias, hidden(oth, i));
        else
            gen_layer<NCB>(blob + l.wt, cur, W, nullptr, nullptr, 0, l.Mp, l.Mp, W / 32, blob + l.bias, hidden(oth, i));
        float* t = cur; cur = oth; oth = t;
        __syncthreads();
        if constexpr (TRAIN) gen_train_store<TS>(*tr, m0, NEFES_TB_L1 + i, cur, W, W);
    }
    {
        const GenLayer& l = g.L[g.iSIGMA];
        const int ch = a.mode == NEFES_FIELD_SIGMA ? 0 : 3 + g.C;
        gen_layer<NCB>(blob + l.wt, cur, W, nullptr, nullptr, 0, l.Mp, l.Mp, 1, blob + l.bias, head(ch, 1, 1));
    }
    if (a.mode == NEFES_FIELD_SIGMA) return;
    {
        const GenLayer& l = g.L[g.iFINAL];
        gen_layer<NCB>(blob + l.wt, cur, W, nullptr, nullptr, 0, l.Mp, l.Mp, W / 32, blob + l.bias, linear(oth));
    }
    __syncthreads();
    float *fin = oth, *gbuf = cur;
    if constexpr (TRAIN) gen_train_store<TS>(*tr, m0, NEFES_TB_FINAL, fin, W, W);
    {
        const GenLayer& l = g.L[g.iDIR];
        gen_layer<NCB>(blob + l.wt, fin, W, blob + l.wt + (long long)W * l.Mp, DV, GEN_DV_ROWS, l.Mp, l.Mp, l.Mp / 32, blob + l.bias,
                       hidden(gbuf, D));
    }
    __syncthreads();
    if constexpr (TRAIN) gen_train_store<TS>(*tr, m0, NEFES_TB_DIR, gbuf, g.L[g.iDIR].Mp, g.L[g.iDIR].Mp);
    {
        const GenLayer& l = g.L[g.iRGB];
        gen_layer<NCB>(blob + l.wt, gbuf, H, nullptr, nullptr, 0, l.Mp, l.Mp, l.Mp / 32, blob + l.bias, head(0, 3 + g.C, 0));
    }
    if (a.mode != NEFES_FIELD_FULL) return;
    __syncthreads();
    {
        const GenLayer& l = g.L[g.iT0];
        gen_layer<NCB>(blob + l.wt, fin, W, blob + l.wt + (long long)W * l.Mp, DV, GEN_DV_ROWS, l.Mp, l.Mp, l.Mp / 32, blob + l.bias,
                       hidden(gbuf, D + 1));
    }
    __syncthreads();
    if constexpr (TRAIN) gen_train_store<TS>(*tr, m0, NEFES_TB_T0, gbuf, g.L[g.iDIR].Mp, g.L[g.iDIR].Mp);
    {
        const GenLayer& l = g.L[g.iT1];
        gen_layer<NCB>(blob + l.wt, gbuf, H, nullptr, nullptr, 0, l.Mp, l.Mp, l.Mp / 32, blob + l.bias, hidden(fin, D + 2));
    }
    __syncthreads();
    if constexpr (TRAIN) gen_train_store<TS>(*tr, m0, NEFES_TB_T1, fin, g.L[g.iDIR].Mp, g.L[g.iDIR].Mp);
    {
        const GenLayer& l = g.L[g.iT2];
        gen_layer<NCB>(blob + l.wt, fin, H, nullptr, nullptr, 0, l.Mp, l.Mp, l.Mp / 32, blob + l.bias, hidden(gbuf, D + 3));
    }
    __syncthreads();
    if constexpr (TRAIN) gen_train_store<TS>(*tr, m0, NEFES_TB_T2, gbuf, g.L[g.iDIR].Mp, g.L[g.iDIR].Mp);
    {
        const GenLayer& l = g.L[g.iTH];
        gen_layer<NCB>(blob + l.wt, gbuf, H, nullptr, nullptr, 0, l.Mp, l.Mp, 1, blob + l.bias, head(3 + g.C + 1, 5, 2));
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The backward to the inputs: mode FULL or STATIC.  Args::train: also every layer's pre-activation gradient to `dacts`; Args::ext:
// gE has ER = 32 rows and is stored as it is, no chain rule (gen_input_grads_ext).
template <int NCB, class Args>
__global__ __launch_bounds__(256, 1) void gen_bwd_kernel(Args a) {
    constexpr int TS = 32 * NCB;
    constexpr bool TRAIN = Args::train;
    constexpr int ER = Args::ext ? GEN_X_ROWS : GEN_E_ROWS;      // rows of the E region
    const GenTrain* const tr = gen_train_of(a);
    extern __shared__ __attribute__((aligned(16))) float gen_smem[];
    const GenLayout& g = a.g;
    const int W = g.W, D = g.D, H = W / 2, C = g.C;
    const int RB = W > GEN_HEAD_ROWS ? W : GEN_HEAD_ROWS;
    float* gE = gen_smem;
    float* gDV = gE + ER * TS;
    float* A = gDV + GEN_DV_ROWS * TS;
    float* B = A + RB * TS;
    float* dsig = B + RB * TS;
    const long long tile = blockIdx.x, m0 = tile * TS;
    const int tid = threadIdx.x, lane = tid & 63, half = lane >> 5, l31 = lane & 31;
    const float* blob = a.blob;
    const uint32_t* mk = a.masks + (tile * g.mask_words) * 64 + lane;
    const bool full = a.mode == NEFES_FIELD_FULL;
    if constexpr (TRAIN) {
        if (m0 >= a.M) {      // (past the masks and the ray-gradient buffers: zeros for the weight-gradient sums, nothing else)
            gen_train_zero<TS>(*tr, m0, tr->map.off[NEFES_TB_L1], tr->map.off[NEFES_TB_END]);
            return;
        }
    }

    // this thread's sample column for the cooperative loads (256 % TS == 0: the same for every row it touches)
    const int s_ld = tid % TS, row_ld = tid / TS;
    const long long m_ld = m0 + s_ld;
    const bool live_ld = m_ld < a.M;
    const long long base_ld = live_ld ? (m_ld / a.S) * a.R * a.S + m_ld % a.S : 0;
    // rows [0, rows_p) of `dst` = d loss / d (pre-activation) of head channels ch0 .. ch0 + m_real - 1; kind as in the forward
    auto load_head = [&](float* dst, int ch0, int m_real, int rows_p, int kind) {
        for (int row = row_ld; row < rows_p; row += 256 / TS) {
            float v = 0.f;
            if (live_ld && row < m_real) {
                const long long at = base_ld + (long long)(ch0 + row) * a.S;
                v = a.g_raw_t[at];
                if (kind == 1 || (kind == 2 && row >= 3)) v *= 1.f - expf(-a.raw_in[at]);
                else if (kind == 2) { const float y = a.raw_in[at]; v *= y * (1.f - y); }
            }
            dst[row * TS + s_ld] = v;
        }
    };
    // gradient of a hidden layer's output: keep where the forward's pre-activation was positive; rows < m_real only
    auto masked = [&](float* out, int slot, int m_real, const float* wsig) {
        const int so = g.slot_off[slot];
        return [=](int rb, f32x16(&acc)[NCB]) {
            const uint32_t bits = mk[(so + rb) * 64];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rb * 32 + gen_rho(half, r);
                if (row >= m_real) continue;
                const float ws = wsig ? wsig[row] : 0.f;
#pragma unroll
                for (int c = 0; c < NCB; ++c) {
                    float v = acc[c][r];
                    if (wsig) v += ws * dsig[32 * c + l31];
                    out[row * TS + 32 * c + l31] = ((bits >> (16 * c + r)) & 1u) ? v : 0.f;
                }
            }
        };
    };
    auto plain = [&](float* out, int m_real, bool accumulate) {
        return [=](int rb, f32x16(&acc)[NCB]) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = rb * 32 + gen_rho(half, r);
                if (row >= m_real) continue;
#pragma unroll
                for (int c = 0; c < NCB; ++c) {
                    float* p = out + row * TS + 32 * c + l31;
                    *p = accumulate ? *p + acc[c][r] : acc[c][r];
                }
            }
        };
    };
    const int HB = (H + 31) / 32;

    if (tid < TS) {      // d loss / d (static density's pre-activation): a rank-1 term of the trunk's last gradient
        float v = 0.f;
        if (live_ld) {
            const long long at = base_ld + (long long)(3 + C) * a.S;
            v = a.g_raw_t[at] * (1.f - expf(-a.raw_in[at]));
        }
        dsig[tid] = v;
    }
    if (full) {
        const GenLayer &th = g.L[g.iTH], &t2 = g.L[g.iT2], &t1 = g.L[g.iT1];
        load_head(A, 3 + C + 1, 5, 32, 2);
        __syncthreads();
        // TRAIN: a gradient block is final behind its barrier and its buffer is next written behind the following one: copy it out here
        if constexpr (TRAIN) gen_train_store<TS>(*tr, m0, NEFES_TB_TH, A, 32, 32);
        gen_layer<NCB>(blob + th.wb, A, 32, nullptr, nullptr, 0, th.Kp, H, HB, nullptr, masked(B, D + 3, H, nullptr));
        __syncthreads();
        if constexpr (TRAIN) gen_train_store<TS>(*tr, m0, NEFES_TB_T2, B, H, 32 * HB);
        gen_layer<NCB>(blob + t2.wb, B, H, nullptr, nullptr, 0, t2.Kp, H, HB, nullptr, masked(A, D + 2, H, nullptr));
        __syncthreads();
        if constexpr (TRAIN) gen_train_store<TS>(*tr, m0, NEFES_TB_T1, A, H, 32 * HB);
        gen_layer<NCB>(blob + t1.wb, A, H, nullptr, nullptr, 0, t1.Kp, H, HB, nullptr, masked(B, D + 1, H, nullptr));
        __syncthreads();
        if constexpr (TRAIN) gen_train_store<TS>(*tr, m0, NEFES_TB_T0, B, H, 32 * HB);
    }
    {
        const GenLayer& rgb = g.L[g.iRGB];
        load_head(A, 0, 3 + C, rgb.Mp, 0);
        __syncthreads();
        if constexpr (TRAIN) {
            gen_train_store<TS>(*tr, m0, NEFES_TB_RGB, A, rgb.Mp, rgb.Mp);
            gen_train_store<TS>(*tr, m0, NEFES_TB_SIG, dsig, 1, 32);
        }
        gen_layer<NCB>(blob + rgb.wb, A, rgb.Mp, nullptr, nullptr, 0, rgb.Kp, H, HB, nullptr, masked(B + H * TS, D, H, nullptr));
        __syncthreads();
        if constexpr (TRAIN) gen_train_store<TS>(*tr, m0, NEFES_TB_DIR, B + H * TS, H, 32 * HB);
    }
    {
        // d loss / d [final, direction embedding] = DIR^T g_g (+ T0^T g_t0)
        const GenLayer& dir = g.L[g.iDIR];
        const float* w0 = blob + dir.wb;
        const float* in0 = B + H * TS;
        const float *w1 = nullptr, *in1 = nullptr;
        int K1 = 0;
        if (full) { w1 = blob + g.L[g.iT0].wb; in1 = B; K1 = H; }
        gen_layer<NCB>(w0, in0, H, w1, in1, K1, dir.Kp, W, W / 32, nullptr, plain(A, W, false));
        gen_layer<NCB>(w0 + W, in0, H, w1 ? w1 + W : nullptr, in1, K1, dir.Kp, GEN_DV_ROWS, 1, nullptr, plain(gDV, GEN_DV_ROWS, false));
        __syncthreads();
        if constexpr (TRAIN) gen_train_store<TS>(*tr, m0, NEFES_TB_FINAL, A, W, W);
    }
    {
        const GenLayer &fin = g.L[g.iFINAL], &sg = g.L[g.iSIGMA];
        gen_layer<NCB>(blob + fin.wb, A, W, nullptr, nullptr, 0, fin.Kp, W, W / 32, nullptr, masked(B, D - 1, W, blob + sg.wb));
        __syncthreads();
        if constexpr (TRAIN) gen_train_store<TS>(*tr, m0, NEFES_TB_L1 + D - 1, B, W, W);
    }
    float *cur = B, *oth = A;
    const bool have_skip = g.skip > 0 && g.skip < D;
    for (int i = D - 1; i >= 1; --i) {
        const GenLayer& l = g.L[i];
        const int hoff = i == g.skip ? ER : 0;
        gen_layer<NCB>(blob + l.wb + hoff, cur, W, nullptr, nullptr, 0, l.Kp, W, W / 32, nullptr, masked(oth, i - 1, W, nullptr));
        if (i == g.skip)
            gen_layer<NCB>(blob + l.wb, cur, W, nullptr, nullptr, 0, l.Kp, ER, ER / 32, nullptr, plain(gE, ER, false));
        float* t = cur; cur = oth; oth = t;
        __syncthreads();
        if constexpr (TRAIN) gen_train_store<TS>(*tr, m0, NEFES_TB_L1 + i - 1, cur, W, W);
    }
    {
        const GenLayer& l = g.L[0];
        gen_layer<NCB>(blob + l.wb, cur, W, nullptr, nullptr, 0, l.Kp, ER, ER / 32, nullptr, plain(gE, ER, have_skip));
        __syncthreads();
    }
    if constexpr (Args::ext) {
        gen_input_grads_ext<NCB>(a, m0, gE, gDV);
        return;
    }
    // through the embeddings: d sin(f x) = f cos(f x), d cos(f x) = -f sin(f x)
    for (int i = tid; i < 3 * TS; i += 256) {
        const int s = i % TS, axis = i / TS;
        const long long m = m0 + s;
        if (m >= a.M) continue;
        {
            const float x = gen_coord(a, m, axis);
            uint32_t hi, lo;
            turns_fixed(x, hi, lo);
            float gx = gE[axis * TS + s];
            for (int k = 0; k < 10; ++k) {
                const uint32_t ph = phase_of(hi, lo, k);
                const float f = (float)(1 << k);
                gx += gE[(3 + 6 * k + axis) * TS + s] * (f * sin_phase(ph + 0x40000000u));
                gx += gE[(6 + 6 * k + axis) * TS + s] * (f * sin_phase(ph + 0x80000000u));
            }
            a.g_pts[m * 3 + axis] = gx;
        }
        {
            const float x = a.viewdirs[(m / a.S) * 3 + axis];
            uint32_t hi, lo;
            turns_fixed(x, hi, lo);
            float gx = gDV[axis * TS + s];
            for (int k = 0; k < 4; ++k) {
                const uint32_t ph = phase_of(hi, lo, k);
                const float f = (float)(1 << k);
                gx += gDV[(3 + 6 * k + axis) * TS + s] * (f * sin_phase(ph + 0x40000000u));
                gx += gDV[(6 + 6 * k + axis) * TS + s] * (f * sin_phase(ph + 0x80000000u));
            }
            a.g_vs[m * 3 + axis] = gx;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
template <class K, class Args>
static int gen_launch(K k, const Args& a, size_t lds, long long n_tiles, hipStream_t st) {
    if (n_tiles > 0x7fffffffLL) return NEFES_E_UNSUPPORTED;
    hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k, dim3((unsigned)n_tiles), dim3(256), lds, st, a);
    return (int)hipGetLastError();
}

static int gen_fill(GenArgs& a, const NefesGenericNetDesc* desc, const void* packed, int mode, int N, int S, int xyz_encoding) {
    int rc = gen_layout(desc, &a.g);
    if (rc) return rc;
    if (desc->xyz_encoding != xyz_encoding) return NEFES_E_UNSUPPORTED;      // each entry point serves one encoding
    if (mode != NEFES_FIELD_SIGMA && mode != NEFES_FIELD_STATIC && mode != NEFES_FIELD_FULL) return NEFES_E_BADARG;
    if (mode == NEFES_FIELD_FULL && !desc->has_transient) return NEFES_E_BADARG;
    a.blob = (const float*)packed;
    a.S = S;
    a.mode = mode;
    a.R = mode == NEFES_FIELD_SIGMA ? 1 : 3 + a.g.C + (mode == NEFES_FIELD_STATIC ? 1 : 6);
    a.M = (long long)N * S;
    return 0;
}

static int gen_fill_train(GenTrain& t, const NefesGenericNetDesc* desc, float* buf, int xyz_encoding) {
    t.buf = buf;
    const int rc = gen_train_map(desc, xyz_encoding, &t.map);
    t.rows = t.map.off[NEFES_TB_END];
    return rc;
}

// whole 128-sample train tiles: the tiles past the last sample write zeros (gen_train_zero)
static long long gen_train_tiles(long long M, int TS) { return (M + 127) / 128 * (128 / TS); }

// forward: E, DV and the two activation buffers; backward: gE, gDV, two gradient buffers that also hold the heads' rows, dsig.
// (On a supplied encoding the E region is GEN_X_ROWS rows: the GEN_E_ROWS - GEN_X_ROWS rows it does not have are not requested.)
static size_t gen_lds_bytes(bool ext, bool bwd, int W, int TS) {
    const int ER = ext ? GEN_X_ROWS : GEN_E_ROWS;
    const int RB = W > GEN_HEAD_ROWS ? W : GEN_HEAD_ROWS;
    return (size_t)(ER + GEN_DV_ROWS + (bwd ? 2 * RB + 1 : 2 * W)) * TS * 4;
}

// Everything behind an entry point's own test of its pointers, sizes and mode, on `a` with that call's pointers in place: the layout,
// the train buffer's row map (train_buf = `acts` / `dacts`; Args::train), the 16-byte alignment of the buffers a supplied encoding
// is moved through as float4 (Args::ext), LDS size, tile count, the instance of the tile size.
template <bool BWD, class Args>
static int gen_run(Args& a, const NefesGenericNetDesc* desc, const void* packed, int mode, int N, int S, float* train_buf, void* stream) {
    constexpr int enc = Args::ext ? NEFES_XYZ_EXTERNAL32 : NEFES_XYZ_FREQ10;
    int rc = gen_fill(a, desc, packed, mode, N, S, enc);
    if (rc) return rc;
    if constexpr (Args::train) {
        rc = gen_fill_train(a.t, desc, train_buf, enc);
        if (rc) return rc;
    }
    if constexpr (Args::ext) {
        uintptr_t p = (uintptr_t)(BWD ? (const float*)a.g_enc : a.xyz_enc);
        if constexpr (Args::train) p |= (uintptr_t)train_buf;
        if (p & 15) return NEFES_E_BADARG;
    }
    const int TS = gen_tile(a.g.W);
    const size_t lds = gen_lds_bytes(Args::ext, BWD, a.g.W, TS);
    const long long n_tiles = Args::train ? gen_train_tiles(a.M, TS) : (a.M + TS - 1) / TS;
    if (TS == 64) return gen_launch(BWD ? gen_bwd_kernel<2, Args> : gen_fwd_kernel<2, Args>, a, lds, n_tiles, (hipStream_t)stream);
    return gen_launch(BWD ? gen_bwd_kernel<1, Args> : gen_fwd_kernel<1, Args>, a, lds, n_tiles, (hipStream_t)stream);
}

// ---- inference: the frequency embedding, then a supplied encoding ---------------------------------------------------------------------
extern "C" int nefes_field_fwd_generic(const NefesGenericNetDesc* desc, const void* packed, int mode, int N, int S,
                                       const float* rays_o, const float* rays_d, const float* z, const float* pts,
                                       const float* viewdirs, float* raw_t, uint32_t* masks, void* stream) {
    if (!desc || !packed || !raw_t || N <= 0 || S <= 0 || (!pts && !(rays_o && rays_d && z)) || (mode != NEFES_FIELD_SIGMA && !viewdirs))
        return NEFES_E_BADARG;
    GenArgs a;
    memset(&a, 0, sizeof(a));
    a.rays_o = rays_o; a.rays_d = rays_d; a.z = z; a.pts = pts;
    a.viewdirs = mode == NEFES_FIELD_SIGMA ? nullptr : viewdirs;
    a.raw_t = raw_t; a.masks = masks;
    return gen_run<false>(a, desc, packed, mode, N, S, nullptr, stream);
}

extern "C" int nefes_field_bwd_generic(const NefesGenericNetDesc* desc, const void* packed, int mode, int N, int S,
                                       const float* rays_o, const float* rays_d, const float* z, const float* pts,
                                       const float* viewdirs, const float* raw_t, const float* g_raw_t, const uint32_t* masks,
                                       float* g_pts, float* g_viewdirs_s, void* stream) {
    if (!desc || !packed || !raw_t || !g_raw_t || !masks || !g_pts || !g_viewdirs_s || !viewdirs || N <= 0 || S <= 0 ||
        (!pts && !(rays_o && rays_d && z)) || mode == NEFES_FIELD_SIGMA)
        return NEFES_E_BADARG;
    GenArgs a;
    memset(&a, 0, sizeof(a));
    a.rays_o = rays_o; a.rays_d = rays_d; a.z = z; a.pts = pts; a.viewdirs = viewdirs;
    a.raw_in = raw_t; a.g_raw_t = g_raw_t; a.masks = const_cast<uint32_t*>(masks);
    a.g_pts = g_pts; a.g_vs = g_viewdirs_s;
    return gen_run<true>(a, desc, packed, mode, N, S, nullptr, stream);
}

extern "C" int nefes_field_fwd_generic_ext(const NefesGenericNetDesc* desc, const void* packed, int mode, int N, int S,
                                           const float* xyz_enc, const float* viewdirs, float* raw_t, uint32_t* masks, void* stream) {
    if (!desc || !packed || !xyz_enc || !raw_t || N <= 0 || S <= 0 || (mode != NEFES_FIELD_SIGMA && !viewdirs)) return NEFES_E_BADARG;
    GenArgsExt a;
    memset(&a, 0, sizeof(a));
    a.xyz_enc = xyz_enc;
    a.viewdirs = mode == NEFES_FIELD_SIGMA ? nullptr : viewdirs;
    a.raw_t = raw_t; a.masks = masks;
    return gen_run<false>(a, desc, packed, mode, N, S, nullptr, stream);
}

extern "C" int nefes_field_bwd_generic_ext(const NefesGenericNetDesc* desc, const void* packed, int mode, int N, int S,
                                           const float* viewdirs, const float* raw_t, const float* g_raw_t, const uint32_t* masks,
                                           float* g_xyz_enc, float* g_viewdirs_s, void* stream) {
    if (!desc || !packed || !raw_t || !g_raw_t || !masks || !g_xyz_enc || !g_viewdirs_s || !viewdirs || N <= 0 || S <= 0 ||
        mode == NEFES_FIELD_SIGMA)
        return NEFES_E_BADARG;
    GenArgsExt a;
    memset(&a, 0, sizeof(a));
    a.viewdirs = viewdirs;
    a.raw_in = raw_t; a.g_raw_t = g_raw_t; a.masks = const_cast<uint32_t*>(masks);
    a.g_enc = g_xyz_enc; a.g_vs = g_viewdirs_s;
    return gen_run<true>(a, desc, packed, mode, N, S, nullptr, stream);
}

// ---- train mode: the same two pairs with the train buffer (`acts` / `dacts`), rays only, mode STATIC or FULL ----------------------------
extern "C" int nefes_field_fwd_train_generic(const NefesGenericNetDesc* desc, const void* packed, int mode, int N, int S,
                                             const float* rays_o, const float* rays_d, const float* z, const float* viewdirs,
                                             float* raw_t, float* acts, uint32_t* masks, void* stream) {
    if (!desc || !packed || !raw_t || !acts || !masks || !viewdirs || !rays_o || !rays_d || !z || N <= 0 || S <= 0 ||
        (mode != NEFES_FIELD_STATIC && mode != NEFES_FIELD_FULL))
        return NEFES_E_BADARG;
    GenArgsTrain a;
    memset(&a, 0, sizeof(a));
    a.rays_o = rays_o; a.rays_d = rays_d; a.z = z; a.viewdirs = viewdirs;
    a.raw_t = raw_t; a.masks = masks;
    return gen_run<false>(a, desc, packed, mode, N, S, acts, stream);
}

extern "C" int nefes_field_bwd_train_generic(const NefesGenericNetDesc* desc, const void* packed, int mode, int N, int S,
                                             const float* rays_o, const float* rays_d, const float* z, const float* viewdirs,
                                             const float* raw_t, const float* g_raw_t, const uint32_t* masks, float* dacts, float* g_pts,
                                             float* g_viewdirs_s, void* stream) {
    if (!desc || !packed || !raw_t || !g_raw_t || !masks || !dacts || !g_pts || !g_viewdirs_s || !viewdirs || !rays_o || !rays_d || !z ||
        N <= 0 || S <= 0 || (mode != NEFES_FIELD_STATIC && mode != NEFES_FIELD_FULL))
        return NEFES_E_BADARG;
    GenArgsTrain a;
    memset(&a, 0, sizeof(a));
    a.rays_o = rays_o; a.rays_d = rays_d; a.z = z; a.viewdirs = viewdirs;
    a.raw_in = raw_t; a.g_raw_t = g_raw_t; a.masks = const_cast<uint32_t*>(masks);
    a.g_pts = g_pts; a.g_vs = g_viewdirs_s;
    return gen_run<true>(a, desc, packed, mode, N, S, dacts, stream);
}

extern "C" int nefes_field_fwd_train_generic_ext(const NefesGenericNetDesc* desc, const void* packed, int mode, int N, int S,
                                                 const float* xyz_enc, const float* viewdirs, float* raw_t, float* acts, uint32_t* masks,
                                                 void* stream) {
    if (!desc || !packed || !xyz_enc || !raw_t || !acts || !masks || !viewdirs || N <= 0 || S <= 0 ||
        (mode != NEFES_FIELD_STATIC && mode != NEFES_FIELD_FULL))
        return NEFES_E_BADARG;
    GenArgsExtTrain a;
    memset(&a, 0, sizeof(a));
    a.xyz_enc = xyz_enc; a.viewdirs = viewdirs;
    a.raw_t = raw_t; a.masks = masks;
    return gen_run<false>(a, desc, packed, mode, N, S, acts, stream);
}

extern "C" int nefes_field_bwd_train_generic_ext(const NefesGenericNetDesc* desc, const void* packed, int mode, int N, int S,
                                                 const float* viewdirs, const float* raw_t, const float* g_raw_t, const uint32_t* masks,
                                                 float* dacts, float* g_xyz_enc, float* g_viewdirs_s, void* stream) {
    if (!desc || !packed || !raw_t || !g_raw_t || !masks || !dacts || !g_xyz_enc || !g_viewdirs_s || !viewdirs || N <= 0 || S <= 0 ||
        (mode != NEFES_FIELD_STATIC && mode != NEFES_FIELD_FULL))
        return NEFES_E_BADARG;
    GenArgsExtTrain a;
    memset(&a, 0, sizeof(a));
    a.viewdirs = viewdirs;
    a.raw_in = raw_t; a.g_raw_t = g_raw_t; a.masks = const_cast<uint32_t*>(masks);
    a.g_enc = g_xyz_enc; a.g_vs = g_viewdirs_s;
    return gen_run<true>(a, desc, packed, mode, N, S, dacts, stream);
}

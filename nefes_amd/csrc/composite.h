// The two sample-per-lane layouts of the compositing kernels (composite.hip) and of the fused coarse-pass sampler (sample_pdf.hip), and
// the per-sample alpha they share.  A layout holds K sample slots per lane and provides what truly differs between the two families:
// ray / lane indexing with the `live` / `in` predicates, rows of the ray read and written, the sum over a ray, the exclusive f64 running
// product, the reverse affine scan, and how feature channels spread over lanes.  The algebra of raw2outputs_NeRFH_NFF is written once,
// over float[K] / double[K], on top of these.
#pragma once
#include "wave.h"

template <int K>
struct Ray {
    float zz[K], dl[K], a_c[K], a_s[K], a_t[K], T[K], Ts[K], e_c[K], e_s[K], e_t[K];
};

// alpha = 1 - exp(-delta * sigma) of the combined, static and transient densities of slot k (nerfh_nff.py:55-68); `last`: the ray's last
// sample (delta = 1e2, no |d| scaling), `in`: the slot holds a sample of the ray (alpha = 0 otherwise)
template <int K>
__device__ __forceinline__ void sample_alpha(bool transient, bool in, bool last, float z0, float z1, float ss, float st, Ray<K>& r, int k) {
    r.zz[k] = z0;
    r.dl[k] = last ? 1e2f : (z1 - z0);
    r.e_c[k] = expf(-(r.dl[k] * (ss + st)));
    r.a_c[k] = in ? 1.f - r.e_c[k] : 0.f;
    if (transient) {
        r.e_s[k] = expf(-(r.dl[k] * ss));
        r.e_t[k] = expf(-(r.dl[k] * st));
        r.a_s[k] = in ? 1.f - r.e_s[k] : 0.f;
        r.a_t[k] = in ? 1.f - r.e_t[k] : 0.f;
    } else {
        r.e_s[k] = r.e_c[k]; r.e_t[k] = 1.f; r.a_s[k] = r.a_c[k]; r.a_t[k] = 0.f;
    }
}

// One sample per lane in Q passes of 64 lanes, any S <= 64 Q: slot k is sample lane + 64 k and the ray is the wave.  A slot may lie
// beyond S; rows move one float per lane (256-byte coalesced rows per pass).  A slot beyond S reads the ray's last sample wherever a row
// is read without a guard (in bounds; its alpha is 0, its delta whatever the two clamped depths give, and every sum, scan and store skips it).
template <int Q>
struct OnePerLane {
    static constexpr int K = Q;
    static constexpr int LANES = 64;                  // lanes that hold feature channels
    static constexpr int AHEAD = 1;                   // feature rows requested before the first is consumed
    int lane, sl, ray, S;
    bool live;
    __device__ __forceinline__ OnePerLane(int N, int S_)
        : lane(threadIdx.x & 63), sl(lane), ray(blockIdx.x * 4 + (threadIdx.x >> 6)), S(S_), live(ray < N) {}
    __device__ __forceinline__ bool idle() const { return !live; }               // the whole wave has no ray
    __device__ __forceinline__ int sample(int k) const { return lane + 64 * k; }
    __device__ __forceinline__ bool in(int k) const { return sample(k) < S; }
    // a row of the ray, named as base + offset (the offset is the same on every lane and stays out of the vector registers): read one
    // float per lane where it is used; slots beyond S read the last sample (in bounds, unused)
    struct Row { const float* base; size_t off; };
    __device__ __forceinline__ Row row(const float* base, size_t off) const { return {base, off}; }
    __device__ __forceinline__ float at(const Row& r, int k) const { return (r.base + (in(k) ? sample(k) : S - 1))[r.off]; }
    __device__ __forceinline__ void load_row(const float* base, size_t off, float (&v)[K]) const {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = at(row(base, off), k);
    }
    __device__ __forceinline__ void store_row(float* base, size_t off, const float (&v)[K]) const {
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (in(k)) base[off + sample(k)] = v[k];
    }
    __device__ __forceinline__ void load_z(const float* zr, float (&z0)[K], float (&z1)[K]) const {      // depths and their successors
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int sc = in(k) ? sample(k) : S - 1;
            z0[k] = zr[sc];
            z1[k] = zr[sc + 1 < S ? sc + 1 : sc];
        }
    }
    __device__ __forceinline__ double sum(double v) const { return wave_sum(v); }
    // exclusive cumprod over the ray, f64 accumulate, rounded to f32 per element: one wave scan per pass and a carry
    __device__ __forceinline__ float excl_pass(double om, double& carry) const {      // one pass of it; carry: the product of the passes before
        const double inc = wave_incl_prod(om, lane);
        const double prev = __shfl_up(inc, 1);
        const float T = (float)(carry * (lane == 0 ? 1.0 : prev));
        carry *= lane_bcast(inc, 63);
        return T;
    }
    template <class F>
    __device__ __forceinline__ void excl_prod(F&& om, float (&T)[K]) const {
        double carry = 1.0;
#pragma unroll
        for (int k = 0; k < K; ++k) T[k] = excl_pass(om(k), carry);
    }
    // X_i = a_i + m_i X_{i+1} over the ray, B_i = X_{i+1}, the maps given as map(k, m, a): one reverse wave scan per pass, last pass
    // first, and a carry
    __device__ __forceinline__ double rev_pass(double m, double a, double& carry) const {      // one pass of it (last pass first): B of the pass's slot
        wave_rev_affine(m, a, lane);
        const double X = a + m * carry;
        const double nxt = __shfl_down(X, 1);
        const double B = (lane < 63) ? nxt : carry;
        carry = lane_bcast(X, 0);
        return B;
    }
};

// Four consecutive samples per lane, S = 64 RW: slot k is sample 4 sl + k, a ray is 16 RW lanes and 4 / RW rays share a wave (Seg<RW>,
// wave.h).  Every slot is inside the ray; idle lanes shadow the last ray (loads stay in bounds, nothing is stored); rows move as one
// 16-byte access per lane (16-byte aligned pointers).  A ray of one row of 16 lanes (RW = 1) scans on DPP row shifts: the same
// Hillis-Steele tree as the ds_bpermute form, the same results.
template <int RW>
struct FourPerLane {
    static constexpr int K = 4;
    static constexpr int LPR = Seg<RW>::LPR, RPW = Seg<RW>::RPW;
    static constexpr int LANES = LPR;
    static constexpr int AHEAD = 4;
    int lane, seg, sl, ray;
    bool live;
    __device__ __forceinline__ FourPerLane(int N, int) : lane(threadIdx.x & 63), seg(lane / LPR), sl(lane - seg * LPR) {
        const int ray_raw = (blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW + seg;
        live = seg < RPW && ray_raw < N;
        ray = live ? ray_raw : N - 1;
    }
    __device__ __forceinline__ bool idle() const { return false; }
    __device__ __forceinline__ int sample(int k) const { return 4 * sl + k; }
    __device__ __forceinline__ bool in(int) const { return true; }
    // a row of the ray: one 16-byte load per lane, requested where the row is named
    // (kept as the 16-byte vector it was loaded as: split into four floats at once, a conditional row costs a copy and a wait)
    struct Row { float4 q; };
    __device__ __forceinline__ Row row(const float* base, size_t off) const { return {*(const float4*)(base + off + 4 * sl)}; }
    __device__ __forceinline__ Row row_if(bool have, const float* base, size_t off) const {      // a row that may be absent: zeros then
        Row r = {make_float4(0.f, 0.f, 0.f, 0.f)};
        if (have) r = row(base, off);
        return r;
    }
    __device__ __forceinline__ float at(const Row& r, int k) const { return k == 0 ? r.q.x : (k == 1 ? r.q.y : (k == 2 ? r.q.z : r.q.w)); }
    __device__ __forceinline__ void load_row(const float* base, size_t off, float (&v)[4]) const {
        const Row r = row(base, off);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = at(r, k);
    }
    __device__ __forceinline__ void store_row(float* base, size_t off, const float (&v)[4]) const {
        // one 16-byte store.  (A wrong gradient row once seen here was not the store's doing but a compiler-made packed fp32 multiply:
        // DESIGN.md 4.7.)
        *(float4*)(base + off + 4 * sl) = make_float4(v[0], v[1], v[2], v[3]);
    }
    __device__ __forceinline__ float next_lane(float v) const { return RW == 1 ? row_next(v) : __shfl_down(v, 1); }
    __device__ __forceinline__ void load_z(const float* zr, float (&z0)[4], float (&z1)[4]) const {
        load_row(zr, 0, z0);
        z1[0] = z0[1]; z1[1] = z0[2]; z1[2] = z0[3];
        z1[3] = next_lane(z0[0]);                                        // first depth of the next lane's group (unused by a ray's last lane)
    }
    __device__ __forceinline__ double sum(double v) const { return seg_sum<RW>(v, lane); }
    // exclusive cumprod: the lane's own running product, times the product of everything in front of the lane (one cross-lane scan)
    template <class F>
    __device__ __forceinline__ void excl_prod(F&& om, float (&T)[4]) const {
        const double p0 = om(0), p1 = p0 * om(1), p2 = p1 * om(2), p3 = p2 * om(3);
        const double inc = RW == 1 ? row_incl_prod(p3) : seg_incl_prod<RW>(p3, sl);
        const double prev = RW == 1 ? row_prev(inc, 1.0) : __shfl_up(inc, 1);
        const double E = sl == 0 ? 1.0 : prev;
        T[0] = (float)E; T[1] = (float)(E * p0); T[2] = (float)(E * p1); T[3] = (float)(E * p2);
    }
    // the lane's four maps composed, one reverse scan across the ray's lanes, then the lane's own elements by back-substitution from
    // the next lane's X
    template <class F>
    __device__ __forceinline__ void rev_affine(F&& map, double (&B)[4]) const {
        double mk[4], ak[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) map(k, mk[k], ak[k]);
        double m = ((mk[0] * mk[1]) * mk[2]) * mk[3];
        double a = ak[0] + mk[0] * (ak[1] + mk[1] * (ak[2] + mk[2] * ak[3]));
        seg_rev_affine<RW>(m, a, sl);
        const double nxt = __shfl_down(a, 1);
        double X = sl + 1 < LPR ? nxt : 0.0;
#pragma unroll
        for (int k = 3; k >= 0; --k) { B[k] = X; X = ak[k] + mk[k] * X; }
    }
};

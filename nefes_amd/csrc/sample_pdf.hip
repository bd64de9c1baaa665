// Hierarchical (inverse-CDF) importance sampling + merge with the coarse depths: one wavefront per ray.
// Restates sample_pdf (script/models/rendering.py:23-66) and rendering.py:132-141
// (z_vals_mid, weights[...,1:-1], detach, sort(cat[z_vals, z_samples])).
//
// Roofline: HBM-bound, ~1.3 KB per ray (256 B weights + 256 B z read, 768 B written at 64+128).
// Bit-exactness: given the same CDF and u, `inds` equals torch.searchsorted(cdf, u, right=True)
// exactly (integer count of cdf[k] <= u) and the interpolation repeats the reference's fp32 op order
// with no FMA contraction.  The CDF itself is built as torch's CPU path does: pdf = (w+1e-5)/sum,
// running sum accumulated in f64 and rounded to f32 per element.
#include "../../include/nefes_hip.h"
#include "composite.h"

#define SP_MAX_NC 256
#define SP_MAX_S 512

// #{k < n : a[k] < v} / #{k < n : a[k] <= v} of a non-decreasing LDS array: what the linear counts below return, in log2(n) steps
__device__ __forceinline__ int count_less(const float* a, int n, float v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ int count_less_equal(const float* a, int n, float v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// true on every lane iff a[0..n) is non-decreasing (NaNs make it false: the callers then take the order-free linear path)
__device__ __forceinline__ bool wave_sorted(const float* a, int n, int lane) {
    bool ok = true;
    for (int k = lane; k + 1 < n; k += 64) ok = ok && (a[k] <= a[k + 1]);
    return __ballot(!ok) == 0ull;
}

__global__ __launch_bounds__(256) void sample_pdf_merge_kernel(int N, int Nc, int Ni, int layout, const float* __restrict__ z_coarse,
                                                               const float* __restrict__ weights, const float* __restrict__ u,
                                                               int u_per_ray, const float* __restrict__ cdf_in, float* z_fine,
                                                               float* z_samples, int32_t* inds_out, float* cdf_out) {
    __shared__ float s_cdf[4][SP_MAX_NC];
    __shared__ float s_bins[4][SP_MAX_NC];
    __shared__ float s_all[4][SP_MAX_S];
    __shared__ float s_sorted[4][SP_MAX_S];    // the merged depths by rank, so that z_fine leaves as whole rows (a scattered 4-byte store per sample before)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int ray = blockIdx.x * 4 + wv;
    if (ray >= N) return;
    float* cdf = s_cdf[wv];
    float* bins = s_bins[wv];
    float* all = s_all[wv];
    const int nb = Nc - 1;      // bins = z_mid, cdf has nb entries (rendering.py:29: cat[0, cumsum(pdf)])
    const int np = Nc - 2;      // pdf entries = weights[1:-1]
    const float* zc = z_coarse + (size_t)ray * (layout ? nb : Nc);
    // w[k+1] is pdf entry k in both layouts
    const float* w = layout ? weights + (size_t)ray * np - 1 : weights + (size_t)ray * Nc;

    if (layout) {
        for (int k = lane; k < nb; k += 64) bins[k] = zc[k];
    } else {
        for (int k = lane; k < nb; k += 64) bins[k] = __fmul_rn(.5f, __fadd_rn(zc[k + 1], zc[k]));   // :132
        for (int k = lane; k < Nc; k += 64) all[k] = zc[k];
    }
    if (cdf_in) {
        for (int k = lane; k < nb; k += 64) cdf[k] = cdf_in[(size_t)ray * nb + k];
    } else {
        double part = 0.0;
        for (int k = lane; k < np; k += 64) part += (double)__fadd_rn(w[k + 1], 1e-5f);          // :26
        const float total = (float)wave_sum(part);
        double carry = 0.0;
        if (lane == 0) cdf[0] = 0.f;
        for (int k0 = 0; k0 < np; k0 += 64) {
            const int k = k0 + lane;
            const double pdf = k < np ? (double)__fdiv_rn(__fadd_rn(w[k + 1], 1e-5f), total) : 0.0;   // :27
            const double inc = wave_incl_sum_dpp(pdf, lane) + carry;                               // :28 (f64 accumulate)
            if (k < np) cdf[k + 1] = (float)inc;
            carry = lane_bcast(inc, 63);
        }
    }
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    if (cdf_out)
        for (int k = lane; k < nb; k += 64) cdf_out[(size_t)ray * nb + k] = cdf[k];

    // a cumulative sum of positive terms is non-decreasing; a caller-supplied CDF is checked rather than trusted
    const bool cdf_sorted = wave_sorted(cdf, nb, lane);
    // two samples per lane per pass: their binary searches are independent chains of LDS reads, issued side by side
    for (int i0 = lane; i0 < Ni; i0 += 128) {
        const int ii[2] = {i0, i0 + 64};
        float uu[2];
        int cnt[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int i = ii[e] < Ni ? ii[e] : Ni - 1;
            uu[e] = u_per_ray ? u[(size_t)ray * Ni + i] : u[i];
        }
        if (cdf_sorted && uu[0] == uu[0] && uu[1] == uu[1]) {          // searchsorted(..., right=True): #{k : cdf[k] <= u}  (:51)
            int lo0 = 0, hi0 = nb, lo1 = 0, hi1 = nb;
            while (lo0 < hi0 || lo1 < hi1) {
                const int m0 = (lo0 + hi0) >> 1, m1 = (lo1 + hi1) >> 1;
                const float c0 = cdf[m0 < nb ? m0 : nb - 1], c1 = cdf[m1 < nb ? m1 : nb - 1];
                if (lo0 < hi0) { if (c0 <= uu[0]) lo0 = m0 + 1; else hi0 = m0; }
                if (lo1 < hi1) { if (c1 <= uu[1]) lo1 = m1 + 1; else hi1 = m1; }
            }
            cnt[0] = lo0; cnt[1] = lo1;
        } else {
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                cnt[e] = 0;
                if (cdf_sorted && uu[e] == uu[e]) cnt[e] = count_less_equal(cdf, nb, uu[e]);
                else for (int k = 0; k < nb; ++k) cnt[e] += (cdf[k] <= uu[e]) ? 1 : 0;
            }
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            if (ii[e] >= Ni) continue;
            const int i = ii[e];
            const int below = cnt[e] - 1 > 0 ? cnt[e] - 1 : 0;      // :52-53
            const int above = cnt[e] < nb - 1 ? cnt[e] : nb - 1;
            const float c_lo = cdf[below], c_hi = cdf[above], b_lo = bins[below], b_hi = bins[above];
            float denom = __fsub_rn(c_hi, c_lo);              // :60-64
            denom = denom < 1e-5f ? 1.f : denom;
            const float t = __fdiv_rn(__fsub_rn(uu[e], c_lo), denom);
            const float smp = __fadd_rn(b_lo, __fmul_rn(t, __fsub_rn(b_hi, b_lo)));
            all[Nc + i] = smp;
            if (z_samples) z_samples[(size_t)ray * Ni + i] = smp;
            if (inds_out) inds_out[(size_t)ray * Ni + i] = cnt[e];
        }
    }
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    if (z_fine) {
        // stable rank sort of cat[z_coarse, z_samples] (values identical to torch.sort(...)[0], :141)
        const int S = Nc + Ni;
        // Both halves are already ordered at test time (coarse depths; inverse CDF of an increasing u): the stable rank is
        // then own index + a binary-search count in the other half (ties: coarse first, as cat[z_vals, z_samples] sorts).
        // Jittered u (train mode) or NaNs fall back to the all-pairs rank.
        const bool ordered = wave_sorted(all, Nc, lane) && wave_sorted(all + Nc, Ni, lane);
        for (int i = lane; i < S; i += 64) {
            const float v = all[i];
            int rank = 0;
            if (ordered) {
                rank = i < Nc ? i + count_less(all + Nc, Ni, v) : (i - Nc) + count_less_equal(all, Nc, v);
            } else {
                // torch.sort order: numbers ascending, NaNs last, ties (and NaNs among themselves) by index: every slot of
                // z_fine is written exactly once whatever the values are
                const bool v_nan = v != v;
                for (int k = 0; k < S; ++k) {
                    const float o = all[k];
                    const bool o_nan = o != o;
                    const bool before = v_nan ? (!o_nan || k < i) : (!o_nan && (o < v || (o == v && k < i)));
                    rank += before ? 1 : 0;
                }
            }
            s_sorted[wv][rank] = v;
        }
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        for (int i = lane; i < S; i += 64) z_fine[(size_t)ray * S + i] = s_sorted[wv][i];
    }
}


// =====================================================================================================================
// The coarse pass behind its field kernel as ONE launch (round 4): compositing variant D (weights of the sigma-only coarse pass,
// nerfh_nff.py:83-89 / composite.hip composite_fwd_kernel) + sample_pdf + sort(cat[z_vals, z_samples]) per ray, for
// Nc = 64 RW coarse samples (RW = 1, 2, 4).  A ray occupies 16 RW lanes with four consecutive coarse samples each: the layout
// FourPerLane<RW> of composite.h -- 4 / RW rays per wave, 16 / RW per workgroup -- so the coarse weights never
// travel to HBM and back (79 MB written by one launch and read by the next at the headline shape) and a 64-entry CDF no longer
// leaves three quarters of a wave idle.  `z` is one row of Nc depths per ray (z_stride = Nc) or one row shared by every ray
// (z_stride = 0: scalar near / far without jitter, rendering.py:96-100 -- the row is then never materialised per ray at all).
// The weights come from the same two pieces as composite_fwd_kernel<FourPerLane<RW>>'s (composite.h: sample_alpha and the layout's
// exclusive running product), the rest repeats sample_pdf_merge_kernel's arithmetic (f64 sums are exact here, so their association
// does not matter): z_fine is bit-identical to the three launches it replaces (tests/test_gpu_surface.py).
// =====================================================================================================================
// LDS floats per ray (16-byte aligned rows): cb [2 Nc] = {cdf_k, bins_k} pairs; zp [Nc + 8] = the coarse depths behind four -inf and
// in front of +inf sentinels; s2 [2 Ni] = {sample_i, count_i} pairs; sorted [S] (the counters of the inverse-CDF histogram live
// here until the merge); hist [Nc + 4].  Per workgroup: up [Ni + 8] = the shared u row, padded the same way.
__host__ __device__ inline int coarse_sample_lds_floats(int Nc, int Ni) { return 2 * Nc + (Nc + 8) + (2 * Ni + 3) / 4 * 4 + (Nc + Ni + 3) / 4 * 4 + (Nc + 4); }
__host__ __device__ inline int coarse_sample_u_floats(int Ni) { return (Ni + 8 + 3) / 4 * 4; }

template <int RW>
__global__ __launch_bounds__(256) void coarse_sample_kernel(int N, int Ni, const float* __restrict__ sigma, const float* __restrict__ z,
                                                            size_t z_stride, const float* __restrict__ u, int u_per_ray, float* z_fine,
                                                            float* z_samples, float* weights_out) {
    constexpr int LPR = Seg<RW>::LPR, RPW = Seg<RW>::RPW, Nc = 64 * RW, nb = Nc - 1, np_ = Nc - 2;
    extern __shared__ __attribute__((aligned(16))) float smem_cs[];
    const FourPerLane<RW> lay(N, Nc);                             // idle lanes shadow the last ray (loads in bounds, nothing stored)
    const int lane = lay.lane, wv = threadIdx.x >> 6, sub = lay.seg, sl = lay.sl, ray = lay.ray;
    const bool live = lay.live;
    const int S = Nc + Ni, S4 = (S + 3) / 4 * 4;
    const int slot = wv * RPW + sub;                              // ray slot inside the workgroup
    float* cb = smem_cs + (size_t)slot * coarse_sample_lds_floats(Nc, Ni);
    float* zp = cb + 2 * Nc;                                      // z_k at zp[4 + k]
    float* s2 = zp + Nc + 8;
    float* sorted = s2 + (2 * Ni + 3) / 4 * 4;
    int* hist = (int*)(sorted + S4);
    int* H = (int*)sorted;                                        // [Ni + 1] counters of the inverse-CDF histogram (free until the merge)
    float* up = smem_cs + (size_t)4 * RPW * coarse_sample_lds_floats(Nc, Ni);      // u_i at up[4 + i]
    auto cdfv = [&](int k) -> float { return cb[2 * k]; };
    auto binv = [&](int k) -> float { return cb[2 * k + 1]; };
    auto zv = [&](int k) -> float { return zp[4 + k]; };
    auto allv = [&](int i) -> float { return i < Nc ? zp[4 + i] : s2[2 * (i - Nc)]; };      // cat[z_vals, z_samples]
    const float inf = __builtin_huge_valf();
    if (!u_per_ray) {     // the shared u row, staged once per workgroup: the searches read it in dependent chains (an L2 round trip each otherwise)
        for (int i = threadIdx.x; i < Ni; i += 256) up[4 + i] = u[i];
        if (threadIdx.x < 4) { up[threadIdx.x] = -inf; up[4 + Ni + threadIdx.x] = inf; }
        __syncthreads();
    }
    const uint64_t seg_mask = LPR == 64 ? ~0ull : (((1ull << LPR) - 1ull) << (sub * LPR));

    // ---- compositing, variant D: weights w_k = alpha_k * prod_{j<k} (1 - alpha_j), on the pieces of composite.hip's kernels ----
    const int s0 = 4 * sl;
    float zz[4], z1[4], ss[4], w[4];
    lay.load_z(z + (size_t)ray * z_stride, zz, z1);
    lay.load_row(sigma, (size_t)ray * Nc, ss);
    const float z_next = z1[3];                                               // (unused by a ray's last lane)
    Ray<4> r;
#pragma unroll
    for (int k = 0; k < 4; ++k) sample_alpha(false, true, s0 + k == Nc - 1, zz[k], z1[k], ss[k], 0.f, r, k);
    lay.excl_prod([&](int k) { return (double)(1.f - r.a_c[k]); }, r.T);
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = r.a_c[k] * r.T[k];
    if (weights_out && live) lay.store_row(weights_out, (size_t)ray * Nc, w);

    // ---- bins = z_mid, cdf = [0, cumsum((w[1:-1] + 1e-5) / sum)]  (rendering.py:26-29,132-134; sample_pdf_merge_kernel) ----
    double part = 0.0;
    float pw[4], cd[4], bn[4];                                    // this lane's four (cdf_k, bins_k): kept in registers too
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int kk = s0 + k;
        bn[k] = __fmul_rn(.5f, __fadd_rn(k < 3 ? zz[k + 1] : z_next, zz[k]));
        pw[k] = __fadd_rn(w[k], 1e-5f);
        if (kk >= 1 && kk <= np_) part += (double)pw[k];
    }
    const float total = (float)seg_sum<RW>(part, lane);
    {
        double run[4], acc_ = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int kk = s0 + k;
            if (kk >= 1 && kk <= np_) acc_ += (double)__fdiv_rn(pw[k], total);
            run[k] = acc_;
        }
        const double incl = RW == 1 ? row_incl_sum(acc_) : seg_incl_sum<RW>(acc_, sl);
        const double base = incl - acc_;                          // everything in front of this lane (the f64 sums are exact here)
#pragma unroll
        for (int k = 0; k < 4; ++k) cd[k] = s0 + k == 0 ? 0.f : (float)(base + run[k]);      // (entry Nc - 1 is never read)
    }
    *(float4*)(cb + 2 * s0) = make_float4(cd[0], bn[0], cd[1], bn[1]);
    *(float4*)(cb + 2 * s0 + 4) = make_float4(cd[2], bn[2], cd[3], bn[3]);
    *(float4*)(zp + 4 + s0) = make_float4(zz[0], zz[1], zz[2], zz[3]);
    if (sl == 0) *(float4*)zp = make_float4(-inf, -inf, -inf, -inf);
    if (sl == LPR - 1) *(float4*)(zp + 4 + Nc) = make_float4(inf, inf, inf, inf);
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();

    // ---- inverse-CDF samples (rendering.py:31-64): searchsorted(cdf, u, right=True) = #{k : cdf[k] <= u} ----
    bool okc = true;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float nxt = k < 3 ? cd[k + 1] : (RW == 1 ? row_next(cd[0]) : __shfl_down(cd[0], 1));
        if (s0 + k + 1 < nb) okc = okc && (cd[k] <= nxt);
    }
    const bool cdf_sorted = (__ballot(!okc) & seg_mask) == 0ull;
    // Test time: ONE ascending u row for every ray (linspace, :33).  A lane then owns PL CONSECUTIVE samples and the search is
    // turned around: each lane takes its own four CDF entries and finds j_k = #{i : u_i < cdf_k} -- for an evenly spaced u an
    // arithmetic guess confirmed against the two neighbouring u values (any ascending u stays correct, only slower) -- and
    // cnt_i = #{k : cdf_k <= u_i} = #{k : j_k <= i} is the prefix sum of the histogram of the j's.  No search chains, the same
    // work on every lane, and every table is read and written in 8- and 16-byte groups: the kernel is bound by LDS instructions.
    const int PL = (Ni + LPR - 1) / LPR;                          // samples per lane
    const bool vec = (PL & 3) == 0 && PL * LPR == Ni;             // whole 16-byte groups per lane (Ni = 64, 128, 256 ...)
    bool u_asc = !u_per_ray && cdf_sorted;
    if (u_asc) {
        bool oku = true;
        for (int i = sl; i + 1 < Ni; i += LPR) oku = oku && (up[4 + i] <= up[5 + i]);
        u_asc = (__ballot(!oku) & seg_mask) == 0ull;
    }
    auto sample_of = [&](float uu, int cnt) {
        const int below = cnt - 1 > 0 ? cnt - 1 : 0;               // :52-53
        const int above = cnt < nb - 1 ? cnt : nb - 1;
        // above is below + 1 except at the two ends, where it equals below: ONE paired read of entries (below, below + 1)
        const float2 lo = *(const float2*)(cb + 2 * below), nx = *(const float2*)(cb + 2 * below + 2);
        const float2 hi = above == below ? lo : nx;
        float denom = __fsub_rn(hi.x, lo.x);                       // :60-64
        denom = denom < 1e-5f ? 1.f : denom;
        const float t = __fdiv_rn(__fsub_rn(uu, lo.x), denom);
        return __fadd_rn(lo.y, __fmul_rn(t, __fsub_rn(hi.y, lo.y)));
    };
    const int i_lo = sl * PL, i_hi = (i_lo + PL) < Ni ? (i_lo + PL) : Ni;
    if (u_asc) {
        if (vec) { for (int i = i_lo; i < i_hi; i += 4) *(int4*)(H + i) = make_int4(0, 0, 0, 0); if (sl == 0) H[Ni] = 0; }
        else for (int i = sl; i < Ni + 1; i += LPR) H[i] = 0;
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        const float span = (float)(Ni - 1);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (s0 + k >= nb) continue;
            const float c = cd[k];
            int j = (int)ceilf(c * span);
            j = j < 0 ? 0 : (j > Ni ? Ni : j);
            for (;;) {                                             // j = #{i : u_i < c}  <=>  u_{j-1} < c and not u_j < c  (sentinels at both ends)
                const float below = up[3 + j], at = up[4 + j];
                if (at < c) ++j; else if (!(below < c)) --j; else break;
            }
            atomicAdd(&H[j], 1);
        }
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        int run = 0;
        if (vec) for (int i = i_lo; i < i_hi; i += 4) { const int4 h = *(const int4*)(H + i); run += (h.x + h.y) + (h.z + h.w); }
        else for (int i = i_lo; i < i_hi; ++i) run += H[i];
        int incl = run;
        if (RW == 1) incl = row_incl_sum(run);
        else {
#pragma unroll
            for (int o = 1; o < LPR; o <<= 1) {
                const int t = __shfl_up(incl, o);
                if (sl >= o) incl += t;
            }
        }
        int cnt = incl - run;
        for (int i0 = i_lo; i0 < i_hi; i0 += 4) {                  // four samples at a time: counts, table reads, arithmetic, one 32-byte store
            int cn[4];
            float uu[4], smp[4];
            if (vec) {
                const int4 h = *(const int4*)(H + i0);
                const float4 u4 = *(const float4*)(up + 4 + i0);
                cn[0] = cnt + h.x; cn[1] = cn[0] + h.y; cn[2] = cn[1] + h.z; cn[3] = cn[2] + h.w;
                uu[0] = u4.x; uu[1] = u4.y; uu[2] = u4.z; uu[3] = u4.w;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = i0 + e < Ni ? i0 + e : Ni - 1;
                    cnt += i0 + e < i_hi ? H[i] : 0;
                    cn[e] = cnt;
                    uu[e] = up[4 + i];
                }
            }
            cnt = cn[3];
#pragma unroll
            for (int e = 0; e < 4; ++e) smp[e] = sample_of(uu[e], cn[e]);
            if (vec) {
                *(float4*)(s2 + 2 * i0) = make_float4(smp[0], __int_as_float(cn[0]), smp[1], __int_as_float(cn[1]));
                *(float4*)(s2 + 2 * i0 + 4) = make_float4(smp[2], __int_as_float(cn[2]), smp[3], __int_as_float(cn[3]));
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i0 + e < i_hi) {
                    if (!vec) { s2[2 * (i0 + e)] = smp[e]; s2[2 * (i0 + e) + 1] = __int_as_float(cn[e]); }
                    if (z_samples && live) z_samples[(size_t)ray * Ni + i0 + e] = smp[e];
                }
        }
    } else {
        for (int i0 = sl; i0 < Ni; i0 += 2 * LPR) {               // two samples per lane and pass, searched side by side
            const int ii[2] = {i0, i0 + LPR};
            float uu[2];
            int cnt[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int i = ii[e] < Ni ? ii[e] : Ni - 1;
                uu[e] = u_per_ray ? u[(size_t)ray * Ni + i] : up[4 + i];
            }
            if (cdf_sorted && uu[0] == uu[0] && uu[1] == uu[1]) {
                int lo0 = 0, hi0 = nb, lo1 = 0, hi1 = nb;
                while (lo0 < hi0 || lo1 < hi1) {
                    const int m0 = (lo0 + hi0) >> 1, m1 = (lo1 + hi1) >> 1;
                    const float c0 = cdfv(m0 < nb ? m0 : nb - 1), c1 = cdfv(m1 < nb ? m1 : nb - 1);
                    if (lo0 < hi0) { if (c0 <= uu[0]) lo0 = m0 + 1; else hi0 = m0; }
                    if (lo1 < hi1) { if (c1 <= uu[1]) lo1 = m1 + 1; else hi1 = m1; }
                }
                cnt[0] = lo0; cnt[1] = lo1;
            } else {
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    cnt[e] = 0;
                    for (int k = 0; k < nb; ++k) cnt[e] += (cdfv(k) <= uu[e]) ? 1 : 0;
                }
            }
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                if (ii[e] >= Ni) continue;
                const float smp = sample_of(uu[e], cnt[e]);
                s2[2 * ii[e]] = smp;
                s2[2 * ii[e] + 1] = __int_as_float(cnt[e]);
                if (z_samples && live) z_samples[(size_t)ray * Ni + ii[e]] = smp;
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();

    // ---- stable rank sort of cat[z_coarse, z_samples] (rendering.py:141), as sample_pdf_merge_kernel ----
    bool oka = true;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (s0 + k + 1 < Nc) oka = oka && (zz[k] <= (k < 3 ? zz[k + 1] : z_next));
    for (int k = sl; k + 1 < Ni; k += LPR) oka = oka && (s2[2 * k] <= s2[2 * k + 2]);
    const bool ordered = (__ballot(!oka) & seg_mask) == 0ull;
    if (ordered) {
        // Both halves ascending.  A sample's rank is its index + c, c = #{coarse <= sample}: the sample was interpolated between the
        // midpoints bins[below] >= z[below] and bins[above] <= z[below + 2], so c is below + 1 or below + 2 -- one paired read of
        // (z[c - 1], z[c]) decides, a walk covers the rest.  A coarse depth's rank is its index + #{samples < z_k} =
        // #{samples : c <= k} (z ascending): a histogram of the c's and its prefix sum over the ray's lanes.
        *(int4*)(hist + s0) = make_int4(0, 0, 0, 0);
        if (sl == 0) *(int4*)(hist + Nc) = make_int4(0, 0, 0, 0);
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        for (int i0 = i_lo; i0 < i_hi; i0 += 4) {
            float v[4];
            int c[4];
            if (vec) {
                const float4 a4 = *(const float4*)(s2 + 2 * i0), b4 = *(const float4*)(s2 + 2 * i0 + 4);
                v[0] = a4.x; v[1] = a4.z; v[2] = b4.x; v[3] = b4.z;
                c[0] = __float_as_int(a4.y); c[1] = __float_as_int(a4.w); c[2] = __float_as_int(b4.y); c[3] = __float_as_int(b4.w);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int i = i0 + e < Ni ? i0 + e : Ni - 1;
                    v[e] = s2[2 * i];
                    c[e] = __float_as_int(s2[2 * i + 1]);
                }
            }
            float lo[4], hi[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                c[e] = c[e] > 1 ? c[e] : 1;
                lo[e] = zp[3 + c[e]];                              // z[c - 1]
                hi[e] = zp[4 + c[e]];                              // z[c]  (+inf behind the last one)
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (hi[e] <= v[e]) { ++c[e]; while (zp[4 + c[e]] <= v[e]) ++c[e]; }
                else if (!(lo[e] <= v[e])) { --c[e]; while (c[e] > 0 && !(zp[3 + c[e]] <= v[e])) --c[e]; }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (i0 + e < i_hi) {
                    sorted[i0 + e + c[e]] = v[e];
                    atomicAdd(&hist[c[e]], 1);
                }
        }
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        const int4 h4 = *(const int4*)(hist + s0);
        const int r0 = h4.x, r1 = r0 + h4.y, r2 = r1 + h4.z, r3 = r2 + h4.w;
        int incl = r3;                                             // inclusive scan of the lanes' totals over the ray
        if (RW == 1) incl = row_incl_sum(r3);
        else {
#pragma unroll
            for (int o = 1; o < LPR; o <<= 1) {
                const int t = __shfl_up(incl, o);
                if (sl >= o) incl += t;
            }
        }
        const int base = incl - r3;
        sorted[s0 + base + r0] = zz[0];
        sorted[s0 + 1 + base + r1] = zz[1];
        sorted[s0 + 2 + base + r2] = zz[2];
        sorted[s0 + 3 + base + r3] = zz[3];
    } else {
        for (int i = sl; i < S; i += LPR) {
            const float v = allv(i);
            const bool v_nan = v != v;
            int rank = 0;
            for (int k = 0; k < S; ++k) {
                const float o = allv(k);
                const bool o_nan = o != o;
                const bool before = v_nan ? (!o_nan || k < i) : (!o_nan && (o < v || (o == v && k < i)));
                rank += before ? 1 : 0;
            }
            sorted[rank] = v;
        }
    }
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    if (live) {
        if ((S & 3) == 0) {                                        // whole 16-byte groups: 16 LPR bytes of a ray's row per instruction
            for (int i = 4 * sl; i < S; i += 4 * LPR) *(float4*)(z_fine + (size_t)ray * S + i) = *(const float4*)(sorted + i);
        } else {
            for (int i = sl; i < S; i += LPR) z_fine[(size_t)ray * S + i] = sorted[i];
        }
    }
}

template <int RW>
static int launch_coarse_sample(int N, int Ni, const float* sigma, const float* z, size_t z_stride, const float* u, int u_per_ray,
                                float* z_fine, float* z_samples, float* weights_out, hipStream_t st) {
    constexpr int RPW = Seg<RW>::RPW, Nc = 64 * RW;
    const size_t lds = ((size_t)4 * RPW * coarse_sample_lds_floats(Nc, Ni) + (size_t)coarse_sample_u_floats(Ni)) * sizeof(float);
    auto k = coarse_sample_kernel<RW>;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(k, dim3((N + 4 * RPW - 1) / (4 * RPW)), dim3(256), lds, st, N, Ni, sigma, z, z_stride, u, u_per_ray, z_fine,
                       z_samples, weights_out);
    return (int)hipGetLastError();
}

extern "C" int nefes_coarse_sample(int N, int Nc, int Ni, const float* sigma, const float* z, int z_shared_row, const float* u,
                                   int u_per_ray, float* z_fine, float* z_samples, float* weights_out, void* stream) {
    if (!sigma || !z || !u || !z_fine || N <= 0 || Ni <= 0) return NEFES_E_BADARG;
    if (Nc + Ni > SP_MAX_S) return NEFES_E_UNSUPPORTED;
    if (((uintptr_t)sigma | (uintptr_t)z | (uintptr_t)weights_out) & 15) return NEFES_E_BADARG;      // 16-byte row loads
    const size_t zs = z_shared_row ? 0 : (size_t)Nc;
    hipStream_t st = (hipStream_t)stream;
    switch (Nc) {
        case 64: return launch_coarse_sample<1>(N, Ni, sigma, z, zs, u, u_per_ray, z_fine, z_samples, weights_out, st);
        case 128: return launch_coarse_sample<2>(N, Ni, sigma, z, zs, u, u_per_ray, z_fine, z_samples, weights_out, st);
        case 256: return launch_coarse_sample<4>(N, Ni, sigma, z, zs, u, u_per_ray, z_fine, z_samples, weights_out, st);
    }
    return NEFES_E_UNSUPPORTED;                                   // other coarse counts: composite D + nefes_sample_pdf_merge
}

extern "C" int nefes_sample_pdf_merge(int N, int Nc, int Ni, int layout, const float* z_coarse, const float* weights,
                                      const float* u, int u_per_ray, const float* cdf_in, float* z_fine, float* z_samples,
                                      int32_t* inds, float* cdf_out, void* stream) {
    if (!z_coarse || !weights || !u || N <= 0 || Nc < 3 || Ni <= 0) return NEFES_E_BADARG;
    if (layout != 0 && (layout != 1 || z_fine)) return NEFES_E_BADARG;
    if (Nc > SP_MAX_NC || Nc + Ni > SP_MAX_S) return NEFES_E_UNSUPPORTED;
    hipLaunchKernelGGL(sample_pdf_merge_kernel, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, N, Nc, Ni, layout, z_coarse,
                       weights, u, u_per_ray, cdf_in, z_fine, z_samples, inds, cdf_out);
    return (int)hipGetLastError();
}

// Alpha compositing of RGB + C-channel feature maps and its backward.
// Restates raw2outputs_NeRFH_NFF (script/models/nerfh_nff.py:25-166), variants A/B/C/D of SURVEY.md §8 a9.
//
// Structure: every formula is stated ONCE, as a __device__ function of one sample's values or of the K sample slots of a lane, and the
// two kernel templates composite_fwd_kernel<Layout> / composite_bwd_kernel<Layout> are specialised on nothing but the layout.  The
// forward has one body for both layouts.  The backward has the formulas in common and one body per layout (ray_backward): how a body
// walks its slots decides registers and time, see there.
//
// The layouts (composite.h): OnePerLane<Q> (one sample per lane, Q passes of 64 lanes, any S <= 512; one wavefront per ray) moves
// 4 bytes per lane and load instruction and walks a ray in Q passes of scans; FourPerLane<RW> (four CONSECUTIVE samples per lane, S = 64 RW up to
// 256, 16-byte aligned pointers) reads every row of a ray as one 16-byte load per lane, scans with four in-lane products plus ONE
// cross-lane scan, and packs 4 / RW rays into a wave.  The launchers choose from what they can see (S % 64, S <= 256, alignment).
//
// Roofline: HBM-bound.  Algorithmic bytes per ray: forward S*R*4 + S*4 read + (3+C+3)*4 write
// (20.1 KB at S=192, R=25); backward 2*S*R*4 + small (38.5 KB).  raw_t is channel-major per ray
// ([N][R][S]) so that lane <-> sample gives coalesced rows per channel.
//
// Numerics follow the CPU reference: transmittance = exclusive cumprod accumulated in f64 and rounded
// to f32 per element (torch CPU cumprod semantics); per-ray sums accumulate in f64.
// The backward is division-free (exact for alpha == 1 saturation; SURVEY.md §7 hard part 5).
#include <type_traits>
#include "../../include/nefes_hip.h"
#include "composite.h"

struct CompArgs {
    int N, S, C, R;
    uint32_t flags;
    float beta_min;
    const float* raw_t;
    const float* z;
    // forward outputs (nullable)
    float *rgb, *feat, *disp, *acc, *depth, *weights, *beta;
    // backward inputs (nullable) and output
    const float *g_rgb, *g_feat, *g_disp, *g_acc, *g_depth, *g_weights, *g_beta;
    float* g_raw_t;
};

struct CompFlags {
    bool transient, sigma_only, static_only;
    bool both;                 // variant A: static + transient
    bool white;                // white background, which only variant A renders
    bool feat_weights_only;
    __device__ __forceinline__ explicit CompFlags(uint32_t f)
        : transient(f & NEFES_COMP_TRANSIENT), sigma_only(f & NEFES_COMP_SIGMA_ONLY), static_only(f & NEFES_COMP_STATIC_ONLY),
          both(transient && !static_only), white((f & NEFES_COMP_WHITE_BKGD) && both), feat_weights_only(f & NEFES_COMP_FEAT_WEIGHTS_ONLY) {}
};

// torch.max(1e-10, x) propagates NaN
__device__ __forceinline__ float max_nan(float lo, float x) { return (x != x) ? x : (x > lo ? x : lo); }

// alphas and transmittances of a ray: T = exclusive cumprod of (1 - alpha) (:71-72), Ts = variant B's second chain (:95-98)
// (one sample per lane in the forward kernel: every row of every pass requested first, no exchange between lanes waits for them)
template <class L>
__device__ __forceinline__ void ray_forward(const L& l, const CompFlags& f, const CompArgs& p, const float* raw, const float* zr, Ray<L::K>& r) {
    constexpr int K = L::K;
    const int S = p.S, C3 = 3 + p.C;
    const int chS = f.sigma_only ? 0 : C3, chT = C3 + 4;
    float z0[K], z1[K], ss[K], st[K];
    l.load_z(zr, z0, z1);
    l.load_row(raw, (size_t)chS * S, ss);
#pragma unroll
    for (int k = 0; k < K; ++k) st[k] = 0.f;
    if (f.transient) l.load_row(raw, (size_t)chT * S, st);
#pragma unroll
    for (int k = 0; k < K; ++k) sample_alpha(f.transient, l.in(k), l.sample(k) == S - 1, z0[k], z1[k], ss[k], st[k], r, k);
    l.excl_prod([&](int k) { return l.in(k) ? (double)(1.f - r.a_c[k]) : 1.0; }, r.T);
    if (f.static_only) {
        l.excl_prod([&](int k) { return l.in(k) ? (double)(1.f - r.a_s[k]) : 1.0; }, r.Ts);
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) r.Ts[k] = r.T[k];
    }
}

// the same for one sample per lane, pass by pass: a pass reads its samples, forms their alphas and scans them before the next one
// starts.  The backward's form: slower than requesting every row first (1 to 3 %), but with fewer values in flight, which the backward
// needs for its registers.
template <int Q>
__device__ __forceinline__ void ray_forward_by_pass(const OnePerLane<Q>& l, const CompFlags& f, const CompArgs& p, const float* raw, const float* zr, Ray<Q>& r) {
    const int S = p.S, C3 = 3 + p.C;
    const int chS = f.sigma_only ? 0 : C3, chT = C3 + 4;
    double carry = 1.0, carry_s = 1.0;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const bool in = l.in(q);
        const int sc = in ? l.sample(q) : S - 1;
        const float z0 = zr[sc];
        const float z1 = zr[sc + 1 < S ? sc + 1 : sc];
        const float ss = raw[(size_t)chS * S + sc];
        const float st = f.transient ? raw[(size_t)chT * S + sc] : 0.f;
        sample_alpha(f.transient, in, sc == S - 1, z0, z1, ss, st, r, q);
        r.T[q] = l.excl_pass(in ? (double)(1.f - r.a_c[q]) : 1.0, carry);
        r.Ts[q] = f.static_only ? l.excl_pass(in ? (double)(1.f - r.a_s[q]) : 1.0, carry_s) : r.T[q];
    }
}

// the same for four samples per lane, in that layout's own order: the three rows requested before the depths are exchanged, both
// chains' factors formed in one sweep
template <int RW>
__device__ __forceinline__ void ray_forward(const FourPerLane<RW>& l, const CompFlags& f, const CompArgs& p, const float* raw, const float* zr, Ray<4>& r) {
    const int S = p.S, C3 = 3 + p.C;
    const int chS = f.sigma_only ? 0 : C3, chT = C3 + 4;
    const typename FourPerLane<RW>::Row z4 = l.row(zr, 0), ss4 = l.row(raw, (size_t)chS * S), st4 = l.row_if(f.transient, raw, (size_t)chT * S);
    const float z_next = l.next_lane(l.at(z4, 0));                     // first depth of the next lane's group
    double om[4], oms[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        sample_alpha(f.transient, true, l.sample(k) == S - 1, l.at(z4, k), k < 3 ? l.at(z4, k + 1) : z_next, l.at(ss4, k), l.at(st4, k), r, k);
        om[k] = (double)(1.f - r.a_c[k]);
        oms[k] = (double)(1.f - r.a_s[k]);
    }
    l.excl_prod([&](int k) { return om[k]; }, r.T);
    if (f.static_only) {
        l.excl_prod([&](int k) { return oms[k]; }, r.Ts);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) r.Ts[k] = r.T[k];
    }
}

// combined, static, transient and the "reported" weights of the lane's slots, and the lane's share of the three per-ray sums
template <int K>
struct Weights {
    float w[K], ws[K], wt[K], wo[K];
    double s_acc, s_dep, s_wo;
};
template <class L>
__device__ __forceinline__ void ray_weights(const L& l, const CompFlags& f, const Ray<L::K>& r, Weights<L::K>& o) {
    o.s_acc = 0; o.s_dep = 0; o.s_wo = 0;
#pragma unroll
    for (int k = 0; k < L::K; ++k) {
        o.w[k] = r.a_c[k] * r.T[k];
        o.ws[k] = f.static_only ? r.a_s[k] * r.Ts[k] : (f.transient ? r.a_s[k] * r.T[k] : o.w[k]);
        o.wt[k] = f.both ? r.a_t[k] * r.T[k] : 0.f;
        o.wo[k] = f.static_only ? o.ws[k] : o.w[k];
        if (l.in(k)) {
            o.s_acc += o.w[k];
            o.s_wo += o.wo[k];
            o.s_dep += (double)(o.wo[k] * r.zz[k]);
        }
    }
}

// sum over the ray of weight x row, f64 accumulate
template <class L>
__device__ __forceinline__ float ray_dot(const L& l, const float (&w)[L::K], const typename L::Row& row) {
    double a = 0;
#pragma unroll
    for (int k = 0; k < L::K; ++k)
        if (l.in(k)) a += (double)(w[k] * l.at(row, k));
    return (float)l.sum(a);
}

template <class L>
__global__ __launch_bounds__(256) void composite_fwd_kernel(CompArgs p) {
    constexpr int K = L::K;
    const L l(p.N, p.S);
    if (l.idle()) return;
    const CompFlags f(p.flags);
    const int S = p.S, C = p.C, C3 = 3 + C, ray = l.ray;
    const float* raw = p.raw_t + (size_t)ray * p.R * S;
    const float* zr = p.z + (size_t)ray * S;
    // blockIdx.y splits the FEATURE channels of a ray over several workgroups (small frames with many channels: the 80x60
    // refinement frame has 4800 rays x 128 channels, i.e. five waves per SIMD walking 131 reductions each); split 0 also writes
    // everything else.  Every split recomputes the ray's weights (two scans: small next to its share of the channels).
    const int split = blockIdx.y, n_split = gridDim.y;
    const bool lead = split == 0;
    Ray<K> r;
    ray_forward(l, f, p, raw, zr, r);
    Weights<K> w;
    ray_weights(l, f, r, w);
    if (p.weights && lead && l.live) l.store_row(p.weights, (size_t)ray * S, w.wo);
    const float acc = (float)l.sum(w.s_acc);
    if (l.sl == 0 && p.acc && lead && l.live) p.acc[ray] = acc;
    if (f.sigma_only) return;                                              // variant D: weights + acc only (:83-89)
    if (lead) {
        const float depth = (float)l.sum(w.s_dep);
        const float sum_wo = f.static_only ? (float)l.sum(w.s_wo) : acc;
        if (l.sl == 0 && l.live) {
            if (p.depth) p.depth[ray] = depth;
            if (p.disp) p.disp[ray] = 1.f / max_nan(1e-10f, depth / sum_wo);   // :115,165
        }
        // rgb = sum w_s * c_s (+ sum w_t * c_t) (:119-131,149 / :101-105 / :153-154)
        typename L::Row c_s[3], c_t[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            c_s[c] = l.row(raw, (size_t)c * S);
            if (f.both) c_t[c] = l.row(raw, (size_t)(C3 + 1 + c) * S);
        }
        float rgb_keep = 0.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = ray_dot(l, w.ws, c_s[c]);
            if (f.white) v = v + (1.f - acc);
            if (f.both) v = v + ray_dot(l, w.wt, c_t[c]);
            if (l.sl == c) rgb_keep = v;
        }
        if (l.sl < 3 && p.rgb && l.live) p.rgb[(size_t)ray * 3 + l.sl] = rgb_keep;
    }
    // features use the same (static) weights, detached (:108-111,122-125,155-157): L::LANES channels per round, one kept per lane,
    // L::AHEAD rows requested before the first is consumed
    if (p.feat) {
        const int per = ((C + n_split - 1) / n_split + 31) / 32 * 32;      // whole 32-channel groups per split
        const int c_lo = split * per, c_hi = (c_lo + per) < C ? (c_lo + per) : C;
        for (int c0 = c_lo; c0 < c_hi; c0 += L::LANES) {
            float keep = 0.f;
            const int nc = (c_hi - c0) < L::LANES ? (c_hi - c0) : L::LANES;
            for (int cb = 0; cb < nc; cb += L::AHEAD) {
                typename L::Row row[L::AHEAD];
#pragma unroll
                for (int i = 0; i < L::AHEAD; ++i) {
                    const int c = cb + i < nc ? cb + i : nc - 1;
                    row[i] = l.row(raw, (size_t)(3 + c0 + c) * S);
                }
#pragma unroll
                for (int i = 0; i < L::AHEAD; ++i) {
                    const float v = ray_dot(l, w.ws, row[i]);
                    if (l.sl == cb + i) keep = v;
                }
            }
            if (l.sl < nc && l.live) p.feat[(size_t)ray * C + c0 + l.sl] = keep;
        }
    }
    if (p.beta && lead) {
        float bv = 0.f;
        if (f.both) {
            bv = ray_dot(l, w.wt, l.row(raw, (size_t)(C3 + 5) * S)) + p.beta_min;      // :133-137
        }
        if (l.sl == 0 && l.live) p.beta[ray] = bv;
    }
}

// ---- backward ----
// The formulas of the backward are stated once, as functions of one sample's values; the two layouts keep their own kernel bodies
// (ray_backward below), because how a body walks its slots -- where rows are requested relative to the scans, one slot at a time or
// four at once -- decides registers and time (profiles/composite_one_algebra/README.md).

// upstream scalars of a ray, with d loss / d disp folded into d depth and d (sum of reported weights), and white_bkgd and the
// shared sum of variants A / C folded into g_acc
struct UpScalars {
    float g_rgb[3], g_acc, g_dep, g_beta, g_sumwo;
};
__device__ __forceinline__ void load_up_scalars(const CompFlags& f, const CompArgs& p, int ray, float depth, float sum_wo, UpScalars& u) {
    u.g_rgb[0] = u.g_rgb[1] = u.g_rgb[2] = 0.f;
    if (p.g_rgb && !f.sigma_only)
#pragma unroll
        for (int c = 0; c < 3; ++c) u.g_rgb[c] = p.g_rgb[(size_t)ray * 3 + c];
    u.g_acc = p.g_acc ? p.g_acc[ray] : 0.f;
    u.g_dep = (p.g_depth && !f.sigma_only) ? p.g_depth[ray] : 0.f;
    u.g_beta = (p.g_beta && f.both) ? p.g_beta[ray] : 0.f;
    u.g_sumwo = 0.f;   // gradient w.r.t. the disparity denominator
    if (p.g_disp && !f.sigma_only) {
        const float gd = p.g_disp[ray];
        const float ratio = depth / sum_wo;
        if (ratio > 1e-10f || ratio != ratio) {           // torch.max passes the gradient to the larger operand
            const float disp = 1.f / ratio;
            const float g_ratio = -gd * disp * disp;
            u.g_dep += g_ratio / sum_wo;
            u.g_sumwo += -g_ratio * ratio / sum_wo;
        }
    }
    if (f.white) u.g_acc -= (u.g_rgb[0] + u.g_rgb[1] + u.g_rgb[2]);
    if (!f.static_only) { u.g_acc += u.g_sumwo; u.g_sumwo = 0.f; }   // same tensor (sum of combined weights) in A/C
}

// d loss / d (static, transient, combined, variant B's own) weight of one sample, from its upstream colour terms
// col_s = g_rgb . static colour, col_t = g_rgb . transient colour, its beta, its d loss / d weight and its depth
struct UpSample {
    float Gs, Gt, Gc, G1;
};
__device__ __forceinline__ UpSample sample_upstream(const CompFlags& f, const UpScalars& u, float col_s, float col_t, float beta, float gw, float zz) {
    UpSample g = {0.f, 0.f, 0.f, 0.f};
    if (f.both) {                     // variant A
        g.Gs = col_s;
        g.Gt = col_t + u.g_beta * beta;
        g.Gc = u.g_acc + u.g_dep * zz + gw;
    } else if (f.static_only) {       // variant B
        g.G1 = col_s + u.g_dep * zz + u.g_sumwo + gw;
        g.Gc = u.g_acc;
    } else {                          // variants C / D
        g.Gc = col_s + u.g_acc + u.g_dep * zz + gw;
    }
    return g;
}
// (the same, the colour terms summed here from colours given as cs(c), ct(c), beta())
template <class Cs, class Ct, class Beta>
__device__ __forceinline__ UpSample sample_upstream(const CompFlags& f, const UpScalars& u, Cs&& cs, Ct&& ct, Beta&& beta, float gw, float zz) {
    float col_s = 0.f, col_t = 0.f;
    if (!f.sigma_only) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            col_s += u.g_rgb[c] * cs(c);
            if (f.both) col_t += u.g_rgb[c] * ct(c);
        }
    }
    return sample_upstream(f, u, col_s, col_t, f.both ? beta() : 0.f, gw, zz);
}
// the affine maps of the reverse scans X_i = a_i + m_i X_{i+1}: the combined chain, and variant B's own
__device__ __forceinline__ void scan_map(const CompFlags& f, bool in, const UpSample& g, float a_c, float a_s, float a_t, double& m, double& a) {
    m = in ? (double)(1.f - a_c) : 1.0;
    a = in ? (double)g.Gs * a_s * (f.both ? 1.0 : 0.0) + (double)g.Gt * a_t + (double)g.Gc * a_c : 0.0;
}
__device__ __forceinline__ void scan_map1(bool in, const UpSample& g, float a_s, double& m, double& a) {
    m = in ? (double)(1.f - a_s) : 1.0;
    a = in ? (double)g.G1 * a_s : 0.0;
}
// d loss / d alpha -> d loss / d sigma_static and sigma_transient of one sample; Bc, B1 = X_{i+1} of the two chains
struct AlphaGrad {
    double d_ac, d_as, d_at;         // d L / d alpha: combined, static, transient
};
template <class R>
__device__ __forceinline__ AlphaGrad alpha_grad(const CompFlags& f, const UpSample& g, const R& r, int k, double Bc, double B1) {
    const double T = r.T[k], Ts = r.Ts[k];
    AlphaGrad d = {(double)g.Gc * T - T * Bc, 0.0, 0.0};
    if (f.both) { d.d_as = (double)g.Gs * T; d.d_at = (double)g.Gt * T; }
    if (f.static_only) d.d_as = (double)g.G1 * Ts - Ts * B1;
    return d;
}
template <class R>
__device__ __forceinline__ float sigma_static_grad(const CompFlags& f, const AlphaGrad& d, const R& r, int k) {
    const double dl = r.dl[k];
    return (float)(f.transient ? d.d_as * dl * r.e_s[k] + d.d_ac * dl * r.e_c[k] : d.d_ac * dl * r.e_c[k]);
}
template <class R>
__device__ __forceinline__ float sigma_transient_grad(const AlphaGrad& d, const R& r, int k) {
    const double dl = r.dl[k];
    return (float)(d.d_at * dl * r.e_t[k] + d.d_ac * dl * r.e_c[k]);
}
// the rows of g_raw_t: put(channel row, value of slot k) for every row a ray gets.  ws / wt: static / transient weight of slot k,
// g_ss / g_st: its two sigma gradients.
template <class Ws, class Wt, class Gss, class Gst, class Put>
__device__ __forceinline__ void g_raw_rows(const CompFlags& f, const CompArgs& p, int ray, const UpScalars& u, Ws&& ws, Wt&& wt, Gss&& g_ss,
                                           Gst&& g_st, Put&& put) {
    const int C = p.C, C3 = 3 + C;
    if (f.sigma_only) { put(0, g_ss); return; }
    put(C3, g_ss);
#pragma unroll
    for (int c = 0; c < 3; ++c) put(c, [&](int k) { return ws(k) * u.g_rgb[c]; });
    if (f.feat_weights_only) {
        // the factored head (field_bwd_h3.hip FH): d loss / d feature channel c at sample s is w_s[s] g_feat[c], which the field backward
        // forms itself from g_feat (one row per RAY) and the static weight -- written HERE, into the first feature channel's row, in
        // place of C rows of products
        put(3, ws);
    } else {
        for (int c = 0; c < C; ++c) {
            const float gfc = p.g_feat ? p.g_feat[(size_t)ray * C + c] : 0.f;
            put(3 + c, [&](int k) { return p.g_feat ? ws(k) * gfc : 0.f; });
        }
    }
    if (f.transient) {
#pragma unroll
        for (int c = 0; c < 3; ++c) put(C3 + 1 + c, [&](int k) { return wt(k) * u.g_rgb[c]; });
        put(C3 + 4, g_st);
        put(C3 + 5, [&](int k) { return wt(k) * u.g_beta; });
    }
}

// ---- the backward of a ray, one body per layout ----
// One sample per lane, in the order of the kernel it replaces: the forward pass by pass, a slot's rows read where its upstream is
// formed (slots beyond S skipped), both reverse chains pass by pass, then slot by slot the gradients and all of the slot's rows, the
// transient sigma gradient formed only where it is stored.  The two-pass instance has no register to spare for its eight waves per
// SIMD, and two shared pieces each cost it one: the row plan as g_raw_rows, and the upstream's colour sums inside sample_upstream.
// So the row plan is written out here, in g_raw_rows' order.
template <int Q>
__device__ __forceinline__ void ray_backward(const OnePerLane<Q>& l, const CompFlags& f, const CompArgs& p) {
    const int lane = l.lane, ray = l.ray;
    const int S = p.S, C = p.C, C3 = 3 + C;
    const float* raw = p.raw_t + (size_t)ray * p.R * S;
    float* graw = p.g_raw_t + (size_t)ray * p.R * S;
    Ray<Q> r;
    ray_forward_by_pass(l, f, p, raw, p.z + (size_t)ray * S, r);
    Weights<Q> w;
    ray_weights(l, f, r, w);
    const float acc = (float)l.sum(w.s_acc);
    const float depth = (float)l.sum(w.s_dep);
    const float sum_wo = f.static_only ? (float)l.sum(w.s_wo) : acc;
    UpScalars u;
    load_up_scalars(f, p, ray, depth, sum_wo, u);

    float Gs[Q], Gt[Q], Gc[Q], G1[Q];      // (four arrays, not UpSample[Q]: that form costs the two-pass instance its eighth wave)
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int s = lane + 64 * q;
        Gs[q] = Gt[q] = Gc[q] = G1[q] = 0.f;
        if (l.in(q)) {
            const float gw = p.g_weights ? p.g_weights[(size_t)ray * S + s] : 0.f;
            float col_s = 0.f, col_t = 0.f;
            if (!f.sigma_only) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    col_s += u.g_rgb[c] * raw[(size_t)c * S + s];
                    if (f.both) col_t += u.g_rgb[c] * raw[(size_t)(C3 + 1 + c) * S + s];
                }
            }
            const UpSample g = sample_upstream(f, u, col_s, col_t, f.both ? raw[(size_t)(C3 + 5) * S + s] : 0.f, gw, r.zz[q]);
            Gs[q] = g.Gs; Gt[q] = g.Gt; Gc[q] = g.Gc; G1[q] = g.G1;
        }
    }
    double Bc[Q], B1[Q], carry = 0.0, carry1 = 0.0;
#pragma unroll
    for (int q = Q - 1; q >= 0; --q) {
        double m, a;
        const UpSample g = {Gs[q], Gt[q], Gc[q], G1[q]};
        scan_map(f, l.in(q), g, r.a_c[q], r.a_s[q], r.a_t[q], m, a);
        Bc[q] = l.rev_pass(m, a, carry);
        B1[q] = 0.0;
        if (f.static_only) {
            scan_map1(l.in(q), g, r.a_s[q], m, a);
            B1[q] = l.rev_pass(m, a, carry1);
        }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        if (!l.in(q)) continue;
        const int s = lane + 64 * q;
        const UpSample g = {Gs[q], Gt[q], Gc[q], G1[q]};
        const AlphaGrad d = alpha_grad(f, g, r, q, Bc[q], B1[q]);
        const float g_ss = sigma_static_grad(f, d, r, q);
        if (f.sigma_only) { graw[s] = g_ss; continue; }
        graw[(size_t)C3 * S + s] = g_ss;
#pragma unroll
        for (int c = 0; c < 3; ++c) graw[(size_t)c * S + s] = w.ws[q] * u.g_rgb[c];
        if (f.feat_weights_only) {
            graw[(size_t)3 * S + s] = w.ws[q];
        } else {
            for (int c = 0; c < C; ++c) graw[(size_t)(3 + c) * S + s] = p.g_feat ? w.ws[q] * p.g_feat[(size_t)ray * C + c] : 0.f;
        }
        if (f.transient) {
#pragma unroll
            for (int c = 0; c < 3; ++c) graw[(size_t)(C3 + 1 + c) * S + s] = w.wt[q] * u.g_rgb[c];
            graw[(size_t)(C3 + 4) * S + s] = sigma_transient_grad(d, r, q);
            graw[(size_t)(C3 + 5) * S + s] = w.wt[q] * u.g_beta;
        }
    }
}

// the nine rows of a ray that FourPerLane's upstream reads, held as 16-byte vectors across the scans
template <int RW>
struct UpRows {
    typename FourPerLane<RW>::Row cs[3], ct[3], b, gw;
};
// four samples per lane: the nine rows the upstream reads are requested before the scans, idle lanes leave only after the scans, and
// every row of g_raw_t is one 16-byte store per lane
template <int RW>
__device__ __forceinline__ void request_up_rows(const FourPerLane<RW>& l, const CompFlags& f, const CompArgs& p, const float* raw,
                                                UpRows<RW>& rows) {
    const int S = p.S, C3 = 3 + p.C;
    if (!f.sigma_only) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            rows.cs[c] = l.row(raw, (size_t)c * S);
            if (f.both) rows.ct[c] = l.row(raw, (size_t)(C3 + 1 + c) * S);
        }
    }
    rows.b = l.row_if(f.both && !f.sigma_only, raw, (size_t)(C3 + 5) * S);
    rows.gw = l.row_if(p.g_weights, p.g_weights, (size_t)l.ray * S);
}
template <int RW>
__device__ __forceinline__ void upstream_to_rows(const FourPerLane<RW>& l, const CompFlags& f, const CompArgs& p, const UpRows<RW>& rows,
                                                 float* graw, const Ray<4>& r, const Weights<4>& w, const UpScalars& u) {
    const int S = p.S;
    UpSample g[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        g[k] = sample_upstream(f, u, [&](int c) { return l.at(rows.cs[c], k); }, [&](int c) { return l.at(rows.ct[c], k); },
                               [&] { return l.at(rows.b, k); }, l.at(rows.gw, k), r.zz[k]);
    }
    double Bc[4], B1[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) B1[k] = 0.0;
    l.rev_affine([&](int k, double& m, double& a) { scan_map(f, true, g[k], r.a_c[k], r.a_s[k], r.a_t[k], m, a); }, Bc);
    if (f.static_only) l.rev_affine([&](int k, double& m, double& a) { scan_map1(true, g[k], r.a_s[k], m, a); }, B1);
    if (!l.live) return;
    float g_ss[4], g_st[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const AlphaGrad d = alpha_grad(f, g[k], r, k, Bc[k], B1[k]);
        g_ss[k] = sigma_static_grad(f, d, r, k);
        g_st[k] = sigma_transient_grad(d, r, k);
    }
    g_raw_rows(f, p, l.ray, u, [&](int k) { return w.ws[k]; }, [&](int k) { return w.wt[k]; }, [&](int k) { return g_ss[k]; },
               [&](int k) { return g_st[k]; }, [&](int ch, auto&& val) {
                   const float v[4] = {val(0), val(1), val(2), val(3)};
                   l.store_row(graw, (size_t)ch * S, v);
               });
}

template <int RW>
__device__ __forceinline__ void ray_backward(const FourPerLane<RW>& l, const CompFlags& f, const CompArgs& p) {
    const int S = p.S, ray = l.ray;
    const float* raw = p.raw_t + (size_t)ray * p.R * S;
    float* graw = p.g_raw_t + (size_t)ray * p.R * S;
    const float* zr = p.z + (size_t)ray * S;
    UpRows<RW> rows;
    request_up_rows(l, f, p, raw, rows);
    Ray<4> r;
    ray_forward(l, f, p, raw, zr, r);
    Weights<4> w;
    ray_weights(l, f, r, w);
    const float acc = (float)l.sum(w.s_acc);
    const float depth = (float)l.sum(w.s_dep);
    const float sum_wo = f.static_only ? (float)l.sum(w.s_wo) : acc;
    UpScalars u;
    load_up_scalars(f, p, ray, depth, sum_wo, u);
    upstream_to_rows(l, f, p, rows, graw, r, w, u);
}

template <class L>
__global__ __launch_bounds__(256) void composite_bwd_kernel(CompArgs p) {
    const L l(p.N, p.S);
    if (l.idle()) return;
    ray_backward(l, CompFlags(p.flags), p);
}

#define NEFES_COMP_MAX_S 512           /* one sample per lane in up to eight passes; four per lane (S % 64 == 0) up to 256 */
static bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }
static int comp_args(CompArgs& a, int N, int S, int C, uint32_t flags) {
    if (N <= 0 || S <= 1 || C < 0) return NEFES_E_BADARG;
    if (S > NEFES_COMP_MAX_S) return NEFES_E_UNSUPPORTED;      // (the sampler's bound too: sample_pdf.hip SP_MAX_S)
    a.N = N; a.S = S; a.C = C; a.flags = flags;
    a.R = (flags & NEFES_COMP_SIGMA_ONLY) ? 1 : ((flags & NEFES_COMP_TRANSIENT) ? 3 + C + 6 : 3 + C + 1);
    return 0;
}
// a run-time count 1..MAX as a compile-time one: fn(std::integral_constant<int, n>); counts above MAX take MAX
template <int MAX, class F>
static void with_count(int n, F&& fn) {
    if constexpr (MAX > 1) {
        if (n < MAX) return with_count<MAX - 1>(n, fn);
    }
    fn(std::integral_constant<int, MAX>());
}

extern "C" int nefes_composite_fwd(int N, int S, int C, uint32_t flags, float beta_min, const float* raw_t,
                                   const float* z, float* rgb, float* feat, float* disp, float* acc, float* depth,
                                   float* weights, float* beta, void* stream) {
    CompArgs a = {};
    int rc = comp_args(a, N, S, C, flags);
    if (rc) return rc;
    if (!raw_t || !z) return NEFES_E_BADARG;
    a.beta_min = beta_min; a.raw_t = raw_t; a.z = z;
    a.rgb = rgb; a.feat = feat; a.disp = disp; a.acc = acc; a.depth = depth; a.weights = weights; a.beta = beta;
    // small frames with many feature channels: split the channels of a ray over up to four workgroups (composite_fwd_kernel)
    const int n_split = (feat && C >= 64 && N < 40000) ? ((C + 31) / 32 < 4 ? (C + 31) / 32 : 4) : 1;
    const dim3 grid((N + 3) / 4, n_split), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (S % 64 == 0 && S <= 256 && aligned16(raw_t) && aligned16(z) && aligned16(weights)) {   // four samples per lane
        const int rw = S / 64, rpw = 4 / rw;
        const dim3 grid4((N + 4 * rpw - 1) / (4 * rpw), n_split);
        with_count<4>(rw, [&](auto n) { hipLaunchKernelGGL(composite_fwd_kernel<FourPerLane<decltype(n)::value>>, grid4, block, 0, st, a); });
        return (int)hipGetLastError();
    }
    // (Q = 5: 64 + 256 samples, Q = 6: 128 + 256)
    with_count<8>((S + 63) / 64, [&](auto n) { hipLaunchKernelGGL(composite_fwd_kernel<OnePerLane<decltype(n)::value>>, grid, block, 0, st, a); });
    return (int)hipGetLastError();
}

extern "C" int nefes_composite_bwd(int N, int S, int C, uint32_t flags, const float* raw_t, const float* z,
                                   const float* g_rgb, const float* g_feat, const float* g_disp, const float* g_acc,
                                   const float* g_depth, const float* g_weights, const float* g_beta, float* g_raw_t,
                                   void* stream) {
    CompArgs a = {};
    int rc = comp_args(a, N, S, C, flags);
    if (rc) return rc;
    if (!raw_t || !z || !g_raw_t) return NEFES_E_BADARG;
    a.raw_t = raw_t; a.z = z; a.g_rgb = g_rgb; a.g_feat = g_feat; a.g_disp = g_disp; a.g_acc = g_acc;
    a.g_depth = g_depth; a.g_weights = g_weights; a.g_beta = g_beta; a.g_raw_t = g_raw_t;
    const dim3 grid((N + 3) / 4), block(256);
    hipStream_t st = (hipStream_t)stream;
    if (S % 64 == 0 && S <= 256 && aligned16(raw_t) && aligned16(z) && aligned16(g_raw_t) && aligned16(g_weights)) {
        const int rw = S / 64, rpw = 4 / rw;
        const dim3 grid4((N + 4 * rpw - 1) / (4 * rpw));
        with_count<4>(rw, [&](auto n) { hipLaunchKernelGGL(composite_bwd_kernel<FourPerLane<decltype(n)::value>>, grid4, block, 0, st, a); });
        return (int)hipGetLastError();
    }
    with_count<8>((S + 63) / 64, [&](auto n) { hipLaunchKernelGGL(composite_bwd_kernel<OnePerLane<decltype(n)::value>>, grid, block, 0, st, a); });
    return (int)hipGetLastError();
}

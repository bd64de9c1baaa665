// The body of the generic backward kernel; field_generic.hip includes it four times: GEN_KERNEL / GEN_ARGS = gen_bwd_kernel / GenArgs
// (the inference instance), gen_bwd_train_kernel / GenArgsTrain (TRAIN: the same code plus the copies to the train buffer),
// gen_bwd_ext_kernel / GenArgsExt (a supplied 32-feature encoding: gE has ER = 32 rows and is stored as it is, no chain rule) and
// gen_bwd_ext_train_kernel / GenArgsExtTrain (both).
template <int NCB>
__global__ __launch_bounds__(256, 1) void GEN_KERNEL(GEN_ARGS a) {
    constexpr int TS = 32 * NCB;
    constexpr bool TRAIN = GEN_ARGS::train;
    constexpr int ER = GEN_ARGS::ext ? GEN_X_ROWS : GEN_E_ROWS;      // rows of the E region
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
    if constexpr (GEN_ARGS::ext) {
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

// The body of the generic forward kernel; field_generic.hip includes it four times: GEN_KERNEL / GEN_ARGS = gen_fwd_kernel / GenArgs
// (the inference instance), gen_fwd_train_kernel / GenArgsTrain (TRAIN: the same code plus the copies to the train buffer),
// gen_fwd_ext_kernel / GenArgsExt (a supplied 32-feature encoding in the E region: ER = 32 rows, gen_embed's other overload) and
// gen_fwd_ext_train_kernel / GenArgsExtTrain (both: the E block of the train buffer is those 32 rows).
template <int NCB>
__global__ __launch_bounds__(256, 1) void GEN_KERNEL(GEN_ARGS a) {
    constexpr int TS = 32 * NCB;
    constexpr bool TRAIN = GEN_ARGS::train;
    constexpr int ER = GEN_ARGS::ext ? GEN_X_ROWS : GEN_E_ROWS;      // rows of the E region
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

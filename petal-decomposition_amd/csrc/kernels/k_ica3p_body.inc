// k_ica3p_body.inc -- the body of k_ica3p<NT> and k_ica3pg<NT, G> (see k_ica_mfma_body.inc).
    static_assert(NT == 2 || NT == 4, "whole 32-component chunks only");
    if (state && state[0]) return;
    constexpr int NCP = 16 * NT, KCH = NCP / 32, WITEMS = KCH * NT * 192;
    constexpr int ROWB = NCP * 2, PLANE = 32 * ROWB, IMG = 3 * PLANE, SLAB = 2 * (NCP * NCP + NCP);
    constexpr int SX = 4 * IMG > SLAB * 4 ? 4 * IMG : SLAB * 4;
    __shared__ bf16x8 sW[WITEMS];
    __shared__ __attribute__((aligned(16))) unsigned char sXb[SX];  // per wave [3 planes][32 samples][NCP bf16]; the slab at the end
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, q = lane >> 4;
    for (int e = threadIdx.x; e < WITEMS; e += 256) sW[e] = Wpk3[e];
    __syncthreads();
    const int64_t wid = (int64_t)blockIdx.x * 4 + wave;
    unsigned char* const img = sXb + wave * IMG;
    f32x4 dacc[NT][NT];  // [component tile][x tile]
    float gpa[NT];
#pragma unroll
    for (int a = 0; a < NT; ++a) {
        gpa[a] = 0.f;
#pragma unroll
        for (int b = 0; b < NT; ++b) dacc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const int64_t b0 = wid * blocks_per_wave, b1 = min((n + 31) / 32, b0 + blocks_per_wave);
    const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};
    bf16x8 xa[2][KCH][3];
    auto load_a = [&](int64_t blk) {
        const bf16x8* src = X1pl + (blk * 2 * KCH * 3) * 64 + lane;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int kc = 0; kc < KCH; ++kc)
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) xa[t][kc][pl] = src[((t * KCH + kc) * 3 + pl) * 64];
    };
    if (b0 < b1) load_a(b0);
    const int trq = (lane >> 2) & 3, trp = lane & 3;
    for (int64_t blk = b0; blk < b1; ++blk) {
        const int64_t r0 = blk * 32;
        // the planes go to the wave's image (row 16 t + i, chunk 4 kc + q), from which the second product reads them transposed
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int kc = 0; kc < KCH; ++kc) {
                unsigned char* a = img + ica_xoff<NT>(16 * t + i, 4 * kc + q);
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) *reinterpret_cast<bf16x8*>(a + pl * PLANE) = xa[t][kc][pl];
            }
        bf16x8 nwh = sW[lane], nwm = sW[64 + lane], nwl = sW[128 + lane];
        f32x4 sacc[2][NT];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int u = 0; u < NT; ++u) sacc[t][u] = z4;
#pragma unroll
        for (int kc = 0; kc < KCH; ++kc) {
#pragma unroll
            for (int u = 0; u < NT; ++u) {
                const bf16x8 wh = nwh, wm = nwm, wl = nwl;
                if (kc * NT + u + 1 < KCH * NT) {  // W's pieces are read one tile ahead (LDS latency off the MFMA path)
                    const bf16x8* sw = sW + (kc * NT + u + 1) * 192 + lane;
                    nwh = sw[0], nwm = sw[64], nwl = sw[128];
                }
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    f32x4 c4 = sacc[t][u];
                    c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[t][kc][2], wh, c4, 0, 0, 0);  // smallest terms first
                    c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[t][kc][1], wm, c4, 0, 0, 0);
                    c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[t][kc][0], wl, c4, 0, 0, 0);
                    c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[t][kc][1], wh, c4, 0, 0, 0);
                    c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[t][kc][0], wm, c4, 0, 0, 0);
                    c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xa[t][kc][0], wh, c4, 0, 0, 0);
                    sacc[t][u] = c4;
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (blk + 1 < b1) load_a(blk + 1);  // next pass's planes land behind tanh and the second product
        // B operand of the second product: lane (j = i, q), slot e <- X1[r0 + (e < 4 ? 4 q + e : 16 + 4 q + e - 4)][16 b + j], transposed
        // reads of the image (T10: lane 16 g + 4 q' + p supplies block row q', columns 4 p .. 4 p + 3)
        // (exp at 32 components keeps u, e and g of eight samples alive beside everything else: there each B tile is read right in front
        // of its MFMAs, once per component tile, instead of all of them ahead of make_g -- 122 registers, four waves per SIMD, no scratch)
        constexpr bool LATE_B = G == ICA_G_EXP && NT == 2;
        bf16x8 bh[NT], bm[NT], bl[NT];
        auto load_b = [&](int b) {
            const unsigned char* a0 = img + ica_xoff<NT>(4 * q + trq, 2 * b + (trp >> 1)) + 8 * (trp & 1);   // (row + 16: + 16 rows, same swizzle)
            bh[b] = lds_tr2(a0, a0 + 16 * ROWB);
            bm[b] = lds_tr2(a0 + PLANE, a0 + PLANE + 16 * ROWB);
            bl[b] = lds_tr2(a0 + 2 * PLANE, a0 + 2 * PLANE + 16 * ROWB);
        };
        if constexpr (!LATE_B) {
#pragma unroll
            for (int b = 0; b < NT; ++b) load_b(b);
        }
        // sacc[t][u][r] = S[sample r0 + 16 t + 4 q + r][component 16 u + i].  Rows past n were stored as zero planes: S = 0
        // and tanh(0) = 0 exactly, so only the g' sum needs masking (last pass).
        const bool tail = r0 + 32 > n;
        const float nvalid = tail ? (float)((n > r0 + 4 * q ? (int)min((int64_t)4, n - r0 - 4 * q) : 0) +
                                            (n > r0 + 16 + 4 * q ? (int)min((int64_t)4, n - r0 - 16 - 4 * q) : 0))
                                  : 8.0f;
        bf16x8 gh, gm, gl;
        auto make_g = [&](int u) {
            f32x8 g8;
            float gs = 0.f;
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if constexpr (G == ICA_G_LOGCOSH) {
                        const float g = tanh_fast(sacc[t][u][r]);
                        g8[4 * t + r] = g;
                        gs = fmaf(-g, g, gs);
                    } else {
                        float g, gp;
                        ica_contrast<G>(sacc[t][u][r], g, gp);
                        g8[4 * t + r] = g;
                        gs += gp;
                    }
                }
            // logcosh: gs = -sum g^2 over the 8 rows (0 for the zero rows), so the valid rows' sum of 1 - g^2 is gs + nvalid;
            // the others sum g' over all 8 rows and take the zero rows' g'(0) back out
            gpa[u] += G == ICA_G_LOGCOSH ? gs + nvalid : gs - ica_gp_pad<G>(8.0f - nvalid);
            split3(g8, gh, gm, gl);
        };
        make_g(0);
        // D[component][x] += sum_samples G[sample][component] X1[sample][x]
#pragma unroll
        for (int a = 0; a < NT; ++a) {
            __builtin_amdgcn_sched_barrier(0);
            const bf16x8 fh = gh, fm = gm, fl = gl;
            if (a + 1 < NT) make_g(a + 1);
#pragma unroll
            for (int b = 0; b < NT; ++b) {
                if constexpr (LATE_B) load_b(b);
                f32x4 c4 = dacc[a][b];
                c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fl, bh[b], c4, 0, 0, 0);
                c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fm, bm[b], c4, 0, 0, 0);
                c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fh, bl[b], c4, 0, 0, 0);
                c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fm, bh[b], c4, 0, 0, 0);
                c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fh, bm[b], c4, 0, 0, 0);
                c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fh, bh[b], c4, 0, 0, 0);
                dacc[a][b] = c4;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();  // the slab aliases the images
    ica_write_slab<NT>(dacc, gpa, reinterpret_cast<float*>(sXb), part);

// k_ica3_body.inc -- the body of k_ica3<NT> and k_ica3g<NT, G> (see k_ica_mfma_body.inc).
    if (state && state[0]) return;
    constexpr int NCP = 16 * NT, KCH = (NCP + 31) / 32, WITEMS = KCH * NT * 192;
    constexpr int XP = NCP + 4;  // row pitch of the transposition buffer: 4 XP = 16 (mod 32) banks
    constexpr int XT_FLOATS = 4 * 32 * XP, SLAB = 2 * (NCP * NCP + NCP);
    __shared__ bf16x8 sW[WITEMS];
    __shared__ __attribute__((aligned(16))) float sX[XT_FLOATS > SLAB ? XT_FLOATS : SLAB];  // per wave [32 samples][XP]; the slab at the end
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, q = lane >> 4;
    for (int e = threadIdx.x; e < WITEMS; e += 256) sW[e] = Wpk3[e];
    __syncthreads();
    const int64_t wid = (int64_t)blockIdx.x * 4 + wave;
    float* xt = sX + wave * 32 * XP;
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
    // A operand of the first product: lane (i, q) <- X1[r0 + 16 t + i][32 kc + 8 q .. + 7]
    f32x4 xa[2][KCH][2];
    auto load_a = [&](int64_t blk) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int64_t ra = blk * 32 + 16 * t + i;
#pragma unroll
            for (int kc = 0; kc < KCH; ++kc) {
                const bool v = ra < n && (32 * kc + 8 * q) < NCP;
                const float* src = X1T + ra * ld + 32 * kc + 8 * q;
                xa[t][kc][0] = v ? *reinterpret_cast<const f32x4*>(src) : z4;
                xa[t][kc][1] = v ? *reinterpret_cast<const f32x4*>(src + 4) : z4;
            }
        }
    };
    if (b0 < b1) load_a(b0);
    // Each group of MFMAs is written next to independent VALU work (chunk kc's MFMAs beside the split of chunk kc + 1 or
    // of the transposed rows; component tile a's MFMAs beside tanh + split of tile a + 1).  Measured (dev/micro_coissue.hip):
    // on a SIMD holding two such waves MFMA time and VALU time ADD rather than overlap, so the pass costs
    // ~3070 (192 MFMAs) + ~3600 (730 VALU, 64 of them quarter-rate transcendentals) cycles; the kernel runs within 25 % of that.
    for (int64_t blk = b0; blk < b1; ++blk) {
        const int64_t r0 = blk * 32;
        bf16x8 ah[2], am[2], al[2];
        auto split_a = [&](int kc) {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const f32x8 x = {xa[t][kc][0][0], xa[t][kc][0][1], xa[t][kc][0][2], xa[t][kc][0][3],
                                 xa[t][kc][1][0], xa[t][kc][1][1], xa[t][kc][1][2], xa[t][kc][1][3]};
                split3(x, ah[t], am[t], al[t]);
            }
        };
        // the raw rows also go to the wave's LDS buffer, from which the second product reads them transposed
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int kc = 0; kc < KCH; ++kc)
                if ((32 * kc + 8 * q) < NCP) {
                    float* dst = xt + (16 * t + i) * XP + 32 * kc + 8 * q;
                    *reinterpret_cast<f32x4*>(dst) = xa[t][kc][0];
                    *reinterpret_cast<f32x4*>(dst + 4) = xa[t][kc][1];
                }
        bf16x8 nwh = sW[lane], nwm = sW[64 + lane], nwl = sW[128 + lane];
        split_a(0);
        __builtin_amdgcn_wave_barrier();
        f32x4 sacc[2][NT];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int u = 0; u < NT; ++u) sacc[t][u] = z4;
        bf16x8 bh[NT], bm[NT], bl[NT];
#pragma unroll
        for (int kc = 0; kc < KCH; ++kc) {
            __builtin_amdgcn_sched_barrier(0);
            bf16x8 ch[2], cm[2], cl[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) { ch[t] = ah[t]; cm[t] = am[t]; cl[t] = al[t]; }
            if (kc + 1 < KCH) {
                split_a(kc + 1);
            } else {
                // B operand: lane (j = i, q), slot e <- X1[r0 + (e < 4 ? 4 q + e : 16 + 4 q + e - 4)][16 b + j]
#pragma unroll
                for (int b = 0; b < NT; ++b) {
                    f32x8 xb;
#pragma unroll
                    for (int e = 0; e < 8; ++e) xb[e] = xt[((e < 4 ? 4 * q + e : 12 + 4 * q + e)) * XP + 16 * b + i];
                    split3(xb, bh[b], bm[b], bl[b]);
                }
            }
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
                    c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cl[t], wh, c4, 0, 0, 0);  // smallest terms first
                    c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cm[t], wm, c4, 0, 0, 0);
                    c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ch[t], wl, c4, 0, 0, 0);
                    c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(cm[t], wh, c4, 0, 0, 0);
                    c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ch[t], wm, c4, 0, 0, 0);
                    c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ch[t], wh, c4, 0, 0, 0);
                    sacc[t][u] = c4;
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // (exp at 32 components keeps u, e and g of eight samples alive beside everything else: there the next pass's rows are asked
        // for at the end of the pass instead, which keeps the kernel at four waves per SIMD -- they cover the exposed latency)
        constexpr bool LATE_A = G == ICA_G_EXP && NT == 2;
        if (!LATE_A && blk + 1 < b1) load_a(blk + 1);  // next pass's rows land behind tanh and the second product
        // sacc[t][u][r] = S[sample r0 + 16 t + 4 q + r][component 16 u + i].  Rows past n were loaded as zeros: S = 0
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
        if (LATE_A && blk + 1 < b1) load_a(blk + 1);
    }
    __syncthreads();  // the slab aliases the transposition buffers
    ica_write_slab<NT>(dacc, gpa, sX, part);

// k_gemm_scores.inc -- part of the ONE translation unit hip_ops.hip (textually included there, inside namespace petal): K1 with the row-score epilogue (k_xp3s, k_xp_mfma_s, k_xp_f64s, k_xp_simple_s).
// ================================================================================================
// Row scores of a fitted projection, from the accumulators of the product kernel at the end of its single pass over X:
//   q_i = |xc_i|^2,  residual_i = max(q_i - sum_j y_ij^2, 0),  weighted_i = sum_j w_j y_ij^2     (xc = x - mu, y = xc P)
// Every kernel here is its K1 counterpart (same operand layout, same MFMA order: the product is bit for bit the one that kernel
// stores) with (a) sum xc^2 accumulated from the centred fragments it already holds and (b) an epilogue that squares the accumulator
// tiles instead of -- or, with Z given, besides -- storing them.  The per-row state st (n x 2, ldst) is [q - sum y^2 | sum w y^2] over
// the column panels launched so far: the first panel (nt0 == 0) initialises it, later panels update it in launch order (one stream),
// the last one clamps the residual at zero.  No atomics: one lane owns a row.
// Cross-lane sums without LDS memory: ds_swizzle in bit mode inside a half wave, v_permlane32_swap between the halves.
template <int XOR>
__device__ __forceinline__ float lane_xor(float v) {   // the value of lane ^ XOR, XOR < 32
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x1f | (XOR << 10)));
}
template <int XOR>
__device__ __forceinline__ double lane_xor(double v) {
    typedef int i32x2 __attribute__((ext_vector_type(2)));
    i32x2 b = __builtin_bit_cast(i32x2, v);
    b[0] = __builtin_amdgcn_ds_swizzle(b[0], 0x1f | (XOR << 10));
    b[1] = __builtin_amdgcn_ds_swizzle(b[1], 0x1f | (XOR << 10));
    return __builtin_bit_cast(double, b);
}
// lower half + upper half, the same sum in the same order on every lane (v_permlane32_swap with both operands v leaves
// [lower | lower] and [upper | upper])
__device__ __forceinline__ float sum_halves(float v) {
    const unsigned u = __builtin_bit_cast(unsigned, v);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
    return __builtin_bit_cast(float, (unsigned)r[0]) + __builtin_bit_cast(float, (unsigned)r[1]);
}
__device__ __forceinline__ double sum_halves(double v) {
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    const u32x2 b = __builtin_bit_cast(u32x2, v);
    const auto r0 = __builtin_amdgcn_permlane32_swap(b[0], b[0], false, false);
    const auto r1 = __builtin_amdgcn_permlane32_swap(b[1], b[1], false, false);
    return __builtin_bit_cast(double, u32x2{(unsigned)r0[0], (unsigned)r1[0]}) + __builtin_bit_cast(double, u32x2{(unsigned)r0[1], (unsigned)r1[1]});
}
// sum over the four 16-lane groups of a wave (lanes i, i + 16, i + 32, i + 48)
template <class T>
__device__ __forceinline__ T sum_groups4(T v) {
    v += lane_xor<16>(v);
    return sum_halves(v);
}
// one row's share of a column panel into the state
template <class T>
__device__ __forceinline__ void score_row_update(T* __restrict__ st, int64_t ldst, int64_t row, bool first, bool last, T q, T s, T w) {
    T* p = st + row * ldst;
    T r = (first ? q : p[0]) - s;
    const T wt = first ? w : p[1] + w;
    if (last && r < T(0)) r = T(0);   // (a NaN stays a NaN)
    p[0] = r;
    p[1] = wt;
}
// epilogue of the fp32 kernels: reg e of lane (i, q), tile (t, u) is Y[row0 + 16 t + i][16 (nt0 + u) + 4 q + e] (the Z^T tile of k_xp_mfma /
// k_xp3); wts (nullable = all ones) is padded with zeros to 16 NTtot columns, like P
template <int RT, int NT>
__device__ __forceinline__ void score_rows_f32(const f32x4 (&acc)[RT][NT], const float (&qs)[RT], int NTtot, int nt0, const float* __restrict__ wts,
                                               float* __restrict__ st, int64_t ldst, int64_t row0, int64_t n, int i, int q) {
    const bool first = nt0 == 0, last = nt0 + NT >= NTtot;
#pragma unroll
    for (int t = 0; t < RT; ++t) {   // row tile by row tile: its accumulators are dead afterwards
        float s = 0.f, w = 0.f;
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            f32x4 wv = f32x4{1.f, 1.f, 1.f, 1.f};
            if (wts) wv = *reinterpret_cast<const f32x4*>(wts + 16 * (nt0 + u) + 4 * q);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float y = acc[t][u][e], y2 = y * y;
                s += y2;
                w = __builtin_fmaf(wv[e], y2, w);
            }
        }
        s = sum_groups4(s);
        w = wts ? sum_groups4(w) : s;   // (no weights: residual + weighted == q up to one rounding)
        const float qv = sum_groups4(qs[t]);
        const int64_t row = row0 + 16 * t + i;
        if (q == 0 && row < n) score_row_update(st, ldst, row, first, last, qv, s, w);
    }
}
// hi + lo += d without losing what the addition rounds off (two-sum): the ONE-tile kernels keep their product this way for the scores.
// With a single tile (k <= 16) the error of a column's fp32 accumulation chain does not average out over columns: measured on one
// component over 256 features, the chain the kernel stores is off by 3.5 (split-product) / 5.1 (fp32 MFMA) eps |x|.
__device__ __forceinline__ void two_sum_acc(f32x4& hi, f32x4& lo, const f32x4 d) {
    const f32x4 s = hi + d, bb = s - hi;
    lo += (hi - (s - bb)) + (d - bb);
    hi = s;
}
__device__ __forceinline__ float sumsq8(const f32x8 a) {
    float s = a[0] * a[0];
#pragma unroll
    for (int e = 1; e < 8; ++e) s = __builtin_fmaf(a[e], a[e], s);
    return s;
}

// ------------------------------------------------------------------------------------------------
// split-product form: k_xp3<4, NT, 1, CENTER, 4, OCC, 3> (64-row wave tiles, three-plane operands, panels of <= 5 tiles) with the
// score epilogue.  Z nullable.
template <int NT, bool CENTER>
__global__ __launch_bounds__(256, PETAL_XP3_OCC) void k_xp3s(const float* __restrict__ X, int64_t n, int K, int64_t ldx, const float* __restrict__ mu,
                                                             const bf16x8* __restrict__ Ppk3, int NTtot, int nt0, int N, float* __restrict__ Z,
                                                             int64_t ldz, const float* __restrict__ wts, float* __restrict__ st, int64_t ldst) {
    constexpr int RT = 4, WVK = 4, NPL = 3;
    constexpr int PITEMS = NT * 64 * NPL;
    constexpr int NTHR = 64 * WVK;
    constexpr int PI = (PITEMS + NTHR - 1) / NTHR;
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_xp3s[];
    bf16x8* sP = reinterpret_cast<bf16x8*>(sm_xp3s);                                // [2][PITEMS]
    float* sMu = reinterpret_cast<float*>(sm_xp3s + sizeof(bf16x8) * 2 * PITEMS);   // [32 nchunk] (zero padded)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int64_t row0 = ((int64_t)blockIdx.x * WVK + wave) * (16 * RT);
    const int nchunk = (K + 31) >> 5;
    if (CENTER)
        for (int k = tid; k < 32 * nchunk; k += NTHR) sMu[k] = k < K ? mu[k] : 0.f;
    // One tile: beside the chain that is stored (acc: k_xp3's, bit for bit) every chunk's product is formed from zero -- the leading
    // piece product on its own (one rounding, at the size of the chunk's share), the five small ones as a chain -- and added to a
    // compensated sum, from which the scores are taken (see two_sum_acc).  Twelve MFMAs per chunk and row tile instead of six: at one
    // tile the kernel waits for HBM either way.
    constexpr bool COMP = NT == 1;
    f32x4 acc[RT][NT];
    f32x4 chi[COMP ? RT : 1], clo[COMP ? RT : 1];   // (the compensated sum: leading part, what the additions rounded off)
    float qs[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        qs[t] = 0.f;
        if (COMP) { chi[t] = f32x4{0.f, 0.f, 0.f, 0.f}; clo[t] = chi[t]; }
#pragma unroll
        for (int u = 0; u < NT; ++u) acc[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const float* xrow[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        const int64_t r = row0 + 16 * t + i;
        xrow[t] = X + (r < n ? r : (n - 1)) * ldx + 8 * q;
    }
    const bf16x8* psrc = Ppk3 + (int64_t)nt0 * 192;
    auto load_a = [&](int c, f32x8(&a)[RT]) {
        const bool in = 32 * c + 8 * q < K;  // K % 32 == 16: the upper half of the last chunk does not exist
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            f32x4 lo = f32x4{0.f, 0.f, 0.f, 0.f}, hi = lo;
            if (in) { lo = ld_stream(xrow[t] + 32 * c); hi = ld_stream(xrow[t] + 32 * c + 4); }
            a[t] = f32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        }
    };
    auto load_p = [&](int c, bf16x8(&pn)[PI]) {
#pragma unroll
        for (int it = 0; it < PI; ++it)
            if (tid + NTHR * it < PITEMS) pn[it] = psrc[(int64_t)c * NTtot * 192 + tid + NTHR * it];
    };
    auto store_p = [&](int buf, const bf16x8(&pn)[PI]) {
#pragma unroll
        for (int it = 0; it < PI; ++it)
            if (tid + NTHR * it < PITEMS) sP[buf * PITEMS + tid + NTHR * it] = pn[it];
    };
    f32x8 a[RT];
    bf16x8 pn[PI];
    load_p(0, pn);
    load_a(0, a);
    store_p(0, pn);
    for (int c = 0; c < nchunk; ++c) {
        const int buf = c & 1;
        __syncthreads();  // chunk c is in sP[buf]; nobody still reads sP[buf ^ 1]
        bf16x8 ah[RT], am[RT], al[RT];
        {
            f32x8 m = f32x8{0, 0, 0, 0, 0, 0, 0, 0};
            if (CENTER) {
                const f32x4 lo = *reinterpret_cast<const f32x4*>(sMu + 32 * c + 8 * q), hi = *reinterpret_cast<const f32x4*>(sMu + 32 * c + 8 * q + 4);
                m = f32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            }
#pragma unroll
            for (int t = 0; t < RT; ++t) {
                if (CENTER) a[t] -= m;
                if (nt0 == 0) qs[t] += sumsq8(a[t]);   // (the centred fragment, before it is split)
                split3(a[t], ah[t], am[t], al[t]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // P first, then X: see k_xp3
        if (c + 1 < nchunk) load_p(c + 1, pn);
        if (c + 1 < nchunk) load_a(c + 1, a);
        __builtin_amdgcn_sched_barrier(0);
        const bf16x8* sPb = sP + buf * PITEMS + lane;
        bf16x8 bh = sPb[0], bm = sPb[64], bl = sPb[128];
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            bf16x8 nh = bh, nm = bm, nl = bl;
            if (u + 1 < NT) { nh = sPb[((u + 1) * NPL) * 64]; nm = sPb[((u + 1) * NPL + 1) * 64]; nl = sPb[((u + 1) * NPL + 2) * 64]; }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < RT; ++t) {  // the six piece products in k_xp3's order: the same bits
                f32x4 c4 = acc[t][u];
                c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bl, ah[t], c4, 0, 0, 0);
                c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bm, am[t], c4, 0, 0, 0);
                c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh, al[t], c4, 0, 0, 0);
                c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bm, ah[t], c4, 0, 0, 0);
                c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh, am[t], c4, 0, 0, 0);
                c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh, ah[t], c4, 0, 0, 0);
                acc[t][u] = c4;
            }
            if constexpr (COMP) {
#pragma unroll
                for (int t = 0; t < RT; ++t) {
                    const f32x4 z4 = f32x4{0.f, 0.f, 0.f, 0.f};
                    f32x4 dm = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bl, ah[t], z4, 0, 0, 0);
                    dm = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bm, am[t], dm, 0, 0, 0);
                    dm = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh, al[t], dm, 0, 0, 0);
                    dm = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bm, ah[t], dm, 0, 0, 0);
                    dm = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh, am[t], dm, 0, 0, 0);
                    const f32x4 dh = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bh, ah[t], z4, 0, 0, 0);
                    two_sum_acc(chi[t], clo[t], dh);
                    clo[t] += dm;   // (2^-8 of the chunk's product: its roundings do not count)
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            bh = nh; bm = nm; bl = nl;
        }
        __builtin_amdgcn_sched_barrier(0);
        if (c + 1 < nchunk) store_p(buf ^ 1, pn);
    }
    if (Z) {
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            const int col = 16 * (nt0 + u) + 4 * q;
            if (col >= N) continue;
#pragma unroll
            for (int t = 0; t < RT; ++t) {
                const int64_t row = row0 + 16 * t + i;
                if (row < n) *reinterpret_cast<f32x4*>(Z + row * ldz + col) = acc[t][u];
            }
        }
    }
    if constexpr (COMP) {
        f32x4 ys[RT][1];
#pragma unroll
        for (int t = 0; t < RT; ++t) ys[t][0] = chi[t] + clo[t];
        score_rows_f32<RT, 1>(ys, qs, NTtot, nt0, wts, st, ldst, row0, n, i, q);
    } else {
        score_rows_f32<RT, NT>(acc, qs, NTtot, nt0, wts, st, ldst, row0, n, i, q);
    }
}

// ------------------------------------------------------------------------------------------------
// fp32-MFMA form: k_xp_mfma<4, NT, CENTER, false> with the score epilogue (every n: the persistent form has no score twin; NT <= 4: at five
// tiles the epilogue's registers do not fit beside 80 accumulators and three register stages without spilling)
// One tile (NT == 1; launched with RT = 2, 32-row wave tiles, which is what keeps the four waves per SIMD of k_xp_mfma<4, 1>): as in k_xp3s
// the scores come from a compensated sum of the chunks' products, each formed from zero, beside the chain that is stored.
template <int NT, bool CENTER, int RT = 4>
__global__ __launch_bounds__(256, 2) void k_xp_mfma_s(const float* __restrict__ X, int64_t n, int K, int64_t ldx, const float* __restrict__ mu,
                                                      const float* __restrict__ Ppk, int NTtot, int nt0, int N, float* __restrict__ Z, int64_t ldz,
                                                      const float* __restrict__ wts, float* __restrict__ st, int64_t ldst) {
    constexpr bool COMP = NT == 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * (16 * RT);
    if (row0 >= n) return;
    f32x4 acc[RT][NT];
    f32x4 chi[COMP ? RT : 1], clo[COMP ? RT : 1];   // (the compensated sum: leading part, what the additions rounded off)
    float qs[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        qs[t] = 0.f;
        if (COMP) { chi[t] = f32x4{0.f, 0.f, 0.f, 0.f}; clo[t] = chi[t]; }
#pragma unroll
        for (int u = 0; u < NT; ++u) acc[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const float* xrow[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        const int64_t r = row0 + 16 * t + i;
        xrow[t] = X + (r < n ? r : (n - 1)) * ldx + 4 * q;
    }
    const f32x4* pb = reinterpret_cast<const f32x4*>(Ppk) + (int64_t)nt0 * 64 + lane;
    const float* mup = mu + 4 * q;
    const int nchunk = K >> 4;
    auto load_chunk = [&](int c, f32x4(&a)[RT], f32x4(&b)[NT], f32x4& m) {
#pragma unroll
        for (int t = 0; t < RT; ++t) a[t] = ld_stream(xrow[t] + 16 * c);
#pragma unroll
        for (int u = 0; u < NT; ++u) b[u] = pb[((int64_t)c * NTtot + u) * 64];
        if (CENTER) m = *reinterpret_cast<const f32x4*>(mup + 16 * c);
    };
    auto compute = [&](f32x4(&a)[RT], f32x4(&b)[NT], const f32x4& m) {
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            if (CENTER) a[t] -= m;
            if (nt0 == 0) qs[t] += __builtin_fmaf(a[t][3], a[t][3], __builtin_fmaf(a[t][2], a[t][2], __builtin_fmaf(a[t][1], a[t][1], a[t][0] * a[t][0])));   // (the uniform branch is the cheaper form here: 122 against 160 registers at one tile)
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int t = 0; t < RT; ++t)
#pragma unroll
                for (int u = 0; u < NT; ++u)
                    acc[t][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[u][s], a[t][s], acc[t][u], 0, 0, 0);  // Z^T tile
        if constexpr (COMP) {
#pragma unroll
            for (int t = 0; t < RT; ++t) {
                f32x4 d4 = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < 4; ++s) d4 = __builtin_amdgcn_mfma_f32_16x16x4f32(b[0][s], a[t][s], d4, 0, 0, 0);
                two_sum_acc(chi[t], clo[t], d4);
            }
        }
    };
    // three register stages, as k_xp_mfma
    f32x4 a0[RT], b0[NT], a1[RT], b1[NT], a2[RT], b2[NT];
    f32x4 m0 = f32x4{0.f, 0.f, 0.f, 0.f}, m1 = m0, m2 = m0;
    const int last = nchunk - 1;
    load_chunk(0, a0, b0, m0);
    load_chunk(last < 1 ? last : 1, a1, b1, m1);
    int c = 0;
    for (; c + 3 <= nchunk; c += 3) {
        load_chunk(c + 2 < last ? c + 2 : last, a2, b2, m2);
        __builtin_amdgcn_sched_barrier(0);
        compute(a0, b0, m0);
        __builtin_amdgcn_sched_barrier(0);
        load_chunk(c + 3 < last ? c + 3 : last, a0, b0, m0);
        __builtin_amdgcn_sched_barrier(0);
        compute(a1, b1, m1);
        __builtin_amdgcn_sched_barrier(0);
        load_chunk(c + 4 < last ? c + 4 : last, a1, b1, m1);
        __builtin_amdgcn_sched_barrier(0);
        compute(a2, b2, m2);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (c < nchunk) compute(a0, b0, m0);
    if (c + 1 < nchunk) compute(a1, b1, m1);
    if (Z) {
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            const int col = 16 * (nt0 + u) + 4 * q;
            if (col >= N) continue;
#pragma unroll
            for (int t = 0; t < RT; ++t) {
                const int64_t row = row0 + 16 * t + i;
                if (row < n) *reinterpret_cast<f32x4*>(Z + row * ldz + col) = acc[t][u];
            }
        }
    }
    if constexpr (COMP) {
        f32x4 ys[RT][1];
#pragma unroll
        for (int t = 0; t < RT; ++t) ys[t][0] = chi[t] + clo[t];
        score_rows_f32<RT, 1>(ys, qs, NTtot, nt0, wts, st, ldst, row0, n, i, q);
    } else {
        score_rows_f32<RT, NT>(acc, qs, NTtot, nt0, wts, st, ldst, row0, n, i, q);
    }
}

// ------------------------------------------------------------------------------------------------
// fp64 form: k_xp_f64<NT, CENTER, false> with the score epilogue.  The X fragment of lane (i, q) belongs to row 16 t + i, register r of
// its accumulator tiles to row 16 t + q + 4 r, column i: sum y^2 is reduced over the 16 column lanes, sum xc^2 over the four groups, and
// the lanes with (i & 3) == q hold both for row 16 t + i.
template <int NT, bool CENTER>
__global__ __launch_bounds__(256) void k_xp_f64s(const double* __restrict__ X, int64_t n, int K, int64_t ldx, const double* __restrict__ mu,
                                                 const f64x2* __restrict__ Ppk, int NTtot, int nt0, int N, double* __restrict__ Z, int64_t ldz,
                                                 const double* __restrict__ wts, double* __restrict__ st, int64_t ldst) {
    constexpr int RT = 2;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int64_t row0 = ((int64_t)blockIdx.x * 4 + wave) * (16 * RT);
    if (row0 >= n) return;
    f64x4 acc[RT][NT];
    double qs[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        qs[t] = 0.0;
#pragma unroll
        for (int u = 0; u < NT; ++u) acc[t][u] = f64x4{0.0, 0.0, 0.0, 0.0};
    }
    const double* xrow[RT];
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        const int64_t r = row0 + 16 * t + i;
        xrow[t] = X + (r < n ? r : (n - 1)) * ldx + 2 * q;
    }
    const f64x2* pb = Ppk + (int64_t)nt0 * 64 + lane;
    const double* mup = mu + 2 * q;
    const int nchunk = K >> 3;
    auto load_chunk = [&](int c, f64x2(&a)[RT], f64x2(&b)[NT], f64x2& m) {
#pragma unroll
        for (int t = 0; t < RT; ++t) a[t] = *reinterpret_cast<const f64x2*>(xrow[t] + 8 * c);
#pragma unroll
        for (int u = 0; u < NT; ++u) b[u] = pb[((int64_t)c * NTtot + u) * 64];
        if (CENTER) m = *reinterpret_cast<const f64x2*>(mup + 8 * c);
    };
    auto compute = [&](f64x2(&a)[RT], f64x2(&b)[NT], const f64x2& m) {
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            if (CENTER) a[t] -= m;
            qs[t] += __builtin_fma(a[t][1], a[t][1], a[t][0] * a[t][0]);   // (every panel: a branch in the pipelined loop costs registers)
        }
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
            for (int t = 0; t < RT; ++t)
#pragma unroll
                for (int u = 0; u < NT; ++u) acc[t][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t][s2], b[u][s2], acc[t][u], 0, 0, 0);
    };
    f64x2 a0[RT], b0[NT], a1[RT], b1[NT], m0 = f64x2{0.0, 0.0}, m1 = m0;
    const int last = nchunk - 1;
    load_chunk(0, a0, b0, m0);
    int c = 0;
    for (; c + 2 <= nchunk; c += 2) {
        load_chunk(c + 1, a1, b1, m1);
        __builtin_amdgcn_sched_barrier(0);
        compute(a0, b0, m0);
        __builtin_amdgcn_sched_barrier(0);
        load_chunk(c + 2 < last ? c + 2 : last, a0, b0, m0);
        __builtin_amdgcn_sched_barrier(0);
        compute(a1, b1, m1);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (c < nchunk) compute(a0, b0, m0);
    const bool first = nt0 == 0, lastp = nt0 + NT >= NTtot;
    if (Z) {
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            const int col = 16 * (nt0 + u) + i;
            if (col >= N) continue;
#pragma unroll
            for (int t = 0; t < RT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t row = row0 + 16 * t + q + 4 * r;
                    if (row < n) Z[row * ldz + col] = acc[t][u][r];
                }
        }
    }
#pragma unroll
    for (int t = 0; t < RT; ++t) {
        f64x4 s = f64x4{0.0, 0.0, 0.0, 0.0}, w = s;
#pragma unroll
        for (int u = 0; u < NT; ++u) {
            const double wv = wts ? wts[16 * (nt0 + u) + i] : 1.0;   // (padded with zeros to 16 NTtot columns)
            const f64x4 y2 = acc[t][u] * acc[t][u];
            s += y2;
            w += wv * y2;
        }
        double sr = 0.0, wr = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double a = s[r], b = w[r];
            a += lane_xor<1>(a); a += lane_xor<2>(a); a += lane_xor<4>(a); a += lane_xor<8>(a);
            if (wts) { b += lane_xor<1>(b); b += lane_xor<2>(b); b += lane_xor<4>(b); b += lane_xor<8>(b); } else b = a;
            if ((i >> 2) == r) { sr = a; wr = b; }
        }
        const double qv = sum_groups4(qs[t]);
        const int64_t row = row0 + 16 * t + i;
        if ((i & 3) == q && row < n) score_row_update(st, ldst, row, first, lastp, qv, sr, wr);
    }
}

// ------------------------------------------------------------------------------------------------
// every other shape (n < 64, odd or unaligned operands): k_xp_simple's product (fp64 accumulation, the same Z), one wave per row,
// all N columns in one launch
template <class T>
__global__ __launch_bounds__(64) void k_xp_simple_s(const T* __restrict__ X, int64_t n, int64_t K, int64_t ldx, const T* __restrict__ mu,
                                                    const double* __restrict__ P, int64_t N, int64_t ldp, T* __restrict__ Z, int64_t ldz,
                                                    const T* __restrict__ wts, T* __restrict__ st, int64_t ldst) {
    const int64_t i = blockIdx.x;
    const int lane = threadIdx.x;
    double qv = 0, s = 0, w = 0;
    for (int64_t k = lane; k < K; k += 64) {
        T xv = X[i * ldx + k];
        if (mu) xv = xv - mu[k];
        qv += (double)xv * (double)xv;
    }
    for (int64_t j = lane; j < N; j += 64) {
        double acc = 0;
        for (int64_t k = 0; k < K; ++k) {
            T xv = X[i * ldx + k];
            if (mu) xv = xv - mu[k];
            acc += (double)xv * (sizeof(T) == 4 ? (double)(float)P[k * ldp + j] : P[k * ldp + j]);
        }
        if (Z) Z[i * ldz + j] = (T)acc;
        s += acc * acc;
        w += (wts ? (double)wts[j] : 1.0) * (acc * acc);
    }
    qv += lane_xor<1>(qv); qv += lane_xor<2>(qv); qv += lane_xor<4>(qv); qv += lane_xor<8>(qv); qv = sum_groups4(qv);
    s += lane_xor<1>(s); s += lane_xor<2>(s); s += lane_xor<4>(s); s += lane_xor<8>(s); s = sum_groups4(s);
    w += lane_xor<1>(w); w += lane_xor<2>(w); w += lane_xor<4>(w); w += lane_xor<8>(w); w = sum_groups4(w);
    if (lane == 0) {
        double r = qv - s;
        if (r < 0) r = 0;
        st[i * ldst] = (T)r;
        st[i * ldst + 1] = (T)w;
    }
}

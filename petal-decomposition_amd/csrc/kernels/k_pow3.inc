// k_pow3.inc -- part of the ONE translation unit hip_ops.hip (textually included there, inside namespace petal): K3: the fused power-iteration pass (k_pow3, k_pow3f).
// ------------------------------------------------------------------------------------------------
// K3 "k_pow3": one power-iteration pass  Y' = Xc^T (Xc P)  (pca.rs:711 + 714) with ONE pass over X -- the two products K1 and K2
// form from two, and no Z in between (round 5).  For K = 512 features and N = 16 NT <= 80 columns; P is the re-based iterate
// DEFINED on two bf16 planes (k_trsm_pack<NB, true>) or a two-plane sketch matrix, so a wave's slice of it fits its registers.
//
// One persistent 8-wave workgroup per CU walks over 32-row stages of X.  Wave w owns the features [64 w, 64 w + 64) in BOTH
// products:
//   * its slice of P sits in registers for the whole launch as MFMA B operands (2 chunks x NT tiles x 2 planes = 80 VGPRs at
//     NT = 5), its slice of the Y' accumulators likewise (4 x NT tiles = 80 VGPRs);
//   * it loads its 32 x 64 piece of the stage in K1's layout (lane (i, q): row 16 t + i, features 32 c + 8 q .. + 7: two 16-B
//     loads), one stage ahead, centres and splits it ONCE into three bf16 planes -- which feed product 1 from registers and go to
//     a wave-private LDS image that product 2 reads back TRANSPOSED with ds_read_b64_tr_b16 (its A operand wants feature i with
//     eight samples per lane): X goes through the vector-memory pipeline once per power iteration;
//   * product 1 gives the wave a PARTIAL z (its 64 of the 512 features) per 16-row half of the stage, in accumulator layout
//     (lane (i, q): samples 4 q + r, column 16 u + i).  The eight partials meet in LDS; wave u < NT adds them for column tile u --
//     after both halves a lane holds the eight samples {4 q + r, 16 + 4 q + r} of one column, which IS a B-operand fragment of
//     product 2 once its k-slots are declared to be those samples (the X side reads its transposed blocks at the same rows) --
//     splits the sum into three planes and publishes the fragment; rows beyond n are zeroed here (their X rows are clamped
//     loads of the last row), and the last pass of a fit stores z as the iterate Z;
//   * product 2 accumulates Y'[64 w .. + 64][:] += Xc^T z over the stage (six piece products, smallest first, as K2).
// LDS: X planes 8 x 12 KB (16-B chunks XOR-swizzled by the row so that the row writes and the transposed reads are both
// conflict-free on 128-B rows), partial z 8 x NT KB, z fragments 3 NT KB, mu 2 KB: 153 KB at NT = 5 -- one workgroup per CU, two
// waves per SIMD, <= 256 registers.  Four barriers per stage (the partial-z buffer holds ONE half: there is no room for two).
// Every workgroup ends with its own 512 x 16 NT fp32 slab of Y', combined in fp64 in a fixed order by k_sum_parts4 like K2's.
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ bf16x8 lds_tr2(const unsigned char* a0, const unsigned char* a1) {
    typedef __attribute__((address_space(3))) s16x4* lp;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(a0));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(a1));
    return __builtin_bit_cast(bf16x8, s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]});
}
// byte offset of 16-B chunk `ch` (eight features) of row `row` inside one plane of a wave's image ([32 rows][128 B])
__device__ __forceinline__ int pow3_xoff(int row, int ch) { return row * 128 + 16 * (ch ^ ((2 * ((row >> 1) & 3)) ^ (row & 1))); }
// MEANS (the FIRST pass of a fit, round 5): `mu` is only a provisional centre mu0 (the means of a strided row sample), and the pass
// gathers what the separate means pass used to: the LAST column of the last tile -- zero padding of P, so z is 0 there -- is set
// to 1 for every valid row, which makes Y'[:, 16 NT - 1] = Xc0^T 1 the column sums about mu0 (product 2 forms them for free) -- the
// sums of the operand PRODUCT 2 READS, in fp32 per slab: here the three planes that re-add to fl32(x - mu0), in k_pow3f the TWO-plane
// rounding of it (a bias of up to 2^-17 mean |x - mu0| per column on data of few distinct values: ops.h states the contract) -- and
// the splits accumulate sum (x - mu0)^2 over the valid rows (one partial per wave in ssq_part).  k_mean_fix then moves everything
// to the true centre mu = mu0 + delta, delta = sums / n:  Xc^T Xc P = Xc0^T Xc0 P - n delta (delta^T P),  sum (x - mu)^2 = ssq - n |delta|^2
// -- a rank-one correction of relative size (delta / sigma)^2, i.e. harmless, where the same identity about mu0 = 0 would cancel
// (mu / sigma)^2 of the product.
template <int NT, bool CENTER, bool STOREZ, bool MEANS = false, int FC = 2>   // FC: 32-feature chunks per wave: K = 256 FC features (round 6: 256 or 512)
__global__ __launch_bounds__(512) void k_pow3(const float* __restrict__ X, int64_t n, int64_t ldx, const float* __restrict__ mu,
                                              const bf16x8* __restrict__ Ppk3, int NTtot, float* __restrict__ part,
                                              float* __restrict__ Z, int64_t ldz, int64_t nstages, double* __restrict__ ssq_part) {
    constexpr int WV = 8, K = 256 * FC, XIMG = 3 * 32 * 128;          // bytes of one wave's plane image
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_pow3[];
    unsigned char* const sX = sm_pow3;                                           // [WV][3][32][128 B]
    f32x4* const sZp = reinterpret_cast<f32x4*>(sm_pow3 + WV * XIMG);            // [WV][NT][64]
    bf16x8* const sZB = reinterpret_cast<bf16x8*>(sm_pow3 + WV * XIMG + WV * NT * 1024);   // [NT][3][64]
    float* const sMu = reinterpret_cast<float*>(sm_pow3 + WV * XIMG + WV * NT * 1024 + NT * 3072);   // [K]
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);           // (uniform: scalar registers)
    // Register budget: two waves per SIMD leave 256, and P (80) + Y' (80) + the raw stage in flight (32) are fixed.  Every per-lane
    // index below is therefore re-derived, phase by phase, from a LAUNDERED copy of the thread index -- left to itself hipcc hoists
    // some thirty loop-invariant LDS offsets and pointers into registers of their own and spills P fragments to pay for them
    // (each reload then waits behind the stage's X loads: vmcnt retires in order -- 7300 cycles for a 1300-cycle phase, measured).
#define POW3_LANE(ln) int ln = threadIdx.x & 63; asm volatile("" : "+v"(ln))
#ifndef PETAL_POW3_ZPF
#define PETAL_POW3_ZPF 0
#endif
#ifndef PETAL_POW3_DEPHASE
#define PETAL_POW3_DEPHASE 0
#endif
    if (CENTER)
        for (int k = threadIdx.x; k < K; k += 64 * WV) sMu[k] = mu[k];
    // this wave's slice of P: chunk c <-> features 64 wave + 32 c .. + 32, B-operand fragments of the packed planes (k_pack_p3's
    // layout: lane (j, q) holds P[32 c' + 8 q + e][16 u + j])
    bf16x8 ph[FC][NT], pm[FC][NT];
    {
        POW3_LANE(ln);
#pragma unroll
        for (int c = 0; c < FC; ++c)
#pragma unroll
            for (int u = 0; u < NT; ++u) {
                const bf16x8* src = Ppk3 + (((int64_t)(FC * wave + c) * NTtot + u) * 3) * 64 + ln;
                ph[c][u] = src[0];
                pm[c][u] = src[64];
            }
    }
    f32x4 acc2[2 * FC][NT];
#pragma unroll
    for (int m = 0; m < 2 * FC; ++m)
#pragma unroll
        for (int u = 0; u < NT; ++u) acc2[m][u] = f32x4{0.f, 0.f, 0.f, 0.f};
    // stage range of this workgroup (contiguous, balanced to one stage)
    const int64_t s0 = (int64_t)blockIdx.x * nstages / gridDim.x, s1 = (int64_t)(blockIdx.x + 1) * nstages / gridDim.x;
    f32x8 xa[2][FC];
    auto load_x = [&](int64_t s) {
        POW3_LANE(ln);
        const int li = ln & 15, lq = ln >> 4;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int64_t r = min(s * 32 + 16 * t + li, n - 1);   // rows beyond n: the last row (finite); their z is zeroed below
            const float* p = X + r * ldx + 32 * FC * wave + 8 * lq;
#pragma unroll
            for (int c = 0; c < FC; ++c) {
                const f32x4 lo = ld_stream(p + 32 * c), hi = ld_stream(p + 32 * c + 4);
                xa[t][c] = f32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            }
        }
    };
    if (s0 < s1) load_x(s0);
    unsigned char* const myX = sX + wave * XIMG;
    // product 1 of one 16-row half: operands read back from the wave's image (rows 16 h + i), X fragment as A (rows = samples), P
    // fragment as B; five piece products per tile, smallest first
    auto prod1 = [&](f32x4(&acc1)[NT], int h) {
        POW3_LANE(ln);
        const int li = ln & 15, lq = ln >> 4;
#pragma unroll
        for (int c = 0; c < FC; ++c) {
            const unsigned char* a = myX + pow3_xoff(16 * h + li, 4 * c + lq);
            const bf16x8 xh = *reinterpret_cast<const bf16x8*>(a), xm = *reinterpret_cast<const bf16x8*>(a + 4096),
                         xl = *reinterpret_cast<const bf16x8*>(a + 8192);
#pragma unroll
            for (int u = 0; u < NT; ++u) {
                f32x4 c4 = acc1[u];
                c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xl, ph[c][u], c4, 0, 0, 0);
                c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xm, pm[c][u], c4, 0, 0, 0);
                c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xm, ph[c][u], c4, 0, 0, 0);
                c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, pm[c][u], c4, 0, 0, 0);
                c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, ph[c][u], c4, 0, 0, 0);
                acc1[u] = c4;
            }
        }
    };
    auto park_partials = [&](const f32x4(&acc1)[NT]) {
        POW3_LANE(ln);
#pragma unroll
        for (int u = 0; u < NT; ++u) sZp[(wave * NT + u) * 64 + ln] = acc1[u];
    };
    // wave u < NT adds the eight partials of column tile u (fixed order)
    auto add_partials = [&]() {
        POW3_LANE(ln);
        f32x4 zs = sZp[(0 * NT + wave) * 64 + ln];
#pragma unroll
        for (int w = 1; w < WV; ++w) zs += sZp[(w * NT + wave) * 64 + ln];
        return zs;
    };
    // the raw fragments of feature chunk c (both row tiles): centred, split into three planes, parked in the wave's image; one
    // piece at a time (two splits in flight cost 28 registers)
    float ssq = 0.f;
    auto split_park = [&](int c, int64_t sidx) {
        POW3_LANE(ln);
        const int li = ln & 15, lq = ln >> 4;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            f32x8 x = xa[t][c];
            if (CENTER) {
                const float* mp = sMu + 32 * FC * wave + 32 * c + 8 * lq;
                const f32x4 lo = *reinterpret_cast<const f32x4*>(mp), hi = *reinterpret_cast<const f32x4*>(mp + 4);
                x -= f32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            }
            if (MEANS) {   // sum (x - mu0)^2 over the valid rows (rows beyond n are clamped loads of the last row)
                float q2 = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) q2 = fmaf(x[e], x[e], q2);
                ssq += sidx * 32 + 16 * t + li < n ? q2 : 0.f;
            }
            bf16x8 xh, xm, xl;
            split3(x, xh, xm, xl);
            unsigned char* a = myX + pow3_xoff(16 * t + li, 4 * c + lq);
            *reinterpret_cast<bf16x8*>(a) = xh;
            *reinterpret_cast<bf16x8*>(a + 4096) = xm;
            *reinterpret_cast<bf16x8*>(a + 8192) = xl;
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    __syncthreads();   // mu
    // Software pipeline over the stages: the planes of stage s + 1 are produced UNDER product 2 of stage s -- its feature tile m
    // reads chunks 2 m, 2 m + 1 of every row, so once the fragments of tiles 0, 1 are in registers the image's first half (chunks
    // 0 .. 3) is free for the next stage's c = 0 pieces, and after those of tiles 2, 3 the second half: the split (180 VALU instructions and twelve
    // 16-B LDS stores per wave and stage) runs beside the other wave's MFMAs instead of in front of everybody's (phase stamps,
    // round 5: the split at the head of the stage was 1400 of its 16000 cycles with the matrix pipe idle).
    if (s0 < s1) {
#pragma unroll
        for (int c = 0; c < FC; ++c) split_park(c, s0);
        if (s0 + 1 < s1) load_x(s0 + 1);
    }
#ifdef PETAL_DEBUG_COUNTERS
    long long php[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    long long tqp = __builtin_amdgcn_s_memtime();
#define POW3_STAMP(i) do { const long long _t = __builtin_amdgcn_s_memtime(); php[i] += _t - tqp; tqp = _t; \
        if (blockIdx.x == 7 && s == s0 + 5 && (threadIdx.x & 63) == 0) g_trace[wave * 16 + (i)] = _t; } while (0)
#else
#define POW3_STAMP(i) do {} while (0)
#endif
    for (int64_t s = s0; s < s1; ++s) {
        f32x4 zlo = f32x4{0.f, 0.f, 0.f, 0.f}, zhi = zlo;
        {
            f32x4 acc1[NT];
#pragma unroll
            for (int u = 0; u < NT; ++u) acc1[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            prod1(acc1, 0);
            POW3_STAMP(0);
            park_partials(acc1);                 // (ordered behind the previous stage's adders by that stage's last barrier)
            __syncthreads();
            POW3_STAMP(1);
            if (wave < NT) zlo = add_partials();
            POW3_STAMP(2);
        }
        {
            f32x4 acc1[NT];
#pragma unroll
            for (int u = 0; u < NT; ++u) acc1[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            prod1(acc1, 1);
            POW3_STAMP(3);
            __syncthreads();                     // the adders have read the first half's partials
            park_partials(acc1);
            __syncthreads();
            POW3_STAMP(4);
            if (wave < NT) zhi = add_partials();
        }
        if (wave < NT) {
            // lane (i, q): z[row 4 q + r][16 wave + i] (zlo), z[16 + 4 q + r][...] (zhi); rows beyond n are zeroed
            POW3_LANE(ln);
            const int li = ln & 15, lq = ln >> 4;
            const int64_t rb = s * 32 + 4 * lq;
            f32x8 z8;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                z8[r] = rb + r < n ? zlo[r] : 0.f;
                z8[4 + r] = rb + 16 + r < n ? zhi[r] : 0.f;
            }
            if (MEANS && wave == NT - 1 && li == 15) {   // the all-ones column: Y'[:, 16 NT - 1] = Xc0^T 1
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    z8[r] = rb + r < n ? 1.f : 0.f;
                    z8[4 + r] = rb + 16 + r < n ? 1.f : 0.f;
                }
            }
            if (STOREZ) {
                float* zp = Z + rb * ldz + 16 * wave + li;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (rb + r < n) zp[r * ldz] = z8[r];
                    if (rb + 16 + r < n) zp[(16 + r) * ldz] = z8[4 + r];
                }
            }
            bf16x8 zh, zm, zl;
            split3(z8, zh, zm, zl);
            sZB[(wave * 3 + 0) * 64 + ln] = zh;
            sZB[(wave * 3 + 1) * 64 + ln] = zm;
            sZB[(wave * 3 + 2) * 64 + ln] = zl;
        }
        POW3_STAMP(5);
        __syncthreads();                         // the z fragments of this stage are published
        POW3_STAMP(6);
        // product 2: Y'[16 m + 4 q + r][16 u + i] += sum over the stage's samples; A = X^T (transposed reads), B = z fragments.
        // Transposed-read addresses (T10): lane 16 g + 4 q' + p of group g supplies block row q', columns 4 p .. 4 p + 3; the block
        // of k-slots e < 4 is rows 4 g + q', of e >= 4 rows 16 + 4 g + q' (g = q: the lane group IS the k group of the operand).
        {
            POW3_LANE(ln);
            const int trq = (ln >> 2) & 3, trp = ln & 3, lq = ln >> 4;
            // the twelve MFMAs per column tile of one pair of feature tiles (one set of z fragments; with ZPF the next tile's set is
            // fetched under them -- the raw registers of the pieces already split are free by then)
            auto mfma_pair = [&](const bf16x8(&ax)[2][3], int mp) {
#if PETAL_POW3_ZPF
                bf16x8 zc[3];
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) zc[pl] = sZB[(0 * 3 + pl) * 64 + ln];
#endif
#pragma unroll
                for (int u = 0; u < NT; ++u) {
                    __builtin_amdgcn_sched_barrier(0);
#if PETAL_POW3_ZPF
                    const bf16x8 zh = zc[0], zm = zc[1], zl = zc[2];
                    if (u + 1 < NT) {
#pragma unroll
                        for (int pl = 0; pl < 3; ++pl) zc[pl] = sZB[((u + 1) * 3 + pl) * 64 + ln];
                    }
                    __builtin_amdgcn_sched_barrier(0);
#else
                    // (ONE set of z fragments, re-read for each pair of feature tiles: its latency is covered by the twelve MFMAs of the
                    // other wave of the SIMD)
                    const bf16x8 zh = sZB[(u * 3 + 0) * 64 + ln], zm = sZB[(u * 3 + 1) * 64 + ln], zl = sZB[(u * 3 + 2) * 64 + ln];
#endif
#pragma unroll
                    for (int mm = 0; mm < 2; ++mm) {
                        f32x4 c4 = acc2[2 * mp + mm][u];
                        c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax[mm][2], zh, c4, 0, 0, 0);   // smallest terms first
                        c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax[mm][1], zm, c4, 0, 0, 0);
                        c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax[mm][0], zl, c4, 0, 0, 0);
                        c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax[mm][1], zh, c4, 0, 0, 0);
                        c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax[mm][0], zm, c4, 0, 0, 0);
                        c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax[mm][0], zh, c4, 0, 0, 0);
                        acc2[2 * mp + mm][u] = c4;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
#pragma unroll
            for (int mp = 0; mp < FC; ++mp) {     // feature tiles in PAIRS: one set of z fragments feeds twelve MFMAs
                bf16x8 ax[2][3];
#pragma unroll
                for (int mm = 0; mm < 2; ++mm) {
                    const unsigned char* a0 = myX + pow3_xoff(4 * lq + trq, 2 * (2 * mp + mm) + (trp >> 1)) + 8 * (trp & 1);   // (row + 16: + 2048, same swizzle)
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl) ax[mm][pl] = lds_tr2(a0 + pl * 4096, a0 + pl * 4096 + 2048);
                }
                // this half of the image has been read for the last time: the next stage's pieces go there.  The two waves of a SIMD
                // (w, w + 4) take the split and the MFMAs in OPPOSITE order (DEPHASE), so that one's VALU run meets the other's MFMAs
                // instead of its VALU run
#if PETAL_POW3_DEPHASE
                const bool split_first = wave < 4;
#else
                const bool split_first = true;
#endif
                if (split_first && s + 1 < s1) {
                    __builtin_amdgcn_sched_barrier(0);
                    split_park(mp, s + 1);
                }
                mfma_pair(ax, mp);
                if (!split_first && s + 1 < s1) {
                    __builtin_amdgcn_sched_barrier(0);
                    split_park(mp, s + 1);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        // (the next stage's first barrier orders these reads of the z fragments and of the partial buffer before they are rewritten)
        if (s + 2 < s1) load_x(s + 2);           // the raw registers are free again: three quarters of a stage ahead of their use
        POW3_STAMP(7);
    }
#ifdef PETAL_DEBUG_COUNTERS
    if ((threadIdx.x & 63) == 0) {
        for (int e = 0; e < 8; ++e) atomicAdd((unsigned long long*)&g_cyc[e], (unsigned long long)php[e]);
        atomicAdd((unsigned long long*)&g_cyc[8], (unsigned long long)(s1 - s0));
    }
#endif
    if (MEANS) {         // one partial of sum (x - mu0)^2 per wave, lanes added in a fixed order
        float v = ssq;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((threadIdx.x & 63) == 0) ssq_part[(int64_t)blockIdx.x * WV + wave] = (double)v;
    }
    // this workgroup's slab: D[row = 4 q + r][col = i] of tile (m, u) is Y'[64 wave + 16 m + 4 q + r][16 u + i]
    {
        POW3_LANE(ln);
        const int li = ln & 15, lq = ln >> 4;
        float* out = part + (int64_t)blockIdx.x * K * (16 * NT);
#pragma unroll
        for (int m = 0; m < 2 * FC; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float* row = out + (int64_t)(32 * FC * wave + 16 * m + 4 * lq + r) * (16 * NT);
#pragma unroll
                for (int u = 0; u < NT; ++u) row[16 * u + li] = acc2[m][u][r];
            }
    }
#undef POW3_LANE
}

// ---- k_pow3f: the fused pass for the INTERMEDIATE power iterations (late round 5).  A pass whose result only steers the iteration --
// every pass but the last one of a fit, whose Y' and Z become B and Q -- may round its operands like the iterate already is: X (after
// centring) and z to 16 significant bits, two bf16 planes each.  That is a perturbation of the same kind and size as the two-plane P
// (numpy model dev/x2_model.py: component errors against the oracle 1.1e-7 -> 3.8e-7 on planted spectra, unchanged on the slowly decaying
// ones, where the spectral verdict sends the fit to the exact pipeline anyway), and it changes the kernel's budget: FOUR piece
// products per tile in both products instead of five and six (160 MFMAs per wave and stage instead of 220), a third less split work, an
// X image of 64 KB instead of 96 -- which leaves room for the partial z of BOTH 16-row halves (80 KB), so a stage has TWO barriers
// instead of four: product 1 of both halves, park, barrier, add + publish z, barrier, product 2.
#define POW3_LANE(ln) int ln = threadIdx.x & 63; asm volatile("" : "+v"(ln))
#ifndef PETAL_POW3F_ZPF
#define PETAL_POW3F_ZPF 0
#endif
#ifndef PETAL_POW3F_DEPHASE
#define PETAL_POW3F_DEPHASE 0
#endif
// MEANS: as k_pow3's (the first pass of a fit about a provisional centre: the last column of z set to one gathers the column sums, the
// splits accumulate sum (x - mu0)^2 -- from the values BEFORE their rounding; the sums themselves are those of the 16-bit values, off the
// exact ones by 2^-17 sigma / sqrt(n) per column on continuous data: 1e-8 sigma at the 200000 rows the fold starts from -- and by up
// to 2^-17 mean |x - mu0|, whatever n, on columns of few distinct values, where equal values round alike: ops.h, op_power_pass_means).
template <int NT, bool CENTER, bool MEANS = false, int FC = 2>
__global__ __launch_bounds__(512) void k_pow3f(const float* __restrict__ X, int64_t n, int64_t ldx, const float* __restrict__ mu,
                                               const bf16x8* __restrict__ Ppk3, int NTtot, float* __restrict__ part, int64_t nstages,
                                               double* __restrict__ ssq_part) {
    constexpr int WV = 8, K = 256 * FC, XIMG = 2 * 32 * 128;          // bytes of one wave's two-plane image
    extern __shared__ __attribute__((aligned(16))) unsigned char sm_pow3[];
    unsigned char* const sX = sm_pow3;                                           // [WV][2][32][128 B]
    f32x4* const sZp = reinterpret_cast<f32x4*>(sm_pow3 + WV * XIMG);            // [2][WV][NT][64]
    bf16x8* const sZB = reinterpret_cast<bf16x8*>(sm_pow3 + WV * XIMG + 2 * WV * NT * 1024);   // [NT][2][64]
    float* const sMu = reinterpret_cast<float*>(sm_pow3 + WV * XIMG + 2 * WV * NT * 1024 + NT * 2048);   // [K]
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (CENTER)
        for (int k = threadIdx.x; k < K; k += 64 * WV) sMu[k] = mu[k];
    bf16x8 ph[FC][NT], pm[FC][NT];
    {
        POW3_LANE(ln);
#pragma unroll
        for (int c = 0; c < FC; ++c)
#pragma unroll
            for (int u = 0; u < NT; ++u) {
                const bf16x8* src = Ppk3 + (((int64_t)(FC * wave + c) * NTtot + u) * 3) * 64 + ln;
                ph[c][u] = src[0];
                pm[c][u] = src[64];
            }
    }
    f32x4 acc2[2 * FC][NT];
#pragma unroll
    for (int m = 0; m < 2 * FC; ++m)
#pragma unroll
        for (int u = 0; u < NT; ++u) acc2[m][u] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int64_t s0 = (int64_t)blockIdx.x * nstages / gridDim.x, s1 = (int64_t)(blockIdx.x + 1) * nstages / gridDim.x;
    f32x8 xa[2][FC];
    auto load_x = [&](int64_t s) {
        POW3_LANE(ln);
        const int li = ln & 15, lq = ln >> 4;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int64_t r = min(s * 32 + 16 * t + li, n - 1);   // rows beyond n: the last row (finite); their z is zeroed below
            const float* p = X + r * ldx + 32 * FC * wave + 8 * lq;
#pragma unroll
            for (int c = 0; c < FC; ++c) {
                const f32x4 lo = ld_stream(p + 32 * c), hi = ld_stream(p + 32 * c + 4);
                xa[t][c] = f32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            }
        }
    };
    if (s0 < s1) load_x(s0);
    unsigned char* const myX = sX + wave * XIMG;
    auto prod1 = [&](f32x4(&acc1)[NT], int h) {
        POW3_LANE(ln);
        const int li = ln & 15, lq = ln >> 4;
#pragma unroll
        for (int c = 0; c < FC; ++c) {
            const unsigned char* a = myX + pow3_xoff(16 * h + li, 4 * c + lq);
            const bf16x8 xh = *reinterpret_cast<const bf16x8*>(a), xm = *reinterpret_cast<const bf16x8*>(a + 4096);
#pragma unroll
            for (int u = 0; u < NT; ++u) {
                f32x4 c4 = acc1[u];
#if PETAL_STEER_PIECES >= 4
                c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xm, pm[c][u], c4, 0, 0, 0);   // smallest terms first
#endif
                c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xm, ph[c][u], c4, 0, 0, 0);
                c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, pm[c][u], c4, 0, 0, 0);
                c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xh, ph[c][u], c4, 0, 0, 0);
                acc1[u] = c4;
            }
        }
    };
    auto park_partials = [&](const f32x4(&acc1)[NT], int h) {
        POW3_LANE(ln);
#pragma unroll
        for (int u = 0; u < NT; ++u) sZp[((h * WV + wave) * NT + u) * 64 + ln] = acc1[u];
    };
    auto add_partials = [&](int h) {     // wave u < NT adds the eight partials of column tile u (fixed order)
        POW3_LANE(ln);
        f32x4 zs = sZp[((h * WV + 0) * NT + wave) * 64 + ln];
#pragma unroll
        for (int w = 1; w < WV; ++w) zs += sZp[((h * WV + w) * NT + wave) * 64 + ln];
        return zs;
    };
    float ssq = 0.f;
    auto split_park = [&](int c, int64_t sidx) {
        POW3_LANE(ln);
        const int li = ln & 15, lq = ln >> 4;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            f32x8 x = xa[t][c];
            if (CENTER) {
                const float* mp = sMu + 32 * FC * wave + 32 * c + 8 * lq;
                const f32x4 lo = *reinterpret_cast<const f32x4*>(mp), hi = *reinterpret_cast<const f32x4*>(mp + 4);
                x -= f32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            }
            if (MEANS) {   // sum (x - mu0)^2 over the valid rows (rows beyond n are clamped loads of the last row)
                float q2 = 0.f;
#pragma unroll
                for (int e = 0; e < 8; ++e) q2 = fmaf(x[e], x[e], q2);
                ssq += sidx * 32 + 16 * t + li < n ? q2 : 0.f;
            }
            bf16x8 xh, xm;
            split2(x, xh, xm);
            unsigned char* a = myX + pow3_xoff(16 * t + li, 4 * c + lq);
            *reinterpret_cast<bf16x8*>(a) = xh;
            *reinterpret_cast<bf16x8*>(a + 4096) = xm;
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    __syncthreads();   // mu
    if (s0 < s1) {
#pragma unroll
        for (int c = 0; c < FC; ++c) split_park(c, s0);
        if (s0 + 1 < s1) load_x(s0 + 1);
    }
    for (int64_t s = s0; s < s1; ++s) {
        {
            f32x4 acc1[NT];
#pragma unroll
            for (int u = 0; u < NT; ++u) acc1[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            prod1(acc1, 0);
            park_partials(acc1, 0);              // (ordered behind the previous stage's adders by that stage's second barrier)
#pragma unroll
            for (int u = 0; u < NT; ++u) acc1[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            prod1(acc1, 1);
            park_partials(acc1, 1);
        }
        __syncthreads();
        if (wave < NT) {
            POW3_LANE(ln);
            const int lq = ln >> 4;
            const int64_t rb = s * 32 + 4 * lq;
            f32x8 z8;
            {
                const f32x4 zlo = add_partials(0);
#pragma unroll
                for (int r = 0; r < 4; ++r) z8[r] = rb + r < n ? zlo[r] : 0.f;
            }
            {
                const f32x4 zhi = add_partials(1);
#pragma unroll
                for (int r = 0; r < 4; ++r) z8[4 + r] = rb + 16 + r < n ? zhi[r] : 0.f;
            }
            if (MEANS && wave == NT - 1 && (ln & 15) == 15) {   // the all-ones column: Y'[:, 16 NT - 1] = Xc0^T 1
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    z8[r] = rb + r < n ? 1.f : 0.f;
                    z8[4 + r] = rb + 16 + r < n ? 1.f : 0.f;
                }
            }
            bf16x8 zh, zm;
            split2(z8, zh, zm);
            sZB[(wave * 2 + 0) * 64 + ln] = zh;
            sZB[(wave * 2 + 1) * 64 + ln] = zm;
        }
        __syncthreads();                         // the z fragments of this stage are published
        {
            POW3_LANE(ln);
            const int trq = (ln >> 2) & 3, trp = ln & 3, lq = ln >> 4;
            auto mfma_pair = [&](const bf16x8(&ax)[2][2], int mp) {
#if PETAL_POW3F_ZPF
                bf16x8 zc[2];
                zc[0] = sZB[(0 * 2 + 0) * 64 + ln]; zc[1] = sZB[(0 * 2 + 1) * 64 + ln];
#endif
#pragma unroll
                for (int u = 0; u < NT; ++u) {
                    __builtin_amdgcn_sched_barrier(0);
#if PETAL_POW3F_ZPF
                    const bf16x8 zh = zc[0], zm = zc[1];
                    if (u + 1 < NT) { zc[0] = sZB[((u + 1) * 2 + 0) * 64 + ln]; zc[1] = sZB[((u + 1) * 2 + 1) * 64 + ln]; }
                    __builtin_amdgcn_sched_barrier(0);
#else
                    const bf16x8 zh = sZB[(u * 2 + 0) * 64 + ln], zm = sZB[(u * 2 + 1) * 64 + ln];
#endif
#pragma unroll
                    for (int mm = 0; mm < 2; ++mm) {
                        f32x4 c4 = acc2[2 * mp + mm][u];
#if PETAL_STEER_PIECES >= 4
                        c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax[mm][1], zm, c4, 0, 0, 0);   // smallest terms first
#endif
                        c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax[mm][1], zh, c4, 0, 0, 0);
                        c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax[mm][0], zm, c4, 0, 0, 0);
                        c4 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ax[mm][0], zh, c4, 0, 0, 0);
                        acc2[2 * mp + mm][u] = c4;
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            };
#pragma unroll
            for (int mp = 0; mp < FC; ++mp) {
                bf16x8 ax[2][2];
#pragma unroll
                for (int mm = 0; mm < 2; ++mm) {
                    const unsigned char* a0 = myX + pow3_xoff(4 * lq + trq, 2 * (2 * mp + mm) + (trp >> 1)) + 8 * (trp & 1);
#pragma unroll
                    for (int pl = 0; pl < 2; ++pl) ax[mm][pl] = lds_tr2(a0 + pl * 4096, a0 + pl * 4096 + 2048);
                }
                // this half of the image has been read for the last time: the next stage's pieces go there -- in front of the pair's MFMAs
                // in one wave of a SIMD, behind them in the other (DEPHASE)
#if PETAL_POW3F_DEPHASE
                const bool split_first = wave < 4;
#else
                const bool split_first = true;
#endif
                if (split_first && s + 1 < s1) {
                    __builtin_amdgcn_sched_barrier(0);
                    split_park(mp, s + 1);
                }
                mfma_pair(ax, mp);
                if (!split_first && s + 1 < s1) {
                    __builtin_amdgcn_sched_barrier(0);
                    split_park(mp, s + 1);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
        if (s + 2 < s1) load_x(s + 2);
    }
    if (MEANS) {         // one partial of sum (x - mu0)^2 per wave, lanes added in a fixed order
        float v = ssq;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((threadIdx.x & 63) == 0) ssq_part[(int64_t)blockIdx.x * WV + wave] = (double)v;
    }
    // this workgroup's slab: D[row = 4 q + r][col = i] of tile (m, u) is Y'[64 wave + 16 m + 4 q + r][16 u + i]
    {
        POW3_LANE(ln);
        const int li = ln & 15, lq = ln >> 4;
        float* out = part + (int64_t)blockIdx.x * K * (16 * NT);
#pragma unroll
        for (int m = 0; m < 2 * FC; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float* row = out + (int64_t)(32 * FC * wave + 16 * m + 4 * lq + r) * (16 * NT);
#pragma unroll
                for (int u = 0; u < NT; ++u) row[16 * u + li] = acc2[m][u][r];
            }
    }
#undef POW3_LANE
}


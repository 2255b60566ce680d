// k_smallmat.inc -- part of the ONE translation unit hip_ops.hip (textually included there, inside namespace petal): fp64 small-matrix kernels: k_dgemm, k_trsm_pack, k_trsm_left_pack, k_chol_inv2, k_chol_rt4, Jacobi solvers.
// ================================================================================================
// fp64 small-matrix kernels
// ================================================================================================
// C[M x N] = alpha op(A) op(B) + beta C, fp64, 16 x 16 outputs per block, 32-deep K steps; the global loads are
// coalesced for every transposition case (the transposed operand is read along its contiguous index and
// transposed on the way into LDS).
// Split-K form (gridDim.z > 1, used when K is long and the output small): slice z covers K-range [z kchunk, (z+1) kchunk)
// and writes its raw partial tile to part[z][M][N]; k_dgemm_reduce adds the slices in fixed order (deterministic).
__global__ __launch_bounds__(256) void k_dgemm(bool ta, bool tb, int64_t M, int64_t N, int64_t K, double alpha,
                                               const double* __restrict__ A, int64_t lda, const double* __restrict__ B, int64_t ldb,
                                               double beta, double* __restrict__ C, int64_t ldc, int64_t kchunk,
                                               double* __restrict__ part, const double* __restrict__ colscale,
                                               bf16x8* __restrict__ pk3, int NTtot) {
    constexpr int BK = 32;
    __shared__ double sa[16][BK + 1], sb[BK][17];
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int64_t i0 = (int64_t)blockIdx.y * 16, j0 = (int64_t)blockIdx.x * 16;
    const int64_t kbeg = (int64_t)blockIdx.z * kchunk;
    if (K > kbeg + kchunk) K = kbeg + kchunk;
    double acc = 0;
    for (int64_t k0 = kbeg; k0 < K; k0 += BK) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (ta) {  // A is K x M: contiguous in i
                const int kk = ty + 16 * h;
                const int64_t k = k0 + kk, i = i0 + tx;
                sa[tx][kk] = (i < M && k < K) ? A[k * lda + i] : 0.0;
            } else {   // A is M x K: contiguous in k
                const int kk = tx + 16 * h;
                const int64_t k = k0 + kk, i = i0 + ty;
                sa[ty][kk] = (i < M && k < K) ? A[i * lda + k] : 0.0;
            }
            if (tb) {  // B is N x K: contiguous in k
                const int kk = tx + 16 * h;
                const int64_t k = k0 + kk, j = j0 + ty;
                sb[kk][ty] = (j < N && k < K) ? B[j * ldb + k] : 0.0;
            } else {   // B is K x N: contiguous in j
                const int kk = ty + 16 * h;
                const int64_t k = k0 + kk, j = j0 + tx;
                sb[kk][tx] = (j < N && k < K) ? B[k * ldb + j] : 0.0;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < BK; ++k) acc += sa[ty][k] * sb[k][tx];
        __syncthreads();
    }
    const int64_t i = i0 + ty, j = j0 + tx;
    if (i < M && j < N) {
        if (part) part[((int64_t)blockIdx.z * M + i) * N + j] = acc;
        else C[i * ldc + j] = alpha * acc * (colscale ? colscale[j] : 1.0) + (beta != 0.0 ? beta * C[i * ldc + j] : 0.0);
    }
    if (pk3) {
        // the product is the small operand of the next split-product GEMM (op_gemm_xp_prod): emit its three bf16 planes in
        // k_pack_p3's layout straight from this tile -- rows i0 .. i0 + 15 are two 8-row operand groups of chunk i0 / 32,
        // columns j0 .. j0 + 15 one column tile.  (M, N multiples of 16; beta = 0, no split-K.)
        __syncthreads();
        float* sv = reinterpret_cast<float*>(&sa[0][0]);  // [16][17] floats
        sv[ty * 17 + tx] = (i < M && j < N) ? (float)(alpha * acc) : 0.f;
        __syncthreads();
        if ((ty & 7) == 0) {
            f32x8 x;
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = sv[(ty + e) * 17 + tx];
            bf16x8 h, m, l;
            split3(x, h, m, l);
            const int64_t c = i0 >> 5, tile = c * NTtot + (j0 >> 4);
            const int lane = tx + 16 * (int)(((i0 & 31) + ty) >> 3);
            pk3[(tile * 3 + 0) * 64 + lane] = h;
            pk3[(tile * 3 + 1) * 64 + lane] = m;
            pk3[(tile * 3 + 2) * 64 + lane] = l;
            if ((M & 31) == 16 && i0 + 16 == M) {   // the last 32-row chunk is half empty: its upper operand groups are zeros
                bf16x8 z; for (int e = 0; e < 8; ++e) z[e] = (__bf16)0.0f;
#pragma unroll
                for (int pl = 0; pl < 3; ++pl) pk3[(tile * 3 + pl) * 64 + lane + 32] = z;
            }
        }
    }
}
__global__ __launch_bounds__(256) void k_dgemm_reduce(const double* __restrict__ part, int ks, int64_t M, int64_t N, double alpha,
                                                      double beta, double* __restrict__ C, int64_t ldc,
                                                      const double* __restrict__ colscale) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= M * N) return;
    double acc = 0;
    for (int z = 0; z < ks; ++z) acc += part[(int64_t)z * M * N + e];
    const int64_t i = e / N, j = e - i * N;
    C[i * ldc + j] = alpha * acc * (colscale ? colscale[j] : 1.0) + (beta != 0.0 ? beta * C[i * ldc + j] : 0.0);
}

// P = A . R^-1 for an upper-triangular R given in "RT form" (k_chol_inv2, rt_form: diagonal 16 x 16 blocks hold T_JJ = R_JJ^-1, the
// blocks above them R itself): blocked forward substitution P_J = (A_J - sum_{I < J} P_I R_IJ) T_JJ on the fp64 matrix cores, ONE
// WAVE per 16 rows of A (rows are independent), transposed so that results feed the next product without leaving the registers:
// X_J = A_J^T lives in the accumulator layout of v_mfma_f64_16x16x4 (register r of lane l = X[(l >> 4) + 4 r][l & 15]);
// P_I^T = T_II^T X_I and X_J -= R_IJ^T P_I^T take those registers directly as the B operands of MFMA r (the k index is summed
// over, so the accumulator's k' = (l >> 4) + 4 r order is as good as any when the A operand uses the same one).  The R / T
// operands come straight from L2 (16 consecutive doubles per row), none of them on the dependency chain, which is
// nb x 8 MFMAs long.  Epilogue as k_dgemm's: P (fp64) and the three bf16 operand planes of the next split-product GEMM (k_pack_p3's
// layout), through one LDS transpose.  M (the order of R) is a multiple of 16, <= 144; K a multiple of 16.
typedef double cf64x4 __attribute__((ext_vector_type(4)));
constexpr int TRSM_MAXM = 144;
__host__ __device__ inline size_t trsm_lds_bytes(int M) { return sizeof(double) * 16 * (size_t)(M + 2); }
// P2: the result is ROUNDED to the sum of its two leading bf16 pieces, P := bf16(p) + bf16(p - bf16(p)) (16 significant bits), in
// P_out too -- the re-based iterate may be any basis of range(A), so this rounding defines the iterate instead of perturbing a
// product (numpy model, configs[1] / configs[3] spectra: no change in the 5e-6 / 1.5e-5 component errors), and the next product
// needs five piece products instead of six (k_xp3<..., NPL = 2>).  The third plane is not written.
// Both pieces are rounded (to nearest, ties to even) FROM THE fp64 VALUE, h = bf16(p), m = bf16(p - h) with p - h exact in fp64, so that
// |P - p| <= 2^-17 |p|: through float32 first the conversion's 2^-24 |p| came on top (one element in some 25000 was up to 1.004 x
// 2^-17 off).  Where h + m would not be a float32 number (|p - h| below the float32 resolution of p: m then carries nothing the next
// product could read) m is taken from float32(p) - h instead, as before; the error there is below 2^-22 |p|.
__device__ __forceinline__ double rne8_f64(double v) {   // v to 8 significant bits (a bf16 number for every |v| in the float32 range)
    unsigned long long u = (unsigned long long)__double_as_longlong(v);
    u = (u + 0x00000FFFFFFFFFFFull + ((u >> 45) & 1ull)) & 0xFFFFE00000000000ull;
    return __longlong_as_double((long long)u);
}
__device__ __forceinline__ void two_plane_f64(double v, double& hd, double& md) {
    hd = rne8_f64(v);
    md = rne8_f64(v - hd);
    const double p = hd + md;
    if ((double)(float)p != p) md = rne8_f64((double)(float)v - hd);
}
template <int NB, bool P2 = false>   // NB = M / 16 at compile time: straight-line code, so every operand load is issued ahead of the MFMA chain
__global__ __launch_bounds__(64) void k_trsm_pack(const double* __restrict__ A, int64_t lda, const double* __restrict__ RT, int64_t ldt,
                                                  int64_t K, double* __restrict__ P_out, int64_t ldpo,
                                                  bf16x8* __restrict__ pk3, int NTtot) {
    extern __shared__ __attribute__((aligned(16))) double sP[];   // [16][M + 2]
    const int lane = threadIdx.x, li = lane & 15, lk = lane >> 4;
    constexpr int M = 16 * NB, ldsp = M + 2;
    const int64_t i0 = (int64_t)blockIdx.x * 16;
    cf64x4 X[NB];
#pragma unroll
    for (int J = 0; J < NB; ++J) {
#pragma unroll
        for (int r = 0; r < 4; ++r) X[J][r] = A[(i0 + li) * lda + 16 * J + lk + 4 * r];
    }
    // Block row I + 1 of RT is requested while block row I is being used (two register sets): with every operand requested up
    // front the 45 tiles of NB = 9 need 360 registers and the compiler serialises them -- each MFMA then waits for its own L2
    // round trip (50 us at l = 138)
    cf64x4 rt[2][NB];
    auto load_row = [&](int I, cf64x4(&dst)[NB]) {
        const double* rrow = RT + (int64_t)(16 * I + lk) * ldt + li;   // row 16 I + lk (+ 4 r), column (16 J +) li
#pragma unroll
        for (int J = 0; J < NB; ++J)
            if (J >= I) {
#pragma unroll
                for (int r = 0; r < 4; ++r) dst[J][r] = rrow[(int64_t)4 * r * ldt + 16 * J];
            }
    };
    load_row(0, rt[0]);
#pragma unroll
    for (int I = 0; I < NB; ++I) {
        if (I + 1 < NB) load_row(I + 1, rt[(I + 1) & 1]);
        const cf64x4(&cur)[NB] = rt[I & 1];
        cf64x4 pt = cf64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int r = 0; r < 4; ++r) pt = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[I][r], X[I][r], pt, 0, 0, 0);
#pragma unroll
        for (int J = I + 1; J < NB; ++J) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                X[J] = __builtin_amdgcn_mfma_f64_16x16x4f64(-cur[J][r], pt[r], X[J], 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) sP[li * ldsp + 16 * I + lk + 4 * r] = pt[r];
        __builtin_amdgcn_sched_barrier(0);   // (keeps the loads of row I + 2 from being hoisted above this row's products)
    }
    __syncthreads();
    if (P_out && !P2)
        for (int e = lane; e < 16 * M; e += 64) {
            const int r = e / M, c = e - r * M;
            P_out[(i0 + r) * ldpo + c] = sP[r * ldsp + c];
        }
    if (pk3) {
        for (int idx = lane; idx < 2 * M; idx += 64) {   // item = 8 rows (group g) of column col
            const int g = idx / M, col = idx - g * M;
            bf16x8 h, m, l;
            if (P2) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    double hd, md;
                    two_plane_f64(sP[(8 * g + e) * ldsp + col], hd, md);
                    h[e] = (__bf16)(float)hd;
                    m[e] = (__bf16)(float)md;
                    if (P_out) P_out[(i0 + 8 * g + e) * ldpo + col] = hd + md;
                }
            } else {
                f32x8 x;
#pragma unroll
                for (int e = 0; e < 8; ++e) x[e] = (float)sP[(8 * g + e) * ldsp + col];
                split3(x, h, m, l);
            }
            const int64_t c = i0 >> 5, tile = c * NTtot + (col >> 4);
            const int ln = (col & 15) + 16 * (int)(((i0 & 31) + 8 * g) >> 3);
            pk3[(tile * 3 + 0) * 64 + ln] = h;
            pk3[(tile * 3 + 1) * 64 + ln] = m;
            if (!P2) pk3[(tile * 3 + 2) * 64 + ln] = l;
            if ((K & 31) == 16 && i0 + 16 == K) {   // half-empty last chunk: zero operand groups for the rows that do not exist
                bf16x8 z; for (int e = 0; e < 8; ++e) z[e] = (__bf16)0.0f;
#pragma unroll
                for (int pl = 0; pl < (P2 ? 2 : 3); ++pl) pk3[(tile * 3 + pl) * 64 + ln + 32] = z;
            }
        }
    }
}

// X = R^-1 . B for an upper-triangular R in RT form (round 6: the final stage's U = Z (R^-1 Uh) without the explicit inverse -- with it
// the last factorisation of a fit can be k_chol_rt4's): blocked BACK substitution X_I = T_II (B_I - sum_{K > I} R_IK X_K), one wave per
// 16 COLUMNS of B (columns are independent), X_K in the accumulator layout (register r of lane (g, c): row g + 4 r, column c) -- the
// B operand of the products that use it; the A operands R_IK / T_II come from L2 with transposed addressing (A[i][k'] = block[i][g + 4 r]).
// Epilogue as k_trsm_pack's: X (fp64) and the three bf16 operand planes of the product that follows (k_pack_p3's layout), through
// one LDS transpose.  M (the order of R) = 16 NB <= 144 is also the row count of B; rows of the planes beyond M are zeros.
template <int NB>
__global__ __launch_bounds__(64) void k_trsm_left_pack(const double* __restrict__ RT, int64_t ldt, const double* __restrict__ B, int64_t ldb,
                                                       double* __restrict__ X_out, int64_t ldxo, bf16x8* __restrict__ pk3, int NTtot) {
    constexpr int M = 16 * NB, MP = (M + 31) / 32 * 32;
    __shared__ double sX[MP * 17];
    const int lane = threadIdx.x, li = lane & 15, lk = lane >> 4;
    const int64_t j0 = (int64_t)blockIdx.x * 16;
    cf64x4 X[NB];
#pragma unroll
    for (int I = 0; I < NB; ++I)
#pragma unroll
        for (int r = 0; r < 4; ++r) X[I][r] = B[(int64_t)(16 * I + lk + 4 * r) * ldb + j0 + li];
    // block row I of RT (its blocks K >= I), transposed addressing, two register sets (as k_trsm_pack: the next row is requested while
    // this one is used)
    cf64x4 rt[2][NB];
    auto load_row = [&](int I, cf64x4(&dst)[NB]) {
        const double* rrow = RT + (int64_t)(16 * I + li) * ldt + lk;
#pragma unroll
        for (int K = 0; K < NB; ++K)
            if (K >= I) {
#pragma unroll
                for (int r = 0; r < 4; ++r) dst[K][r] = rrow[16 * K + 4 * r];
            }
    };
    load_row(NB - 1, rt[(NB - 1) & 1]);
#pragma unroll
    for (int I = NB - 1; I >= 0; --I) {
        if (I > 0) load_row(I - 1, rt[(I - 1) & 1]);
        const cf64x4(&cur)[NB] = rt[I & 1];
        cf64x4 acc = X[I];
#pragma unroll
        for (int K = I + 1; K < NB; ++K) {
#pragma unroll
            for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-cur[K][r], X[K][r], acc, 0, 0, 0);
        }
        cf64x4 xi = cf64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int r = 0; r < 4; ++r) xi = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[I][r], acc[r], xi, 0, 0, 0);
        X[I] = xi;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            sX[(16 * I + lk + 4 * r) * 17 + li] = xi[r];
            if (X_out) X_out[(int64_t)(16 * I + lk + 4 * r) * ldxo + j0 + li] = xi[r];
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if (MP > M)
        for (int e = lane; e < (MP - M) * 17; e += 64) sX[M * 17 + e] = 0.0;
    __syncthreads();
    if (pk3) {
#pragma unroll
        for (int cc = 0; cc < MP / 32; ++cc) {                    // item = 8 rows (group lk of the 32-row chunk) of column li
            f32x8 x;
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = (float)sX[(32 * cc + 8 * lk + e) * 17 + li];
            bf16x8 h, m, l;
            split3(x, h, m, l);
            const int64_t tile = (int64_t)cc * NTtot + blockIdx.x;
            pk3[(tile * 3 + 0) * 64 + lane] = h;
            pk3[(tile * 3 + 1) * 64 + lane] = m;
            pk3[(tile * 3 + 2) * 64 + lane] = l;
        }
    }
}

constexpr int CHOL_THREADS = 512;
// ---- fast Cholesky-inverse for L <= 140: R and T both packed COLUMN-major in LDS (cp(k, c) = c (c + 1) / 2 + k, k <= c),
// so every inner product below walks contiguous words with incremental addresses (no index arithmetic in the loops);
// the 16 x 16 diagonal block is factored AND inverted in the registers of one wave (column c in lane c, pivots and
// multipliers broadcast with v_readlane, reciprocal square roots instead of sqrt + divisions), and the panel solve
// becomes a product with the inverted diagonal block.  Same contract as k_chol_inv.
__device__ __forceinline__ double readlane_d(double x, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), l), hi = __builtin_amdgcn_readlane(__double2hiint(x), l);
    return __hiloint2double(hi, lo);
}
// 1 / sqrt(d) for a positive, normal d: the hardware estimate (v_rsq_f64) and two Newton steps y <- y + (y / 2)(1 - d y^2) -- ~10
// dependent instructions where the library routine's range handling makes it several times that, and it sits on the
// critical path of every Cholesky pivot
__device__ __forceinline__ double fast_rsqrt_pos(double d) {
    double y = __builtin_amdgcn_rsq(d);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const double e = fma(-d * y, y, 1.0);
        y = fma(0.5 * y, e, y);
    }
    return y;
}
__device__ __forceinline__ double bperm_d(double x, int src_lane) {   // x of lane src_lane (per-lane index), through the LDS crossbar
    const int lo = __builtin_amdgcn_ds_bpermute(src_lane << 2, __double2loint(x)), hi = __builtin_amdgcn_ds_bpermute(src_lane << 2, __double2hiint(x));
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ int cp(int k, int c) { return (c * (c + 1)) / 2 + k; }
typedef double cf64x4 __attribute__((ext_vector_type(4)));
// element (r, c) of an upper-triangular matrix kept column-packed; zero below the diagonal and outside the L x L matrix
__device__ __forceinline__ double ld_up(const double* P, int r, int c, int L) { return (r <= c && c < L) ? P[cp(r, c)] : 0.0; }
constexpr int CHOL2_MAXL = 140;
__host__ __device__ inline size_t chol2_lds_bytes(int L) {
    return sizeof(double) * ((size_t)L * (L + 1) + 2 * (size_t)L) + sizeof(int) * (size_t)L;
}
// gd_ref (nullable): the diagonal the pivots are compared with (rel_tol * gd_ref[j]) when G is a Schur complement of a
// larger matrix (blocked factorisation of L > 200: the dependence test stays relative to the ORIGINAL diagonal)
// The factorisation proper, on a column-packed upper triangle that is already in LDS (Rc filled, Tc zeroed, gd = the reference
// diagonal).  Collective over the workgroup; starts with a barrier.  (Split from its loader in round 4 for a kernel that fed it
// from in-launch partial sums -- measured slower than the separate launches, EXPERIMENTS.md -- and kept as the cleaner shape.)
__device__ __forceinline__ void chol2_body(double* sm_chol, int L, double* __restrict__ T, int64_t ldt, double rel_tol,
                                           int* __restrict__ ndead_out, int Lz, int rt_form, int ncount) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int np = L * (L + 1) / 2;
    double* Rc = sm_chol;
    double* Tc = Rc + np;
    double* gd = Tc + np;
    double* rinv = gd + L;
    int* dead = reinterpret_cast<int*>(rinv + L);
    for (int e = tid; e < Lz * Lz; e += nt) {  // zero padding of the output beyond the factored block
        const int r = e / Lz, c = e - r * Lz;
        if (r >= L || c >= L) T[(int64_t)r * ldt + c] = 0.0;
    }
    __syncthreads();
#ifdef PETAL_DEBUG_COUNTERS
    long long _t0 = clock64();
#endif
    const int nb = (L + 15) / 16;
    for (int J = 0; J < nb; ++J) {
        const int jb = 16 * J;
        // (the reference diagonal of this block's pivots, requested before the update phase so that its LDS latency is not paid
        // in the factoring wave's chain; broadcast reads, only wave 0 uses them)
        double gdv[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) gdv[i] = (tid < 64 && jb + i < L) ? gd[jb + i] : 0.0;
        // (1) block row J -= (finished rows above)^T (finished rows above), one 16 x 16 tile per wave pass on the fp64 matrix
        //     cores: C(J, Ct) -= sum_K R_KJ^T R_K,Ct.  MFMA 16x16x4 f64: lane l feeds A[l & 15][l >> 4], B[l >> 4][l & 15];
        //     register r of lane l is C[(l >> 4) + 4 r][l & 15].
        // The diagonal tile (Ct = J, always wave 0's first) does not go back to LDS: the accumulator layout -- register r of lane
        // (lk, li) = row lk + 4 r, column li -- IS the layout the factorisation below holds its block in, so wave 0 subtracts it
        // from the old block in registers and factors straight on while the other waves finish their tiles (no tile of theirs
        // is read by the factorisation, and none of them reads the diagonal tile): one barrier per block row instead of two.
        cf64x4 dacc = cf64x4{0.0, 0.0, 0.0, 0.0};
        if (jb > 0) {
            const int lane = tid & 63, li = lane & 15, lk = lane >> 4;
            for (int Ct = J + (tid >> 6); Ct < nb; Ct += nt >> 6) {
                cf64x4 acc = cf64x4{0.0, 0.0, 0.0, 0.0};
                // (jb is a multiple of 16: the operands of a whole 16-row block are requested before its four MFMAs, so the
                // LDS latency is paid once per block instead of once per k-step)
                for (int k0 = 0; k0 < jb; k0 += 16) {
                    double pa[4], pb[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {  // rows k0 + 4 u + lk of R: (R_KJ^T)[i][k] = R[k][jb + i]
                        pa[u] = ld_up(Rc, k0 + 4 * u + lk, jb + li, L);
                        pb[u] = ld_up(Rc, k0 + 4 * u + lk, 16 * Ct + li, L);
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[u], pb[u], acc, 0, 0, 0);
                }
                if (Ct == J) { dacc = acc; continue; }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rr = jb + lk + 4 * r, cc = 16 * Ct + li;
                    if (rr <= cc && cc < L) Rc[cp(rr, cc)] -= acc[r];
                }
            }
        }
        DBG_T(8);
        // (2) diagonal block in the registers of wave 0, right-looking.  Lane (g, c) = (lane >> 4, lane & 15) holds the four rows
        //     g, g + 4, g + 8, g + 12 of column jb + c of the (symmetric) Schur complement, so a pivot step needs FIVE values from
        //     other lanes -- the scaled pivot row at its own column and at its four rows -- through the LDS crossbar
        //     (ds_bpermute: no SGPR round trip), where the one-column-per-lane form needed 15 - i multipliers by v_readlane pairs
        //     (~460 cycles per pivot, 40 % of this kernel).  Same operations on the same operands in the same order: the upper
        //     triangle comes out bit-identical.  Reciprocal square roots instead of sqrt + divisions.
        if (tid < 64) {
            const int c = tid & 15, g = tid >> 4, col = jb + c;
            double a[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int k = g + 4 * m, row = jb + k;
                a[m] = (col < L && row < L) ? (k <= c ? Rc[cp(row, col)] : Rc[cp(col, row)]) - dacc[m] : 0.0;
            }
            double myinv = 0.0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int gi = i & 3, mi = i >> 2;
                const double dii = readlane_d(a[mi], gi * 16 + i);
                const bool ok = (gdv[i] > 0.0) && (dii > rel_tol * gdv[i]);
                // the UNSCALED pivot row travels while the reciprocal square root is being computed (the exchange is off the
                // critical path) and is scaled where it arrives: the same products as scaling at the source, bit for bit
                const double su_c = bperm_d(a[mi], gi * 16 + c);  // S[i][my column]
                double su_k[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) su_k[m] = (4 * m + 3 > i) ? bperm_d(a[mi], gi * 16 + g + 4 * m) : 0.0;   // S[i][my row k]
                const double rs = fast_rsqrt_pos(ok ? dii : 1.0);
                const double inv = ok ? rs : 0.0;                 // (a select, not a branch: 40 cycles per pivot)
                const double r_own = a[mi] * inv;                 // row i of R, in the lanes that hold it (g == gi)
                const double rc = su_c * inv;                     // R[i][my column]
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int k = g + 4 * m;
                    const double rk = su_k[m] * inv;              // R[i][my row k]
                    if (m == mi) a[m] = (g == gi) ? r_own : (k > i ? a[m] - rk * rc : a[m]);
                    else if (4 * m + 3 > i) a[m] = (k > i) ? a[m] - rk * rc : a[m];
                }
                myinv = (tid == i) ? inv : myinv;                 // (kept in lane i: LDS writes inside the chain cost as much again)
            }
            if (tid < 16 && col < L) { rinv[col] = myinv; dead[col] = myinv > 0.0 ? 0 : 1; }
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int k = g + 4 * m;
                if (k <= c && col < L) Rc[cp(jb + k, col)] = a[m];
            }
        }
        __syncthreads();
        DBG_T(9);
        // (3) panel right of the block by forward substitution, one thread per column (right-looking in registers; the
        //     multipliers R[jb + k][jb + i] are broadcast LDS reads, independent of the dependency chain)
        if (jb + 16 < L) {
            const int c = jb + 16 + tid;
            if (c < L) {
                double v[16];
                double* pc = Rc + (c * (c + 1)) / 2 + jb;
#pragma unroll
                for (int k = 0; k < 16; ++k) v[k] = pc[k];
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    v[k] *= rinv[jb + k];
#pragma unroll
                    for (int i = k + 1; i < 16; ++i) v[i] -= Rc[cp(jb + k, jb + i)] * v[k];
                }
#pragma unroll
                for (int k = 0; k < 16; ++k) pc[k] = v[k];
            }
            __syncthreads();
        }
        DBG_T(10);
    }
    // inverses of all diagonal blocks at once, one wave per block: column c of T_JJ in lane c, back substitution
    // right-looking (column k of R updates every partial sum: independent FMAs), multipliers as broadcast LDS reads
    for (int J = tid >> 6; J < nb; J += nt >> 6) {
        const int jb = 16 * J, ln = tid & 63, c = jb + ln;
        const int kcl = min(jb + 15, L - 1);
        double t[16], acc[16], rv[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) { acc[i] = 0.0; rv[i] = rinv[min(jb + i, kcl)] * ((jb + i <= kcl) ? 1.0 : 0.0); }
#pragma unroll
        for (int k = 15; k >= 0; --k) {
            t[k] = (k == ln) ? rv[k] : (k < ln ? -rv[k] * acc[k] : 0.0);
            const double* pk_ = Rc + cp(jb, min(jb + k, kcl));  // R[jb + i][jb + k], contiguous in i
#pragma unroll
            for (int i = 0; i < k; ++i) acc[i] += pk_[i] * t[k];
        }
        if (ln < 16 && c < L) {
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (i <= ln) Tc[cp(jb + i, c)] = t[i];
        }
    }
    __syncthreads();
    DBG_T(11);
    if (tid < 64 && ndead_out) {   // (wave 0 counts: a serial loop over L LDS reads by one thread was 2 us)
        int cdead = 0;
        for (int j = tid; j < min(L, ncount); j += 64) cdead += dead[j];   // (ncount: only the columns whose loss the caller minds)
        for (int off = 32; off > 0; off >>= 1) cdead += __shfl_down(cdead, off, 64);
        if (tid == 0 && cdead > *ndead_out) *ndead_out = cdead;
    }
    if (rt_form) {
        // "RT form": the caller applies R^-1 by a blocked triangular solve (k_trsm_pack) and only needs the inverses of the
        // diagonal blocks -- the explicit off-diagonal inverse below (30 % of this kernel) is skipped.  Output: diagonal 16 x 16
        // blocks = T_JJ = R_JJ^-1, blocks above them = R itself, zeros below.
        for (int e = tid; e < L * L; e += nt) {
            const int r = e / L, c = e - r * L;
            T[(int64_t)r * ldt + c] = c >= r ? (((r >> 4) == (c >> 4)) ? Tc[cp(r, c)] : Rc[cp(r, c)]) : 0.0;
        }
        return;
    }
    // ---- off-diagonal blocks of T = R^-1: T_IJ = -T_II sum_{K = I+1 .. J} R_IK T_KJ, as 16 x 16 block products on the fp64
    //      matrix cores.  First R~_IK = T_II R_IK for every off-diagonal block (in place: a block is read and written by
    //      one wave only), then block super-diagonal by block super-diagonal T_IJ = -sum_K R~_IK T_KJ.
    {
        const int lane = tid & 63, li = lane & 15, lk = lane >> 4, wv = tid >> 6, nw = nt >> 6;
        for (int blk = wv; blk < nb * (nb - 1) / 2; blk += nw) {
            int bI = blk, dl = 1;
            while (bI >= nb - dl) { bI -= nb - dl; ++dl; }
            const int bK = bI + dl;
            cf64x4 acc = cf64x4{0.0, 0.0, 0.0, 0.0};
            {
                double pa[4], pb[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {  // A = T_II (upper triangular), B = R_IK
                    pa[u] = ld_up(Tc, 16 * bI + li, 16 * bI + 4 * u + lk, L);
                    pb[u] = ld_up(Rc, 16 * bI + 4 * u + lk, 16 * bK + li, L);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[u], pb[u], acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int rr = 16 * bI + lk + 4 * r, cc = 16 * bK + li;
                if (cc < L) Rc[cp(rr, cc)] = acc[r];
            }
        }
        __syncthreads();
        DBG_T(12);
        for (int dl = 1; dl < nb; ++dl) {
            for (int bI = wv; bI < nb - dl; bI += nw) {
                const int bJ = bI + dl;
                cf64x4 acc = cf64x4{0.0, 0.0, 0.0, 0.0};
                for (int bK = bI + 1; bK <= bJ; ++bK) {
                    double pa[4], pb[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {  // A = R~_IK, B = T_KJ (upper triangular when K == J)
                        pa[u] = ld_up(Rc, 16 * bI + li, 16 * bK + 4 * u + lk, L);
                        pb[u] = ld_up(Tc, 16 * bK + 4 * u + lk, 16 * bJ + li, L);
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[u], pb[u], acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int rr = 16 * bI + lk + 4 * r, cc = 16 * bJ + li;
                    if (cc < L) Tc[cp(rr, cc)] = -acc[r];
                }
            }
            __syncthreads();
        }
    }
    DBG_T(13);
    for (int e = tid; e < L * L; e += nt) {
        const int r = e / L, c = e - r * L;
        T[(int64_t)r * ldt + c] = c >= r ? Tc[cp(r, c)] : 0.0;
    }
}

__global__ __launch_bounds__(CHOL_THREADS) void k_chol_inv2(const double* __restrict__ G, int L, int64_t ldg, double* __restrict__ T,
                                                            int64_t ldt, double rel_tol, int* __restrict__ ndead_out, int Lz,
                                                            const double* __restrict__ gd_ref, int rt_form, int ncount) {
    extern __shared__ __attribute__((aligned(16))) double sm_chol[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int np = L * (L + 1) / 2;
    double* Rc = sm_chol;
    double* Tc = Rc + np;
    double* gd = Tc + np;
    // (loads in batches of four: a runtime-trip loop of load -> LDS-store pairs pays an L2 round trip per pair, eleven in a row
    // at l = 74)
    for (int e0 = tid; e0 < L * L; e0 += 4 * nt) {
        double gv[4];
        int rr[4], cc[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + u * nt;
            rr[u] = e / L; cc[u] = e - rr[u] * L;
            gv[u] = (e < L * L && cc[u] >= rr[u]) ? G[(int64_t)rr[u] * ldg + cc[u]] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (e0 + u * nt < L * L && cc[u] >= rr[u]) {
                Rc[cp(rr[u], cc[u])] = gv[u];
                Tc[cp(rr[u], cc[u])] = 0.0;
                if (cc[u] == rr[u]) gd[rr[u]] = gd_ref ? gd_ref[rr[u]] : gv[u];
            }
        }
    }
    chol2_body(sm_chol, L, T, ldt, rel_tol, ndead_out, Lz, rt_form, ncount);
}

// ---- k_chol_rt4<NB>: the re-basing Cholesky of the power iterations, register-resident on four waves (round 6) ----------------
// G = R^T R for an order L <= 16 NB, "RT form" output (diagonal 16 x 16 blocks: T_JJ = R_JJ^-1, blocks above them: R, zeros below:
// what k_trsm_pack reads).  k_chol_inv2 keeps the matrix in LDS and spends a third of its 28 us at l = 74 in barriers and LDS round
// trips between its phases.  Here block (I, J), I <= J, of the working matrix lives in REGISTERS in the accumulator layout of
// v_mfma_f64_16x16x4_f64 -- register m of lane (g, c) = (lane >> 4, lane & 15) is element (g + 4 m, c) of the block -- which is at once
//   * the layout the 16 x 16 diagonal factorisation wants: four rows of a column per lane; the multiplier of row k, S[k][i], sits in
//     column i of the symmetric block, i.e. in lane i of the 16-lane row that holds row k -- a DPP row broadcast (row_newbcast, the
//     one DPP control 64-bit operands have), where k_chol_inv2 sends five values per pivot through the LDS crossbar;
//   * the B operand of an MFMA for the block itself and the A operand for its TRANSPOSE, k-slots declared as k' = (l >> 4) + 4 r,
// so the panel R_JK = T_JJ^T S_JK and the trailing update S_KM -= R_JK^T R_JM take the registers as they are; T_JJ^T is what the
// elimination of [S_JJ | I] leaves, one 2-KB LDS transpose turns it into T_JJ.  Blocks not yet factored are kept NEGATED (N = -S):
// the trailing update is a plain accumulation.  One Newton step on v_rsq_f64 (1.5 ulp): the factor only has to keep the re-based
// iterate well conditioned (backward error 6e-16 either way, dev/chol1w.hip).
// A wave cannot overlap its own MFMAs with its own VALU work (a ONE-wave form of this kernel, dev/chol1w_kernel.h: 12.0 us over an
// empty kernel at l = 74, 41.7 at l = 138, and 78 in the fit, where its 75 KB of straight-line code arrive cold; interleaving the
// MFMAs between the pivots gains nothing), so the three other matrix pipes of the CU take the panel and the trailing update while
// wave 0 runs nothing but the pivot chain (280 cycles a pivot: readlane -> rsq -> Newton -> scale -> update, ~35 instructions):
//   wave 0   factors the diagonal block D_J, publishes -T_JJ, forms R_J,J+1 and N_J+1,J+1 += R_J,J+1^T R_J,J+1 from the two blocks
//            the owner of column J + 1 handed over, goes on;
//   wave h   (1..3) owns whole block COLUMNS M >= 2: after -T_JJ is out it forms its panel blocks R_JM, publishes them, and after every
//            panel is out updates its blocks N_KM += R_JK^T R_JM.
// Two workgroup barriers per block row; what crosses them goes through LDS in register order (lane-contiguous 8-byte words: no bank
// conflicts, no layout change).  Measured (dev/chol1w.hip, over an empty kernel): 9.5 us at l = 74 (k_chol_inv2: 25), 21.4 us at
// l = 138 (72).
// compile-time loops: every block index is a constant expression, so the blocks are registers (a #pragma unroll the optimizer gives
// up on turns the whole array into scratch memory)
template <int I0, int I1, class F>
__device__ __forceinline__ void chol_static_for(F&& f) {
    if constexpr (I0 < I1) {
        f(std::integral_constant<int, I0>{});
        chol_static_for<I0 + 1, I1>(f);
    }
}
template <int NB>
__device__ __forceinline__ constexpr int chol4_owner(int M) {   // columns dealt out from the last (longest) one, boustrophedon over the 3 helpers
    const int idx = NB - 1 - M, round = idx / 3, pos = idx % 3;
    return (round & 1) ? 3 - pos : 1 + pos;
}
// (not __syncthreads(): that also waits for the global stores of the factor -- vmcnt -- a microsecond per barrier; only LDS crosses here)
__device__ __forceinline__ void chol4_sync() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ __forceinline__ void chol4_put(double* slot, const cf64x4& v, int lane) {
#pragma unroll
    for (int r = 0; r < 4; ++r) slot[r * 64 + lane] = v[r];
}
__device__ __forceinline__ cf64x4 chol4_get(const double* slot, int lane) {
    cf64x4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = slot[r * 64 + lane];
    return v;
}
// block (I, J) of G, negated, upper triangle only, zero beyond L (clamped addresses + select: no exec-mask branches)
__device__ __forceinline__ cf64x4 chol4_load(const double* __restrict__ G, int L, int64_t ldg, int I, int J, int g, int c) {
    cf64x4 v;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int row = 16 * I + g + 4 * m, col = 16 * J + c;
        const int rr = (I == J && row > col) ? col : row, cc = (I == J && row > col) ? row : col;
        const double x = G[(int64_t)min(rr, L - 1) * ldg + min(cc, L - 1)];
        v[m] = (row < L && col < L) ? -x : 0.0;
    }
    return v;
}
__device__ __forceinline__ void chol4_store(double* __restrict__ T, int64_t ldt, int I, int J, int g, int c, const cf64x4& v) {
#pragma unroll
    for (int m = 0; m < 4; ++m) T[(int64_t)(16 * I + g + 4 * m) * ldt + 16 * J + c] = v[m];
}
#define CHOL4_MFMA(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

// helper wave H: all of its work, unrolled over the block rows (its blocks are registers)
template <int NB, int H>
__device__ __forceinline__ void chol4_helper(const double* __restrict__ G, int L, int64_t ldg, double* __restrict__ T, int64_t ldt,
                                             double* s_tjj, double* s_hand, double* s_panel, int lane) {
    const int c = lane & 15, g = lane >> 4;
    // S[M][K]: block (K, M) of an owned column M (K <= M); columns that are not mine stay unused (and cost nothing)
    cf64x4 S[NB][NB];
    chol_static_for<2, NB>([&](auto Mc) {
        constexpr int M = decltype(Mc)::value;
        if constexpr (chol4_owner<NB>(M) == H)
            chol_static_for<0, M + 1>([&](auto Kc) { constexpr int K = decltype(Kc)::value; S[M][K] = chol4_load(G, L, ldg, K, M, g, c); });
    });
    // zeros below the block diagonal of the output: rows I = H, H + 3, ...
    chol_static_for<1, NB>([&](auto Ic) {
        constexpr int I = decltype(Ic)::value;
        if constexpr (I % 3 == H % 3)
            chol_static_for<0, I>([&](auto Jc) { chol4_store(T, ldt, I, decltype(Jc)::value, g, c, cf64x4{0.0, 0.0, 0.0, 0.0}); });
    });
    chol_static_for<0, NB>([&](auto Jc) {
        constexpr int J = decltype(Jc)::value;
        // hand column J + 1's two leading blocks to wave 0 (complete through block row J - 1; column 1 is wave 0's own)
        if constexpr (J >= 1 && J + 1 < NB) {
            if constexpr (chol4_owner<NB>(J + 1) == H) {
                chol4_put(s_hand, S[J + 1][J], lane);
                chol4_put(s_hand + 256, S[J + 1][J + 1], lane);
            }
        }
        chol4_sync();   // barrier 1: -T_JJ is out
        if constexpr (J + 2 < NB) {
            const cf64x4 negA = chol4_get(s_tjj, lane);
            chol_static_for<J + 2, NB>([&](auto Mc) {
                constexpr int M = decltype(Mc)::value;
                if constexpr (chol4_owner<NB>(M) == H) {
                    cf64x4 acc = cf64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc = CHOL4_MFMA(negA[r], S[M][J][r], acc);
                    S[M][J] = acc;   // R_JM
                    chol4_put(s_panel + ((J & 1) * NB + M) * 256, acc, lane);
                    chol4_store(T, ldt, J, M, g, c, acc);
                }
            });
        }
        chol4_sync();   // barrier 2: every panel block of row J is out
        if constexpr (J + 2 < NB) {
            // N_KM += R_JK^T R_JM for my columns M >= J + 2, K = J + 1 .. M; R_JK read once per K
            chol_static_for<J + 1, NB>([&](auto Kc) {
                constexpr int K = decltype(Kc)::value;
                constexpr bool any = [] { for (int M = (K > J + 2 ? K : J + 2); M < NB; ++M) if (chol4_owner<NB>(M) == H) return true; return false; }();
                if constexpr (any) {
                    const cf64x4 rk = chol4_get(s_panel + ((J & 1) * NB + K) * 256, lane);
                    chol_static_for<(K > J + 2 ? K : J + 2), NB>([&](auto Mc) {
                        constexpr int M = decltype(Mc)::value;
                        if constexpr (chol4_owner<NB>(M) == H) {
#pragma unroll
                            for (int r = 0; r < 4; ++r) S[M][K] = CHOL4_MFMA(rk[r], S[M][J][r], S[M][K]);
                        }
                    });
                }
            });
        }
    });
}

template <int NB>
__global__ __launch_bounds__(256) void k_chol_rt4(const double* __restrict__ G, int L, int64_t ldg, double* __restrict__ T, int64_t ldt,
                                                  double rel_tol, int* __restrict__ ndead_out, int ncount) {
    __shared__ double s_tr[16 * 17];            // wave 0's transpose scratch
    __shared__ double s_tjj[256];               // -T_JJ in register order
    __shared__ double s_hand[512];              // the two blocks handed to wave 0
    __shared__ double s_panel[2 * NB * 256];    // R_JM of block row J, double buffered
    __shared__ double s_thr[16 * NB];           // the acceptance threshold of every pivot: rel_tol x the original diagonal
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (wave == 1) { chol4_helper<NB, 1>(G, L, ldg, T, ldt, s_tjj, s_hand, s_panel, lane); return; }
    if (wave == 2) { chol4_helper<NB, 2>(G, L, ldg, T, ldt, s_tjj, s_hand, s_panel, lane); return; }
    if (wave == 3) { chol4_helper<NB, 3>(G, L, ldg, T, ldt, s_tjj, s_hand, s_panel, lane); return; }
    const int c = lane & 15, g = lane >> 4;
    cf64x4 D = -chol4_load(G, L, ldg, 0, 0, g, c);
    cf64x4 Off = cf64x4{0.0, 0.0, 0.0, 0.0}, Next = cf64x4{0.0, 0.0, 0.0, 0.0};
    if (NB > 1) { Off = chol4_load(G, L, ldg, 0, 1, g, c); Next = chol4_load(G, L, ldg, 1, 1, g, c); }
    int cdead = 0;
    const int nlim = min(L, ncount);
    for (int e = lane; e < 16 * NB; e += 64) {
        const double gdj = G[(int64_t)min(e, L - 1) * (ldg + 1)];
        s_thr[e] = (e < L && gdj > 0.0) ? rel_tol * gdj : __builtin_inf();
    }
    for (int J = 0; J < NB; ++J) {
        const int jb = 16 * J;
        const double thr = s_thr[jb + c];       // (wave 0's own writes: LDS operations of a wave stay in order)
        cf64x4 Id;
#pragma unroll
        for (int m = 0; m < 4; ++m) Id[m] = (g + 4 * m == c) ? 1.0 : 0.0;
        chol_static_for<0, 16>([&](auto ic) {
            constexpr int i = decltype(ic)::value, mi = i >> 2, gi = i & 3, src = 16 * gi;
            const double dii = readlane_d(D[mi], src + i);
            const double thi = readlane_d(thr, i);
            const bool ok = dii > thi;
            const double su_c = bperm_d(D[mi], src + c), su_ci = bperm_d(Id[mi], src + c);
            double y = __builtin_amdgcn_rsq(dii);
            const double en = fma(-dii * y, y, 1.0);
            y = fma(0.5 * y, en, y);
            const double inv = ok ? y : 0.0;
            const double ninv2 = -(inv * inv);
            const double w = su_c * ninv2, wi = su_ci * ninv2;
            {
                double bk = __builtin_amdgcn_update_dpp(0.0, D[mi], 0x150 + i, 0xf, 0xf, false);
                bk = (g > gi) ? bk : 0.0;
                const double v = (g == gi) ? inv : 1.0;
                Id[mi] = fma(bk, wi, Id[mi] * v);
                D[mi] = fma(bk, w, D[mi] * v);
            }
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                if (m <= mi) continue;
                const double bk = __builtin_amdgcn_update_dpp(0.0, D[m], 0x150 + i, 0xf, 0xf, false);
                Id[m] = fma(bk, wi, Id[m]);
                D[m] = fma(bk, w, D[m]);
            }
            __builtin_amdgcn_sched_barrier(0);
        });
#pragma unroll
        for (int m = 0; m < 4; ++m) s_tr[(g + 4 * m) * 17 + c] = Id[m];
        cf64x4 A;
#pragma unroll
        for (int r = 0; r < 4; ++r) A[r] = s_tr[c * 17 + g + 4 * r];
        const cf64x4 negA = -A;
        chol4_put(s_tjj, negA, lane);
        {
            bool dead = false;
#pragma unroll
            for (int r = 0; r < 4; ++r) dead = dead || (g + 4 * r == c && jb + c < nlim && !(A[r] > 0.0));
            cdead += __builtin_popcountll(__ballot(dead));
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) T[(int64_t)(jb + g + 4 * r) * ldt + jb + c] = A[r];
        chol4_sync();   // barrier 1
        cf64x4 R = cf64x4{0.0, 0.0, 0.0, 0.0};
        if (J + 1 < NB) {
            if (J > 0) { Off = chol4_get(s_hand, lane); Next = chol4_get(s_hand + 256, lane); }
#pragma unroll
            for (int r = 0; r < 4; ++r) R = CHOL4_MFMA(negA[r], Off[r], R);
            chol4_put(s_panel + ((J & 1) * NB + J + 1) * 256, R, lane);
#pragma unroll
            for (int m = 0; m < 4; ++m) T[(int64_t)(jb + g + 4 * m) * ldt + jb + 16 + c] = R[m];
        }
        chol4_sync();   // barrier 2
        if (J + 1 < NB) {
#pragma unroll
            for (int r = 0; r < 4; ++r) Next = CHOL4_MFMA(R[r], R[r], Next);
            D = -Next;
        }
    }
    if (lane == 0 && ndead_out && cdead > *ndead_out) *ndead_out = cdead;
}
#undef CHOL4_MFMA

// ---- convergence of a Jacobi sweep, graded matrices included ------------------------------------------------------------
// Every matrix these solvers see is a Gram matrix (PSD, often with eigenvalues spread over many decades: B B^T of the
// randomized SVD, the covariance of exact Pca / FastICA whitening).  A stopping rule on ||off||_F / ||diag||_F, the
// usual one, declares such a matrix finished while the rows of its SMALL eigenvalues are still coupled -- at
// off = 1e-15 ||diag|| an eigenvalue of 1e-7 lambda_1 has lost half its digits (measured: singular values below
// 10^-3.5 sigma_1 wrong in the 5th digit).  Element (p, q) is therefore finished when
//     a_pq^2 <= tol^2 |a_pp a_qq|        (relative to ITS rows: the Demmel-Veselic criterion, which is what gives two-sided
//                                          Jacobi its high relative accuracy on positive definite matrices), or
//     a_pq^2 <= (1e-16 ||diag||_F)^2      (below the rounding noise of the matrix itself: exact zeros / rank deficiency).
// Returns the largest a_pq^2 / limit over the upper triangle: <= 1 means converged.  Reads r <= c only (the split solver keeps the upper triangle).
// The second limit alone would end the iteration on a GRADED positive definite matrix (A = D H D, entries accurate to their own
// size) while the rows of its eigenvalues below 1e-16 ||A|| are still coupled: cyclic sweeps rotate those rows along with the rest,
// so they are nearly done when the large ones finish, but the last quadratic step is missing -- measured 2.6e-12 relative
// error in the small eigenvalues of a 48 x 48 matrix graded over 24 decades, where a float64 Hestenes iteration has 1.2e-14; with the
// rule below 2.8e-15 (eig-graded-L48-jacobi in profiles/smallmat_errors.txt; tests/smallmat_cases.py, EXPERIMENTS.md).
// s_red[63] (set by the caller before the first sweep: +inf, or 0 to switch this off; in LDS because the value is uniform and the split
// solver has no register to spare) holds the first criterion's violation of the previous call: once the limits above are met, the sweeps go on while the FIRST
// criterion alone is still violated AND the last sweep reduced that violation at least fourfold -- quadratic convergence on a
// graded matrix; on rounding noise (exact zeros, rank deficiency: no progress, or a zero diagonal product) the iteration ends as before.
// Only for tol_rel <= 1e-15 (fp64 callers).  The cost: a solve whose matrix has eigenvalues at its noise level runs one more sweep
// before the no-progress exit (EXPERIMENTS.md).
// Collective over the workgroup; s_red needs 64 doubles.
__device__ double wg_jacobi_violation(const double* A, int64_t ld, int L, double tol_rel, double* s_red) {
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wv = tid >> 6, nw = (nt + 63) >> 6;
    double dg = 0;
    for (int e = tid; e < L; e += nt) { const double v = A[e * ld + e]; dg += v * v; }
    for (int off = 32; off > 0; off >>= 1) dg += __shfl_down(dg, off, 64);
    if (lane == 0) s_red[wv] = dg;
    __syncthreads();
    double tdg = 0;
    for (int x = 0; x < nw; ++x) tdg += s_red[x];
    __syncthreads();
    if (!(tdg > 0.0) || !(tdg < 1e300)) return 0.0;  // zero or non-finite matrix: nothing a rotation could improve
    const double floor2 = 1e-32 * tdg, tol2 = tol_rel * tol_rel;
    double viol = 0, vrel = 0;
    {
        int r = tid / L, c = tid - r * L;
        const int dr = nt / L, dc = nt - dr * L;
        for (int e = tid; e < L * L; e += nt) {
            if (c > r) {
                const double v = A[r * ld + c];
                if (v != 0.0) {
                    const double rel = tol2 * fabs(A[r * ld + r] * A[c * ld + c]);
                    viol = fmax(viol, v * v / fmax(rel, floor2));
                    vrel = fmax(vrel, v * v / rel);   // (+inf on a zero diagonal product)
                }
            }
            r += dr; c += dc;
            if (c >= L) { c -= L; ++r; }
        }
    }
    for (int off = 32; off > 0; off >>= 1) { viol = fmax(viol, __shfl_down(viol, off, 64)); vrel = fmax(vrel, __shfl_down(vrel, off, 64)); }
    if (lane == 0) { s_red[wv] = viol; s_red[32 + wv] = vrel; }
    __syncthreads();
    double tv = 0, tr = 0;
    for (int x = 0; x < nw; ++x) { tv = fmax(tv, s_red[x]); tr = fmax(tr, s_red[32 + x]); }
    const double prev = s_red[63];
    const bool progress = prev != 0.0 && tr < 0.25 * prev;
    __syncthreads();
    if (tid == 0 && prev != 0.0) s_red[63] = tr;   // (read again behind the barriers of the next call; a 0 stays: switched off for good)
    if (!(tv > 1.0) && tr > 1.0 && progress) return tr;
    return tv;
}

// ---- workgroup-wide cyclic Jacobi eigen-solver (fp64) ----------------------------------------------
// A (L x L, lda) symmetric, destroyed; V (L x L, ldv) <- eigenvectors in columns.  Parallel ordering:
// round-robin tournament, L/2 disjoint rotations per round, three barriers per round.
__device__ void wg_jacobi(double* A, int64_t lda, double* V, int64_t ldv, int L, double* s_c, double* s_s, int* s_p, int* s_q,
                          double* s_red, double tol_rel, bool graded = false) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int e = tid; e < L * L; e += nt) V[(int64_t)(e / L) * ldv + (e % L)] = (e / L == e % L) ? 1.0 : 0.0;
    __syncthreads();
    if (L < 2) return;
    const int Le = (L + 1) & ~1, half = Le / 2, rounds = Le - 1;
    if (tid == 0) s_red[63] = (graded && tol_rel <= 1e-15) ? INFINITY : 0.0;   // (0: the continuation of wg_jacobi_violation never starts)
    __syncthreads();
    for (int sweep = 0; sweep < 40; ++sweep) {
        const double viol = wg_jacobi_violation(A, lda, L, tol_rel, s_red);
        // (no "nearly there: one more sweep" shortcut: with clustered or tiny eigenvalues the step after |a_pq| ~ sqrt(tol) is
        // NOT at tol -- a_pq^2 / gap -- and stopping there left 3e-4 in the eigenvectors of a graded test matrix)
        if (!(viol > 1.0)) break;
        for (int rd = 0; rd < rounds; ++rd) {
            for (int k = tid; k < half; k += nt) {
                int p, q;
                if (k == 0) { p = Le - 1; q = rd; }
                else { p = (rd + k) % (Le - 1); q = (rd - k + (Le - 1)) % (Le - 1); }
                if (p > q) { const int t = p; p = q; q = t; }
                double c = 1.0, s = 0.0;
                if (q < L) {
                    const double apq = A[(int64_t)p * lda + q];
                    if (apq != 0.0) {
                        const double theta = (A[(int64_t)q * lda + q] - A[(int64_t)p * lda + p]) / (2.0 * apq);
                        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                        c = 1.0 / sqrt(t * t + 1.0);
                        s = t * c;
                    }
                } else { q = p; }  // bye
                s_p[k] = p; s_q[k] = q; s_c[k] = c; s_s[k] = s;
            }
            __syncthreads();
            for (int e = tid; e < L * half; e += nt) {  // columns: A <- A J, V <- V J
                const int r = e / half, k = e % half;
                const int p = s_p[k], q = s_q[k];
                if (p == q) continue;
                const double c = s_c[k], s = s_s[k];
                const double ap = A[(int64_t)r * lda + p], aq = A[(int64_t)r * lda + q];
                A[(int64_t)r * lda + p] = c * ap - s * aq;
                A[(int64_t)r * lda + q] = s * ap + c * aq;
                const double vp = V[(int64_t)r * ldv + p], vq = V[(int64_t)r * ldv + q];
                V[(int64_t)r * ldv + p] = c * vp - s * vq;
                V[(int64_t)r * ldv + q] = s * vp + c * vq;
            }
            __syncthreads();
            for (int e = tid; e < L * half; e += nt) {  // rows: A <- J^T A
                const int k = e / L, cc = e % L;
                const int p = s_p[k], q = s_q[k];
                if (p == q) continue;
                const double c = s_c[k], s = s_s[k];
                const double ap = A[(int64_t)p * lda + cc], aq = A[(int64_t)q * lda + cc];
                A[(int64_t)p * lda + cc] = c * ap - s * aq;
                A[(int64_t)q * lda + cc] = s * ap + c * aq;
            }
            __syncthreads();
        }
    }
}
// LDS-resident variant for L <= 16 MB: A and V are L x L with an odd leading dimension.  Two barriers per round:
//   (1) one thread per pair computes its rotation (c, s) from A[p][p], A[q][q], A[p][q];
//   (2) A <- J^T A J in ONE pass over 2 x 2 blocks -- the block at rows (p, q) of pair k and columns (p', q') of pair k'
//       is read once, rotated from both sides in registers and written back in place (no other thread touches it) --
//       and V <- V J column-wise in the same phase.
// Every thread gathers all its operands into registers first and scatters afterwards, so the LDS round trips overlap
// instead of serialising behind possibly-aliasing stores; (c, s) and (p, q) are packed for 16-B / 8-B loads.
template <int MB>
__device__ void wg_jacobi_fast(double* A, double* V, int L, double* s_c, double* s_s, int* s_p, int* s_q, double* s_red,
                               double tol_rel, bool graded = false) {
    constexpr int MB2 = (MB + 1) / 2;  // 16-wide groups of pairs: half <= 8 MB
    const int LD = L | 1;  // odd leading dimension: column accesses (stride LD doubles) spread over all LDS banks
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wv = tid >> 6, nw = nt >> 6;
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    typedef int i32x2 __attribute__((ext_vector_type(2)));
    f64x2* s_cs = reinterpret_cast<f64x2*>(s_c);  // [half] (c, s)   (s_s == s_c + half: the two arrays are contiguous)
    i32x2* s_pq = reinterpret_cast<i32x2*>(s_p);  // [half] (p, q)   (s_q == s_p + half)
    (void)s_s; (void)s_q;
    for (int e = tid; e < L * LD; e += nt) V[e] = 0.0;
    __syncthreads();
    for (int e = tid; e < L; e += nt) V[e * LD + e] = 1.0;
    __syncthreads();
    if (L < 2) return;
    const int Le = (L + 1) & ~1, half = Le / 2, rounds = Le - 1;
    if (tid == 0) s_red[63] = (graded && tol_rel <= 1e-15) ? INFINITY : 0.0;   // (0: the continuation of wg_jacobi_violation never starts)
    __syncthreads();
    for (int sweep = 0; sweep < 40; ++sweep) {
        const double viol = wg_jacobi_violation(A, LD, L, tol_rel, s_red);
#ifdef PETAL_DEBUG_COUNTERS
        if (tid == 0) g_dbg[0] = sweep;
#endif
        // (no "nearly there: one more sweep" shortcut: with clustered or tiny eigenvalues the step after |a_pq| ~ sqrt(tol) is
        // NOT at tol -- a_pq^2 / gap -- and stopping there left 3e-4 in the eigenvectors of a graded test matrix)
        if (!(viol > 1.0)) break;
        for (int rd = 0; rd < rounds; ++rd) {
#ifdef PETAL_DEBUG_COUNTERS
            long long _t0 = clock64();
#endif
            if (tid < half) {
                const int k = tid;
                int p, q;
                if (k == 0) { p = Le - 1; q = rd; }
                else { p = rd + k; if (p >= Le - 1) p -= Le - 1; q = rd - k; if (q < 0) q += Le - 1; }
                if (p > q) { const int t = p; p = q; q = t; }
                double c = 1.0, sn = 0.0;
                if (q < L) {
                    const double apq = A[p * LD + q];
                    if (apq != 0.0) {
                        const double theta = (A[q * LD + q] - A[p * LD + p]) / (2.0 * apq);
                        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                        c = 1.0 / sqrt(t * t + 1.0);
                        sn = t * c;
                    }
                } else { q = p; }  // bye: identity rotation on a single index
                s_pq[k] = i32x2{p, q};
                s_cs[k] = f64x2{c, sn};
            }
            DBG_T(0);
            __syncthreads();
            DBG_T(1);
            {   // A <- J^T A J, one 2 x 2 block per (pair k, pair k')
                const int k0 = tid & 15;
                for (int k = tid >> 4; k < half; k += nt >> 4) {
                    const i32x2 pq = s_pq[k];
                    const f64x2 cs = s_cs[k];
                    double* rp = A + pq[0] * LD;
                    double* rq = A + pq[1] * LD;
                    double a[MB2], b[MB2], cc[MB2], d[MB2], c2[MB2], s2[MB2];
                    int p2[MB2], q2[MB2];
#pragma unroll
                    for (int m = 0; m < MB2; ++m) {
                        const int kp = min(k0 + 16 * m, half - 1);
                        const i32x2 pq2 = s_pq[kp];
                        const f64x2 cs2 = s_cs[kp];
                        p2[m] = pq2[0]; q2[m] = (k0 + 16 * m < half) ? pq2[1] : -1;
                        c2[m] = cs2[0]; s2[m] = cs2[1];
                        a[m] = rp[pq2[0]]; b[m] = rp[pq2[1]]; cc[m] = rq[pq2[0]]; d[m] = rq[pq2[1]];
                    }
#pragma unroll
                    for (int m = 0; m < MB2; ++m) {
                        if (q2[m] < 0) continue;
                        // right rotation (columns p', q'), then left rotation (rows p, q)
                        const double a1 = c2[m] * a[m] - s2[m] * b[m], b1 = s2[m] * a[m] + c2[m] * b[m];
                        const double c1 = c2[m] * cc[m] - s2[m] * d[m], d1 = s2[m] * cc[m] + c2[m] * d[m];
                        rp[p2[m]] = cs[0] * a1 - cs[1] * c1;
                        rp[q2[m]] = cs[0] * b1 - cs[1] * d1;
                        rq[p2[m]] = cs[1] * a1 + cs[0] * c1;
                        rq[q2[m]] = cs[1] * b1 + cs[0] * d1;
                    }
                }
            }
            {   // V <- V J (columns)
                const int kk = tid & 7;
                for (int r = tid >> 3; r < L; r += nt >> 3) {
                    double vp[MB], vq[MB], cc[MB], sn[MB];
                    int pp[MB], qq[MB];
                    double* vr = V + r * LD;
#pragma unroll
                    for (int m = 0; m < MB; ++m) {
                        const int k = min(kk + 8 * m, half - 1);
                        const i32x2 pq = s_pq[k];
                        const f64x2 cs = s_cs[k];
                        pp[m] = pq[0];
                        qq[m] = (kk + 8 * m < half && pq[0] != pq[1]) ? pq[1] : -1;
                        cc[m] = cs[0]; sn[m] = cs[1];
                        vp[m] = vr[pq[0]]; vq[m] = vr[pq[1]];
                    }
#pragma unroll
                    for (int m = 0; m < MB; ++m) {
                        if (qq[m] >= 0) {
                            vr[pp[m]] = cc[m] * vp[m] - sn[m] * vq[m];
                            vr[qq[m]] = sn[m] * vp[m] + cc[m] * vq[m];
                        }
                    }
                }
            }
            DBG_T(2);
            __syncthreads();
            DBG_T(3);
        }
    }
}
// MB == 0: matrices in global memory (any L), generic loops; MB > 0: LDS-resident fast path for L <= 16 MB
template <int MB>
__device__ __forceinline__ void wg_jacobi_any(double* A, int64_t lda, double* V, int64_t ldv, int L, double* s_c, double* s_s,
                                              int* s_p, int* s_q, double* s_red, double tol_rel = 1e-15, bool graded = false) {
    if constexpr (MB == 0) wg_jacobi(A, lda, V, ldv, L, s_c, s_s, s_p, s_q, s_red, tol_rel, graded);
    else wg_jacobi_fast<MB>(A, V, L, s_c, s_s, s_p, s_q, s_red, tol_rel, graded);
}
// sort eigenpairs descending: Vout[:, rank] = V[:, j], w[rank] = A[j][j]
__device__ void wg_sort_eig(const double* A, int64_t lda, const double* V, int64_t ldv, int L, double* Vout, int64_t ldo,
                            double* w, int* s_rank) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int j = tid; j < L; j += nt) {
        const double wj = A[(int64_t)j * lda + j];
        int rank = 0;
        for (int k = 0; k < L; ++k) {
            const double wk = A[(int64_t)k * lda + k];
            rank += (wk > wj || (wk == wj && k < j)) ? 1 : 0;
        }
        s_rank[j] = rank;
        w[rank] = wj;
    }
    __syncthreads();
    for (int e = tid; e < L * L; e += nt) {
        const int r = e / L, j = e % L;
        Vout[(int64_t)r * ldo + s_rank[j]] = V[(int64_t)r * ldv + j];
    }
    __syncthreads();
}

constexpr int EIG_MAXL = 8192;
struct JacWs { double* c; double* s; double* red; int* p; int* q; int* rank; };
__host__ __device__ inline size_t jac_ws_doubles(int L, int nthreads) {
    const int half = ((L + 1) & ~1) / 2;
    return (size_t)2 * half + 2 * (size_t)nthreads + (2 * (size_t)half + L + 1) / 2 + 1;
}
__device__ __forceinline__ JacWs jac_carve(double* base, int L, int nthreads) {
    const int half = ((L + 1) & ~1) / 2;
    JacWs w;
    w.c = base; w.s = w.c + half; w.red = w.s + half;
    w.p = reinterpret_cast<int*>(w.red + 2 * nthreads); w.q = w.p + half; w.rank = w.q + half;
    return w;
}
// MB > 0: A and the eigenvector accumulator live in LDS (2 L^2 doubles; L <= 16 MB, L <= 88); MB == 0: global memory
template <int MB>
__global__ __launch_bounds__(MB > 0 ? 768 : 1024) void k_eigh(double* A, int L, int64_t lda, double* Vtmp, double* V, int64_t ldv, double* w,
                                                                  double tol_rel, const int* flag) {
    if (flag && *flag == 0) return;
    extern __shared__ __attribute__((aligned(16))) double sm_eig[];
    const int tid = threadIdx.x, nt = blockDim.x;
    JacWs ws = jac_carve(sm_eig, L, nt);
    double* Aw = A; double* Vw = Vtmp; int64_t la = lda;
    if constexpr (MB > 0) {
        la = L | 1;
        Aw = sm_eig + jac_ws_doubles(L, nt); Vw = Aw + (size_t)L * la;
        for (int e = tid; e < L * L; e += nt) Aw[(e / L) * la + (e % L)] = A[(int64_t)(e / L) * lda + (e % L)];
        __syncthreads();
    }
    wg_jacobi_any<MB>(Aw, la, Vw, la, L, ws.c, ws.s, ws.p, ws.q, ws.red, tol_rel, /*graded=*/true);   // (op_eigh: small eigenvalues to their own size)
    wg_sort_eig(Aw, la, Vw, la, L, V, ldv, w, ws.rank);
}

// ---- split eigen-solver: rotations on A in one workgroup, eigenvector accumulation spread over the chip --------------
// The Jacobi rotations are decided by A alone; V <- V J only consumes (c, s) (the pairs (p, q) of a round are a pure
// function of the round number).  k_jacobi_a keeps A in LDS (so L up to 141 fits: no V beside it), runs the round-robin
// sweeps and LOGS every round's (c, s) to global memory; k_apply_rot then replays the log on the rows of V = I, one row
// per wave (rows are independent, so the replay runs on L waves in parallel instead of inside the single Jacobi
// workgroup), and scatters the columns into descending-eigenvalue order.
typedef double jf64x2 __attribute__((ext_vector_type(2)));
constexpr int JACA_MAX_SWEEPS = 24;
__host__ __device__ inline size_t jaca_lds_bytes(int L) {
    const int half = ((L + 1) & ~1) / 2;
    return sizeof(double) * ((size_t)L * (L | 1) + 2 * (size_t)half + 64);
}
// workgroup barrier that orders LDS traffic only: waits for this wave's LDS operations (lgkmcnt) but leaves its global
// stores in flight, unlike __syncthreads(), whose fence also drains vmcnt
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// round-robin tournament: pair k of round rd (Le players, Le - 1 rounds); p < q, or p == q for a bye (odd L)
__device__ __forceinline__ void pair_pq(int k, int rd, int Le, int L, int& p, int& q) {
    if (k == 0) { p = Le - 1; q = rd; }
    else { p = rd + k; if (p >= Le - 1) p -= Le - 1; q = rd - k; if (q < 0) q += Le - 1; }
    if (p > q) { const int t = p; p = q; q = t; }
    if (q >= L) q = p;
}
// the same pairs, advanced round by round without divisions: raw players (rd + k, rd - k) mod (Le - 1)
struct PairIt {
    int pr, qr;
    __device__ __forceinline__ void init(int k, int rd, int Le) {
        const int m = Le - 1;
        pr = (rd + k) % m; qr = ((rd - k) % m + m) % m;
    }
    __device__ __forceinline__ void next(int Le) {
        if (++pr >= Le - 1) pr = 0;
        if (++qr >= Le - 1) qr = 0;
    }
    __device__ __forceinline__ void get(int k, int Le, int L, int& p, int& q) const {
        p = (k == 0) ? Le - 1 : pr;
        q = (k == 0) ? pr : qr;  // pair 0 is (Le - 1, rd) and pr == rd for k == 0
        if (p > q) { const int t = p; p = q; q = t; }
        if (q >= L) q = p;
    }
};
__device__ __forceinline__ void jacobi_angle(double app, double aqq, double apq, double& c, double& s, double& t) {
    const double d = aqq - app;
    const double m = fmax(fabs(d), fabs(apq));
    if (m > 1e-140 && m < 1e140) {
        // t = sgn(d) 2 apq / (|d| + sqrt(d^2 + 4 apq^2)); hardware rsq / rcp seeds with Newton steps instead of the
        // IEEE sqrt / divide sequences.  t must be the root to full precision, not just c: the caller sets A[p][q] = 0 and
        // updates the diagonal in closed form, so an error delta in t leaves an unrecorded residual ~ delta ||A|| per
        // rotation (one Newton step each left 2e-13: eigenvalues below 1e-7 lambda_1 lost half their digits -- the
        // singular-value cliff at 10^-3.5 sigma_1 that tests/test_gpu_parity.py::test_gram_route_singular_value_floor found)
        const double x = d * d + 4.0 * apq * apq;
        double rs = __builtin_amdgcn_rsq(x);
        rs = rs * (1.5 - 0.5 * x * rs * rs);
        rs = rs * (1.5 - 0.5 * x * rs * rs);
        const double den = fabs(d) + x * rs;
        double r = __builtin_amdgcn_rcp(den);
        r = r * (2.0 - den * r);
        r = r * (2.0 - den * r);
        t = (d >= 0.0 ? 2.0 : -2.0) * apq * r;
    } else {
        const double theta = d / (2.0 * apq);
        t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    }
    const double y = t * t + 1.0;  // in [1, 2]
    double cr = __builtin_amdgcn_rsq(y);
    cr = cr * (1.5 - 0.5 * y * cr * cr);
    cr = cr * (1.5 - 0.5 * y * cr * cr);
    c = cr;
    s = t * cr;
}
// A is symmetric and stays symmetric, so only its UPPER triangle is kept and rotated: element {i, j} lives at
// (min, max).  A round touches every unordered pair of rotation pairs {k, k'} once (a 2 x 2 block, rotated from the left
// with k's and from the right with k''s angle), and the 2 x 2 diagonal block of each pair is updated in closed form by
// the thread that computes its angle.  Two thread roles:
//   angle threads (tid < half, the first PW threads): read (app, aqq, apq), compute (c, s), update the diagonal block;
//   block threads (tid >= PW): 16-lane group g owns the row pairs k = g and k = half-1-g, which together have exactly
//     half-1 partners k' > k.  Their operands do not depend on this round's angles, so addresses and the 2 x 2 blocks are
//     fetched BEFORE the barrier, under the angle threads' latency chain; after it only (c, s) are read and applied.
template <int MB2, int GW>  // GW-wide batches of partner pairs per lane: half - 1 <= GW MB2
__global__ __launch_bounds__(1024) void k_jacobi_a(const double* __restrict__ Ain, int L, int64_t lda, jf64x2* __restrict__ log_cs,
                                                   int* __restrict__ nrounds_out, double* __restrict__ w,
                                                   int* __restrict__ rank_out, int PW, double tol_rel, const int* __restrict__ flag) {
    if (flag && *flag == 0) return;  // the two-stage solver in front of this launch has already delivered (k_trieig_verdict)
    extern __shared__ __attribute__((aligned(16))) double sm_ja[];
    const int LD = L | 1;
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wv = tid >> 6, nw = nt >> 6;
    const int Le = (L + 1) & ~1, half = Le / 2, rounds = Le - 1;
    jf64x2* s_cs = reinterpret_cast<jf64x2*>(sm_ja);
    double* s_red = sm_ja + 2 * half;
    double* A = s_red + 64;
    {
        int r = tid / L, c = tid - r * L;
        const int dr = nt / L, dc = nt - dr * L;
        for (int e = tid; e < L * L; e += nt) {
            if (c >= r) A[r * LD + c] = Ain[(int64_t)r * lda + c];
            r += dr; c += dc;
            if (c >= L) { c -= L; ++r; }
        }
    }
    __syncthreads();
    // this block thread's slots j = k0 + 16 m: slot j < n1 -> (k = g, k' = g + 1 + j), else (k = gb, k' = gb + 1 + j - n1)
    const int bt = tid - PW, g = bt / GW, k0 = bt - g * GW;  // GW lanes per group of two row pairs
    const int gb = half - 1 - g, n1 = half - 1 - g;
    const int nslots = (bt < 0) ? 0 : ((g < gb) ? half - 1 : (g == gb ? n1 : 0));
    int R = 0;  // rounds logged so far
    if (tid == 0) s_red[63] = tol_rel <= 1e-15 ? INFINITY : 0.0;   // (fp64 callers only: a matrix formed from fp32 data has no digits down there)
    __syncthreads();
    for (int sweep = 0; sweep < JACA_MAX_SWEEPS && L >= 2; ++sweep) {
        const double viol = wg_jacobi_violation(A, LD, L, tol_rel, s_red);
        // (no "nearly there: one more sweep" shortcut: with clustered or tiny eigenvalues the step after |a_pq| ~ sqrt(tol) is
        // NOT at tol -- a_pq^2 / gap -- and stopping there left 3e-4 in the eigenvectors of a graded test matrix)
        if (!(viol > 1.0)) break;
#ifdef PETAL_DEBUG_COUNTERS
        if (tid == 0) g_dbg[0] = sweep + 1;
        long long _t0 = clock64();
#endif
        PairIt ita, itb, itk[MB2], itme;
        ita.init(max(g, 0), 0, Le); itb.init(max(gb, 0) % half, 0, Le); itme.init(min(tid, half - 1), 0, Le);
#pragma unroll
        for (int m = 0; m < MB2; ++m) {
            const int j = k0 + GW * m;
            itk[m].init(min(max(j < n1 ? g + 1 + j : gb + 1 + (j - n1), 0), half - 1), 0, Le);
        }
        for (int rd = 0; rd < rounds; ++rd, ++R) {
            double e00[MB2], e01[MB2], e10[MB2], e11[MB2];
            int i00[MB2], i01[MB2], i10[MB2], i11[MB2], kpv[MB2];
            if (tid < half) {
                int p, q;
                itme.get(tid, Le, L, p, q);
                double c = 1.0, sn = 0.0;
                if (p != q) {
                    // (all three operands requested at once: a dependent second LDS round trip costs ~100 cycles of the
                    // angle chain, which is the longest leg of a round)
                    const double apq = A[p * LD + q], app = A[p * LD + p], aqq = A[q * LD + q];
                    if (apq != 0.0) {
                        double t;
                        jacobi_angle(app, aqq, apq, c, sn, t);
                        A[p * LD + p] = app - t * apq;
                        A[q * LD + q] = aqq + t * apq;
                        A[p * LD + q] = 0.0;
                    }
                }
                s_cs[tid] = jf64x2{c, sn};
                log_cs[(size_t)R * half + tid] = jf64x2{c, sn};
            } else if (nslots > 0) {
                int pa, qa, pb, qb;
                ita.get(g, Le, L, pa, qa);
                itb.get(gb, Le, L, pb, qb);
#pragma unroll
                for (int m = 0; m < MB2; ++m) {
                    const int j = k0 + GW * m;
                    const bool first = j < n1;
                    const int kp = min(first ? g + 1 + j : gb + 1 + (j - n1), half - 1);
                    kpv[m] = kp;
                    const int p = first ? pa : pb, q = first ? qa : qb;
                    int p2, q2;
                    itk[m].get(kp, Le, L, p2, q2);
                    i00[m] = min(p, p2) * LD + max(p, p2);
                    i01[m] = min(p, q2) * LD + max(p, q2);
                    i10[m] = min(q, p2) * LD + max(q, p2);
                    i11[m] = min(q, q2) * LD + max(q, q2);
                    e00[m] = A[i00[m]]; e01[m] = A[i01[m]]; e10[m] = A[i10[m]]; e11[m] = A[i11[m]];
                }
            }
            DBG_T(0);
            lds_barrier();  // NOT __syncthreads(): that also waits for the global log stores (vmcnt), ~1 us per round
            DBG_T(1);
            if (nslots > 0) {
                const jf64x2 csa = s_cs[g], csb = s_cs[gb];
                jf64x2 cs2[MB2];
#pragma unroll
                for (int m = 0; m < MB2; ++m) cs2[m] = s_cs[kpv[m]];
#pragma unroll
                for (int m = 0; m < MB2; ++m) {
                    const int j = k0 + GW * m;
                    if (j >= nslots) continue;
                    const jf64x2 cs = (j < n1) ? csa : csb;
                    // right rotation (columns p', q') with the partner's angle, then left rotation (rows p, q) with ours
                    const double a1 = cs2[m][0] * e00[m] - cs2[m][1] * e01[m], b1 = cs2[m][1] * e00[m] + cs2[m][0] * e01[m];
                    const double c1 = cs2[m][0] * e10[m] - cs2[m][1] * e11[m], d1 = cs2[m][1] * e10[m] + cs2[m][0] * e11[m];
                    A[i00[m]] = cs[0] * a1 - cs[1] * c1;
                    A[i01[m]] = cs[0] * b1 - cs[1] * d1;
                    A[i10[m]] = cs[1] * a1 + cs[0] * c1;
                    A[i11[m]] = cs[1] * b1 + cs[0] * d1;
                }
            }
            DBG_T(2);
            lds_barrier();
            DBG_T(3);
            ita.next(Le); itb.next(Le); itme.next(Le);
#pragma unroll
            for (int m = 0; m < MB2; ++m) itk[m].next(Le);
        }
    }
    if (tid == 0) *nrounds_out = R;
    for (int j = tid; j < L; j += nt) {  // descending order: rank[j] = position of eigenvalue j
        const double wj = A[j * LD + j];
        int rank = 0;
        for (int k = 0; k < L; ++k) {
            const double wk = A[k * LD + k];
            rank += (wk > wj || (wk == wj && k < j)) ? 1 : 0;
        }
        rank_out[j] = rank;
        w[rank] = wj;
    }
}


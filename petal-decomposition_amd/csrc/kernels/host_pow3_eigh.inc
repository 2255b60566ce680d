// host_pow3_eigh.inc -- part of the ONE translation unit hip_ops.hip (textually included there, inside namespace petal): host-side launchers: the fused pass, Cholesky / eigen-solver / remaining small ops.
// ---- the fused power-iteration pass (k_pow3) ------------------------------------------------------------------------------
static bool pow3_ok(Dev* d, int dt, const void* X, int64_t n, int64_t K, int64_t ldx, const void* mu, int64_t N, const void* Z, int64_t ldz) {
    const int64_t min_rows = (int64_t)d->opt[OPT_FUSED_PASS_MIN_ROWS];
    return opt_on(d, OPT_FUSED_PASS) && dt == F32 && d->gemm_mode == 0 && (K == 512 || K == 256) && N % 16 == 0 && N >= 16 && N <= 80 && n >= min_rows &&
           n < (int64_t(1) << 40) && ldx % 4 == 0 && aligned16(X) && (!mu || aligned16(mu)) && (!Z || (ldz >= N && aligned16(Z)));
}
// (the knobs that keep an operand at three planes also keep its product off the fused kernel, whose P is a two-plane one by construction)
static bool pow3_knob_off(const Dev* d, int opt) { return !opt_on(d, OPT_TWO_PLANE) || !opt_on(d, opt); }
bool op_power_pass_applies(Dev* d, int dt, const void* X, int64_t n, int64_t K, int64_t ldx, const void* mu, int64_t N) {
    return pow3_ok(d, dt, X, n, K, ldx, mu, N, nullptr, 0);
}
// Ppk3: the packed planes of the K x N small operand (k_pack_p3's layout; planes 0 and 1 are read)
// ssq_parts_out (nullable; needs mu and no Z): the MEANS form -- mu is a provisional centre, Y's last column comes back as the column
// sums about it and *ssq_parts_out as a device array of *nparts_out partials of sum (x - mu)^2 (see k_pow3)
// `steering`: the pass only steers the iteration (not the last one of a fit): it may take the four-piece kernel k_pow3f
static void launch_pow3(Dev* d, const float* X, int64_t n, int64_t K, int64_t ldx, const float* mu, const bf16x8* Ppk3, int64_t N, float* Z, int64_t ldz,
                        double* Y, int64_t ldy, double** ssq_parts_out = nullptr, int* nparts_out = nullptr, bool steering = false) {
    const bool ssq_out = ssq_parts_out != nullptr;
    const bool no_fast = !opt_on(d, OPT_STEERING);
    if (steering && !no_fast && !Z) {
        const int NT = (int)(N / 16);
        const int64_t nstages = cdiv(n, 32);
        const int grid = (int)std::min<int64_t>(num_cus(d), nstages);
        float* part = (float*)dev_alloc(d, sizeof(float) * (size_t)grid * K * N);
        double* ssq_part = ssq_out ? (double*)dev_alloc(d, sizeof(double) * (size_t)grid * 8) : nullptr;
        const size_t lds = (size_t)8 * 8192 + (size_t)2 * 8 * NT * 1024 + (size_t)NT * 2048 + 2048;
#define POW3F_GO(NTv, CE, ME)                                                                                                      \
    do {                                                                                                                           \
        if (K == 512) {                                                                                                            \
            set_max_lds(d, reinterpret_cast<const void*>(k_pow3f<NTv, CE, ME, 2>));                                                \
            hipLaunchKernelGGL((k_pow3f<NTv, CE, ME, 2>), dim3(grid), dim3(512), lds, d->stream, X, n, ldx, mu, Ppk3, NT, part, nstages, ssq_part); \
        } else {                                                                                                                   \
            set_max_lds(d, reinterpret_cast<const void*>(k_pow3f<NTv, CE, ME, 1>));                                                \
            hipLaunchKernelGGL((k_pow3f<NTv, CE, ME, 1>), dim3(grid), dim3(512), lds, d->stream, X, n, ldx, mu, Ppk3, NT, part, nstages, ssq_part); \
        }                                                                                                                          \
    } while (0)
#define POW3F_NT(NTv) do { if (ssq_out) POW3F_GO(NTv, true, true); else if (mu) POW3F_GO(NTv, true, false); else POW3F_GO(NTv, false, false); } while (0)
        {
            TagScope ts(d);
            switch (NT) {
                case 5: POW3F_NT(5); break;
                case 4: POW3F_NT(4); break;
                case 3: POW3F_NT(3); break;
                case 2: POW3F_NT(2); break;
                default: POW3F_NT(1); break;
            }
            launch_check();
            ts.stop();
        }
#undef POW3F_NT
#undef POW3F_GO
        hipLaunchKernelGGL(k_sum_parts4, dim3(cdiv(K * N, 128)), dim3(256), 0, d->stream, part, (int64_t)grid, (int64_t)K * N, Y, N, ldy);
        launch_check();
        dev_free(d, part);
        if (ssq_parts_out) { *ssq_parts_out = ssq_part; *nparts_out = grid * 8; }   // (the caller's next kernel adds them; it frees the block)
        return;
    }
    const int NT = (int)(N / 16);
    const int64_t nstages = cdiv(n, 32);
    const int grid = (int)std::min<int64_t>(num_cus(d), nstages);
    float* part = (float*)dev_alloc(d, sizeof(float) * (size_t)grid * K * N);
    double* ssq_part = ssq_out ? (double*)dev_alloc(d, sizeof(double) * (size_t)grid * 8) : nullptr;
    const size_t lds = (size_t)8 * 12288 + (size_t)8 * NT * 1024 + (size_t)NT * 3072 + 2048;
#define POW3_GO(NTv, CE, SZ, ME)                                                                                                  \
    do {                                                                                                                          \
        if (K == 512) {                                                                                                           \
            set_max_lds(d, reinterpret_cast<const void*>(k_pow3<NTv, CE, SZ, ME, 2>));                                            \
            hipLaunchKernelGGL((k_pow3<NTv, CE, SZ, ME, 2>), dim3(grid), dim3(512), lds, d->stream, X, n, ldx, mu, Ppk3, NT, part, Z, ldz, nstages, ssq_part); \
        } else {                                                                                                                  \
            set_max_lds(d, reinterpret_cast<const void*>(k_pow3<NTv, CE, SZ, ME, 1>));                                            \
            hipLaunchKernelGGL((k_pow3<NTv, CE, SZ, ME, 1>), dim3(grid), dim3(512), lds, d->stream, X, n, ldx, mu, Ppk3, NT, part, Z, ldz, nstages, ssq_part); \
        }                                                                                                                         \
    } while (0)
#define POW3_NT(NTv)                                                                                                              \
    do {                                                                                                                          \
        if (ssq_out) POW3_GO(NTv, true, false, true);                                                                             \
        else if (mu && Z) POW3_GO(NTv, true, true, false); else if (mu) POW3_GO(NTv, true, false, false);                         \
        else if (Z) POW3_GO(NTv, false, true, false); else POW3_GO(NTv, false, false, false);                                     \
    } while (0)
    {
        TagScope ts(d);
        switch (NT) {
            case 5: POW3_NT(5); break;
            case 4: POW3_NT(4); break;
            case 3: POW3_NT(3); break;
            case 2: POW3_NT(2); break;
            default: POW3_NT(1); break;
        }
        launch_check();
        ts.stop();
    }
#undef POW3_NT
#undef POW3_GO
    hipLaunchKernelGGL(k_sum_parts4, dim3(cdiv(K * N, 128)), dim3(256), 0, d->stream, part, (int64_t)grid, (int64_t)K * N, Y, N, ldy);
    launch_check();
    dev_free(d, part);
    if (ssq_parts_out) { *ssq_parts_out = ssq_part; *nparts_out = grid * 8; }   // (the caller's next kernel adds them; it frees the block)
}
// the move from the provisional centre to the true one (see k_pow3, MEANS).  One workgroup per FOUR columns of Y:
//   delta_f = Y[f][c1] / n;  t_j = sum_f delta_f P[f][j];  Y[f][j] -= n delta_f t_j (j < L);  Y[f][c1] = 0;
// workgroup 0 also: mu64 = mu0 + delta (+ muT, the data type's copy) and *tv = (sum of the waves' partials of sum (x - mu0)^2) - n |delta|^2.
// (every workgroup reads the sums column c1, so nobody may zero it in the same launch: that is the second launch, k_mean_fix<true>)
template <bool FINISH>
__global__ __launch_bounds__(256) void k_mean_fix(double* __restrict__ Y, int K, int d, int N, int64_t ldy, int c1, int L, double n_total,
                                                  const double* __restrict__ P, int64_t ldp, double* __restrict__ mu64, float* __restrict__ muT,
                                                  const double* __restrict__ ssq_part, int nparts, double* __restrict__ tv) {
    __shared__ double sd[512];
    __shared__ double sr[256];
    __shared__ double st[4];
    const int tid = threadIdx.x;
    if (FINISH) {        // (second launch, one workgroup: the sums column is no longer needed)
        for (int f = tid; f < K; f += 256) Y[(int64_t)f * ldy + c1] = 0.0;
        return;
    }
    for (int f = tid; f < K; f += 256) sd[f] = f < d ? Y[(int64_t)f * ldy + c1] / n_total : 0.0;
    __syncthreads();
    const int j0 = blockIdx.x * 4, jj = tid & 3, fl = tid >> 2;      // 64 row lanes x 4 columns
    double acc = 0;
    // (the fused pass multiplied by the TWO-PLANE P: the rank-one correction uses the same rounded values -- bf16(p) + bf16(p - bf16(p)),
    // round-to-nearest-even each, what v_cvt_pk_bf16_f32 and the host simulation oracle/cpu_ops.cpp two_plane() do)
    auto two_plane = [](double v) {
        auto bf = [](float f) {
            unsigned u = __float_as_uint(f);
            u = (u + 0x7fffu + ((u >> 16) & 1u)) & 0xffff0000u;
            return __uint_as_float(u);
        };
        const float f = (float)v, h = bf(f), m = bf(f - h);
        return (double)h + (double)m;
    };
    if (j0 + jj < L)
        for (int f = fl; f < K; f += 64) acc += sd[f] * two_plane(P[(int64_t)f * ldp + j0 + jj]);
    sr[tid] = acc;
    __syncthreads();
    if (tid < 4) {
        double t = 0;
        for (int g = 0; g < 64; ++g) t += sr[g * 4 + tid];
        st[tid] = t;
    }
    __syncthreads();
    if (j0 + jj < L && j0 + jj != c1)
        for (int f = fl; f < K; f += 64) Y[(int64_t)f * ldy + j0 + jj] -= n_total * sd[f] * st[jj];
    if (blockIdx.x == 0) {
        double q = 0;
        for (int f = tid; f < K; f += 256) q += sd[f] * sd[f];
        double sp = 0;
        for (int e = tid; e < nparts; e += 256) sp += ssq_part[e];
        __syncthreads();
        sr[tid] = q;
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) { if (tid < h) sr[tid] += sr[tid + h]; __syncthreads(); }
        const double q2 = sr[0];
        __syncthreads();
        sr[tid] = sp;
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) { if (tid < h) sr[tid] += sr[tid + h]; __syncthreads(); }
        if (tid == 0) tv[0] = fmax(sr[0] - n_total * q2, 0.0);
        for (int f = tid; f < K; f += 256) {
            const double m = (double)muT[f] + sd[f];   // (about the centre the pass SUBTRACTED: the float32 one, not the fp64 mean it was rounded from)
            mu64[f] = m;
            muT[f] = (float)m;
        }
    }
}
bool op_power_pass_means(Dev* d, int dt, const void* X, int64_t n, int64_t K, int64_t dcols, int64_t ldx, double n_total, const double* P,
                         int64_t N, int64_t ldp, int64_t L, double* Y, int64_t ldy, double* mu64, void* muT, double* ssq_scratch, double* tv) {
    const bool off = d->opt[OPT_MEANS_FOLD_ROWS] < 0 || pow3_knob_off(d, OPT_TWO_PLANE_OMEGA);
    if (off || L >= N || !pow3_ok(d, dt, X, n, K, ldx, muT, N, nullptr, 0)) return false;
    // the provisional centre: the means of a strided sample of the rows (one small pass)
    const int64_t ns = std::min<int64_t>(n, 4096), stride = n / ns;
    op_colmean(d, dt, X, ns, K, ldx * stride, double(ns), mu64, muT, false);
    const int64_t total = (K / 32) * (N / 16) * 64;
    bf16x8* Ppk3 = (bf16x8*)dev_alloc(d, sizeof(bf16x8) * total * 3);
    hipLaunchKernelGGL(k_pack_p3, dim3(cdiv(total, 256)), dim3(256), 0, d->stream, P, K, N, ldp, Ppk3, (int)(N / 16), total);
    launch_check();
    double* parts = nullptr;
    int nparts = 0;
    launch_pow3(d, (const float*)X, n, K, ldx, (const float*)muT, Ppk3, N, nullptr, 0, Y, ldy, &parts, &nparts, /*steering=*/true);
    dev_free(d, Ppk3);
    (void)ssq_scratch;
    const int c1 = (int)(N - 1);
    hipLaunchKernelGGL(k_mean_fix<false>, dim3((unsigned)cdiv(L, 4)), dim3(256), 0, d->stream, Y, (int)K, (int)dcols, (int)N, ldy, c1, (int)L, n_total, P, ldp,
                       mu64, (float*)muT, (const double*)parts, nparts, tv);
    hipLaunchKernelGGL(k_mean_fix<true>, dim3(1), dim3(256), 0, d->stream, Y, (int)K, (int)dcols, (int)N, ldy, c1, (int)L, n_total, P, ldp, mu64,
                       (float*)muT, (const double*)parts, nparts, tv);
    launch_check();
    dev_free(d, parts);
    return true;
}
bool op_power_pass(Dev* d, int dt, const void* X, int64_t n, int64_t K, int64_t ldx, const void* mu, const double* P, int64_t N, int64_t ldp,
                   void* Z, int64_t ldz, double* Y, int64_t ldy, bool steering) {
    const bool knob = pow3_knob_off(d, OPT_TWO_PLANE_OMEGA);
    if (knob || !pow3_ok(d, dt, X, n, K, ldx, mu, N, Z, ldz)) return false;
    const int64_t total = (K / 32) * (N / 16) * 64;
    bf16x8* Ppk3 = (bf16x8*)dev_alloc(d, sizeof(bf16x8) * total * 3);
    hipLaunchKernelGGL(k_pack_p3, dim3(cdiv(total, 256)), dim3(256), 0, d->stream, P, K, N, ldp, Ppk3, (int)(N / 16), total);
    launch_check();
    launch_pow3(d, (const float*)X, n, K, ldx, (const float*)mu, Ppk3, N, (float*)Z, ldz, Y, ldy, nullptr, nullptr, steering && Z == nullptr);
    dev_free(d, Ppk3);
    return true;
}
bool op_rebase_power_pass(Dev* d, int dt, const void* X, int64_t n, int64_t K, int64_t ldx, const void* mu, const double* G, int64_t L,
                          int64_t ldg, double rel_tol, int* ndead, const double* A, int64_t M, int64_t lda, double* T, int64_t ldt,
                          double* P_out, int64_t ldpo, void* Z, int64_t ldz, double* Y, int64_t ldy, bool steering) {
    const bool no_rt = pow3_knob_off(d, OPT_TWO_PLANE_ITERATE);
    if (!pow3_ok(d, dt, X, n, K, ldx, mu, M, Z, ldz) || no_rt || L == 0 || L > CHOL2_MAXL || M > TRSM_MAXM || M < L || P_out == nullptr) return false;
    launch_chol_rt(d, G, L, ldg, T, ldt, rel_tol, ndead, M);
    const int NTtot = (int)(M / 16);
    const int64_t total = (K / 32) * (int64_t)NTtot * 64;
    bf16x8* Ppk3 = (bf16x8*)dev_alloc(d, sizeof(bf16x8) * total * 3);
    switch (NTtot) {   // P_out = A R^-1, ROUNDED to two planes, and its operand planes
#define PETAL_TRSM_CASE(NB)                                                                                                            \
    case NB:                                                                                                                           \
        hipLaunchKernelGGL((k_trsm_pack<NB, true>), dim3(cdiv(K, 16)), dim3(64), trsm_lds_bytes(16 * NB), d->stream, A, lda, T, ldt, K, P_out, \
                           ldpo, Ppk3, NTtot);                                                                                         \
        break
        PETAL_TRSM_CASE(1); PETAL_TRSM_CASE(2); PETAL_TRSM_CASE(3); PETAL_TRSM_CASE(4); PETAL_TRSM_CASE(5);
#undef PETAL_TRSM_CASE
        default: throw std::runtime_error("op_rebase_power_pass: order out of range");
    }
    launch_check();
    launch_pow3(d, (const float*)X, n, K, ldx, (const float*)mu, Ppk3, M, (float*)Z, ldz, Y, ldy, nullptr, nullptr, steering && Z == nullptr);
    dev_free(d, Ppk3);
    return true;
}

void op_chol_inv(Dev* d, const double* G, int64_t L, int64_t ldg, double* T, int64_t ldt, double rel_tol, int* ndead, int64_t Lz,
                 int64_t ndead_cols) {
    if (L == 0) return;
    if (Lz < L) Lz = L;
    // k_chol_inv2 takes the orders up to 140; beyond, the blocked right-looking factorisation on the chip-wide fp64 GEMM kernel.
    // (Orders 141 .. 200 once ran an older one-workgroup kernel, k_chol_inv, whose build-T-in-global-memory mode no test reached and
    // whose factors were WRONG -- RandomizedPca with 132 <= k <= 190, found by dev/fuzz_rpca.py in round 3; retired in round 6.)
    if (L > CHOL2_MAXL) { chol_inv_blocked(d, G, L, ldg, T, ldt, rel_tol, ndead, Lz); return; }
    set_max_lds(d, reinterpret_cast<const void*>(k_chol_inv2));
    hipLaunchKernelGGL(k_chol_inv2, dim3(1), dim3(CHOL_THREADS), chol2_lds_bytes((int)L), d->stream, G, (int)L, ldg, T, ldt, rel_tol,
                       ndead, (int)Lz, (const double*)nullptr, 0, (int)(ndead_cols > 0 ? ndead_cols : L));
    launch_check();
}
bool op_chol_rt(Dev* d, int dt, int64_t n, const double* G, int64_t L, int64_t ldg, double* T, int64_t ldt, double rel_tol, int* ndead,
                int64_t Lz, int64_t ndead_cols) {
    if (Lz < L) Lz = L;
    (void)dt; (void)n;   // (every data type and GEMM mode: the consumers below have a form without operand planes)
    const bool rt = L > 0 && L <= CHOL2_MAXL && Lz % 16 == 0 && Lz <= TRSM_MAXM;
    if (!rt) { op_chol_inv(d, G, L, ldg, T, ldt, rel_tol, ndead, Lz, ndead_cols); return false; }
    launch_chol_rt(d, G, L, ldg, T, ldt, rel_tol, ndead, Lz, ndead_cols);
    return true;
}
void op_trsm_right(Dev* d, const double* A, int64_t rows, int64_t lda, const double* RT, int64_t M, int64_t ldt, double* out, int64_t ldo) {
    if (rows % 16 != 0 || M % 16 != 0 || M > TRSM_MAXM) throw std::logic_error("op_trsm_right: shape outside the kernel");
    switch ((int)(M / 16)) {
#define PETAL_TRSMR_CASE(NB)                                                                                                         \
    case NB:                                                                                                                         \
        hipLaunchKernelGGL((k_trsm_pack<NB, false>), dim3(cdiv(rows, 16)), dim3(64), trsm_lds_bytes(16 * NB), d->stream, A, lda, RT, ldt, rows, \
                           out, ldo, (bf16x8*)nullptr, NB);                                                                          \
        break
        PETAL_TRSMR_CASE(1); PETAL_TRSMR_CASE(2); PETAL_TRSMR_CASE(3); PETAL_TRSMR_CASE(4); PETAL_TRSMR_CASE(5);
        PETAL_TRSMR_CASE(6); PETAL_TRSMR_CASE(7); PETAL_TRSMR_CASE(8); PETAL_TRSMR_CASE(9);
#undef PETAL_TRSMR_CASE
        default: throw std::logic_error("op_trsm_right: order out of range");
    }
    launch_check();
}
void op_eigh(Dev* d, double* A, int64_t L, int64_t lda, double* V, int64_t ldv, double* w, double tol_rel, bool clustered, int64_t Lz, int64_t ncheck,
             int* verdict, bool verdict_fresh, double gap_tol_override) {
    if (L == 0) { if (verdict && verdict_fresh) HIP_CHECK(hipMemsetAsync(verdict, 0, sizeof(int), d->stream)); return; }
    const bool pad_done = Lz <= L;   // else: rows / columns L .. Lz - 1 of V are to be zeroed here
    if (L > EIG_MAXL) throw std::runtime_error("eigh: matrix too large for the one-workgroup Jacobi solver");
    // Two-stage solver first (tridiagonalisation on one workgroup, then one wave per eigenpair over the chip); the Jacobi
    // launches below run behind it and return at once unless its verdict flags eigenvalues too close for its vectors.
    const bool jacobi_only = opt_on(d, OPT_EIGH_JACOBI);
    int* flag = nullptr;
    char* ts = nullptr;
    const bool two_stage = !jacobi_only && !clustered && L >= 3 && L <= 2048;
    // verdict given (and the order is one the register-resident kernels take): the two-stage result is delivered as it is and
    // the verdict goes to the caller's device word, who decides what to do about a flagged spectrum (RandomizedPca redoes the
    // fit on its robust path) -- the two fallback launches, which return at once on every separated spectrum, are not issued
    const bool ext_verdict = verdict != nullptr && two_stage && L <= 138;
    // (verdict_fresh: the caller's word is cleared first -- by the tridiagonalisation kernel itself where it runs)
    if (verdict && verdict_fresh && !ext_verdict) HIP_CHECK(hipMemsetAsync(verdict, 0, sizeof(int), d->stream));
    // k_tridiag_r (orders up to 138) writes the padding itself; every other route gets one 2-D clear of the Lz x Lz frame first
    if (!pad_done && !(two_stage && L <= 138)) HIP_CHECK(hipMemset2DAsync(V, sizeof(double) * ldv, 0, sizeof(double) * Lz, Lz, d->stream));
    if (two_stage) {
        // eigenvectors of eigenvalues closer than gap_tol ||A|| come out only eps / gap_tol accurate: fp32 results carry
        // 2e-8, fp64 results 2e-11; anything closer goes to Jacobi
        const double gap_tol = gap_tol_override > 0 ? gap_tol_override : (tol_rel >= 1e-9 ? 1e-8 : 1e-5);
        const int64_t ldw = L | 1;
        const size_t lds_in = sizeof(double) * ((size_t)L * ldw + 2 * L + 32);
        const bool inlds = lds_in <= 160 * 1024 - 256;
        const bool regs = L <= 138;                               // (the padded working copy of k_tridiag_r fits the LDS)
        const size_t bytes = sizeof(double) * (4 * L + L * L + (inlds ? 0 : L * ldw)) + 64;
        ts = (char*)dev_alloc(d, bytes);
        double* dd = reinterpret_cast<double*>(ts);
        double* ee = dd + L;
        double* tau = ee + L;
        double* gg = tau + L;
        double* HV = gg + L;
        double* Wg = inlds ? nullptr : HV + L * L;
        flag = reinterpret_cast<int*>(ts + bytes - 64);
        if (ext_verdict) flag = verdict;   // (the closeness verdict ORs into the caller's word; no Jacobi launches behind it)
        if (regs) {
#define PETAL_TRI_LAUNCH(TM, ST)                                                                                                   \
    do {                                                                                                                           \
        const size_t lds_r = sizeof(double) * ((size_t)L * tri_ld((int)L, ST) + 8 * TM + tri_sp_len(TM));                          \
        set_max_lds(d, reinterpret_cast<const void*>(k_tridiag_r<TM, ST>));                                                        \
        hipLaunchKernelGGL((k_tridiag_r<TM, ST>), dim3(1), dim3(TRR_THREADS), lds_r, d->stream, A, (int)L, lda, dd, ee, HV, tau, gg, flag, V, ldv, (int)(pad_done ? 0 : Lz), (ext_verdict && !verdict_fresh) ? 0 : 1); \
    } while (0)
#define PETAL_TRIW_LAUNCH(TM)                                                                                                      \
    do {                                                                                                                           \
        const size_t lds_r = sizeof(double) * ((size_t)L * triw_ld((int)L, TM) + 32 * TM);                                         \
        set_max_lds(d, reinterpret_cast<const void*>(k_tridiag_w<TM>));                                                            \
        hipLaunchKernelGGL((k_tridiag_w<TM>), dim3(1), dim3(TRR_THREADS), lds_r, d->stream, A, (int)L, lda, dd, ee, HV, tau, gg, flag, V, ldv, (int)(pad_done ? 0 : Lz), (ext_verdict && !verdict_fresh) ? 0 : 1); \
    } while (0)
            // l <= 80: the 8-byte form (78.5 us at l = 74, where a step is a chain of latencies and the 16-byte form measures 83.6);
            // above: the 16-byte form (238 us at l = 138 against 290).  (Round 6 built a form with the MATRIX in registers, only vectors
            // through LDS: parity-green and no faster -- 78.2 us at l = 74: the step is a chain of dependent latencies, not LDS
            // bandwidth; dev/tridiag_q_kernel.h, EXPERIMENTS.md.)
            if (L <= 80) PETAL_TRI_LAUNCH(10, 2);
            else PETAL_TRIW_LAUNCH(9);
#undef PETAL_TRI_LAUNCH
#undef PETAL_TRIW_LAUNCH
            launch_check();
            const int hv_rows = (int)std::min<int64_t>(L - 2, (96 * 1024) / (8 * L));
            const size_t lds_e = sizeof(double) * (23 * (((L + 7) & ~7) + 8) + (size_t)hv_rows * L);
            if (L <= 128) {
                set_max_lds(d, reinterpret_cast<const void*>(k_trieig_r<4, 2>));
                hipLaunchKernelGGL((k_trieig_r<4, 2>), dim3(cdiv(L, 4)), dim3(256), lds_e, d->stream, dd, ee, HV, tau, gg, (int)L, gap_tol, hv_rows, w, V, ldv, flag, (int)(ncheck > 0 ? ncheck : L));
            } else {
                set_max_lds(d, reinterpret_cast<const void*>(k_trieig_r<4, 3>));
                hipLaunchKernelGGL((k_trieig_r<4, 3>), dim3(cdiv(L, 4)), dim3(256), lds_e, d->stream, dd, ee, HV, tau, gg, (int)L, gap_tol, hv_rows, w, V, ldv, flag, (int)(ncheck > 0 ? ncheck : L));
            }
            launch_check();
        } else {
            {
            // one launch per Householder step, the whole chip per launch (k_tridiag_mw): 29 -> ~5 ms at order 512
            const int64_t ldm = L | 1;
            double* mw = (double*)dev_alloc(d, sizeof(double) * ((size_t)L * ldm + 4 * L));
            double* vp = mw + (size_t)L * ldm;
            HIP_CHECK(hipMemcpy2DAsync(mw, ldm * sizeof(double), A, lda * sizeof(double), L * sizeof(double), L, hipMemcpyDeviceToDevice, d->stream));
            HIP_CHECK(hipMemsetAsync(vp, 0, sizeof(double) * 4 * L, d->stream));
            HIP_CHECK(hipMemsetAsync(HV, 0, sizeof(double) * L * L, d->stream));
            const size_t lds_mw = sizeof(double) * (3 * L + 16);
            for (int64_t k = 0; k < L; ++k) {
                const int64_t m = L - k - 1;
                const unsigned grid = (unsigned)std::min<int64_t>(512, std::max<int64_t>(1, (m + 3) / 4));
                hipLaunchKernelGGL(k_tridiag_mw, dim3(grid), dim3(256), lds_mw, d->stream, mw, ldm, (int)L, (int)k, vp + ((k + 1) & 1) * 2 * L,
                                   vp + (k & 1) * 2 * L, dd, ee, HV, tau);
            }
            launch_check();
            dev_free(d, mw);
            }
            launch_check();
            if (L <= 512) {
                hipLaunchKernelGGL(k_trieig<4>, dim3(cdiv(L, 4)), dim3(256), sizeof(double) * 15 * L, d->stream, dd, ee, HV, tau, (int)L, w, V, ldv);
            } else {
                set_max_lds(d, reinterpret_cast<const void*>(k_trieig<1>));
                hipLaunchKernelGGL(k_trieig<1>, dim3((unsigned)L), dim3(64), sizeof(double) * 6 * L, d->stream, dd, ee, HV, tau, (int)L, w, V, ldv);
            }
            launch_check();
            hipLaunchKernelGGL(k_trieig_verdict, dim3(1), dim3(1024), 0, d->stream, w, ee, (int)L, gap_tol, A, lda, flag, (int)(ncheck > 0 ? ncheck : L));
            launch_check();
        }
    }
    struct Cleanup { Dev* d; char* p; ~Cleanup() { if (p) dev_free(d, p); } } cleanup{d, ts};
    if (ext_verdict) return;
    if (jaca_lds_bytes((int)L) <= 160 * 1024 - 256) {
        // split solver: A in LDS + rotation log, eigenvectors replayed on L waves
        const int Le = (int)((L + 1) & ~1), half = Le / 2, rounds = Le - 1;
        const size_t nlog = (size_t)JACA_MAX_SWEEPS * rounds * half;
        char* buf = (char*)dev_alloc(d, nlog * 16 + 16 + sizeof(int) * (L + 4));
        jf64x2* log_cs = reinterpret_cast<jf64x2*>(buf);
        int* nrounds = reinterpret_cast<int*>(buf + nlog * 16);
        int* rank = nrounds + 4;
        // block threads: groups of GW lanes own two row pairs each; 32-lane groups (fewer blocks per thread: the rounds are
        // paced by the per-thread work on both sides of the barrier) while the workgroup still fits 1024 threads
        const int groups = (half + 1) / 2;                                // two row pairs each
        const int pw = (half + 63) / 64 * 64;                             // angle threads (whole waves)
        const int gw = (pw + 32 * groups <= 1024) ? 32 : 16;
        const int mb2 = std::max(1, (half - 1 + gw - 1) / gw);            // partner pairs per lane
        const int threads = std::min(1024, (pw + gw * groups + 63) / 64 * 64);
        const size_t lds = jaca_lds_bytes((int)L);
#define JACA_CASE(M, G)                                                                                                  \
    case 10 * M + (G == 32 ? 1 : 0): {                                                                                   \
        set_max_lds(d, reinterpret_cast<const void*>(k_jacobi_a<M, G>));                        \
        hipLaunchKernelGGL((k_jacobi_a<M, G>), dim3(1), dim3(threads), lds, d->stream, A, (int)L, lda, log_cs, nrounds, w, rank, pw, tol_rel, (const int*)flag); \
    } break;
        // (of the eight instantiations only (1, 32), (2, 32), (4, 16) and (5, 16) are ever taken: 16-lane groups need more than 60
        // row pairs, which is mb2 >= 4, and 32-lane groups at most 60, which is mb2 <= 2 -- tests/smallmat_cases.py::jacobi_form)
        switch (10 * std::min(mb2, 5) + (gw == 32 ? 1 : 0)) {
            JACA_CASE(1, 16) JACA_CASE(2, 16) JACA_CASE(3, 16) JACA_CASE(4, 16) JACA_CASE(5, 16)
            JACA_CASE(1, 32) JACA_CASE(2, 32) JACA_CASE(3, 32)
            default: throw std::runtime_error("eigh: unsupported size for the split Jacobi solver");
        }
#undef JACA_CASE
        launch_check();
        const int hp = (half + 63) / 64;
        const dim3 grid((unsigned)cdiv(L, JR_WAVES));
        const size_t lds2 = sizeof(double) * JR_WAVES * Le;
        if (hp <= 1) hipLaunchKernelGGL(k_apply_rot<1>, grid, dim3(64 * JR_WAVES), lds2, d->stream, log_cs, nrounds, rank, (int)L, V, ldv, (const int*)flag);
        else hipLaunchKernelGGL(k_apply_rot<2>, grid, dim3(64 * JR_WAVES), lds2, d->stream, log_cs, nrounds, rank, (int)L, V, ldv, (const int*)flag);
        launch_check();
        dev_free(d, buf);
        return;
    }
    double* Vtmp = (double*)dev_alloc(d, sizeof(double) * L * lda);  // (the kernel indexes it with A's leading dimension)
    const size_t lds = sizeof(double) * jac_ws_doubles((int)L, 1024);
    {
        set_max_lds(d, reinterpret_cast<const void*>(k_eigh<0>));
        hipLaunchKernelGGL(k_eigh<0>, dim3(1), dim3(1024), lds, d->stream, A, (int)L, lda, Vtmp, V, ldv, w, tol_rel, (const int*)flag);
    }
    launch_check();
    dev_free(d, Vtmp);
}
// One-sided (Hestenes) Jacobi on the ROWS of M (L x L), G accumulates the rotations from the identity: one workgroup, 32 lanes
// per row pair, the L / 2 disjoint pairs of a round-robin round in flight together; a round ends with one barrier.  M and G live in
// LDS when both fit (L <= 97: the launcher's 150 KiB test), else in global memory (L2-resident).  Built for accuracy, not speed: it only runs for fp64
// data whose wanted singular values fall below the Gram route's 10^-3.5 sigma_1 accuracy floor.
constexpr int HJ_THREADS = 1024, HJ_GROUP = 32;
template <bool INLDS>
__global__ __launch_bounds__(HJ_THREADS) void k_jacobi_svd_rows(double* __restrict__ A, int L, int64_t lda, double* __restrict__ Gg,
                                                                double* __restrict__ U, int64_t ldu, double* __restrict__ s_inv, int* __restrict__ nonconv) {
    extern __shared__ __attribute__((aligned(16))) double sm_hj[];   // [row norms (L) | flag | M, G when INLDS]: all dynamic
    const int tid = threadIdx.x, gl = tid & (HJ_GROUP - 1), grp = tid / HJ_GROUP, ngrp = HJ_THREADS / HJ_GROUP;
    const int ld = INLDS ? (L | 1) : L;
    double* s_nrm = sm_hj;
    volatile int* s_rotp = reinterpret_cast<volatile int*>(sm_hj + L);
#define s_rot (*s_rotp)
    double* M = INLDS ? sm_hj + L + 2 : A;
    double* G = INLDS ? sm_hj + L + 2 + (size_t)L * ld : Gg;
    const int64_t ldm = INLDS ? ld : lda;
    for (int e = tid; e < L * L; e += HJ_THREADS) {
        const int r = e / L, c = e - r * L;
        if (INLDS) M[r * ld + c] = A[(int64_t)r * lda + c];
        G[(size_t)r * ld + c] = r == c ? 1.0 : 0.0;
    }
    __syncthreads();
    const int n = (L + 1) & ~1, half = n >> 1;   // round-robin over n players (a dummy when L is odd)
    // a pair is orthogonal when |p . q| <= tol |p| |q|, tol = 4 eps sqrt(L): the rounding noise of an L-term fp64 dot product
    // (a fixed 1e-15 sat below it, so the flag rarely cleared and the kernel usually ran all 40 sweeps: ADVICE round 3)
    const double otol = 8.9e-16 * sqrt((double)L);
    bool converged = false;
    for (int sweep = 0; sweep < 40; ++sweep) {
        if (tid == 0) s_rot = 0;
        __syncthreads();
        for (int r = 0; r < n - 1; ++r) {
            for (int slot = grp; slot < half; slot += ngrp) {
                int p = slot == 0 ? n - 1 : (r + slot) % (n - 1);
                int q = (n - 1 - slot + r) % (n - 1);
                if (p > q) { const int t = p; p = q; q = t; }
                if (q >= L) continue;                      // the dummy sits out
                double* mp = M + (size_t)p * ldm;
                double* mq = M + (size_t)q * ldm;
                double al = 0, be = 0, ga = 0;
                for (int j = gl; j < L; j += HJ_GROUP) { const double a = mp[j], b = mq[j]; al += a * a; be += b * b; ga += a * b; }
                for (int off = HJ_GROUP / 2; off > 0; off >>= 1) {
                    al += __shfl_xor(al, off, 64); be += __shfl_xor(be, off, 64); ga += __shfl_xor(ga, off, 64);
                }
                if (!(fabs(ga) > otol * sqrt(al * be))) continue;   // (uniform over the 32 lanes of the pair)
                if (gl == 0) s_rot = 1;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                double* gp = G + (size_t)p * ld;
                double* gq = G + (size_t)q * ld;
                for (int j = gl; j < L; j += HJ_GROUP) {
                    const double a = mp[j], b = mq[j];
                    mp[j] = cs * a - sn * b; mq[j] = sn * a + cs * b;
                    const double u = gp[j], v = gq[j];
                    gp[j] = cs * u - sn * v; gq[j] = sn * u + cs * v;
                }
            }
            __syncthreads();
        }
        const int any = s_rot;
        __syncthreads();
        if (!any) { converged = true; break; }
    }
    if (nonconv && tid == 0 && !converged) *nonconv = 1;   // 40 sweeps were not enough: the caller keeps its other result
    // singular values = row norms; ascending order (ties: lower row first), 1 / s out
    for (int i = tid; i < L; i += HJ_THREADS) {
        double a = 0;
        for (int j = 0; j < L; ++j) { const double v = M[(size_t)i * ldm + j]; a += v * v; }
        s_nrm[i] = sqrt(a);
    }
    __syncthreads();
    for (int i = tid; i < L; i += HJ_THREADS) {
        const double mine = s_nrm[i];
        int rank = 0;
        for (int k2 = 0; k2 < L; ++k2) { const double o = s_nrm[k2]; rank += (o < mine || (o == mine && k2 < i)) ? 1 : 0; }
        s_inv[rank] = mine > 0.0 ? 1.0 / mine : 0.0;
        for (int j = 0; j < L; ++j) U[(int64_t)j * ldu + rank] = G[(size_t)i * ld + j];
    }
#undef s_rot
}
void op_jacobi_svd_rows(Dev* d, double* A, int64_t L, int64_t lda, double* U, int64_t ldu, double* s_inv, int* nonconv) {
    if (L == 0) return;
    if (L > 1024) throw std::runtime_error("jacobi_svd_rows: order above 1024");
    const size_t lds = sizeof(double) * (L + 2 + 2 * (size_t)L * (L | 1));
    if (lds <= 150 * 1024) {
        set_max_lds(d, reinterpret_cast<const void*>(k_jacobi_svd_rows<true>));
        hipLaunchKernelGGL(k_jacobi_svd_rows<true>, dim3(1), dim3(HJ_THREADS), lds, d->stream, A, (int)L, lda, (double*)nullptr, U, ldu, s_inv, nonconv);
        launch_check();
        return;
    }
    double* G = (double*)dev_alloc(d, sizeof(double) * L * L);
    hipLaunchKernelGGL(k_jacobi_svd_rows<false>, dim3(1), dim3(HJ_THREADS), sizeof(double) * (L + 2), d->stream, A, (int)L, lda, G, U, ldu, s_inv, nonconv);
    launch_check();
    dev_free(d, G);
}
// ONE block: lane <-> column (row-major reads stay coalesced), the 16 waves split the rows and add through LDS in a fixed order;
// the largest squared residual, theta_0 and the bad flag (a non-finite residual, or the eigen-solver's closeness verdict `flag`
// when given) are written directly -- no clear, no atomics
__global__ __launch_bounds__(1024) void k_ritz_residual(const double* __restrict__ CV, int64_t ldc, const double* __restrict__ Vr, int64_t ldv,
                                                        int64_t rows, int nc, const double* __restrict__ theta, const int* __restrict__ flag,
                                                        double* __restrict__ out3, double* __restrict__ w_out, const int* __restrict__ flag2) {
    __shared__ double red[16][65];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double worst = 0.0, bad = 0.0;   // (meaningful in wave 0)
    for (int jb = 0; jb < nc; jb += 64) {
        const int j = jb + lane;
        const bool on = j < nc;
        const double th = on ? theta[j] : 0.0;
        double s2 = 0;
        if (on)
            for (int64_t i = wv; i < rows; i += 16) { const double v = CV[i * ldc + j] - th * Vr[i * ldv + j]; s2 += v * v; }
        red[wv][lane] = s2;
        __syncthreads();
        if (wv == 0 && on) {
            double tot = 0;
            for (int w = 0; w < 16; ++w) tot += red[w][lane];
            if (!(tot < 1e300)) bad = 1.0;
            else worst = fmax(worst, tot);
            if (w_out) w_out[j] = th;   // the nc wanted Ritz values, delivered to the caller's array by the way
        }
        __syncthreads();
    }
    if (wv == 0) {
        for (int off = 32; off > 0; off >>= 1) { worst = fmax(worst, __shfl_down(worst, off, 64)); bad = fmax(bad, __shfl_down(bad, off, 64)); }
        if (lane == 0) {
            if (flag && *flag != 0) bad = 1.0;
            if (flag2 && *flag2 != 0) bad = 1.0;
            out3[0] = worst; out3[1] = nc > 0 ? theta[0] : 0.0; out3[2] = bad;
        }
    }
}
void op_ritz_residual(Dev* d, const double* CV, int64_t ldc, const double* Vr, int64_t ldv, int64_t rows, int64_t nc, const double* theta,
                      const int* flag, double* out3, double* w_out, const int* flag2) {
    hipLaunchKernelGGL(k_ritz_residual, dim3(1), dim3(1024), 0, d->stream, CV, ldc, Vr, ldv, rows, (int)nc, theta, flag, out3, w_out, flag2);
    launch_check();
}
// one block per column j: the eigenvector's sign is NORMALISED first (its first component of largest magnitude made positive).
// An eigen-solver returns v or -v at its whim -- the two-stage solver's choice can flip under a last-bit perturbation of the
// matrix, and a flipped whitening row sends the fixed-point iteration from the same w_init down another path (a sharded fit
// and the single-process fit of the same data then stop at different iteration counts).
__global__ __launch_bounds__(256) void k_whiten_k(const double* __restrict__ U, int64_t ldu, const double* __restrict__ lam, int64_t rows,
                                                  int64_t nc, int64_t ncp, double scale, double* __restrict__ KT, double* __restrict__ KTs) {
    __shared__ double rm[256];
    __shared__ int64_t ri[256];
    const int64_t j = blockIdx.x;
    if (j >= nc) {
        for (int64_t i = threadIdx.x; i < rows; i += 256) { KT[i * ncp + j] = 0.0; KTs[i * ncp + j] = 0.0; }
        return;
    }
    double best = -1.0;
    int64_t bi = 0;
    for (int64_t i = threadIdx.x; i < rows; i += 256) {   // ascending rows per thread: strict '>' keeps the first maximum
        const double a = fabs(U[i * ldu + j]);
        if (a > best) { best = a; bi = i; }
    }
    rm[threadIdx.x] = best; ri[threadIdx.x] = bi;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) {
            const double ob = rm[threadIdx.x + st];
            const int64_t oi = ri[threadIdx.x + st];
            if (ob > rm[threadIdx.x] || (ob == rm[threadIdx.x] && oi < ri[threadIdx.x])) { rm[threadIdx.x] = ob; ri[threadIdx.x] = oi; }
        }
        __syncthreads();
    }
    const double sgn = (rm[0] > 0.0 && U[ri[0] * ldu + j] < 0.0) ? -1.0 : 1.0;
    const double sg = sqrt(fmax(lam[j], 0.0));
    const double f = sg > 0.0 ? sgn / sg : 0.0;
    for (int64_t i = threadIdx.x; i < rows; i += 256) {
        const double v = U[i * ldu + j] * f;
        KT[i * ncp + j] = v;
        KTs[i * ncp + j] = v * scale;
    }
}
void op_whiten_k(Dev* d, const double* U, int64_t ldu, const double* lam, int64_t rows, int64_t nc, int64_t ncp, double scale,
                 double* KT, double* KTs) {
    if (rows * ncp == 0) return;
    hipLaunchKernelGGL(k_whiten_k, dim3((unsigned)ncp), dim3(256), 0, d->stream, U, ldu, lam, rows, nc, ncp, scale, KT, KTs);
    launch_check();
}
__global__ __launch_bounds__(256) void k_refill_zero_cols(double* __restrict__ Y, int64_t rows, int64_t ldy, const double* __restrict__ Src, int64_t lds) {
    __shared__ int nz;
    const int64_t j = blockIdx.x;
    if (threadIdx.x == 0) nz = 0;
    __syncthreads();
    bool any = false;
    for (int64_t i = threadIdx.x; i < rows; i += 256) any = any || (Y[i * ldy + j] != 0.0);
    if (any) nz = 1;
    __syncthreads();
    if (nz) return;
    for (int64_t i = threadIdx.x; i < rows; i += 256) Y[i * ldy + j] = Src[i * lds + j];
}
void op_refill_zero_cols(Dev* d, double* Y, int64_t rows, int64_t cols, int64_t ldy, const double* Src, int64_t lds) {
    if (rows == 0 || cols == 0) return;
    hipLaunchKernelGGL(k_refill_zero_cols, dim3((unsigned)cols), dim3(256), 0, d->stream, Y, rows, ldy, Src, lds);
    launch_check();
}
void op_dscal(Dev* d, double* x, int64_t count, double alpha) {
    if (!count) return;
    hipLaunchKernelGGL(k_dscal, dim3(cdiv(count, 256)), dim3(256), 0, d->stream, x, count, alpha);
    launch_check();
}
void op_daxpy(Dev* d, int64_t count, double alpha, const double* x, double* y) {
    if (!count) return;
    hipLaunchKernelGGL(k_daxpy, dim3(cdiv(count, 256)), dim3(256), 0, d->stream, count, alpha, x, y);
    launch_check();
}
void op_dvec(Dev* d, int mode, const double* x, double* y, int64_t count, double thr) {
    if (!count) return;
    hipLaunchKernelGGL(k_dvec, dim3(cdiv(count, 256)), dim3(256), 0, d->stream, mode, x, y, count, thr);
    launch_check();
}
void op_dscale_cols(Dev* d, double* A, int64_t M, int64_t N, int64_t lda, const double* s) {
    if (M * N == 0) return;
    hipLaunchKernelGGL(k_dscale_cols, dim3(cdiv(M * N, 256)), dim3(256), 0, d->stream, A, M, N, lda, s);
    launch_check();
}
void op_cvt_from_f64(Dev* d, int dt, void* dst, const double* src, int64_t count) {
    if (!count) return;
    DISPATCH_T(dt, hipLaunchKernelGGL(k_cvt_from_f64<T>, dim3(cdiv(count, 256)), dim3(256), 0, d->stream, (T*)dst, src, count));
    launch_check();
}
void op_pad_to_f64(Dev* d, int dt, double* dst, int64_t rows_p, int64_t cols_p, const void* src, int64_t rows, int64_t cols, int64_t lds,
                   double* zero_ptr, int64_t zero_count) {
    if (rows_p * cols_p == 0 && zero_count == 0) return;
    DISPATCH_T(dt, hipLaunchKernelGGL(k_pad_to_f64<T>, dim3(cdiv(std::max(rows_p * cols_p, zero_count), 256)), dim3(256), 0, d->stream, dst,
                                      rows_p, cols_p, (const T*)src, rows, cols, lds, zero_ptr, zero_count));
    launch_check();
}
void op_cvt_to_f64(Dev* d, int dt, double* dst, const void* src, int64_t count) {
    if (!count) return;
    DISPATCH_T(dt, hipLaunchKernelGGL(k_cvt_to_f64<T>, dim3(cdiv(count, 256)), dim3(256), 0, d->stream, dst, (const T*)src, count));
    launch_check();
}


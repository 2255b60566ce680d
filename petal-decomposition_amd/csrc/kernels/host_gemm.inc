// host_gemm.inc -- part of the ONE translation unit hip_ops.hip (textually included there, inside namespace petal): host-side launchers: packing, column scans, the X-streaming GEMM kernels.
// ================================================================================================
// host-side launchers
// ================================================================================================
#define DISPATCH_T(dt, ...)                              \
    do {                                                 \
        if ((dt) == F64) { using T = double; __VA_ARGS__; } \
        else { using T = float; __VA_ARGS__; }           \
    } while (0)

void op_pack_strided(Dev* d, int dt, const void* src, int64_t n, int64_t dd, int64_t rs, int64_t cs, void* dst, int64_t ld,
                     int64_t dpad) {
    if (n == 0 || dpad == 0) return;
    const int64_t blocks = (n * dpad + 1023) / 1024;
    if (blocks < (int64_t(1) << 31)) {
        DISPATCH_T(dt, hipLaunchKernelGGL(k_pack_flat<T>, dim3((unsigned)blocks), dim3(256), 0, d->stream, (const T*)src, n, dd, rs, cs,
                                          (T*)dst, ld, dpad));
    } else {
        DISPATCH_T(dt, hipLaunchKernelGGL(k_pack_strided<T>, dim3((unsigned)n, cdiv(dpad, 256)), dim3(256), 0, d->stream,
                                          (const T*)src, n, dd, rs, cs, (T*)dst, ld, dpad));
    }
    launch_check();
}
void op_unpack_strided(Dev* d, int dt, const void* src, int64_t n, int64_t dd, int64_t ld, void* dst, int64_t rs, int64_t cs,
                       const double* scale) {
    if (n == 0 || dd == 0) return;
    const int64_t blocks = (n * dd + 1023) / 1024;
    if (blocks < (int64_t(1) << 31)) {
        DISPATCH_T(dt, hipLaunchKernelGGL(k_unpack_scaled<T>, dim3((unsigned)blocks), dim3(256), 0, d->stream, (const T*)src, n, dd, ld,
                                          (T*)dst, rs, cs, scale));
    } else {
        if (scale) op_scale_cols(d, dt, const_cast<void*>(src), n, dd, ld, scale);
        DISPATCH_T(dt, hipLaunchKernelGGL(k_unpack_strided<T>, dim3((unsigned)n, cdiv(dd, 256)), dim3(256), 0, d->stream,
                                          (const T*)src, n, dd, ld, (T*)dst, rs, cs));
    }
    launch_check();
}

// first stage of the column sums (a 16-byte-per-lane form measured the same: EXPERIMENTS.md round 4)
static void launch_colsum_parts(Dev* d, int dt, const void* X, int64_t n, int64_t dd, int64_t ldx, int64_t rows, int64_t nparts,
                                double* part, bool with_sq, double* part_lo = nullptr) {
    const dim3 grid((unsigned)nparts, cdiv(dd, 64));
    if (with_sq) {
        DISPATCH_T(dt, hipLaunchKernelGGL((k_colsum_part2<T, true>), grid, dim3(256), 0, d->stream, (const T*)X, n, dd, ldx, rows, part, part_lo));
    } else {
        DISPATCH_T(dt, hipLaunchKernelGGL((k_colsum_part2<T, false>), grid, dim3(256), 0, d->stream, (const T*)X, n, dd, ldx, rows, part, part_lo));
    }
    launch_check();
}
void op_colsum(Dev* d, int dt, const void* X, int64_t n, int64_t dd, int64_t ldx, double* out, bool with_sq) {
    if (dd == 0) return;
    const int64_t w = with_sq ? 2 * dd : dd;
    if (n == 0) { dev_memset(d, out, 0, sizeof(double) * w); return; }
    const int64_t rows = scan_rows_per_block(n, dd), nparts = cdiv(n, rows);
    double* part = (double*)dev_alloc(d, sizeof(double) * nparts * w);
    launch_colsum_parts(d, dt, X, n, dd, ldx, rows, nparts, part, with_sq);
    hipLaunchKernelGGL(k_sum_parts2<double>, dim3(cdiv(w, 32)), dim3(256), 0, d->stream, part, nparts, w, out, w, w, false);
    launch_check();
    dev_free(d, part);
}

void op_colmean(Dev* d, int dt, const void* X, int64_t n, int64_t dd, int64_t ldx, double n_total, double* mu64, void* muT, bool with_sq) {
    if (dd == 0) return;
    const int64_t w = with_sq ? 2 * dd : dd;
    if (n == 0) { dev_memset(d, mu64, 0, sizeof(double) * w); dev_memset(d, muT, 0, dtype_size(dt) * dd); return; }
    const int64_t rows = scan_rows_per_block(n, dd), nparts = cdiv(n, rows);
    // fp64 data: the sums as (high, low) pairs, the mean one rounding of the exact one (k_colsum_part2); fp32 data's fp64 sums are
    // rounded to fp32 once anyway
    const bool pairs = dt == F64;
    double* part = (double*)dev_alloc(d, sizeof(double) * nparts * w * (pairs ? 2 : 1));
    double* part_lo = pairs ? part + nparts * w : nullptr;
    {
        TagScope ts(d);   // (the pass over X; bracketed when the caller tagged it)
        launch_colsum_parts(d, dt, X, n, dd, ldx, rows, nparts, part, with_sq, part_lo);
        ts.stop();
    }
    DISPATCH_T(dt, hipLaunchKernelGGL(k_colmean_final<T>, dim3(cdiv(w, 8)), dim3(256), 0, d->stream, part, part_lo, nparts, w, dd, 1.0 / n_total,
                                      n_total, mu64, (T*)muT));
    launch_check();
    dev_free(d, part);
}
void op_sigma_inv(Dev* d, const double* lam, double* sig, double* inv, int64_t count, double thr) {
    if (!count) return;
    hipLaunchKernelGGL(k_sigma_inv, dim3(cdiv(count, 256)), dim3(256), 0, d->stream, lam, sig, inv, count, thr);
    launch_check();
}
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// split-product (bf16x3, see k_xp3) kernels unless the ctx asks for the fp32-MFMA ones (petal_ctx_set_gemm_mode /
// PETAL_GEMM=fp32)
static bool gemm_split_product(const Dev* d) { return d->gemm_mode != 1; }   // (mode 2: the same kernels, three-plane operands only: algo.cpp)
// kernels that ask for more than 64 KB of dynamic LDS: the attribute is set once per device (ctx)
static void set_max_lds(Dev* d, const void* fn) {
    if (d->max_lds_set.count(fn)) return;
    HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    d->max_lds_set.insert(fn);
}
void op_scale_pad_cols(Dev* d, const double* V, int64_t ldv, const double* inv, int64_t rows, int64_t r, int64_t rp, double* P) {
    if (rows == 0 || rp == 0) return;
    hipLaunchKernelGGL(k_scale_pad_cols, dim3(cdiv(rows * rp, 256)), dim3(256), 0, d->stream, V, ldv, inv, rows, r, rp, P);
    launch_check();
}
void op_transpose_out(Dev* d, int dt, const double* V, int64_t ldv, int64_t dd, int64_t k, void* comp) {
    if (dd == 0 || k == 0) return;
    const dim3 grid(cdiv(dd, 32), cdiv(k, 32));
    if (dt == F32) hipLaunchKernelGGL(k_transpose_out<float>, grid, dim3(256), 0, d->stream, V, ldv, dd, k, (float*)comp);
    else hipLaunchKernelGGL(k_transpose_out<double>, grid, dim3(256), 0, d->stream, V, ldv, dd, k, (double*)comp);
    launch_check();
}
void op_components_out(Dev* d, int dt, const double* Bt, int64_t ldb, const double* Uh, int64_t ldu, const double* lam, double thr,
                       int64_t dd, int64_t L, int64_t k, void* comp) {
    if (k == 0 || dd == 0) return;
    const dim3 grid(cdiv(dd, 64), cdiv(k, 16));
    if (dt == F32)
        hipLaunchKernelGGL(k_components_out<float>, grid, dim3(256), 0, d->stream, Bt, ldb, Uh, ldu, lam, thr, dd, (int)L, k, (float*)comp);
    else
        hipLaunchKernelGGL(k_components_out<double>, grid, dim3(256), 0, d->stream, Bt, ldb, Uh, ldu, lam, thr, dd, (int)L, k, (double*)comp);
    launch_check();
}
static int num_cus(Dev* d) {
    if (!d->num_cu) { hipDeviceProp_t prop; HIP_CHECK(hipGetDeviceProperties(&prop, d->device)); d->num_cu = prop.multiProcessorCount; }
    return d->num_cu;
}

template <int RT, int NT>
static void launch_xp(Dev* d, const float* X, int64_t n, int K, int64_t ldx, const float* mu, const float* Ppk, int NTtot,
                      int nt0, int N, const float* bias, float* Z, int64_t ldz, double* ss_part, int blocks) {
    const bool center = mu != nullptr, ss = ss_part != nullptr;
#define XP_ARGS X, n, K, ldx, mu, Ppk, NTtot, nt0, N, bias, Z, ldz, ss_part
    if (center && ss) hipLaunchKernelGGL((k_xp_mfma<RT, NT, true, true>), dim3(blocks), dim3(256), 0, d->stream, XP_ARGS);
    else if (center) hipLaunchKernelGGL((k_xp_mfma<RT, NT, true, false>), dim3(blocks), dim3(256), 0, d->stream, XP_ARGS);
    else if (ss) hipLaunchKernelGGL((k_xp_mfma<RT, NT, false, true>), dim3(blocks), dim3(256), 0, d->stream, XP_ARGS);
    else hipLaunchKernelGGL((k_xp_mfma<RT, NT, false, false>), dim3(blocks), dim3(256), 0, d->stream, XP_ARGS);
#undef XP_ARGS
    launch_check();
}

// prod_A != nullptr: the small operand is the product prod_A (K x prod_M) . P (prod_M x N) (op_gemm_xp_prod); only the
// split-product path forms it inside its pack kernel, every other path gets it from a GEMM launch first
// (split-product path only) svd_flip's column scan of the product, from the kernel's accumulators: cols columns, results as op_col_absmax's
struct AbsmaxReq { int64_t cols, row_offset; double *absmax, *idx, *sign; };
static void gemm_xp_impl(Dev* d, int dt, const void* X, int64_t n, int64_t K, int64_t ldx, const void* mu, const double* P, int64_t N,
                         int64_t ldp, const void* bias, void* Z, int64_t ldz, double* sumsq, const double* prod_A, int64_t prod_M,
                         int64_t prod_lda, double* prod_out, int64_t prod_ldo, int prod_rt, const AbsmaxReq* am = nullptr,
                         bool p2_hint = false, bool steering = false);
void op_gemm_xp(Dev* d, int dt, const void* X, int64_t n, int64_t K, int64_t ldx, const void* mu, const double* P, int64_t N,
                int64_t ldp, const void* bias, void* Z, int64_t ldz, double* sumsq, int p_planes, bool steering) {
    gemm_xp_impl(d, dt, X, n, K, ldx, mu, P, N, ldp, bias, Z, ldz, sumsq, nullptr, 0, 0, nullptr, 0, false, nullptr, p_planes == 2, steering);
}
void op_gemm_xp_prod(Dev* d, int dt, const void* X, int64_t n, int64_t K, int64_t ldx, const void* mu, const double* A, int64_t M,
                     int64_t lda, const double* T, int64_t N, int64_t ldt, double* P_out, int64_t ldpo, void* Z, int64_t ldz) {
    const bool fused = dt == F32 && gemm_split_product(d) && n >= 64 && K % 16 == 0 && K > 0 && N % 16 == 0 && ldx % 4 == 0 &&
                       aligned16(X) && (!mu || aligned16(mu)) && ldz % 4 == 0 && aligned16(Z) && K < (1 << 24) && N < (1 << 24);
    if (fused) {
        double* tmpo = P_out ? nullptr : (double*)dev_alloc(d, sizeof(double) * K * N);
        gemm_xp_impl(d, dt, X, n, K, ldx, mu, T, N, ldt, nullptr, Z, ldz, nullptr, A, M, lda, P_out ? P_out : tmpo, P_out ? ldpo : N, false);
        if (tmpo) dev_free(d, tmpo);
        return;
    }
    double* tmp = nullptr;
    double* P = P_out;
    int64_t ldp = ldpo;
    if (!P) { tmp = (double*)dev_alloc(d, sizeof(double) * K * N); P = tmp; ldp = N; }
    op_dgemm(d, false, false, K, N, M, 1.0, A, lda, T, ldt, 0.0, P, ldp);
    op_gemm_xp(d, dt, X, n, K, ldx, mu, P, N, ldp, nullptr, Z, ldz, nullptr);
    if (tmp) dev_free(d, tmp);
}
void op_gemm_xp_prod_absmax(Dev* d, int dt, const void* X, int64_t n, int64_t K, int64_t ldx, const void* mu, const double* A, int64_t M,
                            int64_t lda, const double* T, int64_t N, int64_t ldt, double* P_out, int64_t ldpo, void* Z, int64_t ldz,
                            int64_t row_offset, double* absmax, double* idx, double* sign, bool store_product, bool a_rt) {
    const bool fused = dt == F32 && gemm_split_product(d) && n >= 64 && K % 16 == 0 && K > 0 && N % 16 == 0 && N > 0 && ldx % 4 == 0 &&
                       aligned16(X) && (!mu || aligned16(mu)) && ldz % 4 == 0 && aligned16(Z) && K < (1 << 24) && N < (1 << 24) &&
                       n < (int64_t(1) << 31) && P_out != nullptr;
    if (a_rt && !(M == K && M % 16 == 0 && M <= TRSM_MAXM && N % 16 == 0 && P_out != nullptr)) throw std::logic_error("op_gemm_xp_prod_absmax: RT-form operand of a shape the solve does not take");
    if (a_rt && !fused) {   // fp32-MFMA mode / fp64 data: P_out = R^-1 T by the same back substitution (no operand planes), then the plain product
        switch ((int)(M / 16)) {
#define PETAL_TRSML_CASE(NB)                                                                                                       \
    case NB:                                                                                                                       \
        hipLaunchKernelGGL((k_trsm_left_pack<NB>), dim3(cdiv(N, 16)), dim3(64), 0, d->stream, A, lda, T, ldt, P_out, ldpo, (bf16x8*)nullptr, 0); \
        break
            PETAL_TRSML_CASE(1); PETAL_TRSML_CASE(2); PETAL_TRSML_CASE(3); PETAL_TRSML_CASE(4); PETAL_TRSML_CASE(5);
            PETAL_TRSML_CASE(6); PETAL_TRSML_CASE(7); PETAL_TRSML_CASE(8); PETAL_TRSML_CASE(9);
#undef PETAL_TRSML_CASE
            default: throw std::logic_error("op_gemm_xp_prod_absmax: order out of range");
        }
        launch_check();
        op_gemm_xp_absmax(d, dt, X, n, K, ldx, mu, P_out, N, ldpo, Z, ldz, row_offset, absmax, idx, sign, store_product);
        return;
    }
    if (!fused) {
        op_gemm_xp_prod(d, dt, X, n, K, ldx, mu, A, M, lda, T, N, ldt, P_out, ldpo, Z, ldz);
        op_col_absmax(d, dt, Z, n, N, ldz, row_offset, absmax, idx, sign);
        return;
    }
    const AbsmaxReq am{N, row_offset, absmax, idx, sign};
    // (store_product = false: the caller only wants svd_flip's scan -- the product stays in the accumulators, 26 MB less to write at
    // configs[1])
    gemm_xp_impl(d, dt, X, n, K, ldx, mu, T, N, ldt, nullptr, store_product ? Z : nullptr, ldz, nullptr, A, M, lda, P_out, ldpo, a_rt ? 2 : 0, &am);
}
// Z = (X - mu) P with svd_flip's column scan (first row of largest |z| per column, its sign) taken from the product kernel's
// accumulators where that kernel runs -- no second pass over Z, and no store of Z at all when store_product is false.
void op_gemm_xp_absmax(Dev* d, int dt, const void* X, int64_t n, int64_t K, int64_t ldx, const void* mu, const double* P, int64_t N,
                       int64_t ldp, void* Z, int64_t ldz, int64_t row_offset, double* absmax, double* idx, double* sign, bool store_product) {
    const bool fused = dt == F32 && gemm_split_product(d) && n >= 64 && K % 16 == 0 && K > 0 && N % 16 == 0 && N > 0 && ldx % 4 == 0 &&
                       aligned16(X) && (!mu || aligned16(mu)) && ldz % 4 == 0 && aligned16(Z) && K < (1 << 24) && N < (1 << 24) &&
                       n < (int64_t(1) << 31);
    if (!fused) {
        op_gemm_xp(d, dt, X, n, K, ldx, mu, P, N, ldp, nullptr, Z, ldz, nullptr);
        op_col_absmax(d, dt, Z, n, N, ldz, row_offset, absmax, idx, sign);
        return;
    }
    const AbsmaxReq am{N, row_offset, absmax, idx, sign};
    gemm_xp_impl(d, dt, X, n, K, ldx, mu, P, N, ldp, nullptr, store_product ? Z : nullptr, ldz, nullptr, nullptr, 0, 0, nullptr, 0, false, &am);
}
static void gemm_xp_impl(Dev* d, int dt, const void* X, int64_t n, int64_t K, int64_t ldx, const void* mu, const double* P, int64_t N,
                         int64_t ldp, const void* bias, void* Z, int64_t ldz, double* sumsq, const double* prod_A, int64_t prod_M,
                         int64_t prod_lda, double* prod_out, int64_t prod_ldo, int prod_rt, const AbsmaxReq* am, bool p2_hint, bool steering) {
    if (n == 0 || N == 0) return;
    const bool mfma = dt == F32 && K % 16 == 0 && K > 0 && ldx % 4 == 0 && aligned16(X) && (!mu || aligned16(mu)) && n >= 64 &&
                      K < (1 << 24) && N < (1 << 24) && N % 16 == 0 && ldz % 4 == 0 && aligned16(Z) && (!bias || aligned16(bias));
    const bool mfma64 = dt == F64 && K % 8 == 0 && K > 0 && ldx % 2 == 0 && aligned16(X) && (!mu || aligned16(mu)) && n >= 64 &&
                        K < (1 << 24) && N < (1 << 24) && N % 16 == 0;
    if (am && !(mfma && gemm_split_product(d) && !sumsq)) throw std::logic_error("gemm_xp_impl: abs-max epilogue outside the split-product path");
    if (mfma64) {  // fp64 inputs: the fp64 matrix cores, 32-row wave tiles, column panels of <= 5 tiles
        const int NTtot = cdiv(N, 16);
        const int64_t total = (K / 8) * (int64_t)NTtot * 64;
        f64x2* Ppk = (f64x2*)dev_alloc(d, sizeof(f64x2) * total);
        hipLaunchKernelGGL(k_pack_p64, dim3(cdiv(total, 256)), dim3(256), 0, d->stream, P, K, N, ldp, Ppk, NTtot, total);
        launch_check();
        const int blocks = cdiv(n, 128);
        double* ssp = sumsq ? (double*)dev_alloc(d, sizeof(double) * blocks * 4) : nullptr;
        const double* Xd = (const double*)X; const double* mud = (const double*)mu; const double* bd = (const double*)bias; double* Zd = (double*)Z;
        TagScope ts(d);
        for (int nt0 = 0; nt0 < NTtot;) {
            const int rem = NTtot - nt0;
            const int w = rem >= 5 ? 5 : rem;
            double* sp = nt0 == 0 ? ssp : nullptr;
#define XP64_ARGS Xd, n, (int)K, ldx, mud, Ppk, NTtot, nt0, (int)N, bd, Zd, ldz, sp
#define XP64_LAUNCH(NTv)                                                                                                            \
            do {                                                                                                                    \
                if (mud && sp) hipLaunchKernelGGL((k_xp_f64<NTv, true, true>), dim3(blocks), dim3(256), 0, d->stream, XP64_ARGS);    \
                else if (mud) hipLaunchKernelGGL((k_xp_f64<NTv, true, false>), dim3(blocks), dim3(256), 0, d->stream, XP64_ARGS);    \
                else if (sp) hipLaunchKernelGGL((k_xp_f64<NTv, false, true>), dim3(blocks), dim3(256), 0, d->stream, XP64_ARGS);     \
                else hipLaunchKernelGGL((k_xp_f64<NTv, false, false>), dim3(blocks), dim3(256), 0, d->stream, XP64_ARGS);            \
            } while (0)
            switch (w) {
                case 5: XP64_LAUNCH(5); break;
                case 4: XP64_LAUNCH(4); break;
                case 3: XP64_LAUNCH(3); break;
                case 2: XP64_LAUNCH(2); break;
                default: XP64_LAUNCH(1); break;
            }
#undef XP64_LAUNCH
#undef XP64_ARGS
            launch_check();
            nt0 += w;
        }
        ts.stop();
        if (sumsq) {
            hipLaunchKernelGGL(k_add_scalar_parts, dim3(1), dim3(256), 0, d->stream, ssp, (int64_t)blocks * 4, sumsq);
            launch_check();
            dev_free(d, ssp);
        }
        dev_free(d, Ppk);
        return;
    }
    if (!mfma) {
        double* ssp = sumsq ? (double*)dev_alloc(d, sizeof(double) * n) : nullptr;
        TagScope ts(d);
        DISPATCH_T(dt, hipLaunchKernelGGL(k_xp_simple<T>, dim3((unsigned)n, cdiv(N, 64)), dim3(64), 0, d->stream, (const T*)X, n,
                                          K, ldx, (const T*)mu, P, N, ldp, (const T*)bias, (T*)Z, ldz, ssp));
        launch_check();
        ts.stop();
        if (sumsq) {
            hipLaunchKernelGGL(k_add_scalar_parts, dim3(1), dim3(256), 0, d->stream, ssp, n, sumsq);
            launch_check();
            dev_free(d, ssp);
        }
        return;
    }
    const int NTtot = cdiv(N, 16);
    if (gemm_split_product(d) && !sumsq) {
        // split-product (bf16x3) form: grid of 64-row wave tiles, column panels of <= 5 tiles
        const int64_t nch = (K + 31) / 32, total = nch * NTtot * 64;
        bf16x8* Ppk3 = (bf16x8*)dev_alloc(d, sizeof(bf16x8) * total * 3);
        // two-plane P (five piece products) where P is the re-based iterate of a power iteration: k_trsm_pack rounds it so
        // (development / test knobs: PETAL_NO_P2 keeps three planes everywhere, PETAL_NO_P2_ITERATE for the re-based iterate only,
        // PETAL_NO_P2_OMEGA for the sketch matrix only)
        const bool no_p2 = !opt_on(d, OPT_TWO_PLANE);
        const bool no_p2_it = no_p2 || !opt_on(d, OPT_TWO_PLANE_ITERATE), no_p2_om = no_p2 || !opt_on(d, OPT_TWO_PLANE_OMEGA);
        const bool p2 = p2_hint && ((prod_A && prod_rt && !no_p2_it) || (!prod_A && !no_p2_om)) && !am;
        const bool x2 = p2 && steering && opt_on(d, OPT_STEERING);   // (a steering pass: X on two planes too; the wide form only)
        if (prod_A) {
            // P = prod_A . P: the fp64 GEMM kernel writes the product (prod_out) AND its operand planes from its epilogue
            if (prod_rt == 2) {   // prod_A is R in RT form and the operand is R^-1 P: blocked back substitution, one wave per 16 columns
                switch ((int)(prod_M / 16)) {
#define PETAL_TRSML_CASE(NB)                                                                                                       \
    case NB:                                                                                                                       \
        hipLaunchKernelGGL((k_trsm_left_pack<NB>), dim3(cdiv(N, 16)), dim3(64), 0, d->stream, prod_A, prod_lda, P, ldp, prod_out, prod_ldo, Ppk3, NTtot); \
        break
                    PETAL_TRSML_CASE(1); PETAL_TRSML_CASE(2); PETAL_TRSML_CASE(3); PETAL_TRSML_CASE(4); PETAL_TRSML_CASE(5);
                    PETAL_TRSML_CASE(6); PETAL_TRSML_CASE(7); PETAL_TRSML_CASE(8); PETAL_TRSML_CASE(9);
#undef PETAL_TRSML_CASE
                    default: throw std::runtime_error("k_trsm_left_pack: order out of range");
                }
            } else if (prod_rt)   // P is R in RT form: blocked triangular solve instead of the product with the explicit inverse
                switch ((int)(N / 16)) {
#define PETAL_TRSM_CASE(NB)                                                                                                        \
    case NB:                                                                                                                       \
        if (p2) hipLaunchKernelGGL((k_trsm_pack<NB, true>), dim3(cdiv(K, 16)), dim3(64), trsm_lds_bytes(16 * NB), d->stream, prod_A, prod_lda, P,  \
                                   ldp, K, prod_out, prod_ldo, Ppk3, NTtot);                                                       \
        else hipLaunchKernelGGL((k_trsm_pack<NB, false>), dim3(cdiv(K, 16)), dim3(64), trsm_lds_bytes(16 * NB), d->stream, prod_A, prod_lda, P,  \
                           ldp, K, prod_out, prod_ldo, Ppk3, NTtot);                                                               \
        break
                    PETAL_TRSM_CASE(1); PETAL_TRSM_CASE(2); PETAL_TRSM_CASE(3); PETAL_TRSM_CASE(4); PETAL_TRSM_CASE(5);
                    PETAL_TRSM_CASE(6); PETAL_TRSM_CASE(7); PETAL_TRSM_CASE(8); PETAL_TRSM_CASE(9);
#undef PETAL_TRSM_CASE
                    default: throw std::runtime_error("k_trsm_pack: order out of range");
                }
            else
            hipLaunchKernelGGL(k_dgemm, dim3(cdiv(N, 16), cdiv(K, 16)), dim3(16, 16), 0, d->stream, false, false, K, N, prod_M, 1.0,
                               prod_A, prod_lda, P, ldp, 0.0, prod_out, prod_ldo, prod_M, (double*)nullptr, (const double*)nullptr,
                               Ppk3, NTtot);
        } else {
            hipLaunchKernelGGL(k_pack_p3, dim3(cdiv(total, 256)), dim3(256), 0, d->stream, P, K, N, ldp, Ppk3, NTtot, total);
        }
        launch_check();
        constexpr int RTv = PETAL_XP3_RT, DPv = PETAL_XP3_DEPTH;
        const float* Xf = (const float*)X; const float* muf = (const float*)mu; const float* bf = (const float*)bias; float* Zf = (float*)Z;
        static_assert(RTv == 4, "both workgroup shapes below cover 256 rows: one abs-max partial per 256 rows");
        const int64_t am_parts = cdiv(n, 256), am_ld = am ? am->cols : 0;
        double* am_part = am ? (double*)dev_alloc(d, sizeof(double) * 3 * am_parts * am_ld) : nullptr;
        TagScope ts(d);
        // Column panels: as few passes over X as 9-tile panels allow, the tiles spread evenly over them.  A panel of <= 5 tiles
        // runs on 64-row wave tiles (RT = 4), one of 6 .. 9 tiles on 32-row wave tiles (RT = 2: 72 accumulator registers at 9
        // tiles, eight waves per workgroup) -- every pass reads and splits X again, so l = 138 in one 9-tile pass instead of
        // 5 + 4 takes 0.41 instead of 0.55 ms at 250000 x 1024 (0.47 with four waves per workgroup, which stage the P chunk
        // twice as often; a one-wave-per-SIMD 64-row form had measured slower; at <= 5 tiles the 32-row form loses, 64 vs 54 us).
        const int npass = cdiv(NTtot, 9);
        for (int nt0 = 0, pass = 0; nt0 < NTtot; ++pass) {
            const int w = (NTtot - nt0 + (npass - pass) - 1) / (npass - pass);
            const size_t lds = sizeof(bf16x8) * 2 * w * 64 * (p2 ? 2 : 3) + sizeof(float) * 32 * nch;
#define XP3_LAUNCH8P(NTv, NPLv)                                                                                                           \
            do {                                                                                                                            \
                const int blocksw = cdiv(n, 256);                                                                                           \
                if (lds > 64 * 1024) set_max_lds(d, muf ? reinterpret_cast<const void*>(k_xp3<2, NTv, DPv, true, 8, PETAL_XP3_OCC, NPLv>) : reinterpret_cast<const void*>(k_xp3<2, NTv, DPv, false, 8, PETAL_XP3_OCC, NPLv>)); \
                if (muf) hipLaunchKernelGGL((k_xp3<2, NTv, DPv, true, 8, PETAL_XP3_OCC, NPLv>), dim3(blocksw), dim3(512), lds, d->stream, Xf, n, (int)K, ldx, muf, Ppk3, NTtot, nt0, (int)N, bf, Zf, ldz, am_part, am_ld); \
                else hipLaunchKernelGGL((k_xp3<2, NTv, DPv, false, 8, PETAL_XP3_OCC, NPLv>), dim3(blocksw), dim3(512), lds, d->stream, Xf, n, (int)K, ldx, muf, Ppk3, NTtot, nt0, (int)N, bf, Zf, ldz, am_part, am_ld); \
            } while (0)
#define XP3_LAUNCH8X(NTv)                                                                                                                 \
            do {                                                                                                                            \
                const int blocksw = cdiv(n, 256);                                                                                           \
                if (lds > 64 * 1024) set_max_lds(d, muf ? reinterpret_cast<const void*>(k_xp3<2, NTv, DPv, true, 8, PETAL_XP3_OCC, 2, true>) : reinterpret_cast<const void*>(k_xp3<2, NTv, DPv, false, 8, PETAL_XP3_OCC, 2, true>)); \
                if (muf) hipLaunchKernelGGL((k_xp3<2, NTv, DPv, true, 8, PETAL_XP3_OCC, 2, true>), dim3(blocksw), dim3(512), lds, d->stream, Xf, n, (int)K, ldx, muf, Ppk3, NTtot, nt0, (int)N, bf, Zf, ldz, am_part, am_ld); \
                else hipLaunchKernelGGL((k_xp3<2, NTv, DPv, false, 8, PETAL_XP3_OCC, 2, true>), dim3(blocksw), dim3(512), lds, d->stream, Xf, n, (int)K, ldx, muf, Ppk3, NTtot, nt0, (int)N, bf, Zf, ldz, am_part, am_ld); \
            } while (0)
#define XP3_LAUNCH8(NTv) do { if (p2 && x2) XP3_LAUNCH8X(NTv); else if (p2) XP3_LAUNCH8P(NTv, 2); else XP3_LAUNCH8P(NTv, 3); } while (0)
            if (w >= 6) {   // eight 32-row waves per workgroup: the P chunk is staged once per 256 rows, as in the 64-row form
                switch (w) {
                    case 9: XP3_LAUNCH8(9); break;
                    case 8: XP3_LAUNCH8(8); break;
                    case 7: XP3_LAUNCH8(7); break;
                    default: XP3_LAUNCH8(6); break;
                }
                launch_check();
                nt0 += w;
                continue;
            }
#define XP3_LAUNCHP(RTw, NTv, NPLv)                                                                                                        \
            do {                                                                                                                            \
                const int blocksw = cdiv(n, 64 * RTw);                                                                                      \
                if (lds > 64 * 1024) set_max_lds(d, muf ? reinterpret_cast<const void*>(k_xp3<RTw, NTv, DPv, true, 4, PETAL_XP3_OCC, NPLv>) : reinterpret_cast<const void*>(k_xp3<RTw, NTv, DPv, false, 4, PETAL_XP3_OCC, NPLv>)); \
                if (muf) hipLaunchKernelGGL((k_xp3<RTw, NTv, DPv, true, 4, PETAL_XP3_OCC, NPLv>), dim3(blocksw), dim3(256), lds, d->stream, Xf, n, (int)K, ldx, muf, Ppk3, NTtot, nt0, (int)N, bf, Zf, ldz, am_part, am_ld); \
                else hipLaunchKernelGGL((k_xp3<RTw, NTv, DPv, false, 4, PETAL_XP3_OCC, NPLv>), dim3(blocksw), dim3(256), lds, d->stream, Xf, n, (int)K, ldx, muf, Ppk3, NTtot, nt0, (int)N, bf, Zf, ldz, am_part, am_ld); \
            } while (0)
#define XP3_LAUNCH(RTw, NTv) do { if (p2) XP3_LAUNCHP(RTw, NTv, 2); else XP3_LAUNCHP(RTw, NTv, 3); } while (0)
            switch (w) {
                case 5: XP3_LAUNCH(RTv, 5); break;
                case 4: XP3_LAUNCH(RTv, 4); break;
                case 3: XP3_LAUNCH(RTv, 3); break;
                case 2: XP3_LAUNCH(RTv, 2); break;
                default: XP3_LAUNCH(RTv, 1); break;
            }
#undef XP3_LAUNCH
#undef XP3_LAUNCH8
#undef XP3_LAUNCHP
#undef XP3_LAUNCH8P
            launch_check();
            nt0 += w;
        }
        ts.stop();
        if (am) {
            hipLaunchKernelGGL(k_absmax_final, dim3((unsigned)am->cols), dim3(64), 0, d->stream, am_part, am_part + am_parts * am_ld,
                               am_part + 2 * am_parts * am_ld, am_parts, am_ld, am->row_offset, am->absmax, am->idx, am->sign);
            launch_check();
            dev_free(d, am_part);
        }
        dev_free(d, Ppk3);
        return;
    }
    float* Ppk = (float*)dev_alloc(d, sizeof(float) * (K / 16) * NTtot * 64 * 4);
    {
        const int64_t total = (K / 16) * (int64_t)NTtot * 64;
        hipLaunchKernelGGL(k_pack_p, dim3(cdiv(total, 256)), dim3(256), 0, d->stream, P, K, N, ldp, Ppk, NTtot);
        launch_check();
    }
    constexpr bool use_classic = false, force_pers = false;
    const int num_cu = num_cus(d);
    // Form selection (measured, MI355X): with fewer than two 64-row tiles per wave slot the grid form leaves SIMDs
    // a whole 64-row tile apart (100000 x 512: 74 TFLOP/s) and the balanced persistent form wins (84); with many tiles
    // per slot the hardware dispatcher balances the grid form dynamically and it is the faster one (1e6 x 512: 95 vs 76).
    const bool small = (n + 63) / 64 < (int64_t)num_cu * 8 * 2;
    if (!use_classic && (small || force_pers)) {
        // persistent form: one 512-thread workgroup per CU, balanced ranges of 16-row tiles, column panels of <= 5 tiles
        const int64_t ntiles16 = (n + 15) / 16;
        const int blocks = (int)std::min<int64_t>(num_cu, (ntiles16 + 7) / 8);
        double* ssp = sumsq ? (double*)dev_alloc(d, sizeof(double) * blocks * 8) : nullptr;
        TagScope ts(d);
        for (int nt0 = 0; nt0 < NTtot;) {
            const int rem = NTtot - nt0;
            const int w = rem >= 5 ? 5 : rem;
            double* sp = nt0 == 0 ? ssp : nullptr;
            const float* Xf = (const float*)X; const float* muf = (const float*)mu; const float* bf = (const float*)bias; float* Zf = (float*)Z;
            const bool center = muf != nullptr, ss = sp != nullptr;
#define XPP_ARGS Xf, n, (int)K, ldx, muf, Ppk, NTtot, nt0, (int)N, bf, Zf, ldz, sp, ntiles16
#define XPP_LAUNCH(NTv)                                                                                                      \
            do {                                                                                                             \
                if (center && ss) hipLaunchKernelGGL((k_xp_pers<NTv, true, true>), dim3(blocks), dim3(512), 0, d->stream, XPP_ARGS);   \
                else if (center) hipLaunchKernelGGL((k_xp_pers<NTv, true, false>), dim3(blocks), dim3(512), 0, d->stream, XPP_ARGS);   \
                else if (ss) hipLaunchKernelGGL((k_xp_pers<NTv, false, true>), dim3(blocks), dim3(512), 0, d->stream, XPP_ARGS);       \
                else hipLaunchKernelGGL((k_xp_pers<NTv, false, false>), dim3(blocks), dim3(512), 0, d->stream, XPP_ARGS);              \
            } while (0)
            switch (w) {
                case 5: XPP_LAUNCH(5); break;
                case 4: XPP_LAUNCH(4); break;
                case 3: XPP_LAUNCH(3); break;
                case 2: XPP_LAUNCH(2); break;
                default: XPP_LAUNCH(1); break;
            }
#undef XPP_LAUNCH
#undef XPP_ARGS
            launch_check();
            nt0 += w;
        }
        ts.stop();
        if (sumsq) {
            hipLaunchKernelGGL(k_add_scalar_parts, dim3(1), dim3(256), 0, d->stream, ssp, (int64_t)blocks * 8, sumsq);
            launch_check();
            dev_free(d, ssp);
        }
        dev_free(d, Ppk);
        return;
    }
    {
        // classic form: 64-row wave tiles, two waves per SIMD, column panels of <= 5 tiles
        const int blocks = cdiv(n, 256);
        double* ssp = sumsq ? (double*)dev_alloc(d, sizeof(double) * blocks * 4) : nullptr;
        TagScope ts(d);
        for (int nt0 = 0; nt0 < NTtot;) {
            const int rem = NTtot - nt0;
            const int w = rem >= 5 ? 5 : rem;
            double* sp = nt0 == 0 ? ssp : nullptr;
            const float* Xf = (const float*)X; const float* muf = (const float*)mu; const float* bf = (const float*)bias; float* Zf = (float*)Z;
            switch (w) {
                case 5: launch_xp<4, 5>(d, Xf, n, (int)K, ldx, muf, Ppk, NTtot, nt0, (int)N, bf, Zf, ldz, sp, blocks); break;
                case 4: launch_xp<4, 4>(d, Xf, n, (int)K, ldx, muf, Ppk, NTtot, nt0, (int)N, bf, Zf, ldz, sp, blocks); break;
                case 3: launch_xp<4, 3>(d, Xf, n, (int)K, ldx, muf, Ppk, NTtot, nt0, (int)N, bf, Zf, ldz, sp, blocks); break;
                case 2: launch_xp<4, 2>(d, Xf, n, (int)K, ldx, muf, Ppk, NTtot, nt0, (int)N, bf, Zf, ldz, sp, blocks); break;
                default: launch_xp<4, 1>(d, Xf, n, (int)K, ldx, muf, Ppk, NTtot, nt0, (int)N, bf, Zf, ldz, sp, blocks); break;
            }
            nt0 += w;
        }
        ts.stop();
        if (sumsq) {
            hipLaunchKernelGGL(k_add_scalar_parts, dim3(1), dim3(256), 0, d->stream, ssp, (int64_t)blocks * 4, sumsq);
            launch_check();
            dev_free(d, ssp);
        }
        dev_free(d, Ppk);
        return;
    }
}

// Row scores from the product kernels' accumulators (k_gemm_scores.inc); dispatched like gemm_xp_impl.  Column panels are launched in
// order on the one stream and each updates the per-row state st: a fixed order, no atomics.
void op_gemm_xp_scores(Dev* d, int dt, const void* X, int64_t n, int64_t K, int64_t ldx, const void* mu, const double* P, int64_t N,
                       int64_t ldp, const void* wts, void* Z, int64_t ldz, void* st, int64_t ldst) {
    if (n == 0) return;
    const bool mfma = dt == F32 && K % 16 == 0 && K > 0 && ldx % 4 == 0 && aligned16(X) && (!mu || aligned16(mu)) && n >= 64 &&
                      K < (1 << 24) && N < (1 << 24) && N % 16 == 0 && N > 0 && ldz % 4 == 0 && aligned16(Z) && (!wts || aligned16(wts));
    const bool mfma64 = dt == F64 && K % 8 == 0 && K > 0 && ldx % 2 == 0 && aligned16(X) && (!mu || aligned16(mu)) && n >= 64 &&
                        K < (1 << 24) && N < (1 << 24) && N % 16 == 0 && N > 0;
    const int NTtot = cdiv(N, 16);
    const int npass = cdiv(NTtot, 5);   // panels of <= 5 tiles, the tiles spread evenly over them
    TagScope ts(d);   // (the product launches, bracketed when the caller tagged them: as gemm_xp_impl)
    if (mfma64) {
        const int64_t total = (K / 8) * (int64_t)NTtot * 64;
        f64x2* Ppk = (f64x2*)dev_alloc(d, sizeof(f64x2) * total);
        hipLaunchKernelGGL(k_pack_p64, dim3(cdiv(total, 256)), dim3(256), 0, d->stream, P, K, N, ldp, Ppk, NTtot, total);
        launch_check();
        const int blocks = cdiv(n, 128);
        for (int nt0 = 0, pass = 0; nt0 < NTtot; ++pass) {
            const int w = (NTtot - nt0 + (npass - pass) - 1) / (npass - pass);
#define XPS_LAUNCH(NTv)                                                                                                                   \
            do {                                                                                                                            \
                if (mu) hipLaunchKernelGGL((k_xp_f64s<NTv, true>), dim3(blocks), dim3(256), 0, d->stream, (const double*)X, n, (int)K, ldx, (const double*)mu, Ppk, NTtot, nt0, (int)N, (double*)Z, ldz, (const double*)wts, (double*)st, ldst); \
                else hipLaunchKernelGGL((k_xp_f64s<NTv, false>), dim3(blocks), dim3(256), 0, d->stream, (const double*)X, n, (int)K, ldx, (const double*)mu, Ppk, NTtot, nt0, (int)N, (double*)Z, ldz, (const double*)wts, (double*)st, ldst); \
            } while (0)
            switch (w) {
                case 5: XPS_LAUNCH(5); break;
                case 4: XPS_LAUNCH(4); break;
                case 3: XPS_LAUNCH(3); break;
                case 2: XPS_LAUNCH(2); break;
                default: XPS_LAUNCH(1); break;
            }
#undef XPS_LAUNCH
            launch_check();
            nt0 += w;
        }
        ts.stop();
        dev_free(d, Ppk);
        return;
    }
    if (!mfma) {
        DISPATCH_T(dt, hipLaunchKernelGGL(k_xp_simple_s<T>, dim3((unsigned)n), dim3(64), 0, d->stream, (const T*)X, n, K, ldx, (const T*)mu, P, N,
                                          ldp, (T*)Z, ldz, (const T*)wts, (T*)st, ldst));
        launch_check();
        ts.stop();
        return;
    }
    const float* Xf = (const float*)X; const float* muf = (const float*)mu; const float* wf = (const float*)wts;
    float* Zf = (float*)Z; float* stf = (float*)st;
    const int blocks = cdiv(n, 256);
    if (gemm_split_product(d)) {   // (three-plane operands in every mode: these scores are results, not steering)
        const int64_t nch = (K + 31) / 32, total = nch * NTtot * 64;
        bf16x8* Ppk3 = (bf16x8*)dev_alloc(d, sizeof(bf16x8) * total * 3);
        hipLaunchKernelGGL(k_pack_p3, dim3(cdiv(total, 256)), dim3(256), 0, d->stream, P, K, N, ldp, Ppk3, NTtot, total);
        launch_check();
        for (int nt0 = 0, pass = 0; nt0 < NTtot; ++pass) {
            const int w = (NTtot - nt0 + (npass - pass) - 1) / (npass - pass);
            const size_t lds = sizeof(bf16x8) * 2 * w * 64 * 3 + sizeof(float) * 32 * nch;
#define XPS_LAUNCH(NTv)                                                                                                                   \
            do {                                                                                                                            \
                if (lds > 64 * 1024) set_max_lds(d, muf ? reinterpret_cast<const void*>(k_xp3s<NTv, true>) : reinterpret_cast<const void*>(k_xp3s<NTv, false>)); \
                if (muf) hipLaunchKernelGGL((k_xp3s<NTv, true>), dim3(blocks), dim3(256), lds, d->stream, Xf, n, (int)K, ldx, muf, Ppk3, NTtot, nt0, (int)N, Zf, ldz, wf, stf, ldst); \
                else hipLaunchKernelGGL((k_xp3s<NTv, false>), dim3(blocks), dim3(256), lds, d->stream, Xf, n, (int)K, ldx, muf, Ppk3, NTtot, nt0, (int)N, Zf, ldz, wf, stf, ldst); \
            } while (0)
            switch (w) {
                case 5: XPS_LAUNCH(5); break;
                case 4: XPS_LAUNCH(4); break;
                case 3: XPS_LAUNCH(3); break;
                case 2: XPS_LAUNCH(2); break;
                default: XPS_LAUNCH(1); break;
            }
#undef XPS_LAUNCH
            launch_check();
            nt0 += w;
        }
        ts.stop();
        dev_free(d, Ppk3);
        return;
    }
    float* Ppk = (float*)dev_alloc(d, sizeof(float) * (K / 16) * NTtot * 64 * 4);
    hipLaunchKernelGGL(k_pack_p, dim3(cdiv((K / 16) * (int64_t)NTtot * 64, 256)), dim3(256), 0, d->stream, P, K, N, ldp, Ppk, NTtot);
    launch_check();
    // Panels of <= 4 tiles (k_xp_mfma_s), spread evenly when centring.  Without centring a 3-tile panel is not launched: that form takes
    // 194 registers, two waves per SIMD where k_xp_mfma<4, 3, false, false> runs three -- the panels are then 4, 2 and 1 tiles wide.
    const int npass4 = cdiv(NTtot, 4);
    for (int nt0 = 0, pass = 0; nt0 < NTtot; ++pass) {
        const int rem = NTtot - nt0;
        const int w = muf ? (rem + (npass4 - pass) - 1) / (npass4 - pass) : (rem >= 4 ? 4 : rem >= 2 ? 2 : 1);
#define XPS_LAUNCH(NTv)                                                                                                                   \
        do {                                                                                                                                \
            if (muf) hipLaunchKernelGGL((k_xp_mfma_s<NTv, true>), dim3(blocks), dim3(256), 0, d->stream, Xf, n, (int)K, ldx, muf, Ppk, NTtot, nt0, (int)N, Zf, ldz, wf, stf, ldst); \
            else hipLaunchKernelGGL((k_xp_mfma_s<NTv, false>), dim3(blocks), dim3(256), 0, d->stream, Xf, n, (int)K, ldx, muf, Ppk, NTtot, nt0, (int)N, Zf, ldz, wf, stf, ldst); \
        } while (0)
        switch (w) {
            case 4: XPS_LAUNCH(4); break;
            case 3: hipLaunchKernelGGL((k_xp_mfma_s<3, true>), dim3(blocks), dim3(256), 0, d->stream, Xf, n, (int)K, ldx, muf, Ppk, NTtot, nt0, (int)N, Zf, ldz, wf, stf, ldst); break;   // (centring only, see above)
            case 2: XPS_LAUNCH(2); break;
            default: {   // one tile: 32-row wave tiles (k_xp_mfma_s)
                const int blocks2 = cdiv(n, 128);
                if (muf) hipLaunchKernelGGL((k_xp_mfma_s<1, true, 2>), dim3(blocks2), dim3(256), 0, d->stream, Xf, n, (int)K, ldx, muf, Ppk, NTtot, nt0, (int)N, Zf, ldz, wf, stf, ldst);
                else hipLaunchKernelGGL((k_xp_mfma_s<1, false, 2>), dim3(blocks2), dim3(256), 0, d->stream, Xf, n, (int)K, ldx, muf, Ppk, NTtot, nt0, (int)N, Zf, ldz, wf, stf, ldst);
                break;
            }
        }
#undef XPS_LAUNCH
        launch_check();
        nt0 += w;
    }
    ts.stop();
    dev_free(d, Ppk);
}

template <int NT>
static void launch_atb(Dev* d, const float* A, int64_t lda, int M, const float* muA, const float* B, int64_t ldb, int N,
                       int n0col, const float* muB, int64_t n, int64_t chunk, float* part, int nsplit) {
    const dim3 grid(8 * cdiv(M, 256), cdiv(nsplit, 8)), block(256);
#define ATB_ARGS A, lda, M, muA, B, ldb, N, n0col, muB, n, chunk, part, N
    if (muA && muB) hipLaunchKernelGGL((k_atb_mfma<NT, true, true>), grid, block, 0, d->stream, ATB_ARGS);
    else if (muA) hipLaunchKernelGGL((k_atb_mfma<NT, true, false>), grid, block, 0, d->stream, ATB_ARGS);
    else if (muB) hipLaunchKernelGGL((k_atb_mfma<NT, false, true>), grid, block, 0, d->stream, ATB_ARGS);
    else hipLaunchKernelGGL((k_atb_mfma<NT, false, false>), grid, block, 0, d->stream, ATB_ARGS);
#undef ATB_ARGS
    launch_check();
}

// live 32 x 64 wave tiles of a symmetric fp64-MFMA product (the enumeration of k_atb_f64 / k_gram_stream), four to a workgroup
static int gram64_sym_workgroups(int mslices, int npanels) {
    int tiles = 0;
    for (int a = 0; a < mslices; ++a) tiles += npanels - std::min(npanels, a / 2);
    return cdiv(tiles, 4);
}
// The row split of the fp64-MFMA products (k_atb_f64, k_gram_stream): the number of row chunks for `active` workgroups per chunk, and
// *chunk, the rows of each (a multiple of 16).
static int64_t gram64_row_split(int64_t n, int64_t M, int64_t N, int active, int64_t* chunk) {
    // row split: workgroups are dealt round-robin to the 256 CUs (up to three resident on each: the kernel's register
    // budget), so the launch takes ceil(active * ns / 256) / ns of the single-split time t1 -- one workgroup's four 32 x 64
    // tiles over all n rows, ~0.1 us a row (20000 x 256 in 15 splits: 119 us) -- plus what the ns fp64 slabs cost to write and
    // to combine (M N 16 bytes each at ~4 TB/s); pick the ns that minimises the sum.  (Round 4: a hard cap "slabs <= 40 % of
    // the input traffic" stood here and left 20000 x 256 on 75 workgroups: 119 us where 250 take half that.)
    const int64_t ns_max = std::min<int64_t>(128, std::max<int64_t>(1, n / 64));
    const double t1 = 0.1 * double(n), slab_us = double(M) * double(N) * 16.0 / 4.0e6;
    auto launch_us = [&](int64_t ns) { return t1 * double((active * ns + 255) / 256) / double(ns) * (active * ns <= 256 ? 1.25 : 1.0); };
    // (a single workgroup per CU leaves one wave per SIMD and the load latency exposed: measured 312 vs 265 us)
    int64_t nsplit = 1;
    double best = 1e30;
    for (int64_t ns = 1; ns <= ns_max; ++ns) {
        const double cost = launch_us(ns) + slab_us * double(ns);
        if (cost < best * 0.97) { best = cost; nsplit = ns; }
    }
    // among the splits that tie with the best one, the finest up to 96: whole "rounds" of workgroups cost the same in this
    // model, but a finer split keeps three workgroups on a CU and shortens the tail of the launch (500000 x 512: 2909 us at
    // 28 splits, 2863 at 42, 2837 at 56, 2757 at 84 -- against 0.4 us of k_sum_parts2 per extra slab) -- while the slabs stay
    // small change (3 % of the launch)
    {
        const double base = launch_us(nsplit);
        for (int64_t ns = nsplit + 1; ns <= std::min<int64_t>(ns_max, 96); ++ns)
            if (launch_us(ns) <= base * 1.005 && slab_us * double(ns) <= 0.03 * base) nsplit = ns;
    }
    *chunk = ((n + nsplit - 1) / nsplit + 15) / 16 * 16;
    return (n + *chunk - 1) / *chunk;
}

void op_gemm_atb(Dev* d, int dt, const void* A, int64_t lda, int64_t M, const void* muA, const void* B, int64_t ldb, int64_t N,
                 const void* muB, int64_t n, double* C, int64_t ldc, bool precise, bool steering) {
    if (M == 0 || N == 0) return;
    const bool p4 = steering && !precise && opt_on(d, OPT_STEERING);   // (a steering pass: both operands on two planes; the wide form only)
    if (n == 0) { HIP_CHECK(hipMemset2DAsync(C, ldc * sizeof(double), 0, N * sizeof(double), M, d->stream)); return; }
    const bool mfma = !precise && dt == F32 && M % 16 == 0 && N % 16 == 0 && lda % 4 == 0 && ldb % 4 == 0 && aligned16(A) && aligned16(B) &&
                      (!muA || aligned16(muA)) && (!muB || aligned16(muB)) && n >= 64 && M < (1 << 24) && N < (1 << 24);
    // fp64 matrix cores: the precise Gram of fp32 data, and every product of fp64 data (8-byte elements: rows 16-B aligned
    // with an even leading dimension)
    const bool mfma64 = ((precise && dt == F32 && lda % 4 == 0 && ldb % 4 == 0) || (dt == F64 && lda % 2 == 0 && ldb % 2 == 0)) &&
                        M % 16 == 0 && N % 16 == 0 && aligned16(A) && aligned16(B) && (!muA || aligned16(muA)) &&
                        (!muB || aligned16(muB)) && n >= 64 && M < (1 << 24) && N < (1 << 24);
    if (mfma64) {
        const int sym = (A == B && muA == muB && lda == ldb && M == N) ? 1 : 0;  // Gram matrix: upper tiles only, then mirror
        const bool ne5 = !sym && N % 80 == 0;  // l = 74 -> 80 columns: one 5-tile panel instead of two 4-tile ones
        const int mslices = cdiv(M, 32), npanels = ne5 ? (int)(N / 80) : cdiv(N, 64);
        const int gx = cdiv(M, 128);
        int active = gx * npanels;  // workgroups per row chunk
        if (sym) active = gram64_sym_workgroups(mslices, npanels);
        int64_t chunk = 0;
        const int64_t nsplit = gram64_row_split(n, M, N, active, &chunk);
        (void)mslices;
        double* part = (double*)dev_alloc(d, sizeof(double) * nsplit * M * N);
        const dim3 grid(sym ? active : gx, sym ? 1 : npanels, (unsigned)nsplit), block(256);
        TagScope ts(d);
#define ATB64_LAUNCH(TT, NEv)                                                                                                     \
        do {                                                                                                                      \
            const TT* Af = (const TT*)A; const TT* Bf = (const TT*)B; const TT* ma = (const TT*)muA; const TT* mb = (const TT*)muB; \
            if (ma && mb) hipLaunchKernelGGL((k_atb_f64<TT, true, true, NEv>), grid, block, 0, d->stream, Af, lda, (int)M, ma, Bf, ldb, (int)N, mb, n, chunk, part, sym); \
            else if (ma) hipLaunchKernelGGL((k_atb_f64<TT, true, false, NEv>), grid, block, 0, d->stream, Af, lda, (int)M, ma, Bf, ldb, (int)N, mb, n, chunk, part, sym); \
            else if (mb) hipLaunchKernelGGL((k_atb_f64<TT, false, true, NEv>), grid, block, 0, d->stream, Af, lda, (int)M, ma, Bf, ldb, (int)N, mb, n, chunk, part, sym); \
            else hipLaunchKernelGGL((k_atb_f64<TT, false, false, NEv>), grid, block, 0, d->stream, Af, lda, (int)M, ma, Bf, ldb, (int)N, mb, n, chunk, part, sym); \
        } while (0)
        if (dt == F64) { if (ne5) ATB64_LAUNCH(double, 5); else ATB64_LAUNCH(double, 4); }
        else { if (ne5) ATB64_LAUNCH(float, 5); else ATB64_LAUNCH(float, 4); }
#undef ATB64_LAUNCH
        launch_check();
        ts.stop();
        hipLaunchKernelGGL(k_sum_parts2<double>, dim3(cdiv(M * N, 32)), dim3(256), 0, d->stream, part, nsplit, M * N, C, N, ldc, false);
        launch_check();
        if (sym) {
            hipLaunchKernelGGL(k_mirror_upper, dim3(cdiv(M * M, 256)), dim3(256), 0, d->stream, C, M, ldc);
            launch_check();
        }
        dev_free(d, part);
        return;
    }
    if (!mfma) {
        const int64_t nparts = cdiv(n, ATB_S_ROWS);
        double* part = (double*)dev_alloc(d, sizeof(double) * nparts * M * N);
        TagScope ts(d);
        DISPATCH_T(dt, hipLaunchKernelGGL(k_atb_simple<T>, dim3((unsigned)nparts, cdiv(N, 16), cdiv(M, 16)), dim3(16, 16), 0,
                                          d->stream, (const T*)A, lda, M, (const T*)muA, (const T*)B, ldb, N, (const T*)muB, n, part));
        launch_check();
        ts.stop();
        hipLaunchKernelGGL(k_sum_parts2<double>, dim3(cdiv(M * N, 32)), dim3(256), 0, d->stream, part, nparts, M * N, C, N, ldc, false);
        launch_check();
        dev_free(d, part);
        return;
    }
    // split the rows so that every SIMD gets one wave (fp32-MFMA kernel: MFMA-bound, 256 workgroups) or two (split-product
    // kernel: paced by loads in flight -- 512 workgroups = two per CU measured 67 vs 75 us at 100000 x 512)
    const int mslices = cdiv(M, 64);
    constexpr int waves_env = 0;
    const int num_cu2 = num_cus(d);
    // (at 100000 rows the extra 128 slabs cost k_sum_parts2 what the kernel gains: two per CU only for long row ranges)
    const int waves_target = waves_env > 0 ? waves_env : num_cu2 * ((gemm_split_product(d) && !muB && n >= 400000) ? 8 : 4);
    int64_t nsplit = std::max<int64_t>(1, waves_target / mslices);
    // A NARROW A (at most 128 columns) takes smaller workgroups -- four waves of 32 columns, two for 64 columns -- instead of eight
    // waves of which most would re-load and re-multiply the clamped last columns (1e6 x 64: 2.3 TB/s); more row chunks keep the
    // chip filled with them (their slabs are small)
    const int NTall = int(N / 16);
    const int narrow_wv = (gemm_split_product(d) && !muB)
                              ? ((M <= 64 && NTall <= 4) ? 2 : ((M <= 128 && NTall <= 8) ? 4 : 0)) : 0;
    nsplit = std::min<int64_t>(nsplit, narrow_wv ? 256 * (8 / narrow_wv) : 256);  // bounds the partial-slab traffic of narrow (Gram) products
    nsplit = std::min<int64_t>(nsplit, std::max<int64_t>(1, n / 64));
    const bool split3_mode = gemm_split_product(d) && !muB && n >= 32 * nsplit;
    const int64_t cq = split3_mode ? 32 : 16;  // rows per pipeline stage
    const int64_t n_main = split3_mode ? n / cq * cq : n, n_tail = n - n_main;  // split-product kernels: whole stages
    const int64_t chunk = ((n_main + nsplit - 1) / nsplit + cq - 1) / cq * cq;
    nsplit = (n_main + chunk - 1) / chunk;
    const int64_t nslab = nsplit;   // (the split-product kernels take the ragged rows along in their last row chunk)
    float* part = (float*)dev_alloc(d, sizeof(float) * nslab * M * N);
    const int NTtot = int(N / 16);
    TagScope ts(d);
    // split-product kernels: as few column panels (passes over A) as 9-tile panels allow, the tiles spread evenly; a panel of
    // 6 .. 9 tiles runs on waves that own 32 columns of A (two m-tiles, 8-B loads: 72 accumulator registers at 9 tiles)
    const int npass3 = cdiv(NTtot, 9);
    for (int nt0 = 0, pass = 0; nt0 < NTtot; ++pass) {
        const int rem = NTtot - nt0;
        const int w = split3_mode ? (rem + (npass3 - pass) - 1) / std::max(npass3 - pass, 1) : (rem >= 5 ? 5 : rem);
        const float* Af = (const float*)A; const float* Bf = (const float*)B;
        const float* ma = (const float*)muA; const float* mb = (const float*)muB;
        // 8-wave workgroups of 64-column waves (one B stage per 512 columns of A) only where the row split already puts two waves
        // on every SIMD (long row ranges); everywhere else, and for every panel of more than 5 tiles, 8 waves of 32 columns:
        // at 100000 x 512 that form takes 55.4 us where four 64-column waves took 57.4 (at 1e6 rows it is the slower one,
        // 0.544 vs 0.533 ms)
        const bool wv8 = M >= 512 && nsplit * mslices >= (int64_t)num_cu2 * 8;
        if (split3_mode && narrow_wv) {
            const dim3 grid(8 * cdiv(M, 32 * narrow_wv), (unsigned)cdiv(nsplit, 8)), block(64 * narrow_wv);
#define ATB3N_LAUNCH(NTv, WVv)                                                                                                        \
            do {                                                                                                                      \
                if (ma) hipLaunchKernelGGL((k_atb3<NTv, true, WVv, 2>), grid, block, 0, d->stream, Af, lda, (int)M, ma, Bf, ldb, (int)N, 16 * nt0, n_main, chunk, part, (int)N, (int)n_tail); \
                else hipLaunchKernelGGL((k_atb3<NTv, false, WVv, 2>), grid, block, 0, d->stream, Af, lda, (int)M, ma, Bf, ldb, (int)N, 16 * nt0, n_main, chunk, part, (int)N, (int)n_tail); \
            } while (0)
            if (narrow_wv == 2) {
                switch (w) {
                    case 4: ATB3N_LAUNCH(4, 2); break;
                    case 3: ATB3N_LAUNCH(3, 2); break;
                    case 2: ATB3N_LAUNCH(2, 2); break;
                    default: ATB3N_LAUNCH(1, 2); break;
                }
            } else {
                switch (w) {
                    case 8: ATB3N_LAUNCH(8, 4); break;
                    case 7: ATB3N_LAUNCH(7, 4); break;
                    case 6: ATB3N_LAUNCH(6, 4); break;
                    case 5: ATB3N_LAUNCH(5, 4); break;
                    case 4: ATB3N_LAUNCH(4, 4); break;
                    case 3: ATB3N_LAUNCH(3, 4); break;
                    case 2: ATB3N_LAUNCH(2, 4); break;
                    default: ATB3N_LAUNCH(1, 4); break;
                }
            }
#undef ATB3N_LAUNCH
            launch_check();
            nt0 += w;
            continue;
        }
        if (split3_mode && (w >= 6 || !wv8)) {
            const dim3 grid(8 * cdiv(M, 256), (unsigned)cdiv(nsplit, 8)), block(512);   // 8 waves x 32 columns per workgroup
#define ATB3W_LAUNCH(NTv)                                                                                                             \
            do {                                                                                                                      \
                if (p4 && ma) hipLaunchKernelGGL((k_atb3<NTv, true, 8, 2, true>), grid, block, 0, d->stream, Af, lda, (int)M, ma, Bf, ldb, (int)N, 16 * nt0, n_main, chunk, part, (int)N, (int)n_tail); \
                else if (p4) hipLaunchKernelGGL((k_atb3<NTv, false, 8, 2, true>), grid, block, 0, d->stream, Af, lda, (int)M, ma, Bf, ldb, (int)N, 16 * nt0, n_main, chunk, part, (int)N, (int)n_tail); \
                else if (ma) hipLaunchKernelGGL((k_atb3<NTv, true, 8, 2>), grid, block, 0, d->stream, Af, lda, (int)M, ma, Bf, ldb, (int)N, 16 * nt0, n_main, chunk, part, (int)N, (int)n_tail); \
                else hipLaunchKernelGGL((k_atb3<NTv, false, 8, 2>), grid, block, 0, d->stream, Af, lda, (int)M, ma, Bf, ldb, (int)N, 16 * nt0, n_main, chunk, part, (int)N, (int)n_tail); \
            } while (0)
            switch (w) {
                case 9: ATB3W_LAUNCH(9); break;
                case 8: ATB3W_LAUNCH(8); break;
                case 7: ATB3W_LAUNCH(7); break;
                case 6: ATB3W_LAUNCH(6); break;
                case 5: ATB3W_LAUNCH(5); break;
                case 4: ATB3W_LAUNCH(4); break;
                case 3: ATB3W_LAUNCH(3); break;
                case 2: ATB3W_LAUNCH(2); break;
                default: ATB3W_LAUNCH(1); break;
            }
#undef ATB3W_LAUNCH
            launch_check();
            nt0 += w;
            continue;
        }
        if (split3_mode) {
            const dim3 grid(8 * cdiv(M, 512), (unsigned)cdiv(nsplit, 8)), block(512);
#define ATB3_LAUNCH(NTv)                                                                                                              \
            do {                                                                                                                      \
                if (ma) hipLaunchKernelGGL((k_atb3<NTv, true, 8>), grid, block, 0, d->stream, Af, lda, (int)M, ma, Bf, ldb, (int)N, 16 * nt0, n_main, chunk, part, (int)N, (int)n_tail); \
                else hipLaunchKernelGGL((k_atb3<NTv, false, 8>), grid, block, 0, d->stream, Af, lda, (int)M, ma, Bf, ldb, (int)N, 16 * nt0, n_main, chunk, part, (int)N, (int)n_tail); \
            } while (0)
            switch (w) {
                case 5: ATB3_LAUNCH(5); break;
                case 4: ATB3_LAUNCH(4); break;
                case 3: ATB3_LAUNCH(3); break;
                case 2: ATB3_LAUNCH(2); break;
                default: ATB3_LAUNCH(1); break;
            }
#undef ATB3_LAUNCH
            launch_check();
        }
        if (split3_mode) {
            nt0 += w;
            continue;
        }
        switch (w) {
            case 5: launch_atb<5>(d, Af, lda, (int)M, ma, Bf, ldb, (int)N, 16 * nt0, mb, n, chunk, part, (int)nsplit); break;
            case 4: launch_atb<4>(d, Af, lda, (int)M, ma, Bf, ldb, (int)N, 16 * nt0, mb, n, chunk, part, (int)nsplit); break;
            case 3: launch_atb<3>(d, Af, lda, (int)M, ma, Bf, ldb, (int)N, 16 * nt0, mb, n, chunk, part, (int)nsplit); break;
            case 2: launch_atb<2>(d, Af, lda, (int)M, ma, Bf, ldb, (int)N, 16 * nt0, mb, n, chunk, part, (int)nsplit); break;
            default: launch_atb<1>(d, Af, lda, (int)M, ma, Bf, ldb, (int)N, 16 * nt0, mb, n, chunk, part, (int)nsplit); break;
        }
        nt0 += w;
    }
    ts.stop();
    if ((M * N) % 2 == 0 && N % 2 == 0)
        hipLaunchKernelGGL(k_sum_parts4, dim3(cdiv(M * N, 128)), dim3(256), 0, d->stream, part, nslab, M * N, C, N, ldc);
    else
        hipLaunchKernelGGL(k_sum_parts2<float>, dim3(cdiv(M * N, 32)), dim3(256), 0, d->stream, part, nslab, M * N, C, N, ldc, false);
    launch_check();
    dev_free(d, part);
}

__global__ void k_flip_key(const double* __restrict__ t, double* __restrict__ key, int64_t L, const int* __restrict__ flag) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j == L && flag) key[L] = verdict_code(flag);   // (the three verdict words' code: ops.h)
    if (j >= L) return;
    const double a = t[j] < 0 ? 0.0 : t[j];
    unsigned long long bits = (unsigned long long)__double_as_longlong(a);
    const double rw = t[L + j];
    const unsigned long long row = rw < (double)(1ll << 28) ? (unsigned long long)rw : (1ull << 28) - 1;
    const unsigned long long payload = ((((1ull << 28) - 1) - row) << 1) | (t[2 * L + j] < 0 ? 1ull : 0ull);
    bits = (bits & ~((1ull << 29) - 1)) | (t[j] < 0 ? 0ull : payload);
    key[j] = __longlong_as_double((long long)bits);
}
void op_flip_key(Dev* d, const double* triple, double* key, int64_t L, const int* flag) {
    if (L == 0 && !flag) return;
    hipLaunchKernelGGL(k_flip_key, dim3(cdiv(L + 1, 256)), dim3(256), 0, d->stream, triple, key, L, flag);
    launch_check();
}
// Was the two-plane (16-bit) rounding of the sketch matrix and of the re-based iterates harmless for THIS spectrum?  (ops.h)
__global__ __launch_bounds__(256) void k_tail_verdict(const double* __restrict__ lam, int L, int k, const double* __restrict__ mu_sq, int dp,
                                                       int d, double n_total, const double* __restrict__ tvp, double eps2, double thr,
                                                       int* __restrict__ flag2) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double s = 0;
    if (mu_sq) for (int j = tid; j < d; j += 256) s += fmax(0.0, mu_sq[dp + j] - n_total * mu_sq[j] * mu_sq[j]);
    red[tid] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) { if (tid < st) red[tid] += red[tid + st]; __syncthreads(); }
    const double tv = mu_sq ? red[0] : tvp[0];
    __syncthreads();
    s = 0;
    for (int j = tid; j < L; j += 256) s += fmax(lam[j], 0.0);
    red[tid] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) { if (tid < st) red[tid] += red[tid + st]; __syncthreads(); }
    const double tail = fmax(tv - red[0], 0.0);
    const double T = sqrt(fmax(lam[L - 1], 0.0) * tail / (double)d);
    int bad = 0;
    for (int j = tid; j < k && j < L; j += 256) {
        const double lj = lam[j];
        if (!(lj > 0.0)) continue;                       // (a sigma = 0 component of rank-deficient data: nothing to perturb)
        double gap = j + 1 < L ? lj - fmax(lam[j + 1], 0.0) : lj;
        if (j > 0) gap = fmin(gap, lam[j - 1] - lj);
        const double relgap = fmax(gap / lj, 1e-3);
        if (eps2 * T / lj / relgap > thr) bad = 1;
    }
    if (__syncthreads_or(bad) && tid == 0) flag2[1] = 1;
}
void op_tail_verdict(Dev* d, const double* lam, int64_t L, int64_t k, const double* mu_sq, int64_t dp, int64_t dd, double n_total,
                     const double* tv, double eps2, double thr, int* flag2) {
    if (L <= 0 || k <= 0) return;
    hipLaunchKernelGGL(k_tail_verdict, dim3(1), dim3(256), 0, d->stream, lam, (int)L, (int)k, mu_sq, (int)dp, (int)dd, n_total, tv, eps2, thr, flag2);
    launch_check();
}
void op_col_absmax(Dev* d, int dt, const void* U, int64_t n, int64_t L, int64_t ldu, int64_t row_offset, double* absmax,
                   double* idx, double* sign) {
    if (L == 0) return;
    const int64_t rows = scan_rows_per_block(n, L), nparts = std::max<int64_t>(1, cdiv(n, rows));
    double* part = (double*)dev_alloc(d, sizeof(double) * 3 * nparts * L);
    double *pm = part, *pi = part + nparts * L, *ps = part + 2 * nparts * L;
    if (n == 0) {
        std::vector<double> h(3 * L);
        for (int64_t j = 0; j < L; ++j) { h[j] = -1.0; h[L + j] = INFINITY; h[2 * L + j] = 1.0; }
        dev_h2d(d, absmax, h.data(), sizeof(double) * L);
        dev_h2d(d, idx, h.data() + L, sizeof(double) * L);
        dev_h2d(d, sign, h.data() + 2 * L, sizeof(double) * L);
        dev_free(d, part);
        return;
    }
    DISPATCH_T(dt, hipLaunchKernelGGL(k_absmax_part2<T>, dim3((unsigned)nparts, cdiv(L, 64)), dim3(256), 0, d->stream, (const T*)U,
                                      n, L, ldu, rows, pm, pi, ps));
    launch_check();
    hipLaunchKernelGGL(k_absmax_final, dim3((unsigned)L), dim3(64), 0, d->stream, pm, pi, ps, nparts, L, row_offset, absmax, idx, sign);
    launch_check();
    dev_free(d, part);
}

void op_scale_cols(Dev* d, int dt, void* A, int64_t n, int64_t L, int64_t lda, const double* s) {
    if (n == 0 || L == 0) return;
    DISPATCH_T(dt, hipLaunchKernelGGL(k_scale_cols<T>, dim3((unsigned)n, cdiv(L, 64)), dim3(64), 0, d->stream, (T*)A, n, L, lda, s));
    launch_check();
}
void op_logcosh_rows(Dev* d, int dt, const void* X, int64_t r, int64_t c, int64_t ldx, void* G, int64_t ldg, double* gp) {
    if (r == 0) return;
    DISPATCH_T(dt, hipLaunchKernelGGL(k_logcosh_rows<T>, dim3(cdiv(r, 64)), dim3(64), 0, d->stream, (const T*)X, r, c, ldx, (T*)G, ldg, gp));
    launch_check();
}


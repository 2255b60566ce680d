// host_small.inc -- part of the ONE translation unit hip_ops.hip (textually included there, inside namespace petal): host-side launchers: FastICA step / tail, fp64 small-matrix ops, re-basing.
// once per fixed-point loop: X1 is constant over its iterations, so its bf16 planes are made here (fp32 data, split-product modes,
// 32 or 64 padded components) and every op_ica_step of the loop reads them instead of splitting X1 twice per iteration
void op_ica_prepare(Dev* d, int dt, const void* X1T, int64_t n, int64_t nc, int64_t ld) {
    constexpr bool off = false;
    d->ica_x1pl_for = nullptr;
    const int NT = int((nc + 15) / 16);
    if (off || dt != F32 || !gemm_split_product(d) || (NT != 2 && NT != 4) || n < 256 || ld % 4 != 0 || ld < 16 * NT || !aligned16(X1T)) return;
    const int KCH = NT / 2;
    const int64_t nfrag = cdiv(n, 32) * 2 * KCH;
    const size_t need = sizeof(bf16x8) * (size_t)nfrag * 3 * 64;
    if (!d->ica_x1pl || d->ica_x1pl_bytes < need) {
        if (d->ica_x1pl) dev_free(d, d->ica_x1pl);
        d->ica_x1pl = dev_alloc(d, need);
        d->ica_x1pl_bytes = need;
    }
    if (KCH == 1) hipLaunchKernelGGL(k_ica_planes<1>, dim3((unsigned)cdiv(nfrag, 4)), dim3(256), 0, d->stream, (const float*)X1T, n, ld, 16 * NT, (bf16x8*)d->ica_x1pl, nfrag);
    else hipLaunchKernelGGL(k_ica_planes<2>, dim3((unsigned)cdiv(nfrag, 4)), dim3(256), 0, d->stream, (const float*)X1T, n, ld, 16 * NT, (bf16x8*)d->ica_x1pl, nfrag);
    launch_check();
    d->ica_x1pl_for = X1T; d->ica_x1pl_n = n; d->ica_x1pl_ld = ld;
}
// the kernel instantiation of a contrast other than logcosh (g: ICA_G_EXP or ICA_G_CUBE, checked by op_ica_step_g)
#define ICA_G_DISPATCH(g, CALL)                                          \
    do {                                                                 \
        if ((g) == ICA_G_EXP) { constexpr int Gv = ICA_G_EXP; CALL; }    \
        else { constexpr int Gv = ICA_G_CUBE; CALL; }                    \
    } while (0)
// one step of the loop with contrast g (ICA_G_LOGCOSH: the kernels the crate's logcosh has always run on)
static void ica_step_impl(Dev* d, int dt, const void* X1T, int64_t n, int64_t nc, int64_t ld, const double* W, double* GX_gp,
                          const int* state, const int g) {
    const int64_t cnt = nc * nc + nc;
    const bool planes_current = d->ica_wpk3_valid && d->ica_wpk3_for == W && d->ica_wpk3_nc == nc;
    d->ica_ortho_tol2 = dt == F32 ? 1e-14 : 1e-26;
    d->ica_wpk3_for = nullptr;  // (only the split-product path below asks the tail kernel to keep the planes current)
    if (n == 0) { dev_memset(d, GX_gp, 0, sizeof(double) * cnt); return; }
    const bool mfma = dt == F32 && nc <= 64 && ld % 4 == 0 && ld >= (nc + 15) / 16 * 16 && aligned16(X1T) && n >= 256;
    if (nc > 64) {
        // more than 64 components (the crate's default is min(n, d) of them, src/ica.rs:173): the step as it stands in the
        // reference -- S = X1^T W^T (ica.rs:332), g = tanh (ica.rs:388-396), G^T X1 (ica.rs:333) -- on the two X-streaming
        // GEMM kernels, with g' from the column sums of g^2.  Unfused: S makes one round trip through HBM.
        const int64_t ncp = (nc + 15) / 16 * 16;
        if (ld < ncp) throw std::runtime_error("ica_step: leading dimension below the padded component count");
        double* WT = (double*)dev_alloc(d, sizeof(double) * ncp * ncp);
        hipLaunchKernelGGL(k_transpose_pad, dim3(cdiv(ncp * ncp, 256)), dim3(256), 0, d->stream, W, nc, WT, ncp);
        launch_check();
        void* S = dev_alloc(d, dtype_size(dt) * (size_t)n * ncp);
        op_gemm_xp(d, dt, X1T, n, ncp, ld, nullptr, WT, ncp, ncp, nullptr, S, ncp, nullptr);
        const int saved_tag = d->tag;
        d->tag = TAG_NONE;  // (only the first product is bracketed as "the step kernel")
        if (g != ICA_G_LOGCOSH) {
            // n - sum g^2 is tanh's identity: here g' is summed explicitly, per 256-row block and then over the blocks in order
            const int64_t nparts = cdiv(n, 256);
            double* gp_part = (double*)dev_alloc(d, sizeof(double) * nparts * ncp);
            ICA_G_DISPATCH(g, DISPATCH_T(dt, hipLaunchKernelGGL((k_contrast_inplace<T, Gv>), dim3((unsigned)nparts), dim3(256), 0, d->stream, (T*)S, n, ncp, gp_part)));
            launch_check();
            double* GXp = (double*)dev_alloc(d, sizeof(double) * ncp * ncp);
            op_gemm_atb(d, dt, S, ncp, ncp, nullptr, X1T, ld, ncp, nullptr, n, GXp, ncp);
            hipLaunchKernelGGL(k_ica_big_out_g, dim3(cdiv(cnt, 256)), dim3(256), 0, d->stream, GXp, gp_part, nparts, nc, ncp, GX_gp, state);
            launch_check();
            d->tag = saved_tag;
            dev_free(d, GXp); dev_free(d, gp_part); dev_free(d, S); dev_free(d, WT);
            return;
        }
        DISPATCH_T(dt, hipLaunchKernelGGL(k_tanh_inplace<T>, dim3(cdiv((int64_t)n * ncp, 256)), dim3(256), 0, d->stream, (T*)S, (int64_t)n * ncp));
        launch_check();
        double* cs = (double*)dev_alloc(d, sizeof(double) * 2 * ncp);
        op_colsum(d, dt, S, n, ncp, ncp, cs, true);
        double* GXp = (double*)dev_alloc(d, sizeof(double) * ncp * ncp);
        op_gemm_atb(d, dt, S, ncp, ncp, nullptr, X1T, ld, ncp, nullptr, n, GXp, ncp);
        hipLaunchKernelGGL(k_ica_big_out, dim3(cdiv(cnt, 256)), dim3(256), 0, d->stream, GXp, cs + ncp, (double)n, nc, ncp, GX_gp, state);
        launch_check();
        d->tag = saved_tag;
        dev_free(d, GXp); dev_free(d, cs); dev_free(d, S); dev_free(d, WT);
        return;
    }
    if (!mfma) {
        const int64_t nparts = cdiv(n, 64);
        double* part = (double*)dev_alloc(d, sizeof(double) * nparts * cnt);
        TagScope ts(d);
        if (g == ICA_G_LOGCOSH) {
            DISPATCH_T(dt, hipLaunchKernelGGL(k_ica_simple<T>, dim3((unsigned)nparts), dim3(256), sizeof(double) * nc * 64, d->stream,
                                              (const T*)X1T, n, (int)nc, ld, W, part, state));
        } else {
            const size_t lds = 2 * sizeof(double) * nc * 64;   // g and g': 64 KB at 64 components
            ICA_G_DISPATCH(g, DISPATCH_T(dt, {
                if (lds >= 64 * 1024) set_max_lds(d, reinterpret_cast<const void*>(k_ica_simple_g<T, Gv>));
                hipLaunchKernelGGL((k_ica_simple_g<T, Gv>), dim3((unsigned)nparts), dim3(256), lds, d->stream, (const T*)X1T, n, (int)nc, ld, W, part, state);
            }));
        }
        launch_check();
        ts.stop();
        hipLaunchKernelGGL(k_sum_parts_state, dim3(cdiv(cnt, 256)), dim3(256), 0, d->stream, part, nparts, cnt, GX_gp, state);
        launch_check();
        dev_free(d, part);
        return;
    }
    const int NT = int((nc + 15) / 16), NCP = 16 * NT;
    const int64_t slab = (int64_t)NCP * NCP + NCP;
    if (gemm_split_product(d)) {
        const int KCH = (NCP + 31) / 32;
        const size_t need = sizeof(bf16x8) * KCH * NT * 192;
        if (!d->ica_wpk3 || d->ica_wpk3_bytes < need) {
            if (d->ica_wpk3) dev_free(d, d->ica_wpk3);
            d->ica_wpk3 = dev_alloc(d, need);
            d->ica_wpk3_bytes = need;
            d->ica_wpk3_valid = false;
        }
        bf16x8* Wpk3 = (bf16x8*)d->ica_wpk3;
        if (!planes_current) {
            hipLaunchKernelGGL(k_pack_w3, dim3(cdiv(KCH * NT * 64, 256)), dim3(256), 0, d->stream, W, (int)nc, Wpk3, NT, KCH);
            launch_check();
        }
        d->ica_wpk3_for = W; d->ica_wpk3_nc = nc; d->ica_wpk3_valid = false;  // valid again once the tail has refreshed them
        const int64_t nblk = (n + 31) / 32;
        int64_t waves = std::min<int64_t>(2048, nblk);
        const int64_t bpw = (nblk + waves - 1) / waves;
        waves = (nblk + bpw - 1) / bpw;
        const int blocks = cdiv(waves, 4);
        float* part = (float*)dev_alloc(d, sizeof(float) * blocks * slab);
        TagScope ts(d);
        const bool pre = d->ica_x1pl_for == X1T && d->ica_x1pl_n == n && d->ica_x1pl_ld == ld && (NT == 2 || NT == 4);
        if (g != ICA_G_LOGCOSH) {
#define ICA3G_LAUNCH(NTv) hipLaunchKernelGGL((k_ica3g<NTv, Gv>), dim3(blocks), dim3(256), 0, d->stream, (const float*)X1T, n, ld, Wpk3, bpw, part, state)
            if (pre) {
                if (NT == 2) ICA_G_DISPATCH(g, hipLaunchKernelGGL((k_ica3pg<2, Gv>), dim3(blocks), dim3(256), 0, d->stream, (const bf16x8*)d->ica_x1pl, n, Wpk3, bpw, part, state));
                else ICA_G_DISPATCH(g, hipLaunchKernelGGL((k_ica3pg<4, Gv>), dim3(blocks), dim3(256), 0, d->stream, (const bf16x8*)d->ica_x1pl, n, Wpk3, bpw, part, state));
            } else
            // (NT = 2 and 4 land here only when the step is called WITHOUT op_ica_prepare, which the op allows (ops.h) and ica_loop never
            // does: its conditions for those two are this path's own, so every fit and every ica_par takes k_ica3pg there, as the logcosh
            // step takes k_ica3p (EXPERIMENTS.md).  k_ica3g<2, *> and <4, *> are built and held to their register budgets, not launched
            // by any caller of the library today; what runs of k_ica3g is NT = 1 and 3.)
            switch (NT) {
                case 1: ICA_G_DISPATCH(g, ICA3G_LAUNCH(1)); break;
                case 2: ICA_G_DISPATCH(g, ICA3G_LAUNCH(2)); break;
                case 3: ICA_G_DISPATCH(g, ICA3G_LAUNCH(3)); break;
                default: ICA_G_DISPATCH(g, ICA3G_LAUNCH(4)); break;
            }
#undef ICA3G_LAUNCH
        } else if (pre) {
            if (NT == 2) hipLaunchKernelGGL(k_ica3p<2>, dim3(blocks), dim3(256), 0, d->stream, (const bf16x8*)d->ica_x1pl, n, Wpk3, bpw, part, state);
            else hipLaunchKernelGGL(k_ica3p<4>, dim3(blocks), dim3(256), 0, d->stream, (const bf16x8*)d->ica_x1pl, n, Wpk3, bpw, part, state);
        } else
        switch (NT) {
            case 1: hipLaunchKernelGGL(k_ica3<1>, dim3(blocks), dim3(256), 0, d->stream, (const float*)X1T, n, ld, Wpk3, bpw, part, state); break;
            case 2: hipLaunchKernelGGL(k_ica3<2>, dim3(blocks), dim3(256), 0, d->stream, (const float*)X1T, n, ld, Wpk3, bpw, part, state); break;
            case 3: hipLaunchKernelGGL(k_ica3<3>, dim3(blocks), dim3(256), 0, d->stream, (const float*)X1T, n, ld, Wpk3, bpw, part, state); break;
            default: hipLaunchKernelGGL(k_ica3<4>, dim3(blocks), dim3(256), 0, d->stream, (const float*)X1T, n, ld, Wpk3, bpw, part, state); break;
        }
        launch_check();
        ts.stop();
        hipLaunchKernelGGL(k_ica_reduce, dim3(cdiv(cnt, 32)), dim3(1024), 0, d->stream, part, (int64_t)blocks, NCP, (int)nc, GX_gp, state);
        launch_check();
        dev_free(d, part);
        return;
    }
    float* Wpk = (float*)dev_alloc(d, sizeof(float) * NT * NT * 64 * 4);
    hipLaunchKernelGGL(k_pack_w, dim3(cdiv(NT * NT * 64, 256)), dim3(256), 0, d->stream, W, (int)nc, Wpk, NT);
    launch_check();
    const int64_t tiles = (n + 15) / 16;
    int64_t waves = std::min<int64_t>(2048, tiles);
    const int64_t tpw = (tiles + waves - 1) / waves;
    waves = (tiles + tpw - 1) / tpw;
    const int blocks = cdiv(waves, 4);
    const int64_t nparts = (int64_t)blocks;  // one slab per workgroup
    float* part = (float*)dev_alloc(d, sizeof(float) * nparts * slab);
    TagScope ts(d);
    if (g != ICA_G_LOGCOSH) {
#define ICAMG_LAUNCH(NTv) hipLaunchKernelGGL((k_ica_mfma_g<NTv, Gv>), dim3(blocks), dim3(256), 0, d->stream, (const float*)X1T, n, ld, Wpk, tpw, part, state)
        switch (NT) {
            case 1: ICA_G_DISPATCH(g, ICAMG_LAUNCH(1)); break;
            case 2: ICA_G_DISPATCH(g, ICAMG_LAUNCH(2)); break;
            case 3: ICA_G_DISPATCH(g, ICAMG_LAUNCH(3)); break;
            default: ICA_G_DISPATCH(g, ICAMG_LAUNCH(4)); break;
        }
#undef ICAMG_LAUNCH
    } else
    switch (NT) {
        case 1: hipLaunchKernelGGL(k_ica_mfma<1>, dim3(blocks), dim3(256), 0, d->stream, (const float*)X1T, n, ld, Wpk, tpw, part, state); break;
        case 2: hipLaunchKernelGGL(k_ica_mfma<2>, dim3(blocks), dim3(256), 0, d->stream, (const float*)X1T, n, ld, Wpk, tpw, part, state); break;
        case 3: hipLaunchKernelGGL(k_ica_mfma<3>, dim3(blocks), dim3(256), 0, d->stream, (const float*)X1T, n, ld, Wpk, tpw, part, state); break;
        default: hipLaunchKernelGGL(k_ica_mfma<4>, dim3(blocks), dim3(256), 0, d->stream, (const float*)X1T, n, ld, Wpk, tpw, part, state); break;
    }
    launch_check();
    ts.stop();
    hipLaunchKernelGGL(k_ica_reduce, dim3(cdiv(cnt, 32)), dim3(1024), 0, d->stream, part, nparts, NCP, (int)nc, GX_gp, state);
    launch_check();
    dev_free(d, part);
    dev_free(d, Wpk);
}
void op_ica_step(Dev* d, int dt, const void* X1T, int64_t n, int64_t nc, int64_t ld, const double* W, double* GX_gp,
                 const int* state) {
    ica_step_impl(d, dt, X1T, n, nc, ld, W, GX_gp, state, ICA_G_LOGCOSH);
}
void op_ica_step_g(Dev* d, int dt, const void* X1T, int64_t n, int64_t nc, int64_t ld, const double* W, double* GX_gp,
                   const int* state, int contrast) {
    if (contrast != ICA_G_LOGCOSH && contrast != ICA_G_EXP && contrast != ICA_G_CUBE) throw std::runtime_error("ica_step: unknown contrast");
    ica_step_impl(d, dt, X1T, n, nc, ld, W, GX_gp, state, contrast);
}


#define MB_DISPATCH(mb, CALL)            \
    switch (mb) {                        \
        case 0: { constexpr int MBv = 0; CALL; } break; \
        case 1: { constexpr int MBv = 1; CALL; } break; \
        case 2: { constexpr int MBv = 2; CALL; } break; \
        case 3: { constexpr int MBv = 3; CALL; } break; \
        case 4: { constexpr int MBv = 4; CALL; } break; \
        case 5: { constexpr int MBv = 5; CALL; } break; \
        default: { constexpr int MBv = 6; CALL; } break; \
    }

void op_ica_tail(Dev* d, int64_t nc, double n_total, double* W, const double* GX_gp, int mode, double tol, int* state, int iter,
                 int* progress) {
    double* scratch = (double*)dev_alloc(d, sizeof(double) * (6 * nc * nc + nc));
    // refresh the step kernel's planes of W if the last step used them for this W
    bf16x8* wpk3 = (d->ica_wpk3 && d->ica_wpk3_for == W && d->ica_wpk3_nc == nc) ? (bf16x8*)d->ica_wpk3 : nullptr;
    const int mb = nc <= 64 ? (int)((nc + 15) / 16) : 0;
    const size_t lds = sizeof(double) * (jac_ws_doubles((int)nc, ICA_TAIL_THREADS) + (mb ? 4 * nc * polar_ld((int)nc) : 0));
    MB_DISPATCH(mb, {
        set_max_lds(d, reinterpret_cast<const void*>(k_ica_tail<MBv>));
        hipLaunchKernelGGL(k_ica_tail<MBv>, dim3(1), dim3(ICA_TAIL_THREADS), lds, d->stream, (int)nc, n_total, W, GX_gp, mode, tol,
                           state, iter, scratch, wpk3, d->ica_ortho_tol2, progress);
    });
    launch_check();
    if (wpk3) d->ica_wpk3_valid = true;
    dev_free(d, scratch);
}
void op_symdecorr(Dev* d, int64_t nc, const double* Win, double* Wout, int mode, int* zero2) {
    d->ica_wpk3_valid = false;
    double* scratch = (double*)dev_alloc(d, sizeof(double) * (4 * nc * nc + nc));
    const int mb = nc <= 64 ? (int)((nc + 15) / 16) : 0;
    const size_t lds = sizeof(double) * (jac_ws_doubles((int)nc, ICA_TAIL_THREADS) + (mb ? 3 * nc * polar_ld((int)nc) : 0));
    MB_DISPATCH(mb, {
        set_max_lds(d, reinterpret_cast<const void*>(k_symdecorr<MBv>));
        hipLaunchKernelGGL(k_symdecorr<MBv>, dim3(1), dim3(ICA_TAIL_THREADS), lds, d->stream, Win, Wout, (int)nc, mode, scratch, zero2);
    });
    launch_check();
    dev_free(d, scratch);
}

// G = A^T A for a tall-skinny fp64 A (K x Mn, Mn a multiple of 16): the re-basing Gram matrices (l x l from a d x l
// iterate).  One workgroup per upper 16 x 16 tile, its four waves take a quarter of K each on the fp64 matrix cores and
// add through LDS; the mirror tile is written too.  (The general kernel needs a split-K launch plus a reduce launch here.)
// SYM = false: C = A^T B for two such matrices (every tile computed; H = P^T Yp of the one-pass thin QR).
template <bool SYM>
__global__ __launch_bounds__(256) void k_syrk_f64(const double* __restrict__ A, int64_t lda, const double* __restrict__ B, int64_t ldb,
                                                  int Mn, int64_t K, double* __restrict__ C, int64_t ldc) {
    __shared__ double red[3][4][64];
    const int nt = Mn >> 4;
    int t = blockIdx.x, ti = 0;
    if (SYM) { while (t >= nt - ti) { t -= nt - ti; ++ti; } t += ti; }
    else { ti = t / nt; t -= ti * nt; }
    const int tj = t;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
    const int64_t kq = ((K + 3) / 4 + 3) / 4 * 4, kbeg = wave * kq, kend = min(K, kbeg + kq);
    const double* pa = A + 16 * ti + i;
    const double* pb = B + 16 * tj + i;
    f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
    // the kernel is pure load latency (a wave's 32 MFMAs take 1 us): all operands of a 128-row batch are requested at once
    for (int64_t kb = kbeg; kb < kend; kb += 128) {
        double a[32], b[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) {
            const int64_t k = kb + 4 * u + q;
            const bool in = k < kend;
            a[u] = in ? pa[k * lda] : 0.0;
            b[u] = in ? pb[k * ldb] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 32; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc, 0, 0, 0);
    }
    if (wave > 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave - 1][r][lane] = acc[r];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double v = acc[r] + red[0][r][lane] + red[1][r][lane] + red[2][r][lane];
            const int row = 16 * ti + q + 4 * r, col = 16 * tj + i;
            C[(int64_t)row * ldc + col] = v;
            if (SYM && ti != tj) C[(int64_t)col * ldc + row] = v;
        }
    }
}

// C = A B for small fp64 matrices whose shapes are whole 16 x 16 tiles (A: M x K, B: K x N, both row-major, not transposed): one
// workgroup per output tile, its four waves take a quarter of K each on the fp64 matrix cores and add through LDS -- ONE launch
// where the generic kernel needs a split-K launch and a reduce launch (the subspace iteration's C Q products: 256 x 256 x 48)
// or walks K in 16-deep LDS stages (Yp T: 512 x 80 x 80).  Like k_syrk_f64 the kernel is load latency: a wave's operands of a
// 64-deep batch are all requested before its 16 MFMAs.
__global__ __launch_bounds__(256) void k_gemm_nn_f64(const double* __restrict__ A, int64_t lda, const double* __restrict__ B, int64_t ldb,
                                                     int64_t K, double* __restrict__ C, int64_t ldc, int ntn) {
    __shared__ double red[3][4][64];
    const int ti = blockIdx.x / ntn, tj = blockIdx.x - ti * ntn;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, q = lane >> 4;
    const int64_t kq = ((K + 3) / 4 + 3) / 4 * 4, kbeg = wave * kq, kend = min(K, kbeg + kq);
    const double* pa = A + (int64_t)(16 * ti + i) * lda;     // A[row][k]
    const double* pb = B + 16 * tj + i;                        // B[k][col]
    f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int64_t kb = kbeg; kb < kend; kb += 64) {
        double a[16], b[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int64_t k = kb + 4 * u + q;
            const bool in = k < kend;
            a[u] = in ? pa[k] : 0.0;
            b[u] = in ? pb[k * ldb] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc, 0, 0, 0);
    }
    if (wave > 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wave - 1][r][lane] = acc[r];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            C[(int64_t)(16 * ti + q + 4 * r) * ldc + 16 * tj + i] = acc[r] + red[0][r][lane] + red[1][r][lane] + red[2][r][lane];
    }
}

void op_dgemm(Dev* d, bool ta, bool tb, int64_t M, int64_t N, int64_t K, double alpha, const double* A, int64_t lda,
              const double* B, int64_t ldb, double beta, double* C, int64_t ldc, const double* colscale) {
    if (M == 0 || N == 0) return;
    if (!colscale && ta && !tb && M == N && M % 16 == 0 && M <= 256 && K >= 64 && alpha == 1.0 && beta == 0.0) {
        const int nt = (int)(M / 16);
        if (A == B && lda == ldb)
            hipLaunchKernelGGL(k_syrk_f64<true>, dim3(nt * (nt + 1) / 2), dim3(256), 0, d->stream, A, lda, B, ldb, (int)M, K, C, ldc);
        else
            hipLaunchKernelGGL(k_syrk_f64<false>, dim3(nt * nt), dim3(256), 0, d->stream, A, lda, B, ldb, (int)M, K, C, ldc);
        launch_check();
        return;
    }
    constexpr bool no_nn = false;
    if (!no_nn && !colscale && !ta && !tb && M % 16 == 0 && N % 16 == 0 && K >= 64 && K <= 4096 && alpha == 1.0 && beta == 0.0 &&
        (M / 16) * (N / 16) <= 4096) {
        hipLaunchKernelGGL(k_gemm_nn_f64, dim3((unsigned)((M / 16) * (N / 16))), dim3(256), 0, d->stream, A, lda, B, ldb, K, C, ldc, (int)(N / 16));
        launch_check();
        return;
    }
    const int64_t tiles = (int64_t)cdiv(N, 16) * cdiv(M, 16);
    int ks = 1;
    if (K >= 256 && tiles < 256) ks = (int)std::min<int64_t>(16, std::min<int64_t>(K / 64, (512 + tiles - 1) / tiles));
    if (ks > 1) {  // long reduction, few output tiles: spread K over the chip, then add the slices in order
        const int64_t kchunk = (cdiv(K, ks) + 31) / 32 * 32;
        ks = cdiv(K, kchunk);
        double* part = (double*)dev_alloc(d, sizeof(double) * ks * M * N);
        hipLaunchKernelGGL(k_dgemm, dim3(cdiv(N, 16), cdiv(M, 16), ks), dim3(16, 16), 0, d->stream, ta, tb, M, N, K, alpha, A, lda, B,
                           ldb, beta, C, ldc, kchunk, part, colscale, (bf16x8*)nullptr, 0);
        launch_check();
        hipLaunchKernelGGL(k_dgemm_reduce, dim3(cdiv(M * N, 256)), dim3(256), 0, d->stream, part, ks, M, N, alpha, beta, C, ldc, colscale);
        launch_check();
        dev_free(d, part);
        return;
    }
    hipLaunchKernelGGL(k_dgemm, dim3(cdiv(N, 16), cdiv(M, 16)), dim3(16, 16), 0, d->stream, ta, tb, M, N, K, alpha, A, lda, B, ldb,
                       beta, C, ldc, K, (double*)nullptr, colscale, (bf16x8*)nullptr, 0);
    launch_check();
}
__global__ void k_copy_diag(const double* __restrict__ G, int64_t ldg, int64_t L, double* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < L) out[j] = G[j * ldg + j];
}
// *ndead = max(*ndead, sum of the per-block counts): the dependent columns of the WHOLE matrix, as ops.h promises
__global__ void k_ndead_total(const int* __restrict__ cnt, int nb, int* __restrict__ ndead) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int tot = 0;
    for (int b = 0; b < nb; ++b) tot += cnt[b];
    if (tot > *ndead) *ndead = tot;
}
// L beyond the one-workgroup kernels (k + n_oversample > 200): blocked right-looking factorisation on the chip-wide fp64
// GEMM kernel, 128-wide diagonal blocks by k_chol_inv2 (which hands back T_JJ = R_JJ^-1 directly):
//   G_J,J.. -= sum_{K<J} R_KJ^T R_K,J..;  T_JJ = chol_inv(G_JJ);  R_J,rest = T_JJ^T G_J,rest;
//   T_IJ = -T_II sum_{K=I+1..J} R_IK T_KJ, block super-diagonal by block super-diagonal.
static void chol_inv_blocked(Dev* d, const double* G, int64_t L, int64_t ldg, double* T, int64_t ldt, double rel_tol, int* ndead,
                             int64_t Lz) {
    constexpr int64_t B = 128;
    const int64_t nb = (L + B - 1) / B;
    double* W = (double*)dev_alloc(d, sizeof(double) * L * L);      // working copy of G (Schur complements of the diagonal blocks)
    double* R = (double*)dev_alloc(d, sizeof(double) * L * L);      // off-diagonal blocks of the factor
    double* gd = (double*)dev_alloc(d, sizeof(double) * L);
    double* tmp = (double*)dev_alloc(d, sizeof(double) * B * B);
    HIP_CHECK(hipMemcpy2DAsync(W, L * sizeof(double), G, ldg * sizeof(double), L * sizeof(double), L, hipMemcpyDeviceToDevice, d->stream));
    hipLaunchKernelGGL(k_copy_diag, dim3(cdiv(L, 256)), dim3(256), 0, d->stream, G, ldg, L, gd);
    launch_check();
    HIP_CHECK(hipMemset2DAsync(T, ldt * sizeof(double), 0, Lz * sizeof(double), Lz, d->stream));
    // every diagonal block counts its own dependent columns; their SUM goes to the caller's word (each block once took the maximum
    // into it directly: dead columns in two blocks were reported as the larger of the two counts)
    int* cnt = ndead ? (int*)dev_alloc(d, sizeof(int) * nb) : nullptr;
    if (cnt) HIP_CHECK(hipMemsetAsync(cnt, 0, sizeof(int) * nb, d->stream));
    set_max_lds(d, reinterpret_cast<const void*>(k_chol_inv2));
    for (int64_t J = 0; J < nb; ++J) {
        const int64_t j0 = J * B, bj = std::min(B, L - j0), rest = L - j0 - bj;
        if (j0 > 0)  // block row J of the Schur complement (its diagonal block and everything right of it)
            op_dgemm(d, true, false, bj, L - j0, j0, -1.0, R + j0, L, R + j0, L, 1.0, W + j0 * L + j0, L);
        hipLaunchKernelGGL(k_chol_inv2, dim3(1), dim3(CHOL_THREADS), chol2_lds_bytes((int)bj), d->stream, W + j0 * L + j0, (int)bj, L,
                           T + j0 * ldt + j0, ldt, rel_tol, cnt ? cnt + J : nullptr, (int)bj, (const double*)(gd + j0), 0, (int)bj);
        launch_check();
        if (rest > 0)
            op_dgemm(d, true, false, bj, rest, bj, 1.0, T + j0 * ldt + j0, ldt, W + j0 * L + j0 + bj, L, 0.0, R + j0 * L + j0 + bj, L);
    }
    for (int64_t dl = 1; dl < nb; ++dl)
        for (int64_t I = 0; I + dl < nb; ++I) {
            const int64_t Jb = I + dl, i0 = I * B, bi = std::min(B, L - i0), j0 = Jb * B, bj = std::min(B, L - j0);
            const int64_t k0 = i0 + bi, kk = j0 + bj - k0;  // rows k0 .. j0 + bj of column block J of T are final
            op_dgemm(d, false, false, bi, bj, kk, 1.0, R + i0 * L + k0, L, T + k0 * ldt + j0, ldt, 0.0, tmp, bj);
            op_dgemm(d, false, false, bi, bj, bi, -1.0, T + i0 * ldt + i0, ldt, tmp, bj, 0.0, T + i0 * ldt + j0, ldt);
        }
    if (cnt) {
        hipLaunchKernelGGL(k_ndead_total, dim3(1), dim3(1), 0, d->stream, (const int*)cnt, (int)nb, ndead);
        launch_check();
        dev_free(d, cnt);
    }
    dev_free(d, tmp); dev_free(d, gd); dev_free(d, R); dev_free(d, W);
}

// the re-basing factorisation in RT form (what k_trsm_pack reads): k_chol_rt4 for M = 16 NB <= 144
static void launch_chol_rt(Dev* d, const double* G, int64_t L, int64_t ldg, double* T, int64_t ldt, double rel_tol, int* ndead, int64_t M,
                           int64_t ncount = 0) {
    switch ((int)(M / 16)) {
#define PETAL_CHOL_RT_CASE(NB)                                                                                                      \
    case NB:                                                                                                                        \
        hipLaunchKernelGGL((k_chol_rt4<NB>), dim3(1), dim3(256), 0, d->stream, G, (int)L, ldg, T, ldt, rel_tol, ndead, (int)(ncount > 0 ? ncount : L)); \
        break
        PETAL_CHOL_RT_CASE(1); PETAL_CHOL_RT_CASE(2); PETAL_CHOL_RT_CASE(3); PETAL_CHOL_RT_CASE(4); PETAL_CHOL_RT_CASE(5);
        PETAL_CHOL_RT_CASE(6); PETAL_CHOL_RT_CASE(7); PETAL_CHOL_RT_CASE(8); PETAL_CHOL_RT_CASE(9);
#undef PETAL_CHOL_RT_CASE
        default: throw std::logic_error("launch_chol_rt: order out of range");
    }
    launch_check();
}

// One re-basing step of the power iteration (see ops.h).  With the split-product kernels and L <= 140 the inverse of R is never
// formed: k_chol_inv2 stops after the diagonal-block inverses ("RT form") and k_trsm_pack applies R^-1 by blocked substitution
// while it packs the operand planes of the product that follows.
void op_rebase_xp(Dev* d, int dt, const void* X, int64_t n, int64_t K, int64_t ldx, const void* mu, const double* G, int64_t L,
                  int64_t ldg, double rel_tol, int* ndead, const double* A, int64_t M, int64_t lda, double* T, int64_t ldt,
                  double* P_out, int64_t ldpo, void* Z, int64_t ldz, int p_planes, bool steering) {
    const bool no_rt = false;
    const bool fused = dt == F32 && gemm_split_product(d) && n >= 64 && K % 16 == 0 && K > 0 && M % 16 == 0 && ldx % 4 == 0 &&
                       aligned16(X) && (!mu || aligned16(mu)) && ldz % 4 == 0 && aligned16(Z) && K < (1 << 24) && M < (1 << 24);
    if (!fused || no_rt || L == 0 || L > CHOL2_MAXL || M > TRSM_MAXM || M < L || P_out == nullptr) {
        // fp32-MFMA mode, fp64 data, shapes off the split-product kernels: still no explicit inverse where the small-matrix kernels
        // apply (round 6) -- k_chol_rt4 + the triangular solve (fp64 result, no operand planes), then the product packs P_out itself
        if (L > 0 && L <= CHOL2_MAXL && M % 16 == 0 && M <= TRSM_MAXM && M >= L && K % 16 == 0 && K > 0 && P_out != nullptr) {
            launch_chol_rt(d, G, L, ldg, T, ldt, rel_tol, ndead, M);
            op_trsm_right(d, A, K, lda, T, M, ldt, P_out, ldpo);
            op_gemm_xp(d, dt, X, n, K, ldx, mu, P_out, M, ldpo, nullptr, Z, ldz, nullptr);
            return;
        }
        op_chol_inv(d, G, L, ldg, T, ldt, rel_tol, ndead, M);
        op_gemm_xp_prod(d, dt, X, n, K, ldx, mu, A, M, lda, T, M, ldt, P_out, ldpo, Z, ldz);
        return;
    }
    launch_chol_rt(d, G, L, ldg, T, ldt, rel_tol, ndead, M);
    gemm_xp_impl(d, dt, X, n, K, ldx, mu, T, M, ldt, nullptr, Z, ldz, nullptr, A, M, lda, P_out, ldpo, true, nullptr, p_planes == 2, steering);
}


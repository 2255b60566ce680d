// k_nmf_cd_csr.inc -- part of the ONE translation unit hip_ops.hip (textually included there, inside namespace petal): Nmf by coordinate
// descent on sparse CSR data (include/petal_hip_nmf_cd_sparse.h).  A "cd sweep" of an image M (R x C) with G (R x KP, updated in place),
// F (C x KP, gathered), S = F^T F + l2 I on the first k diagonal entries (KP x KP) and the penalty l1:
//     z_r = sum over the stored entries t of row r of val[t] F[idx[t], :]                     (k_nmf_csr.inc's gather, nmf_csr_gather)
//     inner times, t = 0 .. KP - 1 in order on the CURRENT g_r, with z = z_r - l1:           (k_nmf_cd.inc's sweep, nmf_cd_sweep)
//         grad = -z[t] + sum_j S[t][j] g_r[j];  pg = g_r[t] == 0 ? min(0, grad) : grad;  violation += |pg|
//         if S[t][t] != 0:  g_r[t] = max(g_r[t] - grad / S[t][t], 0)
//     dots[r] = <z_r, g_r>   (the raw z_r, the new g_r);   viols[s R + r] = the violation of row r in sweep s
// All of F, G, S fp64 with KP = 16, 32 or 64 columns, ZERO in the padding (a padded component has z = -l1, g = 0 and S[t][t] = 0: it is
// skipped, stays zero and adds no violation).
//
//   k_nmf_cd_sweep<T, G, FROM_ZERO>   A WAVE TAKES FOUR CONSECUTIVE WORK ITEMS.  For each in turn all 64 lanes run the gather and the
//                      item's z goes into the wave's own LDS slot; then the 16-lane group q of the wave owns item q and, where the item is
//                      a whole row, runs nmf_cd_sweep<KP / 16> `inner` times (its broadcasts stay inside the group), so that the k-step
//                      dependent chain with its fp64 division runs once per FOUR rows.  The group stores the row of G, dots[row] and the
//                      row's violations.  An item of a split row stores its partial z in slot order and its group sits the sweep out (it
//                      sweeps zeros and stores nothing: no divergence inside the wave).  S sits in LDS once per workgroup with l2 added on
//                      the first k diagonal entries.  FROM_ZERO: g_r starts at zero (transform).
//   k_nmf_cd_sweep_split<KP, FROM_ZERO>  the split rows, four per wave: the partial z added in item order, then the same sweep and stores.
//   k_nmf_cd_gram<KP>  k_nmf_gram's slab (G^T G, the sum of dots) followed by `inner` sums of violations, the rows in the same fixed order;
//                      k_nmf_slabsum (k_nmf.inc) adds the slabs in workgroup order.
// No atomics anywhere; the order of every sum is fixed by the handle (its items) and KP alone.

// S into LDS with l2 on the first k diagonal entries
template <int KP>
__device__ __forceinline__ void nmf_cd_load_s(double* sS, const double* __restrict__ S, int k, double l2, int inner) {
    if (inner > 0)
        for (int t = threadIdx.x; t < KP * KP; t += 256) {
            const int r = t / KP, c = t - r * KP;
            sS[t] = S[t] + (r == c && r < k ? l2 : 0.0);
        }
    __syncthreads();
}

// the sum of one value per lane over the lane's 16-lane group, a fixed tree: the same bits in every lane of the group
__device__ __forceinline__ double nmf_cd_group_sum(double v) {
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// The sweeps and the stores of one row by its 16-lane group.  zs: the raw z_r (KP doubles of LDS, visible); ws: KP doubles of LDS for the
// row of g between sweeps; live: the group has a row (else it sweeps zeros and stores nothing).
template <int KT, bool FROM_ZERO>
__device__ __forceinline__ void nmf_cd_group_rule(const double* sS, const double* zs, double* ws, int lane, double* __restrict__ Gm, int64_t row,
                                                  bool live, int64_t rows, double l1, int inner, double* __restrict__ dots,
                                                  double* __restrict__ viols) {
    constexpr int KP = 16 * KT;
    const int j = lane & 15;
    double zraw[KT], z[KT], w[KT];
#pragma unroll
    for (int u = 0; u < KT; ++u) {
        zraw[u] = live ? zs[16 * u + j] : 0.0;
        z[u] = zraw[u] - l1;
        w[u] = (FROM_ZERO || !live) ? 0.0 : Gm[row * KP + 16 * u + j];
    }
    for (int it = 0; it < inner; ++it) {
#pragma unroll
        for (int u = 0; u < KT; ++u) ws[16 * u + j] = w[u];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const double v = nmf_cd_group_sum(nmf_cd_sweep<KT>(w, z, sS, ws, j, lane));
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                                    // every read of the old row is done
        if (viols && live && j == 0) viols[int64_t(it) * rows + row] = v;
    }
    if (live && inner > 0) {
#pragma unroll
        for (int u = 0; u < KT; ++u) Gm[row * KP + 16 * u + j] = w[u];
    }
    if (dots) {
        double v = 0.0;
#pragma unroll
        for (int u = 0; u < KT; ++u) v = fma(zraw[u], w[u], v);
        v = nmf_cd_group_sum(v);
        if (live && j == 0) dots[row] = v;
    }
}

template <class T, int G, bool FROM_ZERO>
__global__ __launch_bounds__(256) void k_nmf_cd_sweep(const CsrItem* __restrict__ items, int64_t n_items, const int32_t* __restrict__ idx,
                                                      const T* __restrict__ val, const double* __restrict__ F, double* __restrict__ Gm,
                                                      const double* __restrict__ S, int64_t rows, int k, double l1, double l2, int inner,
                                                      double* __restrict__ part, double* __restrict__ dots, double* __restrict__ viols) {
    constexpr int KP = 2 * G;
    __shared__ double sS[KP * KP];
    __shared__ double sZW[4][4][2 * KP];              // [wave][group]: z_r, then the row of g
    nmf_cd_load_s<KP>(sS, S, k, l2, inner);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4;
    const int64_t it0 = (int64_t(blockIdx.x) * 4 + wave) * 4;
    if (it0 >= n_items) return;                       // (whole waves leave: the shuffles below see all 64 lanes)
    const int c0 = (lane % G) * 2;
    int my_row = -1;                                  // the row of this lane's group, -1: none (past the items, or a piece of a split row)
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
        if (it0 + i >= n_items) break;                // (wave-uniform)
        const CsrItem item = items[it0 + i];
        double acc0, acc1;
        nmf_csr_gather<T, G>(item, idx, val, F, lane, acc0, acc1);
        if (lane < G) {
            if (item.slot >= 0) *reinterpret_cast<double2*>(part + int64_t(item.slot) * KP + c0) = make_double2(acc0, acc1);
            else { sZW[wave][i][c0] = acc0; sZW[wave][i][c0 + 1] = acc1; }
        }
        if (q == i && item.slot < 0) my_row = item.row;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    double* zs = sZW[wave][q];
    nmf_cd_group_rule<KP / 16, FROM_ZERO>(sS, zs, zs + KP, lane, Gm, my_row, my_row >= 0, rows, l1, inner, dots, viols);
}

template <int KP, bool FROM_ZERO>
__global__ __launch_bounds__(256) void k_nmf_cd_sweep_split(const CsrSplit* __restrict__ splits, int64_t n_splits, const double* __restrict__ part,
                                                            double* __restrict__ Gm, const double* __restrict__ S, int64_t rows, int k, double l1,
                                                            double l2, int inner, double* __restrict__ dots, double* __restrict__ viols) {
    constexpr int KT = KP / 16;
    __shared__ double sS[KP * KP];
    __shared__ double sZW[4][4][2 * KP];
    nmf_cd_load_s<KP>(sS, S, k, l2, inner);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, j = lane & 15;
    const int64_t s0 = (int64_t(blockIdx.x) * 4 + wave) * 4;
    if (s0 >= n_splits) return;
    const bool live = s0 + q < n_splits;
    int row = -1;
    double* zs = sZW[wave][q];
    if (live) {
        const CsrSplit sp = splits[s0 + q];
        row = sp.row;
#pragma unroll
        for (int u = 0; u < KT; ++u) {
            double sum = 0.0;
            for (int i = 0; i < sp.count; ++i) sum += part[(int64_t(sp.first_slot) + i) * KP + 16 * u + j];
            zs[16 * u + j] = sum;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    nmf_cd_group_rule<KT, FROM_ZERO>(sS, zs, zs + KP, lane, Gm, row, live, rows, l1, inner, dots, viols);
}

// slab[b] = { k_nmf_gram's KP^2 + 1 doubles, then for every sweep s the sum of viols[s rows + r] over the rows of workgroup b's tiles }
template <int KP>
__global__ __launch_bounds__(256) void k_nmf_cd_gram(const double* __restrict__ Gm, int64_t rows, const double* __restrict__ dots,
                                                     const double* __restrict__ viols, int inner, double* __restrict__ slab) {
    __shared__ double tile[16][KP + 1];
    __shared__ double red[256];
    double* out = slab + int64_t(blockIdx.x) * (KP * KP + 1 + inner);
    nmf_gram_slab<KP>(Gm, rows, dots, out, tile, red);
    const int tid = threadIdx.x;
    const int64_t ntiles = (rows + 15) / 16;
    for (int s = 0; s < inner; ++s) {
        double v = 0.0;
        if (tid < 16)
            for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x)
                if (t * 16 + tid < rows) v += viols[int64_t(s) * rows + t * 16 + tid];
        __syncthreads();
        red[tid] = v;
        __syncthreads();
        if (tid == 0) {
            double sum = 0.0;
            for (int i = 0; i < 16; ++i) sum += red[i];
            out[KP * KP + 1 + s] = sum;
        }
    }
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------------
template <class T, int G, bool FROM_ZERO>
static void nmf_cd_sweep_launch(Dev* d, const CsrImage& img, const double* F, double* Gm, const double* S, int k, double l1, double l2, int inner,
                                double* part, double* dots, double* viols) {
    hipLaunchKernelGGL((k_nmf_cd_sweep<T, G, FROM_ZERO>), dim3((unsigned)cdiv64(img.n_items, 16)), dim3(256), 0, d->stream, img.items, img.n_items,
                       img.idx, (const T*)img.val, F, Gm, S, img.rows, k, l1, l2, inner, part, dots, viols);
    launch_check();
    if (img.n_splits) {
        hipLaunchKernelGGL((k_nmf_cd_sweep_split<2 * G, FROM_ZERO>), dim3((unsigned)cdiv64(img.n_splits, 16)), dim3(256), 0, d->stream, img.splits,
                           img.n_splits, (const double*)part, Gm, S, img.rows, k, l1, l2, inner, dots, viols);
        launch_check();
    }
}
template <class T, int G>
static void nmf_cd_sweep_zero(Dev* d, bool from_zero, const CsrImage& img, const double* F, double* Gm, const double* S, int k, double l1, double l2,
                              int inner, double* part, double* dots, double* viols) {
    if (from_zero) nmf_cd_sweep_launch<T, G, true>(d, img, F, Gm, S, k, l1, l2, inner, part, dots, viols);
    else nmf_cd_sweep_launch<T, G, false>(d, img, F, Gm, S, k, l1, l2, inner, part, dots, viols);
}

bool op_nmf_cd_sweep_csr(Dev* d, int dt, const CsrImage& img, int64_t k, int64_t kp, const double* F, double* G, const double* S, bool from_zero,
                         double l1, double l2, int64_t inner, double* gram_dot_viol) {
    if (k < 1 || k > 64 || kp != nmf_csr_padded_k(k) || img.rows < 1 || !F || !G || !S || !aligned16(F) || !aligned16(G) || inner < 0 ||
        inner > (int64_t(1) << 30) || (from_zero && inner < 1) || (gram_dot_viol && inner > (int64_t(1) << 10)))
        return false;
    csr_check_grid(img);
    double* part = img.n_slots ? (double*)dev_alloc(d, sizeof(double) * size_t(img.n_slots) * kp) : nullptr;
    // dots (rows), then the violations (inner x rows)
    double* dots = gram_dot_viol ? (double*)dev_alloc(d, sizeof(double) * size_t(img.rows) * size_t(1 + inner)) : nullptr;
    double* viols = dots && inner > 0 ? dots + img.rows : nullptr;
    TagScope ts(d);
#define PETAL_NMF_CD_SWEEP(Gv) DISPATCH_T(dt, (nmf_cd_sweep_zero<T, Gv>(d, from_zero, img, F, G, S, (int)k, l1, l2, (int)inner, part, dots, viols)))
    if (kp == 16) PETAL_NMF_CD_SWEEP(8);
    else if (kp == 32) PETAL_NMF_CD_SWEEP(16);
    else PETAL_NMF_CD_SWEEP(32);
#undef PETAL_NMF_CD_SWEEP
    ts.stop();
    if (gram_dot_viol) {
        const int g = (int)std::min<int64_t>(cdiv64(img.rows, 16), NMF_GRAM_MAX_WG);
        const int64_t count = kp * kp + 1 + inner;
        double* slab = (double*)dev_alloc(d, sizeof(double) * size_t(g) * count);
        if (kp == 16) hipLaunchKernelGGL(k_nmf_cd_gram<16>, dim3(g), dim3(256), 0, d->stream, (const double*)G, img.rows, (const double*)dots, (const double*)viols, (int)inner, slab);
        else if (kp == 32) hipLaunchKernelGGL(k_nmf_cd_gram<32>, dim3(g), dim3(256), 0, d->stream, (const double*)G, img.rows, (const double*)dots, (const double*)viols, (int)inner, slab);
        else hipLaunchKernelGGL(k_nmf_cd_gram<64>, dim3(g), dim3(256), 0, d->stream, (const double*)G, img.rows, (const double*)dots, (const double*)viols, (int)inner, slab);
        launch_check();
        hipLaunchKernelGGL(k_nmf_slabsum, dim3((unsigned)cdiv64(count, 256)), dim3(256), 0, d->stream, (const double*)slab, g, count, gram_dot_viol);
        launch_check();
        dev_free(d, slab);
    }
    if (part) dev_free(d, part);
    if (dots) dev_free(d, dots);
    return true;
}

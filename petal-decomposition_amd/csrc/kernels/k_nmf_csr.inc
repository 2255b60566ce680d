// k_nmf_csr.inc -- part of the ONE translation unit hip_ops.hip (textually included there, inside namespace petal): Nmf on sparse CSR
// data (include/petal_hip_nmf_sparse.h).  An iteration is two SWEEPS of the same shape, one over the rows of X (it updates W) and one
// over the rows of the transposed image (it updates H^T); A = W^T X (k x d) is never formed.  A sweep of an image M (R x C) with
// G (R x KP, updated in place), F (C x KP, gathered), S = F^T F (KP x KP):
//     z_r = sum over the stored entries t of row r of val[t] F[idx[t], :]
//     inner times:  D = g_r S + l1 + l2 g_r,  D[D == 0] = 2^-23,  g_r <- g_r o (z_r / D)
//     dots[r] = <z_r, g_r>   (the new g_r)
// All of F, G, S fp64 with KP = 16, 32 or 64 columns, ZERO in the padding (a padded component stays zero under the rule: 0 * 0 / D).
//
//   k_nmf_sweep<T, G, CONST>   ONE WAVE PER WORK ITEM (at most PETAL_CSR_ITEM_NNZ stored entries of one image row): k_spmm's gather --
//                      indices and values loaded coalesced 64 at a time and handed round by lane shuffles, G = KP / 2 lanes hold one
//                      gathered row of F as 16-byte loads, every sub-group keeps four rows in flight, fp64 accumulators, the sub-groups
//                      added by the fixed shuffle tree.  An item that is a whole row then runs the rule: z_r and g_r go through the
//                      wave's own 2 KP doubles of LDS, S sits in LDS once per workgroup, and the KP x KP products of D are spread over
//                      ALL 64 lanes -- lane l forms column l mod KP over rows (l / KP) KP^2 / 64 ... of S, the 64 / KP partial columns
//                      meet by xor shuffles -- so that transform's hundreds of updates per row cost KP^2 / 64 fused multiply-adds per
//                      lane each.  CONST: g_r starts as a constant in its k leading columns (transform).  An item of a split row stores
//                      its partial z in slot order instead.
//   k_nmf_sweep_split<KP, CONST>  the split rows, a wave each: the partial z added in item order, then the same rule and stores.
//   k_nmf_gram<KP>     G^T G and the sum of dots over the tall factor: workgroup b takes the 16-row tiles b, b + NB, ... and writes
//                      one slab of KP^2 + 1 doubles; k_nmf_slabsum (k_nmf.inc) adds the slabs in workgroup order.
//   k_csr_densify<T>   the dense image of a resident handle in its own type, duplicates added in position order: the thread of a row's
//                      first item walks the whole row.  Serves the densifying fall-back only.
//   k_nmf_valscan<T>   { sum, sum of squares, min(v, 0), non-finite seen } over the stored values; k_nmf_scan_sum adds the parts.
// No atomics anywhere; the order of every sum is fixed by the handle (its items) and KP alone.

// The rule on one row, by one whole wave.  zs / gs: this wave's KP doubles each in LDS, z_r already stored by the caller's lanes (and
// made visible); sS: S in LDS.  Returns with g_r stored and dots[row] written (where dots is given).
template <int KP, bool CONST>
__device__ __forceinline__ void nmf_row_rule(const double* sS, double* zs, double* gs, int lane, double* __restrict__ Gm, int64_t row, int k,
                                             double gconst, double l1, double l2, int inner, double* __restrict__ dots) {
    constexpr int NPART = 64 / KP, SPAN = KP / NPART;
    const int j = lane % KP, part = lane / KP;
    double gj = CONST ? (j < k ? gconst : 0.0) : Gm[row * KP + j];
    if (part == 0) gs[j] = gj;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const double zj = zs[j];
    for (int it = 0; it < inner; ++it) {
        double dd = 0.0;
#pragma unroll 8
        for (int i = part * SPAN; i < (part + 1) * SPAN; ++i) dd = fma(gs[i], sS[i * KP + j], dd);
#pragma unroll
        for (int off = KP; off < 64; off <<= 1) dd += __shfl_xor(dd, off);   // (a + b on both partners: the same bits in every part)
        double den = (dd + l1) + l2 * gj;
        if (den == 0.0) den = NMF_EPS;
        gj = gj * (zj / den);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();                                    // every read of the old g_r is done
        if (part == 0) gs[j] = gj;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    if (part == 0 && (CONST || inner > 0)) Gm[row * KP + j] = gj;
    if (dots) {
        double v = part == 0 ? zj * gj : 0.0;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off);
        if (lane == 0) dots[row] = v;
    }
}

template <int KP>
__device__ __forceinline__ void nmf_load_s(double* sS, const double* __restrict__ S, int inner) {
    if (inner > 0)
        for (int t = threadIdx.x; t < KP * KP; t += 256) sS[t] = S[t];
    __syncthreads();
}

// The gather of one work item by one whole wave (k_spmm's): lanes 0 .. G - 1 return z[c0], z[c0 + 1] of the item, c0 = 2 (lane % G), in
// acc0 / acc1 (the other lanes: partial sums).  Shared with k_nmf_cd_csr.inc.
template <class T, int G>
__device__ __forceinline__ void nmf_csr_gather(const CsrItem& item, const int32_t* __restrict__ idx, const T* __restrict__ val,
                                               const double* __restrict__ F, int lane, double& acc0, double& acc1) {
    constexpr int KP = 2 * G, NSUB = 64 / G;
    const int sub = lane / G;
    const double* Fc = F + (lane % G) * 2;
    acc0 = 0.0;
    acc1 = 0.0;
    for (int base = 0; base < item.count; base += 64) {
        const int cnt = min(64, item.count - base);
        int my_i = 0;
        double my_v = 0.0;
        if (lane < cnt) { my_i = idx[item.first + base + lane]; my_v = double(val[item.first + base + lane]); }
        for (int j = 0; j < cnt; j += 4 * NSUB) {     // four gathered rows in flight per sub-group
            double2 p[4];
            double v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int src = (j + u * NSUB + sub) & 63;   // (a position past the item reads SOME row that exists -- row 0 or one of the item's -- and is not added)
                v[u] = __shfl(my_v, src);
                p[u] = *reinterpret_cast<const double2*>(Fc + int64_t(__shfl(my_i, src)) * KP);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (j + u * NSUB + sub < cnt) {
                    acc0 = fma(v[u], p[u].x, acc0);
                    acc1 = fma(v[u], p[u].y, acc1);
                }
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= G; off >>= 1) {
        acc0 += __shfl_down(acc0, off);
        acc1 += __shfl_down(acc1, off);
    }
}

template <class T, int G, bool CONST>
__global__ __launch_bounds__(256) void k_nmf_sweep(const CsrItem* __restrict__ items, int64_t n_items, const int32_t* __restrict__ idx,
                                                   const T* __restrict__ val, const double* __restrict__ F, double* __restrict__ Gm,
                                                   const double* __restrict__ S, int k, double gconst, double l1, double l2, int inner,
                                                   double* __restrict__ part, double* __restrict__ dots) {
    constexpr int KP = 2 * G;
    __shared__ double sS[KP * KP];
    __shared__ double sZG[4][2 * KP];
    nmf_load_s<KP>(sS, S, inner);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane / G;
    const int64_t it = int64_t(blockIdx.x) * 4 + wave;
    if (it >= n_items) return;                        // (whole waves leave: the shuffles below see all 64 lanes)
    const CsrItem item = items[it];
    const int c0 = (lane % G) * 2;
    double acc0, acc1;
    nmf_csr_gather<T, G>(item, idx, val, F, lane, acc0, acc1);
    if (item.slot >= 0) {                             // part of a split row: the partial sums, for k_nmf_sweep_split
        if (sub == 0) *reinterpret_cast<double2*>(part + int64_t(item.slot) * KP + c0) = make_double2(acc0, acc1);
        return;
    }
    double* zs = sZG[wave];
    if (sub == 0) { zs[c0] = acc0; zs[c0 + 1] = acc1; }
    nmf_row_rule<KP, CONST>(sS, zs, zs + KP, lane, Gm, item.row, k, gconst, l1, l2, inner, dots);
}

template <int KP, bool CONST>
__global__ __launch_bounds__(256) void k_nmf_sweep_split(const CsrSplit* __restrict__ splits, int64_t n_splits, const double* __restrict__ part,
                                                         double* __restrict__ Gm, const double* __restrict__ S, int k, double gconst, double l1,
                                                         double l2, int inner, double* __restrict__ dots) {
    __shared__ double sS[KP * KP];
    __shared__ double sZG[4][2 * KP];
    nmf_load_s<KP>(sS, S, inner);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t s = int64_t(blockIdx.x) * 4 + wave;
    if (s >= n_splits) return;
    const CsrSplit sp = splits[s];
    double* zs = sZG[wave];
    if (lane < KP) {
        double sum = 0.0;
        for (int i = 0; i < sp.count; ++i) sum += part[(int64_t(sp.first_slot) + i) * KP + lane];
        zs[lane] = sum;
    }
    nmf_row_rule<KP, CONST>(sS, zs, zs + KP, lane, Gm, sp.row, k, gconst, l1, l2, inner, dots);
}

// slab[b] = { sum over the rows of workgroup b's tiles of g_r^T g_r (KP x KP), sum of dots[r] }.  Thread (ty, tx) = (tid / 16, tid % 16)
// holds the KP / 16 x KP / 16 block at (ty, tx) KP / 16 of the product; a tile is 16 rows of G in LDS.
constexpr int NMF_GRAM_MAX_WG = 256;
// the slab of this workgroup into out (KP^2 + 1 doubles); tile: 16 x (KP + 1) doubles of LDS, red: 256.  Shared with k_nmf_cd_csr.inc.
template <int KP>
__device__ __forceinline__ void nmf_gram_slab(const double* __restrict__ Gm, int64_t rows, const double* __restrict__ dots, double* __restrict__ out,
                                              double (*tile)[KP + 1], double* red) {
    constexpr int B = KP / 16;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int64_t ntiles = (rows + 15) / 16;
    double acc[B][B];
#pragma unroll
    for (int a = 0; a < B; ++a)
#pragma unroll
        for (int b = 0; b < B; ++b) acc[a][b] = 0.0;
    double dsum = 0.0;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t row0 = t * 16;
        __syncthreads();
        for (int e = tid; e < 16 * KP; e += 256) {
            const int r = e / KP, c = e - r * KP;
            tile[r][c] = row0 + r < rows ? Gm[(row0 + r) * KP + c] : 0.0;
        }
        if (dots && tid < 16 && row0 + tid < rows) dsum += dots[row0 + tid];
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < 16; ++r) {
            double av[B], bv[B];
#pragma unroll
            for (int a = 0; a < B; ++a) { av[a] = tile[r][ty * B + a]; bv[a] = tile[r][tx * B + a]; }
#pragma unroll
            for (int a = 0; a < B; ++a)
#pragma unroll
                for (int b = 0; b < B; ++b) acc[a][b] = fma(av[a], bv[b], acc[a][b]);
        }
    }
#pragma unroll
    for (int a = 0; a < B; ++a)
#pragma unroll
        for (int b = 0; b < B; ++b) out[(ty * B + a) * KP + tx * B + b] = acc[a][b];
    red[tid] = dsum;                                   // (threads 16 .. 255 hold zeros)
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < 16; ++i) s += red[i];
        out[KP * KP] = s;
    }
}
template <int KP>
__global__ __launch_bounds__(256) void k_nmf_gram(const double* __restrict__ Gm, int64_t rows, const double* __restrict__ dots,
                                                  double* __restrict__ slab) {
    __shared__ double tile[16][KP + 1];
    __shared__ double red[256];
    nmf_gram_slab<KP>(Gm, rows, dots, slab + int64_t(blockIdx.x) * (KP * KP + 1), tile, red);
}

template <class T>
__global__ __launch_bounds__(256) void k_csr_densify(const CsrItem* __restrict__ items, int64_t n_items, const int32_t* __restrict__ idx,
                                                     const T* __restrict__ val, T* __restrict__ out, int64_t ldo) {
    const int64_t it = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (it >= n_items) return;
    const CsrItem first = items[it];
    if (it > 0 && items[it - 1].row == first.row) return;   // (a later item of a split row: the row's first item walks it all)
    T* orow = out + int64_t(first.row) * ldo;
    for (int64_t q = it; q < n_items; ++q) {
        const CsrItem item = items[q];
        if (item.row != first.row) break;
        for (int t = 0; t < item.count; ++t) orow[idx[item.first + t]] += val[item.first + t];
    }
}

template <class T>
__global__ __launch_bounds__(256) void k_nmf_valscan(const T* __restrict__ val, int64_t nnz, double* __restrict__ part) {
    __shared__ double red[4][256];
    const int t = threadIdx.x;
    double s = 0.0, s2 = 0.0, mn = 0.0, bad = 0.0;
    for (int64_t i = int64_t(blockIdx.x) * 256 + t; i < nnz; i += int64_t(gridDim.x) * 256) {
        const double v = (double)val[i];
        s += v;
        s2 += v * v;
        mn = fmin(mn, v);
        if (!(v - v == 0.0)) bad = 1.0;
    }
    red[0][t] = s; red[1][t] = s2; red[2][t] = mn; red[3][t] = bad;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) {
            red[0][t] += red[0][t + w];
            red[1][t] += red[1][t + w];
            red[2][t] = fmin(red[2][t], red[2][t + w]);
            red[3][t] = fmax(red[3][t], red[3][t + w]);
        }
        __syncthreads();
    }
    if (t < 4) part[blockIdx.x * 4 + t] = red[t][0];
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------------
bool op_nmf_valscan(Dev* d, int dt, const void* val, int64_t nnz, double* out4) {
    if (nnz < 1) { dev_memset(d, out4, 0, sizeof(double) * 4); return true; }
    const int g = (int)std::min<int64_t>(cdiv64(nnz, 256), 1024);
    double* part = (double*)dev_alloc(d, sizeof(double) * 4 * size_t(g));
    DISPATCH_T(dt, hipLaunchKernelGGL((k_nmf_valscan<T>), dim3(g), dim3(256), 0, d->stream, (const T*)val, nnz, part));
    launch_check();
    hipLaunchKernelGGL(k_nmf_scan_sum, dim3(1), dim3(256), 0, d->stream, (const double*)part, g, out4);
    launch_check();
    dev_free(d, part);
    return true;
}

bool op_nmf_gram(Dev* d, const double* G, int64_t rows, int64_t kp, const double* dots, double* gram_dot) {
    if (rows < 1 || (kp != 16 && kp != 32 && kp != 64) || !G || !gram_dot) return false;
    const int g = (int)std::min<int64_t>(cdiv64(rows, 16), NMF_GRAM_MAX_WG);
    const int64_t count = kp * kp + 1;
    double* slab = (double*)dev_alloc(d, sizeof(double) * size_t(g) * count);
    if (kp == 16) hipLaunchKernelGGL(k_nmf_gram<16>, dim3(g), dim3(256), 0, d->stream, G, rows, dots, slab);
    else if (kp == 32) hipLaunchKernelGGL(k_nmf_gram<32>, dim3(g), dim3(256), 0, d->stream, G, rows, dots, slab);
    else hipLaunchKernelGGL(k_nmf_gram<64>, dim3(g), dim3(256), 0, d->stream, G, rows, dots, slab);
    launch_check();
    hipLaunchKernelGGL(k_nmf_slabsum, dim3((unsigned)cdiv64(count, 256)), dim3(256), 0, d->stream, (const double*)slab, g, count, gram_dot);
    launch_check();
    dev_free(d, slab);
    return true;
}

template <class T, int G, bool CONST>
static void nmf_sweep_launch(Dev* d, const CsrImage& img, const double* F, double* Gm, const double* S, int k, double gconst, double l1, double l2,
                             int inner, double* part, double* dots) {
    hipLaunchKernelGGL((k_nmf_sweep<T, G, CONST>), dim3((unsigned)cdiv64(img.n_items, 4)), dim3(256), 0, d->stream, img.items, img.n_items, img.idx,
                       (const T*)img.val, F, Gm, S, k, gconst, l1, l2, inner, part, dots);
    launch_check();
    if (img.n_splits) {
        hipLaunchKernelGGL((k_nmf_sweep_split<2 * G, CONST>), dim3((unsigned)cdiv64(img.n_splits, 4)), dim3(256), 0, d->stream, img.splits,
                           img.n_splits, (const double*)part, Gm, S, k, gconst, l1, l2, inner, dots);
        launch_check();
    }
}
template <class T, int G>
static void nmf_sweep_const(Dev* d, bool from_const, const CsrImage& img, const double* F, double* Gm, const double* S, int k, double gconst,
                            double l1, double l2, int inner, double* part, double* dots) {
    if (from_const) nmf_sweep_launch<T, G, true>(d, img, F, Gm, S, k, gconst, l1, l2, inner, part, dots);
    else nmf_sweep_launch<T, G, false>(d, img, F, Gm, S, k, gconst, l1, l2, inner, part, dots);
}

bool op_nmf_sweep_csr(Dev* d, int dt, const CsrImage& img, int64_t k, int64_t kp, const double* F, double* G, const double* S, bool from_const,
                      double gconst, double l1, double l2, int64_t inner, double* gram_dot) {
    if (k < 1 || k > 64 || kp != nmf_csr_padded_k(k) || img.rows < 1 || !F || !G || !S || !aligned16(F) || !aligned16(G) || inner < 0 ||
        inner > (int64_t(1) << 30))
        return false;
    csr_check_grid(img);
    double* part = img.n_slots ? (double*)dev_alloc(d, sizeof(double) * size_t(img.n_slots) * kp) : nullptr;
    double* dots = gram_dot ? (double*)dev_alloc(d, sizeof(double) * size_t(img.rows)) : nullptr;
    TagScope ts(d);
#define PETAL_NMF_SWEEP(Gv) DISPATCH_T(dt, (nmf_sweep_const<T, Gv>(d, from_const, img, F, G, S, (int)k, gconst, l1, l2, (int)inner, part, dots)))
    if (kp == 16) PETAL_NMF_SWEEP(8);
    else if (kp == 32) PETAL_NMF_SWEEP(16);
    else PETAL_NMF_SWEEP(32);
#undef PETAL_NMF_SWEEP
    ts.stop();
    if (gram_dot) op_nmf_gram(d, G, img.rows, kp, dots, gram_dot);
    if (part) dev_free(d, part);
    if (dots) dev_free(d, dots);
    return true;
}

bool op_csr_densify(Dev* d, int dt, const CsrImage& img, void* out, int64_t cols, int64_t ldo) {
    if (img.rows < 1 || cols < 1 || ldo < cols || !out) return false;
    if (cdiv64(img.n_items, 256) >= (int64_t(1) << 31)) throw std::runtime_error("sparse matrix has too many work items for one launch");
    dev_memset(d, out, 0, dtype_size(dt) * size_t(img.rows) * size_t(ldo));
    DISPATCH_T(dt, hipLaunchKernelGGL((k_csr_densify<T>), dim3((unsigned)cdiv64(img.n_items, 256)), dim3(256), 0, d->stream, img.items, img.n_items,
                                      img.idx, (const T*)img.val, (T*)out, ldo));
    launch_check();
    return true;
}

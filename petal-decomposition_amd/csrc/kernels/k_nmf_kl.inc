// k_nmf_kl.inc -- part of the ONE translation unit hip_ops.hip (textually included there, inside namespace petal): Nmf with the
// generalised Kullback-Leibler loss on sparse CSR data (include/petal_hip_nmf_kl.h).  The updates touch X only at its stored entries, so
// an iteration is two SWEEPS of k_nmf_sweep's gather in which every gathered factor row is used twice: for an inner product with the row
// being updated (a sampled dense-dense product) and then accumulated with the quotient.  A sweep of an image M (R x C) with G (R x KP,
// updated in place), F (C x KP, gathered), c = colsum(F) (KP), `inner` times for row r:
//     for every stored entry t:  wh_t = <g_r, F[idx_t, :]>,  wh_t < 2^-23 -> 2^-23,  q_t = val_t / wh_t
//     num = sum_t q_t F[idx_t, :] ;  den = (c + l1) + l2 g_r,  den[den == 0] = 2^-23 ;  g_r <- g_r o (num / den)
// inner == 0: G is left alone and terms[r] = sum_t [val_t > 2^-23] val_t log(val_t / wh_t).
// All of F, G, c fp64 with KP = 16, 32 or 64 columns, ZERO in the padding (a padded component stays zero: 0 * (0 / den)).
//
//   k_nmf_kl_sweep<T, G, CONST>  ONE WAVE PER WORK ITEM, k_nmf_sweep's frame: indices and values loaded coalesced 64 at a time and handed
//                      round by lane shuffles, G = KP / 2 lanes hold one gathered row of F as 16-byte loads, four rows in flight per
//                      sub-group.  Every lane keeps its two entries of g_r in registers; the partial inner product of a gathered row is
//                      reduced over the sub-group's G lanes by a fixed xor-shuffle tree (a + b on both partners: the same bits in every
//                      lane), the four trees of the rows in flight interleaved; then the clamp, ONE fp64 division and acc += q p.  The
//                      sub-groups are added by the fixed shuffle tree, the rule runs in registers (a KP-vector denominator: no S, no LDS)
//                      and the new g_r is handed back to every sub-group for the next update.  An item that is a whole row loops `inner`
//                      times in the kernel, re-reading its indices, values and F rows (L1 / L2 by then).  CONST: g_r starts as a constant
//                      in its k leading columns (transform).  An item of a split row reads the old g_r and stores its partial num (or
//                      its partial term) in slot order.
//   k_nmf_kl_split<KP, CONST>  the split rows, a wave each: the partials added in item order, then the same rule and store.  An image with
//                      split rows and inner > 1 is swept by `inner` launch pairs of one update each (every row is updated once per pair:
//                      the bytes of `inner` single-update sweeps).
//   k_nmf_kl_colsum<KP>  colsum(G) and the sum of terms: workgroup b takes the rows b RL + rl, stride gridDim RL, and writes one slab of
//                      KP + 1 doubles; k_nmf_slabsum (k_nmf.inc) adds the slabs in workgroup order.  No KP x KP Gram matrix.
//   k_nmf_kl_vsum<T>   sum over the stored values of [v > 2^-23] v (the loss's third term), parts added by k_nmf_slabsum.
// No atomics anywhere; the order of every sum is fixed by the handle (its items) and KP alone.

template <class T, int G, bool TERM>
__device__ __forceinline__ void nmf_kl_gather(const CsrItem& item, const int32_t* __restrict__ idx, const T* __restrict__ val,
                                              const double* __restrict__ Fc, int lane, int sub, double g0, double g1, double& acc0,
                                              double& acc1, double& tsum) {
    constexpr int KP = 2 * G, NSUB = 64 / G;
    for (int base = 0; base < item.count; base += 64) {
        const int cnt = min(64, item.count - base);
        int my_i = 0;
        double my_v = 0.0;
        if (lane < cnt) { my_i = idx[item.first + base + lane]; my_v = double(val[item.first + base + lane]); }
        for (int j = 0; j < cnt; j += 4 * NSUB) {     // four gathered rows in flight per sub-group
            double2 p[4];
            double v[4], d[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int src = (j + u * NSUB + sub) & 63;   // (a position past the item reads SOME row that exists -- row 0 or one of the item's -- and is not added)
                v[u] = __shfl(my_v, src);
                p[u] = *reinterpret_cast<const double2*>(Fc + int64_t(__shfl(my_i, src)) * KP);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) d[u] = fma(g1, p[u].y, g0 * p[u].x);
#pragma unroll
            for (int off = G / 2; off >= 1; off >>= 1) {
#pragma unroll
                for (int u = 0; u < 4; ++u) d[u] += __shfl_xor(d[u], off);   // (the four trees interleave; the same bits in all G lanes)
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double wh = d[u] < NMF_EPS ? NMF_EPS : d[u];
                if (j + u * NSUB + sub < cnt) {
                    if (TERM) {
                        if (v[u] > NMF_EPS) tsum += v[u] * log(v[u] / wh);
                    } else {
                        const double q = v[u] / wh;
                        acc0 = fma(q, p[u].x, acc0);
                        acc1 = fma(q, p[u].y, acc1);
                    }
                }
            }
        }
    }
}

__device__ __forceinline__ double nmf_kl_rule(double g, double num, double c, double l1, double l2) {
    double den = (c + l1) + l2 * g;
    if (den == 0.0) den = NMF_EPS;
    return g * (num / den);
}

template <class T, int G, bool CONST>
__global__ __launch_bounds__(256) void k_nmf_kl_sweep(const CsrItem* __restrict__ items, int64_t n_items, const int32_t* __restrict__ idx,
                                                      const T* __restrict__ val, const double* __restrict__ F, double* __restrict__ Gm,
                                                      const double* __restrict__ csum, int k, double gconst, double l1, double l2, int inner,
                                                      double* __restrict__ part, double* __restrict__ tpart, double* __restrict__ terms) {
    constexpr int KP = 2 * G;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane / G;
    const int64_t it = int64_t(blockIdx.x) * 4 + wave;
    if (it >= n_items) return;                        // (whole waves leave: the shuffles below see all 64 lanes)
    const CsrItem item = items[it];
    const int c0 = (lane % G) * 2;
    const double* Fc = F + c0;
    double g0, g1;
    if (CONST) {
        g0 = c0 < k ? gconst : 0.0;
        g1 = c0 + 1 < k ? gconst : 0.0;
    } else {
        const double2 gv = *reinterpret_cast<const double2*>(Gm + int64_t(item.row) * KP + c0);
        g0 = gv.x; g1 = gv.y;
    }
    if (inner == 0) {                                 // the loss's term: G is left alone
        double a0 = 0.0, a1 = 0.0, tsum = 0.0;
        nmf_kl_gather<T, G, true>(item, idx, val, Fc, lane, sub, g0, g1, a0, a1, tsum);
#pragma unroll
        for (int off = 32; off >= G; off >>= 1) tsum += __shfl_down(tsum, off);   // (every lane of a sub-group holds its sub-group's sum)
        if (lane == 0) {
            if (item.slot >= 0) tpart[item.slot] = tsum;
            else terms[item.row] = tsum;
        }
        return;
    }
    const double cs0 = csum[c0], cs1 = csum[c0 + 1];
    for (int upd = 0;;) {
        double acc0 = 0.0, acc1 = 0.0, tsum = 0.0;
        nmf_kl_gather<T, G, false>(item, idx, val, Fc, lane, sub, g0, g1, acc0, acc1, tsum);
#pragma unroll
        for (int off = 32; off >= G; off >>= 1) {
            acc0 += __shfl_down(acc0, off);
            acc1 += __shfl_down(acc1, off);
        }
        if (item.slot >= 0) {                         // part of a split row: the partial sums, for k_nmf_kl_split
            if (sub == 0) *reinterpret_cast<double2*>(part + int64_t(item.slot) * KP + c0) = make_double2(acc0, acc1);
            return;
        }
        g0 = nmf_kl_rule(g0, acc0, cs0, l1, l2);       // (sub-group 0 holds num; the others compute on partial sums and are overwritten)
        g1 = nmf_kl_rule(g1, acc1, cs1, l1, l2);
        g0 = __shfl(g0, lane % G);
        g1 = __shfl(g1, lane % G);
        if (++upd >= inner) break;
    }
    if (sub == 0) *reinterpret_cast<double2*>(Gm + int64_t(item.row) * KP + c0) = make_double2(g0, g1);
}

template <int KP, bool CONST>
__global__ __launch_bounds__(256) void k_nmf_kl_split(const CsrSplit* __restrict__ splits, int64_t n_splits, const double* __restrict__ part,
                                                      const double* __restrict__ tpart, double* __restrict__ Gm,
                                                      const double* __restrict__ csum, int k, double gconst, double l1, double l2, int inner,
                                                      double* __restrict__ terms) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t s = int64_t(blockIdx.x) * 4 + wave;
    if (s >= n_splits) return;
    const CsrSplit sp = splits[s];
    if (inner == 0) {
        if (lane == 0) {
            double sum = 0.0;
            for (int i = 0; i < sp.count; ++i) sum += tpart[int64_t(sp.first_slot) + i];
            terms[sp.row] = sum;
        }
        return;
    }
    if (lane < KP) {
        double sum = 0.0;
        for (int i = 0; i < sp.count; ++i) sum += part[(int64_t(sp.first_slot) + i) * KP + lane];
        const double g = CONST ? (lane < k ? gconst : 0.0) : Gm[int64_t(sp.row) * KP + lane];
        Gm[int64_t(sp.row) * KP + lane] = nmf_kl_rule(g, sum, csum[lane], l1, l2);
    }
}

// slab[b] = { colsum over workgroup b's rows of G (KP), sum of terms over its rows }.  Thread t holds column t mod KP of the rows
// b RL + t / KP, stride gridDim RL (RL = 256 / KP); the RL partial columns are added in order by the first KP threads.
constexpr int NMF_KL_MAX_WG = 256;
template <int KP>
__global__ __launch_bounds__(256) void k_nmf_kl_colsum(const double* __restrict__ Gm, int64_t rows, const double* __restrict__ terms,
                                                       double* __restrict__ slab) {
    constexpr int RL = 256 / KP;
    __shared__ double red[256];
    const int tid = threadIdx.x, j = tid % KP, rl = tid / KP;
    double s = 0.0;
    for (int64_t r = int64_t(blockIdx.x) * RL + rl; r < rows; r += int64_t(gridDim.x) * RL) s += Gm[r * KP + j];
    red[tid] = s;
    __syncthreads();
    double* out = slab + int64_t(blockIdx.x) * (KP + 1);
    if (tid < KP) {
        double a = 0.0;
        for (int i = 0; i < RL; ++i) a += red[i * KP + tid];
        out[tid] = a;
    }
    __syncthreads();
    double ts = 0.0;
    if (terms)
        for (int64_t r = int64_t(blockIdx.x) * 256 + tid; r < rows; r += int64_t(gridDim.x) * 256) ts += terms[r];
    red[tid] = ts;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) out[KP] = red[0];
}

template <class T>
__global__ __launch_bounds__(256) void k_nmf_kl_vsum(const T* __restrict__ val, int64_t nnz, double* __restrict__ part) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int64_t i = int64_t(blockIdx.x) * 256 + t; i < nnz; i += int64_t(gridDim.x) * 256) {
        const double v = (double)val[i];
        if (v > NMF_EPS) s += v;
    }
    red[t] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    if (t == 0) part[blockIdx.x] = red[0];
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------------
bool op_nmf_kl_vsum(Dev* d, int dt, const void* val, int64_t nnz, double* out1) {
    if (nnz < 1) { dev_memset(d, out1, 0, sizeof(double)); return true; }
    const int g = (int)std::min<int64_t>(cdiv64(nnz, 256), 1024);
    double* part = (double*)dev_alloc(d, sizeof(double) * size_t(g));
    DISPATCH_T(dt, hipLaunchKernelGGL((k_nmf_kl_vsum<T>), dim3(g), dim3(256), 0, d->stream, (const T*)val, nnz, part));
    launch_check();
    hipLaunchKernelGGL(k_nmf_slabsum, dim3(1), dim3(256), 0, d->stream, (const double*)part, g, int64_t(1), out1);
    launch_check();
    dev_free(d, part);
    return true;
}

bool op_nmf_kl_colsum(Dev* d, const double* G, int64_t rows, int64_t kp, const double* terms, double* colsum_term) {
    if (rows < 1 || (kp != 16 && kp != 32 && kp != 64) || !G || !colsum_term) return false;
    const int g = (int)std::min<int64_t>(cdiv64(rows, 256), NMF_KL_MAX_WG);
    const int64_t count = kp + 1;
    double* slab = (double*)dev_alloc(d, sizeof(double) * size_t(g) * count);
    if (kp == 16) hipLaunchKernelGGL(k_nmf_kl_colsum<16>, dim3(g), dim3(256), 0, d->stream, G, rows, terms, slab);
    else if (kp == 32) hipLaunchKernelGGL(k_nmf_kl_colsum<32>, dim3(g), dim3(256), 0, d->stream, G, rows, terms, slab);
    else hipLaunchKernelGGL(k_nmf_kl_colsum<64>, dim3(g), dim3(256), 0, d->stream, G, rows, terms, slab);
    launch_check();
    hipLaunchKernelGGL(k_nmf_slabsum, dim3(1), dim3(256), 0, d->stream, (const double*)slab, g, count, colsum_term);
    launch_check();
    dev_free(d, slab);
    return true;
}

template <class T, int G, bool CONST>
static void nmf_kl_launch(Dev* d, const CsrImage& img, const double* F, double* Gm, const double* csum, int k, double gconst, double l1, double l2,
                          int inner, double* part, double* tpart, double* terms) {
    hipLaunchKernelGGL((k_nmf_kl_sweep<T, G, CONST>), dim3((unsigned)cdiv64(img.n_items, 4)), dim3(256), 0, d->stream, img.items, img.n_items,
                       img.idx, (const T*)img.val, F, Gm, csum, k, gconst, l1, l2, inner, part, tpart, terms);
    launch_check();
    if (img.n_splits) {
        hipLaunchKernelGGL((k_nmf_kl_split<2 * G, CONST>), dim3((unsigned)cdiv64(img.n_splits, 4)), dim3(256), 0, d->stream, img.splits,
                           img.n_splits, (const double*)part, (const double*)tpart, Gm, csum, k, gconst, l1, l2, inner, terms);
        launch_check();
    }
}
template <class T, int G>
static void nmf_kl_const(Dev* d, bool from_const, const CsrImage& img, const double* F, double* Gm, const double* csum, int k, double gconst,
                         double l1, double l2, int inner, double* part, double* tpart, double* terms) {
    // an image with split rows takes its updates one launch pair at a time: every row, split or whole, is updated once per pair
    const int pairs = img.n_splits && inner > 1 ? inner : 1, each = pairs > 1 ? 1 : inner;
    for (int p = 0; p < pairs; ++p) {
        if (from_const && p == 0) nmf_kl_launch<T, G, true>(d, img, F, Gm, csum, k, gconst, l1, l2, each, part, tpart, terms);
        else nmf_kl_launch<T, G, false>(d, img, F, Gm, csum, k, gconst, l1, l2, each, part, tpart, terms);
    }
}

bool op_nmf_kl_sweep_csr(Dev* d, int dt, const CsrImage& img, int64_t k, int64_t kp, const double* F, double* G, const double* csum,
                         bool from_const, double gconst, double l1, double l2, int64_t inner, double* colsum_term) {
    if (k < 1 || k > 64 || kp != nmf_csr_padded_k(k) || img.rows < 1 || !F || !G || !csum || !aligned16(F) || !aligned16(G) || inner < 0 ||
        inner > (int64_t(1) << 30) || (inner == 0 && (from_const || !colsum_term)))
        return false;
    csr_check_grid(img);
    double* part = img.n_slots && inner > 0 ? (double*)dev_alloc(d, sizeof(double) * size_t(img.n_slots) * kp) : nullptr;
    double* tpart = img.n_slots && inner == 0 ? (double*)dev_alloc(d, sizeof(double) * size_t(img.n_slots)) : nullptr;
    double* terms = inner == 0 ? (double*)dev_alloc(d, sizeof(double) * size_t(img.rows)) : nullptr;
    TagScope ts(d);
#define PETAL_NMF_KL_SWEEP(Gv) DISPATCH_T(dt, (nmf_kl_const<T, Gv>(d, from_const, img, F, G, csum, (int)k, gconst, l1, l2, (int)inner, part, tpart, terms)))
    if (kp == 16) PETAL_NMF_KL_SWEEP(8);
    else if (kp == 32) PETAL_NMF_KL_SWEEP(16);
    else PETAL_NMF_KL_SWEEP(32);
#undef PETAL_NMF_KL_SWEEP
    ts.stop();
    if (colsum_term) op_nmf_kl_colsum(d, G, img.rows, kp, terms, colsum_term);
    if (part) dev_free(d, part);
    if (tpart) dev_free(d, tpart);
    if (terms) dev_free(d, terms);
    return true;
}

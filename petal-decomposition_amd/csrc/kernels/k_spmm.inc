// k_spmm.inc -- sparse (CSR) times tall-skinny dense, the two X-streaming products of RandomizedPca on sparse data
// (include/petal_hip_sparse.h; an extension beyond the crate).  Part of hip_ops.hip.
//
//   k_spmm<T, G>       out[r, :] = sum_t val[t] P[idx[t], :]  (- a[r] s[:]) over one image of the matrix.  X^T . Z is the same kernel on
//                      the transposed image.  ONE WAVE PER WORK ITEM (at most PETAL_CSR_ITEM_NNZ nonzeros of one row): the item's
//                      indices and values are loaded coalesced, 64 at a time, and handed round by lane shuffles; G lanes hold one
//                      gathered row of P in 16-byte loads and every sub-group keeps four such rows in flight: 256 / G nonzeros per wave.
//                      fp64 accumulators (the products of two fp32 values are exact in them).  Sub-group g takes the nonzeros at
//                      positions g, g + 64 / G, ... of every 64, the sub-groups are added by a fixed shuffle tree: the summation order
//                      is a function of the data alone.  More columns than G lanes hold: blockIdx.y walks the column panels.
//   k_spmm_combine<T>  the rows that were split into several items: their fp64 partial rows are added in item order, then the same
//                      epilogue.  No atomics anywhere.
//   k_csr_rowstats<T>  sum and sum of squares of every image row (the column statistics, on the transposed image), same items.
//   k_tall_small<T>    out = M . S for a tall iterate M (rows x K, in the data's type) and a small fp64 matrix S (K x N): the re-basing
//                      M R^-1 and U = Q Uh of the sparse fit.  Every product and sum in fp64 whatever the ctx's GEMM mode: the sparse
//                      fit never touches a bf16 plane.  S sits in LDS, a thread holds one row of M's panel and 8 output columns.
//
// The gather of P's rows bounds the kernel (4 N bytes per nonzero against 8 for the index and the value), not the arithmetic.

template <class T> struct SpmmVec;
template <> struct SpmmVec<float> { typedef float4 V; };
template <> struct SpmmVec<double> { typedef double2 V; };
__device__ __forceinline__ double spmm_elem(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }
__device__ __forceinline__ double spmm_elem(const double2& v, int e) { return e == 0 ? v.x : v.y; }
__device__ __forceinline__ float4 spmm_pack(const double* r, float) { return make_float4(float(r[0]), float(r[1]), float(r[2]), float(r[3])); }
__device__ __forceinline__ double2 spmm_pack(const double* r, double) { return make_double2(r[0], r[1]); }

template <class T, int G>
__global__ __launch_bounds__(256) void k_spmm(const CsrItem* __restrict__ items, int64_t n_items, const int32_t* __restrict__ idx,
                                              const T* __restrict__ val, const T* __restrict__ P, int64_t N, int64_t ldp,
                                              const double* __restrict__ a, const double* __restrict__ s, T* __restrict__ out,
                                              int64_t ldo, double* __restrict__ part) {
    typedef typename SpmmVec<T>::V V;
    constexpr int VEC = 16 / int(sizeof(T)), NSUB = 64 / G;
    const int lane = threadIdx.x & 63, sub = lane / G;
    const int64_t it = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (it >= n_items) return;                        // (whole waves leave: the shuffles below see all 64 lanes)
    const CsrItem item = items[it];
    const int64_t c0 = (int64_t(blockIdx.y) * G + lane % G) * VEC;
    const bool active = c0 < N;                       // (N is a multiple of 16: a lane's vector is inside or outside as a whole)
    const T* Pc = P + (active ? c0 : 0);
    double acc[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) acc[e] = 0.0;
    for (int base = 0; base < item.count; base += 64) {
        const int cnt = min(64, item.count - base);
        int my_i = 0;
        double my_v = 0.0;
        if (lane < cnt) { my_i = idx[item.first + base + lane]; my_v = double(val[item.first + base + lane]); }
        for (int j = 0; j < cnt; j += 4 * NSUB) {     // four gathered rows in flight per sub-group
            V p[4];
            double v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int src = (j + u * NSUB + sub) & 63;   // (a position past the item reads SOME row that exists -- row 0 or one of the item's -- and is not added)
                v[u] = __shfl(my_v, src);
                p[u] = *reinterpret_cast<const V*>(Pc + int64_t(__shfl(my_i, src)) * ldp);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (j + u * NSUB + sub < cnt) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) acc[e] = fma(v[u], spmm_elem(p[u], e), acc[e]);
                }
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= G; off >>= 1) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] += __shfl_down(acc[e], off);
    }
    if (sub != 0 || !active) return;
    if (item.slot >= 0) {                             // part of a split row: the partial sums, for k_spmm_combine
        double* pr = part + int64_t(item.slot) * N + c0;
#pragma unroll
        for (int e = 0; e < VEC; ++e) pr[e] = acc[e];
        return;
    }
    if (s) {
        const double ar = a ? a[item.row] : 1.0;
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e] -= ar * s[c0 + e];
    }
    *reinterpret_cast<V*>(out + int64_t(item.row) * ldo + c0) = spmm_pack(acc, T(0));
}

template <class T>
__global__ __launch_bounds__(256) void k_spmm_combine(const CsrSplit* __restrict__ splits, int64_t n_splits, const double* __restrict__ part,
                                                      int64_t N, const double* __restrict__ a, const double* __restrict__ s,
                                                      T* __restrict__ out, int64_t ldo) {
    const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
    if (t >= n_splits * N) return;
    const CsrSplit sp = splits[t / N];
    const int64_t c = t % N;
    double sum = 0.0;
    for (int i = 0; i < sp.count; ++i) sum += part[(int64_t(sp.first_slot) + i) * N + c];
    if (s) sum -= (a ? a[sp.row] : 1.0) * s[c];
    out[int64_t(sp.row) * ldo + c] = T(sum);
}

template <class T>
__global__ __launch_bounds__(256) void k_csr_rowstats(const CsrItem* __restrict__ items, int64_t n_items, const T* __restrict__ val,
                                                      double* __restrict__ stats, double* __restrict__ part) {
    const int lane = threadIdx.x & 63;
    const int64_t it = int64_t(blockIdx.x) * 4 + (threadIdx.x >> 6);
    if (it >= n_items) return;
    const CsrItem item = items[it];
    double s1 = 0.0, s2 = 0.0;
    for (int t = lane; t < item.count; t += 64) {
        const double v = double(val[item.first + t]);
        s1 += v;
        s2 = fma(v, v, s2);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) { s1 += __shfl_down(s1, off); s2 += __shfl_down(s2, off); }
    if (lane != 0) return;
    double* dst = item.slot >= 0 ? part + 2 * int64_t(item.slot) : stats + 2 * int64_t(item.row);
    dst[0] = s1;
    dst[1] = s2;
}

// out (rows x N, ldo, in T) = M (rows x K, ldm, in T) . S (K x N fp64, lds): fp64 accumulation, one form for every GEMM mode.
// A 256-thread workgroup takes 32 rows x (up to) 64 columns: S's 64-column panel goes through LDS in slices of 32 rows of S, thread
// (r = tid / 8, c8 = tid % 8) accumulates row r against columns c8, c8 + 8, ... of the panel (conflict-free LDS reads across c8).
template <class T>
__global__ __launch_bounds__(256) void k_tall_small(const T* __restrict__ M, int64_t rows, int64_t K, int64_t ldm,
                                                    const double* __restrict__ S, int64_t N, int64_t lds, T* __restrict__ out, int64_t ldo) {
    __shared__ double sS[32][64];
    const int tid = threadIdx.x, r = tid >> 3, c8 = tid & 7;
    const int64_t row = int64_t(blockIdx.x) * 32 + r, col0 = int64_t(blockIdx.y) * 64;
    double acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.0;
    for (int64_t k0 = 0; k0 < K; k0 += 32) {
        __syncthreads();
        for (int t = tid; t < 32 * 64; t += 256) {
            const int64_t kk = k0 + (t >> 6), cc = col0 + (t & 63);
            sS[t >> 6][t & 63] = (kk < K && cc < N) ? S[kk * lds + cc] : 0.0;
        }
        __syncthreads();
        if (row < rows) {
            const int kmax = int(min<int64_t>(32, K - k0));
            for (int k = 0; k < kmax; ++k) {
                const double m = double(M[row * ldm + k0 + k]);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = fma(m, sS[k][c8 + 8 * e], acc[e]);
            }
        }
    }
    if (row >= rows) return;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int64_t c = col0 + c8 + 8 * e;
        if (c < N) out[row * ldo + c] = T(acc[e]);
    }
}

bool op_csr_supported(Dev*) { return true; }

static void csr_check_grid(const CsrImage& img) {
    if (cdiv64(img.n_items, 4) >= (int64_t(1) << 31)) throw std::runtime_error("sparse matrix has too many work items for one launch");
}

template <class T, int G>
static void launch_spmm(Dev* d, const CsrImage& img, const void* P, int64_t N, int64_t ldp, const double* a, const double* s, void* out,
                        int64_t ldo, double* part) {
    constexpr int panel = G * (16 / int(sizeof(T)));
    hipLaunchKernelGGL((k_spmm<T, G>), dim3((unsigned)cdiv64(img.n_items, 4), (unsigned)cdiv64(N, panel)), dim3(256), 0, d->stream, img.items,
                       img.n_items, img.idx, (const T*)img.val, (const T*)P, N, ldp, a, s, (T*)out, ldo, part);
}

bool op_csr_gemm(Dev* d, int dt, const CsrImage& img, const void* P, int64_t N, int64_t ldp, const double* a, const double* s, void* out,
                 int64_t ldo) {
    if (img.rows == 0 || N == 0) return true;
    if (N % 16 || ldp % 16 || ldo % 16 || reinterpret_cast<uintptr_t>(P) % 16 || reinterpret_cast<uintptr_t>(out) % 16)
        throw std::invalid_argument("op_csr_gemm: operands must be padded to 16 columns and 16-byte aligned");
    csr_check_grid(img);
    double* part = img.n_slots ? (double*)dev_alloc(d, sizeof(double) * size_t(img.n_slots) * N) : nullptr;
    TagScope ts(d);
    // the fewest lanes per gathered row that hold all N columns (more nonzeros in flight per wave), 32 at the most: then column panels
    const int64_t vecs = N / (16 / int64_t(dtype_size(dt)));
    if (dt == F32) {
        if (vecs <= 4) launch_spmm<float, 4>(d, img, P, N, ldp, a, s, out, ldo, part);
        else if (vecs <= 8) launch_spmm<float, 8>(d, img, P, N, ldp, a, s, out, ldo, part);
        else if (vecs <= 16) launch_spmm<float, 16>(d, img, P, N, ldp, a, s, out, ldo, part);
        else launch_spmm<float, 32>(d, img, P, N, ldp, a, s, out, ldo, part);
    } else {
        if (vecs <= 8) launch_spmm<double, 8>(d, img, P, N, ldp, a, s, out, ldo, part);
        else if (vecs <= 16) launch_spmm<double, 16>(d, img, P, N, ldp, a, s, out, ldo, part);
        else launch_spmm<double, 32>(d, img, P, N, ldp, a, s, out, ldo, part);
    }
    launch_check();
    if (img.n_splits) {
        DISPATCH_T(dt, hipLaunchKernelGGL(k_spmm_combine<T>, dim3((unsigned)cdiv64(img.n_splits * N, 256)), dim3(256), 0, d->stream, img.splits,
                                          img.n_splits, part, N, a, s, (T*)out, ldo));
        launch_check();
    }
    ts.stop();
    if (part) dev_free(d, part);
    return true;
}

bool op_csr_colstats(Dev* d, int dt, const CsrImage& img, double* stats) {
    if (img.rows == 0) return true;
    csr_check_grid(img);
    double* part = img.n_slots ? (double*)dev_alloc(d, sizeof(double) * 2 * size_t(img.n_slots)) : nullptr;
    TagScope ts(d);
    DISPATCH_T(dt, hipLaunchKernelGGL(k_csr_rowstats<T>, dim3((unsigned)cdiv64(img.n_items, 4)), dim3(256), 0, d->stream, img.items, img.n_items,
                                      (const T*)img.val, stats, part));
    launch_check();
    if (img.n_splits) {
        hipLaunchKernelGGL(k_spmm_combine<double>, dim3((unsigned)cdiv64(img.n_splits * 2, 256)), dim3(256), 0, d->stream, img.splits, img.n_splits,
                           part, int64_t(2), (const double*)nullptr, (const double*)nullptr, stats, int64_t(2));
        launch_check();
    }
    ts.stop();
    if (part) dev_free(d, part);
    return true;
}

bool op_tall_times_small(Dev* d, int dt, const void* M, int64_t rows, int64_t K, int64_t ldm, const double* S, int64_t N, int64_t lds,
                         void* out, int64_t ldo) {
    if (rows == 0 || N == 0) return true;
    if (cdiv64(rows, 32) >= (int64_t(1) << 31)) throw std::runtime_error("too many rows for one launch");
    TagScope ts(d);
    DISPATCH_T(dt, hipLaunchKernelGGL(k_tall_small<T>, dim3((unsigned)cdiv64(rows, 32), (unsigned)cdiv64(N, 64)), dim3(256), 0, d->stream,
                                      (const T*)M, rows, K, ldm, S, N, lds, (T*)out, ldo));
    launch_check();
    ts.stop();
    return true;
}

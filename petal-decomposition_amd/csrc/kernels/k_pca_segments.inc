// k_pca_segments.inc -- segmented Pca (include/petal_hip_segments.h; an extension beyond the crate, DESIGN.md sections 4 and 7): one exact
// Pca per run of consecutive rows of a row-sorted matrix, every segment on ONE 256-thread workgroup that takes it from raw rows to
// signed components without leaving its CU.  No atomics, no communication between workgroups, no global scratch shared between
// segments: a segment's results are a function of its rows alone, bit for bit, wherever it sits in a batch.
//
//   a) column means        fp64, rows dealt out to G = 256 / LM thread groups (row r to group r mod G), partial sums added in group order
//   b) centred Gram        C = Xc^T Xc in fp64 FMAs on MB x MB register tiles (thread (ti, tj) of a 16 x 16 grid owns rows ti MB .., columns
//                          tj MB ..), rows staged 64 at a time through LDS, centred and widened on the way in; the FULL matrix is formed
//                          (a_ij and a_ji see the same products in the same order, so it is symmetric bit for bit): wg_jacobi_fast rotates
//                          2 x 2 blocks of the whole matrix.  Its trace is the total variance; a non-finite trace marks the segment bad.
//   c) wg_jacobi_fast<MB>  on C in LDS (odd leading dimension), tol 1e-15, graded; eigenpairs ordered by descending eigenvalue, ties
//                          keep the lower index first
//   d) sigma, and which sigma lie above thr sigma_1 (k_sigma_inv's rule: the others are not flipped, as their U column is zero in pca_fit)
//   e) svd_flip            third pass over the rows: y = xc . V_k from LDS; thread (r, jg) holds row r of each 16- or 32-row chunk and components
//                          jg, jg + JG, ..: its candidate per component is the first row that reaches the largest |y| it saw (strict >, rows
//                          ascending); candidates combine across the chunk's lanes by (|y| larger, then row lower) -- a total order, so the
//                          butterfly's result does not depend on its shape.  y leaves unsigned in this pass and the thread that stored an
//                          element negates it afterwards when its column is flipped.
//   f) outputs             components (signed), means, singular values, total variance in the data's type, status as int32
//
// fp64 FMA on register tiles and not v_mfma_f64_16x16x4_f64: a segment's Gram matrix is n d^2 FMAs (256 k at 1000 x 16), the matrix
// pipe's 4x rate would be spent on one or two tiles per workgroup behind the same LDS staging, the MFMA accumulator layout would need a
// transposing pass before the Jacobi solver, and the register form is the same code for every d <= 64 (DESIGN.md section 4).
//
// Static LDS per instantiation (MB = 1 .. 4 for d <= 16, 32, 48, 64): 12, 26, 45 and 69 KB -- eight workgroups per CU at d <= 16, two at d = 64.

template <int MB>
struct SegGeom {
    static constexpr int LM = 16 * MB, LDM = LM | 1;
    static constexpr int A = LM * LDM;                                     // the Gram matrix; afterwards the row chunks of pass (e)
    static constexpr int W = (LM * LDM > 64 * LM) ? LM * LDM : 64 * LM;    // means partials, the 64-row chunks of pass (b), then V
    static constexpr int RC = MB == 1 ? 16 : 32;                           // rows per chunk in pass (e): RC * (LM | 1) <= A
    static constexpr int JG = 256 / RC;                                    // component groups
    static constexpr int NS = (LM + JG - 1) / JG;                          // components per thread
    static constexpr int G = 256 / LM;                                     // row groups of the means pass
};

constexpr int SEG_META = 8;
template <class T> __device__ __forceinline__ T seg_nan() { return static_cast<T>(__builtin_nan("")); }

// (flatten: wg_jacobi_fast and the violation scan it calls are inlined here -- a call would cost a stack frame, and the kernel keeps no scratch)
template <class T, int MB>
__global__ __launch_bounds__(256) __attribute__((flatten)) void k_pca_segments(const T* __restrict__ X, int64_t ldx, int L, int k, int centering,
                                                      const int64_t* __restrict__ meta, int nseg, double thr) {
    // meta: [comp, means, sing, tvar, status, Y (0: not wanted), -, -] as addresses, offsets[nseg + 1], order[nseg] (int32).  The output
    // addresses are read where they are used: as kernel arguments they would sit in scalar registers through the whole eigen-solve.
    const int64_t* __restrict__ offsets = meta + SEG_META;
    const int* __restrict__ order = reinterpret_cast<const int*>(meta + SEG_META + nseg + 1);
    using S = SegGeom<MB>;
    constexpr int LM = S::LM;
    __shared__ __attribute__((aligned(16))) double sm[LM + S::A + S::W + 3 * LM + 64 + 2];
    __shared__ __attribute__((aligned(8))) int smi[3 * LM];
    double* s_cs = sm;                  // wg_jacobi_fast: (c, s) per pair
    double* A = s_cs + LM;
    double* W = A + S::A;
    double* s_mu = W + S::W;
    double* s_sig = s_mu + LM;          // singular values, descending
    double* s_sgn = s_sig + LM;         // svd_flip's sign per component
    double* s_red = s_sgn + LM;         // 64 doubles for wg_jacobi_violation
    double* s_tv = s_red + 64;          // [0] trace
    int* s_pq = smi;                    // wg_jacobi_fast: (p, q) per pair
    int* s_rank = smi + LM;
    int* s_ord = smi + 2 * LM;          // s_ord[rank] = column of V

    const int tid = threadIdx.x;
    const int seg = order[blockIdx.x];
    const int64_t r0 = offsets[seg];
    const int n = (int)(offsets[seg + 1] - r0);
    const T* __restrict__ Xs = X + r0 * ldx;
    const int LD = L | 1;

    // ---- a) column means ---------------------------------------------------------------------------------------------------------
    {
        const int c = tid % LM, g = tid / LM;
        double s = 0.0;
        if (centering && c < L && g < S::G)
            for (int r = g; r < n; r += S::G) s += (double)Xs[(int64_t)r * ldx + c];
        if (g < S::G) W[g * LM + c] = s;
        __syncthreads();
        if (tid < LM) {
            double m = 0.0;
            if (centering && tid < L && n > 0) {
                for (int gg = 0; gg < S::G; ++gg) m += W[gg * LM + tid];
                m /= (double)n;
            }
            s_mu[tid] = m;
        }
        __syncthreads();
    }

    // ---- b) centred Gram matrix ------------------------------------------------------------------------------------------------------
    {
        const int ti = tid >> 4, tj = tid & 15;
        double acc[MB][MB];
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
            for (int j = 0; j < MB; ++j) acc[i][j] = 0.0;
        for (int base = 0; base < n; base += 64) {
            for (int e = tid; e < 64 * LM; e += 256) {
                const int r = e / LM, c = e % LM, row = base + r;
                W[e] = (row < n && c < L) ? (double)Xs[(int64_t)row * ldx + c] - s_mu[c] : 0.0;
            }
            __syncthreads();
            const int rows = min(64, n - base);
#pragma unroll 4
            for (int r = 0; r < rows; ++r) {
                double a[MB], b[MB];
#pragma unroll
                for (int i = 0; i < MB; ++i) { a[i] = W[r * LM + ti * MB + i]; b[i] = W[r * LM + tj * MB + i]; }
#pragma unroll
                for (int i = 0; i < MB; ++i)
#pragma unroll
                    for (int j = 0; j < MB; ++j) acc[i][j] = fma(a[i], b[j], acc[i][j]);
            }
            __syncthreads();
        }
#pragma unroll
        for (int i = 0; i < MB; ++i)
#pragma unroll
            for (int j = 0; j < MB; ++j) {
                const int r = ti * MB + i, c = tj * MB + j;
                if (r < L && c < L) A[r * LD + c] = acc[i][j];
            }
        __syncthreads();
        if (tid < 64) {   // the trace: one wave, a butterfly over the diagonal
            double t = tid < L ? A[tid * LD + tid] : 0.0;
            for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
            if (tid == 0) s_tv[0] = t;
        }
        __syncthreads();
    }
    const double tv = s_tv[0];
    const bool bad = !(fabs(tv) <= 1.79769313486231570e308);   // NaN or infinite
    if (tid < L) reinterpret_cast<T*>(meta[1])[(int64_t)seg * L + tid] = bad ? seg_nan<T>() : (T)s_mu[tid];
    if (tid == 0) { reinterpret_cast<T*>(meta[3])[seg] = bad ? seg_nan<T>() : (T)tv; reinterpret_cast<int*>(meta[4])[seg] = bad ? 1 : 0; }
    if (bad) {   // one bad group must not lose the batch: its results are NaN, the others are untouched
        T* comp_b = reinterpret_cast<T*>(meta[0]) + (int64_t)seg * k * L;
        T* Y = reinterpret_cast<T*>(meta[5]);
        for (int e = tid; e < k * L; e += 256) comp_b[e] = seg_nan<T>();
        if (tid < k) reinterpret_cast<T*>(meta[2])[(int64_t)seg * k + tid] = seg_nan<T>();
        if (Y)
            for (int64_t e = tid; e < (int64_t)n * k; e += 256) Y[r0 * k + e] = seg_nan<T>();
        return;
    }
    if (k == 0) return;

    // ---- c) eigen-solve, descending order ------------------------------------------------------------------------------------------
    double* V = W;
    wg_jacobi_fast<MB>(A, V, L, s_cs, s_cs + LM / 2, s_pq, s_pq + LM / 2, s_red, 1e-15, /*graded=*/true);
    __syncthreads();
    if (tid < L) {
        const double wj = A[tid * LD + tid];
        int rank = 0;
        for (int m = 0; m < L; ++m) {
            const double wm = A[m * LD + m];
            rank += (wm > wj || (wm == wj && m < tid)) ? 1 : 0;
        }
        s_rank[tid] = rank;
        s_ord[rank] = tid;
        s_sig[rank] = sqrt(fmax(wj, 0.0));   // ---- d)
    }
    __syncthreads();

    // ---- e) svd_flip's scan over y = xc . V_k (and y itself, unsigned, when it is wanted) -----------------------------------------------
    {
        constexpr int RC = S::RC, JG = S::JG, NS = S::NS;
        double* Xc = A;   // (the eigenvalues have been read out above)
        T* Y = reinterpret_cast<T*>(meta[5]);
        const int r = tid % RC, jg = tid / RC;
        int oj[NS];
        double best_abs[NS], best_val[NS];
        int best_row[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const int j = jg + JG * s;
            oj[s] = j < k ? s_ord[j] : 0;
            best_abs[s] = 0.0; best_val[s] = 0.0; best_row[s] = 0x7fffffff;
        }
        for (int base = 0; base < n; base += RC) {
            for (int e = tid; e < RC * L; e += 256) {
                const int rr = e / L, c = e - rr * L, row = base + rr;
                Xc[rr * LD + c] = row < n ? (double)Xs[(int64_t)row * ldx + c] - s_mu[c] : 0.0;
            }
            __syncthreads();
            double y[NS];
#pragma unroll
            for (int s = 0; s < NS; ++s) y[s] = 0.0;
            for (int i = 0; i < L; ++i) {
                const double xv = Xc[r * LD + i];
#pragma unroll
                for (int s = 0; s < NS; ++s) y[s] = fma(xv, V[i * LD + oj[s]], y[s]);
            }
            const int row = base + r;
            if (row < n) {
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const int j = jg + JG * s;
                    if (j < k) {
                        const double ay = fabs(y[s]);
                        if (ay > best_abs[s]) { best_abs[s] = ay; best_val[s] = y[s]; best_row[s] = row; }
                        if (Y) Y[(r0 + row) * k + j] = (T)y[s];
                    }
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            double ba = best_abs[s], bv = best_val[s];
            int br = best_row[s];
            for (int off = RC / 2; off > 0; off >>= 1) {
                const double oa = __shfl_xor(ba, off, 64), ov = __shfl_xor(bv, off, 64);
                const int orr = __shfl_xor(br, off, 64);
                if (oa > ba || (oa == ba && orr < br)) { ba = oa; bv = ov; br = orr; }
            }
            const int j = jg + JG * s;
            // (a sigma at or below thr sigma_1 has inverse 0 in pca_fit: a zero column of U, which svd_flip leaves alone)
            if (r == 0 && j < k) s_sgn[j] = (bv < 0.0 && s_sig[j] > thr * s_sig[0] && s_sig[j] > 0.0) ? -1.0 : 1.0;
        }
        __syncthreads();
        if (Y) {   // every thread negates what it stored itself
            for (int base = 0; base < n; base += RC) {
                const int row = base + r;
                if (row < n) {
#pragma unroll
                    for (int s = 0; s < NS; ++s) {
                        const int j = jg + JG * s;
                        if (j < k && s_sgn[j] < 0.0) { T* p = Y + (r0 + row) * k + j; *p = -*p; }
                    }
                }
            }
        }
    }

    // ---- f) outputs ---------------------------------------------------------------------------------------------------------------------
    T* comp_b = reinterpret_cast<T*>(meta[0]) + (int64_t)seg * k * L;
    for (int e = tid; e < k * L; e += 256) {
        const int j = e / L, i = e - j * L;
        comp_b[e] = (T)(s_sgn[j] * V[i * LD + s_ord[j]]);
    }
    if (tid < k) reinterpret_cast<T*>(meta[2])[(int64_t)seg * k + tid] = (T)s_sig[tid];
}

// transform / inverse_transform of a fitted batch: a workgroup takes up to 64 rows of one segment, holds that segment's k x d components
// (widened, M[m][c]: m the reduction index) and its means in LDS and accumulates in fp64; lanes run along the output's columns.
//   FWD:  out[r][j] = sum_i (x[r][i] - mu_i) comp[j][i]            (win = d, wout = k)
//   else: out[r][i] = sum_j y[r][j] comp[j][i] + mu_i              (win = k, wout = d)
template <class T, bool FWD>
__global__ __launch_bounds__(256) void k_seg_project(const T* __restrict__ In, int64_t ldin, const int64_t* __restrict__ offsets,
                                                     const int* __restrict__ cseg, const int64_t* __restrict__ crow,
                                                     const T* __restrict__ comp, const T* __restrict__ means, int k, int d,
                                                     T* __restrict__ Out) {
    __shared__ double M[64 * 65];
    __shared__ double Is[64 * 65];
    __shared__ double s_mu[64];
    const int tid = threadIdx.x;
    const int seg = cseg[blockIdx.x];
    const int64_t row0 = crow[blockIdx.x];
    const int64_t left = offsets[seg + 1] - row0;
    const int rows = left < 64 ? (int)left : 64;
    const int win = FWD ? d : k, wout = FWD ? k : d;
    const T* __restrict__ cb = comp + (int64_t)seg * k * d;
    for (int e = tid; e < k * d; e += 256) {
        const int j = e / d, i = e - j * d;
        M[FWD ? i * 65 + j : j * 65 + i] = (double)cb[e];
    }
    if (tid < d) s_mu[tid] = means ? (double)means[(int64_t)seg * d + tid] : 0.0;
    __syncthreads();
    for (int e = tid; e < rows * win; e += 256) {
        const int r = e / win, c = e - r * win;
        const double v = (double)In[(row0 + r) * ldin + c];
        Is[r * 65 + c] = FWD ? v - s_mu[c] : v;
    }
    __syncthreads();
    const int c = tid & 63, rg = tid >> 6;
    if (c >= wout) return;
    for (int r = rg; r < rows; r += 4) {
        double acc = 0.0;
        for (int m = 0; m < win; ++m) acc = fma(Is[r * 65 + m], M[m * 65 + c], acc);
        Out[(row0 + r) * wout + c] = (T)(FWD ? acc : acc + s_mu[c]);
    }
}

// ---- launchers -------------------------------------------------------------------------------------------------------------------------
constexpr int64_t SEG_MAX_D = 64;

template <class T>
static void launch_pca_segments(Dev* dv, int mb, int grid, const T* X, int64_t ldx, int L, int k, int centering, const int64_t* meta, double thr) {
    switch (mb) {
        case 1: hipLaunchKernelGGL((k_pca_segments<T, 1>), dim3(grid), dim3(256), 0, dv->stream, X, ldx, L, k, centering, meta, grid, thr); break;
        case 2: hipLaunchKernelGGL((k_pca_segments<T, 2>), dim3(grid), dim3(256), 0, dv->stream, X, ldx, L, k, centering, meta, grid, thr); break;
        case 3: hipLaunchKernelGGL((k_pca_segments<T, 3>), dim3(grid), dim3(256), 0, dv->stream, X, ldx, L, k, centering, meta, grid, thr); break;
        default: hipLaunchKernelGGL((k_pca_segments<T, 4>), dim3(grid), dim3(256), 0, dv->stream, X, ldx, L, k, centering, meta, grid, thr); break;
    }
    launch_check();
}

static bool segments_fit_int(const int64_t* offsets, int64_t nseg) {
    if (nseg <= 0 || nseg > 0x7fffffff) return false;
    for (int64_t b = 0; b < nseg; ++b)
        if (offsets[b + 1] - offsets[b] > 0x7fffffff) return false;
    return true;
}

bool op_pca_segments(Dev* dv, int dtype, const void* X, int64_t ldx, int64_t d, const int64_t* offsets, int64_t nseg, int64_t k,
                     bool centering, void* comp, void* means, void* sing, void* tv, int32_t* status, void* Y) {
    if (d < 1 || d > SEG_MAX_D || k < 0 || k > d || !segments_fit_int(offsets, nseg)) return false;
    // the long segments start first: workgroups in descending order of length (ties: ascending index)
    std::vector<int> order(static_cast<size_t>(nseg));
    for (int64_t b = 0; b < nseg; ++b) order[b] = int(b);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return offsets[a + 1] - offsets[a] > offsets[b + 1] - offsets[b]; });
    // one upload: the output addresses, the offsets and the launch order
    std::vector<int64_t> meta(size_t(SEG_META) + size_t(nseg + 1) + size_t((nseg + 1) / 2), 0);
    const void* outs[6] = {comp, means, sing, tv, status, Y};
    for (int i = 0; i < 6; ++i) meta[i] = int64_t(reinterpret_cast<uintptr_t>(outs[i]));
    std::memcpy(meta.data() + SEG_META, offsets, sizeof(int64_t) * size_t(nseg + 1));
    std::memcpy(meta.data() + SEG_META + nseg + 1, order.data(), sizeof(int) * size_t(nseg));
    int64_t* dmeta = static_cast<int64_t*>(dev_alloc(dv, sizeof(int64_t) * meta.size()));
    dev_h2d_async(dv, dmeta, meta.data(), sizeof(int64_t) * meta.size());
    const int mb = int((d + 15) / 16);
    const double thr = dtype == F32 ? 1e-6 : 1e-10;   // op_sigma_inv's thresholds in pca_fit
    if (dtype == F32) launch_pca_segments<float>(dv, mb, int(nseg), static_cast<const float*>(X), ldx, int(d), int(k), centering ? 1 : 0, dmeta, thr);
    else launch_pca_segments<double>(dv, mb, int(nseg), static_cast<const double*>(X), ldx, int(d), int(k), centering ? 1 : 0, dmeta, thr);
    dev_free(dv, dmeta);
    return true;
}

template <bool FWD>
static bool seg_project(Dev* dv, int dtype, const void* In, int64_t ldin, const int64_t* offsets, int64_t nseg, const void* comp,
                        const void* means, int64_t k, int64_t d, void* Out) {
    if (d < 1 || d > SEG_MAX_D || k < 1 || k > SEG_MAX_D || !segments_fit_int(offsets, nseg)) return false;
    std::vector<int> cseg;
    std::vector<int64_t> crow;
    for (int64_t b = 0; b < nseg; ++b)
        for (int64_t r = offsets[b]; r < offsets[b + 1]; r += 64) { cseg.push_back(int(b)); crow.push_back(r); }
    if (cseg.empty()) return true;
    if (cseg.size() > size_t(0x7fffffff)) return false;
    int64_t* doff = static_cast<int64_t*>(dev_alloc(dv, sizeof(int64_t) * size_t(nseg + 1)));
    int* dseg = static_cast<int*>(dev_alloc(dv, sizeof(int) * cseg.size()));
    int64_t* drow = static_cast<int64_t*>(dev_alloc(dv, sizeof(int64_t) * crow.size()));
    dev_h2d_async(dv, doff, offsets, sizeof(int64_t) * size_t(nseg + 1));
    dev_h2d_async(dv, dseg, cseg.data(), sizeof(int) * cseg.size());
    dev_h2d_async(dv, drow, crow.data(), sizeof(int64_t) * crow.size());
    const dim3 grid((unsigned)cseg.size());
    if (dtype == F32)
        hipLaunchKernelGGL((k_seg_project<float, FWD>), grid, dim3(256), 0, dv->stream, static_cast<const float*>(In), ldin, doff, dseg, drow,
                           static_cast<const float*>(comp), static_cast<const float*>(means), int(k), int(d), static_cast<float*>(Out));
    else
        hipLaunchKernelGGL((k_seg_project<double, FWD>), grid, dim3(256), 0, dv->stream, static_cast<const double*>(In), ldin, doff, dseg, drow,
                           static_cast<const double*>(comp), static_cast<const double*>(means), int(k), int(d), static_cast<double*>(Out));
    launch_check();
    dev_free(dv, doff);
    dev_free(dv, dseg);
    dev_free(dv, drow);
    return true;
}
bool op_transform_segments(Dev* dv, int dtype, const void* X, int64_t ldx, const int64_t* offsets, int64_t nseg, const void* comp,
                           const void* means, int64_t k, int64_t d, void* Y) {
    return seg_project<true>(dv, dtype, X, ldx, offsets, nseg, comp, means, k, d, Y);
}
bool op_inverse_transform_segments(Dev* dv, int dtype, const void* Y, int64_t ldy, const int64_t* offsets, int64_t nseg, const void* comp,
                                   const void* means, int64_t k, int64_t d, void* X) {
    return seg_project<false>(dv, dtype, Y, ldy, offsets, nseg, comp, means, k, d, X);
}

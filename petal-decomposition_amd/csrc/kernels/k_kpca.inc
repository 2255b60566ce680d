// k_kpca.inc -- part of the ONE translation unit hip_ops.hip (textually included there, inside namespace petal): kernel PCA
// (include/petal_hip_kpca.h).  The fit side maps the row Gram matrix G to the kernel matrix K element by element and centres it twice
// (k_kmap, k_kmeans, k_kcentre); the transform side is ONE fused pass (k_kapply)
//     out = phi(Xq Xt^T) A'          m query rows against n training rows, A' of any width,
// whose m x n kernel matrix never touches memory, with the row norms it needs (k_krownorm) and the epilogue of transform (k_kfinish).
// ------------------------------------------------------------------------------------------------
// phi(s, na, nb): s = <x, y>, na = |x|^2, nb = |y|^2 (about the centre the caller subtracts).  PETAL_KERNEL_* of petal_hip_kpca.h.
// (laplacian is not here: an L1 distance is not a Gram product)
enum { KP_LINEAR = 0, KP_POLY = 1, KP_RBF = 2, KP_SIGMOID = 3, KP_COSINE = 4 };
struct KSpec { double gamma, coef0; int degree; };

template <int KERNEL>
__device__ __forceinline__ double kphi(double s, double na, double nb, const KSpec& p) {
    if (KERNEL == KP_LINEAR) return s;
    if (KERNEL == KP_POLY) {   // repeated multiplication: integer inputs give exact integers
        const double b = p.gamma * s + p.coef0;
        double v = b;
        for (int t = 1; t < p.degree; ++t) v *= b;
        return v;
    }
    if (KERNEL == KP_RBF) return exp(-p.gamma * fmax(na + nb - 2.0 * s, 0.0));
    if (KERNEL == KP_SIGMOID) return tanh(p.gamma * s + p.coef0);
    const double den = sqrt(na) * sqrt(nb);
    return den > 0.0 ? s / den : 0.0;
}
__device__ __forceinline__ double kphi_rt(int kernel, double s, double na, double nb, const KSpec& p) {
    switch (kernel) {
        case KP_POLY: return kphi<KP_POLY>(s, na, nb, p);
        case KP_RBF: return kphi<KP_RBF>(s, na, nb, p);
        case KP_SIGMOID: return kphi<KP_SIGMOID>(s, na, nb, p);
        case KP_COSINE: return kphi<KP_COSINE>(s, na, nb, p);
        default: return s;
    }
}

// K[i][j] <- phi(G_ij, G_ii, G_jj) in place on the leading n x n block (ldk), dg = the diagonal of G set aside beforehand (a block
// overwrites its own diagonal entry while others still need it).  One workgroup per row; rowsum[i] = sum_j K_ij in a FIXED order:
// thread t adds its columns t, t + 256, ... in order, the 256 partial sums go through an LDS tree.  No atomics.
__global__ __launch_bounds__(256) void k_kmap(int kernel, KSpec spec, double* __restrict__ K, int n, int64_t ldk, const double* __restrict__ dg,
                                              double* __restrict__ rowsum) {
    __shared__ double red[256];
    const int i = blockIdx.x, t = threadIdx.x;
    double* row = K + (int64_t)i * ldk;
    const double di = dg[i];
    double s = 0.0;
    for (int j = t; j < n; j += 256) {
        const double v = kphi_rt(kernel, row[j], di, dg[j], spec);
        row[j] = v;
        s += v;
    }
    red[t] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    if (t == 0) rowsum[i] = red[0];
}

// rbar[i] = rowsum[i] / n, *tbar = (sum_i rbar[i]) / n: one workgroup, the same fixed order.
__global__ __launch_bounds__(256) void k_kmeans(const double* __restrict__ rowsum, int n, double* __restrict__ rbar, double* __restrict__ tbar) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int i = t; i < n; i += 256) {
        const double r = rowsum[i] / (double)n;
        rbar[i] = r;
        s += r;
    }
    red[t] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    if (t == 0) *tbar = red[0] / (double)n;
}

// The double centring: K_ij <- K_ij - rbar_i - rbar_j + tbar on the leading n x n block.
__global__ __launch_bounds__(256) void k_kcentre(double* __restrict__ K, int n, int64_t ldk, const double* __restrict__ rbar,
                                                 const double* __restrict__ tbar) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)n * n) return;
    const int i = (int)(idx / n), j = (int)(idx - (int64_t)i * n);
    double* p = K + (int64_t)i * ldk + j;
    *p = ((*p - rbar[i]) - rbar[j]) + *tbar;
}

// nrm[r] = sum_f (x_rf - c_f)^2, x widened to fp64 before c is subtracted: one wave per row, 16-byte loads, the lanes' partial sums
// through a fixed butterfly.  dp a multiple of 16.
template <class T>
__global__ __launch_bounds__(256) void k_krownorm(const T* __restrict__ X, int64_t ldx, int64_t rows, int64_t dp, const double* __restrict__ c,
                                                  double* __restrict__ nrm) {
    constexpr int E = 16 / (int)sizeof(T);
    typedef T txe __attribute__((ext_vector_type(E)));
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const T* xp = X + r * ldx;
    double s = 0.0;
    for (int64_t f = (int64_t)E * lane; f < dp; f += 64 * E) {
        const txe x = *reinterpret_cast<const txe*>(xp + f);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const double v = (double)x[e] - c[f + e];
            s += v * v;
        }
    }
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) s += __shfl_xor(s, w, 64);
    if (lane == 0) nrm[r] = s;
}

// The fused pass.  v_mfma_f64_16x16x4_f64 takes A as "row = lane & 15, k = lane >> 4", B as "k = lane >> 4, column = lane & 15" and
// delivers C as "column = lane & 15, row = (lane >> 4) + 4 reg" (k_row_gram.inc).  The score tile is formed TRANSPOSED: training rows
// are the A operand and query rows the B operand of the first product, so register r of lane (i, q) = (lane & 15, lane >> 4) holds
//     S[query i][train 4 r + q].
// That IS the A-operand form ("row i, k = q") of a second MFMA that contracts over the four training rows 4 r + q, q = 0 .. 3; its B
// operand is A'[train 4 r + q][column i], one coalesced 128-byte row segment per q.  So the four accumulator registers of a score tile
// go through phi and feed four MFMAs of the second product where they lie: no LDS round trip, no shuffle, no m x n matrix.
// A wave owns 32 query rows (two MFMA tiles) and a panel of 16 NP columns of A', and walks ALL training rows in order, 32 at a time
// (2 x 2 score tiles, the inner loop of k_row_gram: 16-byte loads along the feature axis, widened, centred, E MFMAs per step); a
// workgroup is four such waves = 128 query rows; blockIdx.y is the column panel (a wider A' repeats the first product per panel).
// The order of every sum is fixed by the shape alone: the same input gives the same bytes.  No atomics.
// Rows past m or n are clamped on load; phi of a padded TRAINING row is masked to zero (phi(0) = 1 for rbf and poly), padded query rows
// are never stored.  A' (lda) has round_up(n, 32) readable rows and round_up(cols, 16 NP) readable columns, zero beyond n x cols.
// nt / nq: |xt - c|^2 and |xq - c|^2 per row (read by rbf and cosine only).  c: dp doubles (zeros where the caller does not centre).
template <class T, int KERNEL, int NP>
__global__ __launch_bounds__(256) void k_kapply(const T* __restrict__ Xt, int64_t ldt, int n, const T* __restrict__ Xq, int64_t ldq, int64_t m,
                                                int64_t dp, const double* __restrict__ c, const double* __restrict__ nt,
                                                const double* __restrict__ nq, const double* __restrict__ A, int64_t lda, int cols, KSpec spec,
                                                double* __restrict__ out, int64_t ldo) {
    constexpr int E = 16 / (int)sizeof(T);
    constexpr bool NORMS = KERNEL == KP_RBF || KERNEL == KP_COSINE;
    typedef T txe __attribute__((ext_vector_type(E)));
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int64_t q0 = (int64_t)blockIdx.x * 128 + 32 * wave;
    if (q0 >= m) return;   // wave-uniform
    const int col0 = blockIdx.y * 16 * NP;
    const T* bp[2];
    double nqv[2] = {0.0, 0.0};
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int64_t qr = min(q0 + 16 * u + i, m - 1);
        bp[u] = Xq + qr * ldq;
        if (NORMS) nqv[u] = nq[qr];
    }
    f64x4 o[2][NP];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int p = 0; p < NP; ++p) o[u][p] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int t0 = 0; t0 < n; t0 += 32) {
        const T* ap[2];
#pragma unroll
        for (int v = 0; v < 2; ++v) ap[v] = Xt + (int64_t)min(t0 + 16 * v + i, n - 1) * ldt;
        f64x4 acc[2][2];   // [training tile v][query tile u]
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int u = 0; u < 2; ++u) acc[v][u] = f64x4{0.0, 0.0, 0.0, 0.0};
        for (int64_t f = E * q; f < dp; f += 4 * E) {
            txe xa[2], xb[2];
#pragma unroll
            for (int v = 0; v < 2; ++v) xa[v] = *reinterpret_cast<const txe*>(ap[v] + f);
#pragma unroll
            for (int u = 0; u < 2; ++u) xb[u] = *reinterpret_cast<const txe*>(bp[u] + f);
            double cv[E];
#pragma unroll
            for (int e = 0; e < E; e += 2) {
                const f64x2 c2 = *reinterpret_cast<const f64x2*>(c + f + e);
                cv[e] = c2[0];
                cv[e + 1] = c2[1];
            }
            double ad[2][E], bd[2][E];
#pragma unroll
            for (int w = 0; w < 2; ++w)
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    ad[w][e] = (double)xa[w][e] - cv[e];   // widened first, centred in fp64
                    bd[w][e] = (double)xb[w][e] - cv[e];
                }
#pragma unroll
            for (int e = 0; e < E; ++e)
#pragma unroll
                for (int v = 0; v < 2; ++v)
#pragma unroll
                    for (int u = 0; u < 2; ++u) acc[v][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(ad[v][e], bd[u][e], acc[v][u], 0, 0, 0);
        }
#pragma unroll
        for (int v = 0; v < 2; ++v)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int tr = t0 + 16 * v + 4 * r + q;   // < round_up(n, 32): inside A'
                const bool live = tr < n;
                double ntv = 0.0;
                if (NORMS) ntv = nt[min(tr, n - 1)];
                double bv[NP];
#pragma unroll
                for (int p = 0; p < NP; ++p) bv[p] = A[(int64_t)tr * lda + col0 + 16 * p + i];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const double ph = live ? kphi<KERNEL>(acc[v][u][r], nqv[u], ntv, spec) : 0.0;
#pragma unroll
                    for (int p = 0; p < NP; ++p) o[u][p] = __builtin_amdgcn_mfma_f64_16x16x4f64(ph, bv[p], o[u][p], 0, 0, 0);
                }
            }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t row = q0 + 16 * u + 4 * r + q;
            if (row >= m) continue;
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const int col = col0 + 16 * p + i;
                if (col < cols) out[row * ldo + col] = o[u][p][r];
            }
        }
}

// transform's epilogue from the fused pass's output O (m x ldo; columns 0 .. k - 1 = Kq A, column k = the row sums of Kq):
//     Y_ij = O_ij - ra_j - (O_ik / n - tbar) oa_j,   ra = rbar^T A, oa = 1^T A,   rounded ONCE to the data's type.
template <class T>
__global__ __launch_bounds__(256) void k_kfinish(const double* __restrict__ O, int64_t ldo, int64_t m, int k, const double* __restrict__ ra,
                                                 const double* __restrict__ oa, double n, const double* __restrict__ tbar, T* __restrict__ Y,
                                                 int64_t ldy) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= m * k) return;
    const int64_t i = idx / k;
    const int j = (int)(idx - i * k);
    const double* o = O + i * ldo;
    Y[i * ldy + j] = (T)((o[j] - ra[j]) - (o[k] / n - *tbar) * oa[j]);
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------------
bool op_kpca_map(Dev* d, int kernel, double gamma, double coef0, int degree, double* K, int64_t n, int64_t ldk, const double* diag,
                 double* rbar, double* tbar) {
    if (n < 1 || n > (int64_t(1) << 20) || kernel < KP_LINEAR || kernel > KP_COSINE) return false;
    const KSpec spec{gamma, coef0, degree};
    double* rowsum = (double*)dev_alloc(d, sizeof(double) * size_t(n));
    hipLaunchKernelGGL(k_kmap, dim3((unsigned)n), dim3(256), 0, d->stream, kernel, spec, K, (int)n, ldk, diag, rowsum);
    launch_check();
    hipLaunchKernelGGL(k_kmeans, dim3(1), dim3(256), 0, d->stream, (const double*)rowsum, (int)n, rbar, tbar);
    launch_check();
    hipLaunchKernelGGL(k_kcentre, dim3((unsigned)cdiv64(n * n, 256)), dim3(256), 0, d->stream, K, (int)n, ldk, (const double*)rbar,
                       (const double*)tbar);
    launch_check();
    dev_free(d, rowsum);
    return true;
}

template <class T, int NP>
static void kapply_launch(Dev* d, int kernel, dim3 grid, const T* Xt, int64_t ldt, int n, const T* Xq, int64_t ldq, int64_t m, int64_t dp,
                          const double* c, const double* nt, const double* nq, const double* A, int64_t lda, int cols, KSpec spec, double* out,
                          int64_t ldo) {
#define PETAL_KAPPLY(KN) hipLaunchKernelGGL((k_kapply<T, KN, NP>), grid, dim3(256), 0, d->stream, Xt, ldt, n, Xq, ldq, m, dp, c, nt, nq, A, lda, \
                                            cols, spec, out, ldo)
    switch (kernel) {
        case KP_POLY: PETAL_KAPPLY(KP_POLY); break;
        case KP_RBF: PETAL_KAPPLY(KP_RBF); break;
        case KP_SIGMOID: PETAL_KAPPLY(KP_SIGMOID); break;
        case KP_COSINE: PETAL_KAPPLY(KP_COSINE); break;
        default: PETAL_KAPPLY(KP_LINEAR); break;
    }
#undef PETAL_KAPPLY
}

bool op_kernel_apply(Dev* d, int dt, const void* Xt, int64_t n, int64_t ldt, const void* Xq, int64_t m, int64_t ldq, int64_t dp,
                     const double* centre, const double* nt, int kernel, double gamma, double coef0, int degree, const double* A, int64_t lda,
                     int64_t cols, double* out, int64_t ldo) {
    // 16-byte loads along the feature axis of both matrices: the layout every ingested matrix has (anything else: the caller's fallback)
    const int64_t el = dt == F32 ? 4 : 2;
    if (n < 1 || n > (int64_t(1) << 24) || m < 1 || m > (int64_t(1) << 30) || cols < 1 || cols > (int64_t(1) << 20) || dp < 16 || dp % 16 ||
        ldt < dp || ldt % el || ldq < dp || ldq % el || !aligned16(Xt) || !aligned16(Xq) || !centre || !aligned16(centre) ||
        kernel < KP_LINEAR || kernel > KP_COSINE || lda < cdiv64(cols, 64) * 64 || ldo < cols)
        return false;
    const KSpec spec{gamma, coef0, degree};
    const bool norms = kernel == KP_RBF || kernel == KP_COSINE;
    double *nq = nullptr, *ntown = nullptr;
    if (norms) {
        nq = (double*)dev_alloc(d, sizeof(double) * size_t(m));
        DISPATCH_T(dt, hipLaunchKernelGGL((k_krownorm<T>), dim3((unsigned)cdiv64(m, 4)), dim3(256), 0, d->stream, (const T*)Xq, ldq, m, dp, centre, nq));
        launch_check();
        if (!nt) {
            ntown = (double*)dev_alloc(d, sizeof(double) * size_t(n));
            DISPATCH_T(dt, hipLaunchKernelGGL((k_krownorm<T>), dim3((unsigned)cdiv64(n, 4)), dim3(256), 0, d->stream, (const T*)Xt, ldt, n, dp, centre, ntown));
            launch_check();
            nt = ntown;
        }
    }
    const int np = cols <= 32 ? 2 : 4;   // a panel of 32 or 64 columns of A'
    const dim3 grid((unsigned)cdiv64(m, 128), (unsigned)cdiv64(cols, 16 * np));
    TagScope ts(d);
    if (np == 2) DISPATCH_T(dt, (kapply_launch<T, 2>(d, kernel, grid, (const T*)Xt, ldt, (int)n, (const T*)Xq, ldq, m, dp, centre, nt, nq, A, lda, (int)cols, spec, out, ldo)));
    else DISPATCH_T(dt, (kapply_launch<T, 4>(d, kernel, grid, (const T*)Xt, ldt, (int)n, (const T*)Xq, ldq, m, dp, centre, nt, nq, A, lda, (int)cols, spec, out, ldo)));
    launch_check();
    ts.stop();
    if (nq) dev_free(d, nq);
    if (ntown) dev_free(d, ntown);
    return true;
}

bool op_kpca_finish(Dev* d, int dt, const double* O, int64_t ldo, int64_t m, int64_t k, const double* ra, const double* oa, double n,
                    const double* tbar, void* Y, int64_t ldy) {
    if (m < 1 || k < 1) return false;
    DISPATCH_T(dt, hipLaunchKernelGGL((k_kfinish<T>), dim3((unsigned)cdiv64(m * k, 256)), dim3(256), 0, d->stream, O, ldo, m, (int)k, ra, oa, n, tbar, (T*)Y, ldy));
    launch_check();
    return true;
}

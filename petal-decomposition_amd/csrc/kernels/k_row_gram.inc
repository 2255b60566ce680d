// k_row_gram.inc -- part of the ONE translation unit hip_ops.hip (textually included there, inside namespace petal): the ROW Gram
// matrix of exact Pca's dual route on wide data (n < d; include/petal_hip_wide.h),
//     K[i][i'] = sum_j (x_ij - c_j)(x_i'j - c_j),
// the one Gram product of the library that contracts over the contiguous FEATURE axis of a row-major X (k_atb_f64, k_gram_stream,
// k_gram5 contract over rows), with its fixed-order slab sum (k_row_gram_sum) and launcher.
// ------------------------------------------------------------------------------------------------
// v_mfma_f64_16x16x4_f64 takes A as "row i = lane & 15, k = lane >> 4" and B as "k = lane >> 4, column = lane & 15": for K = Xc Xc^T both
// operands are "row of X by lane & 15, feature by lane >> 4".  A lane therefore fetches 16 contiguous bytes of its row -- E = 4 floats or
// 2 doubles -- and element e of that fetch feeds MFMA e on both sides: MFMA e contracts over the features f + E q + e, q = 0 .. 3, the
// same four on either side, and the E MFMAs of a step cover 4 E consecutive features.  A wave owns a 32 x 32 tile of K (2 x 2 MFMA
// tiles); only tiles on or above the diagonal exist (row block a keeps the blocks b >= a), and a diagonal tile's B fragments ARE its
// A fragments.  x is widened to fp64 BEFORE c is subtracted (k_gram_stream's arithmetic), every product and sum is fp64.
// Rows past n are clamped to row n - 1 and their outputs never stored.  The feature range is a multiple of 16 (the padded width of an
// ingested matrix: the padding columns hold zeros and so does the centre there), cut into chunks of a multiple of 16: blockIdx.z owns
// one chunk and writes its own n x n slab (upper wave tiles only).
template <class T, bool CENTER>
__global__ __launch_bounds__(256) void k_row_gram(const T* __restrict__ X, int64_t ldx, int n, int64_t dp, const double* __restrict__ c,
                                                  int64_t chunk, double* __restrict__ part) {
    constexpr int E = 16 / (int)sizeof(T);
    typedef T txe __attribute__((ext_vector_type(E)));
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int nb = (n + 31) / 32;
    int t = blockIdx.x * 4 + wave, a = 0;
    for (;;) {   // row block a keeps the tiles b = a .. nb - 1
        const int kept = nb - a;
        if (kept <= 0) return;
        if (t < kept) break;
        t -= kept;
        ++a;
    }
    const int b = a + t;
    const bool diag = a == b;   // wave-uniform
    const int r0 = 32 * a, c0 = 32 * b;
    const T* ap[2];
    const T* bp[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        ap[u] = X + (int64_t)min(r0 + 16 * u + i, n - 1) * ldx;
        bp[u] = X + (int64_t)min(c0 + 16 * u + i, n - 1) * ldx;
    }
    const int64_t fbeg = (int64_t)blockIdx.z * chunk, fend = min(dp, fbeg + chunk);
    f64x4 acc[2][2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int64_t f = fbeg + E * q; f < fend; f += 4 * E) {
        txe xa[2], xb[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) xa[u] = *reinterpret_cast<const txe*>(ap[u] + f);
        if (!diag) {
#pragma unroll
            for (int u = 0; u < 2; ++u) xb[u] = *reinterpret_cast<const txe*>(bp[u] + f);
        }
        double cv[E];
        if (CENTER) {
#pragma unroll
            for (int e = 0; e < E; e += 2) {
                const f64x2 c2 = *reinterpret_cast<const f64x2*>(c + f + e);
                cv[e] = c2[0];
                cv[e + 1] = c2[1];
            }
        }
        double ad[2][E], bd[2][E];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int e = 0; e < E; ++e) {
                ad[u][e] = (double)xa[u][e];          // widened first, centred in fp64
                if (CENTER) ad[u][e] -= cv[e];
                if (diag) bd[u][e] = ad[u][e];
                else {
                    bd[u][e] = (double)xb[u][e];
                    if (CENTER) bd[u][e] -= cv[e];
                }
            }
#pragma unroll
        for (int e = 0; e < E; ++e)
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int v = 0; v < 2; ++v) acc[u][v] = __builtin_amdgcn_mfma_f64_16x16x4f64(ad[u][e], bd[v][e], acc[u][v], 0, 0, 0);
    }
    double* out = part + (int64_t)blockIdx.z * n * n;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = r0 + 16 * u + 4 * r + q;
            if (row >= n) continue;
#pragma unroll
            for (int v = 0; v < 2; ++v) {
                const int col = c0 + 16 * v + i;
                if (col < n) out[(int64_t)row * n + col] = acc[u][v][r];
            }
        }
}

// K[i][j] = K[j][i] = the sum over the slabs of element (i, j), i <= j, in a FIXED order: four running sums take every fourth slab
// each (loads in flight instead of one chain of dependent latencies) and are added as (s0 + s1) + (s2 + s3).  Nothing outside the
// leading n x n block of K (ldk) is written.
__global__ __launch_bounds__(256) void k_row_gram_sum(const double* __restrict__ part, int nslab, int n, double* __restrict__ K, int64_t ldk) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x, nn = (int64_t)n * n;
    if (idx >= nn) return;
    const int i = (int)(idx / n), j = (int)(idx - (int64_t)i * n);
    if (i > j) return;
    const double* src = part + idx;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    int z = 0;
    for (; z + 3 < nslab; z += 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += src[(int64_t)(z + k) * nn];
    }
    for (int k = 0; z < nslab; ++z, ++k) s[k] += src[(int64_t)z * nn];
    const double v = (s[0] + s[1]) + (s[2] + s[3]);
    K[(int64_t)i * ldk + j] = v;
    if (i != j) K[(int64_t)j * ldk + i] = v;
}

// The cut of the feature axis: enough chunks that the upper wave tiles fill the chip four workgroups deep, none shorter than 256
// features (a chunk's slab is written once and read once: n^2 doubles against 256 n elements read), and all slabs within 512 MiB.
static int64_t row_gram_chunks(Dev* d, int64_t n, int64_t dp, int64_t* chunk) {
    const int64_t nb = cdiv64(n, 32), wgs = cdiv64(nb * (nb + 1) / 2, 4);
    int64_t ns = std::max<int64_t>(1, (4 * (int64_t)num_cus(d)) / wgs);
    ns = std::min(ns, std::max<int64_t>(1, dp / 256));
    ns = std::min(ns, std::max<int64_t>(1, (int64_t(1) << 26) / (n * n)));
    *chunk = cdiv64(cdiv64(dp, ns), 16) * 16;
    return cdiv64(dp, *chunk);
}

bool op_row_gram(Dev* d, int dt, const void* X, int64_t n, int64_t dp, int64_t ldx, const double* centre, double* K, int64_t ldk,
                 int64_t* chunks) {
    if (chunks) *chunks = 0;
    // 16-byte loads along the feature axis: the layout every ingested matrix has (anything else: the caller's fallback)
    if (n < 1 || n > (int64_t(1) << 20) || dp < 16 || dp % 16 || ldx < dp || ldx % (dt == F32 ? 4 : 2) || !aligned16(X) ||
        (centre && !aligned16(centre)))
        return false;
    int64_t chunk = 0;
    const int64_t ns = row_gram_chunks(d, n, dp, &chunk);
    const int64_t nb = cdiv64(n, 32), wgs = cdiv64(nb * (nb + 1) / 2, 4);
    double* part = (double*)dev_alloc(d, sizeof(double) * size_t(ns) * n * n);
    const dim3 grid((unsigned)wgs, 1, (unsigned)ns), block(256);
    TagScope ts(d);
    if (centre) DISPATCH_T(dt, hipLaunchKernelGGL((k_row_gram<T, true>), grid, block, 0, d->stream, (const T*)X, ldx, (int)n, dp, centre, chunk, part));
    else DISPATCH_T(dt, hipLaunchKernelGGL((k_row_gram<T, false>), grid, block, 0, d->stream, (const T*)X, ldx, (int)n, dp, centre, chunk, part));
    launch_check();
    ts.stop();
    hipLaunchKernelGGL(k_row_gram_sum, dim3((unsigned)cdiv64(n * n, 256)), dim3(256), 0, d->stream, part, (int)ns, (int)n, K, ldk);
    launch_check();
    dev_free(d, part);
    if (chunks) *chunks = ns;
    return true;
}

// k_ipca.inc -- part of the ONE translation unit hip_ops.hip (textually included there, inside namespace petal): IncrementalPca's
// per-batch pass (k_gram_stream) and the update of the running statistic (k_ipca_merge), with their launchers (include/petal_hip_ipca.h).
// ------------------------------------------------------------------------------------------------
// One pass over a batch X (n rows, M = dp columns, ldx) about a fixed fp64 centre c:
//     G = sum (x - c)(x - c)^T   -> part  (one M x M slab per row chunk; only the wave tiles on or above the diagonal are written)
//     s = sum (x - c)            -> spart (one M-vector per row chunk)
// on v_mfma_f64_16x16x4_f64, with k_atb_f64's symmetric wave-tile enumeration, row-chunk slabs, clamped and masked ragged rows and
// columns.  It differs from k_atb_f64 where IncrementalPca's arithmetic does: x is WIDENED to fp64 before c is subtracted (k_atb_f64
// subtracts in the storage type, the crate's `input - &means`; here that would make the statistic depend on the batching), and the
// column sums come out of the same fragments: the first live wave tile of every 32-row slice a -- the one that reaches the diagonal --
// adds up its A-side operands (columns 32 a .. 32 a + 31), lane by lane over its rows and then over the four row groups of the wave
// in a fixed order.  CENTER = false (centering off): c = 0, no subtraction and no sums.
template <class T, bool CENTER>
__global__ __launch_bounds__(256) void k_gram_stream(const T* __restrict__ X, int64_t ldx, int M, const double* __restrict__ c, int64_t n,
                                                     int64_t chunk, double* __restrict__ part, double* __restrict__ spart) {
    typedef T tx2 __attribute__((ext_vector_type(2)));
    typedef T tx4 __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int gy = (M + 63) / 64;
    int t = blockIdx.x * 4 + wave, a = 0;
    for (;;) {   // (k_atb_f64's enumeration: slice a keeps the panels b >= a / 2)
        const int kept = gy - min(gy, a >> 1);
        if (kept == 0) return;
        if (t < kept) break;
        t -= kept;
        ++a;
    }
    const int m0 = 32 * a, n0 = (min(gy, a >> 1) + t) * 64;
    if (m0 >= M) return;
    const bool sums = CENTER && t == 0;   // wave-uniform
    const int64_t rbeg = (int64_t)blockIdx.z * chunk, rend = min(n, rbeg + chunk);
    const int mc = min(m0 + 2 * i, M - 2), ncl = min(n0 + 4 * i, M - 4);  // clamped: out-of-range outputs are never stored
    const T* ap = X + mc;
    const T* bp = X + ncl;
    double ca[2] = {0.0, 0.0}, cb[4] = {0.0, 0.0, 0.0, 0.0}, sa[2] = {0.0, 0.0};
    if (CENTER) {
        ca[0] = c[mc];
        ca[1] = c[mc + 1];
#pragma unroll
        for (int e = 0; e < 4; ++e) cb[e] = c[ncl + e];
    }
    f64x4 acc[2][4];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[u][e] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int64_t r0 = rbeg; r0 < rend; r0 += 16) {
        tx2 av[4];
        tx4 bv[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int64_t r = r0 + 4 * s + q;
            const int64_t rc = r < rend ? r : rend - 1;
            av[s] = *reinterpret_cast<const tx2*>(ap + rc * ldx);
            bv[s] = *reinterpret_cast<const tx4*>(bp + rc * ldx);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const bool rv = (r0 + 4 * s + q) < rend;
            double ad[2], bd[4];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                ad[u] = (double)av[s][u];          // widened first, centred in fp64
                if (CENTER) ad[u] -= ca[u];
                if (!rv) ad[u] = 0.0;              // a row past the chunk contributes nothing to G or s
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                bd[e] = (double)bv[s][e];
                if (CENTER) bd[e] -= cb[e];   // (not masked: the A side's zero removes the product, and a clamped row is a row of this chunk)
            }
            if (sums) { sa[0] += ad[0]; sa[1] += ad[1]; }
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[u][e] = __builtin_amdgcn_mfma_f64_16x16x4f64(ad[u], bd[e], acc[u][e], 0, 0, 0);
        }
    }
    double* out = part + (int64_t)blockIdx.z * M * M;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 2 * (q + 4 * r) + u;
            if (m >= M) continue;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int col = n0 + 4 * i + e;
                if (col < M) out[(int64_t)m * M + col] = acc[u][e][r];
            }
        }
    if (sums) {   // the four row groups of the wave, in a fixed order: (q0 + q2) + (q1 + q3)
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            sa[u] += __shfl_down(sa[u], 32, 64);
            sa[u] += __shfl_down(sa[u], 16, 64);
        }
        if (q == 0 && m0 + 2 * i + 1 < M) {
            spart[(int64_t)blockIdx.z * M + m0 + 2 * i] = sa[0];
            spart[(int64_t)blockIdx.z * M + m0 + 2 * i + 1] = sa[1];
        }
    }
}

// The update of the statistic, one launch, a 16 x 16 tile of M2 per workgroup (tiles below the diagonal leave at once; both triangles
// are written from the tiles on and above it):
//     M2[i][j] += G[i][j] + alpha u_i u_j,      mu_out[j] = base[j] + beta u_j
// mode 0, a batch:   G = the row-chunk slabs of k_gram_stream (only their upper tiles are read), u = s = the slabs of column sums
//                    (U == nullptr: no centring, u = 0 and mu_out is not written), alpha = -1 / n', beta = 1 / n', base = the centre of
//                    the pass.  mu_out may BE base: entry j is read and written by one thread only.
// mode 1, a handle:  G = the other statistic's M2 (nslab == 1), u = U - base = mean_b - mean_a, alpha = n m / n', beta = m / n' -- the
//                    pairwise form.  mu_out must NOT be base here (every workgroup reads base).
// n: rows seen before, m: rows added, inv = 1 / (n + m).
// The slabs are summed in a FIXED order with loads in flight: four threads per element of G take every fourth slab each (eight loads
// at a time) and their four sums are added in order, eight threads per element of u likewise.  (One thread per element walking all --
// up to 128 -- slabs was a chain of dependent load latencies: 74 us a batch at 15625 x 64 against 50 us for the two-pass path.)
__global__ __launch_bounds__(1024) void k_ipca_merge(double* __restrict__ M2, int dp, const double* __restrict__ G, int nslab, int64_t slab_stride,
                                                     const double* __restrict__ U, const double* base, double* mu_out, int mode, double n,
                                                     double m, double inv) {
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (ti > tj) return;
    __shared__ double u[2][16], su[8][32], red[4][256];
    const int tid = threadIdx.x;
    if (tid < 256) {   // u: 32 entries (16 of the tile's rows, 16 of its columns) x 8 slab lanes
        const int w = tid & 31, pl = tid >> 5;
        const int idx = (w < 16 ? ti : tj) * 16 + (w & 15);
        double v = 0.0;
        if (U) {
            if (mode == 0) for (int z = pl; z < nslab; z += 8) v += U[(int64_t)z * dp + idx];
            else if (pl == 0) v = U[idx] - base[idx];
        }
        su[pl][w] = v;
    }
    const int e = tid & 255, pl = tid >> 8;
    const int r = e >> 4, cj = e & 15;
    const int i = ti * 16 + r, j = tj * 16 + cj;
    double g = 0.0;
    if (i <= j) {
        const double* src = G + (int64_t)i * dp + j;
        int z = pl;
        for (; z + 28 < nslab; z += 32) {
            double v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = src[(int64_t)(z + 4 * k) * slab_stride];
#pragma unroll
            for (int k = 0; k < 8; ++k) g += v[k];
        }
        for (; z < nslab; z += 4) g += src[(int64_t)z * slab_stride];
    }
    red[pl][e] = g;
    __syncthreads();
    if (tid < 32) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) v += su[k][tid];
        u[tid >> 4][tid & 15] = v;
    }
    __syncthreads();
    if (tid >= 256) return;
    const double alpha = mode == 0 ? -inv : n * m * inv, beta = mode == 0 ? inv : m * inv;
    if (i <= j) {
        g = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
        const double v = (M2[(int64_t)i * dp + j] + g) + alpha * (u[0][r] * u[1][cj]);
        M2[(int64_t)i * dp + j] = v;
        if (i != j) M2[(int64_t)j * dp + i] = v;
    }
    if (ti == tj && r == 0 && U) mu_out[j] = base[j] + beta * u[1][cj];
}

bool op_ipca_accumulate(Dev* d, int dt, const void* X, int64_t m, int64_t dp, int64_t ldx, const double* centre, double n_seen, double* M2,
                        double* mean) {
    if (dp < 16 || dp > 1024 || dp % 16 || !aligned16(X) || ldx % (dt == F32 ? 4 : 2)) return false;
    if (m == 0) return true;
    const int active = gram64_sym_workgroups(cdiv(dp, 32), cdiv(dp, 64));
    int64_t chunk = 0;
    const int64_t nsplit = gram64_row_split(m, dp, dp, active, &chunk);
    double* part = (double*)dev_alloc(d, sizeof(double) * size_t(nsplit) * dp * dp);
    double* spart = centre ? (double*)dev_alloc(d, sizeof(double) * size_t(nsplit) * dp) : nullptr;
    const dim3 grid(active, 1, (unsigned)nsplit), block(256);
    TagScope ts(d);
    if (centre) DISPATCH_T(dt, hipLaunchKernelGGL((k_gram_stream<T, true>), grid, block, 0, d->stream, (const T*)X, ldx, (int)dp, centre, m, chunk, part, spart));
    else DISPATCH_T(dt, hipLaunchKernelGGL((k_gram_stream<T, false>), grid, block, 0, d->stream, (const T*)X, ldx, (int)dp, centre, m, chunk, part, spart));
    launch_check();
    ts.stop();
    hipLaunchKernelGGL(k_ipca_merge, dim3(dp / 16, dp / 16), dim3(1024), 0, d->stream, M2, (int)dp, part, (int)nsplit, dp * dp, spart, centre, mean, 0,
                       n_seen, double(m), 1.0 / (n_seen + double(m)));
    launch_check();
    dev_free(d, part);
    if (spart) dev_free(d, spart);
    return true;
}

bool op_ipca_merge(Dev* d, int64_t dp, double n_a, double* M2_a, const double* mean_a, double* mean_out, double n_b, const double* M2_b,
                   const double* mean_b) {
    if (dp < 16 || dp > 1024 || dp % 16) return false;
    hipLaunchKernelGGL(k_ipca_merge, dim3(dp / 16, dp / 16), dim3(1024), 0, d->stream, M2_a, (int)dp, M2_b, 1, dp * dp, mean_b, mean_a, mean_out, 1,
                       n_a, n_b, 1.0 / (n_a + n_b));
    launch_check();
    return true;
}

// k_generic.inc -- part of the ONE translation unit hip_ops.hip (textually included there, inside namespace petal): generic kernels: packing, column scans, slab combines, any-shape fp64-accumulate products.
// ================================================================================================
// generic kernels (any shape, T = float | double, fp64 accumulation)
// ================================================================================================
template <class T>
__global__ void k_pack_strided(const T* __restrict__ src, int64_t n, int64_t d, int64_t rs, int64_t cs, T* __restrict__ dst,
                               int64_t ld, int64_t dpad) {
    const int64_t j = blockIdx.y * (int64_t)blockDim.x + threadIdx.x;
    const int64_t i = blockIdx.x;
    if (j >= dpad) return;
    dst[i * ld + j] = j < d ? src[i * rs + j * cs] : T(0);
}
template <class T>
__global__ void k_unpack_strided(const T* __restrict__ src, int64_t n, int64_t d, int64_t ld, T* __restrict__ dst, int64_t rs,
                                 int64_t cs) {
    const int64_t j = blockIdx.y * (int64_t)blockDim.x + threadIdx.x;
    const int64_t i = blockIdx.x;
    if (j >= d) return;
    dst[i * rs + j * cs] = src[i * ld + j];
}
// (flattened like k_unpack_scaled below: a device input whose width is not a multiple of 16 is copied into the padded layout)
template <class T>
__global__ __launch_bounds__(256) void k_pack_flat(const T* __restrict__ src, int64_t n, int64_t d, int64_t rs, int64_t cs, T* __restrict__ dst,
                                                   int64_t ld, int64_t dpad) {
    const int64_t total = n * dpad;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t e = ((int64_t)blockIdx.x * 4 + u) * 256 + threadIdx.x;
        if (e >= total) return;
        const int64_t i = e / dpad, j = e - i * dpad;
        dst[i * ld + j] = j < d ? src[i * rs + j * cs] : T(0);
    }
}
// the same over a flattened index -- a thread per element, consecutive threads along a row, 1024 elements per workgroup -- with
// an optional per-column factor (fit_transform's sigma_j and svd_flip sign, applied in fp64 as k_scale_cols does).  The row-per-
// workgroup form above launches n workgroups of mostly idle lanes: 1e6 x 64 took 0.25 ms for the scaling and the copy-out each.
template <class T>
__global__ __launch_bounds__(256) void k_unpack_scaled(const T* __restrict__ src, int64_t n, int64_t d, int64_t ld, T* __restrict__ dst,
                                                       int64_t rs, int64_t cs, const double* __restrict__ scale) {
    const int64_t total = n * d;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t e = ((int64_t)blockIdx.x * 4 + u) * 256 + threadIdx.x;
        if (e >= total) return;
        const int64_t i = e / d, j = e - i * d;
        const T v = src[i * ld + j];
        dst[i * rs + j * cs] = scale ? (T)((double)v * scale[j]) : v;
    }
}

// Column scans over a tall row-major matrix, first stage: block = 64 column lanes x 4 row lanes over `rows` rows (the
// loads of a thread are independent: many in flight), row lanes combined through LDS in fixed order.
constexpr int SCAN_RY = 4;
// rows per block of the column scans: ~256 row parts for wide matrices; a narrow one (few 64-column blocks) gets more parts so that
// the launch still puts ~2048 workgroups on the chip (1e6 x 64 on 256 workgroups streamed at 2.1 TB/s)
__host__ inline int64_t scan_rows_per_block(int64_t n, int64_t cols = 512) {
    const int64_t col_blocks = std::max<int64_t>(1, (cols + 63) / 64);
    const int64_t parts = std::min<int64_t>(1024, std::max<int64_t>(256, 2048 / col_blocks));   // (more parts cost the final combine more than they save)
    return std::max<int64_t>(256, (cdiv64(n, parts) + 3) / 4 * 4);
}
// s <- fl(s + v), c += the rounding error of that addition (Knuth's two-sum: exact for any s, v)
__device__ __forceinline__ void two_sum_acc(double& s, double& c, double v) {
    const double t = s + v, b = t - s;
    c += (s - (t - b)) + (v - b);
    s = t;
}
// part_lo (fp64 data's column MEANS only, else null; [nparts][w] like part): the sums are carried as (part, part_lo) pairs, every addition
// a two-sum -- a mean is then good to one rounding, where the plain sums spend three to four (data 40 standard deviations off
// centre: 1.7 eps (|mean| + std) measured, tests/whitening_cases.py).  The sums of squares stay plain.
template <class T, bool SQ>  // SQ: also the column sums of squares, part = [nparts][2 d] = [sums | sums of squares]
__global__ __launch_bounds__(256) void k_colsum_part2(const T* __restrict__ X, int64_t n, int64_t d, int64_t ldx, int64_t rows,
                                                      double* __restrict__ part, double* __restrict__ part_lo) {
    __shared__ double red[SCAN_RY][64], redq[SQ ? SCAN_RY : 1][64];
    if (sizeof(T) == 8 && part_lo) {   // (uniform over the launch; fp32 data's kernel holds none of this)
        __shared__ double redc[SCAN_RY][64];
        const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
        const int64_t j = blockIdx.y * (int64_t)64 + cx;
        const int64_t r0 = (int64_t)blockIdx.x * rows, r1 = min(n, r0 + rows);
        double s0 = 0, s1 = 0, c0 = 0, c1 = 0, q0 = 0, q1 = 0;
        if (j < d) {
            int64_t i = r0 + ry;
            for (; i + SCAN_RY < r1; i += 2 * SCAN_RY) {
                const double v0 = (double)X[i * ldx + j], v1 = (double)X[(i + SCAN_RY) * ldx + j];
                two_sum_acc(s0, c0, v0);
                two_sum_acc(s1, c1, v1);
                if (SQ) { q0 += v0 * v0; q1 += v1 * v1; }
            }
            for (; i < r1; i += SCAN_RY) {
                const double v0 = (double)X[i * ldx + j];
                two_sum_acc(s0, c0, v0);
                if (SQ) q0 += v0 * v0;
            }
        }
        c0 += c1;
        two_sum_acc(s0, c0, s1);
        red[ry][cx] = s0; redc[ry][cx] = c0;
        if (SQ) redq[ry][cx] = q0 + q1;
        __syncthreads();
        if (ry == 0 && j < d) {
            const int64_t w = SQ ? 2 * d : d;
            double s = red[0][cx], c = (redc[0][cx] + redc[1][cx]) + (redc[2][cx] + redc[3][cx]);
            two_sum_acc(s, c, red[1][cx]);
            two_sum_acc(s, c, red[2][cx]);
            two_sum_acc(s, c, red[3][cx]);
            part[(int64_t)blockIdx.x * w + j] = s;
            part_lo[(int64_t)blockIdx.x * w + j] = c;
            if (SQ) {
                part[(int64_t)blockIdx.x * w + d + j] = (redq[0][cx] + redq[1][cx]) + (redq[2][cx] + redq[3][cx]);
                part_lo[(int64_t)blockIdx.x * w + d + j] = 0.0;
            }
        }
        return;
    }
    const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
    const int64_t j = blockIdx.y * (int64_t)64 + cx;
    const int64_t r0 = (int64_t)blockIdx.x * rows, r1 = min(n, r0 + rows);
    double s0 = 0, s1 = 0, s2 = 0, s3 = 0, q0 = 0, q1 = 0, q2 = 0, q3 = 0;
    if (j < d) {
        int64_t i = r0 + ry;
        for (; i + 3 * SCAN_RY < r1; i += 4 * SCAN_RY) {
            const double v0 = (double)X[i * ldx + j], v1 = (double)X[(i + SCAN_RY) * ldx + j];
            const double v2 = (double)X[(i + 2 * SCAN_RY) * ldx + j], v3 = (double)X[(i + 3 * SCAN_RY) * ldx + j];
            s0 += v0; s1 += v1; s2 += v2; s3 += v3;
            if (SQ) { q0 += v0 * v0; q1 += v1 * v1; q2 += v2 * v2; q3 += v3 * v3; }
        }
        for (; i < r1; i += SCAN_RY) {
            const double v0 = (double)X[i * ldx + j];
            s0 += v0;
            if (SQ) q0 += v0 * v0;
        }
    }
    red[ry][cx] = (s0 + s1) + (s2 + s3);
    if (SQ) redq[ry][cx] = (q0 + q1) + (q2 + q3);
    __syncthreads();
    if (ry == 0 && j < d) {
        const int64_t w = SQ ? 2 * d : d;
        part[(int64_t)blockIdx.x * w + j] = (red[0][cx] + red[1][cx]) + (red[2][cx] + red[3][cx]);
        if (SQ) part[(int64_t)blockIdx.x * w + d + j] = (redq[0][cx] + redq[1][cx]) + (redq[2][cx] + redq[3][cx]);
    }
}
template <class T>
__global__ __launch_bounds__(256) void k_absmax_part2(const T* __restrict__ U, int64_t n, int64_t L, int64_t ldu, int64_t rows,
                                                      double* __restrict__ pmax, double* __restrict__ pidx,
                                                      double* __restrict__ psgn) {
    __shared__ double rm[SCAN_RY][64], ri[SCAN_RY][64], rs[SCAN_RY][64];
    const int cx = threadIdx.x & 63, ry = threadIdx.x >> 6;
    const int64_t j = blockIdx.y * (int64_t)64 + cx;
    const int64_t r0 = (int64_t)blockIdx.x * rows, r1 = min(n, r0 + rows);
    double best = -1.0, bi = INFINITY, bs = 1.0;
    if (j < L) {
#pragma unroll 4
        for (int64_t i = r0 + ry; i < r1; i += SCAN_RY) {  // ascending rows, strict '>' keeps the first maximum (pca.rs:830)
            const double v = (double)U[i * ldu + j], a = fabs(v);
            if (a > best) { best = a; bi = (double)i; bs = signbit(v) ? -1.0 : 1.0; }
        }
    }
    rm[ry][cx] = best; ri[ry][cx] = bi; rs[ry][cx] = bs;
    __syncthreads();
    if (ry == 0 && j < L) {
#pragma unroll
        for (int k = 1; k < SCAN_RY; ++k)
            if (rm[k][cx] > best || (rm[k][cx] == best && ri[k][cx] < bi)) { best = rm[k][cx]; bi = ri[k][cx]; bs = rs[k][cx]; }
        const int64_t o = (int64_t)blockIdx.x * L + j;
        pmax[o] = best; pidx[o] = bi; psgn[o] = bs;
    }
}
// out[(e / N) * ldc + e % N] = sum_p part[p * count + e]  (fp64 accumulation, fixed order => deterministic).
// block = 32 elements x 8 part-lanes.
template <class TP>
__global__ __launch_bounds__(256) void k_sum_parts2(const TP* __restrict__ part, int64_t nparts, int64_t count,
                                                    double* __restrict__ out, int64_t N, int64_t ldc, bool accumulate) {
    __shared__ double red[8][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t e = (int64_t)blockIdx.x * 32 + tx;
    double s = 0;
    if (e < count)
        for (int64_t p = ty; p < nparts; p += 8) s += (double)part[p * count + e];
    red[ty][tx] = s;
    __syncthreads();
    if (ty == 0 && e < count) {
        double t = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) t += red[k][tx];
        double* o = out + (e / N) * ldc + (e % N);
        *o = accumulate ? *o + t : t;
    }
}
// the same for fp32 slabs whose count and row length are even: a block owns 128 consecutive outputs (512 B contiguous in
// every slab, one 8-B load per lane), its four waves each take a quarter of the slabs, eight loads in flight
__global__ __launch_bounds__(256) void k_sum_parts4(const float* __restrict__ part, int64_t nparts, int64_t count,
                                                    double* __restrict__ out, int64_t N, int64_t ldc) {
    __shared__ double red[3][64][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t e = ((int64_t)blockIdx.x * 64 + lane) * 2;
    double s0 = 0, s1 = 0;
    if (e < count) {
        const float* src = part + e;
        int64_t p = wave;
        for (; p + 28 < nparts; p += 32) {
            f32x2 v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = *reinterpret_cast<const f32x2*>(src + (p + 4 * k) * count);
#pragma unroll
            for (int k = 0; k < 8; ++k) { s0 += (double)v[k][0]; s1 += (double)v[k][1]; }
        }
        for (; p < nparts; p += 4) {
            const f32x2 v = *reinterpret_cast<const f32x2*>(src + p * count);
            s0 += (double)v[0]; s1 += (double)v[1];
        }
    }
    if (wave > 0) { red[wave - 1][lane][0] = s0; red[wave - 1][lane][1] = s1; }
    __syncthreads();
    if (wave == 0 && e < count) {
#pragma unroll
        for (int w = 0; w < 3; ++w) { s0 += red[w][lane][0]; s1 += red[w][lane][1]; }
        double* o = out + (e / N) * ldc + (e % N);
        o[0] = s0; o[1] = s1;
    }
}
__global__ __launch_bounds__(256) void k_add_scalar_parts(const double* __restrict__ part, int64_t nparts, double* __restrict__ out) {
    __shared__ double red[256];
    double s = 0;
    for (int64_t p = threadIdx.x; p < nparts; p += 256) s += part[p];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] += red[0];
}

template <class T>
__global__ void k_xp_simple(const T* __restrict__ X, int64_t n, int64_t K, int64_t ldx, const T* __restrict__ mu,
                            const double* __restrict__ P, int64_t N, int64_t ldp, const T* __restrict__ bias,
                            T* __restrict__ Z, int64_t ldz, double* __restrict__ ss_part) {
    const int64_t j = blockIdx.y * (int64_t)blockDim.x + threadIdx.x;
    const int64_t i = blockIdx.x;
    double acc = 0, ss = 0;
    const bool want_ss = ss_part != nullptr && blockIdx.y == 0 && threadIdx.x == 0;
    if (j < N || want_ss) {
        for (int64_t k = 0; k < K; ++k) {
            T xv = X[i * ldx + k];
            if (mu) xv = xv - mu[k];
            const double a = (double)xv;
            if (j < N) acc += a * (sizeof(T) == 4 ? (double)(float)P[k * ldp + j] : P[k * ldp + j]);
            ss += a * a;
        }
    }
    if (j < N) Z[i * ldz + j] = (T)(acc + (bias ? (double)bias[j] : 0.0));
    if (want_ss) ss_part[i] = ss;
}

constexpr int ATB_S_ROWS = 256;
template <class T>
__global__ void k_atb_simple(const T* __restrict__ A, int64_t lda, int64_t M, const T* __restrict__ muA,
                             const T* __restrict__ B, int64_t ldb, int64_t N, const T* __restrict__ muB, int64_t n,
                             double* __restrict__ part) {
    const int64_t j = blockIdx.y * (int64_t)blockDim.x + threadIdx.x;
    const int64_t m = blockIdx.z * (int64_t)blockDim.y + threadIdx.y;
    if (j >= N || m >= M) return;
    const int64_t r0 = (int64_t)blockIdx.x * ATB_S_ROWS, r1 = min(n, r0 + ATB_S_ROWS);
    const T ma = muA ? muA[m] : T(0), mb = muB ? muB[j] : T(0);
    double s = 0;
    for (int64_t i = r0; i < r1; ++i) s += (double)(T)(A[i * lda + m] - ma) * (double)(T)(B[i * ldb + j] - mb);
    part[((int64_t)blockIdx.x * M + m) * N + j] = s;
}
// one wave per column: lanes scan the row chunks in order (strict '>' keeps the first maximum, pca.rs:830),
// then a lexicographic (larger |u|, then smaller row) butterfly picks the winner.
__global__ __launch_bounds__(64) void k_absmax_final(const double* __restrict__ pmax, const double* __restrict__ pidx,
                                                     const double* __restrict__ psgn, int64_t nparts, int64_t L,
                                                     int64_t row_offset, double* __restrict__ omax, double* __restrict__ oidx,
                                                     double* __restrict__ osgn) {
    const int64_t j = blockIdx.x;
    const int lane = threadIdx.x;
    double best = -2.0, bi = INFINITY, bs = 1.0;
    for (int64_t p = lane; p < nparts; p += 64) {
        const double a = pmax[p * L + j];
        if (a > best) { best = a; bi = pidx[p * L + j]; bs = psgn[p * L + j]; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double ob = __shfl_down(best, off, 64), oi = __shfl_down(bi, off, 64), os = __shfl_down(bs, off, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; bs = os; }
    }
    if (lane == 0) { omax[j] = best; oidx[j] = bi + (double)row_offset; osgn[j] = bs; }
}
template <class T>
__global__ void k_scale_cols(T* __restrict__ A, int64_t n, int64_t L, int64_t lda, const double* __restrict__ s) {
    const int64_t j = blockIdx.y * (int64_t)blockDim.x + threadIdx.x;
    const int64_t i = blockIdx.x;
    if (j < L) A[i * lda + j] = (T)((double)A[i * lda + j] * s[j]);
}
template <class T>
__global__ void k_logcosh_rows(const T* __restrict__ X, int64_t r, int64_t c, int64_t ldx, T* __restrict__ G, int64_t ldg,
                               double* __restrict__ gp) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= r) return;
    double s = 0;
    for (int64_t j = 0; j < c; ++j) {
        const double g = tanh((double)X[i * ldx + j]);
        G[i * ldg + j] = (T)g;
        s += 1.0 - g * g;
    }
    gp[i] = s;
}


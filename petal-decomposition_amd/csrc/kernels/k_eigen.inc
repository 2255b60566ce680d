// k_eigen.inc -- part of the ONE translation unit hip_ops.hip (textually included there, inside namespace petal): the two-stage symmetric eigen-solver, the polar iteration / FastICA tail, result kernels.
// ================================================================================================
// two-stage symmetric eigen-solver: Householder tridiagonalisation, then per eigenpair (one wave each, spread over the
// chip) multisection on the Sturm count, the eigenvector from the twisted factorisation, and the back-transformation.
// ================================================================================================
// The Jacobi solvers above spend ~1 us per round on a chain of on-chip latencies, (L - 1) rounds per sweep, 4-5 sweeps:
// 0.36 ms at L = 74, 1.8 ms at L = 138, all on ONE workgroup.  Here the only serial part is the reduction to tridiagonal
// form T = Q^T A Q (L - 2 Householder steps on one workgroup); everything after it is independent per eigenpair:
//   lambda_j   64-way multisection of the Sturm count of T (6 bits per pass, 10 passes to fp64 resolution),
//   z_j        twisted factorisation (Parlett-Dhillon): the two Sturm recurrences from the top and from the bottom meet at
//              the index of smallest |gamma|; one sweep each way gives the eigenvector of T without iteration,
//   v_j        = H_0 ... H_{L-3} z_j, the reflectors applied to that one column.
// Accuracy is that of a backward-stable dense method, eps ||A|| absolute in the eigenvalues.  Eigenvectors of eigenvalues
// closer than 1e-10 ||A|| (rank deficiency, exact multiplicities) are not guaranteed orthogonal by this route: k_trieig
// leaves the verdict in `flag` and the Jacobi solver, launched behind it, runs only then (it returns at once otherwise).
// ---- the same reduction for orders beyond the LDS (139 ... 2048), ONE LAUNCH PER STEP on the whole chip (round 4).  k_tridiag
// walks such a matrix with one workgroup and its working copy in global memory: 29 ms at order 512, which is where an exact Pca of
// data without a spectral gap behind its k components ends up (the subspace iteration cannot converge there and the d x d
// covariance is eigen-decomposed in full).  Launch k applies the PENDING rank-2 update of step k - 1 to the rows below row k and, in
// the same pass over each row, forms that row's entry of p_k = tau_k A22 v_k: one pass over the trailing block per step.  Every
// workgroup first rebuilds, redundantly and bit-identically, what the pass needs -- w_{k-1} = p_{k-1} + K v_{k-1} from the vectors
// the previous launch left in global memory, row k as the pending update leaves it, and from it reflector k -- so nothing but
// a launch boundary orders the steps.  Vectors are indexed by absolute column (zeros outside their range).
constexpr int TMW_NV = 8;                                          // orders up to 256 * TMW_NV
__global__ __launch_bounds__(256) void k_tridiag_mw(double* __restrict__ W, int64_t ld, int L, int k, const double* __restrict__ vp_prev,
                                                    double* __restrict__ vp_cur, double* __restrict__ dd, double* __restrict__ ee,
                                                    double* __restrict__ HV, double* __restrict__ tau) {
    extern __shared__ __attribute__((aligned(16))) double sm_mw[];
    double* svp = sm_mw;            // v_{k-1}
    double* swp = svp + L;          // w_{k-1}
    double* svn = swp + L;          // v_k
    double* s_red = svn + L;        // 2 x 4 partial sums
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int red_slot = 0;
    auto block_sum = [&](double a) {                               // to every thread; alternating slots: one barrier per sum
        for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, 64);
        double* slot = s_red + 4 * red_slot;
        red_slot ^= 1;
        if (lane == 0) slot[wv] = a;
        __syncthreads();
        return (slot[0] + slot[1]) + (slot[2] + slot[3]);
    };
    // (a) w_{k-1} = p_{k-1} + K v_{k-1}, K = -tau_{k-1} (p^T v) / 2
    double vq[TMW_NV], pq[TMW_NV];
    double pv = 0;
#pragma unroll
    for (int t = 0; t < TMW_NV; ++t) {
        const int j = tid + 256 * t;
        vq[t] = (k > 0 && j < L) ? vp_prev[j] : 0.0;
        pq[t] = (k > 0 && j < L) ? vp_prev[L + j] : 0.0;
        pv = fma(pq[t], vq[t], pv);
    }
    const double tkp = k > 0 ? tau[k - 1] : 0.0;
    const double Kp = -0.5 * tkp * block_sum(pv);
#pragma unroll
    for (int t = 0; t < TMW_NV; ++t) {
        const int j = tid + 256 * t;
        pq[t] = fma(Kp, vq[t], pq[t]);                            // w_{k-1}
        if (j < L) { svp[j] = vq[t]; swp[j] = pq[t]; }
    }
    __syncthreads();
    // (b) row k as the pending update leaves it (v_{k-1}[k] = 1), and reflector k from it
    const double wk = k > 0 ? swp[k] : 0.0, vk = k > 0 ? svp[k] : 0.0;
    double rq[TMW_NV];
    double sq = 0;
#pragma unroll
    for (int t = 0; t < TMW_NV; ++t) {
        const int j = tid + 256 * t;
        rq[t] = (j >= k && j < L) ? fma(-vk, pq[t], fma(-wk, vq[t], W[(size_t)k * ld + j])) : 0.0;
        sq = fma(j >= k + 2 ? rq[t] : 0.0, j >= k + 2 ? rq[t] : 0.0, sq);
    }
    // (row k's own entries k and k + 1 sit in whichever thread owns those columns: they travel through LDS)
#pragma unroll
    for (int t = 0; t < TMW_NV; ++t) {
        const int j = tid + 256 * t;
        if (j == k) s_red[8] = rq[t];
        if (j == k + 1) s_red[9] = rq[t];
    }
    const double sigma = block_sum(sq);                           // (its barrier also publishes s_red[8 .. 9])
    const double dk = s_red[8], alpha = k + 1 < L ? s_red[9] : 0.0;
    double beta = alpha, tk = 0.0, scale = 0.0;
    if (k + 2 < L && sigma > 0.0) {
        beta = -copysign(sqrt(fma(alpha, alpha, sigma)), alpha);
        tk = (beta - alpha) / beta;
        scale = 1.0 / (alpha - beta);
    }
    const bool refl = k + 2 < L;
#pragma unroll
    for (int t = 0; t < TMW_NV; ++t) {
        const int j = tid + 256 * t;
        const double vj = !refl ? 0.0 : (j == k + 1 ? 1.0 : (j >= k + 2 ? rq[t] * scale : 0.0));
        if (j < L) {
            svn[j] = vj;
            if (blockIdx.x == 0) {
                vp_cur[j] = vj;
                if (refl) HV[(size_t)k * L + j] = vj;
            }
        }
    }
    if (blockIdx.x == 0 && tid == 0) { dd[k] = dk; ee[k] = k + 1 < L ? beta : 0.0; tau[k] = tk; }
    __syncthreads();
    // (c) rows below k: the pending update, and p_k = tau_k A22 v_k from the updated row -- one wave per row
    for (int i = k + 1 + blockIdx.x * 4 + wv; i < L; i += 4 * gridDim.x) {
        double* row = W + (size_t)i * ld;
        const double vi = svp[i], wi = swp[i];
        double acc = 0;
        for (int j = k + 1 + lane; j < L; j += 64) {
            const double nv = fma(-vi, swp[j], fma(-wi, svp[j], row[j]));
            if (k > 0) row[j] = nv;
            acc = fma(nv, svn[j], acc);
        }
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (lane == 0) vp_cur[L + i] = tk * acc;
    }
}

// one wave per eigenpair j (descending): lambda_j, z_j, v_j.  d, e in LDS; q+ / q- / z per wave in LDS.
template <int WPB>
__global__ __launch_bounds__(64 * WPB) void k_trieig(const double* __restrict__ dd, const double* __restrict__ ee,
                                                     const double* __restrict__ HV, const double* __restrict__ tau, int L,
                                                     double* __restrict__ w, double* __restrict__ V, int64_t ldv) {
    extern __shared__ __attribute__((aligned(16))) double sm_te[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double* sd = sm_te;                 // d
    double* se = sd + L;                // e (sub-diagonal), e[L - 1] = 0
    double* s2 = se + L;                // e^2
    double* qp = s2 + L + (size_t)wv * 3 * L;   // per wave: q+, q-, z
    double* qm = qp + L;
    double* z = qm + L;
    for (int i = tid; i < L; i += 64 * WPB) { const double ev = ee[i]; sd[i] = dd[i]; se[i] = ev; s2[i] = ev * ev; }
    __syncthreads();
    const int j = blockIdx.x * WPB + wv;                         // descending index
    if (j >= L) return;
    // Gershgorin interval and the scale of T
    double glo = 1e300, ghi = -1e300;
    for (int i = lane; i < L; i += 64) {
        const double r = (i > 0 ? fabs(se[i - 1]) : 0.0) + (i + 1 < L ? fabs(se[i]) : 0.0);
        glo = fmin(glo, sd[i] - r); ghi = fmax(ghi, sd[i] + r);
    }
    for (int off = 32; off > 0; off >>= 1) { glo = fmin(glo, __shfl_xor(glo, off, 64)); ghi = fmax(ghi, __shfl_xor(ghi, off, 64)); }
    const double tnorm = fmax(fabs(glo), fabs(ghi));
    const double tiny = fmax(tnorm, 1e-300) * 1e-30;            // stands for an exact zero pivot in the recurrences
    const int kth = L - 1 - j;                                    // 0-based ascending index of the wanted eigenvalue
    auto sturm = [&](double x) {                                  // number of eigenvalues of T below x
        double q = sd[0] - x;
        if (fabs(q) < tiny) q = -tiny;
        int cnt = q < 0.0 ? 1 : 0;
        for (int i = 1; i < L; ++i) {
            q = sd[i] - x - s2[i - 1] / q;
            if (fabs(q) < tiny) q = -tiny;
            cnt += q < 0.0 ? 1 : 0;
        }
        return cnt;
    };
    double lo = glo - 1e-12 * tnorm - tiny, hi = ghi + 1e-12 * tnorm + tiny;
    if (!(tnorm < 1e300)) { lo = 0; hi = 0; }                     // non-finite input: leave a NaN-free nonsense, the flag catches it
    for (int pass = 0; pass < 11; ++pass) {                       // 65-way split per pass
        const double h = (hi - lo) * (1.0 / 65.0);
        const double x = lo + h * (lane + 1);
        const int c = sturm(x);
        const unsigned long long mask = __ballot(c > kth);        // lanes whose point has more than kth eigenvalues below it
        if (mask) {
            const int first = __ffsll((long long)mask) - 1;
            const double nhi = lo + h * (first + 1), nlo = lo + h * first;
            hi = nhi; lo = nlo;
        } else {
            lo = lo + h * 64;
        }
    }
    const double lam = 0.5 * (lo + hi);
    if (lane == 0) w[j] = lam;
    // eigenvector of T: twisted factorisation at the index of smallest |gamma| (two independent recurrences: one lane each)
    if (lane == 0) {
        double q = sd[0] - lam;
        if (fabs(q) < tiny) q = tiny;
        qp[0] = q;
        for (int i = 1; i < L; ++i) { q = sd[i] - lam - s2[i - 1] / q; if (fabs(q) < tiny) q = tiny; qp[i] = q; }
    } else if (lane == 1) {
        double q = sd[L - 1] - lam;
        if (fabs(q) < tiny) q = tiny;
        qm[L - 1] = q;
        for (int i = L - 2; i >= 0; --i) { q = sd[i] - lam - s2[i] / q; if (fabs(q) < tiny) q = tiny; qm[i] = q; }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    double gbest = 1e300;
    int rbest = 0;
    for (int i = lane; i < L; i += 64) {
        const double g = fabs(qp[i] + qm[i] - (sd[i] - lam));
        if (g < gbest) { gbest = g; rbest = i; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double og = __shfl_xor(gbest, off, 64);
        const int orr = __shfl_xor(rbest, off, 64);
        if (og < gbest || (og == gbest && orr < rbest)) { gbest = og; rbest = orr; }
    }
    if (lane == 0) {
        z[rbest] = 1.0;
        double zi = 1.0;
        for (int i = rbest - 1; i >= 0; --i) { zi = -se[i] * zi / qp[i]; z[i] = zi; }
    } else if (lane == 1) {
        double zi = 1.0;
        for (int i = rbest + 1; i < L; ++i) { zi = -se[i - 1] * zi / qm[i]; z[i] = zi; }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // normalise (scaled against overflow), then v = H_0 ... H_{L-3} z: reflector k acts on entries k + 1 ..
    double zmax = 0;
    for (int i = lane; i < L; i += 64) zmax = fmax(zmax, fabs(z[i]));
    for (int off = 32; off > 0; off >>= 1) zmax = fmax(zmax, __shfl_xor(zmax, off, 64));
    const double zs = zmax > 0.0 && zmax < 1e300 ? 1.0 / zmax : 1.0;
    double nrm = 0;
    for (int i = lane; i < L; i += 64) { const double v = z[i] * zs; z[i] = v; nrm += v * v; }
    for (int off = 32; off > 0; off >>= 1) nrm += __shfl_xor(nrm, off, 64);
    const double rn = nrm > 0.0 ? 1.0 / sqrt(nrm) : 0.0;
    for (int i = lane; i < L; i += 64) z[i] *= rn;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int k = L - 3; k >= 0; --k) {
        const double tk = tau[k];
        if (tk == 0.0) continue;
        const double* hv = HV + (size_t)k * L;
        double dot = 0;
        for (int i = k + 1 + lane; i < L; i += 64) dot += hv[i] * z[i];
        for (int off = 32; off > 0; off >>= 1) dot += __shfl_xor(dot, off, 64);
        const double f = tk * dot;
        for (int i = k + 1 + lane; i < L; i += 64) z[i] -= f * hv[i];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    for (int i = lane; i < L; i += 64) V[(int64_t)i * ldv + j] = z[i];
}
// verdict of the two-stage route, read by the Jacobi kernels launched behind it: flag = 1 (run Jacobi) when some eigenvalue
// is not finite or two neighbours are closer than 1e-10 of the largest magnitude (their vectors need not be orthogonal)
__global__ __launch_bounds__(1024) void k_trieig_verdict(const double* __restrict__ w, const double* __restrict__ ee, int L, double gap_tol,
                                                         const double* __restrict__ A, int64_t lda, int* __restrict__ flag, int ncheck) {
    __shared__ int bad;
    __shared__ double red[3][16];
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    const double scale = fmax(fabs(w[0]), fabs(w[L - 1]));
    for (int j = threadIdx.x; j < L; j += blockDim.x) {
        const double a = w[j];
        bool b = !(fabs(a) < 1e300);
        if (j + 1 < L) b = b || (j < ncheck && !(a - w[j + 1] > gap_tol * scale)) || !(fabs(ee[j]) > 1e-14 * scale);   // (or the matrix decouples)
        if (b) bad = 1;
    }
    // two invariants of the similarity transform, checked against the INPUT matrix (k_tridiag works on a copy): the trace and
    // the squared Frobenius norm.  A defect anywhere in the reduction or the eigenvalue search shows up here instead of in
    // the caller's results (orders above the workgroup size once went through a truncated Householder step unnoticed).
    double tr = 0, fr = 0, sw = 0, sw2 = 0;
    for (int64_t e = threadIdx.x; e < (int64_t)L * L; e += blockDim.x) {
        const int64_t r = e / L, c = e - r * L;
        const double v = A[r * lda + c];
        fr += v * v;
        if (r == c) tr += v;
    }
    for (int j = threadIdx.x; j < L; j += blockDim.x) { const double a = w[j]; sw += a; sw2 += a * a; }
    double d0 = tr - sw, d1 = fr - sw2, d2 = fr;
    for (int off = 32; off > 0; off >>= 1) { d0 += __shfl_down(d0, off, 64); d1 += __shfl_down(d1, off, 64); d2 += __shfl_down(d2, off, 64); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = d0; red[1][threadIdx.x >> 6] = d1; red[2][threadIdx.x >> 6] = d2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t0 = 0, t1 = 0, t2 = 0;
        for (int x = 0; x < (int)(blockDim.x >> 6); ++x) { t0 += red[0][x]; t1 += red[1][x]; t2 += red[2][x]; }
        const double fn = sqrt(fmax(t2, 0.0));
        const bool off_inv = !(fabs(t0) <= 1e-9 * fmax(fn, 1e-300) * sqrt((double)L)) || !(fabs(t1) <= 1e-9 * fmax(t2, 1e-300));
        *flag = (bad || off_inv || !(scale > 0.0)) ? 1 : 0;
    }
}

// ---- register-resident variants for L <= 141 (the l = k + 10 of the randomized fits, the nc x nc problems of FastICA) ----
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
// sum over the 64 lanes, the same bits in every lane: four DPP butterfly steps inside each row of 16 lanes, then the four
// row sums through v_readlane
__device__ __forceinline__ double wave_sum_f64(double v) {
    v += dpp_f64<0xB1>(v);    // quad_perm [1,0,3,2]
    v += dpp_f64<0x4E>(v);    // quad_perm [2,3,0,1]
    v += dpp_f64<0x141>(v);   // row_half_mirror
    v += dpp_f64<0x140>(v);   // row_mirror
    return (readlane_d(v, 0) + readlane_d(v, 16)) + (readlane_d(v, 32) + readlane_d(v, 48));
}
__device__ __forceinline__ double rcp_nr(double x) {     // 1 / x to fp64 rounding error: v_rcp_f64 and two Newton steps
    double r = __builtin_amdgcn_rcp(x);
    r = fma(fma(-x, r, 1.0), r, r);
    r = fma(fma(-x, r, 1.0), r, r);
    return r;
}
__device__ __forceinline__ double rsqrt_nr(double x) {   // 1 / sqrt(x) for normal x > 0
    double r = __builtin_amdgcn_rsq(x);
    r = r * fma(-0.5 * x * r, r, 1.5);
    r = r * fma(-0.5 * x * r, r, 1.5);
    return r;
}
__device__ __forceinline__ void wave_sum2_f64(double& a, double& b) {  // two sums at once: the two chains interleave
    a += dpp_f64<0xB1>(a);  b += dpp_f64<0xB1>(b);
    a += dpp_f64<0x4E>(a);  b += dpp_f64<0x4E>(b);
    a += dpp_f64<0x141>(a); b += dpp_f64<0x141>(b);
    a += dpp_f64<0x140>(a); b += dpp_f64<0x140>(b);
    const double a0 = readlane_d(a, 0) + readlane_d(a, 16), b0 = readlane_d(b, 0) + readlane_d(b, 16);
    const double a1 = readlane_d(a, 32) + readlane_d(a, 48), b1 = readlane_d(b, 32) + readlane_d(b, 48);
    a = a0 + a1;
    b = b0 + b1;
}
__device__ __forceinline__ double oct_sum_f64(double v) {  // sum over each group of 8 consecutive lanes
    v += dpp_f64<0xB1>(v);
    v += dpp_f64<0x4E>(v);
    v += dpp_f64<0x141>(v);
    return v;
}

// Householder tridiagonalisation with two barriers per step and no global-memory traffic inside the loop.  The kernel is
// bound by instruction issue and by fp64 latency on ONE compute unit, so it runs one wave per SIMD and keeps the per-wave
// instruction count down.  Thread (g, sub) = (tid / 8, tid % 8): the eight lanes of a group share a row, lane sub owns the
// columns j = sub (mod 8) of the trailing block and keeps v_j (and later w_j) of ITS columns in registers, read from row k
// of the symmetric working copy -- every group computes sigma, beta, tau and p^T v redundantly (bit-identically) from
// those, so nothing but p has to cross a barrier before the rank-2 update.  The step is a template on the number T of
// column slots per lane (trailing order m <= 8 T) and the kernel walks down a ladder of T as the block shrinks; the working
// copy carries PAD zero columns on the right, at least the ladder's overshoot 8 T - m, so no column needs a bound check
// (v and w are exactly zero there and the update leaves the zeros alone).  Reflector k is parked in column k of the working
// copy (dead by then), beta and tau in row k; one pass at the end writes d, e, tau and the reflector rows out.
#ifndef PETAL_TRR_THREADS
#define PETAL_TRR_THREADS 512   // two waves per SIMD: 256 and 1024 threads measured 6 % and 12 % slower at L = 74
#endif
constexpr int TRR_THREADS = PETAL_TRR_THREADS;
template <int T>
__device__ __forceinline__ void tri_step(double* __restrict__ W, int ld, int L, int k, double* __restrict__ sv,
                                         double* __restrict__ sp, long long& _t0) {
    constexpr int NG = TRR_THREADS / 8;                          // row groups
    constexpr int RB = (8 * T + NG - 1) / NG;                    // rows per group: the whole trailing block in one unrolled pass
    const int tid = threadIdx.x, g = tid >> 3, sub = tid & 7;
    const int m = L - k - 1;
    double* rowk = W + k * ld + k + 1;                           // x_j = W[k][k + 1 + j] (= W[k + 1 + j][k]); zeros from j = m on
    double xv[T], wj[T];
    double sq0 = 0, sq1 = 0;
    const double alpha = rowk[0];
#pragma unroll
    for (int t = 0; t < T; ++t) {
        xv[t] = rowk[sub + 8 * t];
        if (t == 0) sq0 = sub > 0 ? xv[0] * xv[0] : 0.0;
        else if (t & 1) sq1 = fma(xv[t], xv[t], sq1);
        else sq0 = fma(xv[t], xv[t], sq0);
    }
    const double sigma = oct_sum_f64(sq0 + sq1);
    double beta = alpha, tk = 0.0, scale = 0.0;
    if (sigma > 0.0) {                                            // v_rsq / v_rcp + Newton, the reciprocal seeded from the raw rsq
        const double n2 = fma(alpha, alpha, sigma);
        double rs = __builtin_amdgcn_rsq(n2);
        double rc = __builtin_amdgcn_rcp(fma(n2, rs, fabs(alpha)));   // ~ 1 / (|alpha| + ||x||), refined below
        rs = rs * fma(-0.5 * n2 * rs, rs, 1.5);
        rs = rs * fma(-0.5 * n2 * rs, rs, 1.5);
        const double nrm = n2 * rs;
        beta = -copysign(nrm, alpha);
        const double den = fabs(alpha) + nrm;                     // |alpha - beta|
        rc = fma(fma(-den, rc, 1.0), rc, rc);
        rc = fma(fma(-den, rc, 1.0), rc, rc);
        scale = copysign(rc, alpha);
        tk = den * rs;                                            // (beta - alpha) / beta
    }
#pragma unroll
    for (int t = 0; t < T; ++t) xv[t] *= scale;                   // v_j (exactly 0 from j = m on)
    if (sub == 0) xv[0] = 1.0;
    if (g == 0) {
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int j = sub + 8 * t;
            sv[j] = xv[t];
            if (j < m) W[(k + 1 + j) * ld + k] = xv[t];
        }
    }
    DBG_T(0);
    if (tk != 0.0) {                                              // (uniform: every thread holds the same bits)
        double acc[RB][2];                                        // p = tau A22 v: the rows of a group side by side (ILP)
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int i = g + NG * r;
            const double* row = W + (k + 1 + min(i, m - 1)) * ld + k + 1 + sub;
            acc[r][0] = 0; acc[r][1] = 0;
#pragma unroll
            for (int t = 0; t < T; ++t) acc[r][t & 1] = fma(row[8 * t], xv[t], acc[r][t & 1]);
        }
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int i = g + NG * r;
            const double a = oct_sum_f64(acc[r][0] + acc[r][1]);
            if (sub == 0 && i < 8 * T) sp[i] = i < m ? tk * a : 0.0;  // (p is exactly 0 from i = m on, like v)
        }
    }
    DBG_T(1);
    __syncthreads();                                              // every read of row k is done: it now keeps beta and tau
    DBG_T(2);
    if (tid == 0) { rowk[0] = beta; rowk[1] = tk; }
    if (tk != 0.0) {
        double pv0 = 0, pv1 = 0;
#pragma unroll
        for (int t = 0; t < T; ++t) {
            wj[t] = sp[sub + 8 * t];
            if (t & 1) pv1 = fma(wj[t], xv[t], pv1);
            else pv0 = fma(wj[t], xv[t], pv0);
        }
        const double K = -0.5 * tk * oct_sum_f64(pv0 + pv1);
#pragma unroll
        for (int t = 0; t < T; ++t) wj[t] = fma(K, xv[t], wj[t]);  // w = p + K v
        DBG_T(3);
#pragma unroll
        for (int r = 0; r < RB; ++r) {                            // A22 -= v w^T + w v^T
            const int i = g + NG * r;
            if (i < m) {
                const double vi = sv[i], wi = fma(K, vi, sp[i]);
                double* row = W + (k + 1 + i) * ld + k + 1 + sub;
#pragma unroll
                for (int t = 0; t < T; ++t) row[8 * t] = fma(-vi, wj[t], fma(-wi, xv[t], row[8 * t]));
            }
        }
    }
    DBG_T(4);
    __syncthreads();
    DBG_T(5);
}
// the steps whose trailing order m = L - k - 1 needs T slots (m > 8 (T - STEP)), then down the ladder
template <int T, int STEP>
__device__ __forceinline__ void tri_ladder(double* __restrict__ W, int ld, int L, int& k, double* __restrict__ sv,
                                           double* __restrict__ sp, long long& _t0) {
    for (const int kend = min(L - 2, L - 1 - 8 * (T - STEP)); k < kend; ++k) tri_step<T>(W, ld, L, k, sv, sp, _t0);
    if constexpr (T - STEP > 0) tri_ladder<T - STEP, STEP>(W, ld, L, k, sv, sp, _t0);
}
// row pitch of the working copy: at least L + PAD, and 8 or 24 (mod 32) doubles where the LDS has room -- the four rows that a
// 32-lane half reads (8 lanes each, 8 consecutive doubles) then fall on four different quarters of the bank row (ds_read_b64
// banks: (a / 4) mod 64); an odd pitch, the round-3 choice, leaves two of them overlapping: 85.4 -> 80.5 us at l = 74
__host__ __device__ constexpr int tri_ld(int L, int step) {
    const int lo = L + 8 * step, r = lo % 32;
    const int v = r <= 8 ? lo + (8 - r) : (r <= 24 ? lo + (24 - r) : lo + (40 - r));
    return (size_t)8 * ((size_t)L * v + 288) <= 160 * 1024 ? v : (step == 1 ? L + 8 : (lo | 1));
}
__host__ __device__ constexpr int tri_sp_len(int tmax) { return 8 * tmax; }
template <int TMAX, int STEP>  // L <= 8 TMAX; PAD = 8 STEP zero columns
__global__ __launch_bounds__(TRR_THREADS) void k_tridiag_r(const double* __restrict__ A, int L, int64_t lda, double* __restrict__ dd,
                                                           double* __restrict__ ee, double* __restrict__ HV,
                                                           double* __restrict__ tau, double* __restrict__ gg,
                                                           int* __restrict__ flag, double* __restrict__ V, int64_t ldv, int Lz, int reset_flag) {
    extern __shared__ __attribute__((aligned(16))) double sm_tri[];
    const int tid = threadIdx.x;
    const int ld = tri_ld(L, STEP);
    for (int e = tid; e < Lz * Lz; e += TRR_THREADS) {           // the caller's zero padding of V (rows / columns L .. Lz - 1)
        const int r = e / Lz, c = e - r * Lz;
        if (r >= L || c >= L) V[(int64_t)r * ldv + c] = 0.0;
    }
    double* W = sm_tri;
    double* sv = W + (size_t)L * ld;                              // 8 TMAX entries
    double* sp = sv + 8 * TMAX;                                   // tri_sp_len(TMAX) entries
    for (int e0 = tid; e0 < L * ld; e0 += 8 * TRR_THREADS) {     // (eight loads in flight per thread: a load -> LDS-store loop pays
        double t8[8];                                            //  an L2 round trip per trip, thirteen in a row at L = 74)
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = e0 + u * TRR_THREADS, r = e / ld, c = e - r * ld;
            t8[u] = (e < L * ld && c < L) ? A[(int64_t)r * lda + c] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int e = e0 + u * TRR_THREADS; if (e < L * ld) W[e] = t8[u]; }
    }
    if (tid == 0 && reset_flag) *flag = 0;   // (a caller-owned verdict word accumulates: it is not reset here)
    __syncthreads();
    long long _t0 = 0;
#ifdef PETAL_DEBUG_COUNTERS
    _t0 = clock64();
    const long long _w0 = wall_clock64();
#endif
    int k = 0;
    tri_ladder<TMAX, STEP>(W, ld, L, k, sv, sp, _t0);
#ifdef PETAL_DEBUG_COUNTERS
    if (tid == 0) g_cyc[25] += wall_clock64() - _w0;
#endif
    for (int e = tid; e < (L - 2) * L; e += TRR_THREADS) {       // reflector k: row k of HV, entries k + 1 .. L - 1
        const int kk = e / L, c = e - kk * L;
        HV[e] = c > kk ? W[c * ld + kk] : 0.0;
    }
    for (int kk = tid; kk < L; kk += TRR_THREADS) {
        dd[kk] = W[kk * ld + kk];
        ee[kk] = kk + 2 < L ? W[kk * ld + kk + 1] : (kk + 2 == L ? W[(L - 1) * ld + L - 2] : 0.0);
        tau[kk] = kk + 2 < L ? W[kk * ld + kk + 2] : 0.0;
    }
    // gg[k] = v_k . v_{k-1} (lets the back-transformation apply two reflectors per reduction round), eight lanes per k
    for (int kk = tid >> 3; kk < L; kk += TRR_THREADS / 8) {
        double acc = 0;
        if (kk >= 1 && kk + 2 < L)
            for (int c = kk + 1 + (tid & 7); c < L; c += 8) acc += W[c * ld + kk] * W[c * ld + kk - 1];
        acc = oct_sum_f64(acc);
        if ((tid & 7) == 0) gg[kk] = acc;
    }
}

// ---- the same reduction on 16-byte LDS accesses (round 4).  With two waves per SIMD the LDS hands out 8-byte reads at a fraction
// of its rate (MI355X_MICROARCH.md, LDS: ds_read_b64 needs ~4 waves per SIMD, ds_read_b128 one), and a step of k_tridiag_r is paced
// by the number of LDS instructions between its two barriers (measured with the look-ahead experiment, EXPERIMENTS.md round 4).
// Here lane `sub` owns the ABSOLUTE column pairs {2 sub, 2 sub + 1} (mod 16): its slots mean the same columns in every step and
// start on 16-byte boundaries, so every row access is one ds_read_b128 / ds_write_b128 per 16 columns -- half the LDS
// instructions of the 8-byte form.  Columns that have left the trailing block keep v = w = 0: the update writes their old
// values back unchanged, so nothing needs a guard; reflector k is parked in ROW k (dead once the step has read it), contiguous,
// with beta in the slot of its unit entry and tau in the dead column k below it.
template <int TM, int T>
__device__ __forceinline__ void triw_step(double* __restrict__ W, int ld, int L, int off, int k, double* __restrict__ sv,
                                          double* __restrict__ sp) {
    constexpr int NG = TRR_THREADS / 8;
    constexpr int RB = (16 * T + NG - 1) / NG;
    constexpr int A0 = TM - T;
    const int tid = threadIdx.x, g = tid >> 3, sub = tid & 7;
    const int c0 = 2 * sub - off;                                 // column of element 0 of slot a: c0 + 16 a
    // ---- reflector k from row k ----
    const double* rowk = W + k * ld;
    const double alpha = rowk[k + 1];
    f64x2 x[TM];
    double sq0 = 0, sq1 = 0;
#pragma unroll
    for (int a = A0; a < TM; ++a) {
        const int c = c0 + 16 * a;
        x[a] = *reinterpret_cast<const f64x2*>(rowk + c);
        if (a == A0) {                                            // (only the rung's leading slot holds columns that have left the block)
            x[a].x = c > k + 1 ? x[a].x : 0.0;
            x[a].y = c + 1 > k + 1 ? x[a].y : 0.0;
        }
        sq0 = fma(x[a].x, x[a].x, sq0);
        sq1 = fma(x[a].y, x[a].y, sq1);
    }
    const double sigma = oct_sum_f64(sq0 + sq1);
    double beta = alpha, tk = 0.0, scale = 0.0;
    if (sigma > 0.0) {                                            // (uniform: every thread holds the same bits)
        const double n2 = fma(alpha, alpha, sigma);
        double rs = __builtin_amdgcn_rsq(n2);
        double rc = __builtin_amdgcn_rcp(fma(n2, rs, fabs(alpha)));
        rs = rs * fma(-0.5 * n2 * rs, rs, 1.5);
        rs = rs * fma(-0.5 * n2 * rs, rs, 1.5);
        const double nrm = n2 * rs;
        beta = -copysign(nrm, alpha);
        const double den = fabs(alpha) + nrm;
        rc = fma(fma(-den, rc, 1.0), rc, rc);
        rc = fma(fma(-den, rc, 1.0), rc, rc);
        scale = copysign(rc, alpha);
        tk = den * rs;
    }
#pragma unroll
    for (int a = A0; a < TM; ++a) {
        const int c = c0 + 16 * a;
        x[a].x = (a == A0 && c == k + 1) ? 1.0 : x[a].x * scale;
        x[a].y = (a == A0 && c + 1 == k + 1) ? 1.0 : x[a].y * scale;
    }
    if (g == 0) {
#pragma unroll
        for (int a = A0; a < TM; ++a) *reinterpret_cast<f64x2*>(sv + 2 * sub + 16 * a) = x[a];
        // tau is parked in the dead column k of the row below -- BEFORE the barrier: the update behind it writes the old values
        // of dead columns back, so it has to find tau there (the product in front of it multiplies it by v = 0 either way)
        if (sub == 0) W[(k + 1) * ld + k] = tk;
    }
    if (tk != 0.0) {                                              // (uniform)
        // ---- p = tau A22 v ----
        double acc[RB][2];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int i = k + 1 + g + NG * r;
            const double* row = W + min(i, L - 1) * ld + c0;
            acc[r][0] = 0; acc[r][1] = 0;
#pragma unroll
            for (int a = A0; a < TM; ++a) {
                const f64x2 rv = *reinterpret_cast<const f64x2*>(row + 16 * a);
                acc[r][0] = fma(rv.x, x[a].x, acc[r][0]);
                acc[r][1] = fma(rv.y, x[a].y, acc[r][1]);
            }
        }
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int i = k + 1 + g + NG * r;
            const double s = oct_sum_f64(acc[r][0] + acc[r][1]);
            if (sub == 0 && i < L) sp[i + off] = tk * s;
        }
    }
    __syncthreads();
    // reflector k is parked now that every group has read row k (no update touches row k): v, with beta where its unit entry sits
    // (by a group of the second wave: the first has the most rows to update)
    if (g == 8) {
        double* rk = W + k * ld;
#pragma unroll
        for (int a = A0; a < TM; ++a) {
            const int c = c0 + 16 * a;
            if (c + 1 > k) {
                f64x2 pv = x[a];
                if (c == k + 1) pv.x = beta;
                if (c + 1 == k + 1) pv.y = beta;
                if (c == k) pv.x = rk[k];                          // (the diagonal entry stays)
                *reinterpret_cast<f64x2*>(rk + c) = pv;
            }
        }
    }
    if (tk != 0.0) {
        f64x2 w[TM];
        double pv0 = 0, pv1 = 0;
#pragma unroll
        for (int a = A0; a < TM; ++a) {
            const int c = c0 + 16 * a;
            w[a] = *reinterpret_cast<const f64x2*>(sp + 2 * sub + 16 * a);
            if (a == A0) {                                        // (entries of p from rows that have left the block are stale)
                w[a].x = c > k ? w[a].x : 0.0;
                w[a].y = c + 1 > k ? w[a].y : 0.0;
            }
            pv0 = fma(w[a].x, x[a].x, pv0);
            pv1 = fma(w[a].y, x[a].y, pv1);
        }
        const double K = -0.5 * tk * oct_sum_f64(pv0 + pv1);
#pragma unroll
        for (int a = A0; a < TM; ++a) { w[a].x = fma(K, x[a].x, w[a].x); w[a].y = fma(K, x[a].y, w[a].y); }
#pragma unroll
        for (int r = 0; r < RB; ++r) {                            // A22 -= v w^T + w v^T
            const int i = k + 1 + g + NG * r;
            if (i < L) {
                const double vi = sv[i + off], wi = fma(K, vi, sp[i + off]);
                double* row = W + i * ld + c0;
#pragma unroll
                for (int a = A0; a < TM; ++a) {
                    f64x2 rv = *reinterpret_cast<const f64x2*>(row + 16 * a);
                    rv.x = fma(-vi, w[a].x, fma(-wi, x[a].x, rv.x));
                    rv.y = fma(-vi, w[a].y, fma(-wi, x[a].y, rv.y));
                    *reinterpret_cast<f64x2*>(row + 16 * a) = rv;
                }
            }
        }
    }
    __syncthreads();
}
template <int TM, int T>
__device__ __forceinline__ void triw_ladder(double* __restrict__ W, int ld, int L, int S2, int off, int& k, double* __restrict__ sv,
                                            double* __restrict__ sp) {
    if (S2 >= T) {                                                // (a rung with more slots than the matrix has is skipped)
        const int kend = T > 1 ? min(L - 2, 16 * (S2 - T + 1) - 1) : L - 2;
        for (; k < kend; ++k) triw_step<TM, T>(W, ld, L, off, k, sv, sp);
    }
    if constexpr (T > 1) triw_ladder<TM, T - 1>(W, ld, L, S2, off, k, sv, sp);
}
// row pitch: every 16-column slot addressable; 16 (mod 32) doubles where the LDS has room -- the four 8-double pieces of a
// ds_read_b128 lane group (two rows x two half slots) then fall on four different quarters of the bank row
__host__ __device__ inline int triw_ld(int L, int tm) {
    const int s16 = 16 * ((L + 15) / 16);
    const int want = (s16 % 32 == 16) ? s16 : s16 + 16;
    return sizeof(double) * ((size_t)L * want + 32 * tm) <= 160 * 1024 ? want : s16;
}
template <int TM>  // L <= 16 TM
__global__ __launch_bounds__(TRR_THREADS) void k_tridiag_w(const double* __restrict__ A, int L, int64_t lda, double* __restrict__ dd,
                                                           double* __restrict__ ee, double* __restrict__ HV,
                                                           double* __restrict__ tau, double* __restrict__ gg,
                                                           int* __restrict__ flag, double* __restrict__ V, int64_t ldv, int Lz, int reset_flag) {
    extern __shared__ __attribute__((aligned(16))) double sm_tri[];
    const int tid = threadIdx.x;
    const int S2 = (L + 15) >> 4, off = 16 * (TM - S2);
    const int ld = triw_ld(L, TM);
    for (int e = tid; e < Lz * Lz; e += TRR_THREADS) {           // the caller's zero padding of V (rows / columns L .. Lz - 1)
        const int r = e / Lz, c = e - r * Lz;
        if (r >= L || c >= L) V[(int64_t)r * ldv + c] = 0.0;
    }
    double* W = sm_tri;
    double* sv = W + (size_t)L * ld;                              // 16 TM entries, indexed by column + off
    double* sp = sv + 16 * TM;                                    // 16 TM entries
    for (int e0 = tid; e0 < L * ld; e0 += 8 * TRR_THREADS) {
        double t8[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int e = e0 + u * TRR_THREADS, r = e / ld, c = e - r * ld;
            t8[u] = (e < L * ld && c < L) ? A[(int64_t)r * lda + c] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int e = e0 + u * TRR_THREADS; if (e < L * ld) W[e] = t8[u]; }
    }
    for (int e = tid; e < 32 * TM; e += TRR_THREADS) sv[e] = 0.0;
    if (tid == 0 && reset_flag) *flag = 0;   // (a caller-owned verdict word accumulates: it is not reset here)
    __syncthreads();
    int k = 0;
    triw_ladder<TM, TM>(W, ld, L, S2, off, k, sv, sp);
    for (int e = tid; e < (L - 2) * L; e += TRR_THREADS) {       // reflector k: row k of HV, entries k + 1 .. L - 1
        const int kk = e / L, c = e - kk * L;
        HV[e] = c > kk + 1 ? W[kk * ld + c] : (c == kk + 1 ? 1.0 : 0.0);
    }
    for (int kk = tid; kk < L; kk += TRR_THREADS) {
        dd[kk] = W[kk * ld + kk];
        ee[kk] = kk + 2 < L ? W[kk * ld + kk + 1] : (kk + 2 == L ? W[(L - 1) * ld + L - 2] : 0.0);
        tau[kk] = kk + 2 < L ? W[(kk + 1) * ld + kk] : 0.0;
    }
    // gg[k] = v_k . v_{k-1} (lets the back-transformation apply two reflectors per reduction round), eight lanes per k: v_k is row k
    // from column k + 2 on and 1 at column k + 1
    for (int kk = tid >> 3; kk < L; kk += TRR_THREADS / 8) {
        double acc = 0;
        if (kk >= 1 && kk + 2 < L)
            for (int c = kk + 1 + (tid & 7); c < L; c += 8) acc += (c == kk + 1 ? 1.0 : W[kk * ld + c]) * W[(kk - 1) * ld + c];
        acc = oct_sum_f64(acc);
        if ((tid & 7) == 0) gg[kk] = acc;
    }
}

// one wave per eigenpair.  The Sturm count runs on the three-term recurrence of the leading minors, renormalised by their
// exponent every step (v_frexp_mant / v_ldexp: no division on the chain); d and e^2 are fetched eight at a time so the LDS
// latency is paid once per eight steps.  The twisted factorisation keeps both recurrences in one instruction stream
// (lanes 0 and 1) and stores the multipliers, so the two sweeps of z are products only; z then lives in registers and the
// reflector rows come from an LDS stage filled while the eigenvalue search runs.  An eigenvalue with a neighbour inside
// gap_tol ||T|| (its vector is then only eps / gap_tol accurate) or a non-finite result raises *flag for the Jacobi solver
// launched behind this kernel.
template <int WPB, int QMAX>  // L <= 64 QMAX
__global__ __launch_bounds__(64 * WPB) void k_trieig_r(const double* __restrict__ dd, const double* __restrict__ ee,
                                                       const double* __restrict__ HV, const double* __restrict__ tau,
                                                       const double* __restrict__ gg, int L, double gap_tol, int hv_rows,
                                                       double* __restrict__ w, double* __restrict__ V, int64_t ldv,
                                                       int* __restrict__ flag, int ncheck) {
    extern __shared__ __attribute__((aligned(16))) double sm_te[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#ifdef PETAL_DEBUG_COUNTERS
    long long _t0 = clock64();
    const long long _w0 = wall_clock64();
#define DBG_E(i) do { if (threadIdx.x == 0 && blockIdx.x == 0) { long long _t = clock64(); g_cyc[i] += _t - _t0; _t0 = _t; } } while (0)
#else
#define DBG_E(i) do {} while (0)
#endif
    const int LP = ((L + 7) & ~7) + 8;          // d, e, e^2 padded: whole batches of eight may run past L without a bound check
    double* sd = sm_te;
    double* se = sd + LP;
    double* s2 = se + LP;
    double* st = s2 + LP;                       // tau
    double* sdr = st + LP;                      // d and e^2 in reversed order (the recurrence from the bottom)
    double* s2r = sdr + LP;
    double* sg = s2r + LP;                      // v_k . v_{k-1}
    double* qp = sg + LP + (size_t)wv * 4 * LP; // per wave: minors from the top / bottom and their predecessors; later l+, u-, z
    double* qm = qp + LP;
    double* lp = qm + LP;
    double* lm = lp + LP;
    double* shv = sg + LP + (size_t)WPB * 4 * LP;   // hv_rows reflector rows, staged for the back-transformation
    // the last hv_rows reflectors (the first ones applied) start their way into LDS now
    int kbase = max(L - 2 - hv_rows, 0);
    auto stage = [&](int k0, int nrows) {                          // eight loads per thread in flight: the rows come from HBM / MALL
        const int ne = nrows * L;
        const double* src = HV + (size_t)k0 * L;
        for (int e0 = tid; e0 < ne; e0 += 64 * WPB * 8) {
            double t8[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int e = e0 + u * 64 * WPB; t8[u] = e < ne ? src[e] : 0.0; }
#pragma unroll
            for (int u = 0; u < 8; ++u) { const int e = e0 + u * 64 * WPB; if (e < ne) shv[e] = t8[u]; }
        }
    };
    stage(kbase, L - 2 - kbase);
    // Gershgorin interval and the scale of T (every wave, from global memory: L values)
    double glo = 1e300, ghi = -1e300;
    for (int i = lane; i < L; i += 64) {
        const double r = (i > 0 ? fabs(ee[i - 1]) : 0.0) + (i + 1 < L ? fabs(ee[i]) : 0.0);
        glo = fmin(glo, dd[i] - r); ghi = fmax(ghi, dd[i] + r);
    }
    for (int off = 32; off > 0; off >>= 1) { glo = fmin(glo, __shfl_xor(glo, off, 64)); ghi = fmax(ghi, __shfl_xor(ghi, off, 64)); }
    const double tnorm = fmax(fabs(glo), fabs(ghi));
    const bool sane = tnorm > 1e-140 && tnorm < 1e140;
    const double inv = sane ? 1.0 / tnorm : 0.0;
    for (int i = tid; i < LP; i += 64 * WPB) {
        const double ev = i < L ? ee[i] * inv : 0.0;
        sd[i] = i < L ? dd[i] * inv : 4.0;                        // padding: d - x > 0 and e = 0 there, no sign change is added
        se[i] = ev;
        s2[i] = fmax(ev * ev, 1e-280);                            // never an exact split: the minors cannot stick at zero
        // a (numerically) decoupled matrix: the twisted factorisation's choice of r compares pivots that the 1e-30 clamp has
        // flattened (an exactly diagonal A with lambda hit to the last bit picked a neighbour's unit vector) -- Jacobi's case
        if (i + 1 < L && !(fabs(ev) > 1e-14)) atomicOr(flag, 1);
        st[i] = i < L ? tau[i] : 0.0;
        sg[i] = i < L ? gg[i] : 0.0;
        const int ir = L - 1 - i;                                 // reversed: sdr[t] = d_{L-1-t}, s2r[u] = e^2_{L-2-u}
        sdr[i] = ir >= 0 ? dd[ir] * inv : 4.0;
        const double evr = ir >= 1 ? ee[ir - 1] * inv : 0.0;
        s2r[i] = fmax(evr * evr, 1e-280);
    }
    __syncthreads();
    DBG_E(16);
    const int j = min(blockIdx.x * WPB + wv, L - 1);             // descending index (a surplus wave repeats the last one)
    const int kth = L - 1 - j;
    // (p0, p1) = two consecutive leading minors of T - x on a common power-of-two scale.  The scale follows the exponent of
    // the OLDER of the two (integer instructions on the exponent field, off the dependent chain), so the chain per step is
    // one fma and one multiply; the magnitudes stay within a few decades of 1 because a step grows a minor at most 3 x.
    auto step_scale = [](double p1) {
        const int ef = max((__double2hiint(p1) >> 20) & 0x7ff, 423);
        return __hiloint2double((2045 - ef) << 20, 0);            // 2^(1022 - ef), at most 2^599 (exact zero, denormals)
    };
    auto sturm = [&](double x) {                                  // number of eigenvalues of T / ||T|| below x
        double p0 = 1.0, p1 = sd[0] - x;
        unsigned sprev = (unsigned)__double2hiint(p1) >> 31, cnt = sprev;
        for (int i0 = 1; i0 < L; i0 += 8) {
            double dv[8], e2v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { dv[u] = sd[i0 + u]; e2v[u] = s2[i0 + u - 1]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) {                         // (runs into the padding: no bound check per step)
                const double raw = fma(dv[u] - x, p1, -e2v[u] * p0);
                const unsigned sg = (unsigned)__double2hiint(raw) >> 31;
                cnt += sg ^ sprev;                                // sign change (a zero minor: either sign)
                sprev = sg;
                if ((u & 3) == 3) {                               // renormalise every FOURTH step (round 6; every second until then): four
                    const double sc = step_scale(p1);             // steps move a minor by at most 1e64 either way from a scale near 1 -- far
                                                                  // inside the range -- and the rescaling was half of the count's dependent chain
                    p0 = p1 * sc;
                    p1 = raw * sc;
                } else {
                    p0 = p1;
                    p1 = raw;
                }
            }
        }
        return (int)cnt;
    };
    double lo = glo * inv - 1e-12, hi = ghi * inv + 1e-12;
    for (int pass = 0; pass < 9; ++pass) {                        // 65-way split per pass: (2 + 2e-12) / 65^9 < 1e-16 of ||T||
        const double h = (hi - lo) * (1.0 / 65.0);
        const int c = sturm(lo + h * (lane + 1));
        const unsigned long long mask = __ballot(c > kth);
        if (mask) {
            const int first = __ffsll((long long)mask) - 1;
            const double nhi = lo + h * (first + 1), nlo = lo + h * first;
            hi = nhi; lo = nlo;
        } else {
            lo = lo + h * 64;
        }
    }
    const double lam = 0.5 * (lo + hi);
    DBG_E(17);
    if (lane == 0) w[j] = lam * tnorm;
    // neighbours inside gap_tol? (counts at lam -+ gap_tol: exactly this one eigenvalue should lie between)
    {
        const int c = sturm((lane & 1) ? lam + gap_tol : lam - gap_tol);
        const int c0 = __builtin_amdgcn_readlane(c, 0), c1 = __builtin_amdgcn_readlane(c, 1);
        // (ncheck: the caller only uses the leading ncheck pairs -- a cluster further down keeps its eps / gap vectors)
        if (lane == 0 && ((c1 - c0 != 1 && j < ncheck) || !sane)) atomicOr(flag, 1);
    }
    DBG_E(18);
    // twisted factorisation.  The pivots are ratios of consecutive minors: q+_i = p_{i+1} / p_i from the top (lane 0), q-_i
    // likewise from the bottom (lane 1), both on the division-free recurrence of the Sturm count in ONE instruction stream:
    // lane 1 walks the REVERSED copies of d and e^2 and leaves its results in reversed order, so both lanes address
    // base + step.  The divisions, gamma and the multipliers are then lane-parallel.
    const bool fw = lane == 0;
    if (lane < 2) {
        const double* bd = fw ? sd : sdr;
        const double* be = fw ? s2 : s2r;
        double* narr = fw ? qp : qm;
        double* darr = fw ? lp : lm;
        double p0 = 1.0, p1 = bd[0] - lam;
        narr[0] = p1;
        darr[0] = 1.0;
        for (int t0 = 1; t0 < L; t0 += 8) {                       // (steps past L - 1 read and write the padding)
            double dv[8], e2v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { dv[u] = bd[t0 + u]; e2v[u] = be[t0 + u - 1]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const double raw = fma(dv[u] - lam, p1, -e2v[u] * p0);
                narr[t0 + u] = raw;
                darr[t0 + u] = p1;
                if (u & 1) {
                    const double sc = step_scale(p1);
                    p0 = p1 * sc;
                    p1 = raw * sc;
                } else {
                    p0 = p1;
                    p1 = raw;
                }
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    DBG_E(19);
    double gbest = 1e300;
    int rbest = 0;
    {
        double qpv[QMAX], qmv[QMAX];
        auto pivot = [](double num, double den) {                 // a vanishing or non-finite pivot is replaced, as dstein does
            double q = num / den;
            if (!(fabs(q) >= 1e-30)) q = 1e-30;
            if (!(fabs(q) <= 1e300)) q = copysign(1e300, num) * (den < 0.0 ? -1.0 : 1.0);
            return q;
        };
#pragma unroll
        for (int q = 0; q < QMAX; ++q) {
            const int i = lane + 64 * q;
            if (i < L) {
                qpv[q] = pivot(qp[i], lp[i]);
                qmv[q] = pivot(qm[L - 1 - i], lm[L - 1 - i]);
                const double gm = fabs(qpv[q] + qmv[q] - (sd[i] - lam));
                if (gm < gbest) { gbest = gm; rbest = i; }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // multipliers, laid out for the two sweeps away from r: lp[L - 2 - i] = l+_i = e_i / q+_i (lane 0 walks i downwards,
        // the array upwards), lm[i] = u-_{i-1} = e_{i-1} / q-_i
#pragma unroll
        for (int q = 0; q < QMAX; ++q) {
            const int i = lane + 64 * q;
            if (i < L) {
                if (i + 1 < L) lp[L - 2 - i] = se[i] * rcp_nr(qpv[q]);
                if (i > 0) lm[i] = se[i - 1] * rcp_nr(qmv[q]);
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double og = __shfl_xor(gbest, off, 64);
        const int orr = __shfl_xor(rbest, off, 64);
        if (og < gbest || (og == gbest && orr < rbest)) { gbest = og; rbest = orr; }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    DBG_E(20);
    // z_r = 1, z_i = -l+_i z_{i+1} below r (lane 0: kept reversed in qm), z_i = -u-_{i-1} z_{i-1} above (lane 1: in qp)
    if (lane < 2) {
        const double* bm = fw ? lp + (L - 2 - rbest) : lm + rbest;   // the multiplier of step t sits at bm[t]
        double* bz = fw ? qm + (L - 1 - rbest) : qp + rbest;         // z of step t goes to bz[t]
        const int tcap = (fw ? rbest : L - 1 - rbest) + 8;           // steps past a lane's own end land in the padding
        const int nmax = max(rbest, L - 1 - rbest);
        double zi = 1.0;
        bz[0] = 1.0;
        for (int t0 = 1; t0 <= nmax; t0 += 8) {
            double mv[8];
            int tt[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { tt[u] = min(t0 + u, tcap); mv[u] = bm[tt[u]]; }
#pragma unroll
            for (int u = 0; u < 8; ++u) { zi = -mv[u] * zi; bz[tt[u]] = zi; }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    DBG_E(21);
    double zq[QMAX];
    double zmax = 0;
#pragma unroll
    for (int q = 0; q < QMAX; ++q) {
        const int i = lane + 64 * q;
        zq[q] = i < L ? (i < rbest ? qm[L - 1 - i] : qp[i]) : 0.0;
        zmax = fmax(zmax, fabs(zq[q]));
    }
    for (int off = 32; off > 0; off >>= 1) zmax = fmax(zmax, __shfl_xor(zmax, off, 64));
    const double zs = zmax > 0.0 && zmax < 1e300 ? 1.0 / zmax : 1.0;
    double nrm = 0;
#pragma unroll
    for (int q = 0; q < QMAX; ++q) { zq[q] *= zs; nrm += zq[q] * zq[q]; }
    nrm = wave_sum_f64(nrm);
    const double rn = nrm > 0.0 ? 1.0 / sqrt(nrm) : 0.0;
    if (lane == 0 && !(nrm > 0.0 && nrm < 1e300)) atomicOr(flag, 1);
#pragma unroll
    for (int q = 0; q < QMAX; ++q) zq[q] *= rn;
    DBG_E(22);
    // v = H_0 ... H_{L-3} z from the staged rows, hv_rows at a time (one stage when they all fit)
    for (int ktop = L - 3; ktop >= 0;) {
        for (int k = ktop; k >= kbase; k -= 4) {
            double hv[4][QMAX], tk[4];
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                const int kk = max(k - b, kbase);
                tk[b] = k - b >= kbase ? st[kk] : 0.0;
#pragma unroll
                for (int q = 0; q < QMAX; ++q) {
                    const int i = lane + 64 * q;
                    hv[b][q] = i < L ? shv[(kk - kbase) * L + i] : 0.0;
                }
            }
#pragma unroll
            for (int b = 0; b < 4; b += 2) {                      // reflectors k - b, then k - b - 1: one reduction round for both
                double da = 0, db = 0;
#pragma unroll
                for (int q = 0; q < QMAX; ++q) { da += hv[b][q] * zq[q]; db += hv[b + 1][q] * zq[q]; }
                wave_sum2_f64(da, db);
                const double fa = tk[b] * da;
                const double fb = tk[b + 1] * (db - fa * sg[max(k - b, 0)]);   // v_b . (z - fa v_a) = db - fa (v_a . v_b)
#pragma unroll
                for (int q = 0; q < QMAX; ++q) zq[q] -= fa * hv[b][q] + fb * hv[b + 1][q];
            }
        }
        ktop = kbase - 1;
        if (ktop < 0) break;
        __syncthreads();                                          // (uniform: every wave of the block walks the same stages)
        kbase = max(ktop + 1 - hv_rows, 0);
        stage(kbase, ktop + 1 - kbase);
        __syncthreads();
    }
    DBG_E(23);
#ifdef PETAL_DEBUG_COUNTERS
    if (threadIdx.x == 0 && blockIdx.x == 0) g_cyc[24] += wall_clock64() - _w0;
#endif
#pragma unroll
    for (int q = 0; q < QMAX; ++q) {
        const int i = lane + 64 * q;
        if (i < L) V[(int64_t)i * ldv + j] = zq[q];
    }
}

// replay of the rotation log on V = I: wave <-> row r of V (kept in LDS), lanes <-> the disjoint pairs of a round.
// The angles of JR_BATCH rounds are fetched ahead (independent loads) so the global-memory latency is paid once per batch.
constexpr int JR_WAVES = 4, JR_BATCH = 8;
template <int HP>  // pairs per lane: half <= 64 HP
__global__ __launch_bounds__(64 * JR_WAVES) void k_apply_rot(const jf64x2* __restrict__ log_cs, const int* __restrict__ nrounds,
                                                             const int* __restrict__ rank, int L, double* __restrict__ V, int64_t ldv,
                                                             const int* __restrict__ flag) {
    if (flag && *flag == 0) return;
    extern __shared__ __attribute__((aligned(16))) double sm_jr[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int Le = (L + 1) & ~1, half = Le / 2, rounds = Le - 1;
    const int r = blockIdx.x * JR_WAVES + wv;
    double* row = sm_jr + (size_t)wv * Le;
    for (int j = lane; j < Le; j += 64) row[j] = (j == r) ? 1.0 : 0.0;
    const int nR = *nrounds;
    PairIt it[HP];
#pragma unroll
    for (int h = 0; h < HP; ++h) it[h].init(min(lane + 64 * h, half - 1), 0, Le);
    for (int R0 = 0; R0 < nR; R0 += JR_BATCH) {
        jf64x2 cs[JR_BATCH][HP];
#pragma unroll
        for (int u = 0; u < JR_BATCH; ++u) {
            const int Ru = min(R0 + u, nR - 1);
#pragma unroll
            for (int h = 0; h < HP; ++h) cs[u][h] = log_cs[(size_t)Ru * half + min(lane + 64 * h, half - 1)];
        }
#pragma unroll
        for (int u = 0; u < JR_BATCH; ++u) {
            if (R0 + u < nR) {
                double vp[HP], vq[HP];
                int p[HP], q[HP];
#pragma unroll
                for (int h = 0; h < HP; ++h) {
                    it[h].get(min(lane + 64 * h, half - 1), Le, L, p[h], q[h]);
                    it[h].next(Le);  // the sweeps restart at round 0 after Le - 1 rounds: the raw players wrap with them
                    vp[h] = row[p[h]]; vq[h] = row[q[h]];
                }
#pragma unroll
                for (int h = 0; h < HP; ++h) {
                    if (lane + 64 * h < half && p[h] != q[h]) {
                        row[p[h]] = cs[u][h][0] * vp[h] - cs[u][h][1] * vq[h];
                        row[q[h]] = cs[u][h][1] * vp[h] + cs[u][h][0] * vq[h];
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        }
    }
    if (r < L)
        for (int j = lane; j < L; j += 64) V[(int64_t)r * ldv + rank[j]] = row[j];
}

#ifndef PETAL_NS_CAP
#define PETAL_NS_CAP 1.25
#endif
template <int CTRL>
__device__ __forceinline__ float dpp_f32(float v) {  // v as seen through the DPP lane pattern CTRL (VALU speed, no LDS)
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}
// Wout = symmetric_decorrelation(Win) (ica.rs:363-381).  S (= W W^T, then destroyed) and the eigenvector accumulator
// Zt are the Jacobi-hot matrices (LDS when nc <= 64); Z, Mm, w are scratch in global memory.
template <int MB>
__device__ void wg_symdecorr(const double* Win, double* Wout, int nc, int mode, double* S, double* Zt, double* Z, double* Mm,
                             double* w, JacWs& ws) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int ls = MB > 0 ? (nc | 1) : nc;  // the LDS-resident matrices use an odd leading dimension
    for (int e = tid; e < nc * nc; e += nt) {  // S = W W^T (ica.rs:369)
        const int i = e / nc, j = e % nc;
        double acc = 0;
        for (int k = 0; k < nc; ++k) acc += Win[i * nc + k] * Win[j * nc + k];
        S[i * ls + j] = acc;
    }
    __syncthreads();
    wg_jacobi_any<MB>(S, ls, Zt, ls, nc, ws.c, ws.s, ws.p, ws.q, ws.red);
    wg_sort_eig(S, ls, Zt, ls, nc, Z, nc, w, ws.rank);
    // textbook (W W^T)^(-1/2) = Z D Z^T.  literal crate arithmetic (SURVEY.md Q3): Z_asc^T D Z_asc with LAPACK's
    // ascending order; for nc == 2 LAPACK's dlaev2 path returns a symmetric Z for PSD input, where both agree.
    // The literal form is not invariant under eigenvector sign flips, and LAPACK's raw signs are an artefact of the
    // backend (MKL in the crate's CI, OpenBLAS elsewhere): eigenvectors are therefore sign-NORMALISED -- the first
    // component of largest magnitude made positive -- which the oracle's literal mode can be asked to do as well.
    const bool literal = mode == 1 && nc > 2;
    if (literal) {
        for (int c = tid; c < nc; c += nt) {
            double best = -1.0, sg = 1.0;
            for (int k = 0; k < nc; ++k) {
                const double v = Z[k * nc + c];
                if (fabs(v) > best) { best = fabs(v); sg = v < 0.0 ? -1.0 : 1.0; }
            }
            ws.red[c] = sg;
        }
        __syncthreads();
    }
    for (int e = tid; e < nc * nc; e += nt) {
        const int i = e / nc, j = e % nc;
        double acc = 0;
        for (int k = 0; k < nc; ++k) {
            if (literal) acc += Z[k * nc + (nc - 1 - i)] * (1.0 / sqrt(w[nc - 1 - k])) * Z[k * nc + (nc - 1 - j)];
            else acc += Z[i * nc + k] * (1.0 / sqrt(w[k])) * Z[j * nc + k];
        }
        if (literal) acc *= ws.red[nc - 1 - i] * ws.red[nc - 1 - j];
        Mm[e] = acc;
    }
    __syncthreads();
    for (int e = tid; e < nc * nc; e += nt) {
        const int i = e / nc, j = e % nc;
        double acc = 0;
        for (int k = 0; k < nc; ++k) acc += Mm[i * nc + k] * Win[k * nc + j];
        Wout[e] = acc;
    }
    __syncthreads();
}
// Orthogonal polar factor of D (= (D D^T)^(-1/2) D, the symmetric decorrelation of ica.rs:363-381) by the
// Newton-Schulz iteration X <- 1.5 X - 0.5 (X X^T) X from X0 = D / ||D||_F, entirely in LDS: two nc^3 products and
// three barriers per step instead of a full Jacobi eigen-solve (305 us -> tens of us at nc = 32).  Converges
// quadratically once the singular values are O(1); returns false (caller falls back to the eigen-solver) if D is
// singular / non-finite or 60 steps do not reach ||X X^T - I||_F <= 1e-13.
// On entry X (LDS, leading dimension nc | 1) holds D; returns the LDS buffer holding the polar factor, or nullptr.
// Leading dimension of the three LDS matrices of the iteration.  The fp64 MFMA operands are read as 16 rows x 4 consecutive doubles per
// instruction (lane (i, k): row i, column k0 + k): with the odd pitch of the Jacobi solvers (nc | 1: 130 dwords = 2 mod 64 banks) the
// lanes (i, k) and (i + 1, k - 1) share a bank pair -- every operand read of X X^T a 2- to 4-way conflict, and the products are LDS time,
// not matrix time (7400 clock ticks for 32 MFMAs per wave at nc = 64).  nc + 2 puts a row 4 (mod 8) dwords on: conflict-free for
// the row-wise operands (both of X X^T, T of T X).
__host__ __device__ constexpr int polar_ld(int nc) { return (nc & 15) ? (nc | 1) : nc + 2; }
// NTC: the number of 16-wide tiles per side when it is known at compile time (nc = 16 NTC: the products' k loops unroll completely and
// a tile's operand reads are all in flight before its first MFMA -- a 4-deep unroll exposed the LDS latency four times per tile), 0 otherwise.
template <int NTC>
__device__ double* wg_polar_ns(int nc_rt, double* X_, double* T_, double* Y_, double* s_red_, double tol2 = 1e-26) {
    // The four buffers are LDS.  Through generic pointers -- this function is not inlined into its callers -- every access was a FLAT
    // instruction (165 of them at nc = 64, each waiting on vmcnt AND lgkmcnt; the products looked like LDS-latency chains whatever was
    // done to them): the address space is stated here.  64 components: 48.8 -> 32.7 us per FastICA iteration's tail.
    typedef __attribute__((address_space(3))) double lds_f64;
    typedef __attribute__((address_space(3))) float lds_f32;
    lds_f64* X = (lds_f64*)X_;
    lds_f64* T = (lds_f64*)T_;
    lds_f64* Y = (lds_f64*)Y_;
    lds_f64* const s_red = (lds_f64*)s_red_;
    const int nc = NTC ? 16 * NTC : nc_rt;
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wv = tid >> 6, nw = nt >> 6;
    const int ld = polar_ld(nc);
    // nc a multiple of 16: the two nc^3 products of a step run on the fp64 matrix cores (v_mfma_f64_16x16x4_f64, operands
    // straight from LDS); the scalar loops below are LDS-bound -- two reads per FMA -- and cost 20 us per product at nc = 64
    const bool use_mfma = (nc & 15) == 0;
    const int ntile = nc >> 4;
    // ONE barrier per sum: consecutive calls alternate between two slots of s_red, so a call's writes cannot overtake the
    // reads of the call before it (whose slot is rewritten only two calls later, with the call in between's barrier behind them)
    int sum_slot = 0;
    auto block_sum = [&](double v) {
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        lds_f64* slot = s_red + 16 * sum_slot;
        sum_slot ^= 1;
        if (lane == 0) slot[wv] = v;
        __syncthreads();
        // (ONE LDS read per lane and four DPP steps inside each row of 16 lanes -- every row forms the same sum, the same bits in
        // every lane -- instead of nw dependent reads: 8 x ~130 cycles, once per step)
        double t = (lane & 15) < nw ? slot[lane & 15] : 0.0;
        t += dpp_f64<0xB1>(t);
        t += dpp_f64<0x4E>(t);
        t += dpp_f64<0x141>(t);
        t += dpp_f64<0x140>(t);
        return t;
    };
    double ss = 0;
    for (int e = tid; e < nc * nc; e += nt) { const double v = X[(e / nc) * ld + (e % nc)]; ss += v * v; }
    const double fro2 = block_sum(ss);
    if (!(fro2 > 0.0) || !(fro2 < 1e300)) return nullptr;
    const double inv = 1.0 / sqrt(fro2);
    for (int e = tid; e < nc * nc; e += nt) X[(e / nc) * ld + (e % nc)] *= inv;
    __syncthreads();
    bool ok = false;
#ifdef PETAL_DEBUG_COUNTERS
    long long _t0 = clock64();
    if (tid == 0) g_dbg[2] += 1;   // polar factors formed / Newton-Schulz steps taken (dev/tail_phases.py)
#endif
    for (int it = 0; it < 60; ++it) {
        double err = 0;
#ifdef PETAL_DEBUG_COUNTERS
        DBG_T(16);
        if (tid == 0) g_dbg[1] += 1;
#endif
        if (use_mfma) {
            // T = X X^T: tile (ti, tj) per wave pass; A[i][k] = X[16 ti + i][k], B[k][j] = X[16 tj + j][k];
            // C/D: reg r of lane l is row (l >> 4) + 4 r, column l & 15
            for (int tile = wv; tile < ntile * ntile; tile += nw) {
                const int ti = tile / ntile, tj = tile - ti * ntile;
                const lds_f64* pa = X + (16 * ti + (lane & 15)) * ld + (lane >> 4);
                const lds_f64* pb = X + (16 * tj + (lane & 15)) * ld + (lane >> 4);
                f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
                if constexpr (NTC > 0) {
#pragma unroll
                    for (int k0 = 0; k0 < 16 * NTC; k0 += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[k0], pb[k0], acc, 0, 0, 0);
                } else {
#pragma unroll 4
                    for (int k0 = 0; k0 < nc; k0 += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[k0], pb[k0], acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * ti + (lane >> 4) + 4 * r, j = 16 * tj + (lane & 15);
                    T[i * ld + j] = acc[r];
                    const double dlt = acc[r] - (i == j ? 1.0 : 0.0);
                    err += dlt * dlt;
                }
            }
        } else {
            for (int e = tid; e < nc * nc; e += nt) {
                const int i = e / nc, j = e - i * nc;
                double acc = 0;
                for (int k = 0; k < nc; ++k) acc += X[i * ld + k] * X[j * ld + k];
                T[i * ld + j] = acc;
                const double dlt = acc - (i == j ? 1.0 : 0.0);
                err += dlt * dlt;
            }
        }
#ifdef PETAL_DEBUG_COUNTERS
        DBG_T(17);
#endif
        const double terr = block_sum(err);  // (its barriers also publish T)
#ifdef PETAL_DEBUG_COUNTERS
        DBG_T(18);
#endif
        if (!(terr == terr)) return nullptr;
        if (terr <= tol2) { ok = true; break; }  // tol2 = the square of the accepted ||X X^T - I||_F
        // Scaled step: g = max_i sum_j |T_ij| >= lambda_max(T) = sigma_max(X)^2 (Gershgorin), so X / sqrt(g) still has all
        // singular values <= 1 (the iteration stays monotone) but the largest one is pushed towards 1.  For a nearly
        // orthogonal D -- the FastICA case: D ~ beta W -- T is nearly diagonal, the bound is tight, and the iteration
        // turns quadratic after one step instead of crawling up from sigma = 1 / sqrt(nc) by factors of 1.5.
        // (LDS latency is ~110 cycles: a serial loop over nc entries costs microseconds, so the row sums use eight lanes per
        // row and the maximum is a per-wave DPP reduction; fp32 is plenty for a scaling bound)
        // Once ||T - I||_F <= 0.3 every singular value of X lies in [0.83, 1.15]: the plain step X (3 I - T) / 2 converges
        // quadratically from there (errors 0.3 -> 0.1 -> 0.02 -> 5e-4 -> 4e-7 -> ...) and the bounds below -- one more pass
        // over T and a barrier per step -- would only reproduce a ~ 1, g ~ 1.
        double ca = 1.5, cb = 0.5;
        if (terr > 0.09) {
        lds_f32* s_rs = (lds_f32*)(s_red + 64);
        for (int row = tid >> 3; row < nc; row += nt >> 3) {
            float rs = 0.f;
            for (int j = tid & 7; j < nc; j += 8) rs += (float)fabs(T[row * ld + j]);
            rs += dpp_f32<0xB1>(rs);   // quad_perm [1,0,3,2]
            rs += dpp_f32<0x4E>(rs);   // quad_perm [2,3,0,1]
            rs += dpp_f32<0x141>(rs);  // row_half_mirror
            if ((tid & 7) == 0) { s_rs[row] = rs * 1.000001f; s_rs[64 + row] = 2.f * (float)T[row * ld + row] - rs * 1.000001f; }
        }
        __syncthreads();
        float gm = lane < nc ? s_rs[lane] : 0.f;
        gm = fmaxf(gm, dpp_f32<0xB1>(gm));
        gm = fmaxf(gm, dpp_f32<0x4E>(gm));
        gm = fmaxf(gm, dpp_f32<0x141>(gm));
        gm = fmaxf(gm, dpp_f32<0x140>(gm));  // row_mirror: every lane of a 16-lane row holds the row maximum
        auto row_max = [&](int l0) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gm), l0)); };
        const double g = (double)fmaxf(fmaxf(row_max(0), row_max(16)), fmaxf(row_max(32), row_max(48)));
        // ... and a lower bound on lambda_min(T): Gershgorin's min_i (T_ii - sum_{j != i} |T_ij|), or 1 - ||T - I||_F
        float gl = lane < nc ? s_rs[64 + lane] : 3.0e38f;
        gl = fminf(gl, dpp_f32<0xB1>(gl));
        gl = fminf(gl, dpp_f32<0x4E>(gl));
        gl = fminf(gl, dpp_f32<0x141>(gl));
        gl = fminf(gl, dpp_f32<0x140>(gl));
        auto row_min = [&](int l0) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(gl), l0)); };
        const double glo = fmax(fmax((double)fminf(fminf(row_min(0), row_min(16)), fminf(row_min(32), row_min(48))), 1.0 - sqrt(terr)), 0.0);
        // Over-relaxed step (Chen & Chow's scaled Newton-Schulz): with the singular values of X / sqrt(g) in [l, 1] the
        // polynomial a x (3 - a^2 x^2) / 2 with a = sqrt(3 / (1 + l + l^2)) maps both ends to the same value and lifts the
        // small ones by up to 1.5 a per step instead of 1.5.  l comes from the lower bound above (0 while T is far from
        // diagonally dominant); a is capped at 1.25 (measured: 1.35 costs steps at nc = 64) so that an underestimated l cannot push the large singular values down
        // by more than 10 % (a -> 1 as l -> 1: the last steps are the plain quadratic iteration).
        const double gs = (g > 0.0 && g < 1.0) ? g : 1.0;
        const double l = sqrt(fmin(glo / gs, 1.0));
        const double al = fmin(PETAL_NS_CAP, sqrt(3.0 / (1.0 + l + l * l)));
        const double rg = 1.0 / sqrt(gs);
        ca = 1.5 * al * rg; cb = 0.5 * al * al * al * rg / gs;
        }
        if (use_mfma) {
            // Y = ca X - cb T X: A[i][k] = T[16 ti + i][k], B[k][j] = X[k][16 tj + j]
            for (int tile = wv; tile < ntile * ntile; tile += nw) {
                const int ti = tile / ntile, tj = tile - ti * ntile;
                const lds_f64* pa = T + (16 * ti + (lane & 15)) * ld + (lane >> 4);
                const lds_f64* pb = X + (lane >> 4) * ld + 16 * tj + (lane & 15);
                f64x4 acc = f64x4{0.0, 0.0, 0.0, 0.0};
                if constexpr (NTC > 0) {
#pragma unroll
                    for (int k0 = 0; k0 < 16 * NTC; k0 += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[k0], pb[k0 * ld], acc, 0, 0, 0);
                } else {
#pragma unroll 4
                    for (int k0 = 0; k0 < nc; k0 += 4) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[k0], pb[k0 * ld], acc, 0, 0, 0);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * ti + (lane >> 4) + 4 * r, j = 16 * tj + (lane & 15);
                    Y[i * ld + j] = ca * X[i * ld + j] - cb * acc[r];
                }
            }
        } else {
            for (int e = tid; e < nc * nc; e += nt) {
                const int i = e / nc, j = e - i * nc;
                double acc = 0;
                for (int k = 0; k < nc; ++k) acc += T[i * ld + k] * X[k * ld + j];
                Y[i * ld + j] = ca * X[i * ld + j] - cb * acc;
            }
        }
        __syncthreads();
        lds_f64* sw = X; X = Y; Y = sw;
    }
    return ok ? (double*)X : nullptr;
}

constexpr int ICA_TAIL_THREADS = 512;
template <int MB>
__global__ __launch_bounds__(ICA_TAIL_THREADS) void k_symdecorr(const double* Win, double* Wout, int nc, int mode, double* scratch,
                                                                int* zero2) {
    if (zero2 && threadIdx.x < 2) zero2[threadIdx.x] = 0;   // (the loop's {converged, iterations} state, cleared by the way)
    constexpr bool use_lds = MB > 0;
    extern __shared__ __attribute__((aligned(16))) double sm_sd[];
    JacWs ws = jac_carve(sm_sd, nc, blockDim.x);
    double* S = scratch; double* Zt = S + nc * nc; double* Z = Zt + nc * nc; double* Mm = Z + nc * nc; double* w = Mm + nc * nc;
    if (use_lds) { S = sm_sd + jac_ws_doubles(nc, blockDim.x); Zt = S + nc * (nc | 1); }
    // textbook (W W^T)^(-1/2) W is the orthogonal polar factor of W: scaled Newton-Schulz first, eigen-solver as fallback
    if constexpr (MB > 0) {
        if (mode == 0 || nc <= 2) {
            const int ld = polar_ld(nc);
            double* const P1 = S + nc * ld;   // (the polar iteration's own carving of the matrices' space: its pitch is not the solver's)
            for (int e = threadIdx.x; e < nc * nc; e += blockDim.x) S[(e / nc) * ld + (e % nc)] = Win[e];
            __syncthreads();
            constexpr int NTS = MB <= 4 ? MB : 0;   // (80 / 96 components: the unrolled products spill)
            const double* res = nc == 16 * NTS ? wg_polar_ns<NTS>(nc, S, P1, P1 + nc * ld, ws.red) : wg_polar_ns<0>(nc, S, P1, P1 + nc * ld, ws.red);
            if (res) {
                for (int e = threadIdx.x; e < nc * nc; e += blockDim.x) Wout[e] = res[(e / nc) * ld + (e % nc)];
                return;
            }
            __syncthreads();
        }
    }
    wg_symdecorr<MB>(Win, Wout, nc, mode, S, Zt, Z, Mm, w, ws);
}
template <int MB>
__global__ __launch_bounds__(ICA_TAIL_THREADS) void k_ica_tail(int nc, double n_total, double* W, const double* GX_gp, int mode,
                                                               double tol, int* state, int iter, double* scratch,
                                                               bf16x8* __restrict__ wpk3, double ortho_tol2, int* progress) {
    // (the loop's "converged" word is only LOOKED AT in front of the first write: its load, a memory round trip, travels with the
    // operands' instead of in front of them; a launch queued behind the converging one computes for nothing and leaves no trace)
    const int done = __builtin_nontemporal_load(state);
    constexpr bool use_lds = MB > 0;
    extern __shared__ __attribute__((aligned(16))) double sm_tail[];
    const int tid = threadIdx.x, nt = blockDim.x;
    JacWs ws = jac_carve(sm_tail, nc, nt);
    double* S = scratch; double* Zt = S + nc * nc; double* Z = Zt + nc * nc; double* Mm = Z + nc * nc; double* w = Mm + nc * nc;
    double* D = w + nc; double* W1 = D + nc * nc;
    if (use_lds) { S = sm_tail + jac_ws_doubles(nc, nt); Zt = S + nc * (nc | 1); }
    const double* GX = GX_gp; const double* gp = GX_gp + nc * nc;
    const double pinv = 1.0 / n_total;
    const int ldl = polar_ld(nc);
    double* const P1 = S + nc * ldl;   // (the polar iteration's own carving of the matrices' space)
    double* Wl = nullptr;        // LDS copy of W (fast path): one global read of W, none of W1
    const double* res = nullptr; // LDS result of the polar iteration
    if constexpr (MB > 0) {
        if (mode == 0 || nc <= 2) {
            Wl = P1 + 2 * nc * ldl;
            // D = GX / n - diag(g') W / n (ica.rs:334-342), straight into LDS; the loads of four trips are in flight together (a
            // load -> LDS-store loop pays a memory round trip per trip: eight in a row at nc = 64)
            for (int e0 = tid; e0 < nc * nc; e0 += 4 * nt) {
                double wv4[4], gx4[4], gp4[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int e = min(e0 + u * nt, nc * nc - 1);
                    wv4[u] = W[e]; gx4[u] = GX[e]; gp4[u] = gp[e / nc];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int e = e0 + u * nt;
                    if (e < nc * nc) {
                        const int i = e / nc, j = e - i * nc;
                        Wl[i * ldl + j] = wv4[u];
                        S[i * ldl + j] = gx4[u] * pinv - gp4[u] * pinv * wv4[u];
                    }
                }
            }
            __syncthreads();
            constexpr int NTS = MB <= 4 ? MB : 0;   // (80 / 96 components: the unrolled products spill)
            res = nc == 16 * NTS ? wg_polar_ns<NTS>(nc, S, P1, P1 + nc * ldl, ws.red, ortho_tol2)
                                 : wg_polar_ns<0>(nc, S, P1, P1 + nc * ldl, ws.red, ortho_tol2);  // ica.rs:343
        }
    }
    typedef __attribute__((address_space(3))) double lds_f64;   // (the polar factor and the copy of W are LDS: no FLAT accesses)
    const lds_f64* const resl = (const lds_f64*)res;
    const lds_f64* const Wll = (const lds_f64*)Wl;
    double lim = 0;  // ica.rs:344-354
    if (res) {
        // (eight lanes per row: one thread per row walked nc dependent LDS reads, ~4 us at 64 components)
        for (int i = tid >> 3; i < nc; i += nt >> 3) {
            double dot = 0;
            for (int j = tid & 7; j < nc; j += 8) dot += resl[i * ldl + j] * (mode == 1 ? Wll[j * ldl + i] : Wll[i * ldl + j]);  // ica.rs:345-349
            dot = oct_sum_f64(dot);
            lim = fmax(lim, fabs(fabs(dot) - 1.0));
        }
    } else {
        __syncthreads();
        for (int e = tid; e < nc * nc; e += nt) D[e] = GX[e] * pinv - gp[e / nc] * pinv * W[e];
        __syncthreads();
        wg_symdecorr<MB>(D, W1, nc, mode, S, Zt, Z, Mm, w, ws);
        for (int i = tid; i < nc; i += nt) {
            double dot = 0;
            for (int j = 0; j < nc; ++j) dot += W1[i * nc + j] * (mode == 1 ? W[j * nc + i] : W[i * nc + j]);
            lim = fmax(lim, fabs(fabs(dot) - 1.0));
        }
    }
    // max over the workgroup: inside each wave by shuffles, across the waves through LDS (one barrier pair; a tree over the 512
    // threads was nine)
    for (int off = 32; off > 0; off >>= 1) lim = fmax(lim, __shfl_xor(lim, off, 64));
    __syncthreads();                                              // (ws.red's last readers are done)
    if ((tid & 63) == 0) ws.red[tid >> 6] = lim;
    __syncthreads();
    double tl = 0;
    for (int w = 0; w < (nt >> 6); ++w) tl = fmax(tl, ws.red[w]);
    if (done) return;                                             // (uniform)
    if (res) { for (int e = tid; e < nc * nc; e += nt) W[e] = resl[(e / nc) * ldl + (e % nc)]; }
    else { for (int e = tid; e < nc * nc; e += nt) W[e] = W1[e]; }
    if (wpk3) {  // the next step kernel's operand planes (k_pack_w3's layout), straight from the new W
        const int NT = (nc + 15) >> 4, KCH = (16 * NT + 31) >> 5;
        for (int idx = tid; idx < KCH * NT * 64; idx += nt) {
            const int lane = idx & 63, tile = idx >> 6, u = tile % NT, kc = tile / NT;
            const int comp = 16 * u + (lane & 15), k0 = 32 * kc + 8 * (lane >> 4);
            f32x8 x;
#pragma unroll
            for (int e = 0; e < 8; ++e)
                x[e] = (comp < nc && k0 + e < nc) ? (float)(res ? resl[comp * ldl + k0 + e] : W1[comp * nc + k0 + e]) : 0.f;
            bf16x8 h, m, l;
            split3(x, h, m, l);
            wpk3[(tile * 3 + 0) * 64 + lane] = h;
            wpk3[(tile * 3 + 1) * 64 + lane] = m;
            wpk3[(tile * 3 + 2) * 64 + lane] = l;
        }
    }
    if (tid == 0 && (tl < tol)) { state[0] = 1; state[1] = iter + 1; }  // ica.rs:355-357
    if (tid == 0 && progress) {  // host-visible progress: plain stores to pinned memory, the host polls without a sync
        if (tl < tol) __hip_atomic_store(progress, iter + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(progress + 1, iter + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ void k_dscal(double* x, int64_t count, double alpha) {
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e < count) x[e] *= alpha;
}
__global__ void k_daxpy(int64_t count, double alpha, const double* x, double* y) {
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e < count) y[e] += alpha * x[e];
}
__global__ void k_dvec(int mode, const double* x, double* y, int64_t count, double thr) {
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e >= count) return;
    if (mode == 0) y[e] = sqrt(fmax(x[e], 0.0));
    else if (mode == 2) y[e] = x[e] * x[e];
    else y[e] = (x[e] > thr * x[0] && x[e] > 0.0) ? 1.0 / x[e] : 0.0;
}
__global__ void k_sigma_inv(const double* __restrict__ lam, double* __restrict__ sig, double* __restrict__ inv, int64_t count, double thr) {
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e >= count) return;
    const double s = sqrt(fmax(lam[e], 0.0)), s0 = sqrt(fmax(lam[0], 0.0));
    sig[e] = s;
    inv[e] = (s > thr * s0 && s > 0.0) ? 1.0 / s : 0.0;
}
// The fitted components straight in the caller's layout and type (pca.rs:543: rows of V^T): comp[j][i] = (T)(B^T u_j)[i] / sigma_j
// for j < k, from Bt (d x l fp64), the eigenvectors Uh (columns) and eigenvalues lam of B B^T.  1 / sigma_j is formed here
// (sigma_j = sqrt(lam_j); 0 below thr sigma_0, the rule of k_sigma_inv), so the fit ends with one small launch and a k x d copy in
// the output type instead of a scaling launch, an fp64 d x l product and a d x l fp64 copy.  Block = 64 i's x 16 j's.
template <class T>
__global__ __launch_bounds__(256) void k_components_out(const double* __restrict__ Bt, int64_t ldb, const double* __restrict__ Uh,
                                                        int64_t ldu, const double* __restrict__ lam, double thr, int64_t d, int L,
                                                        int64_t k, T* __restrict__ comp) {
    __shared__ double sB[64][65];       // [i][l] of the current 64-wide slice of l
    __shared__ double sU[64][16];       // [l][j]
    const int tid = threadIdx.x, ti = tid & 15, tj = tid >> 4;
    const int64_t i0 = (int64_t)blockIdx.x * 64, j0 = (int64_t)blockIdx.y * 16;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int l0 = 0; l0 < L; l0 += 64) {
        // (all of a slice's loads are issued before the first LDS store waits for one: a runtime-trip loop of load -> store
        // pairs pays an L2 round trip per pair)
        double vb[16], vu[4];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int r = (tid >> 6) + 4 * u, l = l0 + (tid & 63);
            vb[u] = (i0 + r < d && l < L) ? Bt[(i0 + r) * ldb + l] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int l = l0 + (tid >> 4) + 16 * u;
            vu[u] = (l < L && j0 + ti < k) ? Uh[(int64_t)l * ldu + j0 + ti] : 0.0;
        }
        __syncthreads();   // (the previous slice's readers are done)
#pragma unroll
        for (int u = 0; u < 16; ++u) sB[(tid >> 6) + 4 * u][tid & 63] = vb[u];
#pragma unroll
        for (int u = 0; u < 4; ++u) sU[(tid >> 4) + 16 * u][ti] = vu[u];
        __syncthreads();
#pragma unroll 8
        for (int l = 0; l < 64; ++l) {
            const double u = sU[l][tj];
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] += sB[ti + 16 * r][l] * u;
        }
    }
    const int64_t j = j0 + tj;
    if (j < k) {
        const double s = sqrt(fmax(lam[j], 0.0)), s0 = sqrt(fmax(lam[0], 0.0));
        const double inv = (s > thr * s0 && s > 0.0) ? 1.0 / s : 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t i = i0 + ti + 16 * r;
            if (i < d) comp[j * d + i] = (T)(acc[r] * inv);
        }
    }
}
// exact Pca's small-matrix tail, two one-launch helpers:
// P[i][j] = j < r ? V[i][j] * inv[j] : 0 (rows x rp, the right-hand side of U = Xc V / sigma, zero padded) ...
__global__ void k_scale_pad_cols(const double* __restrict__ V, int64_t ldv, const double* __restrict__ inv, int64_t rows, int64_t r,
                                 int64_t rp, double* __restrict__ P) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rows * rp) return;
    const int64_t i = e / rp, j = e - i * rp;
    P[e] = j < r ? V[i * ldv + j] * inv[j] : 0.0;
}
// ... and the components in the caller's layout and type: comp[j][i] = (T)V[i][j] for j < k, i < d (32 x 32 tiles through LDS)
template <class T>
__global__ __launch_bounds__(256) void k_transpose_out(const double* __restrict__ V, int64_t ldv, int64_t d, int64_t k, T* __restrict__ comp) {
    __shared__ double tile[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int64_t i0 = (int64_t)blockIdx.x * 32, j0 = (int64_t)blockIdx.y * 32;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t i = i0 + ty + 8 * u, j = j0 + tx;
        tile[ty + 8 * u][tx] = (i < d && j < k) ? V[i * ldv + j] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int64_t j = j0 + ty + 8 * u, i = i0 + tx;
        if (j < k && i < d) comp[j * d + i] = (T)tile[tx][ty + 8 * u];
    }
}
// column means from the per-block partial sums of k_colsum_part2, in one launch: fixed-order fp64 sum of the parts,
// mu64[j] = sum / n_total for j < d (the sums of squares at d <= j < w stay unscaled), muT[j] = (T)mu64[j]
// part_lo (nullable): the low words of the parts (k_colsum_part2): the sum stays a (high, low) pair to the end and the mean is ONE
// rounding of it -- quotient, exact remainder by fma, correction; n_total is then used, not its rounded reciprocal
template <class T>
__global__ __launch_bounds__(256) void k_colmean_final(const double* __restrict__ part, const double* __restrict__ part_lo, int64_t nparts,
                                                       int64_t w, int64_t d, double inv_n, double n_total, double* __restrict__ mu64,
                                                       T* __restrict__ muT) {
    __shared__ double red[32][9], redc[32][9];
    const int e = threadIdx.x & 7, pl = threadIdx.x >> 3;  // 8 outputs x 32 part-lanes per block
    const int64_t j = (int64_t)blockIdx.x * 8 + e;
    const bool pairs = sizeof(T) == 8 && part_lo;
    double acc = 0, lo = 0;
    if (j < w) {
        if (pairs) {
            for (int64_t p = pl; p < nparts; p += 32) { two_sum_acc(acc, lo, part[p * w + j]); lo += part_lo[p * w + j]; }
        } else {
            for (int64_t p = pl; p < nparts; p += 32) acc += part[p * w + j];
        }
    }
    red[pl][e] = acc; redc[pl][e] = lo;
    __syncthreads();
    if (pl == 0 && j < w) {
        double t = 0;
        if (pairs) {
            double c = 0;
#pragma unroll
            for (int k = 0; k < 32; ++k) { two_sum_acc(t, c, red[k][e]); c += redc[k][e]; }
            if (j < d) {
                const double q = t / n_total;
                t = q + (fma(-q, n_total, t) + c) / n_total;
                muT[j] = (T)t;
            } else {
                t += c;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 32; ++k) t += red[k][e];
            if (j < d) { t *= inv_n; muT[j] = (T)t; }
        }
        mu64[j] = t;
    }
}
__global__ void k_dscale_cols(double* A, int64_t M, int64_t N, int64_t lda, const double* s) {
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e < M * N) A[(e / N) * lda + (e % N)] *= s[e % N];
}
template <class T>
__global__ void k_cvt_from_f64(T* dst, const double* src, int64_t count) {
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e < count) dst[e] = (T)src[e];
}
// dst (rows_p x cols_p fp64, zero padded) <- the leading rows x cols block of src (row-major, leading dimension lds)
template <class T>
__global__ void k_pad_to_f64(double* __restrict__ dst, int64_t rows_p, int64_t cols_p, const T* __restrict__ src, int64_t rows,
                             int64_t cols, int64_t lds, double* __restrict__ zero_ptr, int64_t zero_count) {
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e < zero_count) zero_ptr[e] = 0.0;
    if (e >= rows_p * cols_p) return;
    const int64_t r = e / cols_p, c = e - r * cols_p;
    dst[e] = (r < rows && c < cols) ? (double)src[r * lds + c] : 0.0;
}
template <class T>
__global__ void k_cvt_to_f64(double* dst, const T* src, int64_t count) {
    const int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (e < count) dst[e] = (double)src[e];
}

// ---- FastICA step with more than 64 components: the pieces around the two GEMM kernels -------------------------------
__global__ void k_transpose_pad(const double* __restrict__ W, int64_t nc, double* __restrict__ WT, int64_t ncp) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= ncp * ncp) return;
    const int64_t k = e / ncp, i = e - k * ncp;  // WT[k][i] = W[i][k]
    WT[e] = (k < nc && i < nc) ? W[i * nc + k] : 0.0;
}
template <class T>
__global__ void k_tanh_inplace(T* __restrict__ x, int64_t count) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < count) x[e] = (T)tanh((double)x[e]);
}
// the other contrasts (k_ica_step.inc: ica_contrast): S <- g(S) in place, and the column sums of g'(S) over this block's 256 rows to
// gp_part[block][ncp] -- one thread per column walks the rows in order, so the sums are the same bits on every run
template <class T, int G>
__global__ __launch_bounds__(256) void k_contrast_inplace(T* __restrict__ S, int64_t n, int64_t ncp, double* __restrict__ gp_part) {
    const int64_t r0 = (int64_t)blockIdx.x * 256, r1 = min(n, r0 + 256);
    for (int64_t c = threadIdx.x; c < ncp; c += 256) {
        double acc = 0;
        for (int64_t r = r0; r < r1; ++r) {
            T g, gp;
            ica_contrast<G>(S[r * ncp + c], g, gp);
            S[r * ncp + c] = g;
            acc += (double)gp;
        }
        gp_part[(int64_t)blockIdx.x * ncp + c] = acc;
    }
}
// GX_gp = [ GXp[:nc, :nc] | sum over the row blocks of gp_part, in block order ]
__global__ void k_ica_big_out_g(const double* __restrict__ GXp, const double* __restrict__ gp_part, int64_t nparts, int64_t nc, int64_t ncp,
                                double* __restrict__ GX_gp, const int* __restrict__ state) {
    if (state && state[0]) return;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < nc * nc) GX_gp[e] = GXp[(e / nc) * ncp + (e % nc)];
    else if (e < nc * nc + nc) {
        double s = 0;
        for (int64_t p = 0; p < nparts; ++p) s += gp_part[p * ncp + (e - nc * nc)];
        GX_gp[e] = s;
    }
}
// GX_gp = [ GXp[:nc, :nc] | n - sum_s g_si^2 ]   (sum_s (1 - g^2) = n - sum g^2, fp64)
__global__ void k_ica_big_out(const double* __restrict__ GXp, const double* __restrict__ sumsq, double n, int64_t nc, int64_t ncp,
                              double* __restrict__ GX_gp, const int* __restrict__ state) {
    if (state && state[0]) return;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < nc * nc) GX_gp[e] = GXp[(e / nc) * ncp + (e % nc)];
    else if (e < nc * nc + nc) GX_gp[e] = n - sumsq[e - nc * nc];
}


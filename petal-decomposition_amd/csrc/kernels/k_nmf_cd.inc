// k_nmf_cd.inc -- part of the ONE translation unit hip_ops.hip (textually included there, inside namespace petal): Nmf by coordinate
// descent (include/petal_hip_nmf_cd.h; scikit-learn's NMF(solver="cd"), shuffle=False).  One iteration is ONE fused pass over X
// (k_nmf_cd_pass: k_nmf_pass's frame with the multiplicative rule replaced by a Gauss-Seidel sweep over the coordinates of each row)
//     Z = X H^T,  S = H H^T + l2 I (the first k diagonal entries),  z = Z[i, :] - l1,  one sweep of row w of W for t = 0 .. KP - 1:
//         grad = -z[t] + sum_r S[t][r] w[r]   (the CURRENT w);   pg = w[t] == 0 ? min(0, grad) : grad;   violation += |pg|
//         if S[t][t] != 0:  w[t] = max(w[t] - grad / S[t][t], 0)
//     A = W^T X,  B = W^T W      (the NEW W in A and B)
// and the same sweep on the dp rows of H^T from A and B (k_nmf_cd_hrule).  eps is not used.  Device layouts are k_nmf.inc's.
// ------------------------------------------------------------------------------------------------
// The sweep.  The 256 lanes of a workgroup are 16 rows x 16 lanes: lane j of a row's group owns the KT = KP / 16 coordinates
// 16 u + j and keeps its share of g = S w - z in registers.  g is formed afresh from the row of w (in LDS) at the start of every sweep
// -- r = 0 .. KP - 1 in order -- so the sweeps of a transform do not accumulate drift.  Step t: every lane evaluates the owner's
// expressions on its own registers (the division costs a SIMD the same for one lane as for 64), the step delta = w_new - w of the
// owner lane t & 15 is broadcast inside the 16-lane group, and every lane adds delta S[t][16 u + j] to its g.  S is symmetric and sits
// in LDS (KP x KP, with l2 on the first k diagonal entries only: a padded component has S[t][t] = 0, is skipped, stays zero and adds
// nothing to the violation: z = -l1, w = 0, so grad >= 0 and pg = 0).  The order of every sum is fixed by the shape alone.
// (S is the same for every sweep and every tile, and the compiler would keep all of a lane's KP KT entries in registers across the
// sweeps -- 512 at 64 components: they spill; the offset is made opaque once per sweep so that every step reads its row of S from LDS)
template <int KT>
__device__ __forceinline__ double nmf_cd_sweep(double (&w)[KT], const double (&z)[KT], const double* sl0, const double* wrow, int j, int lane) {
    constexpr int KP = 16 * KT;
    int opaque = 0;
    asm volatile("" : "+v"(opaque));
    const double* sl = sl0 + opaque;
    double g[KT];
#pragma unroll
    for (int u = 0; u < KT; ++u) g[u] = 0.0;
#pragma unroll 4
    for (int r = 0; r < KP; ++r) {
        const double wr = wrow[r];
#pragma unroll
        for (int u = 0; u < KT; ++u) g[u] = fma(sl[r * KP + 16 * u + j], wr, g[u]);
    }
#pragma unroll
    for (int u = 0; u < KT; ++u) g[u] -= z[u];
    double viol = 0.0;
#pragma unroll
    for (int ut = 0; ut < KT; ++ut) {
#pragma unroll 1
        for (int jt = 0; jt < 16; ++jt) {
            const int t = 16 * ut + jt;
            const double stt = sl[t * KP + t];
            const double gr = g[ut], wv = w[ut];
            const double wn = stt != 0.0 ? fmax(wv - gr / stt, 0.0) : wv;
            const double pg = wv == 0.0 ? fmin(0.0, gr) : gr;
            const double dl = __shfl(wn - wv, (lane & 48) | jt, 64);
            if (j == jt) {
                w[ut] = wn;
                viol += fabs(pg);
            }
#pragma unroll
            for (int u = 0; u < KT; ++u) g[u] = fma(dl, sl[t * KP + 16 * u + j], g[u]);
        }
    }
    return viol;
}

// the sum of one value per thread over a workgroup of 256, a fixed tree; red: 256 doubles of LDS nobody else touches
__device__ __forceinline__ double nmf_cd_wgsum(double v, double* red, int tid) {
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    return red[0];
}

template <int KT, bool AB>
constexpr size_t nmf_cd_lds_bytes() { return nmf_lds_bytes<KT, AB>() + sizeof(double) * (256 * KT * KT + 256); }

// k_nmf_pass's frame (k_nmf.inc): four waves on a tile of 16 rows, persistent workgroups, product 1 over the waves' feature slices, the
// partial Z in LDS, A and B from the tile of W in LDS, one slab per workgroup.  The middle is the sweep: thread (row R = tid >> 4,
// j = tid & 15) adds the four waves' partials of its coordinates IN WAVE ORDER straight from zpart, sweeps `inner` times (inner = 0
// leaves W alone; from_zero: transform's start) and leaves its coordinates of the new row in the tile of W.  violp (nullable; g x inner
// doubles): sweep s of workgroup b adds its tiles' violations, in tile order, to violp[b inner + s].
template <class T, int KT, int FT, bool AB>
__global__ __launch_bounds__(64 * NMF_WAVES) void k_nmf_cd_pass(const T* __restrict__ X, int64_t ldx, int64_t n, int nt, const double* __restrict__ H,
                                                     int64_t ldh, const double* __restrict__ HHt, double* W, int from_zero, int k, double l1,
                                                     double l2, int inner, double* __restrict__ slabA, double* __restrict__ slabB,
                                                     double* __restrict__ violp) {
    constexpr int KP = 16 * KT, WLD = nmf_wld<KT>();
    constexpr int E = 16 / (int)sizeof(T), S = 16 / (4 * E);
    typedef T txe __attribute__((ext_vector_type(E)));
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(32))) double nmf_cd_lds[];
    double* zpart = nmf_cd_lds;                        // [wave][component tile][lane] f64x4
    double* wl = nmf_cd_lds + NMF_WAVES * KT * 256;    // the tile of W: 16 rows x KP, row pitch WLD
    double* bl = wl + 16 * WLD;                        // AB: the KT x KT accumulator tiles of B in fragment order, [tile][lane] f64x4
    double* sl = bl + (AB ? 256 * KT * KT : 0);        // S = H H^T + l2 I, KP x KP
    double* red = sl + KP * KP;                        // the violation's tree
    constexpr int BT = (KT * KT + NMF_WAVES - 1) / NMF_WAVES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int R = tid >> 4, j = tid & 15;              // the sweep's view: row of the tile, lane of the row's group
    const int ft0 = wave * FT;
    const int64_t ntiles = (n + 15) / 16;
    for (int idx = tid; idx < KP * KP; idx += 64 * NMF_WAVES) {
        const int r = idx / KP, c = idx - r * KP;
        sl[idx] = HHt[idx] + (r == c && r < k ? l2 : 0.0);
    }
    if (violp && tid == 0)
        for (int s = 0; s < inner; ++s) violp[(int64_t)blockIdx.x * inner + s] = 0.0;
    double vacc = 0.0;                                 // inner == 1 (a fit's iteration): this thread's violation over the workgroup's tiles
    f64x4 accA[KT][FT];
    if (AB) {
#pragma unroll
        for (int t = 0; t < KT; ++t)
#pragma unroll
            for (int jj = 0; jj < FT; ++jj) accA[t][jj] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int u = 0; u < BT; ++u)
            if (wave + NMF_WAVES * u < KT * KT) *reinterpret_cast<f64x4*>(bl + ((wave + NMF_WAVES * u) * 64 + lane) * 4) = f64x4{0.0, 0.0, 0.0, 0.0};
    }
    txe xr[FT][S];
    const auto load_rows = [&](int64_t tile) {
        const T* xp = X + min(tile * 16 + i, n - 1) * ldx + E * q;
#pragma unroll
        for (int jj = 0; jj < FT; ++jj) {
            const bool live = ft0 + jj < nt;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const txe v = *reinterpret_cast<const txe*>(xp + 16 * min(ft0 + jj, nt - 1) + 4 * E * s);
#pragma unroll
                for (int e = 0; e < E; ++e) xr[jj][s][e] = live ? v[e] : T(0);
            }
        }
    };
    if ((int64_t)blockIdx.x < ntiles) load_rows(blockIdx.x);
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * 16;
        const double* Ht = H;
        asm volatile("" : "+s"(Ht));   // (k_nmf_pass: H is read again by every tile, from L1 / L2, instead of living in registers)
        for (int idx = tid; idx < 16 * KP; idx += 64 * NMF_WAVES) {
            const int r = idx / KP, c = idx - r * KP;
            wl[r * WLD + c] = (row0 + r < n && !from_zero) ? W[(row0 + r) * KP + c] : 0.0;
        }
        // product 1 over this wave's features
        f64x4 z[KT];
#pragma unroll
        for (int t = 0; t < KT; ++t) z[t] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int jj = 0; jj < FT; ++jj) {
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const double* hq = Ht + 16 * min(ft0 + jj, nt - 1) + 4 * E * s + E * q + (int64_t)i * ldh;
#pragma unroll
                for (int t = 0; t < KT; ++t) {
                    const double* hp = hq + (int64_t)(16 * t) * ldh;
                    double hv[E];
#pragma unroll
                    for (int e = 0; e < E; e += 2) {
                        const f64x2 h2 = *reinterpret_cast<const f64x2*>(hp + e);
                        hv[e] = h2[0];
                        hv[e + 1] = h2[1];
                    }
#pragma unroll
                    for (int e = 0; e < E; ++e) z[t] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)xr[jj][s][e], hv[e], z[t], 0, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int t = 0; t < KT; ++t) *reinterpret_cast<f64x4*>(zpart + ((wave * KT + t) * 64 + lane) * 4) = z[t];
        if (tile + gridDim.x < ntiles) load_rows(tile + gridDim.x);
        __syncthreads();
        // the sweep: Z[row R][component 16 u + j] is register R >> 2 of lane j + 16 (R & 3) in zpart's fragment order
        if (inner > 0) {
            const bool live = row0 + R < n;
            double zr[KT], wr[KT];
#pragma unroll
            for (int u = 0; u < KT; ++u) {
                double s = 0.0;
#pragma unroll
                for (int w = 0; w < NMF_WAVES; ++w) s += zpart[((w * KT + u) * 64 + j + 16 * (R & 3)) * 4 + (R >> 2)];
                zr[u] = (live ? s : 0.0) - l1;          // (a row past n: z = -l1, w = 0 -- it stays zero and adds no violation)
                wr[u] = wl[R * WLD + 16 * u + j];
            }
            for (int it = 0; it < inner; ++it) {
                const double v = nmf_cd_sweep<KT>(wr, zr, sl, wl + R * WLD, j, lane);
                __syncthreads();   // every read of the old rows is done
#pragma unroll
                for (int u = 0; u < KT; ++u) wl[R * WLD + 16 * u + j] = wr[u];
                if (violp) {
                    if (inner == 1) vacc += v;
                    else {
                        const double s = nmf_cd_wgsum(v, red, tid);
                        if (tid == 0) violp[(int64_t)blockIdx.x * inner + it] += s;
                    }
                }
                __syncthreads();
            }
            if (live) {
#pragma unroll
                for (int u = 0; u < KT; ++u) W[(row0 + R) * KP + 16 * u + j] = wr[u];
            }
        }
        if (AB) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double wv[KT];
#pragma unroll
                for (int u = 0; u < KT; ++u) wv[u] = wl[(4 * r + q) * WLD + 16 * u + i];
                const T* xp = X + min(row0 + 4 * r + q, n - 1) * ldx + i;
#pragma unroll
                for (int jj = 0; jj < FT; ++jj) {
                    const double xb = (double)xp[16 * min(ft0 + jj, nt - 1)];
#pragma unroll
                    for (int u = 0; u < KT; ++u) accA[u][jj] = __builtin_amdgcn_mfma_f64_16x16x4f64(wv[u], xb, accA[u][jj], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int u = 0; u < BT; ++u) {
                const int p = wave + NMF_WAVES * u;   // p = ti KT + tj
                if (p < KT * KT) {
                    const int ti = p / KT, tj = p - ti * KT;
                    f64x4 acc = *reinterpret_cast<const f64x4*>(bl + (p * 64 + lane) * 4);
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(wl[(4 * r + q) * WLD + 16 * ti + i], wl[(4 * r + q) * WLD + 16 * tj + i], acc, 0, 0, 0);
                    *reinterpret_cast<f64x4*>(bl + (p * 64 + lane) * 4) = acc;
                }
            }
        }
        __syncthreads();   // the tile of W and the partials are free again
    }
    if (violp && inner == 1) {
        const double s = nmf_cd_wgsum(vacc, red, tid);
        if (tid == 0) violp[blockIdx.x] = s;
    }
    if (AB) {
        const int64_t dp = 16 * (int64_t)nt;
        double* sa = slabA + (int64_t)blockIdx.x * KP * dp;
#pragma unroll
        for (int u = 0; u < KT; ++u)
#pragma unroll
            for (int jj = 0; jj < FT; ++jj)
                if (ft0 + jj < nt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) sa[(int64_t)(16 * u + 4 * r + q) * dp + 16 * (ft0 + jj) + i] = accA[u][jj][r];
                }
        double* sb = slabB + (int64_t)blockIdx.x * KP * KP;
#pragma unroll
        for (int u = 0; u < BT; ++u) {
            const int p = wave + NMF_WAVES * u;
            if (p < KT * KT) {
                const int ti = p / KT, tj = p - ti * KT;
                const f64x4 acc = *reinterpret_cast<const f64x4*>(bl + (p * 64 + lane) * 4);
#pragma unroll
                for (int r = 0; r < 4; ++r) sb[(16 * ti + 4 * r + q) * KP + 16 * tj + i] = acc[r];
            }
        }
    }
}

// out[s] = sum_b part[b inner + s], b in order: the fixed-order sum of the workgroups' violations.
__global__ __launch_bounds__(256) void k_nmf_cd_violsum(const double* __restrict__ part, int g, int inner, double* __restrict__ out) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= inner) return;
    double v = 0.0;
    for (int b = 0; b < g; ++b) v += part[(int64_t)b * inner + s];
    out[s] = v;
}

// The H side: the same sweep on the rows of H^T, one 16-lane group per feature f (16 features per workgroup), with z = A[:, f] - l1 and
// S = B + l2 I on the first k diagonal entries; H (KP x dp, ld dp) is read and written in place with the stride dp.  A padding feature
// has A = 0 and H = 0: grad = l1 >= 0, so it stays zero and adds no violation.  violp[workgroup] = the workgroup's violation.
template <int KT>
__global__ __launch_bounds__(256) void k_nmf_cd_hrule(double* __restrict__ H, const double* __restrict__ A, const double* __restrict__ B, int64_t dp,
                                                      int k, double l1, double l2, double* __restrict__ violp) {
    constexpr int KP = 16 * KT, WLD = nmf_wld<KT>();
    __shared__ double sl[KP * KP];
    __shared__ double wl[16 * WLD];
    __shared__ double red[256];
    const int tid = threadIdx.x, lane = tid & 63, R = tid >> 4, j = tid & 15;
    const int64_t f = (int64_t)blockIdx.x * 16 + R;   // (dp is a multiple of 16: every group has a feature)
    for (int idx = tid; idx < KP * KP; idx += 256) {
        const int r = idx / KP, c = idx - r * KP;
        sl[idx] = B[idx] + (r == c && r < k ? l2 : 0.0);
    }
    double zr[KT], wr[KT];
#pragma unroll
    for (int u = 0; u < KT; ++u) {
        zr[u] = A[(int64_t)(16 * u + j) * dp + f] - l1;
        wr[u] = H[(int64_t)(16 * u + j) * dp + f];
        wl[R * WLD + 16 * u + j] = wr[u];
    }
    __syncthreads();
    const double v = nmf_cd_sweep<KT>(wr, zr, sl, wl + R * WLD, j, lane);
#pragma unroll
    for (int u = 0; u < KT; ++u) H[(int64_t)(16 * u + j) * dp + f] = wr[u];
    const double s = nmf_cd_wgsum(v, red, tid);
    if (tid == 0) violp[blockIdx.x] = s;
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------------
template <class T, int KT, int FT, bool AB>
static void nmf_cd_pass_launch(Dev* d, int g, const T* X, int64_t ldx, int64_t n, int nt, const double* H, int64_t ldh, const double* HHt, double* W,
                               int from_zero, int k, double l1, double l2, int inner, double* slabA, double* slabB, double* violp) {
    const void* fn = reinterpret_cast<const void*>(k_nmf_cd_pass<T, KT, FT, AB>);
    constexpr size_t lds = nmf_cd_lds_bytes<KT, AB>();
    if (lds > 64 * 1024) set_max_lds(d, fn);
    hipLaunchKernelGGL((k_nmf_cd_pass<T, KT, FT, AB>), dim3(g), dim3(64 * NMF_WAVES), lds, d->stream, X, ldx, n, nt, H, ldh, HHt, W, from_zero, k,
                       l1, l2, inner, slabA, slabB, violp);
}
template <class T, int KT, int FT>
static void nmf_cd_pass_ab(Dev* d, bool ab, int g, const T* X, int64_t ldx, int64_t n, int nt, const double* H, int64_t ldh, const double* HHt,
                           double* W, int from_zero, int k, double l1, double l2, int inner, double* slabA, double* slabB, double* violp) {
    if (ab) nmf_cd_pass_launch<T, KT, FT, true>(d, g, X, ldx, n, nt, H, ldh, HHt, W, from_zero, k, l1, l2, inner, slabA, slabB, violp);
    else nmf_cd_pass_launch<T, KT, FT, false>(d, g, X, ldx, n, nt, H, ldh, HHt, W, from_zero, k, l1, l2, inner, slabA, slabB, violp);
}
template <class T, int KT>
static void nmf_cd_pass_ft(Dev* d, bool ab, int g, const T* X, int64_t ldx, int64_t n, int nt, const double* H, int64_t ldh, const double* HHt,
                           double* W, int from_zero, int k, double l1, double l2, int inner, double* slabA, double* slabB, double* violp) {
    if (nt <= NMF_WAVES) nmf_cd_pass_ab<T, KT, 1>(d, ab, g, X, ldx, n, nt, H, ldh, HHt, W, from_zero, k, l1, l2, inner, slabA, slabB, violp);
    else if (nt <= 2 * NMF_WAVES) nmf_cd_pass_ab<T, KT, 2>(d, ab, g, X, ldx, n, nt, H, ldh, HHt, W, from_zero, k, l1, l2, inner, slabA, slabB, violp);
    else if (nt <= 4 * NMF_WAVES) nmf_cd_pass_ab<T, KT, 4>(d, ab, g, X, ldx, n, nt, H, ldh, HHt, W, from_zero, k, l1, l2, inner, slabA, slabB, violp);
    else nmf_cd_pass_ab<T, KT, 8>(d, ab, g, X, ldx, n, nt, H, ldh, HHt, W, from_zero, k, l1, l2, inner, slabA, slabB, violp);
}

bool op_nmf_cd_pass(Dev* d, int dt, const void* X, int64_t n, int64_t dp, int64_t ldx, const double* H, const double* HHt, int64_t k, int64_t kp,
                    double* W, bool from_zero, double l1, double l2, int64_t inner, double* A, double* B, double* viol) {
    const int64_t el = dt == F32 ? 4 : 2;
    // op_nmf_pass's envelope: 16, 32 or 64 padded components (k = 33 .. 48 pads to 48: the composed path), at most 512 padded columns
    if (kp != 16 && kp != 32 && kp != 64) return false;
    if (n < 1 || n > (int64_t(1) << 40) || k < 1 || k > 64 || kp != nmf_padded_k(k) || dp < 16 || dp % 16 || dp > 512 || ldx < dp || ldx % el ||
        !aligned16(X) || !aligned16(H) || inner < 0 || inner > (int64_t(1) << 20) || !W || !aligned16(W) || !HHt || ((A == nullptr) != (B == nullptr)))
        return false;
    const bool ab = A != nullptr;
    const int nt = (int)(dp / 16), kt = (int)(kp / 16);
    const int g = (int)std::min<int64_t>((n + 15) / 16, NMF_MAX_WG);
    double* slabA = ab ? (double*)dev_alloc(d, sizeof(double) * size_t(g) * kp * (dp + kp)) : nullptr;   // g slabs of A, then g slabs of B
    double* slabB = ab ? slabA + size_t(g) * kp * dp : nullptr;
    double* violp = viol && inner > 0 ? (double*)dev_alloc(d, sizeof(double) * size_t(g) * size_t(inner)) : nullptr;
    TagScope ts(d);
#define PETAL_NMF_CD_PASS(KTv) DISPATCH_T(dt, (nmf_cd_pass_ft<T, KTv>(d, ab, g, (const T*)X, ldx, n, nt, H, dp, HHt, W, from_zero ? 1 : 0, (int)k, l1, l2, (int)inner, slabA, slabB, violp)))
    if (kt == 1) PETAL_NMF_CD_PASS(1);
    else if (kt == 2) PETAL_NMF_CD_PASS(2);
    else PETAL_NMF_CD_PASS(4);
#undef PETAL_NMF_CD_PASS
    launch_check();
    ts.stop();
    if (ab) {
        hipLaunchKernelGGL(k_nmf_slabsum, dim3((unsigned)cdiv64(kp * dp, 256)), dim3(256), 0, d->stream, (const double*)slabA, g, kp * dp, A);
        launch_check();
        hipLaunchKernelGGL(k_nmf_slabsum, dim3((unsigned)cdiv64(kp * kp, 256)), dim3(256), 0, d->stream, (const double*)slabB, g, kp * kp, B);
        launch_check();
        dev_free(d, slabA);
    }
    if (violp) {
        hipLaunchKernelGGL(k_nmf_cd_violsum, dim3((unsigned)cdiv64(inner, 256)), dim3(256), 0, d->stream, (const double*)violp, g, (int)inner, viol);
        launch_check();
        dev_free(d, violp);
    }
    return true;
}

bool op_nmf_cd_hupdate(Dev* d, int64_t k, int64_t kp, int64_t dp, const double* A, const double* B, double* H, double* HHt, double l1, double l2,
                       double* dots2, double* viol1) {
    if ((kp != 16 && kp != 32 && kp != 64) || k < 1 || k > kp || dp < 16 || dp % 16 || dp > (int64_t(1) << 24) || !viol1) return false;
    const int g = (int)(dp / 16);
    double* violp = (double*)dev_alloc(d, sizeof(double) * size_t(g));
    if (kp == 16) hipLaunchKernelGGL((k_nmf_cd_hrule<1>), dim3(g), dim3(256), 0, d->stream, H, A, B, dp, (int)k, l1, l2, violp);
    else if (kp == 32) hipLaunchKernelGGL((k_nmf_cd_hrule<2>), dim3(g), dim3(256), 0, d->stream, H, A, B, dp, (int)k, l1, l2, violp);
    else hipLaunchKernelGGL((k_nmf_cd_hrule<4>), dim3(g), dim3(256), 0, d->stream, H, A, B, dp, (int)k, l1, l2, violp);
    launch_check();
    hipLaunchKernelGGL(k_nmf_cd_violsum, dim3(1), dim3(256), 0, d->stream, (const double*)violp, g, 1, viol1);
    launch_check();
    dev_free(d, violp);
    op_dgemm(d, false, true, kp, kp, dp, 1.0, H, dp, H, dp, 0.0, HHt, kp);
    hipLaunchKernelGGL(k_nmf_dots, dim3(1), dim3(256), 0, d->stream, A, (const double*)H, kp * dp, B, (const double*)HHt, kp * kp, dots2);
    launch_check();
    return true;
}

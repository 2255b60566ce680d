// k_nmf_kl_dense.inc -- part of the ONE translation unit hip_ops.hip (textually included there, inside namespace petal): Nmf with the
// generalised Kullback-Leibler loss on DENSE data (include/petal_hip_nmf_kl_dense.h).  One iteration is ONE fused pass over X
// (k_nmf_kl_pass)
//     WH = W H, WH[WH < eps] = eps, Q = X / WH,  den = rowsum(H) + l1 + l2 W, den[den == 0] = eps,  W <- W o ((Q H^T) / den),
//     Q' = X / max(W H, eps) with the NEW W,  A = W^T Q',  c = colsum(W)
// and k x d work on H (k_nmf_kl_hrule, k_nmf_kl_rowsum).  Device layouts are k_nmf.inc's: W n x KP, H and A KP x dp (ld dp), fp64,
// KP = 16, 32 or 64 >= k, ZERO in the padding (a padded component stays zero: 0 * (0 / den); a padding column gives 0 / eps = 0).
// ------------------------------------------------------------------------------------------------
// The fused pass is k_nmf_pass's frame with a different middle (the operand layouts of v_mfma_f64_16x16x4_f64 are stated there).  With
// (i, q) = (lane & 15, lane >> 4) and rho(r, q) = 4 E (r / E) + E q + r % E (E = 4 for float, 2 for double: the feature, within a tile of
// 16, that load_rows leaves in register r of lane (i, q)):
//   phase 1     (W H)^T per feature tile: A operand H^T with its rows in the order "row m = 4 r + q is feature rho(r, q)", B operand W
//               (LDS) as "k = component, column = row i": register r of lane (i, q) holds WH[row i][feature rho(r, q)] -- the element
//               that xr holds of X.  Clamp and divide register against register.  The quotient register IS the A operand "row = i,
//               k = q" of num[t] += Q_r x H[16 t + i][rho(r, q)] (B operand "k = q, column = component i"), and num comes out as
//               "column = component i, row = 4 r + q": k_nmf_pass's layout of the rule.  The four waves' partial num meet in LDS, wave
//               t < KT adds them IN WAVE ORDER, applies  w * (num / den)  (no reciprocal) and leaves its tile of W_new in LDS.
//               `inner` times on the rows held in registers: transform reads X once whatever max_iter is.
//   phase 2     (AB) W_new H per feature tile, untransposed (A operand W_new from LDS, B operand H): register r holds [row 4 r + q]
//               [feature i], the one element X[row 4 r + q][feature i] per lane (the second touch of the rows, L1 / L2) is divided by
//               it, and that register is the B operand "k = q, column = feature i" of A[u][j] += W_new[4 r + q][16 u + i] x Q'_r.
//               The A accumulators stay in registers over the tiles; colsum(W_new) is kept by wave 0 (lane c < KP: column c, the 16 rows
//               in order).  inner == 0 (the loss pass, W left alone) also sums term = sum [x > eps] x log(x / WH') and sum [x > eps] x.
// Rows past n are clamped on load and their QUOTIENTS are masked to exact zeros (a zero W row alone would give 0 * inf); a wave's
// feature tiles past nt read tile nt - 1, have zero quotients in phase 1 and are never stored or summed in phase 2.  Each workgroup
// writes one slab of A (row pitch lda) and one of { colsum (KP; zeros without want_csum), term, sum x }; k_nmf_slabsum adds the slabs in
// workgroup order.  No atomics; the order of every sum is fixed by the shape alone (G = min(tiles, 256)).
// KT = 4 with FT = 8 and the H side (64 padded components, more than 256 padded columns: 256 accumulator registers beside phase 1's
// working set) does not fit in 512 registers and is NOT instantiated.  Phase 2 is separable over the features, so op_nmf_kl_pass splits
// such a pass into the update without the H side (FT = 8) and two loss-pass launches with the H side over the two halves of the
// feature axis (FT <= 4): three launches, X read from memory twice instead of once, the same sums in the same order.
template <int KT>
constexpr size_t nmf_kl_lds_bytes() { return sizeof(double) * (size_t(NMF_WAVES) * KT * 256 + 16 * nmf_wld<KT>()); }

template <class T, int KT, int FT, bool AB>
__global__ __launch_bounds__(64 * NMF_WAVES) void k_nmf_kl_pass(const T* __restrict__ X, int64_t ldx, int64_t n, int nt, const double* __restrict__ H,
                                                     int64_t ldh, const double* __restrict__ rsum, double* W, int from_const, double wconst,
                                                     int k, double l1, double l2, int inner, double* __restrict__ slabA, int64_t lda,
                                                     double* __restrict__ slabC, int want_csum) {
    constexpr int KP = 16 * KT, WLD = nmf_wld<KT>();
    constexpr int E = 16 / (int)sizeof(T), S = 16 / (4 * E);
    typedef T txe __attribute__((ext_vector_type(E)));
    extern __shared__ __attribute__((aligned(32))) double nmf_kl_lds[];
    double* zpart = nmf_kl_lds;                        // [wave][component tile][lane] f64x4 (at the end: the 256 lanes' term and sum x)
    double* wl = nmf_kl_lds + NMF_WAVES * KT * 256;    // the tile of W: 16 rows x KP, row pitch WLD
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int ft0 = wave * FT;
    const int64_t ntiles = (n + 15) / 16;
    // the feature (within a tile of 16) of row m = lane & 15 of phase 1's H^T operand: m = 4 r + q -> rho(r, q)
    const int hperm = 4 * E * ((i >> 2) / E) + E * (i & 3) + (i >> 2) % E;
    f64x4 accA[KT][FT];
    double csum = 0.0, tsum = 0.0, xsum = 0.0;
    if (AB) {
#pragma unroll
        for (int t = 0; t < KT; ++t)
#pragma unroll
            for (int j = 0; j < FT; ++j) accA[t][j] = f64x4{0.0, 0.0, 0.0, 0.0};
    }
    txe xr[FT][S];
    const auto load_rows = [&](int64_t tile) {
        const T* xp = X + min(tile * 16 + i, n - 1) * ldx + E * q;
#pragma unroll
        for (int j = 0; j < FT; ++j) {
            const bool live = ft0 + j < nt;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const txe v = *reinterpret_cast<const txe*>(xp + 16 * min(ft0 + j, nt - 1) + 4 * E * s);
#pragma unroll
                for (int e = 0; e < E; ++e) xr[j][s][e] = live ? v[e] : T(0);
            }
        }
    };
    if ((int64_t)blockIdx.x < ntiles) load_rows(blockIdx.x);
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * 16;
        // H is the same for every tile, and the compiler would keep it in registers across the loop (hundreds: they spill); the pointer
        // is made opaque once per tile so that every tile reads it again -- from L1 / L2
        const double* Ht = H;
        asm volatile("" : "+s"(Ht));
        for (int idx = tid; idx < 16 * KP; idx += 64 * NMF_WAVES) {
            const int r = idx / KP, c = idx - r * KP;
            double v = 0.0;
            if (row0 + r < n) v = from_const ? (c < k ? wconst : 0.0) : W[(row0 + r) * KP + c];
            wl[r * WLD + c] = v;
        }
        __syncthreads();
        const int t = wave;
        f64x4 wc = f64x4{0.0, 0.0, 0.0, 0.0};
        double rs = 0.0;
        if (t < KT && inner > 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) wc[r] = wl[(4 * r + q) * WLD + 16 * t + i];
            rs = rsum[16 * t + i];
        }
        const bool rowlive = row0 + i < n;
        for (int it = 0; it < inner; ++it) {
            asm volatile("" : "+s"(Ht));   // (H does not change over the updates either: read again, not kept)
            // phase 1 over this wave's features: the partial numerator of every component tile
            f64x4 num[KT];
#pragma unroll
            for (int u = 0; u < KT; ++u) num[u] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int j = 0; j < FT; ++j) {
                const double* hj = Ht + 16 * min(ft0 + j, nt - 1);
                f64x4 wh = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
                for (int c0 = 0; c0 < KP; c0 += 4)
                    wh = __builtin_amdgcn_mfma_f64_16x16x4f64(hj[(int64_t)(c0 + q) * ldh + hperm], wl[i * WLD + c0 + q], wh, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double den = wh[r] < NMF_EPS ? NMF_EPS : wh[r];
                    const double qv = rowlive ? (double)xr[j][r / E][r % E] / den : 0.0;
                    const double* hp = hj + 4 * E * (r / E) + E * q + r % E + (int64_t)i * ldh;
#pragma unroll
                    for (int u = 0; u < KT; ++u) num[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(qv, hp[(int64_t)(16 * u) * ldh], num[u], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);   // (keeps the loads of H next to their use: registers, not latency, are scarce here)
            }
#pragma unroll
            for (int u = 0; u < KT; ++u) *reinterpret_cast<f64x4*>(zpart + ((wave * KT + u) * 64 + lane) * 4) = num[u];
            __syncthreads();   // the partials are complete and every read of the old tile is done
            if (t < KT) {
                f64x4 zs = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int w = 0; w < NMF_WAVES; ++w) zs += *reinterpret_cast<const f64x4*>(zpart + ((w * KT + t) * 64 + lane) * 4);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    double den = (rs + l1) + l2 * wc[r];
                    if (den == 0.0) den = NMF_EPS;
                    wc[r] = row0 + 4 * r + q < n ? wc[r] * (zs[r] / den) : 0.0;
                    wl[(4 * r + q) * WLD + 16 * t + i] = wc[r];
                }
            }
            __syncthreads();
        }
        if (t < KT && inner > 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t row = row0 + 4 * r + q;
                if (row < n) W[row * KP + 16 * t + i] = wc[r];
            }
        }
        // the next tile's rows are requested as soon as the last update has consumed this tile's registers
        if (tile + gridDim.x < ntiles) load_rows(tile + gridDim.x);
        if (AB) {
            if (want_csum && wave == 0 && lane < KP) {
#pragma unroll
                for (int r = 0; r < 16; ++r) csum += wl[r * WLD + lane];
            }
            // phase 2: Q' = X / max(W_new H, eps) one element per lane, A += W_new^T Q'
            asm volatile("" : "+s"(Ht));
#pragma unroll
            for (int j = 0; j < FT; ++j) {
                const int ftile = min(ft0 + j, nt - 1);
                const bool live = ft0 + j < nt;
                const double* hj = Ht + 16 * ftile + i;
                f64x4 wh = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
                for (int c0 = 0; c0 < KP; c0 += 4)
                    wh = __builtin_amdgcn_mfma_f64_16x16x4f64(wl[i * WLD + c0 + q], hj[(int64_t)(c0 + q) * ldh], wh, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int64_t row = row0 + 4 * r + q;
                    const double xv = (double)X[min(row, n - 1) * ldx + 16 * ftile + i];
                    const double den = wh[r] < NMF_EPS ? NMF_EPS : wh[r];
                    const bool on = row < n && live;
                    const double qv = on ? xv / den : 0.0;
                    if (inner == 0 && on && xv > NMF_EPS) {
                        tsum += xv * log(xv / den);
                        xsum += xv;
                    }
#pragma unroll
                    for (int u = 0; u < KT; ++u)
                        accA[u][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(wl[(4 * r + q) * WLD + 16 * u + i], qv, accA[u][j], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();   // the tile of W and the partials are free again
    }
    if (AB) {
        double* sa = slabA + (int64_t)blockIdx.x * KP * lda;
#pragma unroll
        for (int u = 0; u < KT; ++u)
#pragma unroll
            for (int j = 0; j < FT; ++j)
                if (ft0 + j < nt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) sa[(int64_t)(16 * u + 4 * r + q) * lda + 16 * (ft0 + j) + i] = accA[u][j][r];
                }
        double* sc = slabC + (int64_t)blockIdx.x * (KP + 2);
        if (wave == 0 && lane < KP) sc[lane] = csum;
        // the 256 lanes' term and sum x through an LDS tree: a fixed order
        zpart[tid] = tsum;
        zpart[256 + tid] = xsum;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (tid < w) {
                zpart[tid] += zpart[tid + w];
                zpart[256 + tid] += zpart[256 + tid + w];
            }
            __syncthreads();
        }
        if (tid < 2) sc[KP + tid] = zpart[256 * tid];
    }
}

// The H rule, element by element: den = (colsum(W)[row] + l1) + l2 H, den[den == 0] = eps, H <- H o (A / den).
__global__ __launch_bounds__(256) void k_nmf_kl_hrule(double* __restrict__ H, const double* __restrict__ A, const double* __restrict__ cs,
                                                      int64_t dp, int64_t count, double l1, double l2) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= count) return;
    const double h = H[idx];
    double den = (cs[idx / dp] + l1) + l2 * h;
    if (den == 0.0) den = NMF_EPS;
    H[idx] = h * (A[idx] / den);
}

// out[row] = the sum of row `row` of H (kp x dp): one workgroup per row, thread t takes the columns t, t + 256, ..., then an LDS tree.
__global__ __launch_bounds__(256) void k_nmf_kl_rowsum(const double* __restrict__ H, int64_t dp, double* __restrict__ out) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int64_t f = t; f < dp; f += 256) s += H[(int64_t)blockIdx.x * dp + f];
    red[t] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    if (t == 0) out[blockIdx.x] = red[0];
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------------
struct NmfKlArgs {
    int g;
    int64_t ldx, n;
    const double* H;
    int64_t ldh;
    const double* rsum;
    double* W;
    int from_const;
    double wconst;
    int k;
    double l1, l2;
    int64_t lda;
};
template <class T, int KT, int FT, bool AB>
static void nmf_kl_pass_launch(Dev* d, const NmfKlArgs& a, const T* X, int nt, const double* H, int inner, double* slabA, double* slabC, int want_csum) {
    hipLaunchKernelGGL((k_nmf_kl_pass<T, KT, FT, AB>), dim3(a.g), dim3(64 * NMF_WAVES), nmf_kl_lds_bytes<KT>(), d->stream, X, a.ldx, a.n, nt, H, a.ldh,
                       a.rsum, a.W, inner > 0 ? a.from_const : 0, a.wconst, a.k, a.l1, a.l2, inner, slabA, a.lda, slabC, want_csum);
    launch_check();
}
template <class T, int KT, int FT>
static void nmf_kl_pass_ab(Dev* d, bool ab, const NmfKlArgs& a, const T* X, int nt, const double* H, int inner, double* slabA, double* slabC, int want_csum) {
    if constexpr (KT == 4 && FT == 8) {   // (no form with the H side: op_nmf_kl_pass splits it)
        nmf_kl_pass_launch<T, KT, FT, false>(d, a, X, nt, H, inner, nullptr, nullptr, 0);
    } else {
        if (ab) nmf_kl_pass_launch<T, KT, FT, true>(d, a, X, nt, H, inner, slabA, slabC, want_csum);
        else nmf_kl_pass_launch<T, KT, FT, false>(d, a, X, nt, H, inner, nullptr, nullptr, 0);
    }
}
template <class T, int KT>
static void nmf_kl_pass_ft(Dev* d, bool ab, const NmfKlArgs& a, const T* X, int nt, const double* H, int inner, double* slabA, double* slabC, int want_csum) {
    if (nt <= NMF_WAVES) nmf_kl_pass_ab<T, KT, 1>(d, ab, a, X, nt, H, inner, slabA, slabC, want_csum);
    else if (nt <= 2 * NMF_WAVES) nmf_kl_pass_ab<T, KT, 2>(d, ab, a, X, nt, H, inner, slabA, slabC, want_csum);
    else if (nt <= 4 * NMF_WAVES) nmf_kl_pass_ab<T, KT, 4>(d, ab, a, X, nt, H, inner, slabA, slabC, want_csum);
    else nmf_kl_pass_ab<T, KT, 8>(d, ab, a, X, nt, H, inner, slabA, slabC, want_csum);
}
template <class T>
static void nmf_kl_pass_kt(Dev* d, int kt, bool ab, const NmfKlArgs& a, const T* X, int nt, const double* H, int inner, double* slabA, double* slabC,
                           int want_csum) {
    if (kt == 1) nmf_kl_pass_ft<T, 1>(d, ab, a, X, nt, H, inner, slabA, slabC, want_csum);
    else if (kt == 2) nmf_kl_pass_ft<T, 2>(d, ab, a, X, nt, H, inner, slabA, slabC, want_csum);
    else nmf_kl_pass_ft<T, 4>(d, ab, a, X, nt, H, inner, slabA, slabC, want_csum);
}

bool op_nmf_kl_pass(Dev* d, int dt, const void* X, int64_t n, int64_t dp, int64_t ldx, const double* H, const double* rsum, int64_t k, int64_t kp,
                    double* W, bool from_const, double wconst, double l1, double l2, int64_t inner, double* A, double* cts) {
    const int64_t el = dt == F32 ? 4 : 2;
    // (k_nmf_pass's envelope: 16, 32 or 64 padded components -- nmf_padded_k gives 48 for k = 33 .. 48 -- and at most 512 padded columns)
    if (kp != 16 && kp != 32 && kp != 64) return false;
    if (n < 1 || n > (int64_t(1) << 40) || k < 1 || k > 64 || kp != nmf_padded_k(k) || dp < 16 || dp % 16 || dp > 512 || ldx < dp || ldx % el ||
        !aligned16(X) || !aligned16(H) || inner < 0 || inner > (int64_t(1) << 30) || !W || !aligned16(W) || !rsum || ((A == nullptr) != (cts == nullptr)) ||
        (inner == 0 && (from_const || !A)))
        return false;
    const bool ab = A != nullptr;
    const int nt = (int)(dp / 16), kt = (int)(kp / 16);
    const int g = (int)std::min<int64_t>((n + 15) / 16, NMF_MAX_WG);
    // 64 padded components and more than 256 padded columns with the H side: the update by itself, then the H side over the two halves
    // of the feature axis (k_nmf_kl_pass has no one-launch form there: registers)
    const bool split = ab && kt == 4 && nt > 4 * NMF_WAVES;
    const int halves = split ? 2 : 1;
    const int64_t count = kp + 2;
    double* slabA = ab ? (double*)dev_alloc(d, sizeof(double) * size_t(g) * (kp * dp + halves * count)) : nullptr;   // g slabs of A, then of { colsum, term, sum x }
    double* slabC = ab ? slabA + size_t(g) * kp * dp : nullptr;
    const NmfKlArgs a{g, ldx, n, H, dp, rsum, W, from_const ? 1 : 0, wconst, (int)k, l1, l2, dp};
    TagScope ts(d);
    DISPATCH_T(dt, {
        const T* Xt = (const T*)X;
        if (!split) {
            nmf_kl_pass_kt<T>(d, kt, ab, a, Xt, nt, H, (int)inner, slabA, slabC, 1);
        } else {
            const int h0 = 4 * NMF_WAVES;   // feature tiles of the first half
            if (inner > 0) nmf_kl_pass_kt<T>(d, kt, false, a, Xt, nt, H, (int)inner, nullptr, nullptr, 0);
            nmf_kl_pass_kt<T>(d, kt, true, a, Xt, h0, H, 0, slabA, slabC, 1);
            nmf_kl_pass_kt<T>(d, kt, true, a, Xt + 16 * h0, nt - h0, H + 16 * h0, 0, slabA + 16 * h0, slabC + size_t(g) * count, 0);
        }
    });
    ts.stop();
    if (ab) {
        hipLaunchKernelGGL(k_nmf_slabsum, dim3((unsigned)cdiv64(kp * dp, 256)), dim3(256), 0, d->stream, (const double*)slabA, g, kp * dp, A);
        launch_check();
        hipLaunchKernelGGL(k_nmf_slabsum, dim3(1), dim3(256), 0, d->stream, (const double*)slabC, halves * g, count, cts);
        launch_check();
        dev_free(d, slabA);
    }
    return true;
}

bool op_nmf_kl_hrule(Dev* d, int64_t kp, int64_t dp, const double* A, const double* colsum, double* H, double l1, double l2) {
    if (kp < 1 || dp < 1 || !A || !colsum || !H) return false;
    hipLaunchKernelGGL(k_nmf_kl_hrule, dim3((unsigned)cdiv64(kp * dp, 256)), dim3(256), 0, d->stream, H, A, colsum, dp, kp * dp, l1, l2);
    launch_check();
    return true;
}

bool op_nmf_kl_rowsum(Dev* d, int64_t kp, int64_t dp, const double* H, double* out) {
    if (kp < 1 || dp < 1 || !H || !out) return false;
    hipLaunchKernelGGL(k_nmf_kl_rowsum, dim3((unsigned)kp), dim3(256), 0, d->stream, H, dp, out);
    launch_check();
    return true;
}

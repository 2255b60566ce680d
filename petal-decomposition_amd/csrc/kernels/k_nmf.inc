// k_nmf.inc -- part of the ONE translation unit hip_ops.hip (textually included there, inside namespace petal): non-negative matrix
// factorisation by multiplicative updates (include/petal_hip_nmf.h).  One iteration is ONE fused pass over X (k_nmf_pass)
//     Z = X H^T,  D = W (H H^T) + l1 + l2 W,  D[D == 0] = eps,  W <- W o Z / D,  A = W^T X,  B = W^T W      (the NEW W in A and B)
// and k x d work on H (k_nmf_hrule, k_nmf_dots around two op_dgemm).  k_nmf_scan is the one look at X in front of a fit or a transform.
// Device layouts: W n x KP, H and A KP x dp (ld dp), H H^T and B KP x KP, all fp64, KP = 16, 32 or 64 >= k, ZERO in the padding (a
// padded component stays zero under the rule: 0 * 0 / D).
// ------------------------------------------------------------------------------------------------
// The fused pass.  v_mfma_f64_16x16x4_f64 takes A as "row = lane & 15, k = lane >> 4", B as "k = lane >> 4, column = lane & 15" and
// delivers C as "column = lane & 15, row = (lane >> 4) + 4 reg" (k_row_gram.inc).  With (i, q) = (lane & 15, lane >> 4):
//   product 1   X rows are the A operand, H rows the B operand: register r holds Z[row 4 r + q][component i];
//   D           W rows (from LDS) are the A operand, H H^T the B operand: the same layout, so the rule is register against register;
//   A, B        W_new in that layout IS the A operand "row = component i, k = row 4 r + q" and the B operand "k = q, column =
//               component i": W_new^T X takes one element X[row 4 r + q][feature i] per lane as its other operand -- the second touch
//               of the 16 rows just read, from L1 / L2 -- and W_new^T W_new takes W_new (from LDS) twice.
// A workgroup is four waves (one per SIMD: 512 registers each) on a tile of 16 rows; workgroups are persistent over the tiles g,
// g + G, ...  The FEATURE axis is split over the waves, FT tiles of 16 features each: a wave forms its partial Z over its own features
// (16-byte loads along the row, E MFMAs per load), the partials meet in LDS (4 x 16 x KP doubles), wave t < KT adds them IN WAVE ORDER
// for component tile t, forms its tile of D, applies the rule and leaves its tile of W_new in LDS; every wave then accumulates its own
// feature slice of A (KT x FT accumulator tiles: 256 registers at k = 64, d = 512) and its share of the KT x KT tiles of B, whose
// accumulators live in LDS between the tiles (the registers are taken: 32 KiB at k = 64, read and written once per tile by their wave).
// inner > 1 (transform) repeats the rule on the same Z with D from the current W; inner == 0 leaves W alone (A = W^T X: the loss at the
// start).  Each workgroup writes one slab of A and one of B; k_nmf_slabsum adds the slabs in workgroup order.  No atomics; the order of every sum is
// fixed by the shape alone (G = min(tiles, 256), whatever the device).  The next tile's rows are requested as soon as product 1 has
// consumed this tile's registers.  Rows past n are clamped on load and masked to zero in W_new; X has nt = dp / 16 feature tiles whose
// padding columns hold zeros.
constexpr int NMF_WAVES = 4;
constexpr int NMF_MAX_WG = 256;
constexpr double NMF_EPS = 1.1920928955078125e-07;   // 2^-23 for both data types

template <int KT>
constexpr int nmf_wld() { return 16 * KT + 2; }
template <int KT, bool AB>
constexpr size_t nmf_lds_bytes() { return sizeof(double) * (size_t(NMF_WAVES) * KT * 256 + 16 * nmf_wld<KT>() + (AB ? 256 * KT * KT : 0)); }

template <class T, int KT, int FT, bool AB>
__global__ __launch_bounds__(64 * NMF_WAVES) void k_nmf_pass(const T* __restrict__ X, int64_t ldx, int64_t n, int nt, const double* __restrict__ H,
                                                  int64_t ldh, const double* __restrict__ HHt, double* W, int from_const, double wconst, int k,
                                                  double l1, double l2, int inner, double* __restrict__ slabA, double* __restrict__ slabB) {
    constexpr int KP = 16 * KT, WLD = nmf_wld<KT>();
    constexpr int E = 16 / (int)sizeof(T), S = 16 / (4 * E);
    typedef T txe __attribute__((ext_vector_type(E)));
    typedef double f64x2 __attribute__((ext_vector_type(2)));
    extern __shared__ __attribute__((aligned(32))) double nmf_lds[];
    double* zpart = nmf_lds;                           // [wave][component tile][lane] f64x4
    double* wl = nmf_lds + NMF_WAVES * KT * 256;       // the tile of W: 16 rows x KP, row pitch WLD
    double* bl = wl + 16 * WLD;                        // AB: the KT x KT accumulator tiles of B in fragment order, [tile][lane] f64x4
    constexpr int BT = (KT * KT + NMF_WAVES - 1) / NMF_WAVES;   // tiles of B per wave (tile p belongs to wave p mod 4: no wave touches another's)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int ft0 = wave * FT;
    const int64_t ntiles = (n + 15) / 16;
    f64x4 accA[KT][FT];
    if (AB) {
#pragma unroll
        for (int t = 0; t < KT; ++t)
#pragma unroll
            for (int j = 0; j < FT; ++j) accA[t][j] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int u = 0; u < BT; ++u)
            if (wave + NMF_WAVES * u < KT * KT) *reinterpret_cast<f64x4*>(bl + ((wave + NMF_WAVES * u) * 64 + lane) * 4) = f64x4{0.0, 0.0, 0.0, 0.0};
    }
    txe xr[FT][S];
    // (a wave's feature tiles past nt are loaded from tile nt - 1 and zeroed: the loop below has no branches)
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
        // H and H H^T are the same for every tile, and the compiler would keep them in registers across the loop (hundreds: they spill);
        // the pointers are made opaque once per tile so that every tile reads them again -- from L1 / L2
        const double *Ht = H, *HHtt = HHt;
        asm volatile("" : "+s"(Ht), "+s"(HHtt));
        // the tile of W into LDS (from_const: transform's constant start instead of W's contents)
        for (int idx = tid; idx < 16 * KP; idx += 64 * NMF_WAVES) {
            const int r = idx / KP, c = idx - r * KP;
            double v = 0.0;
            if (row0 + r < n) v = from_const ? (c < k ? wconst : 0.0) : W[(row0 + r) * KP + c];
            wl[r * WLD + c] = v;
        }
        // product 1 over this wave's features
        f64x4 z[KT];
#pragma unroll
        for (int t = 0; t < KT; ++t) z[t] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < FT; ++j) {
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const double* hq = Ht + 16 * min(ft0 + j, nt - 1) + 4 * E * s + E * q + (int64_t)i * ldh;
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
                    for (int e = 0; e < E; ++e) z[t] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)xr[j][s][e], hv[e], z[t], 0, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);   // (keeps the loads of H next to their use: registers, not latency, are scarce here)
        }
#pragma unroll
        for (int t = 0; t < KT; ++t) *reinterpret_cast<f64x4*>(zpart + ((wave * KT + t) * 64 + lane) * 4) = z[t];
        if (tile + gridDim.x < ntiles) load_rows(tile + gridDim.x);
        __syncthreads();
        // the rule, on wave t < KT for component tile t
        const int t = wave;
        f64x4 zs = f64x4{0.0, 0.0, 0.0, 0.0}, wc = zs;
        if (t < KT && inner > 0) {
#pragma unroll
            for (int w = 0; w < NMF_WAVES; ++w) zs += *reinterpret_cast<const f64x4*>(zpart + ((w * KT + t) * 64 + lane) * 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) wc[r] = wl[(4 * r + q) * WLD + 16 * t + i];
        }
        for (int it = 0; it < inner; ++it) {
            if (t < KT) {
                f64x4 dd = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
                for (int c0 = 0; c0 < KP; c0 += 4)
                    dd = __builtin_amdgcn_mfma_f64_16x16x4f64(wl[i * WLD + c0 + q], HHtt[(c0 + q) * KP + 16 * t + i], dd, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    double den = (dd[r] + l1) + l2 * wc[r];
                    if (den == 0.0) den = NMF_EPS;
                    wc[r] = row0 + 4 * r + q < n ? wc[r] * (zs[r] / den) : 0.0;
                }
            }
            __syncthreads();   // every read of the old tile is done
            if (t < KT) {
#pragma unroll
                for (int r = 0; r < 4; ++r) wl[(4 * r + q) * WLD + 16 * t + i] = wc[r];
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
        if (AB) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double wv[KT];
#pragma unroll
                for (int u = 0; u < KT; ++u) wv[u] = wl[(4 * r + q) * WLD + 16 * u + i];
                const T* xp = X + min(row0 + 4 * r + q, n - 1) * ldx + i;
#pragma unroll
                for (int j = 0; j < FT; ++j) {
                    const double xb = (double)xp[16 * min(ft0 + j, nt - 1)];
#pragma unroll
                    for (int u = 0; u < KT; ++u) accA[u][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(wv[u], xb, accA[u][j], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            // B += W_new^T W_new: the accumulators live in LDS (the registers hold A), each wave on its own tiles
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
    if (AB) {
        const int64_t dp = 16 * (int64_t)nt;
        double* sa = slabA + (int64_t)blockIdx.x * KP * dp;
#pragma unroll
        for (int u = 0; u < KT; ++u)
#pragma unroll
            for (int j = 0; j < FT; ++j)
                if (ft0 + j < nt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) sa[(int64_t)(16 * u + 4 * r + q) * dp + 16 * (ft0 + j) + i] = accA[u][j][r];
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

// out[idx] = sum_g slab[g][idx], g in order: the fixed-order sum of the workgroups' slabs.
__global__ __launch_bounds__(256) void k_nmf_slabsum(const double* __restrict__ slab, int g, int64_t count, double* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= count) return;
    double s = 0.0;
    for (int b = 0; b < g; ++b) s += slab[b * count + idx];
    out[idx] = s;
}

// The one look at X in front of a fit or a transform: part[b] = { sum x, sum x^2, min x, non-finite seen } over the rows b, b + G, ...
// (fp64; thread t takes the 16-byte pieces t, t + 256, ... of a row, the 256 partial results go through an LDS tree), then one
// workgroup adds the G parts in a fixed order.  The padding columns (zeros) take part: the minimum only ever answers "is one negative".
template <class T>
__global__ __launch_bounds__(256) void k_nmf_scan(const T* __restrict__ X, int64_t ldx, int64_t n, int64_t dp, double* __restrict__ part) {
    constexpr int E = 16 / (int)sizeof(T);
    typedef T txe __attribute__((ext_vector_type(E)));
    __shared__ double red[4][256];
    const int t = threadIdx.x;
    double s = 0.0, s2 = 0.0, mn = 0.0, bad = 0.0;
    for (int64_t r = blockIdx.x; r < n; r += gridDim.x)
        for (int64_t f = (int64_t)E * t; f < dp; f += 256 * E) {
            const txe x = *reinterpret_cast<const txe*>(X + r * ldx + f);
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const double v = (double)x[e];
                s += v;
                s2 += v * v;
                mn = fmin(mn, v);
                if (!(v - v == 0.0)) bad = 1.0;
            }
        }
    red[0][t] = s; red[1][t] = s2; red[2][t] = mn; red[3][t] = bad;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) {
            red[0][t] += red[0][t + w];
            red[1][t] += red[1][t + w];
            red[2][t] = fmin(red[2][t], red[2][t + w]);
            red[3][t] = fmax(red[3][t], red[3][t + w]);
        }
        __syncthreads();
    }
    if (t < 4) part[blockIdx.x * 4 + t] = red[t][0];
}
__global__ __launch_bounds__(256) void k_nmf_scan_sum(const double* __restrict__ part, int g, double* __restrict__ out4) {
    __shared__ double red[4][256];
    const int t = threadIdx.x;
    double s = 0.0, s2 = 0.0, mn = 0.0, bad = 0.0;
    for (int b = t; b < g; b += 256) {
        s += part[4 * b];
        s2 += part[4 * b + 1];
        mn = fmin(mn, part[4 * b + 2]);
        bad = fmax(bad, part[4 * b + 3]);
    }
    red[0][t] = s; red[1][t] = s2; red[2][t] = mn; red[3][t] = bad;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) {
            red[0][t] += red[0][t + w];
            red[1][t] += red[1][t + w];
            red[2][t] = fmin(red[2][t], red[2][t + w]);
            red[3][t] = fmax(red[3][t], red[3][t + w]);
        }
        __syncthreads();
    }
    if (t < 4) out4[t] = red[t][0];
}

// The H rule, element by element: E = (B H) + l1 + l2 H, E[E == 0] = eps, H <- H o A / E  (Eh = B H on entry).
__global__ __launch_bounds__(256) void k_nmf_hrule(double* __restrict__ H, const double* __restrict__ A, const double* __restrict__ Eh,
                                                   int64_t count, double l1, double l2) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= count) return;
    const double h = H[idx];
    double den = (Eh[idx] + l1) + l2 * h;
    if (den == 0.0) den = NMF_EPS;
    H[idx] = h * (A[idx] / den);
}

// The two inner products of the loss: out2 = { <A, H>, <B, H H^T> }, one workgroup, a fixed order.
__global__ __launch_bounds__(256) void k_nmf_dots(const double* __restrict__ A, const double* __restrict__ H, int64_t na,
                                                  const double* __restrict__ B, const double* __restrict__ HHt, int64_t nb,
                                                  double* __restrict__ out2) {
    __shared__ double red[2][256];
    const int t = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (int64_t idx = t; idx < na; idx += 256) a += A[idx] * H[idx];
    for (int64_t idx = t; idx < nb; idx += 256) b += B[idx] * HHt[idx];
    red[0][t] = a; red[1][t] = b;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) {
            red[0][t] += red[0][t + w];
            red[1][t] += red[1][t + w];
        }
        __syncthreads();
    }
    if (t < 2) out2[t] = red[t][0];
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------------
bool op_nmf_scan(Dev* d, int dt, const void* X, int64_t n, int64_t dp, int64_t ldx, double* out4) {
    const int64_t el = dt == F32 ? 4 : 2;
    if (n < 1 || dp < 16 || dp % 16 || ldx < dp || ldx % el || !aligned16(X)) return false;
    const int g = (int)std::min<int64_t>(n, 1024);
    double* part = (double*)dev_alloc(d, sizeof(double) * 4 * size_t(g));
    DISPATCH_T(dt, hipLaunchKernelGGL((k_nmf_scan<T>), dim3(g), dim3(256), 0, d->stream, (const T*)X, ldx, n, dp, part));
    launch_check();
    hipLaunchKernelGGL(k_nmf_scan_sum, dim3(1), dim3(256), 0, d->stream, (const double*)part, g, out4);
    launch_check();
    dev_free(d, part);
    return true;
}

template <class T, int KT, int FT, bool AB>
static void nmf_pass_launch(Dev* d, int g, const T* X, int64_t ldx, int64_t n, int nt, const double* H, int64_t ldh, const double* HHt, double* W,
                            int from_const, double wconst, int k, double l1, double l2, int inner, double* slabA, double* slabB) {
    const void* fn = reinterpret_cast<const void*>(k_nmf_pass<T, KT, FT, AB>);
    constexpr size_t lds = nmf_lds_bytes<KT, AB>();
    if (lds > 64 * 1024) set_max_lds(d, fn);
    hipLaunchKernelGGL((k_nmf_pass<T, KT, FT, AB>), dim3(g), dim3(64 * NMF_WAVES), lds, d->stream, X, ldx, n, nt, H, ldh, HHt, W,
                       from_const, wconst, k, l1, l2, inner, slabA, slabB);
}
template <class T, int KT, int FT>
static void nmf_pass_ab(Dev* d, bool ab, int g, const T* X, int64_t ldx, int64_t n, int nt, const double* H, int64_t ldh, const double* HHt,
                        double* W, int from_const, double wconst, int k, double l1, double l2, int inner, double* slabA, double* slabB) {
    if (ab) nmf_pass_launch<T, KT, FT, true>(d, g, X, ldx, n, nt, H, ldh, HHt, W, from_const, wconst, k, l1, l2, inner, slabA, slabB);
    else nmf_pass_launch<T, KT, FT, false>(d, g, X, ldx, n, nt, H, ldh, HHt, W, from_const, wconst, k, l1, l2, inner, slabA, slabB);
}
template <class T, int KT>
static void nmf_pass_ft(Dev* d, bool ab, int g, const T* X, int64_t ldx, int64_t n, int nt, const double* H, int64_t ldh, const double* HHt,
                        double* W, int from_const, double wconst, int k, double l1, double l2, int inner, double* slabA, double* slabB) {
    if (nt <= NMF_WAVES) nmf_pass_ab<T, KT, 1>(d, ab, g, X, ldx, n, nt, H, ldh, HHt, W, from_const, wconst, k, l1, l2, inner, slabA, slabB);
    else if (nt <= 2 * NMF_WAVES) nmf_pass_ab<T, KT, 2>(d, ab, g, X, ldx, n, nt, H, ldh, HHt, W, from_const, wconst, k, l1, l2, inner, slabA, slabB);
    else if (nt <= 4 * NMF_WAVES) nmf_pass_ab<T, KT, 4>(d, ab, g, X, ldx, n, nt, H, ldh, HHt, W, from_const, wconst, k, l1, l2, inner, slabA, slabB);
    else nmf_pass_ab<T, KT, 8>(d, ab, g, X, ldx, n, nt, H, ldh, HHt, W, from_const, wconst, k, l1, l2, inner, slabA, slabB);
}

bool op_nmf_pass(Dev* d, int dt, const void* X, int64_t n, int64_t dp, int64_t ldx, const double* H, const double* HHt, int64_t k, int64_t kp,
                 double* W, bool from_const, double wconst, double l1, double l2, int64_t inner, double* A, double* B) {
    const int64_t el = dt == F32 ? 4 : 2;
    // (the kernel exists for 16, 32 and 64 padded components only: nmf_padded_k gives 48 for k = 33 .. 48, which the KT = 4 form would
    //  walk with a row pitch of 64 -- past the end of W, H and H H^T; those fits take the composed path)
    if (kp != 16 && kp != 32 && kp != 64) return false;
    if (n < 1 || n > (int64_t(1) << 40) || k < 1 || k > 64 || kp != nmf_padded_k(k) || dp < 16 || dp % 16 || dp > 512 || ldx < dp || ldx % el ||
        !aligned16(X) || !aligned16(H) || inner < 0 || inner > (int64_t(1) << 30) || !W || !aligned16(W) || !HHt || ((A == nullptr) != (B == nullptr)))
        return false;
    const bool ab = A != nullptr;
    const int nt = (int)(dp / 16), kt = (int)(kp / 16);
    const int g = (int)std::min<int64_t>((n + 15) / 16, NMF_MAX_WG);
    double* slabA = ab ? (double*)dev_alloc(d, sizeof(double) * size_t(g) * kp * (dp + kp)) : nullptr;   // g slabs of A, then g slabs of B
    double* slabB = ab ? slabA + size_t(g) * kp * dp : nullptr;
    TagScope ts(d);
#define PETAL_NMF_PASS(KTv) DISPATCH_T(dt, (nmf_pass_ft<T, KTv>(d, ab, g, (const T*)X, ldx, n, nt, H, dp, HHt, W, from_const ? 1 : 0, wconst, (int)k, l1, l2, (int)inner, slabA, slabB)))
    if (kt == 1) PETAL_NMF_PASS(1);
    else if (kt == 2) PETAL_NMF_PASS(2);
    else PETAL_NMF_PASS(4);
#undef PETAL_NMF_PASS
    launch_check();
    ts.stop();
    if (ab) {
        hipLaunchKernelGGL(k_nmf_slabsum, dim3((unsigned)cdiv64(kp * dp, 256)), dim3(256), 0, d->stream, (const double*)slabA, g, kp * dp, A);
        launch_check();
        hipLaunchKernelGGL(k_nmf_slabsum, dim3((unsigned)cdiv64(kp * kp, 256)), dim3(256), 0, d->stream, (const double*)slabB, g, kp * kp, B);
        launch_check();
        dev_free(d, slabA);
    }
    return true;
}

bool op_nmf_hupdate(Dev* d, int64_t kp, int64_t dp, const double* A, const double* B, double* H, double* HHt, double l1, double l2, double* dots2) {
    if (kp < 1 || dp < 1) return false;
    double* eh = (double*)dev_alloc(d, sizeof(double) * size_t(kp) * dp);
    op_dgemm(d, false, false, kp, dp, kp, 1.0, B, kp, H, dp, 0.0, eh, dp);
    hipLaunchKernelGGL(k_nmf_hrule, dim3((unsigned)cdiv64(kp * dp, 256)), dim3(256), 0, d->stream, H, A, (const double*)eh, kp * dp, l1, l2);
    launch_check();
    dev_free(d, eh);
    op_dgemm(d, false, true, kp, kp, dp, 1.0, H, dp, H, dp, 0.0, HHt, kp);
    hipLaunchKernelGGL(k_nmf_dots, dim3(1), dim3(256), 0, d->stream, A, (const double*)H, kp * dp, B, (const double*)HHt, kp * kp, dots2);
    launch_check();
    return true;
}

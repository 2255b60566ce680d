// k_ica_step.inc -- part of the ONE translation unit hip_ops.hip (textually included there, inside namespace petal): K7: the fused FastICA step (k_ica_mfma, k_ica3, k_ica3p, k_ica_reduce; k_ica_mfma_g, k_ica3g, k_ica3pg: the same bodies, k_ica*_body.inc, with the exp / cube contrast).
// ================================================================================================
// K7: fused FastICA step (ica.rs:332-333) -- per 16-sample tile: S = X1 . W^T (MFMA) -> tanh ->
// D += G^T . X1 (MFMA) and gp += sum(1 - g^2); partial D / gp per wave, combined in fp64.
// ================================================================================================
__device__ __forceinline__ float tanh_fast(float x) {
    // tanh(x) = 1 - 2 / (exp(2x) + 1); saturates correctly at +-inf; |abs err| ~ 1e-7; tanh(0) = 0 exactly.
    // v_exp_f32 + v_rcp_f32 (1 ulp each): five VALU instructions instead of the ~14 of an IEEE division
    const float e = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);
    return fmaf(-2.0f, __builtin_amdgcn_rcpf(e + 1.0f), 1.0f);
}
// The contrast functions of the fixed-point iteration beyond the crate's logcosh (DESIGN.md section 7): g and g' of
//   ICA_G_LOGCOSH  tanh u,  1 - g^2       ICA_G_EXP  u exp(-u^2/2),  (1 - u^2) exp(-u^2/2)       ICA_G_CUBE  u^3,  3 u^2
// exp: e = exp2(-u^2 log2(e)/2) is ONE v_exp_f32 and no reciprocal (underflows to 0 for |u| > 14.4: g = g' = 0, the limit);
// g' = e - u g.  g(0) = 0 for all three, so zero rows add nothing to D; g'(0) is 1, 1, 0: see ica_gp_pad.
enum { ICA_G_LOGCOSH = 0, ICA_G_EXP = 1, ICA_G_CUBE = 2 };
template <int G>
__device__ __forceinline__ void ica_contrast(float u, float& g, float& gp) {
    static_assert(G == ICA_G_LOGCOSH || G == ICA_G_EXP || G == ICA_G_CUBE, "unknown contrast");
    if constexpr (G == ICA_G_LOGCOSH) {
        g = tanh_fast(u);
        gp = fmaf(-g, g, 1.0f);
    } else if constexpr (G == ICA_G_EXP) {
        const float e = __builtin_amdgcn_exp2f(u * u * -0.72134752044448170f);
        g = u * e;
        gp = fmaf(-u, g, e);
    } else {
        const float u2 = u * u;
        g = u2 * u;
        gp = 3.0f * u2;
    }
}
template <int G>
__device__ __forceinline__ void ica_contrast(double u, double& g, double& gp) {
    if constexpr (G == ICA_G_LOGCOSH) {
        g = tanh(u);
        gp = 1.0 - g * g;
    } else if constexpr (G == ICA_G_EXP) {
        const double e = exp(-0.5 * u * u);
        g = u * e;
        gp = e - u * g;
    } else {
        g = u * u * u;
        gp = 3.0 * u * u;
    }
}
// what the `pad` zero rows of a ragged last block (S = 0 there) put into an UNMASKED sum of g': g'(0) each
template <int G>
__device__ __forceinline__ float ica_gp_pad(float pad) { return G == ICA_G_CUBE ? 0.f : pad; }
// Wpk[((kc * NT + nt) * 64 + lane) * 4 + s] = W[16 nt + (lane&15)][16 kc + 4 (lane>>4) + s]   (B = W^T)
__global__ void k_pack_w(const double* __restrict__ W, int nc, float* __restrict__ Wpk, int NT) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= NT * NT * 64) return;
    const int lane = e & 63, cn = e >> 6, nt = cn % NT, kc = cn / NT, q = lane >> 4, j = lane & 15;
    f32x4 v;
    for (int s = 0; s < 4; ++s) {
        const int comp = 16 * nt + j, k = 16 * kc + 4 * q + s;
        v[s] = (comp < nc && k < nc) ? (float)W[comp * nc + k] : 0.f;
    }
    reinterpret_cast<f32x4*>(Wpk)[e] = v;
}

// one partial slab per WORKGROUP, deterministic: waves 0 and 1 store their tiles into two LDS slabs, waves 2 and 3 add
// theirs on top, and the sum (w0 + w2) + (w1 + w3) of the two slabs [NCP*NCP D | NCP gp] is written once, coalesced.
// s_slab holds 2 (NCP*NCP + NCP) floats.
template <int NT>
__device__ __forceinline__ void ica_write_slab(const f32x4 (&dacc)[NT][NT], const float (&gpa)[NT], float* s_slab,
                                               float* __restrict__ part) {
    constexpr int NCP = 16 * NT, SLAB = NCP * NCP + NCP;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, q = lane >> 4;
    float* mine = s_slab + (wave & 1) * SLAB;
    for (int ph = 0; ph < 2; ++ph) {
        if ((wave >> 1) == ph) {
#pragma unroll
            for (int a = 0; a < NT; ++a)
#pragma unroll
                for (int b = 0; b < NT; ++b)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float* dst = &mine[(16 * a + 4 * q + r) * NCP + 16 * b + i];
                        *dst = (ph == 0 ? 0.f : *dst) + dacc[a][b][r];
                    }
#pragma unroll
            for (int a = 0; a < NT; ++a) {
                float gsum = gpa[a];
                gsum += __shfl_xor(gsum, 16, 64);
                gsum += __shfl_xor(gsum, 32, 64);
                if (q == 0) {
                    float* dst = &mine[NCP * NCP + 16 * a + i];
                    *dst = (ph == 0 ? 0.f : *dst) + gsum;
                }
            }
        }
        __syncthreads();
    }
    float* out = part + (int64_t)blockIdx.x * SLAB;
    for (int e = threadIdx.x; e < SLAB; e += 256) out[e] = s_slab[e] + s_slab[SLAB + e];
}
template <int NT>
__global__ __launch_bounds__(256) void k_ica_mfma(const float* __restrict__ X1T, int64_t n, int64_t ld,
                                                  const float* __restrict__ Wpk, int64_t tiles_per_wave,
                                                  float* __restrict__ part, const int* __restrict__ state) {
    constexpr int G = ICA_G_LOGCOSH;
#include "k_ica_mfma_body.inc"
}
template <int NT, int G>
__global__ __launch_bounds__(256) void k_ica_mfma_g(const float* __restrict__ X1T, int64_t n, int64_t ld,
                                                    const float* __restrict__ Wpk, int64_t tiles_per_wave,
                                                    float* __restrict__ part, const int* __restrict__ state) {
#include "k_ica_mfma_body.inc"
}
// K7, split-product form: both products of the step on the bf16 matrix cores (six piece products each, see K1).  One
// wave handles 32 samples per pass.  The first product is laid out so that its OUTPUT is already the second product's
// A operand: C[row = sample][col = component] puts S[samples 4q+r of either 16-sample tile][component i] in lane (i, q),
// and since the k-slot <-> sample assignment of an MFMA is free as long as A and B agree, slot e of lane group q is
// declared to be sample (e < 4 ? 4q+e : 16+4q+e-4); X1 is then loaded in exactly that order for the B operand.  No
// cross-lane traffic between the two products.  W's three planes live in LDS (shared by the four waves).
// Wpk3[((kc NT + u) 3 + plane) 64 + lane][e] = plane of (float)W[16 u + (lane & 15)][32 kc + 8 (lane >> 4) + e]
__global__ __launch_bounds__(256) void k_pack_w3(const double* __restrict__ W, int nc, bf16x8* __restrict__ out, int NT,
                                                 int KCH) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= KCH * NT * 64) return;
    const int lane = idx & 63, tile = idx >> 6, u = tile % NT, kc = tile / NT;
    const int comp = 16 * u + (lane & 15), k0 = 32 * kc + 8 * (lane >> 4);
    f32x8 x;
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = (comp < nc && k0 + e < nc) ? (float)W[comp * nc + k0 + e] : 0.f;
    bf16x8 h, m, l;
    split3(x, h, m, l);
    out[(tile * 3 + 0) * 64 + lane] = h;
    out[(tile * 3 + 1) * 64 + lane] = m;
    out[(tile * 3 + 2) * 64 + lane] = l;
}

template <int NT>
__global__ __launch_bounds__(256, 2) void k_ica3(const float* __restrict__ X1T, int64_t n, int64_t ld,
                                                 const bf16x8* __restrict__ Wpk3, int64_t blocks_per_wave,
                                                 float* __restrict__ part, const int* __restrict__ state) {
    constexpr int G = ICA_G_LOGCOSH;
#include "k_ica3_body.inc"
}
template <int NT, int G>
__global__ __launch_bounds__(256, 2) void k_ica3g(const float* __restrict__ X1T, int64_t n, int64_t ld,
                                                  const bf16x8* __restrict__ Wpk3, int64_t blocks_per_wave,
                                                  float* __restrict__ part, const int* __restrict__ state) {
#include "k_ica3_body.inc"
}
// K7 on PRE-SPLIT whitened data (round 5).  X1 is constant over the 10 .. 200 iterations of a fit, and k_ica3 split it into bf16
// planes twice per iteration (row fragments for the first product, transposed fragments for the second): a third or more of the
// VALU instructions of a kernel that is paced by them (9.3 per MFMA, 16 % matrix-pipe busy: profiles/r04_pmc_fastica_*).  Here the
// planes are made ONCE per fit (k_ica_planes), in fragment order:
//     X1pl[(((b 2 + t) KCH + kc) 3 + plane) 64 + lane][e] = plane of X1[32 b + 16 t + (lane & 15)][32 kc + 8 (lane >> 4) + e]
// -- a wave's load of one fragment is 1 KB contiguous -- and the step kernel loads them as they are: they ARE the first product's A
// operand, and, parked in a wave-private row-major image (16-B chunks XOR-swizzled by the row, as k_pow3's), come back TRANSPOSED
// through ds_read_b64_tr_b16 as the second product's B operand (k-slots declared to be the samples {4 q + r, 16 + 4 q + r}, which is
// the first product's output layout: see k_ica3).  Only G = tanh(S) is split inside the loop.
template <int KCH>
__global__ __launch_bounds__(256) void k_ica_planes(const float* __restrict__ X1T, int64_t n, int64_t ld, int NCP, bf16x8* __restrict__ out,
                                                    int64_t nfrag) {
    const int64_t frag = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);   // (b, t, kc)
    if (frag >= nfrag) return;
    const int lane = threadIdx.x & 63, i = lane & 15, q = lane >> 4;
    const int kc = (int)(frag % KCH);
    const int64_t bt = frag / KCH, row = 16 * bt + i;
    f32x8 x = f32x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (row < n && 32 * kc + 8 * q < NCP) {
        const float* src = X1T + row * ld + 32 * kc + 8 * q;
        const f32x4 lo = *reinterpret_cast<const f32x4*>(src), hi = *reinterpret_cast<const f32x4*>(src + 4);
        x = f32x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    }
    bf16x8 h, m, l;
    split3(x, h, m, l);
    bf16x8* o = out + (frag * 3) * 64 + lane;
    o[0] = h; o[64] = m; o[128] = l;
}
// byte offset of 16-B chunk `ch` of row `row` in one plane of a wave's image: 128-B rows (64 components) as k_pow3's; 64-B rows (32
// components): rows r and r + 4 share a 256-B bank row, so the upper four of each eight take the other half of it
template <int NT>
__device__ __forceinline__ int ica_xoff(int row, int ch) {
    return NT == 4 ? pow3_xoff(row, ch) : row * 64 + 16 * (ch ^ (2 * ((row >> 2) & 1)));
}
template <int NT>
__global__ __launch_bounds__(256, 2) void k_ica3p(const bf16x8* __restrict__ X1pl, int64_t n, const bf16x8* __restrict__ Wpk3,
                                                  int64_t blocks_per_wave, float* __restrict__ part, const int* __restrict__ state) {
    constexpr int G = ICA_G_LOGCOSH;
#include "k_ica3p_body.inc"
}
template <int NT, int G>
__global__ __launch_bounds__(256, 2) void k_ica3pg(const bf16x8* __restrict__ X1pl, int64_t n, const bf16x8* __restrict__ Wpk3,
                                                   int64_t blocks_per_wave, float* __restrict__ part, const int* __restrict__ state) {
#include "k_ica3p_body.inc"
}
// combine the per-workgroup slabs in fp64 (fixed order) and drop the padding: GX_gp = [nc*nc | nc].
// block = 32 outputs x 32 part-lanes (the reduction is latency-bound: many short independent load chains).
__global__ __launch_bounds__(1024) void k_ica_reduce(const float* __restrict__ part, int64_t nparts, int NCP, int nc,
                                                     double* __restrict__ out, const int* __restrict__ state) {
    if (state && state[0]) return;
    __shared__ double red[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int e = blockIdx.x * 32 + tx;
    const int64_t slab = (int64_t)NCP * NCP + NCP;
    double sacc = 0;
    if (e < nc * nc + nc) {
        const int src = e < nc * nc ? (e / nc) * NCP + (e % nc) : NCP * NCP + (e - nc * nc);
        for (int64_t p = ty; p < nparts; p += 32) sacc += (double)part[p * slab + src];
    }
    red[ty][tx] = sacc;
    __syncthreads();
    if (ty == 0 && e < nc * nc + nc) {
        double t = 0;
#pragma unroll
        for (int k = 0; k < 32; ++k) t += red[k][tx];  // fixed order: deterministic
        out[e] = t;
    }
}

// generic FastICA step: one block per chunk of 64 samples, fp64
// (the other contrasts keep g' beside g in shared memory: [nc][64] each)
template <class T, int G>
__device__ __forceinline__ void ica_simple_body(const T* __restrict__ X1T, int64_t n, int nc, int64_t ld, const double* __restrict__ W,
                                                double* __restrict__ part, const int* __restrict__ state) {
    if (state && state[0]) return;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double* g = reinterpret_cast<double*>(smem_raw);  // [nc][64]
    double* gd = g + (G == ICA_G_LOGCOSH ? 0 : nc * 64);
    const int64_t s0 = (int64_t)blockIdx.x * 64;
    const int ns = (int)min((int64_t)64, n - s0);
    for (int e = threadIdx.x; e < nc * 64; e += blockDim.x) {
        const int c = e / 64, s = e % 64;
        double v = 0, vd = 0;
        if (s < ns) {
            double wx = 0;
            for (int j = 0; j < nc; ++j) wx += (sizeof(T) == 4 ? (double)(float)W[c * nc + j] : W[c * nc + j]) * (double)X1T[(s0 + s) * ld + j];
            if constexpr (G == ICA_G_LOGCOSH) v = tanh(wx);
            else ica_contrast<G>(wx, v, vd);
        }
        g[e] = v;
        if constexpr (G != ICA_G_LOGCOSH) gd[e] = vd;
    }
    __syncthreads();
    double* out = part + (int64_t)blockIdx.x * (nc * nc + nc);
    for (int e = threadIdx.x; e < nc * nc + nc; e += blockDim.x) {
        double s = 0;
        if (e < nc * nc) {
            const int c = e / nc, j = e % nc;
            for (int t = 0; t < ns; ++t) s += g[c * 64 + t] * (double)X1T[(s0 + t) * ld + j];
        } else {
            const int c = e - nc * nc;
            if constexpr (G == ICA_G_LOGCOSH) {
                for (int t = 0; t < ns; ++t) s += 1.0 - g[c * 64 + t] * g[c * 64 + t];
            } else {
                for (int t = 0; t < ns; ++t) s += gd[c * 64 + t];
            }
        }
        out[e] = s;
    }
}
template <class T>
__global__ void k_ica_simple(const T* __restrict__ X1T, int64_t n, int nc, int64_t ld, const double* __restrict__ W,
                             double* __restrict__ part, const int* __restrict__ state) {
    ica_simple_body<T, ICA_G_LOGCOSH>(X1T, n, nc, ld, W, part, state);
}
template <class T, int G>
__global__ void k_ica_simple_g(const T* __restrict__ X1T, int64_t n, int nc, int64_t ld, const double* __restrict__ W,
                               double* __restrict__ part, const int* __restrict__ state) {
    ica_simple_body<T, G>(X1T, n, nc, ld, W, part, state);
}
__global__ void k_sum_parts_state(const double* __restrict__ part, int64_t nparts, int64_t count, double* __restrict__ out,
                                  const int* __restrict__ state) {
    if (state && state[0]) return;
    const int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (j >= count) return;
    double s = 0;
    for (int64_t p = 0; p < nparts; ++p) s += part[p * count + j];
    out[j] = s;
}


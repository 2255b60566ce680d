// k_ica_mfma_body.inc -- the body of k_ica_mfma<NT> and k_ica_mfma_g<NT, G> (k_ica_step.inc includes it into both, with the contrast G a
// constant of the one and a template parameter of the other: the logcosh kernel stays the code it was, statement for statement).
    if (state && state[0]) return;
    constexpr int NCP = 16 * NT;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = lane & 15, q = lane >> 4;
    const int64_t wid = (int64_t)blockIdx.x * 4 + wave;
    f32x4 wf[NT][NT];  // [kc][nt]
#pragma unroll
    for (int kc = 0; kc < NT; ++kc)
#pragma unroll
        for (int u = 0; u < NT; ++u) wf[kc][u] = reinterpret_cast<const f32x4*>(Wpk)[(kc * NT + u) * 64 + lane];
    f32x4 dacc[NT][NT];  // [component tile][x tile]
    float gpa[NT];
#pragma unroll
    for (int a = 0; a < NT; ++a) {
        gpa[a] = 0.f;
#pragma unroll
        for (int b = 0; b < NT; ++b) dacc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const int64_t t0 = wid * tiles_per_wave, t1 = min((n + 15) / 16, t0 + tiles_per_wave);
    for (int64_t tile = t0; tile < t1; ++tile) {
        const int64_t r0 = tile * 16;
        // A layout: lane (i, q) <- X1[r0 + i][16 kc + 4 q .. +3]
        const int64_t ra = r0 + i;
        const bool va = ra < n;
        f32x4 xa[NT];
#pragma unroll
        for (int kc = 0; kc < NT; ++kc)
            xa[kc] = va ? *reinterpret_cast<const f32x4*>(X1T + ra * ld + 16 * kc + 4 * q) : f32x4{0.f, 0.f, 0.f, 0.f};
        // B layout for the second product: lane (j = i, q), k-step s <- X1[r0 + 4 q + s][16 b + j]
        float xb[4][NT];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int64_t rb = r0 + 4 * q + s;
            const bool vb = rb < n;
#pragma unroll
            for (int b = 0; b < NT; ++b) xb[s][b] = vb ? X1T[rb * ld + 16 * b + i] : 0.f;
        }
        f32x4 sacc[NT];
#pragma unroll
        for (int u = 0; u < NT; ++u) sacc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kc = 0; kc < NT; ++kc)
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int u = 0; u < NT; ++u)
                    sacc[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[kc][s], wf[kc][u][s], sacc[u], 0, 0, 0);
        // sacc[u][r] = S[sample r0 + 4 q + r][component 16 u + i]
#pragma unroll
        for (int u = 0; u < NT; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if constexpr (G == ICA_G_LOGCOSH) {
                    const float g = tanh_fast(sacc[u][r]);
                    const bool v = (r0 + 4 * q + r) < n;
                    sacc[u][r] = v ? g : 0.f;
                    gpa[u] += v ? (1.0f - g * g) : 0.f;
                } else {
                    float g, gp;
                    ica_contrast<G>(sacc[u][r], g, gp);
                    const bool v = (r0 + 4 * q + r) < n;
                    sacc[u][r] = v ? g : 0.f;
                    gpa[u] += v ? gp : 0.f;
                }
            }
        // D[component][x] += sum_samples G[sample][component] X1[sample][x]:
        // A operand (i = component, k = q) of k-step s is G[r0 + 4 q + s][16 a + i] = sacc[a][s]
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int a = 0; a < NT; ++a)
#pragma unroll
                for (int b = 0; b < NT; ++b)
                    dacc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(sacc[a][s], xb[s][b], dacc[a][b], 0, 0, 0);
    }
    __shared__ float s_slab[2 * (NCP * NCP + NCP)];
    ica_write_slab<NT>(dacc, gpa, s_slab, part);

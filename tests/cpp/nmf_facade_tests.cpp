// Nmf in the C++ facade (include/petal_decomposition.hpp over petal_hip_nmf.h): a custom-init fit of 60 x 12 rows against the statement
// restated here in plain loops, fit_transform's W, transform, inverse_transform = W H, the random initialisation twice with one seed,
// the forced composed path against the default path, info() and the errors.
//   nmf_facade_tests kernel      the library has k_nmf_pass (libpetal_hip.so)
//   nmf_facade_tests fallback    it has not (the host simulation): the same statements from the library's other products
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "petal_decomposition.hpp"

using namespace petal_decomposition;

static int failures = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static const double EPS = 1.1920928955078125e-07;

// one iteration of the header's statement on row-major vectors (w: n x k, h: k x d)
static void iterate(const Array2<double>& x, std::vector<double>& w, std::vector<double>& h, int n, int d, int k) {
    std::vector<double> hht(size_t(k) * k, 0.0), a(size_t(k) * d, 0.0), b(size_t(k) * k, 0.0);
    for (int p = 0; p < k; ++p)
        for (int q = 0; q < k; ++q)
            for (int j = 0; j < d; ++j) hht[p * k + q] += h[p * d + j] * h[q * d + j];
    for (int i = 0; i < n; ++i) {
        std::vector<double> wn(k);
        for (int p = 0; p < k; ++p) {
            double z = 0, den = 0;
            for (int j = 0; j < d; ++j) z += x(i, j) * h[p * d + j];
            for (int q = 0; q < k; ++q) den += w[i * k + q] * hht[q * k + p];
            if (den == 0) den = EPS;
            wn[p] = w[i * k + p] * (z / den);
        }
        for (int p = 0; p < k; ++p) w[i * k + p] = wn[p];
    }
    for (int p = 0; p < k; ++p) {
        for (int j = 0; j < d; ++j)
            for (int i = 0; i < n; ++i) a[p * d + j] += w[i * k + p] * x(i, j);
        for (int q = 0; q < k; ++q)
            for (int i = 0; i < n; ++i) b[p * k + q] += w[i * k + p] * w[i * k + q];
    }
    std::vector<double> hn(h);
    for (int p = 0; p < k; ++p)
        for (int j = 0; j < d; ++j) {
            double den = 0;
            for (int q = 0; q < k; ++q) den += b[p * k + q] * h[q * d + j];
            if (den == 0) den = EPS;
            hn[p * d + j] = h[p * d + j] * (a[p * d + j] / den);
        }
    h = hn;
}

int main(int argc, char** argv) {
    const bool fallback = argc > 1 && std::strcmp(argv[1], "fallback") == 0;
    const int n = 60, d = 12, k = 3, m = 7, iters = 5;
    Pcg rng((unsigned __int128)1234567891011121314ull + 38);
    Array2<double> x(n, d), xq(m, d), w0(n, k), h0(k, d);
    for (int i = 0; i < n + m; ++i) {
        double f[3];
        for (int t = 0; t < 3; ++t) f[t] = std::fabs(rng.standard_normal());
        for (int j = 0; j < d; ++j) {
            double v = 0.02 * std::fabs(rng.standard_normal());
            for (int t = 0; t < 3; ++t) v += f[t] * (1.0 + std::sin(0.9 * (t + 1) * j + 0.3 * t));
            (i < n ? x(i, j) : xq(i - n, j)) = v;
        }
    }
    for (auto& v : w0.data) v = 0.5 * std::fabs(rng.standard_normal()) + 0.01;
    for (auto& v : h0.data) v = 0.5 * std::fabs(rng.standard_normal()) + 0.01;
    Context ctx;
    static_assert(PETAL_OPT_NMF_FALLBACK == 38, "petal_hip_nmf.h");
    CHECK(ctx.get_option(PETAL_OPT_NMF_FALLBACK) == 0.0);
    {
        Nmf<double> nm(k, iters, 0.0, 0, 0.0, -1.0, 0.0, &ctx);
        const Array2<double> w = nm.fit_transform(x, w0, h0);
        const NmfInfo in = nm.info();
        CHECK(in.n == n && in.d == d && in.k == k && in.n_iter == iters && nm.n_iter() == iters);
        CHECK(in.fit_kernel == !fallback && in.transform_kernel == -1);
        std::vector<double> mw(w0.data), mh(h0.data);
        for (int it = 0; it < iters; ++it) iterate(x, mw, mh, n, d, k);
        const Array2<double> h = nm.components();
        double wmax = 0, hmax = 0, res = 0;
        for (double v : mw) wmax = std::max(wmax, v);
        for (double v : mh) hmax = std::max(hmax, v);
        for (int i = 0; i < n * k; ++i) CHECK(std::fabs(w.data[i] - mw[i]) <= 1e-9 * wmax);
        for (int i = 0; i < k * d; ++i) CHECK(std::fabs(h.data[i] - mh[i]) <= 1e-9 * hmax);
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < d; ++j) {
                double v = x(i, j);
                for (int p = 0; p < k; ++p) v -= mw[i * k + p] * mh[p * d + j];
                res += v * v;
            }
        CHECK(std::fabs(nm.reconstruction_err() - std::sqrt(res)) <= 1e-9 * std::sqrt(res));
        // transform of fresh rows, inverse_transform = W H
        const Array2<double> wq = nm.transform(xq);
        CHECK(nm.info().transform_kernel == (fallback ? 0 : 1));
        CHECK(wq.nrows() == m && wq.ncols() == k);
        const Array2<double> back = nm.inverse_transform(wq);
        double bmax = 0;
        for (double v : back.data) bmax = std::max(bmax, std::fabs(v));
        for (int i = 0; i < m; ++i)
            for (int j = 0; j < d; ++j) {
                double v = 0;
                for (int p = 0; p < k; ++p) v += wq(i, p) * h(p, j);
                CHECK(std::fabs(back(i, j) - v) <= 1e-9 * bmax);
                CHECK(wq(i, 0) >= 0);
            }
        // the forced composed path agrees with the default path
        ctx.set_option(PETAL_OPT_NMF_FALLBACK, 1);
        Nmf<double> nf(k, iters, 0.0, 0, 0.0, -1.0, 0.0, &ctx);
        const Array2<double> wf = nf.fit_transform(x, w0, h0);
        const Array2<double> wqf = nf.transform(xq);
        CHECK(!nf.info().fit_kernel && nf.info().transform_kernel == 0);
        ctx.set_option(PETAL_OPT_NMF_FALLBACK, 0);
        for (int i = 0; i < n * k; ++i) CHECK(std::fabs(wf.data[i] - w.data[i]) <= 1e-9 * wmax);
        for (int i = 0; i < m * k; ++i) CHECK(std::fabs(wqf.data[i] - wq.data[i]) <= 1e-9 * wmax);
        // random initialisation: one seed twice gives the same bytes, another seed does not; the loss falls
        Nmf<float> r1(k, 20, 0.0, 7, 0.0, -1.0, 0.0, &ctx), r2(k, 20, 0.0, 7, 0.0, -1.0, 0.0, &ctx), r3(k, 20, 0.0, 8, 0.0, -1.0, 0.0, &ctx);
        Array2<float> xf(n, d);
        for (int i = 0; i < n * d; ++i) xf.data[i] = float(x.data[i]);
        const Array2<float> a1 = r1.fit_transform(xf), a2 = r2.fit_transform(xf), a3 = r3.fit_transform(xf);
        CHECK(std::memcmp(a1.data.data(), a2.data.data(), sizeof(float) * a1.data.size()) == 0);
        CHECK(std::memcmp(a1.data.data(), a3.data.data(), sizeof(float) * a1.data.size()) != 0);
        double nx = 0;
        for (double v : x.data) nx += v * v;
        CHECK(r1.reconstruction_err() < 0.5 * std::sqrt(nx));
        // a regularised fit runs and shrinks W
        Nmf<double> rg(k, iters, 0.0, 0, 0.05, 0.02, 0.3, &ctx);
        const Array2<double> wr = rg.fit_transform(x, w0, h0);
        double sw = 0, swr = 0;
        for (int i = 0; i < n * k; ++i) { sw += w.data[i]; swr += wr.data[i]; }
        CHECK(swr < sw);
        // errors
        bool threw = false;
        try { Nmf<double>(d + 1, iters, 0.0, 0, 0.0, -1.0, 0.0, &ctx).fit(x); }
        catch (const DecompositionError& e) { threw = std::string(e.what()).find("every dimension should be at least") != std::string::npos; }
        CHECK(threw);
        threw = false;
        try { nm.transform(Array2<double>(2, d + 1)); }
        catch (const DecompositionError& e) { threw = std::string(e.what()).find("# of columns should be 12") != std::string::npos; }
        CHECK(threw);
        threw = false;
        Array2<double> neg(x);
        neg(3, 4) = -1.0;
        try { Nmf<double>(k, iters, 0.0, 0, 0.0, -1.0, 0.0, &ctx).fit(neg); }
        catch (const DecompositionError& e) { threw = std::string(e.what()).find("negative values in data") != std::string::npos; }
        CHECK(threw);
        threw = false;
        try { Nmf<double>(k, 0, 0.0, 0, 0.0, -1.0, 0.0, &ctx).fit(x); } catch (const DecompositionError&) { threw = true; }
        CHECK(threw);
        threw = false;
        try { Nmf<double>(k, iters, 0.0, 0, 0.0, -1.0, 0.0, &ctx).transform(x); } catch (const DecompositionError&) { threw = true; }
        CHECK(threw);
    }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("nmf facade tests passed (%s)\n", fallback ? "fallback" : "kernel");
    return 0;
}

// KernelPca in the C++ facade (include/petal_decomposition.hpp over petal_hip_kpca.h): an rbf fit of 60 x 12 rows -- transform of the
// training rows equals fit_transform, the forced fallback agrees with the default path, the linear kernel equals Pca, info() and the
// errors.
//   kpca_facade_tests kernel      the library has k_kmap / k_kapply (libpetal_hip.so)
//   kpca_facade_tests fallback    it has not (the host simulation): the same statements from the library's other products
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>

#include "petal_decomposition.hpp"

using namespace petal_decomposition;

static int failures = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

int main(int argc, char** argv) {
    const bool fallback = argc > 1 && std::strcmp(argv[1], "fallback") == 0;
    const int n = 60, d = 12, k = 3, m = 7;
    Pcg rng((unsigned __int128)1234567891011121314ull + 35);
    Array2<double> x(n, d), xq(m, d);
    for (int i = 0; i < n + m; ++i) {
        double f[3];
        for (int t = 0; t < 3; ++t) f[t] = 2.0 * std::pow(0.6, t) * rng.standard_normal();
        for (int j = 0; j < d; ++j) {
            double v = 1.0 + 0.1 * j + 0.05 * rng.standard_normal();
            for (int t = 0; t < 3; ++t) v += f[t] * std::sin(0.9 * (t + 1) * j + 0.3 * t);
            (i < n ? x(i, j) : xq(i - n, j)) = v;
        }
    }
    Context ctx;
    static_assert(PETAL_OPT_KPCA_FALLBACK == 36 && PETAL_KERNEL_RBF == 2 && PETAL_KERNEL_COSINE == 4, "petal_hip_kpca.h");
    CHECK(ctx.get_option(PETAL_OPT_KPCA_FALLBACK) == 0.0);
    {
        KernelPca<double> kp(k, PETAL_KERNEL_RBF, 0.0, 3, 1.0, &ctx);
        const Array2<double> y = kp.fit_transform(x);
        KernelPcaInfo in = kp.info();
        CHECK(in.n == n && in.d == d && in.k == k && in.order == n && in.kernel == PETAL_KERNEL_RBF);
        CHECK(in.fit_kernel == !fallback && in.transform_kernel == -1);
        const Array2<double> yt = kp.transform(x);
        CHECK(kp.info().transform_kernel == (fallback ? 0 : 1));
        const std::vector<double> lam = kp.eigenvalues();
        CHECK(lam.size() == size_t(k) && lam[0] >= lam[1] && lam[1] >= lam[2] && lam[2] > 0);
        for (int j = 0; j < k; ++j) {
            double ss = 0;
            for (int i = 0; i < n; ++i) {
                CHECK(std::fabs(y(i, j) - yt(i, j)) <= 1e-9 * std::sqrt(lam[0]));
                ss += y(i, j) * y(i, j);
            }
            CHECK(std::fabs(ss - lam[j]) <= 1e-9 * lam[0]);   // |V sqrt(lambda)|^2 per column = lambda
        }
        const Array2<double> yq = kp.transform(xq);
        ctx.set_option(PETAL_OPT_KPCA_FALLBACK, 1);
        KernelPca<double> kf(k, PETAL_KERNEL_RBF, 0.0, 3, 1.0, &ctx);
        kf.fit(x);
        const Array2<double> yf = kf.transform(xq);
        CHECK(!kf.info().fit_kernel && kf.info().transform_kernel == 0);
        ctx.set_option(PETAL_OPT_KPCA_FALLBACK, 0);
        for (int j = 0; j < k; ++j)
            for (int i = 0; i < m; ++i) CHECK(std::fabs(yq(i, j) - yf(i, j)) <= 1e-9 * std::sqrt(lam[0]));
        // the linear kernel is Pca
        KernelPca<double> kl(k, PETAL_KERNEL_LINEAR, 0.0, 3, 1.0, &ctx);
        const Array2<double> yl = kl.fit_transform(x);
        Pca<double> pca(k, true, &ctx);
        const Array2<double> yp = pca.fit_transform(x);
        const double s0 = pca.singular_values()[0];
        for (int j = 0; j < k; ++j) {
            CHECK(std::fabs(kl.eigenvalues()[j] - pca.singular_values()[j] * pca.singular_values()[j]) <= 1e-9 * s0 * s0);
            for (int i = 0; i < n; ++i) CHECK(std::fabs(yl(i, j) - yp(i, j)) <= 1e-9 * s0);
        }
        // errors
        bool threw = false;
        try { KernelPca<double>(n + 1, PETAL_KERNEL_RBF, 0.0, 3, 1.0, &ctx).fit(x); }
        catch (const DecompositionError& e) { threw = std::string(e.what()).find("every dimension should be at least") != std::string::npos; }
        CHECK(threw);
        threw = false;
        try { kp.transform(Array2<double>(2, d + 1)); }
        catch (const DecompositionError& e) { threw = std::string(e.what()).find("# of columns should be 12") != std::string::npos; }
        CHECK(threw);
        threw = false;
        try { KernelPca<double>(2, 9, 0.0, 3, 1.0, &ctx).fit(x); } catch (const DecompositionError&) { threw = true; }
        CHECK(threw);
        threw = false;
        try { KernelPca<double>(2, PETAL_KERNEL_POLY, 0.0, 0, 1.0, &ctx).fit(x); } catch (const DecompositionError&) { threw = true; }
        CHECK(threw);
        threw = false;
        try { KernelPca<double>(2, PETAL_KERNEL_RBF, 0.0, 3, 1.0, &ctx).transform(x); } catch (const DecompositionError&) { threw = true; }
        CHECK(threw);
    }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("kpca facade tests passed (%s)\n", fallback ? "fallback" : "kernel");
    return 0;
}

// Exact Pca on wide data in the C++ facade (include/petal_decomposition.hpp over petal_hip_wide.h): a 40 x 300 fit on the dual route
// against the same fit on the primal route, the option constants through Context::set_option / get_option, Pca::last_route().
//   wide_facade_tests kernel      the library has k_row_gram (libpetal_hip.so)
//   wide_facade_tests fallback    it has not (the host simulation): K comes from the library's other products
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
    const int n = 40, d = 300, k = 5;
    // five planted directions with gaps over small noise, a mean away from zero
    Pcg rng((unsigned __int128)1234567891011121314ull + 33);
    Array2<double> x(n, d);
    for (int i = 0; i < n; ++i) {
        double f[5];
        for (int t = 0; t < 5; ++t) f[t] = 30.0 * std::pow(0.45, t) * rng.standard_normal();
        for (int j = 0; j < d; ++j) {
            double v = 3.0 + 0.01 * j + 0.01 * rng.standard_normal();
            for (int t = 0; t < 5; ++t) v += f[t] * std::sin(0.37 * (t + 1) * j + 0.3 * t);
            x(i, j) = v;
        }
    }
    Context ctx;
    static_assert(PETAL_OPT_PCA_DUAL == 33 && PETAL_OPT_PCA_DUAL_FALLBACK == 34, "petal_hip_wide.h");
    CHECK(ctx.get_option(PETAL_OPT_PCA_DUAL) == 0.0 && ctx.get_option(PETAL_OPT_PCA_DUAL_FALLBACK) == 0.0);

    ctx.set_option(PETAL_OPT_PCA_DUAL, 1);
    CHECK(ctx.get_option(PETAL_OPT_PCA_DUAL) == 1.0);
    Pca<double> dual(k, true, &ctx);
    const Array2<double> yd = dual.fit_transform(x);
    const PcaRoute rd = dual.last_route();
    CHECK(rd.dual && rd.order == n && rd.kernel == !fallback && (rd.chunks >= 1) == !fallback);

    ctx.set_option(PETAL_OPT_PCA_DUAL, -1);
    CHECK(ctx.get_option(PETAL_OPT_PCA_DUAL) == -1.0);
    Pca<double> primal(k, true, &ctx);
    const Array2<double> yp = primal.fit_transform(x);
    const PcaRoute rp = primal.last_route();
    CHECK(!rp.dual && rp.order == d && !rp.kernel && rp.chunks == 0);
    ctx.set_option(PETAL_OPT_PCA_DUAL, 0);

    const double s0 = primal.singular_values()[0];
    for (int j = 0; j < k; ++j) {
        CHECK(std::fabs(dual.singular_values()[j] - primal.singular_values()[j]) <= 2e-8 * s0);
        for (int i = 0; i < d; ++i) CHECK(std::fabs(dual.components()(j, i) - primal.components()(j, i)) <= 2e-8);   // signs included
        for (int i = 0; i < n; ++i) CHECK(std::fabs(yd(i, j) - yp(i, j)) <= 2e-8 * s0);
    }
    for (int j = 0; j < d; ++j) CHECK(dual.mean()[j] == primal.mean()[j]);
    CHECK(std::fabs(dual.explained_variance_ratio()[0] - primal.explained_variance_ratio()[0]) <= 1e-9);

    // the default rule leaves a narrow fit on the primal route
    Pca<double> narrow(k, true, &ctx);
    narrow.fit(x);
    CHECK(!narrow.last_route().dual);

    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("wide facade tests passed (%s)\n", fallback ? "fallback" : "kernel");
    return 0;
}

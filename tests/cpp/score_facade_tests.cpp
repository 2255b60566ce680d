// The row-score members of the C++ facade's Pca / RandomizedPca (include/petal_decomposition.hpp over petal_hip_score.h).
//   score_facade_tests scores    the library has the score op (libpetal_hip.so): the scores are checked against their definitions
//   score_facade_tests refuses   it has not (the host simulation): InvalidInput with the refusal message -- after the argument checks
// In both: explained_variance / noise_variance follow their formulas, a wrong column count is the crate's transform message.
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

static const unsigned __int128 RNG_SEED = (unsigned __int128)1234567891011121314ull;

// 400 x 6: three strong directions, weak isotropic noise, means off the origin
static Array2<double> data(int n) {
    Pcg rng(RNG_SEED + 2);
    Array2<double> x(n, 6);
    for (int i = 0; i < n; ++i) {
        const double a = 3.0 * rng.standard_normal(), b = 2.0 * rng.standard_normal(), c = rng.standard_normal();
        const double s[6] = {a + b, a - b, c + 0.5 * a, c - b, 0.25 * c, a};
        for (int j = 0; j < 6; ++j) x(i, j) = 5.0 + j + s[j] + 0.1 * rng.standard_normal();
    }
    return x;
}

int main(int argc, char** argv) {
    const bool refuses = argc > 1 && std::strcmp(argv[1], "refuses") == 0;
    const int n = 400, k = 3;
    const Array2<double> x = data(n);
    Pca<double> pca(k);
    pca.fit(x);
    const auto sv = pca.singular_values();
    const auto ev = pca.explained_variance();
    const auto evr = pca.explained_variance_ratio();
    CHECK(ev.size() == size_t(k));
    double kept = 0;
    for (int j = 0; j < k; ++j) { CHECK(std::fabs(ev[j] - sv[j] * sv[j] / (n - 1)) <= 1e-12 * ev[j]); kept += sv[j] * sv[j]; }
    const double total = sv[0] * sv[0] / evr[0];
    const double s2 = pca.noise_variance();
    CHECK(s2 > 0 && std::fabs(s2 - (total - kept) / (n - 1) / (6 - k)) <= 1e-9 * s2);
    CHECK(Pca<double>(6).noise_variance() == 0.0);   // (unfitted / nothing discarded: 0, and score_samples refuses)
    try { pca.reconstruction_error(Array2<double>(4, 5)); CHECK(false); } catch (const DecompositionError& e) {
        CHECK(e.kind == DecompositionError::InvalidInput && std::string(e.what()).find("# of columns should be 6") != std::string::npos);
    }
    try {
        const auto q = pca.reconstruction_error(x);
        const auto t2 = pca.hotelling_t2(x);
        const auto ll = pca.score_samples(x);
        CHECK(!refuses);
        const auto y = pca.transform(x);
        const auto xr = pca.inverse_transform(y);
        CHECK(q.size() == size_t(n) && t2.size() == size_t(n) && ll.size() == size_t(n));
        for (int i = 0; i < n; ++i) {
            double r = 0, xx = 0, t = 0;
            for (int j = 0; j < 6; ++j) { r += (x(i, j) - xr(i, j)) * (x(i, j) - xr(i, j)); xx += (x(i, j) - pca.mean()[j]) * (x(i, j) - pca.mean()[j]); }
            for (int j = 0; j < k; ++j) t += y(i, j) * y(i, j) / ev[j];
            CHECK(q[i] >= 0 && std::fabs(q[i] - r) <= 1e-12 * xx);
            CHECK(std::fabs(t2[i] - t) <= 1e-12 * (1 + t));
            double c = 6 * std::log(2 * 3.14159265358979323846) + (6 - k) * std::log(s2);
            for (int j = 0; j < k; ++j) c += std::log(ev[j]);
            const double want = -0.5 * (c + r / s2 + t);
            CHECK(std::fabs(ll[i] - want) <= 1e-9 * (1 + std::fabs(want)));
        }
        auto rp = RandomizedPca<double>::with_seed(k, RNG_SEED);
        rp.fit(x);
        const auto q2 = rp.reconstruction_error(x);
        for (int i = 0; i < n; ++i) CHECK(std::fabs(q2[i] - q[i]) <= 1e-6 * (1 + q[i]));
    } catch (const DecompositionError& e) {
        CHECK(refuses);
        CHECK(e.kind == DecompositionError::InvalidInput && std::string(e.what()).find("row scores not available in this device-op layer") != std::string::npos);
    }
    Pca<double> full(6);
    full.fit(x);
    try { full.score_samples(x); CHECK(false); } catch (const DecompositionError& e) {
        CHECK(e.kind == DecompositionError::InvalidInput && std::string(e.what()).find("noise variance is not positive") != std::string::npos);
    }
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("score facade tests passed (%s)\n", refuses ? "refuses" : "scores");
    return 0;
}

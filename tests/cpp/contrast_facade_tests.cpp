// The contrast member of the C++ facade's FastIca (include/petal_decomposition.hpp) and the builder's setter.
//   contrast_facade_tests fits      the library has the exp / cube step (libpetal_hip.so): the fits must separate two sources
//   contrast_facade_tests refuses   it has not (the host simulation): InvalidInput with the refusal message, never a tanh fit
// In both: an explicit PETAL_ICA_CONTRAST_LOGCOSH is the default fit, and an undefined contrast field is InvalidInput.
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

// two independent sub-Gaussian sources (uniform, from the facade's own generator), mixed
static Array2<double> mixed(int n) {
    Pcg rng(RNG_SEED + 1);
    Array2<double> x(n, 2);
    for (int i = 0; i < n; ++i) {
        // Phi(z) of a standard normal is uniform: erf keeps the test free of another generator
        const double s0 = std::erf(rng.standard_normal() / std::sqrt(2.0)), s1 = std::erf(rng.standard_normal() / std::sqrt(2.0));
        x(i, 0) = 2.0 * s0 + 1.0 * s1;
        x(i, 1) = 1.0 * s0 - 1.5 * s1;
    }
    return x;
}
// |correlation| of the recovered sources with each other: independent components are uncorrelated, and unit-norm by construction
static double cross(const Array2<double>& y) {
    double c = 0, a = 0, b = 0;
    for (int64_t i = 0; i < y.nrows(); ++i) { c += y(i, 0) * y(i, 1); a += y(i, 0) * y(i, 0); b += y(i, 1) * y(i, 1); }
    return std::fabs(c) / std::sqrt(a * b);
}

int main(int argc, char** argv) {
    const bool refuses = argc > 1 && std::strcmp(argv[1], "refuses") == 0;
    const Array2<double> x = mixed(4000);
    auto base = FastIca<double>::with_seed(RNG_SEED);
    const auto y0 = base.fit_transform(x);
    auto same = FastIcaBuilder<>::new_().seed(RNG_SEED).contrast(PETAL_ICA_CONTRAST_LOGCOSH).build<double>();
    CHECK(same.contrast == PETAL_ICA_CONTRAST_LOGCOSH);
    const auto y1 = same.fit_transform(x);
    CHECK(base.n_iter() == same.n_iter() && y0.data.size() == y1.data.size());
    for (size_t i = 0; i < y0.data.size(); ++i) CHECK(y0.data[i] == y1.data[i]);
    for (int contrast : {PETAL_ICA_CONTRAST_EXP, PETAL_ICA_CONTRAST_CUBE}) {
        auto ica = FastIcaBuilder<>::new_().seed(RNG_SEED).contrast(contrast).build<double>();
        CHECK(ica.contrast == contrast);
        try {
            const auto y = ica.fit_transform(x);
            CHECK(!refuses);
            CHECK(ica.n_iter() >= 1 && ica.n_iter() < 200);
            CHECK(y.nrows() == 4000 && y.ncols() == 2 && cross(y) < 1e-6);
            bool differs = false;
            for (size_t i = 0; i < y.data.size(); ++i) { CHECK(std::isfinite(y.data[i])); differs = differs || y.data[i] != y0.data[i]; }
            CHECK(differs);   // not the tanh fit
        } catch (const DecompositionError& e) {
            CHECK(refuses);
            CHECK(e.kind == DecompositionError::InvalidInput && std::string(e.what()).find("contrast not available in this device-op layer") != std::string::npos);
        }
    }
    auto bad = FastIca<double>::with_seed(RNG_SEED);
    bad.contrast = 48;
    try { bad.fit(x); CHECK(false); } catch (const DecompositionError& e) {
        CHECK(e.kind == DecompositionError::InvalidInput && std::string(e.what()).find("contrast") != std::string::npos);
    }
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("contrast facade tests passed (%s)\n", refuses ? "refuses" : "fits");
    return 0;
}

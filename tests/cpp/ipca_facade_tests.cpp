// IncrementalPca in the C++ facade (include/petal_decomposition.hpp over petal_hip_ipca.h): batches against Pca::fit on the concatenation,
// the sign rule, merge, the state round trip, reset, and the error messages.
//   ipca_facade_tests kernel      the library has the streaming kernel (libpetal_hip.so): every batch is a kernel batch
//   ipca_facade_tests fallback    it has not (the host simulation): no batch is
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

template <class F>
static std::string message_of(F&& f) {
    try { f(); } catch (const DecompositionError& e) { return e.what(); }
    return "";
}

static Array2<double> rows_of(const Array2<double>& x, int64_t a, int64_t b) {
    Array2<double> out(b - a, x.ncols());
    for (int64_t i = a; i < b; ++i)
        for (int64_t j = 0; j < x.ncols(); ++j) out(i - a, j) = x(i, j);
    return out;
}

int main(int argc, char** argv) {
    const bool fallback = argc > 1 && std::strcmp(argv[1], "fallback") == 0;
    const int n = 300, d = 24, k = 3;
    // three planted directions with gaps over unit noise, a mean away from zero
    Pcg rng((unsigned __int128)1234567891011121314ull + 5);
    Array2<double> x(n, d);
    for (int i = 0; i < n; ++i) {
        const double f[3] = {30.0 * rng.standard_normal(), 12.0 * rng.standard_normal(), 5.0 * rng.standard_normal()};
        for (int j = 0; j < d; ++j)
            x(i, j) = 3.0 + 0.1 * j + f[0] * std::sin(0.7 * j + 0.3) + f[1] * std::cos(1.3 * j) + f[2] * std::sin(2.1 * j * j) + rng.standard_normal();
    }
    Pca<double> whole(k);
    whole.fit(x);

    const int64_t cuts[5] = {0, 1, 100, 117, n};
    IncrementalPca<double> inc(k);
    CHECK(inc.n_samples_seen() == 0);
    for (int b = 0; b < 4; ++b) inc.partial_fit(rows_of(x, cuts[b], cuts[b + 1]));
    inc.partial_fit(Array2<double>(0, d));                             // an empty batch is a no-op
    const std::vector<int64_t> info = inc.info();
    CHECK(info[0] == d && info[1] == PETAL_F64 && info[2] == 1 && info[3] == n && info[4] == 4 && info[5] == (fallback ? 0 : 4));
    const double s0 = whole.singular_values()[0];
    for (int j = 0; j < k; ++j) {
        CHECK(std::fabs(inc.singular_values()[j] - whole.singular_values()[j]) <= 1e-9 * s0);
        double dot = 0, big = 0;
        int at = 0;
        for (int i = 0; i < d; ++i) {
            dot += inc.components()(j, i) * whole.components()(j, i);
            if (std::fabs(inc.components()(j, i)) > big) { big = std::fabs(inc.components()(j, i)); at = i; }
        }
        CHECK(inc.components()(j, at) > 0);                            // the sign rule: the entry of largest magnitude is positive
        const double sg = dot < 0 ? -1.0 : 1.0;
        for (int i = 0; i < d; ++i) CHECK(std::fabs(sg * inc.components()(j, i) - whole.components()(j, i)) <= 1e-9);
    }
    for (int j = 0; j < d; ++j) CHECK(std::fabs(inc.mean()[j] - whole.mean()[j]) <= 1e-12 * (1.0 + std::fabs(whole.mean()[j])));
    CHECK(std::fabs(inc.noise_variance() - whole.noise_variance()) <= 1e-9 * whole.noise_variance());
    const Array2<double> ti = inc.transform(x), tw = whole.transform(x);
    for (int j = 0; j < k; ++j) {
        const double sg = ti(0, j) * tw(0, j) < 0 ? -1.0 : 1.0;
        for (int i = 0; i < n; ++i) CHECK(std::fabs(sg * ti(i, j) - tw(i, j)) <= 1e-8 * s0);
    }
    CHECK(inc.explained_variance().size() == size_t(k));
    if (!fallback) {   // (row scores are a kernel of the device library; the host simulation has none)
        const std::vector<double> qi = inc.reconstruction_error(x), qw = whole.reconstruction_error(x);
        for (int i = 0; i < n; ++i) CHECK(std::fabs(qi[i] - qw[i]) <= 1e-8 * s0 * s0);
    }

    // two handles over a split of the rows, merged, against the one handle; the state round trip; reset
    IncrementalPca<double> left(k), right(k), empty(k);
    left.partial_fit(rows_of(x, 0, 130));
    right.partial_fit(rows_of(x, 130, 200)).partial_fit(rows_of(x, 200, n));
    left.merge(right).merge(empty);
    CHECK(left.n_samples_seen() == n && right.n_samples_seen() == n - 130 && left.info()[6] == 1);
    for (int j = 0; j < k; ++j) CHECK(std::fabs(left.singular_values()[j] - inc.singular_values()[j]) <= 1e-9 * s0);
    std::vector<double> mean, m2;
    const double seen = inc.get_state(mean, m2);
    CHECK(seen == n && mean.size() == size_t(d) && m2.size() == size_t(d) * d);
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) CHECK(m2[i * d + j] == m2[j * d + i]);
    IncrementalPca<double> restored(k);
    restored.set_state(seen, mean, m2);
    for (int j = 0; j < k; ++j) {
        CHECK(restored.singular_values()[j] == inc.singular_values()[j]);
        for (int i = 0; i < d; ++i) CHECK(restored.components()(j, i) == inc.components()(j, i));
    }
    restored.reset();
    CHECK(restored.n_samples_seen() == 0 && restored.components().ncols() == 0);

    // the error messages
    CHECK(message_of([&] { inc.partial_fit(Array2<double>(4, d + 1)); }).find("# of columns should be 24") != std::string::npos);
    IncrementalPca<double> big(d + 1);
    big.partial_fit(x);
    CHECK(message_of([&] { big.components(); }).find("every dimension should be at least 25") != std::string::npos);
    IncrementalPca<double> none(k);
    none.partial_fit(Array2<double>(0, d));
    CHECK(none.info()[4] == 0 && none.components().ncols() == 0);      // nothing seen: the model stays empty
    none.set_state(0.0, mean, m2);
    CHECK(none.n_samples_seen() == 0 && none.singular_values().empty());
    IncrementalPca<double> other(k, false);
    other.partial_fit(x);
    CHECK(message_of([&] { inc.merge(other); }).find("differ in d, dtype or centering") != std::string::npos);

    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("ipca facade tests passed (%s)\n", fallback ? "fallback" : "kernel");
    return 0;
}

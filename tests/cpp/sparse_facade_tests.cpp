// CsrMatrix and the sparse overloads of RandomizedPca in the C++ facade (include/petal_decomposition.hpp over petal_hip_sparse.h): a sparse
// fit against the dense fit of the same matrix from the same generator state, the transform, the test aid product, and the error messages.
//   sparse_facade_tests kernel      the library has the sparse product kernel (libpetal_hip.so): kernel_path == 1, close to the dense fit
//   sparse_facade_tests fallback    it has not (the host simulation): kernel_path == 0 and the fit equals the dense fit bit for bit
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

template <class F>
static std::string message_of(F&& f) {
    try { f(); } catch (const DecompositionError& e) { return e.what(); }
    return "";
}

int main(int argc, char** argv) {
    const bool fallback = argc > 1 && std::strcmp(argv[1], "fallback") == 0;
    const int n = 300, d = 40, k = 3;
    // a sparse low-rank matrix: three planted factors with sparse support, a little sparse noise, one long row
    Pcg rng(RNG_SEED + 9);
    Array2<double> x(n, d);
    for (int f = 0; f < 6; ++f) {
        std::vector<double> u(n, 0.0), v(d, 0.0);
        for (auto& e : u) { const double g = rng.standard_normal(), w = 0.5 + rng.standard_normal(); if (g > 0.8) e = w; }
        for (auto& e : v) { const double g = rng.standard_normal(), w = 0.5 + rng.standard_normal(); if (g > 0.5) e = w; }
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < d; ++j) x(i, j) += 100.0 * std::pow(0.3, f) * u[i] * v[j];
    }
    for (int j = 0; j < d; ++j) x(7, j) += 1.0 + 0.01 * j;
    std::vector<int64_t> indptr(1, 0);
    std::vector<int32_t> indices;
    std::vector<double> values;
    for (int i = 0; i < n; ++i) {
        for (int j = d - 1; j >= 0; --j)      // (descending: indices need not be sorted)
            if (x(i, j) != 0.0) { indices.push_back(j); values.push_back(x(i, j)); }
        indptr.push_back(int64_t(indices.size()));
    }
    CsrMatrix<double> sx(n, d, indptr, indices, values);
    CHECK(sx.nrows() == n && sx.ncols() == d && sx.nnz() == int64_t(values.size()) && sx.nnz() < int64_t(n) * d / 2);
    CHECK(sx.resident() == !fallback);

    auto dense = RandomizedPca<double>::with_seed(k, RNG_SEED);
    auto sparse = RandomizedPca<double>::with_seed(k, RNG_SEED);
    const Array2<double> yd = dense.fit_transform(x);
    const Array2<double> ys = sparse.fit_transform(sx);
    CHECK(sparse.kernel_path() == (fallback ? 0 : 1));
    const double s0 = dense.singular_values()[0];
    for (int j = 0; j < k; ++j) {
        const double s = sparse.singular_values()[j], s1 = dense.singular_values()[j];
        CHECK(fallback ? s == s1 : std::fabs(s - s1) <= 1e-9 * s0);
        for (int i = 0; i < d; ++i)
            CHECK(fallback ? sparse.components()(j, i) == dense.components()(j, i)
                           : std::fabs(sparse.components()(j, i) - dense.components()(j, i)) <= 1e-8);
        for (int i = 0; i < n; ++i) CHECK(fallback ? ys(i, j) == yd(i, j) : std::fabs(ys(i, j) - yd(i, j)) <= 1e-8 * s0);
    }
    for (int j = 0; j < d; ++j) CHECK(std::fabs(sparse.mean()[j] - dense.mean()[j]) <= 1e-12 * (1.0 + std::fabs(dense.mean()[j])));
    const Array2<double> ts = sparse.transform(sx), td = dense.transform(x);
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < k; ++j) {
            CHECK(std::fabs(ts(i, j) - td(i, j)) <= 1e-8 * s0);
            CHECK(std::fabs(ts(i, j) - ys(i, j)) <= 1e-7 * s0);
        }
    CHECK(sparse.explained_variance().size() == size_t(k) && sparse.inverse_transform(ts).ncols() == d);

    // the test aid: X^T . 1 minus the epilogue against plain loops
    std::vector<double> ones(size_t(n) * 2, 1.0), a(d), s = {2.0, -1.0};
    for (int j = 0; j < d; ++j) a[j] = 0.5 * j;
    const std::vector<double> g = sx.gemm(ones, 2, true, a, s);
    for (int j = 0; j < d; ++j) {
        double col = 0;
        for (int i = 0; i < n; ++i) col += x(i, j);
        CHECK(std::fabs(g[2 * j] - (col - a[j] * 2.0)) <= 1e-10 * (1.0 + std::fabs(col)));
        CHECK(std::fabs(g[2 * j + 1] - (col + a[j])) <= 1e-10 * (1.0 + std::fabs(col)));
    }

    // the error messages
    std::vector<int64_t> bad = indptr;
    bad[5] = bad[4] - 1;
    CHECK(message_of([&] { CsrMatrix<double> m(n, d, bad, indices, values); }).find("indptr[5]") != std::string::npos);
    std::vector<int32_t> wild = indices;
    wild[11] = d;
    CHECK(message_of([&] { CsrMatrix<double> m(n, d, indptr, wild, values); }).find("indices[11] = 40 is outside [0, 40)") != std::string::npos);
    CHECK(message_of([&] { CsrMatrix<double> m(n + 1, d, indptr, indices, values); }).find("indptr should have") != std::string::npos);
    CsrMatrix<double> narrow(n, d + 1, indptr, indices, values);
    CHECK(message_of([&] { sparse.transform(narrow); }).find("# of columns should be 40") != std::string::npos);
    auto big = RandomizedPca<double>::with_seed(d + 2, RNG_SEED);
    CHECK(message_of([&] { big.fit(sx); }).find("every dimension should be at least 42") != std::string::npos);

    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("sparse facade tests passed (%s)\n", fallback ? "fallback" : "kernel");
    return 0;
}

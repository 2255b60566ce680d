// Nmf on sparse input in the C++ facade (include/petal_decomposition.hpp over petal_hip_nmf_sparse.h): a custom-init fit of a 60 x 40
// CsrMatrix (one fully dense row, an empty row, an empty column) against dense Nmf on the same matrix, fit_transform's W, transform of
// sparse query rows by the CSR-fitted and by the dense-fitted model, the random initialisation, kernel_path and the errors.
//   nmf_sparse_facade_tests kernel      the library has k_nmf_sweep (libpetal_hip.so): kernel_path 1, the dense results within 1e-9
//   nmf_sparse_facade_tests fallback    it has not (the host simulation): kernel_path 0, the dense results bit for bit
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

template <class M>
static double rel_diff(const M& a, const M& b) {
    double num = 0, den = 0;
    CHECK(a.data.size() == b.data.size());
    for (size_t i = 0; i < a.data.size() && i < b.data.size(); ++i) {
        num = std::fmax(num, std::fabs(double(a.data[i]) - double(b.data[i])));
        den = std::fmax(den, std::fabs(double(b.data[i])));
    }
    return den > 0 ? num / den : num;
}

struct Triple {
    std::vector<int64_t> indptr;
    std::vector<int32_t> indices;
    std::vector<double> values;
};
static Triple to_csr(const Array2<double>& x) {
    Triple t;
    t.indptr.push_back(0);
    for (int64_t i = 0; i < x.nrows(); ++i) {
        for (int64_t j = x.ncols() - 1; j >= 0; --j)             // (unsorted inside the row: descending)
            if (x(i, j) != 0) { t.indices.push_back(int32_t(j)); t.values.push_back(x(i, j)); }
        t.indptr.push_back(int64_t(t.indices.size()));
    }
    return t;
}

int main(int argc, char** argv) {
    const bool fallback = argc > 1 && std::strcmp(argv[1], "fallback") == 0;
    const int n = 60, d = 40, k = 3, m = 7, iters = 5;
    Pcg rng((unsigned __int128)1234567891011121314ull + 39);
    Array2<double> x(n, d), xq(m, d), w0(n, k), h0(k, d);
    for (int i = 0; i < n + m; ++i) {
        double f[3];
        for (int t = 0; t < 3; ++t) f[t] = std::fabs(rng.standard_normal());
        for (int j = 0; j < d; ++j) {
            double v = 0.02 * std::fabs(rng.standard_normal());
            for (int t = 0; t < 3; ++t) v += f[t] * (1.0 + std::sin(0.9 * (t + 1) * j + 0.3 * t));
            const bool keep = std::fabs(rng.standard_normal()) < 0.4 || i == 2;      // about 30 % stored; row 2 fully dense
            (i < n ? x(i, j) : xq(i - n, j)) = (keep && j != 7 && i != 5 && i != n + 1) ? v : 0.0;   // column 7, row 5 and query row 1 empty
        }
    }
    for (auto& v : w0.data) v = 0.5 * std::fabs(rng.standard_normal()) + 0.01;
    for (auto& v : h0.data) v = 0.5 * std::fabs(rng.standard_normal()) + 0.01;
    const Triple tx = to_csr(x), tq = to_csr(xq);
    Context ctx;
    {
        CsrMatrix<double> sx(n, d, tx.indptr, tx.indices, tx.values, &ctx), sq(m, d, tq.indptr, tq.indices, tq.values, &ctx);
        CHECK(sx.resident() == !fallback);
        Nmf<double> sparse(k, iters, 0.0, 0, 0.0, -1.0, 0.0, &ctx), dense(k, iters, 0.0, 0, 0.0, -1.0, 0.0, &ctx);
        const Array2<double> ws = sparse.fit_transform(sx, w0, h0), wd = dense.fit_transform(x, w0, h0);
        CHECK(sparse.kernel_path() == (fallback ? 0 : 1));
        const NmfInfo in = sparse.info();
        CHECK(in.n == n && in.d == d && in.k == k && in.n_iter == iters && in.transform_kernel == -1);
        CHECK(fallback || in.fit_kernel);
        const double tol = fallback ? 0.0 : 1e-9;
        CHECK(rel_diff(ws, wd) <= tol);
        CHECK(rel_diff(sparse.components(), dense.components()) <= tol);
        CHECK(std::fabs(sparse.reconstruction_err() - dense.reconstruction_err()) <= tol * dense.reconstruction_err());
        bool empty_row = true;
        for (int p = 0; p < k; ++p) empty_row = empty_row && ws(5, p) == 0.0;
        CHECK(empty_row);
        // fit (without W) gives the same model
        Nmf<double> again(k, iters, 0.0, 0, 0.0, -1.0, 0.0, &ctx);
        again.fit(sx, w0, h0);
        CHECK(rel_diff(again.components(), sparse.components()) == 0.0);
        // transform: sparse rows by both models, dense rows by the CSR-fitted model
        const Array2<double> want = dense.transform(xq);
        const Array2<double> t1 = sparse.transform(sq);
        CHECK(sparse.kernel_path() == (fallback ? 0 : 1) && sparse.info().transform_kernel == (fallback ? 0 : 1));
        const Array2<double> t2 = dense.transform(sq), t3 = sparse.transform(xq);
        CHECK(dense.kernel_path() == (fallback ? 0 : 1));
        CHECK(rel_diff(t1, want) <= tol && rel_diff(t2, want) <= tol && rel_diff(t3, want) <= tol);
        CHECK(t1.nrows() == m && t1.ncols() == k);
        CHECK(rel_diff(sparse.inverse_transform(t1), dense.inverse_transform(t1)) <= tol);
        // random initialisation: one seed, one stream, dense or sparse
        Nmf<double> r1(k, 2, 0.0, 77, 0.0, -1.0, 0.0, &ctx), r2(k, 2, 0.0, 77, 0.0, -1.0, 0.0, &ctx), r3(k, 2, 0.0, 78, 0.0, -1.0, 0.0, &ctx);
        const Array2<double> a1 = r1.fit_transform(sx), a2 = r2.fit_transform(x), a3 = r3.fit_transform(sx);
        CHECK(rel_diff(a1, a2) <= tol && rel_diff(a1, a3) > 1e-3);
        // the forced fall-back: the dense fit, bit for bit
        ctx.set_option(PETAL_OPT_NMF_FALLBACK, 1.0);
        Nmf<double> f1(k, iters, 0.0, 0, 0.0, -1.0, 0.0, &ctx), f2(k, iters, 0.0, 0, 0.0, -1.0, 0.0, &ctx);
        const Array2<double> b1 = f1.fit_transform(sx, w0, h0), b2 = f2.fit_transform(x, w0, h0);
        ctx.set_option(PETAL_OPT_NMF_FALLBACK, 0.0);
        CHECK(f1.kernel_path() == 0 && rel_diff(b1, b2) == 0.0 && rel_diff(f1.components(), f2.components()) == 0.0);
        CHECK(rel_diff(b1, ws) <= 1e-9);
        // float32 data
        std::vector<float> v32(tx.values.begin(), tx.values.end());
        Array2<float> x32(n, d), w32(n, k), h32(k, d);
        for (size_t i = 0; i < x.data.size(); ++i) x32.data[i] = float(x.data[i]);
        for (size_t i = 0; i < w0.data.size(); ++i) w32.data[i] = float(w0.data[i]);
        for (size_t i = 0; i < h0.data.size(); ++i) h32.data[i] = float(h0.data[i]);
        CsrMatrix<float> s32(n, d, tx.indptr, tx.indices, v32, &ctx);
        Nmf<float> n32(k, iters, 0.0, 0, 0.0, -1.0, 0.0, &ctx), d32(k, iters, 0.0, 0, 0.0, -1.0, 0.0, &ctx);
        const Array2<float> ws32 = n32.fit_transform(s32, w32, h32), wd32 = d32.fit_transform(x32, w32, h32);
        CHECK(rel_diff(ws32, wd32) <= (fallback ? 0.0 : 1e-5) && n32.kernel_path() == (fallback ? 0 : 1));
        // errors
        auto throws = [&](auto&& fn, const char* text) {
            try {
                fn();
            } catch (const DecompositionError& e) {
                return std::string(e.what()).find(text) != std::string::npos;
            }
            return false;
        };
        CHECK(throws([&] { Nmf<double>(41, 2, 0.0, 0, 0.0, -1.0, 0.0, &ctx).fit(sx); }, "every dimension should be at least 41"));
        CHECK(throws([&] { Nmf<double>(k, 2, 0.0, 0, 0.0, -1.0, 0.0, &ctx).transform(sq); }, "not been fitted"));
        Triple neg = tx;
        neg.values[3] = -1.0;
        CsrMatrix<double> sneg(n, d, neg.indptr, neg.indices, neg.values, &ctx);
        CHECK(throws([&] { Nmf<double>(k, 2, 0.0, 0, 0.0, -1.0, 0.0, &ctx).fit(sneg); }, "negative values in data"));
        Array2<double> xn(m, d - 1);
        const Triple tn = to_csr(xn);
        CsrMatrix<double> snarrow(m, d - 1, tn.indptr, tn.indices, tn.values, &ctx);
        CHECK(throws([&] { sparse.transform(snarrow); }, "# of columns should be 40"));
    }
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("nmf sparse facade tests passed (%s)\n", fallback ? "fallback" : "kernel");
    return 0;
}

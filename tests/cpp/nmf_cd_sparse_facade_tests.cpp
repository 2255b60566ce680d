// Nmf with the coordinate-descent solver on sparse CSR data in the C++ facade (include/petal_decomposition.hpp over
// petal_hip_nmf_cd_sparse.h): Nmf<A>::sparse_path(NmfSparsePath::Sweep) on the CsrMatrix overloads.  A custom-init fit of a 60 x 40
// matrix with empty rows against a plain restatement of the header's sweep on the dense image, fit_transform's W, transform from
// W = 0, the stopping rule, the densifying fall-back against the dense solver byte for byte, the random initialisation, float32 data,
// what the default still refuses and what the multiplicative solver still gives, and the C entries.
//   nmf_cd_sparse_facade_tests kernel    the library has k_nmf_cd_sweep (libpetal_hip.so): kernel_path 1
//   nmf_cd_sparse_facade_tests host      it has not (the host simulation): kernel_path 0, every call densifies
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

template <class M, class N>
static double rel_diff(const M& a, const N& b) {
    double num = 0, den = 0;
    CHECK(a.data.size() == b.data.size());
    for (size_t i = 0; i < a.data.size() && i < b.data.size(); ++i) {
        num = std::fmax(num, std::fabs(double(a.data[i]) - double(b.data[i])));
        den = std::fmax(den, std::fabs(double(b.data[i])));
    }
    return den > 0 ? num / den : num;
}

static Array2<double> transposed(const Array2<double>& a) {
    Array2<double> t(a.ncols(), a.nrows());
    for (int64_t i = 0; i < a.nrows(); ++i)
        for (int64_t j = 0; j < a.ncols(); ++j) t(j, i) = a(i, j);
    return t;
}

// one sweep of every row of w with S = f f^T + l2 I and z = x f^T - l1 (f: k x d); returns the violation
static double sweep(const Array2<double>& x, Array2<double>& w, const Array2<double>& f, double l1, double l2) {
    const int64_t n = x.nrows(), d = x.ncols(), k = f.nrows();
    std::vector<double> s(size_t(k * k), 0.0), z(static_cast<size_t>(k), 0.0);
    for (int64_t p = 0; p < k; ++p)
        for (int64_t r = 0; r < k; ++r) {
            for (int64_t j = 0; j < d; ++j) s[size_t(p * k + r)] += f(p, j) * f(r, j);
            if (p == r) s[size_t(p * k + r)] += l2;
        }
    double viol = 0;
    for (int64_t i = 0; i < n; ++i) {
        for (int64_t p = 0; p < k; ++p) {
            z[size_t(p)] = -l1;
            for (int64_t j = 0; j < d; ++j) z[size_t(p)] += x(i, j) * f(p, j);
        }
        for (int64_t t = 0; t < k; ++t) {
            double grad = -z[size_t(t)];
            for (int64_t r = 0; r < k; ++r) grad += s[size_t(t * k + r)] * w(i, r);
            viol += std::fabs(w(i, t) == 0 ? std::fmin(0.0, grad) : grad);
            if (s[size_t(t * k + t)] != 0) w(i, t) = std::fmax(w(i, t) - grad / s[size_t(t * k + t)], 0.0);
        }
    }
    return viol;
}

template <class A>
static CsrMatrix<A> compress(const Array2<double>& x, Context* ctx) {
    std::vector<int64_t> indptr(size_t(x.nrows() + 1), 0);
    std::vector<int32_t> indices;
    std::vector<A> values;
    for (int64_t i = 0; i < x.nrows(); ++i) {
        for (int64_t j = 0; j < x.ncols(); ++j)
            if (x(i, j) != 0) { indices.push_back(int32_t(j)); values.push_back(A(x(i, j))); }
        indptr[size_t(i + 1)] = int64_t(indices.size());
    }
    return CsrMatrix<A>(x.nrows(), x.ncols(), indptr, indices, values, ctx);
}

int main(int argc, char** argv) {
    const bool host = argc > 1 && std::strcmp(argv[1], "host") == 0;
    const int n = 60, d = 40, k = 3, m = 7, iters = 5;
    Pcg rng((unsigned __int128)1234567891011121314ull + 53);
    Array2<double> x(n, d), xq(m, d), w0(n, k), h0(k, d);
    for (int i = 0; i < n + m; ++i) {
        double f[3];
        for (int t = 0; t < 3; ++t) f[t] = std::fabs(rng.standard_normal());
        for (int j = 0; j < d; ++j) {
            double v = 0.02 * std::fabs(rng.standard_normal());
            for (int t = 0; t < 3; ++t) v += f[t] * (1.0 + std::sin(0.9 * (t + 1) * j + 0.3 * t));
            const bool keep = rng.standard_normal() > 0.5 || j == 4 || i == 2;   // about 30 %, a dense row and a dense column
            (i < n ? x(i, j) : xq(i - n, j)) = keep ? v : 0.0;
        }
    }
    for (int j = 0; j < d; ++j) { xq(3, j) = 0.0; if (j != 4) x(11, j) = 0.0; }   // an empty query row, a row with one entry
    for (auto& v : w0.data) v = 0.5 * std::fabs(rng.standard_normal()) + 0.01;
    for (auto& v : h0.data) v = 0.5 * std::fabs(rng.standard_normal()) + 0.01;
    const double alpha = 0.01, rho = 0.5;
    const double l1w = d * alpha * rho, l2w = d * alpha * (1 - rho), l1h = n * alpha * rho, l2h = n * alpha * (1 - rho);
    // the reference: `iters` iterations "W sweep, then H sweep with the new W" (the H sweep is the W sweep of the transposed problem)
    Array2<double> wr = w0, hr = h0;
    const Array2<double> xt = transposed(x);
    std::vector<double> viol;
    for (int it = 0; it < iters; ++it) {
        double v = sweep(x, wr, hr, l1w, l2w);
        Array2<double> ht = transposed(hr);
        v += sweep(xt, ht, transposed(wr), l1h, l2h);
        hr = transposed(ht);
        viol.push_back(v);
    }
    Context ctx;
    {
        CsrMatrix<double> sx = compress<double>(x, &ctx), sq = compress<double>(xq, &ctx);
        auto throws = [&](auto&& fn, const char* text) {
            try {
                fn();
            } catch (const DecompositionError& e) {
                return std::string(e.what()).find(text) != std::string::npos;
            }
            return false;
        };
        Nmf<double> cd(k, iters, 0.0, 0, alpha, -1.0, rho, &ctx);
        CHECK(cd.sparse_path() == NmfSparsePath::Refuse);
        cd.solver(NmfSolver::CoordinateDescent);
        // the default still refuses
        CHECK(throws([&] { cd.fit(sx, w0, h0); }, "does not take a CsrMatrix"));
        cd.sparse_path(NmfSparsePath::Sweep);
        CHECK(cd.sparse_path() == NmfSparsePath::Sweep);
        const Array2<double> w = cd.fit_transform(sx, w0, h0);
        CHECK(cd.kernel_path() == (host ? 0 : 1));
        CHECK(cd.model_solver() == NmfSolver::CoordinateDescent && cd.model_loss() == NmfLoss::Frobenius);
        const NmfInfo in = cd.info();
        CHECK(in.n == n && in.d == d && in.k == k && in.n_iter == iters && in.transform_kernel == -1 && in.fit_kernel == !host);
        CHECK(rel_diff(w, wr) <= 1e-9);
        CHECK(rel_diff(cd.components(), hr) <= 1e-9);
        CHECK(cd.reconstruction_err() > 0);
        // fit (without W) gives the same model
        Nmf<double> again(k, iters, 0.0, 0, alpha, -1.0, rho, &ctx);
        again.solver(NmfSolver::CoordinateDescent).sparse_path(NmfSparsePath::Sweep).fit(sx, w0, h0);
        CHECK(rel_diff(again.components(), cd.components()) == 0.0);
        // transform: from W = 0, `iters` sweeps with the fit's l1_w, l2_w; the empty row stays at zero; the dense transform agrees
        Array2<double> tw(m, k);
        for (auto& v : tw.data) v = 0.0;
        for (int it = 0; it < iters; ++it) sweep(xq, tw, cd.components(), l1w, l2w);
        const Array2<double> t1 = cd.transform(sq);
        CHECK(cd.kernel_path() == (host ? 0 : 1) && cd.info().transform_kernel == (host ? 0 : 1));
        CHECK(rel_diff(t1, tw) <= 1e-9 && t1.nrows() == m && t1.ncols() == k);
        CHECK(t1(3, 0) == 0.0 && t1(3, 1) == 0.0 && t1(3, 2) == 0.0);
        CHECK(rel_diff(cd.transform(xq), tw) <= 1e-9);
        CHECK(cd.inverse_transform(t1).ncols() == d);
        // a model fitted dense transforms a CsrMatrix under Sweep, and is refused without
        Nmf<double> dense(k, iters, 0.0, 0, alpha, -1.0, rho, &ctx);
        dense.solver(NmfSolver::CoordinateDescent).fit(x, w0, h0);
        CHECK(throws([&] { dense.transform(sq); }, "does not take CSR input"));
        dense.sparse_path(NmfSparsePath::Sweep);
        Array2<double> td(m, k);
        for (auto& v : td.data) v = 0.0;
        for (int it = 0; it < iters; ++it) sweep(xq, td, dense.components(), l1w, l2w);
        CHECK(rel_diff(dense.transform(sq), td) <= 1e-9);
        // the stopping rule: a tolerance between the ratios of two iterations stops at the first iteration at or below it
        int rules = 0;
        for (int cut = 1; cut + 1 < iters; ++cut) {
            const double tol = std::sqrt(viol[size_t(cut)] / viol[0] * (viol[size_t(cut) + 1] / viol[0]));
            int expect = iters;
            bool decided = true;
            for (int it = iters - 1; it >= 0; --it) {
                const double r = viol[size_t(it)] / viol[0];
                if (r <= tol) expect = it + 1;
                decided = decided && std::fabs(r - tol) >= 0.01 * tol;
            }
            if (!decided) continue;   // (a ratio within 1 % of this tolerance: not a case for the rule)
            Nmf<double> s1(k, iters, tol, 0, alpha, -1.0, rho, &ctx);
            s1.solver(NmfSolver::CoordinateDescent).sparse_path(NmfSparsePath::Sweep).fit(sx, w0, h0);
            CHECK(s1.n_iter() == expect);
            ++rules;
        }
        CHECK(rules >= 2);
        // under the multiplicative solver the keyword changes nothing
        Nmf<double> mu(k, iters, 0.0, 0, alpha, -1.0, rho, &ctx), mu2(k, iters, 0.0, 0, alpha, -1.0, rho, &ctx);
        mu2.sparse_path(NmfSparsePath::Sweep);
        const Array2<double> wm = mu.fit_transform(sx, w0, h0), wm2 = mu2.fit_transform(sx, w0, h0);
        CHECK(mu2.model_solver() == NmfSolver::MultiplicativeUpdate && rel_diff(wm, wm2) == 0.0 && rel_diff(wm, w) > 1e-6);
        CHECK(rel_diff(mu.transform(sq), mu2.transform(sq)) == 0.0);
        // random initialisation: one seed, one stream
        Nmf<double> r1(k, 2, 0.0, 77, 0.0, -1.0, 0.0, &ctx), r2b(k, 2, 0.0, 77, 0.0, -1.0, 0.0, &ctx), r3b(k, 2, 0.0, 78, 0.0, -1.0, 0.0, &ctx);
        r1.solver(NmfSolver::CoordinateDescent).sparse_path(NmfSparsePath::Sweep);
        r2b.solver(NmfSolver::CoordinateDescent).sparse_path(NmfSparsePath::Sweep);
        r3b.solver(NmfSolver::CoordinateDescent).sparse_path(NmfSparsePath::Sweep);
        const Array2<double> a1 = r1.fit_transform(sx), a2 = r2b.fit_transform(sx), a3 = r3b.fit_transform(sx);
        CHECK(rel_diff(a1, a2) == 0.0 && rel_diff(a1, a3) > 1e-3);
        // the forced fall-back densifies: byte for byte the dense solver, within the parity bar of the sweep
        ctx.set_option(PETAL_OPT_NMF_FALLBACK, 1.0);
        Nmf<double> f1(k, iters, 0.0, 0, alpha, -1.0, rho, &ctx), f2(k, iters, 0.0, 0, alpha, -1.0, rho, &ctx);
        f1.solver(NmfSolver::CoordinateDescent).sparse_path(NmfSparsePath::Sweep);
        f2.solver(NmfSolver::CoordinateDescent);
        const Array2<double> b1 = f1.fit_transform(sx, w0, h0), b2 = f2.fit_transform(x, w0, h0);
        const int64_t path = f1.kernel_path();
        const Array2<double> q1 = f1.transform(sq), q2 = f2.transform(xq);
        ctx.set_option(PETAL_OPT_NMF_FALLBACK, 0.0);
        CHECK(path == 0 && rel_diff(b1, b2) == 0.0 && rel_diff(f1.components(), f2.components()) == 0.0 && rel_diff(q1, q2) == 0.0);
        CHECK(rel_diff(b1, w) <= 1e-9 && rel_diff(f1.components(), cd.components()) <= 1e-9);
        // float32 data
        Array2<float> w32(n, k), h32(k, d);
        for (size_t i = 0; i < w0.data.size(); ++i) w32.data[i] = float(w0.data[i]);
        for (size_t i = 0; i < h0.data.size(); ++i) h32.data[i] = float(h0.data[i]);
        CsrMatrix<float> sx32 = compress<float>(x, &ctx);
        Nmf<float> n32(k, iters, 0.0, 0, alpha, -1.0, rho, &ctx);
        n32.solver(NmfSolver::CoordinateDescent).sparse_path(NmfSparsePath::Sweep);
        const Array2<float> ws32 = n32.fit_transform(sx32, w32, h32);
        CHECK(rel_diff(ws32, wr) <= 1e-4 && n32.kernel_path() == (host ? 0 : 1));
        // errors
        CHECK(throws([&] {
            Nmf<double> b(k, 2, 0.0, 0, 0.0, -1.0, 0.0, &ctx);
            b.solver(NmfSolver::CoordinateDescent).sparse_path(NmfSparsePath::Sweep).loss(NmfLoss::KullbackLeibler).fit(sx);
        }, "does not take the kullback-leibler loss"));
        CHECK(throws([&] {
            Nmf<double> b(41, 2, 0.0, 0, 0.0, -1.0, 0.0, &ctx);
            b.solver(NmfSolver::CoordinateDescent).sparse_path(NmfSparsePath::Sweep).fit(sx);
        }, "every dimension should be at least 41"));
        // the C entries: an unknown solver; solver 0 is petal_nmf_fit_csr; petal_nmf_transform_csr still refuses a solver-1 handle
        {
            petal_nmf_spec spec{};
            spec.max_iter = 2;
            petal_matrix m0 = w0.view(), m1 = h0.view();
            petal_nmf* none = nullptr;
            CHECK(petal_nmf_fit_csr_solver(ctx.get(), sx.get(), k, &spec, 2, &m0, &m1, 0, &none, nullptr, nullptr) == PETAL_INVALID_INPUT);
            CHECK(throws([&] { ctx.check(PETAL_INVALID_INPUT); }, "unknown solver"));
            CHECK(none == nullptr);
            petal_nmf *ha = nullptr, *hb = nullptr, *hc = nullptr;
            int64_t pa = -1, pb = -1;
            CHECK(petal_nmf_fit_csr_solver(ctx.get(), sx.get(), k, &spec, PETAL_NMF_SOLVER_MU, &m0, &m1, 0, &ha, nullptr, &pa) == PETAL_OK);
            CHECK(petal_nmf_fit_csr(ctx.get(), sx.get(), k, &spec, &m0, &m1, 0, &hb, nullptr, &pb) == PETAL_OK);
            Array2<double> ca(k, d), cb(k, d), ta(m, k), tb(m, k);
            int64_t sv = -1;
            CHECK(petal_nmf_get(ha, ca.data.data(), nullptr, nullptr) == PETAL_OK && petal_nmf_get(hb, cb.data.data(), nullptr, nullptr) == PETAL_OK);
            CHECK(pa == pb && std::memcmp(ca.data.data(), cb.data.data(), sizeof(double) * ca.data.size()) == 0);
            CHECK(petal_nmf_get_solver(ha, &sv) == PETAL_OK && sv == PETAL_NMF_SOLVER_MU);
            petal_matrix ma = ta.view(), mb = tb.view();
            CHECK(petal_nmf_transform_csr_solver(ctx.get(), ha, sq.get(), &ma, &pa) == PETAL_OK);
            CHECK(petal_nmf_transform_csr(ctx.get(), hb, sq.get(), &mb, &pb) == PETAL_OK);
            CHECK(pa == pb && std::memcmp(ta.data.data(), tb.data.data(), sizeof(double) * ta.data.size()) == 0);
            CHECK(petal_nmf_fit_csr_solver(ctx.get(), sx.get(), k, &spec, PETAL_NMF_SOLVER_CD, &m0, &m1, 0, &hc, nullptr, &pa) == PETAL_OK);
            CHECK(petal_nmf_get_solver(hc, &sv) == PETAL_OK && sv == PETAL_NMF_SOLVER_CD && pa == (host ? 0 : 1));
            CHECK(petal_nmf_transform_csr(ctx.get(), hc, sq.get(), &ma, &pa) == PETAL_INVALID_INPUT);
            CHECK(throws([&] { ctx.check(PETAL_INVALID_INPUT); }, "does not take CSR input"));
            petal_nmf_destroy(ha);
            petal_nmf_destroy(hb);
            petal_nmf_destroy(hc);
        }
    }
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("nmf cd sparse facade tests passed (%s)\n", host ? "host" : "kernel");
    return 0;
}

// Nmf with the Kullback-Leibler loss on dense data in the C++ facade (include/petal_decomposition.hpp over petal_hip_nmf_kl_dense.h):
// Nmf<A>::dense_path(NmfDensePath::Fused) sends an Array2 to the fused dense pass.  A custom-init fit of a 60 x 40 matrix (about 30 %
// non-zero, one fully dense row, an empty row, an empty column) against a plain restatement of the header's updates, fit_transform's W,
// transform of dense and of CSR query rows, a CSR-fitted model on dense rows, kernel_path, the forced composed path, the random
// initialisation, and the errors (without dense_path(Fused) the dense overloads still throw under this loss).
//   nmf_kl_dense_facade_tests kernel    the library has k_nmf_kl_pass (libpetal_hip.so): kernel_path 1
//   nmf_kl_dense_facade_tests host      it has not (the host simulation): kernel_path 0, the composed path
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

struct Triple {
    std::vector<int64_t> indptr;
    std::vector<int32_t> indices;
    std::vector<double> values;
};
static Triple to_csr(const Array2<double>& x) {
    Triple t;
    t.indptr.push_back(0);
    for (int64_t i = 0; i < x.nrows(); ++i) {
        for (int64_t j = 0; j < x.ncols(); ++j)
            if (x(i, j) != 0) { t.indices.push_back(int32_t(j)); t.values.push_back(x(i, j)); }
        t.indptr.push_back(int64_t(t.indices.size()));
    }
    return t;
}

static const double EPS = 1.1920928955078125e-07;

// W <- W o ((X / (W H)) H^T) / rowsum(H), `updates` times
static void update_w(const Array2<double>& x, Array2<double>& w, const Array2<double>& h, int updates) {
    const int64_t n = x.nrows(), d = x.ncols(), k = h.nrows();
    std::vector<double> c(static_cast<size_t>(k), 0.0), num(static_cast<size_t>(k));
    for (int64_t p = 0; p < k; ++p)
        for (int64_t j = 0; j < d; ++j) c[p] += h(p, j);
    for (int u = 0; u < updates; ++u)
        for (int64_t i = 0; i < n; ++i) {
            std::fill(num.begin(), num.end(), 0.0);
            for (int64_t j = 0; j < d; ++j) {
                double wh = 0;
                for (int64_t p = 0; p < k; ++p) wh += w(i, p) * h(p, j);
                if (wh < EPS) wh = EPS;
                for (int64_t p = 0; p < k; ++p) num[p] += x(i, j) / wh * h(p, j);
            }
            for (int64_t p = 0; p < k; ++p) w(i, p) *= num[p] / (c[p] == 0 ? EPS : c[p]);
        }
}
static Array2<double> transposed(const Array2<double>& a) {
    Array2<double> t(a.ncols(), a.nrows());
    for (int64_t i = 0; i < a.nrows(); ++i)
        for (int64_t j = 0; j < a.ncols(); ++j) t(j, i) = a(i, j);
    return t;
}

int main(int argc, char** argv) {
    const bool host = argc > 1 && std::strcmp(argv[1], "host") == 0;
    const int path = host ? 0 : 1;
    const int n = 60, d = 40, k = 3, m = 7, iters = 5;
    Pcg rng((unsigned __int128)1234567891011121314ull + 43);
    Array2<double> x(n, d), xq(m, d), w0(n, k), h0(k, d);
    for (int i = 0; i < n + m; ++i) {
        double f[3];
        for (int t = 0; t < 3; ++t) f[t] = std::fabs(rng.standard_normal());
        for (int j = 0; j < d; ++j) {
            double v = 0.02 * std::fabs(rng.standard_normal());
            for (int t = 0; t < 3; ++t) v += f[t] * (1.0 + std::sin(0.9 * (t + 1) * j + 0.3 * t));
            const bool keep = std::fabs(rng.standard_normal()) < 0.4 || i == 2;      // about 30 % non-zero; row 2 fully dense
            (i < n ? x(i, j) : xq(i - n, j)) = (keep && j != 7 && i != 5 && i != n + 1) ? v : 0.0;   // column 7, row 5 and query row 1 empty
        }
    }
    for (auto& v : w0.data) v = 0.5 * std::fabs(rng.standard_normal()) + 0.01;
    for (auto& v : h0.data) v = 0.5 * std::fabs(rng.standard_normal()) + 0.01;
    // the reference: `iters` iterations "new W, then H with the new W" (the H update is the W update of the transposed problem)
    Array2<double> wr = w0, hr = h0;
    const Array2<double> xt = transposed(x);
    for (int it = 0; it < iters; ++it) {
        update_w(x, wr, hr, 1);
        Array2<double> ht = transposed(hr);
        update_w(xt, ht, transposed(wr), 1);
        hr = transposed(ht);
    }
    Context ctx;
    {
        Nmf<double> kl(k, iters, 0.0, 0, 0.0, -1.0, 0.0, &ctx);
        kl.loss(NmfLoss::KullbackLeibler).dense_path(NmfDensePath::Fused);
        CHECK(kl.dense_path() == NmfDensePath::Fused);
        const Array2<double> w = kl.fit_transform(x, w0, h0);
        CHECK(kl.kernel_path() == path && kl.model_loss() == NmfLoss::KullbackLeibler);
        const NmfInfo in = kl.info();
        CHECK(in.n == n && in.d == d && in.k == k && in.n_iter == iters && in.transform_kernel == -1 && in.fit_kernel == !host);
        CHECK(rel_diff(w, wr) <= 1e-9);
        CHECK(rel_diff(kl.components(), hr) <= 1e-9);
        CHECK(kl.reconstruction_err() > 0);
        bool empty_row = true;
        for (int p = 0; p < k; ++p) empty_row = empty_row && w(5, p) == 0.0;
        CHECK(empty_row);
        // fit (without W) gives the same model
        Nmf<double> again(k, iters, 0.0, 0, 0.0, -1.0, 0.0, &ctx);
        again.loss(NmfLoss::KullbackLeibler).dense_path(NmfDensePath::Fused).fit(x, w0, h0);
        CHECK(rel_diff(again.components(), kl.components()) == 0.0);
        // transform: `iters` updates from the constant sqrt(mean(xq) / k), dense rows and CSR rows
        double mean = 0;
        for (double v : xq.data) mean += v;
        mean /= double(xq.data.size());
        Array2<double> tw(m, k);
        for (auto& v : tw.data) v = std::sqrt(mean / k);
        update_w(xq, tw, kl.components(), iters);
        const Array2<double> t1 = kl.transform(xq);
        CHECK(kl.kernel_path() == path && kl.info().transform_kernel == path);
        CHECK(rel_diff(t1, tw) <= 1e-9 && t1.nrows() == m && t1.ncols() == k);
        CHECK(t1(1, 0) == 0.0 && t1(1, 1) == 0.0 && t1(1, 2) == 0.0);
        CHECK(kl.inverse_transform(t1).ncols() == d);
        const Triple tx = to_csr(x), tq = to_csr(xq);
        CsrMatrix<double> sx(n, d, tx.indptr, tx.indices, tx.values, &ctx), sq(m, d, tq.indptr, tq.indices, tq.values, &ctx);
        CHECK(rel_diff(kl.transform(sq), t1) <= 1e-9);
        // a model fitted on CSR transforms dense rows through the new entry
        Nmf<double> sp(k, iters, 0.0, 0, 0.0, -1.0, 0.0, &ctx);
        sp.loss(NmfLoss::KullbackLeibler).fit(sx, w0, h0);
        CHECK(rel_diff(sp.components(), kl.components()) <= 1e-9);
        sp.dense_path(NmfDensePath::Fused);
        CHECK(rel_diff(sp.transform(xq), t1) <= 1e-9 && sp.kernel_path() == path);
        // under the Frobenius loss the route changes nothing
        Nmf<double> fro(k, iters, 0.0, 0, 0.0, -1.0, 0.0, &ctx), fro2(k, iters, 0.0, 0, 0.0, -1.0, 0.0, &ctx);
        fro2.dense_path(NmfDensePath::Fused);
        const Array2<double> wf = fro.fit_transform(x, w0, h0), wf2 = fro2.fit_transform(x, w0, h0);
        CHECK(fro2.model_loss() == NmfLoss::Frobenius && rel_diff(wf, wf2) == 0.0 && rel_diff(wf, w) > 1e-6);
        CHECK(rel_diff(fro.transform(xq), fro2.transform(xq)) == 0.0);
        // random initialisation: one seed, one stream
        Nmf<double> r1(k, 2, 0.0, 77, 0.0, -1.0, 0.0, &ctx), r2(k, 2, 0.0, 77, 0.0, -1.0, 0.0, &ctx), r3(k, 2, 0.0, 78, 0.0, -1.0, 0.0, &ctx);
        r1.loss(NmfLoss::KullbackLeibler).dense_path(NmfDensePath::Fused);
        r2.loss(NmfLoss::KullbackLeibler).dense_path(NmfDensePath::Fused);
        r3.loss(NmfLoss::KullbackLeibler).dense_path(NmfDensePath::Fused);
        const Array2<double> a1 = r1.fit_transform(x), a2 = r2.fit_transform(x), a3 = r3.fit_transform(x);
        CHECK(rel_diff(a1, a2) == 0.0 && rel_diff(a1, a3) > 1e-3);
        // the forced composed path, within the parity bar of the kernel
        ctx.set_option(PETAL_OPT_NMF_FALLBACK, 1.0);
        Nmf<double> f1(k, iters, 0.0, 0, 0.0, -1.0, 0.0, &ctx);
        f1.loss(NmfLoss::KullbackLeibler).dense_path(NmfDensePath::Fused);
        const Array2<double> b1 = f1.fit_transform(x, w0, h0);
        ctx.set_option(PETAL_OPT_NMF_FALLBACK, 0.0);
        CHECK(f1.kernel_path() == 0 && rel_diff(b1, w) <= 1e-9 && rel_diff(f1.components(), kl.components()) <= 1e-9);
        // float32 data
        Array2<float> x32(n, d), w32(n, k), h32(k, d);
        for (size_t i = 0; i < x.data.size(); ++i) x32.data[i] = float(x.data[i]);
        for (size_t i = 0; i < w0.data.size(); ++i) w32.data[i] = float(w0.data[i]);
        for (size_t i = 0; i < h0.data.size(); ++i) h32.data[i] = float(h0.data[i]);
        Nmf<float> n32(k, iters, 0.0, 0, 0.0, -1.0, 0.0, &ctx);
        n32.loss(NmfLoss::KullbackLeibler).dense_path(NmfDensePath::Fused);
        const Array2<float> ws32 = n32.fit_transform(x32, w32, h32);
        CHECK(rel_diff(ws32, wr) <= 1e-4 && n32.kernel_path() == path);
        // errors
        auto throws = [&](auto&& fn, const char* text) {
            try {
                fn();
            } catch (const DecompositionError& e) {
                return std::string(e.what()).find(text) != std::string::npos;
            }
            return false;
        };
        CHECK(throws([&] { Nmf<double> b(k, 2, 0.0, 0, 0.0, -1.0, 0.0, &ctx); b.loss(NmfLoss::KullbackLeibler).fit(x); }, "takes a CsrMatrix"));
        CHECK(throws([&] {
            Nmf<double> b(k, 2, 0.0, 0, 0.0, -1.0, 0.0, &ctx);
            b.loss(NmfLoss::KullbackLeibler).dense_path(NmfDensePath::Fused).dense_path(NmfDensePath::Compress).fit_transform(x, w0, h0);
        }, "takes a CsrMatrix"));
        CHECK(throws([&] { Nmf<double> b(41, 2, 0.0, 0, 0.0, -1.0, 0.0, &ctx); b.loss(NmfLoss::KullbackLeibler).dense_path(NmfDensePath::Fused).fit(x); },
                     "every dimension should be at least 41"));
        Array2<double> neg = x;
        neg(3, 4) = -1.0;
        CHECK(throws([&] { Nmf<double> b(k, 2, 0.0, 0, 0.0, -1.0, 0.0, &ctx); b.loss(NmfLoss::KullbackLeibler).dense_path(NmfDensePath::Fused).fit(neg); },
                     "negative values in data"));
        // the C entries: an unknown loss, and petal_nmf_transform still refuses a model of this loss
        {
            petal_nmf_spec spec{};
            spec.max_iter = 2;
            petal_matrix mx = x.view(), m0 = w0.view(), m1 = h0.view(), mq = xq.view();
            petal_nmf* hnd = nullptr;
            CHECK(petal_nmf_fit_loss(ctx.get(), &mx, k, &spec, PETAL_NMF_LOSS_KL, &m0, &m1, 0, &hnd, nullptr) == PETAL_OK);
            Array2<double> out(m, k);
            petal_matrix mo = out.view();
            CHECK(petal_nmf_transform(ctx.get(), hnd, &mq, &mo) == PETAL_INVALID_INPUT);
            CHECK(throws([&] { ctx.check(PETAL_INVALID_INPUT); }, "kullback-leibler"));
            CHECK(petal_nmf_transform_loss(ctx.get(), hnd, &mq, &mo) == PETAL_OK);
            petal_nmf* none = nullptr;
            CHECK(petal_nmf_fit_loss(ctx.get(), &mx, k, &spec, 7, &m0, &m1, 0, &none, nullptr) == PETAL_INVALID_INPUT);
            CHECK(throws([&] { ctx.check(PETAL_INVALID_INPUT); }, "unknown loss"));
            CHECK(none == nullptr);
            petal_nmf_destroy(hnd);
        }
    }
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("nmf kl dense facade tests passed (%s)\n", host ? "host" : "kernel");
    return 0;
}

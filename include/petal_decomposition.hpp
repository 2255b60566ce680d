// petal_decomposition.hpp -- header-only C++17 facade over the C ABI (petal_hip.h) with the reference crate's
// type and method names (petabi/petal-decomposition v0.9.0, src/lib.rs:17-18):
//
//   Pca / PcaBuilder                      src/pca.rs:41-283
//   RandomizedPca / RandomizedPcaBuilder  src/pca.rs:317-663
//   FastIca / FastIcaBuilder              src/ica.rs:41-308
//
// fit / transform / fit_transform / inverse_transform take and return `Array2<A>` (row-major, A = float | double),
// errors are thrown as `DecompositionError` with the crate's messages (src/lib.rs:22-28).  Models own their RNG and
// advance it on every fit like the crate (src/pca.rs:532, src/ica.rs:211); the default RNG is the crate's
// `Mcg128Xsl64` (rand_pcg) with a Ziggurat StandardNormal -- a restatement of un-vendored third-party code whose
// exact stream is NOT pinned by any reference test ("stream parity unpinned").
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "petal_hip.h"
#include "petal_hip_score.h"
#include "petal_hip_segments.h"
#include "petal_hip_sparse.h"
#include "petal_hip_ipca.h"
#include "petal_hip_wide.h"
#include "petal_hip_kpca.h"
#include "petal_hip_nmf.h"
#include "petal_hip_nmf_sparse.h"
#include "petal_hip_nmf_kl.h"
#include "petal_hip_nmf_kl_dense.h"
#include "petal_hip_nmf_cd.h"
#include "petal_hip_nmf_cd_sparse.h"

namespace petal_decomposition {

struct DecompositionError : std::runtime_error {
    enum Kind { InvalidInput, LinalgError } kind;
    DecompositionError(Kind k, const std::string& m)
        : std::runtime_error((k == InvalidInput ? "invalid matrix: " : "linear algerba operation failed: ") + m), kind(k) {}
};

template <class A> struct DTypeOf;
template <> struct DTypeOf<float> { static constexpr int value = PETAL_F32; };
template <> struct DTypeOf<double> { static constexpr int value = PETAL_F64; };

// minimal owned row-major matrix (ndarray::Array2)
template <class A>
struct Array2 {
    std::vector<A> data;
    int64_t rows = 0, cols = 0;
    Array2() = default;
    Array2(int64_t r, int64_t c, A v = A(0)) : data(size_t(r) * c, v), rows(r), cols(c) {}
    Array2(std::initializer_list<std::initializer_list<A>> init) {
        rows = int64_t(init.size());
        cols = rows ? int64_t(init.begin()->size()) : 0;
        for (auto& r : init) data.insert(data.end(), r.begin(), r.end());
    }
    A& operator()(int64_t i, int64_t j) { return data[size_t(i) * cols + j]; }
    const A& operator()(int64_t i, int64_t j) const { return data[size_t(i) * cols + j]; }
    int64_t nrows() const { return rows; }
    int64_t ncols() const { return cols; }
    petal_matrix view() const {
        return petal_matrix{const_cast<A*>(data.data()), rows, cols, cols, 1, DTypeOf<A>::value, PETAL_HOST};
    }
};

// ---- rand_pcg::Mcg128Xsl64 + rand_distr::StandardNormal (Ziggurat), restated ---------------------------------
class Pcg {  // rand_pcg::Mcg128Xsl64: state *= MULT; output = rotr64(hi ^ lo, state >> 122)
  public:
    // Mcg128Xsl64::new(state) / Pcg64Mcg::new (src/pca.rs:991): the state is forced odd
    explicit Pcg(unsigned __int128 state) : state_(state | 1) {}
    // SeedableRng::from_seed(seed.to_be_bytes()) as the crate's with_seed does (src/pca.rs:356-359, src/ica.rs:75-78):
    // rand_pcg reads the 16 seed bytes as a little-endian u128, i.e. the big-endian bytes of `seed` byte-swapped
    static Pcg from_seed_be_bytes(unsigned __int128 seed) {
        unsigned __int128 sw = 0;
        for (int i = 0; i < 16; ++i) sw |= ((seed >> (8 * i)) & 0xff) << (8 * (15 - i));
        return Pcg(sw);
    }
    uint64_t next_u64() {
        state_ *= (((unsigned __int128)0x2360ED051FC65DA4ull) << 64) | 0x4385DF649FCCF645ull;
        const unsigned rot = unsigned(state_ >> 122);
        const uint64_t x = uint64_t(state_ >> 64) ^ uint64_t(state_);
        return (x >> rot) | (x << ((64 - rot) & 63));
    }
    double next_f64() { return double(next_u64() >> 11) * (1.0 / 9007199254740992.0); }            // rand Standard: [0, 1)
    double next_f64_open01() { return double(next_u64() >> 12) * (1.0 / 4503599627370496.0) + (1.0 / 9007199254740992.0); }  // Open01
    // rand_distr::StandardNormal: the 256-layer Ziggurat (tables recomputed from the published recurrence)
    double standard_normal() {
        static const Tables t;
        for (;;) {
            const uint64_t bits = next_u64();
            const int i = int(bits & 0xff);
            // (bits >> 12) as the mantissa of a float in [2, 4), minus 3: u in [-1, 1)
            const double u = double(int64_t(bits >> 12)) * (2.0 / 4503599627370496.0) - 1.0;
            const double x = u * t.x[i];
            if (std::fabs(x) < t.x[i + 1]) return x;
            if (i == 0) {  // tail beyond R
                double xx = 1.0, yy = 0.0;
                while (-2.0 * yy < xx * xx) {
                    xx = std::log(next_f64_open01()) / Tables::R;
                    yy = std::log(next_f64_open01());
                }
                return u < 0 ? xx - Tables::R : Tables::R - xx;
            }
            if (t.f[i + 1] + (t.f[i] - t.f[i + 1]) * next_f64() < std::exp(-0.5 * x * x)) return x;
        }
    }

  private:
    struct Tables {
        static constexpr double R = 3.654152885361009;
        double x[257], f[257];
        Tables() {
            const double v = 0.00492867323399;  // area of each layer
            x[0] = v / std::exp(-0.5 * R * R);
            x[1] = R;
            for (int i = 2; i < 256; ++i) x[i] = std::sqrt(-2.0 * std::log(v / x[i - 1] + std::exp(-0.5 * x[i - 1] * x[i - 1])));
            x[256] = 0.0;
            for (int i = 0; i < 257; ++i) f[i] = std::exp(-0.5 * x[i] * x[i]);
        }
    };
    unsigned __int128 state_;
};

inline unsigned __int128 random_seed() {
    std::random_device rd;
    unsigned __int128 s = 0;
    for (int i = 0; i < 4; ++i) s = (s << 32) | rd();
    return s;
}

// one context per process / GPU, shared by the models (src: models are plain data, the ctx is the device handle)
class Context {
  public:
    explicit Context(int device = 0, void* stream = nullptr) {
        if (petal_ctx_create(device, stream, &ctx_) != PETAL_OK || !ctx_)
            throw DecompositionError(DecompositionError::LinalgError, "no usable gfx950 device (there is no CPU fallback)");
    }
    ~Context() { petal_ctx_destroy(ctx_); }
    Context(const Context&) = delete;
    Context& operator=(const Context&) = delete;
    petal_ctx* get() const { return ctx_; }
    void check(int rc) const {
        if (rc == PETAL_OK) return;
        const std::string msg = petal_last_error(ctx_);
        throw DecompositionError(rc == PETAL_INVALID_INPUT ? DecompositionError::InvalidInput : DecompositionError::LinalgError, msg);
    }
    static Context& global() { static Context c; return c; }
    // petal_ctx_set_option / petal_ctx_get_option with a PETAL_OPT_* number.  Added for PETAL_OPT_PCA_DUAL / PETAL_OPT_PCA_DUAL_FALLBACK
    // (petal_hip_wide.h), but GENERAL: every option of petal_hip.h and its extension headers goes through the same pair, as in the Python
    // Context.  An extension beyond the crate, which has no options.
    void set_option(int option, double value) { check(petal_ctx_set_option(ctx_, option, value)); }
    double get_option(int option) const {
        double v = 0;
        if (petal_ctx_get_option(ctx_, option, &v) != PETAL_OK) throw DecompositionError(DecompositionError::InvalidInput, "unknown ctx option");
        return v;
    }

  private:
    petal_ctx* ctx_ = nullptr;
};

namespace detail {
template <class A>
struct PcaState {  // src/pca.rs:41-51 / 317-329
    Array2<A> components;
    int64_t n_samples = 0;
    std::vector<A> means;
    A total_variance = A(0);
    std::vector<A> singular;
    bool centering = true;
    int64_t k = 0;
    Context* ctx = nullptr;
    Context& context() const { return ctx ? *ctx : Context::global(); }

    Array2<A> transform(const Array2<A>& input) const {  // src/pca.rs:726-750
        const int64_t d = int64_t(means.size());
        if (input.ncols() != d) throw DecompositionError(DecompositionError::InvalidInput, "# of columns should be " + std::to_string(d));
        Array2<A> y(input.nrows(), k);
        petal_matrix mx = input.view(), my = y.view();
        context().check(petal_transform(context().get(), &mx, components.data.data(), means.data(), k, d, centering, &my));
        return y;
    }
    Array2<A> inverse_transform(const Array2<A>& input) const {  // src/pca.rs:788-811
        const int64_t d = int64_t(means.size());
        if (input.ncols() != k) throw DecompositionError(DecompositionError::InvalidInput, "# of columns should be " + std::to_string(k));
        Array2<A> x(input.nrows(), d);
        petal_matrix my = input.view(), mx = x.view();
        context().check(petal_inverse_transform(context().get(), &my, components.data.data(), means.data(), k, d, centering, &mx));
        return x;
    }
    std::vector<A> explained_variance_ratio() const {  // src/pca.rs:101-105
        std::vector<A> r(singular.size());
        for (size_t i = 0; i < r.size(); ++i) r[i] = singular[i] * singular[i] / total_variance;
        return r;
    }
    // ---- scores of rows against the fitted model: an extension beyond the crate (petal_hip_score.h) ----
    std::vector<A> explained_variance() const {  // lambda_j = sigma_j^2 / (n_samples - 1)
        std::vector<A> r(singular.size());
        for (size_t i = 0; i < r.size(); ++i) r[i] = singular[i] * singular[i] / A(n_samples - 1);
        return r;
    }
    A noise_variance() const {  // mean variance of the min(n_samples, d) - k discarded directions (scikit-learn's definition)
        const int64_t rest = std::min<int64_t>(n_samples, int64_t(means.size())) - k;
        if (rest <= 0) return A(0);
        double kept = 0;
        for (const A s : singular) kept += double(s) * double(s);
        return A((double(total_variance) - kept) / double(n_samples - 1) / double(rest));
    }
    // n x 2: [residual, weighted] (weights: k values or empty = all ones), one pass over the input
    Array2<A> score_rows(const Array2<A>& input, const std::vector<A>& weights) const {
        const int64_t d = int64_t(means.size());
        if (input.ncols() != d) throw DecompositionError(DecompositionError::InvalidInput, "# of columns should be " + std::to_string(d));
        Array2<A> out(input.nrows(), 2);
        petal_matrix mx = input.view(), mo = out.view();
        context().check(petal_score_rows(context().get(), &mx, components.data.data(), means.data(), k, d, centering,
                                         weights.empty() ? nullptr : weights.data(), &mo, nullptr));
        return out;
    }
    std::vector<A> inverse_variances() const {
        std::vector<A> w = explained_variance();
        for (A& v : w) {
            if (!(v > A(0))) throw DecompositionError(DecompositionError::InvalidInput, "a kept component has zero variance");
            v = A(1) / v;
        }
        return w;
    }
    std::vector<A> reconstruction_error(const Array2<A>& input) const {  // |xc|^2 - |xc V^T|^2: rounding noise below ~1e-5 |xc|^2 in float
        const Array2<A> sc = score_rows(input, {});
        std::vector<A> r(size_t(sc.nrows()));
        for (int64_t i = 0; i < sc.nrows(); ++i) r[size_t(i)] = sc(i, 0);
        return r;
    }
    std::vector<A> hotelling_t2(const Array2<A>& input) const {
        const Array2<A> sc = score_rows(input, inverse_variances());
        std::vector<A> r(size_t(sc.nrows()));
        for (int64_t i = 0; i < sc.nrows(); ++i) r[size_t(i)] = sc(i, 1);
        return r;
    }
    std::vector<A> score_samples(const Array2<A>& input) const {  // probabilistic-PCA log-likelihood per row (scikit-learn's score_samples)
        const double s2 = double(noise_variance());
        if (!(s2 > 0)) throw DecompositionError(DecompositionError::InvalidInput, "the noise variance is not positive (no discarded direction, or an exactly low-rank fit)");
        const std::vector<A> w = inverse_variances();
        const int64_t d = int64_t(means.size());
        double c = double(d) * std::log(2.0 * 3.14159265358979323846) + double(d - k) * std::log(s2);
        for (const A v : w) c -= std::log(double(v));
        const Array2<A> sc = score_rows(input, w);
        std::vector<A> r(size_t(sc.nrows()));
        for (int64_t i = 0; i < sc.nrows(); ++i) r[size_t(i)] = A(-0.5 * (c + double(sc(i, 0)) / s2 + double(sc(i, 1))));
        return r;
    }
};
}  // namespace detail

// Facts of the last exact Pca fit on a ctx (petal_hip_wide.h: an extension beyond the crate): dual = the n x n row-Gram route of wide
// data (not sharded, n < d, d > 2048; PETAL_OPT_PCA_DUAL forces or forbids it), kernel = k_row_gram ran, the order of the eigenproblem,
// the feature chunks of the row-Gram launch.
struct PcaRoute {
    bool dual = false, kernel = false;
    int64_t order = 0, chunks = 0;
};

template <class A>
class Pca {  // src/pca.rs:41-232
  public:
    explicit Pca(int64_t n_components, bool centering = true, Context* ctx = nullptr) {
        st_.k = n_components; st_.centering = centering; st_.ctx = ctx;
        st_.components = Array2<A>(n_components, 0);
    }
    const Array2<A>& components() const { return st_.components; }
    const std::vector<A>& mean() const { return st_.means; }
    int64_t n_components() const { return st_.k; }
    const std::vector<A>& singular_values() const { return st_.singular; }
    std::vector<A> explained_variance_ratio() const { return st_.explained_variance_ratio(); }
    void fit(const Array2<A>& input) { inner_fit(input, nullptr); }
    Array2<A> fit_transform(const Array2<A>& input) {
        if (st_.centering && input.nrows() == 0) { inner_fit(input, nullptr); return Array2<A>(0, st_.k ? input.ncols() : 0); }
        Array2<A> y(input.nrows(), st_.k);
        inner_fit(input, &y);
        return y;
    }
    Array2<A> transform(const Array2<A>& input) const { return st_.transform(input); }
    Array2<A> inverse_transform(const Array2<A>& input) const { return st_.inverse_transform(input); }
    // extension beyond the crate (petal_hip_score.h): scores of rows against the fitted model, one pass over the input each
    std::vector<A> explained_variance() const { return st_.explained_variance(); }
    A noise_variance() const { return st_.noise_variance(); }
    std::vector<A> reconstruction_error(const Array2<A>& input) const { return st_.reconstruction_error(input); }
    std::vector<A> hotelling_t2(const Array2<A>& input) const { return st_.hotelling_t2(input); }
    std::vector<A> score_samples(const Array2<A>& input) const { return st_.score_samples(input); }
    // extension beyond the crate (petal_hip_wide.h): which route the last exact fit on this model's ctx took
    PcaRoute last_route() const {
        int64_t v[4] = {0, 0, 0, 0};
        st_.context().check(petal_pca_last_route(st_.context().get(), v));
        PcaRoute r;
        r.dual = v[0] != 0; r.kernel = v[1] != 0; r.order = v[2]; r.chunks = v[3];
        return r;
    }

  private:
    void inner_fit(const Array2<A>& input, Array2<A>* y) {
        const int64_t d = input.ncols(), k = st_.k;
        Array2<A> comp(k, d);
        std::vector<A> means(d), sing(k);
        A tv = A(0);
        petal_matrix mx = input.view(), my{};
        if (y) my = y->view();
        st_.context().check(petal_pca_fit(st_.context().get(), &mx, k, st_.centering, comp.data.data(), means.data(), sing.data(),
                                          &tv, y ? &my : nullptr));
        if (st_.centering && input.nrows() == 0) return;
        st_.components = std::move(comp); st_.means = std::move(means); st_.singular = std::move(sing);
        st_.total_variance = tv; st_.n_samples = input.nrows();
    }
    detail::PcaState<A> st_;
};

// One exact Pca per row segment of a row-sorted matrix, in one call (petal_hip_segments.h: an extension beyond the crate).  Segment b is
// rows offsets[b] .. offsets[b + 1] - 1 and gets what Pca::fit gives on those rows alone; for d <= 64 the batch is one launch, a
// workgroup per segment (a very long segment is correct and not fast: fit it with Pca).
template <class A>
class SegmentedPca {
  public:
    explicit SegmentedPca(int64_t n_components, bool centering = true, Context* ctx = nullptr)
        : k_(n_components), centering_(centering), ctx_(ctx) {}
    int64_t n_components() const { return k_; }
    int64_t n_segments() const { return nseg_; }
    const std::vector<A>& components() const { return comp_; }           // n_segments x k x d, row-major, svd_flip's sign applied
    const std::vector<A>& mean() const { return means_; }                // n_segments x d
    const std::vector<A>& singular_values() const { return sing_; }      // n_segments x k
    const std::vector<A>& total_variance() const { return tv_; }         // n_segments
    const std::vector<int32_t>& status() const { return status_; }       // 0: fitted; 1: the segment held a NaN or an infinity (results NaN)
    int64_t kernel_segments() const { return kernel_segments_; }         // how many segments of the last fit the segment kernel fitted
    std::vector<A> explained_variance_ratio() const {
        std::vector<A> r(sing_.size());
        for (int64_t b = 0; b < nseg_; ++b)
            for (int64_t j = 0; j < k_; ++j) r[b * k_ + j] = sing_[b * k_ + j] * sing_[b * k_ + j] / tv_[b];
        return r;
    }
    void fit(const Array2<A>& input, const std::vector<int64_t>& offsets) { inner_fit(input, offsets, nullptr); }
    Array2<A> fit_transform(const Array2<A>& input, const std::vector<int64_t>& offsets) {
        Array2<A> y(input.nrows(), k_);
        inner_fit(input, offsets, &y);
        return y;
    }
    Array2<A> transform(const Array2<A>& input, const std::vector<int64_t>& offsets) const {
        if (input.ncols() != d_) throw DecompositionError(DecompositionError::InvalidInput, "# of columns should be " + std::to_string(d_));
        Array2<A> y(input.nrows(), k_);
        petal_matrix mx = input.view(), my = y.view();
        context().check(petal_transform_segments(context().get(), &mx, offsets_of(offsets), n_of(offsets), comp_.data(), means_.data(), k_, d_,
                                                 centering_, &my));
        return y;
    }
    Array2<A> inverse_transform(const Array2<A>& input, const std::vector<int64_t>& offsets) const {
        if (input.ncols() != k_) throw DecompositionError(DecompositionError::InvalidInput, "# of columns should be " + std::to_string(k_));
        Array2<A> x(input.nrows(), d_);
        petal_matrix my = input.view(), mx = x.view();
        context().check(petal_inverse_transform_segments(context().get(), &my, offsets_of(offsets), n_of(offsets), comp_.data(), means_.data(),
                                                         k_, d_, centering_, &mx));
        return x;
    }
    static std::vector<int64_t> offsets_from_lengths(const std::vector<int64_t>& lengths) {
        std::vector<int64_t> off(lengths.size() + 1, 0);
        for (size_t b = 0; b < lengths.size(); ++b) off[b + 1] = off[b] + lengths[b];
        return off;
    }

  private:
    Context& context() const { return ctx_ ? *ctx_ : Context::global(); }
    static const int64_t* offsets_of(const std::vector<int64_t>& offsets) {
        if (offsets.empty()) throw DecompositionError(DecompositionError::InvalidInput, "offsets needs n_segments + 1 values");
        return offsets.data();
    }
    static int64_t n_of(const std::vector<int64_t>& offsets) { return int64_t(offsets.size()) - 1; }
    void inner_fit(const Array2<A>& input, const std::vector<int64_t>& offsets, Array2<A>* y) {
        const int64_t* off = offsets_of(offsets);
        const int64_t nseg = n_of(offsets), d = input.ncols();
        std::vector<A> comp(size_t(nseg * k_ * d)), means(size_t(nseg * d)), sing(size_t(nseg * k_)), tv(size_t(nseg), A(0));
        std::vector<int32_t> status(size_t(nseg), 0);
        int64_t ks = 0;
        petal_matrix mx = input.view(), my{};
        if (y) my = y->view();
        context().check(petal_pca_fit_segments(context().get(), &mx, off, nseg, k_, centering_, comp.data(), means.data(), sing.data(), tv.data(),
                                               status.data(), y ? &my : nullptr, &ks));
        comp_ = std::move(comp); means_ = std::move(means); sing_ = std::move(sing); tv_ = std::move(tv); status_ = std::move(status);
        nseg_ = nseg; d_ = d; kernel_segments_ = ks;
    }
    int64_t k_, nseg_ = 0, d_ = 0, kernel_segments_ = 0;
    bool centering_;
    Context* ctx_;
    std::vector<A> comp_, means_, sing_, tv_;
    std::vector<int32_t> status_;
};

// The exact Pca fitted batch by batch (petal_hip_ipca.h: an extension beyond the crate).  partial_fit folds a batch into the float64
// statistic (rows seen, mean, M2) resident with the ctx; the model is what Pca::fit returns on the concatenation of the batches, up to
// the SIGN of each component: its entry of largest magnitude is positive (scikit-learn's rule), because a streaming fit never holds U.
// The model is refreshed lazily, by the first accessor after a batch.  Gram route only.  Destroy it before its Context.
template <class A>
class IncrementalPca {
  public:
    explicit IncrementalPca(int64_t n_components, bool centering = true, Context* ctx = nullptr) {
        st_.k = n_components; st_.centering = centering; st_.ctx = ctx;
        st_.components = Array2<A>(n_components, 0);
    }
    IncrementalPca(const IncrementalPca&) = delete;
    IncrementalPca& operator=(const IncrementalPca&) = delete;
    IncrementalPca(IncrementalPca&& o) noexcept : st_(std::move(o.st_)), h_(o.h_), dirty_(o.dirty_) { o.h_ = nullptr; }
    ~IncrementalPca() { petal_ipca_destroy(h_); }
    // the first batch fixes d
    IncrementalPca& partial_fit(const Array2<A>& batch) {
        open(batch.ncols());
        petal_matrix mx = batch.view();
        st_.context().check(petal_ipca_partial_fit(st_.context().get(), h_, &mx));
        dirty_ = true;
        return *this;
    }
    // adds the statistic of `other` (same ctx, d and centering), exactly; `other` is unchanged
    IncrementalPca& merge(const IncrementalPca& other) {
        if (!other.h_) return *this;
        open(other.info()[0]);
        st_.context().check(petal_ipca_merge(st_.context().get(), h_, other.h_));
        dirty_ = true;
        return *this;
    }
    void reset() {
        if (h_) st_.context().check(petal_ipca_reset(h_));
        st_.components = Array2<A>(st_.k, 0); st_.means.clear(); st_.singular.clear(); st_.total_variance = A(0); st_.n_samples = 0;
        dirty_ = false;
    }
    // { d, dtype, centering, rows seen, batches, batches the streaming kernel took, merges, 0 }
    std::vector<int64_t> info() const {
        std::vector<int64_t> v(8, 0);
        if (h_) petal_ipca_info(h_, v.data());
        return v;
    }
    int64_t n_samples_seen() const { return info()[3]; }
    // the statistic as host float64 (checkpoints; combining several processes by hand): returns rows seen
    double get_state(std::vector<double>& mean, std::vector<double>& m2) const {
        if (!h_) throw DecompositionError(DecompositionError::InvalidInput, "no batch has been seen yet");
        const int64_t d = info()[0];
        double n = 0;
        mean.assign(size_t(d), 0.0); m2.assign(size_t(d * d), 0.0);
        st_.context().check(petal_ipca_get_state(st_.context().get(), h_, &n, mean.data(), m2.data()));
        return n;
    }
    void set_state(double n, const std::vector<double>& mean, const std::vector<double>& m2) {
        if (m2.size() != mean.size() * mean.size()) throw DecompositionError(DecompositionError::InvalidInput, "m2 should be d x d");
        open(int64_t(mean.size()));
        st_.context().check(petal_ipca_set_state(st_.context().get(), h_, n, mean.data(), m2.data()));
        dirty_ = true;
    }
    const Array2<A>& components() { return model().components; }
    const std::vector<A>& mean() { return model().means; }
    int64_t n_components() const { return st_.k; }
    const std::vector<A>& singular_values() { return model().singular; }
    std::vector<A> explained_variance_ratio() { return model().explained_variance_ratio(); }
    Array2<A> transform(const Array2<A>& input) { return model().transform(input); }
    Array2<A> inverse_transform(const Array2<A>& input) { return model().inverse_transform(input); }
    std::vector<A> explained_variance() { return model().explained_variance(); }
    A noise_variance() { return model().noise_variance(); }
    std::vector<A> reconstruction_error(const Array2<A>& input) { return model().reconstruction_error(input); }
    std::vector<A> hotelling_t2(const Array2<A>& input) { return model().hotelling_t2(input); }
    std::vector<A> score_samples(const Array2<A>& input) { return model().score_samples(input); }

  private:
    void open(int64_t d) {
        if (h_) return;
        st_.context().check(petal_ipca_create(st_.context().get(), d, DTypeOf<A>::value, st_.centering, &h_));
    }
    const detail::PcaState<A>& model() {
        if (dirty_ && h_ && n_samples_seen() > 0) {   // (nothing seen yet: the model stays empty, as an unfitted Pca's)
            const int64_t d = info()[0], k = st_.k;
            Array2<A> comp(k, d);
            std::vector<A> means(d), sing(k);
            A tv = A(0);
            st_.context().check(petal_ipca_finalize(st_.context().get(), h_, k, comp.data.data(), means.data(), sing.data(), &tv));
            st_.components = std::move(comp); st_.means = std::move(means); st_.singular = std::move(sing);
            st_.total_variance = tv; st_.n_samples = n_samples_seen();
            dirty_ = false;
        }
        return st_;
    }
    detail::PcaState<A> st_;
    petal_ipca* h_ = nullptr;
    bool dirty_ = false;
};

// Kernel PCA (petal_hip_kpca.h: an extension beyond the crate; scikit-learn's KernelPCA).  kernel = PETAL_KERNEL_*; gamma <= 0 means
// 1 / d.  fit_transform = V sqrt(lambda); transform is one fused pass whose m x n kernel matrix never touches memory.  The fitted
// model lives with its ctx (destroy the model before the Context) and keeps its own device copy of the training rows.
struct KernelPcaInfo {
    int64_t n = 0, d = 0, k = 0, order = 0;
    bool fit_kernel = false;        // k_kmap ran on the fit's map (false: the fallback built K~)
    int transform_kernel = -1;      // k_kapply ran on the last transform (1 / 0; -1 before the first)
    int kernel = 0;
    bool topk_solver = false;       // the top-k subspace iteration delivered the eigenpairs (false: the full eigen-solver of order n ran)
};

template <class A>
class KernelPca {
  public:
    explicit KernelPca(int64_t n_components, int kernel = PETAL_KERNEL_LINEAR, double gamma = 0.0, int degree = 3, double coef0 = 1.0,
                       Context* ctx = nullptr)
        : k_(n_components), ctx_(ctx) {
        spec_.kernel = kernel; spec_.degree = degree; spec_.gamma = gamma; spec_.coef0 = coef0;
    }
    KernelPca(const KernelPca&) = delete;
    KernelPca& operator=(const KernelPca&) = delete;
    KernelPca(KernelPca&& o) noexcept : k_(o.k_), spec_(o.spec_), ctx_(o.ctx_), h_(o.h_) { o.h_ = nullptr; }
    ~KernelPca() { petal_kpca_destroy(h_); }
    KernelPca& fit(const Array2<A>& input) { inner_fit(input, nullptr); return *this; }
    Array2<A> fit_transform(const Array2<A>& input) {
        Array2<A> y(input.nrows(), k_);
        inner_fit(input, &y);
        return y;
    }
    Array2<A> transform(const Array2<A>& input) {
        Array2<A> y(input.nrows(), k_);
        petal_matrix mx = input.view(), my = y.view();
        context().check(petal_kpca_transform(context().get(), handle(), &mx, &my));
        return y;
    }
    int64_t n_components() const { return k_; }
    // the k leading eigenvalues of the centred kernel matrix, as computed (descending)
    std::vector<double> eigenvalues() const {
        std::vector<double> lam(size_t(k_), 0.0);
        if (petal_kpca_get(handle(), lam.data(), nullptr, nullptr) != PETAL_OK)
            throw DecompositionError(DecompositionError::InvalidInput, "petal_kpca_get failed");
        return lam;
    }
    KernelPcaInfo info() const {
        int64_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (petal_kpca_get(handle(), nullptr, nullptr, v) != PETAL_OK)
            throw DecompositionError(DecompositionError::InvalidInput, "petal_kpca_get failed");
        KernelPcaInfo r;
        r.n = v[0]; r.d = v[1]; r.k = v[2]; r.fit_kernel = v[3] != 0; r.transform_kernel = int(v[4]); r.order = v[5]; r.kernel = int(v[6]); r.topk_solver = v[7] != 0;
        return r;
    }

  private:
    Context& context() const { return ctx_ ? *ctx_ : Context::global(); }
    petal_kpca* handle() const {
        if (!h_) throw DecompositionError(DecompositionError::InvalidInput, "the model has not been fitted");
        return h_;
    }
    void inner_fit(const Array2<A>& input, Array2<A>* y) {
        petal_matrix mx = input.view(), my{};
        if (y) my = y->view();
        petal_kpca* h = nullptr;
        context().check(petal_kpca_fit(context().get(), &mx, k_, &spec_, &h, y ? &my : nullptr));
        petal_kpca_destroy(h_);
        h_ = h;
    }
    int64_t k_;
    petal_kernel_spec spec_{};
    Context* ctx_;
    petal_kpca* h_ = nullptr;
};

// Non-negative matrix factorisation X ~ W H (petal_hip_nmf.h: an extension beyond the crate; scikit-learn's NMF(solver="mu",
// beta_loss="frobenius")).  alpha_w, alpha_h (negative: the same as alpha_w) and l1_ratio are scikit-learn's penalties.  fit(x) draws
// W0 and H0 from Pcg(seed); fit(x, w0, h0) starts from the caller's.  tol > 0 stops at a check every 10th iteration; transform runs
// exactly max_iter W-updates in one pass over its input.  The fitted model lives with its ctx (destroy the model before the Context).
struct NmfInfo {
    int64_t n = 0, d = 0, k = 0, n_iter = 0;
    bool fit_kernel = false;        // k_nmf_pass ran in the fit (false: the composed path)
    int transform_kernel = -1;      // the same for the last transform (1 / 0; -1 before the first)
};

template <class A>
class CsrMatrix;   // (declared below: Nmf takes it in place of an Array2, petal_hip_nmf_sparse.h)

// extension beyond the crate (petal_hip_nmf_kl.h): the loss of a fit on sparse CSR input.  KullbackLeibler is scikit-learn's
// beta_loss="kullback-leibler"; it is taken by the CsrMatrix overloads only -- the dense overloads throw InvalidInput under it.
enum class NmfLoss : int64_t { Frobenius = PETAL_NMF_LOSS_FROBENIUS, KullbackLeibler = PETAL_NMF_LOSS_KL };
// extension beyond the crate (petal_hip_nmf_kl_dense.h): what the dense overloads do under the Kullback-Leibler loss.  Compress (the
// default) keeps them throwing "takes a CsrMatrix"; Fused sends the Array2 to the fused dense pass k_nmf_kl_pass (petal_nmf_fit_loss,
// petal_nmf_transform_loss; the composed path outside the kernel's envelope, no cap on the components).  Under the Frobenius loss it
// changes nothing.
enum class NmfDensePath : int { Compress = 0, Fused = 1 };
// extension beyond the crate (petal_hip_nmf_cd.h): the solver of the NEXT dense fit.  MultiplicativeUpdate (the default) is everything
// above, byte for byte; CoordinateDescent is scikit-learn's NMF(solver="cd") (its default, shuffle=False) under the Frobenius loss:
// the stopping rule runs after every iteration, transform starts from W = 0.  With the Kullback-Leibler loss or a CsrMatrix it throws.
enum class NmfSolver : int64_t { MultiplicativeUpdate = PETAL_NMF_SOLVER_MU, CoordinateDescent = PETAL_NMF_SOLVER_CD };
// extension beyond the crate (petal_hip_nmf_cd_sparse.h): what the CsrMatrix overloads do under CoordinateDescent.  Refuse (the default)
// keeps them throwing "does not take a CsrMatrix"; Sweep sends the matrix to the coordinate-descent sweeps k_nmf_cd_sweep
// (petal_nmf_fit_csr_solver, petal_nmf_transform_csr_solver; at most 64 components on the kernel, otherwise the library densifies).
// Under MultiplicativeUpdate it changes nothing.
enum class NmfSparsePath : int { Refuse = 0, Sweep = 1 };

template <class A>
class Nmf {
  public:
    explicit Nmf(int64_t n_components, int64_t max_iter = 200, double tol = 1e-4, uint64_t seed = 0, double alpha_w = 0.0,
                 double alpha_h = -1.0, double l1_ratio = 0.0, Context* ctx = nullptr)
        : k_(n_components), max_iter_(max_iter), tol_(tol), seed_(seed), alpha_w_(alpha_w), alpha_h_(alpha_h < 0 ? alpha_w : alpha_h),
          l1_ratio_(l1_ratio), ctx_(ctx) {}
    Nmf(const Nmf&) = delete;
    Nmf& operator=(const Nmf&) = delete;
    Nmf(Nmf&& o) noexcept
        : k_(o.k_), max_iter_(o.max_iter_), tol_(o.tol_), seed_(o.seed_), alpha_w_(o.alpha_w_), alpha_h_(o.alpha_h_), l1_ratio_(o.l1_ratio_),
          ctx_(o.ctx_), h_(o.h_), kernel_path_(o.kernel_path_), loss_(o.loss_), dense_path_(o.dense_path_), solver_(o.solver_),
          sparse_path_(o.sparse_path_) { o.h_ = nullptr; }
    ~Nmf() { petal_nmf_destroy(h_); }
    Nmf& loss(NmfLoss l) { loss_ = l; return *this; }   // the loss of the NEXT fit on a CsrMatrix (petal_hip_nmf_kl.h)
    NmfLoss loss() const { return loss_; }
    Nmf& dense_path(NmfDensePath p) { dense_path_ = p; return *this; }   // the route of the NEXT dense call under the Kullback-Leibler loss
    NmfDensePath dense_path() const { return dense_path_; }
    Nmf& solver(NmfSolver s) { solver_ = s; return *this; }   // the solver of the NEXT dense fit (petal_hip_nmf_cd.h)
    NmfSolver solver() const { return solver_; }
    Nmf& sparse_path(NmfSparsePath p) { sparse_path_ = p; return *this; }   // the route of the NEXT CsrMatrix call under CoordinateDescent
    NmfSparsePath sparse_path() const { return sparse_path_; }
    // the solver the fitted model remembers
    NmfSolver model_solver() const {
        int64_t v = 0;
        if (petal_nmf_get_solver(handle(), &v) != PETAL_OK) throw DecompositionError(DecompositionError::InvalidInput, "petal_nmf_get_solver failed");
        return static_cast<NmfSolver>(v);
    }
    // the loss the fitted model remembers
    NmfLoss model_loss() const {
        int64_t v = 0;
        if (petal_nmf_get_loss(handle(), &v) != PETAL_OK) throw DecompositionError(DecompositionError::InvalidInput, "petal_nmf_get_loss failed");
        return static_cast<NmfLoss>(v);
    }
    Nmf& fit(const Array2<A>& input) { inner_fit(input, nullptr, nullptr, nullptr); return *this; }
    Nmf& fit(const Array2<A>& input, const Array2<A>& w0, const Array2<A>& h0) { inner_fit(input, &w0, &h0, nullptr); return *this; }
    Array2<A> fit_transform(const Array2<A>& input) {
        Array2<A> w(input.nrows(), k_);
        inner_fit(input, nullptr, nullptr, &w);
        return w;
    }
    Array2<A> fit_transform(const Array2<A>& input, const Array2<A>& w0, const Array2<A>& h0) {
        Array2<A> w(input.nrows(), k_);
        inner_fit(input, &w0, &h0, &w);
        return w;
    }
    Array2<A> transform(const Array2<A>& input) {
        if (dense_path_ != NmfDensePath::Fused) no_dense_kl();
        Array2<A> w(input.nrows(), k_);
        petal_matrix mx = input.view(), mw = w.view();
        if (dense_path_ == NmfDensePath::Fused) {   // dispatches on the model's loss; a Frobenius model: petal_nmf_transform's bytes
            context().check(petal_nmf_transform_loss(context().get(), handle(), &mx, &mw));
            if (model_loss() == NmfLoss::KullbackLeibler && input.nrows() > 0) kernel_path_ = info().transform_kernel;
        } else {
            context().check(petal_nmf_transform(context().get(), handle(), &mx, &mw));
        }
        return w;
    }
    Array2<A> inverse_transform(const Array2<A>& w) {
        Array2<A> x(w.nrows(), info().d);
        petal_matrix mw = w.view(), mx = x.view();
        context().check(petal_nmf_inverse_transform(context().get(), handle(), &mw, &mx));
        return x;
    }
    // extension beyond the crate (petal_hip_nmf_sparse.h): sparse CSR input, never densified where the sweep kernel runs (at most 64
    // components, a resident handle); otherwise the library densifies and runs the dense fit, bit for bit its result
    Nmf& fit(const CsrMatrix<A>& input) { inner_fit_sparse(input, nullptr, nullptr, nullptr); return *this; }
    Nmf& fit(const CsrMatrix<A>& input, const Array2<A>& w0, const Array2<A>& h0) { inner_fit_sparse(input, &w0, &h0, nullptr); return *this; }
    Array2<A> fit_transform(const CsrMatrix<A>& input) {
        Array2<A> w(input.nrows(), k_);
        inner_fit_sparse(input, nullptr, nullptr, &w);
        return w;
    }
    Array2<A> fit_transform(const CsrMatrix<A>& input, const Array2<A>& w0, const Array2<A>& h0) {
        Array2<A> w(input.nrows(), k_);
        inner_fit_sparse(input, &w0, &h0, &w);
        return w;
    }
    Array2<A> transform(const CsrMatrix<A>& input) {
        Array2<A> w(input.nrows(), k_);
        petal_matrix mw = w.view();
        if (sparse_path_ == NmfSparsePath::Sweep)   // dispatches on the model's solver; a multiplicative model: petal_nmf_transform_csr's bytes
            context().check(petal_nmf_transform_csr_solver(context().get(), handle(), input.get(), &mw, &kernel_path_));
        else
            context().check(petal_nmf_transform_csr(context().get(), handle(), input.get(), &mw, &kernel_path_));
        return w;
    }
    // the last sparse call: 1 the sweep kernel, 0 the densifying fall-back; the last fused dense Kullback-Leibler call: 1 k_nmf_kl_pass, 0 the composed path
    int64_t kernel_path() const { return kernel_path_; }
    int64_t n_components() const { return k_; }
    // H, k x d, float64
    Array2<double> components() const {
        const NmfInfo in = info();
        Array2<double> h(in.k, in.d);
        if (petal_nmf_get(handle(), h.data.data(), nullptr, nullptr) != PETAL_OK)
            throw DecompositionError(DecompositionError::InvalidInput, "petal_nmf_get failed");
        return h;
    }
    int64_t n_iter() const { return info().n_iter; }
    double reconstruction_err() const {
        double e[2] = {0, 0};
        if (petal_nmf_get(handle(), nullptr, nullptr, e) != PETAL_OK)
            throw DecompositionError(DecompositionError::InvalidInput, "petal_nmf_get failed");
        return e[0];
    }
    NmfInfo info() const {
        int64_t v[6] = {0, 0, 0, 0, 0, 0};
        if (petal_nmf_get(handle(), nullptr, v, nullptr) != PETAL_OK)
            throw DecompositionError(DecompositionError::InvalidInput, "petal_nmf_get failed");
        NmfInfo r;
        r.n = v[0]; r.d = v[1]; r.k = v[2]; r.n_iter = v[3]; r.fit_kernel = v[4] != 0; r.transform_kernel = int(v[5]);
        return r;
    }

  private:
    Context& context() const { return ctx_ ? *ctx_ : Context::global(); }
    petal_nmf* handle() const {
        if (!h_) throw DecompositionError(DecompositionError::InvalidInput, "the model has not been fitted");
        return h_;
    }
    void no_dense_kl() const {
        if (loss_ == NmfLoss::KullbackLeibler)
            throw DecompositionError(DecompositionError::InvalidInput,
                                     "Nmf: the kullback-leibler loss takes a CsrMatrix (compress the dense rows to the CSR of their non-zero entries)");
    }
    void no_sparse_cd() const {
        if (solver_ != NmfSolver::CoordinateDescent) return;
        if (sparse_path_ != NmfSparsePath::Sweep)
            throw DecompositionError(DecompositionError::InvalidInput, "Nmf: the coordinate-descent solver does not take a CsrMatrix in this version");
        if (loss_ != NmfLoss::Frobenius)
            throw DecompositionError(DecompositionError::InvalidInput, "Nmf: the coordinate-descent solver does not take the kullback-leibler loss");
    }
    void inner_fit(const Array2<A>& input, const Array2<A>* w0, const Array2<A>* h0, Array2<A>* w) {
        const bool cd = solver_ == NmfSolver::CoordinateDescent;
        if (cd && loss_ != NmfLoss::Frobenius)
            throw DecompositionError(DecompositionError::InvalidInput, "Nmf: the coordinate-descent solver does not take the kullback-leibler loss");
        const bool fused = loss_ == NmfLoss::KullbackLeibler && dense_path_ == NmfDensePath::Fused;
        if (!fused) no_dense_kl();
        petal_matrix mx = input.view(), m0{}, m1{}, mw{};
        if (w0) { m0 = w0->view(); m1 = h0->view(); }
        if (w) mw = w->view();
        const double n = double(input.nrows()), d = double(input.ncols());
        petal_nmf_spec spec{};
        spec.max_iter = max_iter_; spec.tol = tol_;
        spec.l1_w = d * alpha_w_ * l1_ratio_; spec.l2_w = d * alpha_w_ * (1.0 - l1_ratio_);
        spec.l1_h = n * alpha_h_ * l1_ratio_; spec.l2_h = n * alpha_h_ * (1.0 - l1_ratio_);
        petal_nmf* h = nullptr;
        if (cd)
            context().check(petal_nmf_fit_solver(context().get(), &mx, k_, &spec, static_cast<int64_t>(solver_), w0 ? &m0 : nullptr,
                                                 w0 ? &m1 : nullptr, int64_t(seed_), &h, w ? &mw : nullptr));
        else if (fused)
            context().check(petal_nmf_fit_loss(context().get(), &mx, k_, &spec, static_cast<int64_t>(loss_), w0 ? &m0 : nullptr,
                                               w0 ? &m1 : nullptr, int64_t(seed_), &h, w ? &mw : nullptr));
        else
            context().check(petal_nmf_fit(context().get(), &mx, k_, &spec, w0 ? &m0 : nullptr, w0 ? &m1 : nullptr, int64_t(seed_), &h,
                                          w ? &mw : nullptr));
        petal_nmf_destroy(h_);
        h_ = h;
        if (fused) kernel_path_ = info().fit_kernel ? 1 : 0;
    }
    void inner_fit_sparse(const CsrMatrix<A>& input, const Array2<A>* w0, const Array2<A>* h0, Array2<A>* w) {
        no_sparse_cd();
        petal_matrix m0{}, m1{}, mw{};
        if (w0) { m0 = w0->view(); m1 = h0->view(); }
        if (w) mw = w->view();
        const double n = double(input.nrows()), d = double(input.ncols());
        petal_nmf_spec spec{};
        spec.max_iter = max_iter_; spec.tol = tol_;
        spec.l1_w = d * alpha_w_ * l1_ratio_; spec.l2_w = d * alpha_w_ * (1.0 - l1_ratio_);
        spec.l1_h = n * alpha_h_ * l1_ratio_; spec.l2_h = n * alpha_h_ * (1.0 - l1_ratio_);
        petal_nmf* h = nullptr;
        if (solver_ == NmfSolver::CoordinateDescent)   // sparse_path(Sweep): petal_hip_nmf_cd_sparse.h
            context().check(petal_nmf_fit_csr_solver(context().get(), input.get(), k_, &spec, static_cast<int64_t>(solver_), w0 ? &m0 : nullptr,
                                                     w0 ? &m1 : nullptr, int64_t(seed_), &h, w ? &mw : nullptr, &kernel_path_));
        else if (loss_ == NmfLoss::Frobenius)
            context().check(petal_nmf_fit_csr(context().get(), input.get(), k_, &spec, w0 ? &m0 : nullptr, w0 ? &m1 : nullptr, int64_t(seed_), &h,
                                              w ? &mw : nullptr, &kernel_path_));
        else
            context().check(petal_nmf_fit_csr_loss(context().get(), input.get(), k_, &spec, static_cast<int64_t>(loss_), w0 ? &m0 : nullptr,
                                                   w0 ? &m1 : nullptr, int64_t(seed_), &h, w ? &mw : nullptr, &kernel_path_));
        petal_nmf_destroy(h_);
        h_ = h;
    }
    int64_t k_, max_iter_;
    double tol_;
    uint64_t seed_;
    double alpha_w_, alpha_h_, l1_ratio_;
    Context* ctx_;
    petal_nmf* h_ = nullptr;
    int64_t kernel_path_ = 0;
    NmfLoss loss_ = NmfLoss::Frobenius;
    NmfDensePath dense_path_ = NmfDensePath::Compress;
    NmfSolver solver_ = NmfSolver::MultiplicativeUpdate;
    NmfSparsePath sparse_path_ = NmfSparsePath::Refuse;
};

class PcaBuilder {  // src/pca.rs:246-283
  public:
    explicit PcaBuilder(int64_t n_components) : k_(n_components) {}
    static PcaBuilder new_(int64_t n_components) { return PcaBuilder(n_components); }
    PcaBuilder& centering(bool c) { centering_ = c; return *this; }
    PcaBuilder& context(Context* c) { ctx_ = c; return *this; }
    template <class A> Pca<A> build() const { return Pca<A>(k_, centering_, ctx_); }

  private:
    int64_t k_; bool centering_ = true; Context* ctx_ = nullptr;
};

// A sparse matrix in CSR form, resident with its ctx (petal_hip_sparse.h: an extension beyond the crate).  The arrays are checked and
// copied, the transposed image and the work items are built on the host, both images are uploaded once; RandomizedPca::fit,
// fit_transform and transform take it in place of an Array2.  Indices inside a row need not be sorted, duplicates act as their sum.
// Destroy it before its Context.
template <class A>
class CsrMatrix {
  public:
    CsrMatrix(int64_t rows, int64_t cols, const std::vector<int64_t>& indptr, const std::vector<int32_t>& indices, const std::vector<A>& values,
              Context* ctx = nullptr)
        : rows_(rows), cols_(cols), nnz_(int64_t(values.size())), ctx_(ctx) {
        if (int64_t(indptr.size()) != rows + 1)
            throw DecompositionError(DecompositionError::InvalidInput, "indptr should have " + std::to_string(rows + 1) + " entries");
        if (indices.size() != values.size()) throw DecompositionError(DecompositionError::InvalidInput, "indices and values differ in length");
        context().check(petal_csr_create(context().get(), rows, cols, nnz_, indptr.data(), indices.data(), values.data(),
                                         sizeof(A) == 4 ? PETAL_F32 : PETAL_F64, &h_));
    }
    CsrMatrix(const CsrMatrix&) = delete;
    CsrMatrix& operator=(const CsrMatrix&) = delete;
    CsrMatrix(CsrMatrix&& o) noexcept : rows_(o.rows_), cols_(o.cols_), nnz_(o.nnz_), ctx_(o.ctx_), h_(o.h_) { o.h_ = nullptr; }
    ~CsrMatrix() { petal_csr_destroy(h_); }
    int64_t nrows() const { return rows_; }
    int64_t ncols() const { return cols_; }
    int64_t nnz() const { return nnz_; }
    bool resident() const { int64_t v[8]; petal_csr_info(h_, v); return v[4] != 0; }   // false: no sparse kernel in the device-op layer, the entries densify
    const petal_csr* get() const { return h_; }
    Context& context() const { return ctx_ ? *ctx_ : Context::global(); }
    // test aid (petal_csr_gemm): X . P or X^T . P minus a s^T (s empty: no epilogue; a empty: all ones), row-major float64
    std::vector<double> gemm(const std::vector<double>& p, int64_t n, bool transposed = false, const std::vector<double>& a = {},
                             const std::vector<double>& s = {}) const {
        std::vector<double> out(size_t((transposed ? cols_ : rows_) * n));
        context().check(petal_csr_gemm(context().get(), h_, transposed, p.data(), n, a.empty() ? nullptr : a.data(), s.empty() ? nullptr : s.data(),
                                       out.data()));
        return out;
    }

  private:
    int64_t rows_, cols_, nnz_;
    Context* ctx_;
    petal_csr* h_ = nullptr;
};

template <class A, class R = Pcg>
class RandomizedPca {  // src/pca.rs:317-551
  public:
    RandomizedPca(int64_t n_components, R rng, bool centering = true, Context* ctx = nullptr) : rng_(rng) {
        st_.k = n_components; st_.centering = centering; st_.ctx = ctx;
        st_.components = Array2<A>(n_components, 0);
    }
    static RandomizedPca with_seed(int64_t n_components, unsigned __int128 seed) { return RandomizedPca(n_components, R::from_seed_be_bytes(seed)); }
    static RandomizedPca with_rng(int64_t n_components, R rng) { return RandomizedPca(n_components, rng); }
    const Array2<A>& components() const { return st_.components; }
    const std::vector<A>& mean() const { return st_.means; }
    int64_t n_components() const { return st_.k; }
    const std::vector<A>& singular_values() const { return st_.singular; }
    std::vector<A> explained_variance_ratio() const { return st_.explained_variance_ratio(); }
    void fit(const Array2<A>& input) { inner_fit(input, nullptr); }
    Array2<A> fit_transform(const Array2<A>& input) {
        Array2<A> y(input.nrows(), st_.k);
        inner_fit(input, &y);
        return y;
    }
    Array2<A> transform(const Array2<A>& input) const { return st_.transform(input); }
    Array2<A> inverse_transform(const Array2<A>& input) const { return st_.inverse_transform(input); }
    // extension beyond the crate (petal_hip_sparse.h): sparse CSR input, never densified.  Row scores take dense input only.
    void fit(const CsrMatrix<A>& input) { inner_fit_sparse(input, nullptr); }
    Array2<A> fit_transform(const CsrMatrix<A>& input) {
        Array2<A> y(input.nrows(), st_.k);
        inner_fit_sparse(input, &y);
        return y;
    }
    Array2<A> transform(const CsrMatrix<A>& input) {
        const int64_t d = int64_t(st_.means.size());
        if (input.ncols() != d) throw DecompositionError(DecompositionError::InvalidInput, "# of columns should be " + std::to_string(d));
        Array2<A> y(input.nrows(), st_.k);
        petal_matrix my = y.view();
        st_.context().check(petal_transform_csr(st_.context().get(), input.get(), st_.components.data.data(), st_.means.data(), st_.k, d,
                                                st_.centering, &my, &kernel_path_));
        return y;
    }
    int64_t kernel_path() const { return kernel_path_; }   // the last sparse call: 1 the sparse product kernel, 0 the densifying fall-back
    // extension beyond the crate (petal_hip_score.h): scores of rows against the fitted model, one pass over the input each
    std::vector<A> explained_variance() const { return st_.explained_variance(); }
    A noise_variance() const { return st_.noise_variance(); }
    std::vector<A> reconstruction_error(const Array2<A>& input) const { return st_.reconstruction_error(input); }
    std::vector<A> hotelling_t2(const Array2<A>& input) const { return st_.hotelling_t2(input); }
    std::vector<A> score_samples(const Array2<A>& input) const { return st_.score_samples(input); }
    static constexpr int64_t N_OVERSAMPLE = 10, N_ITER = 7;  // src/pca.rs:679-680

  private:
    void inner_fit(const Array2<A>& input, Array2<A>* y) {
        const int64_t d = input.ncols(), k = st_.k, l = k + N_OVERSAMPLE;
        // the crate draws Omega only after the shape check and the mean (src/pca.rs:513-532, 701-705); an input it
        // rejects or returns early on must not advance the model's RNG
        std::vector<A> omega;
        const bool will_draw = !(input.nrows() < k || d < k) && !(st_.centering && input.nrows() == 0);
        if (will_draw) {
            omega.resize(size_t(d) * l);
            for (auto& v : omega) v = A(rng_.standard_normal());  // row-major d x l fill, f64 draw cast to A
        }
        Array2<A> comp(k, d);
        std::vector<A> means(d), sing(k);
        A tv = A(0);
        petal_matrix mx = input.view(), my{};
        if (y) my = y->view();
        st_.context().check(petal_rpca_fit(st_.context().get(), &mx, k, N_OVERSAMPLE, N_ITER, st_.centering,
                                           omega.empty() ? nullptr : omega.data(), comp.data.data(), means.data(), sing.data(),
                                           &tv, y ? &my : nullptr));
        if (st_.centering && input.nrows() == 0) return;
        st_.components = std::move(comp); st_.means = std::move(means); st_.singular = std::move(sing);
        st_.total_variance = tv; st_.n_samples = input.nrows();
    }
    void inner_fit_sparse(const CsrMatrix<A>& input, Array2<A>* y) {
        const int64_t d = input.ncols(), k = st_.k, l = k + N_OVERSAMPLE;
        std::vector<A> omega;
        const bool will_draw = !(input.nrows() < k || d < k) && !(st_.centering && input.nrows() == 0);
        if (will_draw) {
            omega.resize(size_t(d) * l);
            for (auto& v : omega) v = A(rng_.standard_normal());
        }
        Array2<A> comp(k, d);
        std::vector<A> means(d), sing(k);
        A tv = A(0);
        petal_matrix my{};
        if (y) my = y->view();
        st_.context().check(petal_rpca_fit_csr(st_.context().get(), input.get(), k, N_OVERSAMPLE, N_ITER, st_.centering,
                                               omega.empty() ? nullptr : omega.data(), comp.data.data(), means.data(), sing.data(), &tv,
                                               y ? &my : nullptr, &kernel_path_));
        if (st_.centering && input.nrows() == 0) return;
        st_.components = std::move(comp); st_.means = std::move(means); st_.singular = std::move(sing);
        st_.total_variance = tv; st_.n_samples = input.nrows();
    }
    R rng_;
    detail::PcaState<A> st_;
    int64_t kernel_path_ = 0;
};

template <class R = Pcg>
class RandomizedPcaBuilder {  // src/pca.rs:564-663
  public:
    explicit RandomizedPcaBuilder(int64_t n_components) : k_(n_components), rng_(R::from_seed_be_bytes(random_seed())) {}
    static RandomizedPcaBuilder new_(int64_t n_components) { return RandomizedPcaBuilder(n_components); }
    static RandomizedPcaBuilder with_rng(R rng, int64_t n_components) { RandomizedPcaBuilder b(n_components); b.rng_ = rng; return b; }
    RandomizedPcaBuilder& seed(unsigned __int128 s) { rng_ = R::from_seed_be_bytes(s); return *this; }
    RandomizedPcaBuilder& centering(bool c) { centering_ = c; return *this; }
    RandomizedPcaBuilder& context(Context* c) { ctx_ = c; return *this; }
    template <class A> RandomizedPca<A, R> build() const { return RandomizedPca<A, R>(k_, rng_, centering_, ctx_); }

  private:
    int64_t k_; R rng_; bool centering_ = true; Context* ctx_ = nullptr;
};

template <class A, class R = Pcg>
class FastIca {  // src/ica.rs:41-221
  public:
    explicit FastIca(R rng, Context* ctx = nullptr) : rng_(rng), ctx_(ctx) {}
    static FastIca with_seed(unsigned __int128 seed) { return FastIca(R::from_seed_be_bytes(seed)); }
    static FastIca with_rng(R rng) { return FastIca(rng); }
    void fit(const Array2<A>& input) { inner_fit(input, nullptr); }
    Array2<A> fit_transform(const Array2<A>& input) {
        const int64_t nc = std::min(input.nrows(), input.ncols());
        if (input.nrows() == 0) return Array2<A>(0, input.ncols());  // src/ica.rs:174-176
        Array2<A> y(input.nrows(), nc);
        inner_fit(input, &y);
        return y;
    }
    Array2<A> transform(const Array2<A>& input) const {  // src/ica.rs:120-131
        const int64_t d = int64_t(means_.size());
        if (input.ncols() != d) throw DecompositionError(DecompositionError::InvalidInput, "too many columns");
        Array2<A> y(input.nrows(), components_.nrows());
        petal_matrix mx = input.view(), my = y.view();
        context().check(petal_transform(context().get(), &mx, components_.data.data(), means_.data(), components_.nrows(), d, 1, &my));
        return y;
    }
    const Array2<A>& components() const { return components_; }
    int64_t n_iter() const { return n_iter_; }
    int mode = PETAL_ICA_TEXTBOOK;  // PETAL_ICA_REFERENCE_LITERAL follows src/ica.rs:345-349, 369-380 as written
    // the contrast function g: PETAL_ICA_CONTRAST_LOGCOSH (the crate's, src/ica.rs:383-398), _EXP or _CUBE (extensions of this library)
    int contrast = PETAL_ICA_CONTRAST_LOGCOSH;

  private:
    Context& context() const { return ctx_ ? *ctx_ : Context::global(); }
    void inner_fit(const Array2<A>& input, Array2<A>* y) {
        if (input.nrows() == 0) return;
        const int64_t d = input.ncols(), nc = std::min(input.nrows(), d);  // src/ica.rs:173
        std::vector<A> w_init(size_t(nc) * nc);
        for (auto& v : w_init) v = A(rng_.standard_normal());  // src/ica.rs:210-214
        Array2<A> comp(nc, d);
        std::vector<A> means(d);
        int64_t it = 0;
        petal_matrix mx = input.view(), my{};
        if (y) my = y->view();
        context().check(petal_fastica_fit(context().get(), &mx, 0, 1e-4, 200, mode | contrast, w_init.data(), comp.data.data(), means.data(),
                                          &it, y ? &my : nullptr));
        components_ = std::move(comp); means_ = std::move(means); n_iter_ = it;
    }
    R rng_;
    Context* ctx_;
    Array2<A> components_;
    std::vector<A> means_;
    int64_t n_iter_ = 0;
};

template <class R = Pcg>
class FastIcaBuilder {  // src/ica.rs:244-308
  public:
    FastIcaBuilder() : rng_(R::from_seed_be_bytes(random_seed())) {}
    static FastIcaBuilder new_() { return FastIcaBuilder(); }
    static FastIcaBuilder with_rng(R rng) { FastIcaBuilder b; b.rng_ = rng; return b; }
    FastIcaBuilder& seed(unsigned __int128 s) { rng_ = R::from_seed_be_bytes(s); return *this; }
    FastIcaBuilder& context(Context* c) { ctx_ = c; return *this; }
    FastIcaBuilder& contrast(int c) { contrast_ = c; return *this; }  // PETAL_ICA_CONTRAST_*
    template <class A> FastIca<A, R> build() const {
        FastIca<A, R> m(rng_, ctx_);
        m.contrast = contrast_;
        return m;
    }

  private:
    R rng_; Context* ctx_ = nullptr; int contrast_ = PETAL_ICA_CONTRAST_LOGCOSH;
};

}  // namespace petal_decomposition

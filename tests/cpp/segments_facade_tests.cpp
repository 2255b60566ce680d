// SegmentedPca of the C++ facade (include/petal_decomposition.hpp over petal_hip_segments.h): a batch of segments against Pca on each
// segment alone, the transform round trip at k = d, a planted NaN segment, and the error messages.
//   segments_facade_tests kernel    the library has the segment kernel (libpetal_hip.so): kernel_segments == n_segments
//   segments_facade_tests loop      it has not (the host simulation): kernel_segments == 0 and the batch equals Pca bit for bit
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>

#include "petal_decomposition.hpp"

using namespace petal_decomposition;

static int failures = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static const unsigned __int128 RNG_SEED = (unsigned __int128)1234567891011121314ull;

static Array2<double> data(int n, int d) {
    Pcg rng(RNG_SEED + 5);
    Array2<double> x(n, d);
    for (int i = 0; i < n; ++i) {
        const double a = 3.0 * rng.standard_normal(), b = 2.0 * rng.standard_normal(), c = rng.standard_normal();
        for (int j = 0; j < d; ++j) x(i, j) = 1.0 + j + a * std::cos(0.7 * j) + b * std::sin(1.3 * j + 0.2) + c * ((j % 3) - 1.0) + 0.05 * rng.standard_normal();
    }
    return x;
}

int main(int argc, char** argv) {
    const bool loop = argc > 1 && std::strcmp(argv[1], "loop") == 0;
    const int d = 6, k = 3;
    const std::vector<int64_t> lengths = {40, 7, 130};
    const std::vector<int64_t> off = SegmentedPca<double>::offsets_from_lengths(lengths);
    const Array2<double> x = data(int(off.back()), d);
    SegmentedPca<double> seg(k);
    const Array2<double> y = seg.fit_transform(x, off);
    CHECK(seg.n_segments() == 3 && seg.kernel_segments() == (loop ? 0 : 3));
    CHECK(y.nrows() == off.back() && y.ncols() == k);
    const auto evr = seg.explained_variance_ratio();
    for (int b = 0; b < 3; ++b) {
        Array2<double> xb(lengths[b], d);
        std::memcpy(xb.data.data(), &x(off[b], 0), sizeof(double) * size_t(lengths[b]) * d);
        Pca<double> one(k);
        const Array2<double> yb = one.fit_transform(xb);
        CHECK(seg.status()[b] == 0);
        for (int j = 0; j < k; ++j) {
            const double s = seg.singular_values()[b * k + j], s1 = one.singular_values()[j];
            CHECK(loop ? s == s1 : std::fabs(s - s1) <= 1e-12 * one.singular_values()[0]);
            CHECK(std::fabs(evr[b * k + j] - one.explained_variance_ratio()[j]) <= 1e-11);
            for (int i = 0; i < d; ++i) {
                const double c = seg.components()[(b * k + j) * d + i], c1 = one.components()(j, i);
                CHECK(loop ? c == c1 : std::fabs(c - c1) <= 1e-10);
            }
            for (int64_t r = 0; r < lengths[b]; ++r)
                CHECK(loop ? y(off[b] + r, j) == yb(r, j) : std::fabs(y(off[b] + r, j) - yb(r, j)) <= 1e-10 * one.singular_values()[0]);
        }
        for (int i = 0; i < d; ++i) CHECK(std::fabs(seg.mean()[b * d + i] - one.mean()[i]) <= 1e-13 * (1 + std::fabs(one.mean()[i])));
    }
    // transform of the fitted batch is fit_transform's y; at k = d the inverse gives the rows back
    const Array2<double> y2 = seg.transform(x, off);
    for (size_t e = 0; e < y.data.size(); ++e) CHECK(std::fabs(y2.data[e] - y.data[e]) <= 1e-10 * (1 + std::fabs(y.data[e])));
    SegmentedPca<double> full(d);
    full.fit(x, off);
    const Array2<double> xr = full.inverse_transform(full.transform(x, off), off);
    for (size_t e = 0; e < x.data.size(); ++e) CHECK(std::fabs(xr.data[e] - x.data[e]) <= 1e-11 * (1 + std::fabs(x.data[e])));
    // one bad group does not lose the batch
    Array2<double> xn = x;
    xn(off[1] + 2, 4) = std::numeric_limits<double>::quiet_NaN();
    SegmentedPca<double> bad(k);
    const Array2<double> yn = bad.fit_transform(xn, off);
    CHECK(bad.status()[0] == 0 && bad.status()[1] == 1 && bad.status()[2] == 0);
    CHECK(std::isnan(bad.singular_values()[1 * k]) && std::isnan(bad.components()[(1 * k) * d]) && std::isnan(bad.total_variance()[1]));
    CHECK(std::isnan(yn(off[1], 0)) && std::isnan(yn(off[2] - 1, k - 1)));
    for (int b = 0; b < 3; b += 2)
        for (int j = 0; j < k; ++j) CHECK(bad.singular_values()[b * k + j] == seg.singular_values()[b * k + j]);
    // messages
    try { seg.fit(x, {0, 40, 30, off.back()}); CHECK(false); } catch (const DecompositionError& e) {
        CHECK(e.kind == DecompositionError::InvalidInput && std::string(e.what()).find("offsets[2]") != std::string::npos);
    }
    try { seg.fit(x, {0, 2, off.back()}); CHECK(false); } catch (const DecompositionError& e) {
        CHECK(e.kind == DecompositionError::InvalidInput && std::string(e.what()).find("segment 0: every dimension should be at least 3") != std::string::npos);
    }
    try { seg.transform(Array2<double>(4, 5), {0, 4}); CHECK(false); } catch (const DecompositionError& e) {
        CHECK(e.kind == DecompositionError::InvalidInput && std::string(e.what()).find("# of columns should be 6") != std::string::npos);
    }
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("segments facade tests passed (%s)\n", loop ? "loop" : "kernel");
    return 0;
}

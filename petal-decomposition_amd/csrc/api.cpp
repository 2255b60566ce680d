// api.cpp -- the extern "C" boundary declared in include/petal_hip.h.  Every entry point catches all
// exceptions: nothing unwinds or aborts across the ABI (the reference panics at ica.rs:369 and
// linalg.rs:75/106/132; here those become PETAL_LINALG_ERROR / PETAL_INVALID_INPUT).
#include <cstdio>
#include <new>

#include "ctx.h"
#include "../../include/petal_hip_score.h"
#include "../../include/petal_hip_segments.h"
#include "../../include/petal_hip_sparse.h"
#include "../../include/petal_hip_ipca.h"
#include "../../include/petal_hip_wide.h"
#include "../../include/petal_hip_kpca.h"
#include "../../include/petal_hip_nmf.h"
#include "../../include/petal_hip_nmf_sparse.h"
#include "../../include/petal_hip_nmf_kl.h"
#include "../../include/petal_hip_nmf_kl_dense.h"
#include "../../include/petal_hip_nmf_cd.h"
#include "../../include/petal_hip_nmf_cd_sparse.h"
#include "../../include/petal_hip_probe.h"

using namespace petal;

namespace {

// makes the ctx's device current on the calling thread for the duration of an entry point (the ctx may live on a device
// other than the thread's current one, or be used from a thread that never called hipSetDevice) and restores the
// previous device afterwards
struct DeviceScope {
    petal::Dev* dev;
    int prev = -1;
    explicit DeviceScope(petal::Dev* d) : dev(d) { if (dev) prev = dev_push_current(dev); }
    ~DeviceScope() { if (dev) dev_pop_current(dev, prev); }
};

template <class F>
int guarded(petal_ctx* ctx, F&& f) {
    if (!ctx) return PETAL_INVALID_INPUT;
    try {
        ctx->err.clear();
        DeviceScope scope(ctx->dev);
        f();
        return PETAL_OK;
    } catch (const Error& e) {
        ctx->err = e.what();
        if (ctx->dev) dev_abort(ctx->dev);
        return e.code;
    } catch (const std::bad_alloc&) {
        ctx->err = "out of host memory";
        if (ctx->dev) dev_abort(ctx->dev);
        return PETAL_DEVICE_ERROR;
    } catch (const std::exception& e) {
        ctx->err = e.what();
        if (ctx->dev) dev_abort(ctx->dev);
        return PETAL_DEVICE_ERROR;
    } catch (...) {
        ctx->err = "unknown error";
        if (ctx->dev) dev_abort(ctx->dev);
        return PETAL_DEVICE_ERROR;
    }
}

void need(const void* p, const char* what) {
    if (!p) invalid_input(std::string(what) + " must not be null");
}

}  // namespace

extern "C" {

const char* petal_version(void) { return "petal-hip 0.1.0 (gfx950)"; }

int petal_ctx_create(int device, void* stream, petal_ctx** out) {
    if (!out) return PETAL_INVALID_INPUT;
    *out = nullptr;
    petal_ctx* c = new (std::nothrow) petal_ctx();
    if (!c) return PETAL_DEVICE_ERROR;
    char err[512] = {0};
    c->dev = dev_create(device, stream, err, sizeof(err));
    if (!c->dev) {
        std::fprintf(stderr, "petal_ctx_create: %s\n", err);
        delete c;
        return PETAL_DEVICE_ERROR;
    }
    c->force_collective = std::getenv("PETAL_FORCE_COLLECTIVE") != nullptr;   // (the default of PETAL_OPT_FORCE_COLLECTIVE)
    *out = c;
    return PETAL_OK;
}

void petal_ctx_destroy(petal_ctx* ctx) {
    if (!ctx) return;
    try { rccl_release(*ctx); } catch (...) {}
    if (ctx->dev) dev_destroy(ctx->dev);
    delete ctx;
}

int petal_rccl_unique_id(void* out128) {
    if (!out128) return PETAL_INVALID_INPUT;
    try { rccl_unique_id(out128); return PETAL_OK; } catch (const Error& e) { return e.code; } catch (...) { return PETAL_DEVICE_ERROR; }
}

int petal_ctx_init_rccl(petal_ctx* ctx, const void* unique_id128, int rank, int world_size) {
    return guarded(ctx, [&] { rccl_init(*ctx, unique_id128, rank, world_size); });
}

const char* petal_last_error(const petal_ctx* ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

int petal_ctx_set_collective(petal_ctx* ctx, petal_allreduce_fn fn, void* user, int rank, int world_size) {
    return guarded(ctx, [&] {
        if (world_size < 1 || rank < 0 || rank >= world_size) invalid_input("bad rank / world_size");
        if (world_size > 1 && !fn) invalid_input("world_size > 1 needs an all-reduce hook");
        rccl_release(*ctx);
        ctx->allreduce = fn;
        ctx->allreduce_user = user;
        ctx->rank = rank;
        ctx->world = world_size;
    });
}

int petal_ctx_set_profiling(petal_ctx* ctx, int profiling) {
    return guarded(ctx, [&] {
        ctx->profiling = profiling < 0 ? 0 : (profiling > 2 ? 2 : profiling);
        dev_set_profiling(ctx->dev, ctx->profiling);
    });
}

int petal_ctx_collective_info(const petal_ctx* ctx, int* kind, int* rank, int* world_size, int* comm_count, int* comm_device,
                              int* comm_rank) {
    if (!ctx) return PETAL_INVALID_INPUT;
    int cnt = -1, dev = -1, rk = -1;
    petal::rccl_info(*ctx, &cnt, &dev, &rk);
    if (kind) *kind = ctx->rccl ? 2 : (ctx->allreduce ? 1 : 0);
    if (rank) *rank = ctx->rank;
    if (world_size) *world_size = ctx->world;
    if (comm_count) *comm_count = cnt;
    if (comm_device) *comm_device = dev;
    if (comm_rank) *comm_rank = rk;
    return PETAL_OK;
}

int petal_ctx_set_gemm_mode(petal_ctx* ctx, int mode) {
    return guarded(ctx, [&] {
        if (mode != PETAL_GEMM_SPLIT_BF16X3 && mode != PETAL_GEMM_FP32_MFMA && mode != PETAL_GEMM_SPLIT_BF16X3_EXACT) invalid_input("unknown GEMM mode");
        dev_set_gemm_mode(ctx->dev, mode);
    });
}

int petal_ctx_set_option(petal_ctx* ctx, int option, double value) {
    return guarded(ctx, [&] {
        if (option == PETAL_OPT_FORCE_COLLECTIVE) { ctx->force_collective = value != 0; return; }
        if (option == PETAL_OPT_IPCA_FALLBACK) { ctx->ipca_fallback = value != 0; return; }
        if (option == PETAL_OPT_PCA_DUAL) {
            if (!(value == value)) invalid_input("unknown ctx option or NaN value");
            ctx->pca_dual = value > 0 ? 1 : (value < 0 ? -1 : 0);
            return;
        }
        if (option == PETAL_OPT_PCA_DUAL_FALLBACK) { ctx->pca_dual_fallback = value != 0; return; }
        if (option == PETAL_OPT_KPCA_FALLBACK) { ctx->kpca_fallback = value != 0; return; }
        if (option == PETAL_OPT_NMF_FALLBACK) { ctx->nmf_fallback = value != 0; return; }
        if (option < 0 || option >= OPT_COUNT || !(value == value)) invalid_input("unknown ctx option or NaN value");
        dev_set_option(ctx->dev, option, value);
    });
}

int petal_ctx_get_option(const petal_ctx* ctx, int option, double* value) {
    if (!ctx || !value) return PETAL_INVALID_INPUT;
    if (option == PETAL_OPT_FORCE_COLLECTIVE) { *value = ctx->force_collective ? 1.0 : 0.0; return PETAL_OK; }
    if (option == PETAL_OPT_IPCA_FALLBACK) { *value = ctx->ipca_fallback ? 1.0 : 0.0; return PETAL_OK; }
    if (option == PETAL_OPT_PCA_DUAL) { *value = double(ctx->pca_dual); return PETAL_OK; }
    if (option == PETAL_OPT_PCA_DUAL_FALLBACK) { *value = ctx->pca_dual_fallback ? 1.0 : 0.0; return PETAL_OK; }
    if (option == PETAL_OPT_KPCA_FALLBACK) { *value = ctx->kpca_fallback ? 1.0 : 0.0; return PETAL_OK; }
    if (option == PETAL_OPT_NMF_FALLBACK) { *value = ctx->nmf_fallback ? 1.0 : 0.0; return PETAL_OK; }
    if (option < 0 || option >= OPT_COUNT) return PETAL_INVALID_INPUT;
    *value = dev_option(ctx->dev, option);
    return PETAL_OK;
}

int petal_get_stats(const petal_ctx* ctx, petal_stats* out) {
    if (!ctx || !out) return PETAL_INVALID_INPUT;
    *out = ctx->stats;
    return PETAL_OK;
}

int petal_pca_fit(petal_ctx* ctx, const petal_matrix* x, int64_t k, int centering, void* components, void* means,
                  void* singular, void* total_variance, const petal_matrix* y_out) {
    return guarded(ctx, [&] {
        need(x, "x");
        pca_fit(*ctx, *x, k, centering != 0, components, means, singular, total_variance, y_out);
    });
}

int petal_rpca_fit(petal_ctx* ctx, const petal_matrix* x, int64_t k, int64_t n_oversample, int64_t n_iter,
                   int centering, const void* omega, void* components, void* means, void* singular,
                   void* total_variance, const petal_matrix* y_out) {
    return guarded(ctx, [&] {
        need(x, "x");
        rpca_fit(*ctx, *x, k, n_oversample, n_iter, centering != 0, omega, components, means, singular, total_variance,
                 y_out);
    });
}

int petal_transform(petal_ctx* ctx, const petal_matrix* x, const void* components, const void* means, int64_t k,
                    int64_t d, int centering, const petal_matrix* y_out) {
    return guarded(ctx, [&] {
        need(x, "x");
        need(y_out, "y_out");
        transform(*ctx, *x, components, means, k, d, centering != 0, *y_out);
    });
}

int petal_inverse_transform(petal_ctx* ctx, const petal_matrix* y, const void* components, const void* means,
                            int64_t k, int64_t d, int centering, const petal_matrix* x_out) {
    return guarded(ctx, [&] {
        need(y, "y");
        need(x_out, "x_out");
        inverse_transform(*ctx, *y, components, means, k, d, centering != 0, *x_out);
    });
}

int petal_score_rows(petal_ctx* ctx, const petal_matrix* x, const void* components, const void* means, int64_t k, int64_t d,
                     int centering, const void* weights, const petal_matrix* out, const petal_matrix* y_out) {
    return guarded(ctx, [&] {
        need(x, "x");
        need(out, "out");
        score_rows(*ctx, *x, components, means, k, d, centering != 0, weights, *out, y_out);
    });
}

// ---- include/petal_hip_sparse.h: RandomizedPca on a resident CSR matrix ------------------------------------------------------------
int petal_csr_create(petal_ctx* ctx, int64_t rows, int64_t cols, int64_t nnz, const int64_t* indptr, const int32_t* indices,
                     const void* values, int32_t dtype, petal_csr** out) {
    if (out) *out = nullptr;
    return guarded(ctx, [&] {
        need(out, "out");
        *out = csr_create(*ctx, rows, cols, nnz, indptr, indices, values, dtype);
    });
}
void petal_csr_destroy(petal_csr* x) {
    if (!x) return;
    try {
        DeviceScope scope(x->owner->dev);
        csr_destroy(x);
    } catch (...) {}
}
int petal_csr_info(const petal_csr* x, int64_t* out8) {
    if (!x || !out8) return PETAL_INVALID_INPUT;
    const int64_t items[2] = {x->resident ? x->dev[0].n_items : int64_t(x->host[0].items.size()),
                              x->resident ? x->dev[1].n_items : int64_t(x->host[1].items.size())};
    const int64_t v[8] = {x->rows, x->cols, x->nnz, x->dtype, x->resident ? 1 : 0, items[0], items[1], PETAL_CSR_ITEM_NNZ};
    for (int i = 0; i < 8; ++i) out8[i] = v[i];
    return PETAL_OK;
}
int petal_csr_image(const petal_csr* x, int transposed, int64_t* indptr, int32_t* indices, void* values, int64_t* items) {
    if (!x) return PETAL_INVALID_INPUT;
    return guarded(x->owner, [&] { csr_image(*x, transposed, indptr, indices, values, items); });
}
int petal_rpca_fit_csr(petal_ctx* ctx, const petal_csr* x, int64_t k, int64_t n_oversample, int64_t n_iter, int centering,
                       const void* omega, void* components, void* means, void* singular, void* total_variance,
                       const petal_matrix* y_out, int64_t* kernel_path) {
    return guarded(ctx, [&] {
        need(x, "x");
        rpca_fit_csr(*ctx, *x, k, n_oversample, n_iter, centering != 0, omega, components, means, singular, total_variance, y_out, kernel_path);
    });
}
int petal_transform_csr(petal_ctx* ctx, const petal_csr* x, const void* components, const void* means, int64_t k, int64_t d,
                        int centering, const petal_matrix* y_out, int64_t* kernel_path) {
    return guarded(ctx, [&] {
        need(x, "x");
        need(y_out, "y_out");
        transform_csr(*ctx, *x, components, means, k, d, centering != 0, *y_out, kernel_path);
    });
}
int petal_ctx_workspace_in_use(petal_ctx* ctx, int64_t* blocks, int64_t* bytes) {
    return guarded(ctx, [&] {
        need(blocks, "blocks");
        need(bytes, "bytes");
        if (!dev_live(ctx->dev, blocks, bytes)) { *blocks = -1; *bytes = -1; }
    });
}
int petal_csr_gemm(petal_ctx* ctx, const petal_csr* x, int transposed, const double* P, int64_t N, const double* a, const double* s,
                   double* out) {
    return guarded(ctx, [&] {
        need(x, "x");
        csr_gemm(*ctx, *x, transposed != 0, P, N, a, s, out);
    });
}

// ---- include/petal_hip_ipca.h: IncrementalPca --------------------------------------------------------------------------------------
int petal_ipca_create(petal_ctx* ctx, int64_t d, int32_t dtype, int centering, petal_ipca** out) {
    if (out) *out = nullptr;
    return guarded(ctx, [&] {
        need(out, "out");
        *out = ipca_create(*ctx, d, dtype, centering != 0);
    });
}
void petal_ipca_destroy(petal_ipca* h) {
    if (!h) return;
    try {
        DeviceScope scope(h->owner->dev);
        ipca_destroy(h);
    } catch (...) {}
}
int petal_ipca_reset(petal_ipca* h) {
    if (!h) return PETAL_INVALID_INPUT;
    return guarded(h->owner, [&] { ipca_reset(*h); });
}
int petal_ipca_partial_fit(petal_ctx* ctx, petal_ipca* h, const petal_matrix* x) {
    return guarded(ctx, [&] {
        need(h, "handle");
        need(x, "x");
        ipca_partial_fit(*ctx, *h, *x);
    });
}
int petal_ipca_merge(petal_ctx* ctx, petal_ipca* into, const petal_ipca* other) {
    return guarded(ctx, [&] {
        need(into, "into");
        need(other, "other");
        ipca_merge(*ctx, *into, *other);
    });
}
int petal_ipca_finalize(petal_ctx* ctx, const petal_ipca* h, int64_t k, void* components, void* means, void* singular,
                        void* total_variance) {
    return guarded(ctx, [&] {
        need(h, "handle");
        ipca_finalize(*ctx, *h, k, components, means, singular, total_variance);
    });
}
int petal_ipca_info(const petal_ipca* h, int64_t* out8) {
    if (!h || !out8) return PETAL_INVALID_INPUT;
    const int64_t v[8] = {h->d, h->dtype, h->centering ? 1 : 0, int64_t(h->n), h->batches, h->kernel_batches, h->merges, 0};
    for (int i = 0; i < 8; ++i) out8[i] = v[i];
    return PETAL_OK;
}
int petal_ipca_get_state(petal_ctx* ctx, const petal_ipca* h, double* n, double* mean_d, double* m2_dxd) {
    return guarded(ctx, [&] {
        need(h, "handle");
        ipca_get_state(*ctx, *h, n, mean_d, m2_dxd);
    });
}
int petal_ipca_set_state(petal_ctx* ctx, petal_ipca* h, double n, const double* mean_d, const double* m2_dxd) {
    return guarded(ctx, [&] {
        need(h, "handle");
        ipca_set_state(*ctx, *h, n, mean_d, m2_dxd);
    });
}

// ---- include/petal_hip_wide.h: exact Pca on wide data --------------------------------------------------------------------------------
int petal_pca_last_route(petal_ctx* ctx, int64_t* out4) {
    if (!ctx || !out4) return PETAL_INVALID_INPUT;
    for (int i = 0; i < 4; ++i) out4[i] = ctx->pca_route[i];
    return PETAL_OK;
}
int petal_row_gram(petal_ctx* ctx, const petal_matrix* x, const double* centre, double* out, int64_t* info2) {
    return guarded(ctx, [&] {
        need(x, "x");
        row_gram(*ctx, *x, centre, out, info2);
    });
}

// ---- include/petal_hip_kpca.h: KernelPca ---------------------------------------------------------------------------------------------
int petal_kpca_fit(petal_ctx* ctx, const petal_matrix* x, int64_t k, const petal_kernel_spec* spec, petal_kpca** out,
                   const petal_matrix* y_out) {
    if (out) *out = nullptr;
    return guarded(ctx, [&] {
        need(x, "x");
        need(spec, "spec");
        need(out, "out");
        *out = kpca_fit(*ctx, *x, k, KernelSpec{spec->kernel, spec->degree, spec->gamma, spec->coef0}, y_out);
    });
}
void petal_kpca_destroy(petal_kpca* h) {
    if (!h) return;
    try {
        DeviceScope scope(h->owner->dev);
        kpca_destroy(h);
    } catch (...) {}
}
int petal_kpca_transform(petal_ctx* ctx, petal_kpca* h, const petal_matrix* x, const petal_matrix* y_out) {
    return guarded(ctx, [&] {
        need(h, "handle");
        need(x, "x");
        need(y_out, "y_out");
        kpca_transform(*ctx, *h, *x, *y_out);
    });
}
int petal_kpca_get(const petal_kpca* h, double* eigenvalues, double* scaled_vectors, int64_t* info8) {
    if (!h) return PETAL_INVALID_INPUT;
    return guarded(h->owner, [&] { kpca_get(*h, eigenvalues, scaled_vectors, info8); });
}
int petal_kernel_apply(petal_ctx* ctx, const petal_matrix* xq, const petal_matrix* xt, const petal_kernel_spec* spec, const double* a,
                       int64_t cols, const double* centre, double* out, int64_t* info1) {
    return guarded(ctx, [&] {
        need(xq, "xq");
        need(xt, "xt");
        need(spec, "spec");
        kernel_apply(*ctx, *xq, *xt, KernelSpec{spec->kernel, spec->degree, spec->gamma, spec->coef0}, a, cols, centre, out, info1);
    });
}

// ---- include/petal_hip_nmf.h: Nmf ---------------------------------------------------------------------------------------------------
namespace {
NmfSpec nmf_spec(const petal_nmf_spec& s) { return NmfSpec{s.max_iter, s.tol, s.l1_w, s.l2_w, s.l1_h, s.l2_h}; }
}  // namespace
int petal_nmf_fit(petal_ctx* ctx, const petal_matrix* x, int64_t k, const petal_nmf_spec* spec, const petal_matrix* w0, const petal_matrix* h0,
                  int64_t seed, petal_nmf** out, const petal_matrix* w_out) {
    if (out) *out = nullptr;
    return guarded(ctx, [&] {
        need(x, "x");
        need(spec, "spec");
        need(out, "out");
        *out = nmf_fit(*ctx, *x, k, nmf_spec(*spec), w0, h0, seed, w_out);
    });
}
void petal_nmf_destroy(petal_nmf* h) {
    if (!h) return;
    try {
        DeviceScope scope(h->owner->dev);
        nmf_destroy(h);
    } catch (...) {}
}
int petal_nmf_transform(petal_ctx* ctx, petal_nmf* h, const petal_matrix* x, const petal_matrix* w_out) {
    return guarded(ctx, [&] {
        need(h, "handle");
        need(x, "x");
        need(w_out, "w_out");
        nmf_transform(*ctx, *h, *x, *w_out);
    });
}
int petal_nmf_inverse_transform(petal_ctx* ctx, petal_nmf* h, const petal_matrix* w, const petal_matrix* x_out) {
    return guarded(ctx, [&] {
        need(h, "handle");
        need(w, "w");
        need(x_out, "x_out");
        nmf_inverse_transform(*ctx, *h, *w, *x_out);
    });
}
int petal_nmf_get(const petal_nmf* h, double* components, int64_t* info6, double* err2) {
    if (!h) return PETAL_INVALID_INPUT;
    return guarded(h->owner, [&] { nmf_get(*h, components, info6, err2); });
}
int petal_nmf_pass(petal_ctx* ctx, const petal_matrix* x, int64_t k, const double* w_in, const double* h, const petal_nmf_spec* spec, int64_t inner_iters,
                   double* w_out, double* a_out, double* b_out, int64_t* info1) {
    return guarded(ctx, [&] {
        need(x, "x");
        need(w_in, "w_in");
        need(h, "h");
        need(spec, "spec");
        need(w_out, "w_out");
        nmf_pass(*ctx, *x, k, w_in, h, nmf_spec(*spec), inner_iters, w_out, a_out, b_out, info1);
    });
}

// ---- include/petal_hip_nmf_sparse.h: Nmf on a resident CSR matrix -----------------------------------------------------------------
int petal_nmf_fit_csr(petal_ctx* ctx, const petal_csr* x, int64_t k, const petal_nmf_spec* spec, const petal_matrix* w0, const petal_matrix* h0,
                      int64_t seed, petal_nmf** out, const petal_matrix* w_out, int64_t* kernel_path) {
    if (out) *out = nullptr;
    return guarded(ctx, [&] {
        need(x, "x");
        need(spec, "spec");
        need(out, "out");
        *out = nmf_fit_csr(*ctx, *x, k, nmf_spec(*spec), w0, h0, seed, w_out, kernel_path);
    });
}
int petal_nmf_transform_csr(petal_ctx* ctx, petal_nmf* h, const petal_csr* x, const petal_matrix* w_out, int64_t* kernel_path) {
    return guarded(ctx, [&] {
        need(h, "handle");
        need(x, "x");
        need(w_out, "w_out");
        nmf_transform_csr(*ctx, *h, *x, *w_out, kernel_path);
    });
}
int petal_nmf_sweep_csr(petal_ctx* ctx, const petal_csr* x, int transposed, int64_t k, const double* g_in, const double* f,
                        const petal_nmf_spec* spec, int64_t inner_iters, double* g_out, double* gram_out, double* dot_out, int64_t* info1) {
    return guarded(ctx, [&] {
        need(x, "x");
        need(g_in, "g_in");
        need(f, "f");
        need(spec, "spec");
        need(g_out, "g_out");
        nmf_sweep_csr(*ctx, *x, transposed != 0, k, g_in, f, nmf_spec(*spec), inner_iters, g_out, gram_out, dot_out, info1);
    });
}

// ---- include/petal_hip_nmf_kl.h: the Kullback-Leibler loss on a resident CSR matrix ------------------------------------------------
int petal_nmf_fit_csr_loss(petal_ctx* ctx, const petal_csr* x, int64_t k, const petal_nmf_spec* spec, int64_t loss, const petal_matrix* w0,
                           const petal_matrix* h0, int64_t seed, petal_nmf** out, const petal_matrix* w_out, int64_t* kernel_path) {
    if (out) *out = nullptr;
    return guarded(ctx, [&] {
        need(x, "x");
        need(spec, "spec");
        need(out, "out");
        *out = nmf_fit_csr_loss(*ctx, *x, k, nmf_spec(*spec), loss, w0, h0, seed, w_out, kernel_path);
    });
}
int petal_nmf_get_loss(const petal_nmf* h, int64_t* loss) {
    if (!h || !loss) return PETAL_INVALID_INPUT;
    *loss = h->loss;
    return PETAL_OK;
}
int petal_nmf_kl_sweep_csr(petal_ctx* ctx, const petal_csr* x, int transposed, int64_t k, const double* g_in, const double* f,
                           const petal_nmf_spec* spec, int64_t inner_iters, double* g_out, double* colsum_out, double* term_out, int64_t* info1) {
    return guarded(ctx, [&] {
        need(x, "x");
        need(g_in, "g_in");
        need(f, "f");
        need(spec, "spec");
        need(g_out, "g_out");
        nmf_kl_sweep_csr(*ctx, *x, transposed != 0, k, g_in, f, nmf_spec(*spec), inner_iters, g_out, colsum_out, term_out, info1);
    });
}

// ---- include/petal_hip_nmf_kl_dense.h: the Kullback-Leibler loss on a dense matrix ---------------------------------------------------
int petal_nmf_fit_loss(petal_ctx* ctx, const petal_matrix* x, int64_t k, const petal_nmf_spec* spec, int64_t loss, const petal_matrix* w0,
                       const petal_matrix* h0, int64_t seed, petal_nmf** out, const petal_matrix* w_out) {
    if (out) *out = nullptr;
    return guarded(ctx, [&] {
        need(x, "x");
        need(spec, "spec");
        need(out, "out");
        *out = nmf_fit_loss(*ctx, *x, k, nmf_spec(*spec), loss, w0, h0, seed, w_out);
    });
}
int petal_nmf_transform_loss(petal_ctx* ctx, petal_nmf* h, const petal_matrix* x, const petal_matrix* w_out) {
    return guarded(ctx, [&] {
        need(h, "handle");
        need(x, "x");
        need(w_out, "w_out");
        nmf_transform_loss(*ctx, *h, *x, *w_out);
    });
}
int petal_nmf_kl_pass(petal_ctx* ctx, const petal_matrix* x, int64_t k, const double* w_in, const double* h, const petal_nmf_spec* spec,
                      int64_t inner_iters, double* w_out, double* a_out, double* colsum_out, double* term_out, int64_t* info1) {
    return guarded(ctx, [&] {
        need(x, "x");
        need(w_in, "w_in");
        need(h, "h");
        need(spec, "spec");
        need(w_out, "w_out");
        nmf_kl_pass(*ctx, *x, k, w_in, h, nmf_spec(*spec), inner_iters, w_out, a_out, colsum_out, term_out, info1);
    });
}

// ---- include/petal_hip_nmf_cd.h: the coordinate-descent solver on a dense matrix ------------------------------------------------------
int petal_nmf_fit_solver(petal_ctx* ctx, const petal_matrix* x, int64_t k, const petal_nmf_spec* spec, int64_t solver, const petal_matrix* w0,
                         const petal_matrix* h0, int64_t seed, petal_nmf** out, const petal_matrix* w_out) {
    if (out) *out = nullptr;
    return guarded(ctx, [&] {
        need(x, "x");
        need(spec, "spec");
        need(out, "out");
        *out = nmf_fit_solver(*ctx, *x, k, nmf_spec(*spec), solver, w0, h0, seed, w_out);
    });
}
int petal_nmf_get_solver(const petal_nmf* h, int64_t* solver) {
    if (!h || !solver) return PETAL_INVALID_INPUT;
    *solver = h->solver;
    return PETAL_OK;
}
int petal_nmf_cd_pass(petal_ctx* ctx, const petal_matrix* x, int64_t k, const double* w_in, const double* h, const petal_nmf_spec* spec,
                      int64_t inner_iters, int from_zero, double* w_out, double* a_out, double* b_out, double* violation_out, int64_t* info1) {
    return guarded(ctx, [&] {
        need(x, "x");
        need(w_in, "w_in");
        need(h, "h");
        need(spec, "spec");
        need(w_out, "w_out");
        nmf_cd_pass(*ctx, *x, k, w_in, h, nmf_spec(*spec), inner_iters, from_zero != 0, w_out, a_out, b_out, violation_out, info1);
    });
}
int petal_nmf_cd_hupdate(petal_ctx* ctx, int64_t k, int64_t d, const double* a, const double* b, const double* h_in, const petal_nmf_spec* spec,
                         double* h_out, double* violation_out, int64_t* info1) {
    return guarded(ctx, [&] {
        need(a, "a");
        need(b, "b");
        need(h_in, "h_in");
        need(spec, "spec");
        need(h_out, "h_out");
        nmf_cd_hupdate(*ctx, k, d, a, b, h_in, nmf_spec(*spec), h_out, violation_out, info1);
    });
}

// ---- include/petal_hip_nmf_cd_sparse.h: the coordinate-descent solver on a resident CSR matrix ------------------------------------------
int petal_nmf_fit_csr_solver(petal_ctx* ctx, const petal_csr* x, int64_t k, const petal_nmf_spec* spec, int64_t solver, const petal_matrix* w0,
                             const petal_matrix* h0, int64_t seed, petal_nmf** out, const petal_matrix* w_out, int64_t* kernel_path) {
    if (out) *out = nullptr;
    return guarded(ctx, [&] {
        need(x, "x");
        need(spec, "spec");
        need(out, "out");
        *out = nmf_fit_csr_solver(*ctx, *x, k, nmf_spec(*spec), solver, w0, h0, seed, w_out, kernel_path);
    });
}
int petal_nmf_transform_csr_solver(petal_ctx* ctx, petal_nmf* h, const petal_csr* x, const petal_matrix* w_out, int64_t* kernel_path) {
    return guarded(ctx, [&] {
        need(h, "handle");
        need(x, "x");
        need(w_out, "w_out");
        nmf_transform_csr_solver(*ctx, *h, *x, *w_out, kernel_path);
    });
}
int petal_nmf_cd_sweep_csr(petal_ctx* ctx, const petal_csr* x, int transposed, int64_t k, const double* g_in, const double* f,
                           const petal_nmf_spec* spec, int64_t inner_iters, int from_zero, double* g_out, double* gram_out, double* dot_out,
                           double* violation_out, int64_t* info1) {
    return guarded(ctx, [&] {
        need(x, "x");
        need(g_in, "g_in");
        need(f, "f");
        need(spec, "spec");
        need(g_out, "g_out");
        nmf_cd_sweep_csr(*ctx, *x, transposed != 0, k, g_in, f, nmf_spec(*spec), inner_iters, from_zero != 0, g_out, gram_out, dot_out,
                         violation_out, info1);
    });
}

// ---- include/petal_hip_segments.h: one exact Pca per row segment ------------------------------------------------------------------
int petal_pca_fit_segments(petal_ctx* ctx, const petal_matrix* x, const int64_t* offsets, int64_t n_segments, int64_t k, int centering,
                           void* components, void* means, void* singular, void* total_variance, int32_t* status,
                           const petal_matrix* y_out, int64_t* kernel_segments) {
    return guarded(ctx, [&] {
        need(x, "x");
        need(offsets, "offsets");
        pca_fit_segments(*ctx, *x, offsets, n_segments, k, centering != 0, components, means, singular, total_variance, status, y_out,
                         kernel_segments);
    });
}

int petal_transform_segments(petal_ctx* ctx, const petal_matrix* x, const int64_t* offsets, int64_t n_segments, const void* components,
                             const void* means, int64_t k, int64_t d, int centering, const petal_matrix* y_out) {
    return guarded(ctx, [&] {
        need(x, "x");
        need(offsets, "offsets");
        need(y_out, "y_out");
        transform_segments(*ctx, *x, offsets, n_segments, components, means, k, d, centering != 0, *y_out);
    });
}

int petal_inverse_transform_segments(petal_ctx* ctx, const petal_matrix* y, const int64_t* offsets, int64_t n_segments,
                                     const void* components, const void* means, int64_t k, int64_t d, int centering,
                                     const petal_matrix* x_out) {
    return guarded(ctx, [&] {
        need(y, "y");
        need(offsets, "offsets");
        need(x_out, "x_out");
        inverse_transform_segments(*ctx, *y, offsets, n_segments, components, means, k, d, centering != 0, *x_out);
    });
}

int petal_fastica_fit(petal_ctx* ctx, const petal_matrix* x, int64_t n_components, double tol, int64_t max_iter,
                      int mode, const void* w_init, void* components, void* means, int64_t* n_iter,
                      const petal_matrix* y_out) {
    return guarded(ctx, [&] {
        need(x, "x");
        fastica_fit(*ctx, *x, n_components, tol, max_iter, mode, w_init, components, means, n_iter, y_out);
    });
}

int petal_ica_par(petal_ctx* ctx, const petal_matrix* x1, double tol, int64_t max_iter, int mode, const void* w_init,
                  void* w_out, int64_t* n_iter) {
    return guarded(ctx, [&] {
        need(x1, "x1");
        need(w_init, "w_init");
        need(w_out, "w_out");
        ica_par(*ctx, *x1, tol, max_iter, mode, w_init, w_out, n_iter);
    });
}

int petal_symmetric_decorrelation(petal_ctx* ctx, const void* w, int64_t nc, int32_t dtype, int mode, void* out) {
    return guarded(ctx, [&] {
        need(w, "w");
        need(out, "out");
        symmetric_decorrelation(*ctx, w, nc, dtype, mode, out);
    });
}

int petal_logcosh(petal_ctx* ctx, const petal_matrix* x, const petal_matrix* g_out, void* gprime_out) {
    return guarded(ctx, [&] {
        need(x, "x");
        need(g_out, "g_out");
        need(gprime_out, "gprime_out");
        logcosh(*ctx, *x, *g_out, gprime_out);
    });
}

int petal_svd_flip(petal_ctx* ctx, const petal_matrix* u, const petal_matrix* vt) {
    return guarded(ctx, [&] {
        need(u, "u");
        need(vt, "vt");
        svd_flip(*ctx, *u, *vt);
    });
}

int petal_gemm_xp(petal_ctx* ctx, const petal_matrix* x, const void* mu, const void* p, int64_t N, const void* bias,
                  const petal_matrix* z_out) {
    return guarded(ctx, [&] {
        need(x, "x");
        need(p, "p");
        need(z_out, "z_out");
        gemm_xp(*ctx, *x, mu, p, N, bias, *z_out);
    });
}

int petal_power_pass(petal_ctx* ctx, const petal_matrix* x, const void* mu, const void* p, int64_t N, double* y_out,
                     const petal_matrix* z_out, int* fused_out) {
    return guarded(ctx, [&] {
        need(x, "x");
        need(p, "p");
        need(y_out, "y_out");
        power_pass(*ctx, *x, mu, p, N, y_out, z_out, fused_out);
    });
}

int petal_gemm_atb(petal_ctx* ctx, const petal_matrix* a, const void* mu_a, const petal_matrix* b, const void* mu_b,
                   double* c_out) {
    return guarded(ctx, [&] {
        need(a, "a");
        need(c_out, "c_out");
        gemm_atb(*ctx, *a, mu_a, b, mu_b, c_out);
    });
}

// ---- include/petal_hip_probe.h: test aids ---------------------------------------------------------------------------------------
int petal_probe_chol(petal_ctx* ctx, const double* G, int64_t L, int64_t ldg, double rel_tol, int64_t Lz, int64_t ndead_cols, int route,
                     const double* B, int64_t b_rows, int64_t b_cols, int64_t ldb, double* out, int64_t ldo, int* ndead, int* rt) {
    return guarded(ctx, [&] {
        need(G, "G");
        need(out, "out");
        need(ndead, "ndead");
        need(rt, "rt");
        probe_chol(*ctx, G, L, ldg, rel_tol, Lz, ndead_cols, route, B, b_rows, b_cols, ldb, out, ldo, ndead, rt);
    });
}

int petal_probe_eigh(petal_ctx* ctx, const double* A, int64_t L, int64_t lda, double tol_rel, int clustered, int64_t Lz, int64_t ncheck,
                     int verdict_mode, int verdict_in, double gap_tol_override, double* w, double* V, int64_t ldv, int* verdict_out) {
    return guarded(ctx, [&] {
        need(A, "A");
        need(w, "w");
        need(V, "V");
        need(verdict_out, "verdict_out");
        probe_eigh(*ctx, A, L, lda, tol_rel, clustered != 0, Lz, ncheck, verdict_mode, verdict_in, gap_tol_override, w, V, ldv, verdict_out);
    });
}

int petal_probe_jacobi_svd_rows(petal_ctx* ctx, const double* A, int64_t L, int64_t lda, double* U, int64_t ldu, double* s_inv,
                                int* nonconv) {
    return guarded(ctx, [&] {
        need(A, "A");
        need(U, "U");
        need(s_inv, "s_inv");
        need(nonconv, "nonconv");
        probe_jacobi_svd_rows(*ctx, A, L, lda, U, ldu, s_inv, nonconv);
    });
}

int petal_probe_dgemm(petal_ctx* ctx, int ta, int tb, int64_t M, int64_t N, int64_t K, double alpha, const double* A, int64_t lda,
                      const double* B, int64_t ldb, double beta, double* C, int64_t ldc, const double* colscale) {
    return guarded(ctx, [&] {
        need(A, "A");
        need(B, "B");
        need(C, "C");
        probe_dgemm(*ctx, ta != 0, tb != 0, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc, colscale);
    });
}

int petal_probe_ritz_residual(petal_ctx* ctx, const double* CV, int64_t ldc, const double* Vr, int64_t ldv, int64_t rows, int64_t nc,
                              const double* theta, const int* flag, const int* flag2, double* out3, double* w_out, int64_t w_len) {
    return guarded(ctx, [&] {
        need(CV, "CV");
        need(Vr, "Vr");
        if (nc > 0) need(theta, "theta");
        need(out3, "out3");
        need(w_out, "w_out");
        probe_ritz_residual(*ctx, CV, ldc, Vr, ldv, rows, nc, theta, flag, flag2, out3, w_out, w_len);
    });
}

int petal_probe_topk_eigh(petal_ctx* ctx, const double* C, int64_t d, int64_t ldc, int64_t nc, int32_t dtype, int mode, int* delivered,
                          double* w, double* V, int64_t ldv, int* checks, double* r3, int* verdict, double* diag) {
    return guarded(ctx, [&] {
        need(C, "C");
        need(delivered, "delivered");
        need(w, "w");
        need(V, "V");
        need(checks, "checks");
        need(r3, "r3");
        need(verdict, "verdict");
        probe_topk_eigh(*ctx, C, d, ldc, nc, dtype, mode, delivered, w, V, ldv, checks, r3, verdict, diag);
    });
}

int petal_probe_power_pass_means(petal_ctx* ctx, const void* X, int32_t dtype, int64_t n, int64_t K, int64_t d, int64_t ldx, const double* P,
                                 int64_t N, int64_t ldp, int64_t L, int* done, double* Y, int64_t ldy, double* mu64, double* muT, double* mu0,
                                 double* tv) {
    return guarded(ctx, [&] {
        need(X, "X");
        need(P, "P");
        need(done, "done");
        need(Y, "Y");
        need(mu64, "mu64");
        need(muT, "muT");
        need(mu0, "mu0");
        need(tv, "tv");
        probe_power_pass_means(*ctx, X, dtype, n, K, d, ldx, P, N, ldp, L, done, Y, ldy, mu64, muT, mu0, tv);
    });
}

int petal_probe_rebase(petal_ctx* ctx, const void* X, int32_t dtype, int64_t n, int64_t K, int64_t ldx, const void* mu, const double* G,
                       int64_t L, int64_t ldg, double rel_tol, const double* A, int64_t M, int64_t lda, int p_planes, int steering, int route,
                       int* done, double* P_out, int64_t ldpo, double* Z, int64_t ldz, double* Y, int64_t ldy, int* ndead) {
    return guarded(ctx, [&] {
        need(X, "X");
        need(G, "G");
        need(A, "A");
        need(done, "done");
        need(P_out, "P_out");
        need(ndead, "ndead");
        probe_rebase(*ctx, X, dtype, n, K, ldx, mu, G, L, ldg, rel_tol, A, M, lda, p_planes, steering != 0, route, done, P_out, ldpo, Z, ldz, Y,
                     ldy, ndead);
    });
}

}  // extern "C"

// ctx.h -- petal_ctx and small host-side helpers shared by algo.cpp / api.cpp.
#pragma once
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/petal_hip.h"
#include "ops.h"

struct petal_ctx {
    petal::Dev* dev = nullptr;
    std::string err;
    petal_allreduce_fn allreduce = nullptr;
    void* allreduce_user = nullptr;
    int rank = 0, world = 1;
    int profiling = 0;
    bool ipca_fallback = false;      // PETAL_OPT_IPCA_FALLBACK (include/petal_hip_ipca.h): a test aid
    int pca_dual = 0;                // PETAL_OPT_PCA_DUAL (include/petal_hip_wide.h): 0 the auto rule, 1 always (non-sharded), -1 never
    bool pca_dual_fallback = false;  // PETAL_OPT_PCA_DUAL_FALLBACK: a test aid
    int64_t pca_route[4] = {0, 0, 0, 0};   // petal_pca_last_route: route, kernel, order of the eigenproblem, feature chunks
    bool kpca_fallback = false;      // PETAL_OPT_KPCA_FALLBACK (include/petal_hip_kpca.h): a test aid
    bool nmf_fallback = false;       // PETAL_OPT_NMF_FALLBACK (include/petal_hip_nmf.h): a test aid
    bool force_collective = false;   // PETAL_OPT_FORCE_COLLECTIVE (default: env PETAL_FORCE_COLLECTIVE at petal_ctx_create)
    petal_stats stats{};
    void* rccl = nullptr;  // the built-in RCCL communicator (rccl.cpp), when petal_ctx_init_rccl installed it
    // the fixed pseudo-random start block of the subspace iteration (topk_eigh), kept on the device per shape: generating it on the
    // host and uploading it cost 20 us of idle device per exact Pca / FastICA fit
    double* topk_seed = nullptr;
    int64_t topk_seed_d = 0, topk_seed_dp = 0, topk_seed_p = 0;
};

// include/petal_hip_sparse.h: a sparse matrix and its transposed image with their work items, in device memory (resident) or, where the
// device-op layer has no sparse product, on the host
struct petal_csr {
    petal_ctx* owner = nullptr;
    int64_t rows = 0, cols = 0, nnz = 0;
    int dtype = 0;
    bool resident = false;
    struct Image {                       // [0] the matrix, [1] its transpose
        std::vector<int64_t> ptr;        // image rows + 1 (host only)
        std::vector<int32_t> idx;
        std::vector<char> val;
        std::vector<petal::CsrItem> items;
        std::vector<petal::CsrSplit> splits;
        int64_t n_slots = 0;
    } host[2];
    petal::CsrImage dev[2];              // resident: views of the four device blocks of each image
    void* blocks[2][4] = {{nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}};
};

// include/petal_hip_ipca.h: the running statistic of an IncrementalPca, resident with its ctx
struct petal_ipca {
    petal_ctx* owner = nullptr;
    int64_t d = 0, dp = 0;
    int dtype = 0;
    bool centering = true;
    double n = 0;                        // rows seen (the one part of the statistic that lives on the host)
    int64_t batches = 0, kernel_batches = 0, merges = 0;
    double* mean = nullptr;              // device fp64, dp (zero when centering is off)
    double* m2 = nullptr;                // device fp64, dp x dp, symmetric, both triangles
};

// include/petal_hip_kpca.h: a fitted KernelPca, resident with its ctx
struct petal_kpca {
    petal_ctx* owner = nullptr;
    int64_t n = 0, d = 0, dp = 0, k = 0, lda = 0;
    int dtype = 0, kernel = 0, degree = 3;
    double gamma = 0, coef0 = 1;         // as resolved at the fit (gamma <= 0 -> 1 / d)
    int64_t fit_kernel = 0, last_kernel = -1, order = 0, topk = 0;   // topk: gram_eigen's top-k subspace iteration delivered the eigenpairs (0: the full eigen-solver ran)
    void* xt = nullptr;                  // device, n x dp in dtype (ld = dp): the model's OWN copy of the training rows
    double* cen = nullptr;               // device fp64, dp: the centre c (zeros unless rbf)
    double* diag = nullptr;              // device fp64, n: diag(G) = |x_i - c|^2
    double* a = nullptr;                 // device fp64, round_up(n, 32) x lda: A' = [V lambda^(-1/2) | 1], zero padded
    double* epi = nullptr;               // device fp64, n + 1 + 2 lda: [rbar | tbar | rbar^T A' | 1^T A']
    double tbar = 0;
    std::vector<double> lam;             // k eigenvalues, as computed
};

// include/petal_hip_nmf.h: a fitted Nmf, resident with its ctx
struct petal_nmf {
    petal_ctx* owner = nullptr;
    int64_t n = 0, d = 0, dp = 0, k = 0, kp = 0, max_iter = 0, n_iter = 0;
    int dtype = 0;
    double l1_w = 0, l2_w = 0;
    int64_t fit_kernel = 0, last_kernel = -1;
    int64_t loss = 0;                    // PETAL_NMF_LOSS_FROBENIUS / PETAL_NMF_LOSS_KL (include/petal_hip_nmf_kl.h)
    int64_t solver = 0;                  // PETAL_NMF_SOLVER_MU / PETAL_NMF_SOLVER_CD (include/petal_hip_nmf_cd.h)
    double err = 0, err_init = 0;
    double* h = nullptr;                 // device fp64, kp x dp (ld dp): H, zero in the padding
    double* hht = nullptr;               // device fp64, kp x kp: H H^T (zeros in a Kullback-Leibler model, which never reads it)
};

namespace petal {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
[[noreturn]] inline void invalid_input(const std::string& m) { throw Error(PETAL_INVALID_INPUT, m); }
[[noreturn]] inline void linalg_error(const std::string& m) { throw Error(PETAL_LINALG_ERROR, m); }
[[noreturn]] inline void device_error(const std::string& m) { throw Error(PETAL_DEVICE_ERROR, m); }

inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }

// true when the fit must take the sharded code path: several ranks, or PETAL_OPT_FORCE_COLLECTIVE with a collective
// installed (runs the complete multi-rank path -- packing kernels, all-reduces -- on a one-rank group: test / timing aid)
inline bool sharded(const petal_ctx& c) {
    return c.world > 1 || (c.allreduce != nullptr && c.force_collective);
}

// rccl.cpp: the built-in collective
void rccl_unique_id(void* out128);
void rccl_init(petal_ctx& c, const void* unique_id128, int rank, int world);
void rccl_release(petal_ctx& c);
void rccl_info(const petal_ctx& c, int* count, int* device, int* rank);

// RAII device buffer from the ctx's caching allocator
struct DBuf {
    Dev* dev = nullptr;
    void* p = nullptr;
    size_t bytes = 0;
    DBuf() = default;
    DBuf(Dev* d, size_t b) : dev(d), p(b ? dev_alloc(d, b) : nullptr), bytes(b) {}
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
    DBuf(DBuf&& o) noexcept : dev(o.dev), p(o.p), bytes(o.bytes) { o.p = nullptr; }
    DBuf& operator=(DBuf&& o) noexcept {
        if (this != &o) { release(); dev = o.dev; p = o.p; bytes = o.bytes; o.p = nullptr; }
        return *this;
    }
    ~DBuf() { release(); }
    void release() { if (p) dev_free(dev, p); p = nullptr; }
    double* f64() const { return static_cast<double*>(p); }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

// a row-major matrix in device memory, K-dimension padded to a multiple of 16 with zeros
struct DevMat {
    const void* p = nullptr;
    int64_t n = 0, d = 0, dp = 0, ld = 0;  // rows, real cols, padded cols, leading dimension (elements)
    int dtype = F32;
    DBuf owned;                             // empty when zero-copy
    bool zero_copy = false;                 // the caller's device buffer is streamed in place
};

// host algorithms (algo.cpp)
DevMat ingest(petal_ctx& c, const petal_matrix& x);
void   emit(petal_ctx& c, int dtype, const void* src, int64_t n, int64_t cols, int64_t ld, const petal_matrix& out, const double* scale = nullptr);   // scale: device, cols doubles (per-column factor on the way out)
void   allreduce_f64(petal_ctx& c, double* dev_buf, int64_t count, int op);

void rpca_fit(petal_ctx& c, const petal_matrix& x, int64_t k, int64_t n_oversample, int64_t n_iter, bool centering,
              const void* omega, void* components, void* means, void* singular, void* total_variance,
              const petal_matrix* y_out);
void pca_fit(petal_ctx& c, const petal_matrix& x, int64_t k, bool centering, void* components, void* means,
             void* singular, void* total_variance, const petal_matrix* y_out);
void transform(petal_ctx& c, const petal_matrix& x, const void* components, const void* means, int64_t k, int64_t d,
               bool centering, const petal_matrix& y_out);
void score_rows(petal_ctx& c, const petal_matrix& x, const void* components, const void* means, int64_t k, int64_t d, bool centering,
                const void* weights, const petal_matrix& out, const petal_matrix* y_out);
void inverse_transform(petal_ctx& c, const petal_matrix& y, const void* components, const void* means, int64_t k,
                       int64_t d, bool centering, const petal_matrix& x_out);
// include/petal_hip_segments.h: one exact Pca per row segment
void pca_fit_segments(petal_ctx& c, const petal_matrix& x, const int64_t* offsets, int64_t n_segments, int64_t k, bool centering,
                      void* components, void* means, void* singular, void* total_variance, int32_t* status, const petal_matrix* y_out,
                      int64_t* kernel_segments);
void transform_segments(petal_ctx& c, const petal_matrix& x, const int64_t* offsets, int64_t n_segments, const void* components,
                        const void* means, int64_t k, int64_t d, bool centering, const petal_matrix& y_out);
void inverse_transform_segments(petal_ctx& c, const petal_matrix& y, const int64_t* offsets, int64_t n_segments, const void* components,
                                const void* means, int64_t k, int64_t d, bool centering, const petal_matrix& x_out);
// include/petal_hip_sparse.h: RandomizedPca on a resident CSR matrix
petal_csr* csr_create(petal_ctx& c, int64_t rows, int64_t cols, int64_t nnz, const int64_t* indptr, const int32_t* indices, const void* values,
                      int32_t dtype);
void csr_destroy(petal_csr* x);
void csr_image(const petal_csr& x, int transposed, int64_t* indptr, int32_t* indices, void* values, int64_t* items);
void rpca_fit_csr(petal_ctx& c, const petal_csr& x, int64_t k, int64_t n_oversample, int64_t n_iter, bool centering, const void* omega,
                  void* components, void* means, void* singular, void* total_variance, const petal_matrix* y_out, int64_t* kernel_path);
void transform_csr(petal_ctx& c, const petal_csr& x, const void* components, const void* means, int64_t k, int64_t d, bool centering,
                   const petal_matrix& y_out, int64_t* kernel_path);
void csr_gemm(petal_ctx& c, const petal_csr& x, bool transposed, const double* P, int64_t N, const double* a, const double* s, double* out);
// include/petal_hip_wide.h: the row Gram matrix of exact Pca's dual route by itself (a test aid)
void row_gram(petal_ctx& c, const petal_matrix& x, const double* centre, double* out, int64_t* info2);
// include/petal_hip_kpca.h: KernelPca
struct KernelSpec { int kernel; int degree; double gamma, coef0; };
petal_kpca* kpca_fit(petal_ctx& c, const petal_matrix& x, int64_t k, const KernelSpec& spec, const petal_matrix* y_out);
void kpca_destroy(petal_kpca* h);
void kpca_transform(petal_ctx& c, petal_kpca& h, const petal_matrix& x, const petal_matrix& y_out);
void kpca_get(const petal_kpca& h, double* eigenvalues, double* scaled_vectors, int64_t* info8);
void kernel_apply(petal_ctx& c, const petal_matrix& xq, const petal_matrix& xt, const KernelSpec& spec, const double* a, int64_t cols,
                  const double* centre, double* out, int64_t* info1);
// include/petal_hip_nmf.h: Nmf
struct NmfSpec { int64_t max_iter; double tol, l1_w, l2_w, l1_h, l2_h; };
petal_nmf* nmf_fit(petal_ctx& c, const petal_matrix& x, int64_t k, const NmfSpec& spec, const petal_matrix* w0, const petal_matrix* h0,
                   int64_t seed, const petal_matrix* w_out);
void nmf_destroy(petal_nmf* h);
void nmf_transform(petal_ctx& c, petal_nmf& h, const petal_matrix& x, const petal_matrix& w_out);
void nmf_inverse_transform(petal_ctx& c, petal_nmf& h, const petal_matrix& w, const petal_matrix& x_out);
void nmf_get(const petal_nmf& h, double* components, int64_t* info6, double* err2);
// include/petal_hip_nmf_sparse.h: Nmf on a sparse matrix
petal_nmf* nmf_fit_csr(petal_ctx& c, const petal_csr& x, int64_t k, const NmfSpec& spec, const petal_matrix* w0, const petal_matrix* h0,
                       int64_t seed, const petal_matrix* w_out, int64_t* kernel_path);
void nmf_transform_csr(petal_ctx& c, petal_nmf& h, const petal_csr& x, const petal_matrix& w_out, int64_t* kernel_path);
void nmf_sweep_csr(petal_ctx& c, const petal_csr& x, bool transposed, int64_t k, const double* g_in, const double* f, const NmfSpec& spec,
                   int64_t inner, double* g_out, double* gram_out, double* dot_out, int64_t* info1);
// include/petal_hip_nmf_kl.h: the Kullback-Leibler loss on a sparse matrix
petal_nmf* nmf_fit_csr_loss(petal_ctx& c, const petal_csr& x, int64_t k, const NmfSpec& spec, int64_t loss, const petal_matrix* w0,
                            const petal_matrix* h0, int64_t seed, const petal_matrix* w_out, int64_t* kernel_path);
void nmf_kl_sweep_csr(petal_ctx& c, const petal_csr& x, bool transposed, int64_t k, const double* g_in, const double* f, const NmfSpec& spec,
                      int64_t inner, double* g_out, double* colsum_out, double* term_out, int64_t* info1);
void nmf_pass(petal_ctx& c, const petal_matrix& x, int64_t k, const double* w_in, const double* h, const NmfSpec& spec, int64_t inner, double* w_out,
              double* a_out, double* b_out, int64_t* info1);
// include/petal_hip_nmf_kl_dense.h: the Kullback-Leibler loss on a dense matrix
petal_nmf* nmf_fit_loss(petal_ctx& c, const petal_matrix& x, int64_t k, const NmfSpec& spec, int64_t loss, const petal_matrix* w0,
                        const petal_matrix* h0, int64_t seed, const petal_matrix* w_out);
void nmf_transform_loss(petal_ctx& c, petal_nmf& h, const petal_matrix& x, const petal_matrix& w_out);
void nmf_kl_pass(petal_ctx& c, const petal_matrix& x, int64_t k, const double* w_in, const double* h, const NmfSpec& spec, int64_t inner,
                 double* w_out, double* a_out, double* colsum_out, double* term_out, int64_t* info1);
// include/petal_hip_nmf_cd.h: the coordinate-descent solver on a dense matrix
petal_nmf* nmf_fit_solver(petal_ctx& c, const petal_matrix& x, int64_t k, const NmfSpec& spec, int64_t solver, const petal_matrix* w0,
                          const petal_matrix* h0, int64_t seed, const petal_matrix* w_out);
void nmf_cd_transform(petal_ctx& c, petal_nmf& h, const petal_matrix& x, const petal_matrix& w_out);
void nmf_cd_pass(petal_ctx& c, const petal_matrix& x, int64_t k, const double* w_in, const double* h, const NmfSpec& spec, int64_t inner,
                 bool from_zero, double* w_out, double* a_out, double* b_out, double* violation_out, int64_t* info1);
void nmf_cd_hupdate(petal_ctx& c, int64_t k, int64_t d, const double* a, const double* b, const double* h_in, const NmfSpec& spec, double* h_out,
                    double* violation_out, int64_t* info1);
// include/petal_hip_nmf_cd_sparse.h: the coordinate-descent solver on a sparse matrix
petal_nmf* nmf_fit_csr_solver(petal_ctx& c, const petal_csr& x, int64_t k, const NmfSpec& spec, int64_t solver, const petal_matrix* w0,
                              const petal_matrix* h0, int64_t seed, const petal_matrix* w_out, int64_t* kernel_path);
void nmf_transform_csr_solver(petal_ctx& c, petal_nmf& h, const petal_csr& x, const petal_matrix& w_out, int64_t* kernel_path);
void nmf_cd_sweep_csr(petal_ctx& c, const petal_csr& x, bool transposed, int64_t k, const double* g_in, const double* f, const NmfSpec& spec,
                      int64_t inner, bool from_zero, double* g_out, double* gram_out, double* dot_out, double* violation_out, int64_t* info1);
// include/petal_hip_ipca.h: IncrementalPca
petal_ipca* ipca_create(petal_ctx& c, int64_t d, int32_t dtype, bool centering);
void ipca_destroy(petal_ipca* h);
void ipca_reset(petal_ipca& h);
void ipca_partial_fit(petal_ctx& c, petal_ipca& h, const petal_matrix& x);
void ipca_merge(petal_ctx& c, petal_ipca& into, const petal_ipca& other);
void ipca_finalize(petal_ctx& c, const petal_ipca& h, int64_t k, void* components, void* means, void* singular, void* total_variance);
void ipca_get_state(petal_ctx& c, const petal_ipca& h, double* n, double* mean, double* m2);
void ipca_set_state(petal_ctx& c, petal_ipca& h, double n, const double* mean, const double* m2);
void fastica_fit(petal_ctx& c, const petal_matrix& x, int64_t n_components, double tol, int64_t max_iter, int mode,
                 const void* w_init, void* components, void* means, int64_t* n_iter, const petal_matrix* y_out);
void ica_par(petal_ctx& c, const petal_matrix& x1, double tol, int64_t max_iter, int mode, const void* w_init,
             void* w_out, int64_t* n_iter);
void symmetric_decorrelation(petal_ctx& c, const void* w, int64_t nc, int dtype, int mode, void* out);
void logcosh(petal_ctx& c, const petal_matrix& x, const petal_matrix& g_out, void* gprime_out);
void svd_flip(petal_ctx& c, const petal_matrix& u, const petal_matrix& vt);
void gemm_xp(petal_ctx& c, const petal_matrix& x, const void* mu, const void* p, int64_t N, const void* bias,
             const petal_matrix& z_out);
void gemm_atb(petal_ctx& c, const petal_matrix& a, const void* mu_a, const petal_matrix* b, const void* mu_b, double* c_out);
void power_pass(petal_ctx& c, const petal_matrix& x, const void* mu, const void* p, int64_t N, double* y_out, const petal_matrix* z_out,
                int* fused_out);
// the probe entries of include/petal_hip_probe.h (test aids: one fp64 small-matrix operation per call)
void probe_chol(petal_ctx& c, const double* G, int64_t L, int64_t ldg, double rel_tol, int64_t Lz, int64_t ndead_cols, int route,
                const double* B, int64_t b_rows, int64_t b_cols, int64_t ldb, double* out, int64_t ldo, int* ndead, int* rt);
void probe_eigh(petal_ctx& c, const double* A, int64_t L, int64_t lda, double tol_rel, bool clustered, int64_t Lz, int64_t ncheck,
                int verdict_mode, int verdict_in, double gap_tol_override, double* w, double* V, int64_t ldv, int* verdict_out);
void probe_jacobi_svd_rows(petal_ctx& c, const double* A, int64_t L, int64_t lda, double* U, int64_t ldu, double* s_inv, int* nonconv);
void probe_dgemm(petal_ctx& c, bool ta, bool tb, int64_t M, int64_t N, int64_t K, double alpha, const double* A, int64_t lda,
                 const double* B, int64_t ldb, double beta, double* C, int64_t ldc, const double* colscale);
// ... the top-k subspace eigen-solver (topk_eigh through gram_topk_eigh / gram_eigen) and its residual verdict (op_ritz_residual)
void probe_ritz_residual(petal_ctx& c, const double* CV, int64_t ldc, const double* Vr, int64_t ldv, int64_t rows, int64_t nc,
                         const double* theta, const int* flag, const int* flag2, double* out3, double* w_out, int64_t w_len);
void probe_topk_eigh(petal_ctx& c, const double* C, int64_t d, int64_t ldc, int64_t nc, int dtype, int mode, int* delivered, double* w,
                     double* V, int64_t ldv, int* checks, double* r3, int* verdict, double* diag);
// ... and the composite operations that steer the optimistic fit (op_power_pass_means; op_rebase_xp / op_rebase_power_pass)
void probe_power_pass_means(petal_ctx& c, const void* X, int dtype, int64_t n, int64_t K, int64_t d, int64_t ldx, const double* P, int64_t N,
                            int64_t ldp, int64_t L, int* done, double* Y, int64_t ldy, double* mu64, double* muT, double* mu0, double* tv);
void probe_rebase(petal_ctx& c, const void* X, int dtype, int64_t n, int64_t K, int64_t ldx, const void* mu, const double* G, int64_t L,
                  int64_t ldg, double rel_tol, const double* A, int64_t M, int64_t lda, int p_planes, bool steering, int route, int* done,
                  double* P_out, int64_t ldpo, double* Z, int64_t ldz, double* Y, int64_t ldy, int* ndead);

}  // namespace petal

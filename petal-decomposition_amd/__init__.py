"""petal-decomposition_amd -- host-side mirror of the reference crate's public interface
(``Pca``/``PcaBuilder``/``RandomizedPca``/``RandomizedPcaBuilder``/``FastIca``/``FastIcaBuilder``,
``src/lib.rs:17-18``) over the C ABI of ``include/petal_hip.h``.

The arithmetic lives in ``libpetal_hip.so`` (hand-written HIP for gfx950, ``csrc/``).  This module
is plumbing only: it describes caller arrays (numpy on the host, torch / ``__cuda_array_interface__``
on the device) as ``petal_matrix`` and forwards.  There is no CPU fallback: if the library is
missing or no MI355X is visible, constructing a context raises.

The directory name carries a hyphen (it is the name the build contract asks for); import it through
``petal_decomposition_amd`` at the repo root.
"""
from __future__ import annotations

import ctypes as C
import os
import weakref
from contextlib import contextmanager as _contextmanager
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIBRARY = os.path.join(_HERE, "libpetal_hip.so")

PETAL_OK, PETAL_INVALID_INPUT, PETAL_LINALG_ERROR, PETAL_DEVICE_ERROR = 0, 1, 2, 3
PETAL_F32, PETAL_F64 = 0, 1
PETAL_HOST, PETAL_DEVICE = 0, 1
PETAL_SUM, PETAL_MAX, PETAL_MIN = 0, 1, 2
GEMM_SPLIT_BF16X3, GEMM_FP32_MFMA, GEMM_SPLIT_BF16X3_EXACT = 0, 1, 2
# petal_ctx_set_option (petal_hip.h PETAL_OPT_*): name -> option number
OPTIONS = {"two_plane_operands": 0, "two_plane_omega": 1, "two_plane_iterate": 2, "steering_passes": 3, "fused_pass": 4,
           "fused_pass_min_rows": 5, "verdict_threshold": 6, "means_fold_rows": 7, "gram_split": 8, "gram_split_hook": 9,
           "d2h_kernel": 10, "row_pad": 11, "eigh_jacobi": 12, "poison": 13, "force_collective": 14, "steering_hook": 15,
           "ipca_fallback": 32,   # (32: PETAL_OPT_IPCA_FALLBACK, include/petal_hip_ipca.h -- a test aid)
           "pca_dual": 33, "pca_dual_fallback": 34,   # (PETAL_OPT_PCA_DUAL, PETAL_OPT_PCA_DUAL_FALLBACK: include/petal_hip_wide.h)
           "kpca_fallback": 36,   # (PETAL_OPT_KPCA_FALLBACK, include/petal_hip_kpca.h -- a test aid)
           "nmf_fallback": 38}   # (PETAL_OPT_NMF_FALLBACK, include/petal_hip_nmf.h -- a test aid; 37 stays unknown)
ICA_TEXTBOOK, ICA_REFERENCE_LITERAL = 0, 1
# the contrast function of the FastICA iteration: bits 4-7 of the same `mode` argument (include/petal_hip.h); EXP and CUBE are an
# extension beyond the crate, whose only contrast is logcosh
ICA_CONTRAST_LOGCOSH, ICA_CONTRAST_EXP, ICA_CONTRAST_CUBE = 0, 16, 32
ICA_SEMANTICS_MASK, ICA_CONTRAST_MASK = 15, 240
_ICA_FUN = {"logcosh": ICA_CONTRAST_LOGCOSH, "exp": ICA_CONTRAST_EXP, "cube": ICA_CONTRAST_CUBE}


def _ica_contrast(fun) -> int:
    try:
        return _ICA_FUN[fun]
    except (KeyError, TypeError):
        raise InvalidInput(f"unknown contrast function {fun!r}: one of {sorted(_ICA_FUN)}") from None


from .pcg import Pcg  # noqa: E402  (rand_pcg::Mcg128Xsl64 + Ziggurat StandardNormal)


class DecompositionError(Exception):
    """``DecompositionError`` (src/lib.rs:22-28)."""


class InvalidInput(DecompositionError):
    def __str__(self):  # "invalid matrix: {0}" (src/lib.rs:24)
        return "invalid matrix: " + super().__str__()


class LinalgError(DecompositionError):
    def __str__(self):  # sic, src/lib.rs:26
        return "linear algerba operation failed: " + super().__str__()


class DeviceError(DecompositionError):
    pass


class petal_matrix(C.Structure):
    _fields_ = [("data", C.c_void_p), ("rows", C.c_int64), ("cols", C.c_int64),
                ("row_stride", C.c_int64), ("col_stride", C.c_int64),
                ("dtype", C.c_int32), ("space", C.c_int32)]


class petal_stats(C.Structure):
    _fields_ = [("fit_ms", C.c_double),
                ("xp_ms", C.c_double), ("xp_launches", C.c_int64),
                ("atb_ms", C.c_double), ("atb_launches", C.c_int64),
                ("pass_flops", C.c_double), ("pass_bytes", C.c_double),
                ("ica_step_ms", C.c_double), ("ica_step_launches", C.c_int64),
                ("ica_step_flops", C.c_double), ("ica_step_bytes", C.c_double),
                ("n_iter", C.c_int64),
                ("allreduce_calls", C.c_int64), ("allreduce_bytes", C.c_double),
                ("allreduce_ms", C.c_double), ("allreduce_timed", C.c_int64),
                ("x_row_pitch_bytes", C.c_int64), ("x_zero_copy", C.c_int64),
                ("rpca_redo", C.c_int64), ("pow_ms", C.c_double), ("pow_launches", C.c_int64),
                ("stream_ms", C.c_double), ("stream_launches", C.c_int64), ("ica_redo", C.c_int64), ("ica_gram_split", C.c_int64),
                ("means_folded", C.c_int64), ("eigh_redo", C.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p)

# every symbol include/petal_hip.h declares: (name, restype, argtypes)
_P = C.c_void_p
_M = C.POINTER(petal_matrix)
ABI = [
    ("petal_ctx_create", C.c_int, [C.c_int, _P, C.POINTER(_P)]),
    ("petal_ctx_destroy", None, [_P]),
    ("petal_last_error", C.c_char_p, [_P]),
    ("petal_version", C.c_char_p, []),
    ("petal_ctx_set_collective", C.c_int, [_P, ALLREDUCE_FN, _P, C.c_int, C.c_int]),
    ("petal_ctx_set_profiling", C.c_int, [_P, C.c_int]),
    ("petal_ctx_set_gemm_mode", C.c_int, [_P, C.c_int]),
    ("petal_ctx_set_option", C.c_int, [_P, C.c_int, C.c_double]),
    ("petal_ctx_get_option", C.c_int, [_P, C.c_int, C.POINTER(C.c_double)]),
    ("petal_rccl_unique_id", C.c_int, [_P]),
    ("petal_ctx_init_rccl", C.c_int, [_P, _P, C.c_int, C.c_int]),
    ("petal_get_stats", C.c_int, [_P, C.POINTER(petal_stats)]),
    ("petal_ctx_collective_info", C.c_int, [_P] + [C.POINTER(C.c_int)] * 6),
    ("petal_power_pass", C.c_int, [_P, _M, _P, _P, C.c_int64, C.POINTER(C.c_double), _M, C.POINTER(C.c_int)]),
    ("petal_pca_fit", C.c_int, [_P, _M, C.c_int64, C.c_int, _P, _P, _P, _P, _M]),
    ("petal_rpca_fit", C.c_int, [_P, _M, C.c_int64, C.c_int64, C.c_int64, C.c_int, _P, _P, _P, _P, _P, _M]),
    ("petal_transform", C.c_int, [_P, _M, _P, _P, C.c_int64, C.c_int64, C.c_int, _M]),
    ("petal_inverse_transform", C.c_int, [_P, _M, _P, _P, C.c_int64, C.c_int64, C.c_int, _M]),
    ("petal_fastica_fit", C.c_int, [_P, _M, C.c_int64, C.c_double, C.c_int64, C.c_int, _P, _P, _P, C.POINTER(C.c_int64), _M]),
    ("petal_ica_par", C.c_int, [_P, _M, C.c_double, C.c_int64, C.c_int, _P, _P, C.POINTER(C.c_int64)]),
    ("petal_symmetric_decorrelation", C.c_int, [_P, _P, C.c_int64, C.c_int32, C.c_int, _P]),
    ("petal_logcosh", C.c_int, [_P, _M, _M, _P]),
    ("petal_svd_flip", C.c_int, [_P, _M, _M]),
    ("petal_gemm_xp", C.c_int, [_P, _M, _P, _P, C.c_int64, _P, _M]),
    ("petal_gemm_atb", C.c_int, [_P, _M, _P, _M, _P, C.POINTER(C.c_double)]),
]

# every symbol include/petal_hip_score.h declares (row scores: an extension beyond the crate, kept apart from the mirrored set above)
ABI_SCORE = [
    ("petal_score_rows", C.c_int, [_P, _M, _P, _P, C.c_int64, C.c_int64, C.c_int, _P, _M, _M]),
]

# every symbol include/petal_hip_segments.h declares (segmented Pca: an extension beyond the crate, kept apart from the mirrored set above)
_L = C.POINTER(C.c_int64)
ABI_SEGMENTS = [
    ("petal_pca_fit_segments", C.c_int, [_P, _M, _L, C.c_int64, C.c_int64, C.c_int, _P, _P, _P, _P, C.POINTER(C.c_int32), _M, _L]),
    ("petal_transform_segments", C.c_int, [_P, _M, _L, C.c_int64, _P, _P, C.c_int64, C.c_int64, C.c_int, _M]),
    ("petal_inverse_transform_segments", C.c_int, [_P, _M, _L, C.c_int64, _P, _P, C.c_int64, C.c_int64, C.c_int, _M]),
]

# every symbol include/petal_hip_probe.h declares (TEST AIDS: the fp64 small-matrix operations through entries of their own; not part
# of the mirrored interface, no Rust binding)
_D = C.POINTER(C.c_double)
_I = C.POINTER(C.c_int)
ABI_PROBE = [
    ("petal_probe_chol", C.c_int, [_P, _D, C.c_int64, C.c_int64, C.c_double, C.c_int64, C.c_int64, C.c_int, _D, C.c_int64, C.c_int64,
                                   C.c_int64, _D, C.c_int64, _I, _I]),
    ("petal_probe_eigh", C.c_int, [_P, _D, C.c_int64, C.c_int64, C.c_double, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_double,
                                   _D, _D, C.c_int64, _I]),
    ("petal_probe_jacobi_svd_rows", C.c_int, [_P, _D, C.c_int64, C.c_int64, _D, C.c_int64, _D, _I]),
    ("petal_probe_dgemm", C.c_int, [_P, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_double, _D, C.c_int64, _D, C.c_int64,
                                    C.c_double, _D, C.c_int64, _D]),
    ("petal_probe_ritz_residual", C.c_int, [_P, _D, C.c_int64, _D, C.c_int64, C.c_int64, C.c_int64, _D, _I, _I, _D, _D, C.c_int64]),
    ("petal_probe_topk_eigh", C.c_int, [_P, _D, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int, _I, _D, _D, C.c_int64, _I, _D, _I, _D]),
    ("petal_probe_power_pass_means", C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int64, _D, C.c_int64, C.c_int64,
                                               C.c_int64, _I, _D, C.c_int64, _D, _D, _D, _D]),
    ("petal_probe_rebase", C.c_int, [_P, _P, C.c_int32, C.c_int64, C.c_int64, C.c_int64, _P, _D, C.c_int64, C.c_int64, C.c_double, _D,
                                     C.c_int64, C.c_int64, C.c_int, C.c_int, C.c_int, _I, _D, C.c_int64, _D, C.c_int64, _D, C.c_int64, _I]),
]

# every symbol include/petal_hip_sparse.h declares (RandomizedPca on sparse CSR data: an extension beyond the crate, kept apart from the
# mirrored set above)
_I32 = C.POINTER(C.c_int32)
ABI_SPARSE = [
    ("petal_csr_create", C.c_int, [_P, C.c_int64, C.c_int64, C.c_int64, _L, _I32, _P, C.c_int32, C.POINTER(_P)]),
    ("petal_csr_destroy", None, [_P]),
    ("petal_csr_info", C.c_int, [_P, _L]),
    ("petal_csr_image", C.c_int, [_P, C.c_int, _L, _I32, _P, _L]),
    ("petal_rpca_fit_csr", C.c_int, [_P, _P, C.c_int64, C.c_int64, C.c_int64, C.c_int, _P, _P, _P, _P, _P, _M, _L]),
    ("petal_transform_csr", C.c_int, [_P, _P, _P, _P, C.c_int64, C.c_int64, C.c_int, _M, _L]),
    ("petal_csr_gemm", C.c_int, [_P, _P, C.c_int, _D, C.c_int64, _D, _D, _D]),
    ("petal_ctx_workspace_in_use", C.c_int, [_P, _L, _L]),
]
CSR_ITEM_NNZ = 256   # PETAL_CSR_ITEM_NNZ

# every symbol include/petal_hip_ipca.h declares (IncrementalPca: an extension beyond the crate)
ABI_IPCA = [
    ("petal_ipca_create", C.c_int, [_P, C.c_int64, C.c_int32, C.c_int, C.POINTER(_P)]),
    ("petal_ipca_destroy", None, [_P]),
    ("petal_ipca_reset", C.c_int, [_P]),
    ("petal_ipca_partial_fit", C.c_int, [_P, _P, _M]),
    ("petal_ipca_merge", C.c_int, [_P, _P, _P]),
    ("petal_ipca_finalize", C.c_int, [_P, _P, C.c_int64, _P, _P, _P, _P]),
    ("petal_ipca_info", C.c_int, [_P, _L]),
    ("petal_ipca_get_state", C.c_int, [_P, _P, _D, _D, _D]),
    ("petal_ipca_set_state", C.c_int, [_P, _P, C.c_double, _D, _D]),
]
IPCA_KERNEL_MAX_D = 1024   # PETAL_IPCA_KERNEL_MAX_D

# every symbol include/petal_hip_wide.h declares (exact Pca on wide data: the dual route's facts and its row Gram matrix by itself)
ABI_WIDE = [
    ("petal_pca_last_route", C.c_int, [_P, _L]),
    ("petal_row_gram", C.c_int, [_P, _M, _D, _D, _L]),
]


# every symbol include/petal_hip_kpca.h declares (KernelPca and its fused pass by itself)
class petal_kernel_spec(C.Structure):
    _fields_ = [("kernel", C.c_int32), ("degree", C.c_int32), ("gamma", C.c_double), ("coef0", C.c_double)]


_KS = C.POINTER(petal_kernel_spec)
KERNELS = {"linear": 0, "poly": 1, "rbf": 2, "sigmoid": 3, "cosine": 4}   # PETAL_KERNEL_*
ABI_KPCA = [
    ("petal_kpca_fit", C.c_int, [_P, _M, C.c_int64, _KS, C.POINTER(C.c_void_p), _M]),
    ("petal_kpca_destroy", None, [_P]),
    ("petal_kpca_transform", C.c_int, [_P, _P, _M, _M]),
    ("petal_kpca_get", C.c_int, [_P, _D, _D, _L]),
    ("petal_kernel_apply", C.c_int, [_P, _M, _M, _KS, _D, C.c_int64, _D, _D, _L]),
]

# every symbol include/petal_hip_nmf.h declares (Nmf and its fused pass by itself)
class petal_nmf_spec(C.Structure):
    _fields_ = [("max_iter", C.c_int64), ("tol", C.c_double), ("l1_w", C.c_double), ("l2_w", C.c_double), ("l1_h", C.c_double),
                ("l2_h", C.c_double)]


_NS = C.POINTER(petal_nmf_spec)
ABI_NMF = [
    ("petal_nmf_fit", C.c_int, [_P, _M, C.c_int64, _NS, _M, _M, C.c_int64, C.POINTER(C.c_void_p), _M]),
    ("petal_nmf_destroy", None, [_P]),
    ("petal_nmf_transform", C.c_int, [_P, _P, _M, _M]),
    ("petal_nmf_inverse_transform", C.c_int, [_P, _P, _M, _M]),
    ("petal_nmf_get", C.c_int, [_P, _D, _L, _D]),
    ("petal_nmf_pass", C.c_int, [_P, _M, C.c_int64, _D, _D, _NS, C.c_int64, _D, _D, _D, _L]),
]

# every symbol include/petal_hip_nmf_sparse.h declares (Nmf on sparse CSR data and its sweep by itself)
ABI_NMF_SPARSE = [
    ("petal_nmf_fit_csr", C.c_int, [_P, _P, C.c_int64, _NS, _M, _M, C.c_int64, C.POINTER(C.c_void_p), _M, _L]),
    ("petal_nmf_transform_csr", C.c_int, [_P, _P, _P, _M, _L]),
    ("petal_nmf_sweep_csr", C.c_int, [_P, _P, C.c_int, C.c_int64, _D, _D, _NS, C.c_int64, _D, _D, _D, _L]),
]

# every symbol include/petal_hip_nmf_kl.h declares (Nmf with the Kullback-Leibler loss on sparse CSR data and its sweep by itself)
NMF_LOSS_FROBENIUS, NMF_LOSS_KL = 0, 1
ABI_NMF_KL = [
    ("petal_nmf_fit_csr_loss", C.c_int, [_P, _P, C.c_int64, _NS, C.c_int64, _M, _M, C.c_int64, C.POINTER(C.c_void_p), _M, _L]),
    ("petal_nmf_get_loss", C.c_int, [_P, _L]),
    ("petal_nmf_kl_sweep_csr", C.c_int, [_P, _P, C.c_int, C.c_int64, _D, _D, _NS, C.c_int64, _D, _D, _D, _L]),
]
# every symbol include/petal_hip_nmf_kl_dense.h declares (Nmf with the Kullback-Leibler loss on dense data and its fused pass by itself)
ABI_NMF_KL_DENSE = [
    ("petal_nmf_fit_loss", C.c_int, [_P, _M, C.c_int64, _NS, C.c_int64, _M, _M, C.c_int64, C.POINTER(C.c_void_p), _M]),
    ("petal_nmf_transform_loss", C.c_int, [_P, _P, _M, _M]),
    ("petal_nmf_kl_pass", C.c_int, [_P, _M, C.c_int64, _D, _D, _NS, C.c_int64, _D, _D, _D, _D, _L]),
]
# every symbol include/petal_hip_nmf_cd.h declares (Nmf with the coordinate-descent solver, its fused pass and its H side by themselves)
NMF_SOLVER_MU, NMF_SOLVER_CD = 0, 1
ABI_NMF_CD = [
    ("petal_nmf_fit_solver", C.c_int, [_P, _M, C.c_int64, _NS, C.c_int64, _M, _M, C.c_int64, C.POINTER(C.c_void_p), _M]),
    ("petal_nmf_get_solver", C.c_int, [_P, _L]),
    ("petal_nmf_cd_pass", C.c_int, [_P, _M, C.c_int64, _D, _D, _NS, C.c_int64, C.c_int, _D, _D, _D, _D, _L]),
    ("petal_nmf_cd_hupdate", C.c_int, [_P, C.c_int64, C.c_int64, _D, _D, _D, _NS, _D, _D, _L]),
]
# every symbol include/petal_hip_nmf_cd_sparse.h declares (the coordinate-descent solver on sparse CSR data and its sweep by itself)
ABI_NMF_CD_SPARSE = [
    ("petal_nmf_fit_csr_solver", C.c_int, [_P, _P, C.c_int64, _NS, C.c_int64, _M, _M, C.c_int64, C.POINTER(C.c_void_p), _M, _L]),
    ("petal_nmf_transform_csr_solver", C.c_int, [_P, _P, _P, _M, _L]),
    ("petal_nmf_cd_sweep_csr", C.c_int, [_P, _P, C.c_int, C.c_int64, _D, _D, _NS, C.c_int64, C.c_int, _D, _D, _D, _D, _L]),
]

# header file name (include/) -> its table, in the order the headers were added: what load_library types and the tests check
ABI_TABLES = {"petal_hip.h": ABI, "petal_hip_score.h": ABI_SCORE, "petal_hip_segments.h": ABI_SEGMENTS, "petal_hip_probe.h": ABI_PROBE,
              "petal_hip_sparse.h": ABI_SPARSE, "petal_hip_ipca.h": ABI_IPCA, "petal_hip_wide.h": ABI_WIDE, "petal_hip_kpca.h": ABI_KPCA,
              "petal_hip_nmf.h": ABI_NMF, "petal_hip_nmf_sparse.h": ABI_NMF_SPARSE, "petal_hip_nmf_kl.h": ABI_NMF_KL,
              "petal_hip_nmf_kl_dense.h": ABI_NMF_KL_DENSE, "petal_hip_nmf_cd.h": ABI_NMF_CD, "petal_hip_nmf_cd_sparse.h": ABI_NMF_CD_SPARSE}


def _preload_torch_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64 and load them by the unversioned
    file name, so a process that first loads the system HIP runtime (through this library) and then imports
    torch ends up with TWO HSA runtimes and torch sees no GPU.  Importing torch first makes the dynamic
    loader resolve this library's ``libamdhip64.so.7`` to the copy torch already loaded: one runtime, shared
    streams and device pointers.  Skipped when torch is absent or PETAL_NO_TORCH=1."""
    import sys
    if "torch" in sys.modules or os.environ.get("PETAL_NO_TORCH") == "1":
        return
    try:
        import torch  # noqa: F401
    except Exception:
        pass


def load_library(path: Optional[str] = None, preload_torch: bool = True) -> C.CDLL:
    """dlopen a library implementing every header in ``ABI_TABLES`` (include/) and type its entry points."""
    path = path or os.environ.get("PETAL_HIP_LIBRARY") or DEFAULT_LIBRARY
    if not os.path.exists(path):
        raise RuntimeError(
            f"petal-decomposition_amd: native library not found at {path}. Build it with "
            f"`python __graft_entry__.py build` (hipcc --offload-arch=gfx950). There is no CPU fallback.")
    if preload_torch:
        _preload_torch_hip_runtime()
    lib = C.CDLL(path)
    for name, res, args in (entry for table in ABI_TABLES.values() for entry in table):
        fn = getattr(lib, name)  # AttributeError if the library does not export the symbol
        fn.restype = res
        fn.argtypes = args
    lib._petal_path = path
    return lib


_default_lib = None


def default_library() -> C.CDLL:
    global _default_lib
    if _default_lib is None:
        _default_lib = load_library()
    return _default_lib


# ------------------------------------------------------------------------------------------------
def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _np_dtype(code):
    return np.float32 if code == PETAL_F32 else np.float64


def describe(x, keep: list) -> petal_matrix:
    """ndarray-style (ptr, shape, strides) descriptor of a 2-D numpy array / torch tensor."""
    if _is_torch(x):
        import torch
        if x.dim() != 2:
            raise InvalidInput("expected a 2-D array")
        if x.dtype == torch.float32:
            dt = PETAL_F32
        elif x.dtype == torch.float64:
            dt = PETAL_F64
        else:
            raise InvalidInput(f"unsupported dtype {x.dtype}")
        keep.append(x)
        space = PETAL_DEVICE if x.is_cuda else PETAL_HOST
        if x.is_cuda:
            # the ctx launches on its own stream: whatever torch still has queued for this tensor on ITS current stream
            # must be finished first (the calls are synchronous anyway; a no-op when the ctx shares torch's stream)
            torch.cuda.current_stream(x.device).synchronize()
        return petal_matrix(x.data_ptr(), x.shape[0], x.shape[1], x.stride(0), x.stride(1), dt, space)
    if hasattr(x, "__cuda_array_interface__") and not isinstance(x, np.ndarray):
        cai = x.__cuda_array_interface__
        shape, typestr = cai["shape"], cai["typestr"]
        if len(shape) != 2:
            raise InvalidInput("expected a 2-D array")
        dt = {"<f4": PETAL_F32, "<f8": PETAL_F64}[typestr]
        isz = 4 if dt == PETAL_F32 else 8
        strides = cai.get("strides") or (shape[1] * isz, isz)
        keep.append(x)
        return petal_matrix(cai["data"][0], shape[0], shape[1], strides[0] // isz, strides[1] // isz, dt, PETAL_DEVICE)
    a = np.asarray(x)
    if a.ndim != 2:
        raise InvalidInput("expected a 2-D array")
    if a.dtype not in (np.float32, np.float64):
        a = a.astype(np.float64)
    keep.append(a)
    dt = PETAL_F32 if a.dtype == np.float32 else PETAL_F64
    isz = a.dtype.itemsize
    return petal_matrix(a.ctypes.data, a.shape[0], a.shape[1], a.strides[0] // isz, a.strides[1] // isz, dt, PETAL_HOST)


def _alloc_like(x, rows, cols, dtype_code):
    """Output array in the memory space of x (torch device tensor or numpy)."""
    if _is_torch(x) and x.is_cuda:
        import torch
        return torch.empty((rows, cols), dtype=x.dtype, device=x.device)
    return np.empty((rows, cols), dtype=_np_dtype(dtype_code))


def _out_like(x, rows, cols, dtype_code, keep):
    """(output array in the memory space of x, its petal_matrix)"""
    y = _alloc_like(x, rows, cols, dtype_code)
    return y, describe(y, keep)


def _host(a, dtype_code, shape=None):
    out = np.ascontiguousarray(np.asarray(a, dtype=_np_dtype(dtype_code)))
    if shape is not None and out.shape != tuple(shape):
        raise InvalidInput(f"expected shape {tuple(shape)}, got {out.shape}")
    return out


def _f64c(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64))


def _dp(a):
    """a float64 array as `double*`; None stays NULL"""
    return a.ctypes.data_as(_D) if a is not None else None


def _ref(m):
    """byref of a ctypes value; None stays NULL"""
    return C.byref(m) if m is not None else None


def _with_info(out, info, want_info, keys=("kernel",)):
    return (out, {k: int(v) for k, v in zip(keys, info)}) if want_info else out


class Context:
    """One GPU, one stream, one caching workspace (``petal_ctx``)."""

    def __init__(self, device: int = 0, stream: Optional[int] = None, lib: Optional[C.CDLL] = None):
        self.lib = lib or default_library()
        self._h = C.c_void_p()
        self._cb = None
        rc = self.lib.petal_ctx_create(int(device), C.c_void_p(stream) if stream else None, C.byref(self._h))
        if rc != PETAL_OK or not self._h:
            raise DeviceError(f"petal_ctx_create(device={device}) failed with code {rc}: no usable gfx950 device? "
                              f"(library {getattr(self.lib, '_petal_path', '?')})")
        self.rank, self.world_size = 0, 1
        self._owned = weakref.WeakSet()   # what lives with this ctx and is released before it: sparse matrices, IncrementalPca
        #                                   statistics, fitted KernelPca and Nmf models (_HandleOwner._adopt)
        self._nmf = self._owned           # (the name tests/nmf_kl_dense_cases.py registers a hand-made Nmf under: the same set)

    def close(self):
        if getattr(self, "_h", None):
            for m in list(getattr(self, "_owned", ())):
                m.close()
            self.lib.petal_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc: int):
        if rc == PETAL_OK:
            return
        msg = (self.lib.petal_last_error(self._h) or b"").decode()
        raise {PETAL_INVALID_INPUT: InvalidInput, PETAL_LINALG_ERROR: LinalgError}.get(rc, DeviceError)(msg)

    def workspace_in_use(self):
        """(blocks, bytes) of device memory the ctx's allocator has handed out and not got back (test aid, include/petal_hip_sparse.h);
        (-1, -1) where the device-op layer keeps no count."""
        blocks, nbytes = C.c_int64(0), C.c_int64(0)
        self.check(self.lib.petal_ctx_workspace_in_use(self._h, C.byref(blocks), C.byref(nbytes)))
        return int(blocks.value), int(nbytes.value)

    def set_profiling(self, level):
        """0/False off, 1/True one sampled launch of each hot kernel per fit, 2 every launch (petal_hip.h)."""
        self.check(self.lib.petal_ctx_set_profiling(self._h, int(level)))

    def set_gemm_mode(self, mode):
        """GEMM_SPLIT_BF16X3 (default), GEMM_FP32_MFMA or GEMM_SPLIT_BF16X3_EXACT; also accepts "bf16x3" / "fp32" / "bf16x3-exact"
        (petal_hip.h)."""
        if isinstance(mode, str):
            mode = {"bf16x3": GEMM_SPLIT_BF16X3, "fp32": GEMM_FP32_MFMA, "bf16x3-exact": GEMM_SPLIT_BF16X3_EXACT}[mode]
        self.check(self.lib.petal_ctx_set_gemm_mode(self._h, int(mode)))

    def set_option(self, option, value) -> None:
        """petal_ctx_set_option: `option` a PETAL_OPT_* number or its name in OPTIONS ("steering_passes", "means_fold_rows", ...).
        The defaults were read from the environment once, when the ctx was created; nothing in the library reads it afterwards."""
        opt = OPTIONS[option] if isinstance(option, str) else int(option)
        self.check(self.lib.petal_ctx_set_option(self._h, opt, float(value)))

    def get_option(self, option) -> float:
        opt = OPTIONS[option] if isinstance(option, str) else int(option)
        v = C.c_double(0.0)
        self.check(self.lib.petal_ctx_get_option(self._h, opt, C.byref(v)))
        return v.value

    def collective_info(self) -> dict:
        """kind ("none" / "hook" / "rccl"), rank / world_size as the ctx was told them, and -- for the built-in communicator -- what
        RCCL itself reports: ncclCommCount, ncclCommCuDevice, ncclCommUserRank (-1 where unavailable)."""
        v = [C.c_int(-1) for _ in range(6)]
        self.check(self.lib.petal_ctx_collective_info(self._h, *[C.byref(x) for x in v]))
        return {"kind": {0: "none", 1: "hook", 2: "rccl"}.get(v[0].value, "?"), "rank": v[1].value, "world_size": v[2].value,
                "ncclCommCount": v[3].value, "ncclCommCuDevice": v[4].value, "ncclCommUserRank": v[5].value}

    def stats(self) -> dict:
        s = petal_stats()
        self.lib.petal_get_stats(self._h, C.byref(s))
        return s.as_dict()

    def set_collective(self, fn, rank: int, world_size: int):
        """fn(ptr:int, count:int, dtype:int, op:int, stream:int) -> int (0 = ok)."""
        def tramp(_user, buf, count, dtype, op, stream):
            try:
                return int(fn(int(buf or 0), int(count), int(dtype), int(op), int(stream or 0)) or 0)
            except Exception as e:  # never unwind through C
                import sys
                print(f"petal all-reduce hook failed: {e!r}", file=sys.stderr)
                return 1
        self._cb = ALLREDUCE_FN(tramp)
        self.check(self.lib.petal_ctx_set_collective(self._h, self._cb, None, int(rank), int(world_size)))
        self.rank, self.world_size = rank, world_size

    @staticmethod
    def torch_allreduce_hook(group=None, host_buffers=False):
        """The all-reduce hook as a Python callable ``hook(ptr, count, dtype, op, stream) -> 0``: wraps the raw
        buffer zero-copy as a torch tensor and calls ``torch.distributed.all_reduce`` on ``group``.  Backend "nccl" ==
        RCCL over xGMI on ROCm, enqueued on the ctx stream.  Backend "gloo" with DEVICE buffers (several ranks sharing one
        GPU, where RCCL refuses to form a communicator; or a node without xGMI): the buffer is staged through the host in
        stream order -- D2H on the ctx stream, gloo all-reduce, H2D on the ctx stream.  ``host_buffers=True`` is the
        host-memory simulation of the CPU tests, whose "device" pointers are plain host pointers."""
        import torch
        import torch.distributed as dist
        ops = {PETAL_SUM: dist.ReduceOp.SUM, PETAL_MAX: dist.ReduceOp.MAX, PETAL_MIN: dist.ReduceOp.MIN}
        backend = dist.get_backend(group)

        class _Cai:  # zero-copy view of a device buffer for torch.as_tensor
            def __init__(self, ptr, count, typestr):
                self.__cuda_array_interface__ = {"shape": (count,), "typestr": typestr, "data": (ptr, False), "version": 3}

        def hook(ptr, count, dtype, op, stream):
            npdt = _np_dtype(dtype)
            if host_buffers:
                ctype = C.c_float if dtype == PETAL_F32 else C.c_double
                view = np.ctypeslib.as_array((ctype * count).from_address(ptr))
                t = torch.from_numpy(view)
                dist.all_reduce(t, op=ops[op], group=group)
                return 0
            t = torch.as_tensor(_Cai(ptr, count, np.dtype(npdt).str), device="cuda")
            if backend == "gloo":
                ext = torch.cuda.ExternalStream(stream) if stream else torch.cuda.default_stream()
                with torch.cuda.stream(ext):
                    h = t.cpu()                      # ordered behind the kernels queued on the ctx stream; blocks the host
                    dist.all_reduce(h, op=ops[op], group=group)
                    t.copy_(h)                       # pageable source: returns once staged, ordered on the ctx stream
                return 0
            if stream:
                with torch.cuda.stream(torch.cuda.ExternalStream(stream)):
                    dist.all_reduce(t, op=ops[op], group=group)
            else:
                dist.all_reduce(t, op=ops[op], group=group)
            return 0

        return hook

    def use_rccl(self, group=None):
        """Sample-sharded multi-GPU with the library's BUILT-IN collective: ncclAllReduce issued by the library on the ctx
        stream (petal_ctx_init_rccl).  torch.distributed is only used once, to hand rank 0's ncclUniqueId to the others.
        Collective: every rank of ``group`` must call it."""
        import torch.distributed as dist
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        uid = C.create_string_buffer(128)
        if rank == 0:
            rc = self.lib.petal_rccl_unique_id(uid)
            if rc != 0:
                raise DeviceError("petal_rccl_unique_id failed: RCCL could not be loaded")
        box = [uid.raw if rank == 0 else None]
        dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        buf = C.create_string_buffer(box[0], 128)
        self.check(self.lib.petal_ctx_init_rccl(self._h, buf, rank, world))
        self.rank, self.world_size = rank, world

    def use_torch_distributed(self, group=None):
        """Sample-sharded multi-GPU: sum the small replicated buffers with torch.distributed."""
        import torch.distributed as dist
        host_buffers = bool(getattr(self.lib, "_petal_host_buffers", False))
        self.set_collective(self.torch_allreduce_hook(group, host_buffers), dist.get_rank(group), dist.get_world_size(group))


_default_ctx = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


class _CtxUser:
    """what works on the ctx its constructor was given (``self.ctx``) or, failing that, on the default one from the first use on"""

    def _ctx(self) -> Context:
        if self.ctx is None:
            self.ctx = default_context()
        return self.ctx

    @_contextmanager
    def _sparse(self, x):
        """x as a CsrMatrix on this model's ctx; one made here is released when the block is over."""
        if isinstance(x, CsrMatrix):
            if self.ctx is None:
                self.ctx = x.ctx
            yield x
            return
        sx = CsrMatrix.from_scipy_like(x, ctx=self._ctx())
        try:
            yield sx
        finally:
            sx.close()


class _HandleOwner(_CtxUser):
    """what owns a handle of the library that lives with its ctx; a subclass names the entry that destroys the handle and the message
    of a missing one"""
    _destroy = None     # "petal_..._destroy"
    _no_handle = None   # the InvalidInput message when there is no handle

    def _adopt(self, ctx, handle):
        self.close()
        self._h = handle
        ctx._owned.add(self)

    def close(self):
        if getattr(self, "_h", None) and getattr(self.ctx, "_h", None):
            getattr(self.ctx.lib, self._destroy)(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if not self._h:
            raise InvalidInput(self._no_handle)
        return self._h


class _FitsWithY:
    """fit / fit_transform of a model whose ``_inner_fit(x, want_y)`` takes nothing else"""

    def fit(self, x):
        self._inner_fit(x, False)
        return self

    def fit_transform(self, x):
        return self._inner_fit(x, True)



# ---- serde interchange (the crate's `serde` feature, Cargo.toml:41-47): models as the JSON serde_json writes for the
# reference structs -- same field names and order (src/pca.rs:41-51, 317-329; src/ica.rs:41-50), ndarray's
# {"v": 1, "dim": [...], "data": [...]} arrays, rand_pcg's {"state": u128} generator.
def _nd_to_serde(a) -> dict:
    a = np.asarray(a)
    return {"v": 1, "dim": list(a.shape), "data": [float(v) for v in a.reshape(-1)]}


def _nd_from_serde(obj: dict, dtype) -> np.ndarray:
    if obj.get("v") != 1:
        raise InvalidInput("unknown ndarray serde version")
    return np.asarray(obj["data"], dtype=dtype).reshape([int(v) for v in obj["dim"]])


def _rng_to_serde(rng):
    if isinstance(rng, Pcg):
        return rng.to_serde()
    raise InvalidInput("only the crate's Pcg generator has a serde form: build the model with seed()/with_seed() or a Pcg")


# ------------------------------------------------------------------------------------------------
def _is_sparse(x) -> bool:
    """A CsrMatrix, or any object with .data / .indices / .indptr / .shape (scipy.sparse.csr_matrix among them; scipy is never imported)."""
    if isinstance(x, CsrMatrix):
        return True
    if isinstance(x, np.ndarray) or _is_torch(x):
        return False
    return all(hasattr(x, a) for a in ("data", "indices", "indptr", "shape"))


class CsrMatrix(_HandleOwner):
    """A sparse matrix in CSR form, resident with its ctx (``petal_csr``, include/petal_hip_sparse.h): the arrays are checked, the
    transposed image and the work items of both images are built on the host, and both images are uploaded once.  ``RandomizedPca.fit``,
    ``fit_transform`` and ``transform`` take it in place of a dense matrix.  An extension beyond the crate.

    ``indices`` inside a row need not be sorted, duplicates act as their sum, explicit zeros, empty rows and empty columns are legal."""

    _destroy, _no_handle = "petal_csr_destroy", "the sparse matrix was closed (or its ctx was)"

    def __init__(self, data, indices, indptr, shape, ctx: Optional["Context"] = None):
        data = np.asarray(data)
        if data.dtype not in (np.float32, np.float64):
            data = data.astype(np.float64)
        data = np.ascontiguousarray(data).ravel()
        if len(tuple(shape)) != 2:
            raise InvalidInput("expected a 2-D shape")
        rows, cols = int(shape[0]), int(shape[1])
        if cols >= 2 ** 31 or rows >= 2 ** 31:
            raise InvalidInput("sparse input: too many rows/columns (32-bit indices)")
        idx = np.asarray(indices).ravel()
        if idx.size and (int(idx.max()) >= 2 ** 31 or int(idx.min()) < -2 ** 31):
            raise InvalidInput("sparse input: a column index does not fit 32 bits")
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        ptr = np.ascontiguousarray(np.asarray(indptr).ravel(), dtype=np.int64)
        if ptr.size != rows + 1:
            raise InvalidInput(f"indptr should have {rows + 1} entries (it has {ptr.size})")
        if idx.size != data.size:
            raise InvalidInput(f"indices and data differ in length ({idx.size} and {data.size})")
        self.ctx = ctx if ctx is not None else default_context()
        self.shape, self.nnz, self.dtype = (rows, cols), int(data.size), data.dtype
        self._dt = PETAL_F32 if data.dtype == np.float32 else PETAL_F64
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.petal_csr_create(self.ctx._h, rows, cols, self.nnz, ptr.ctypes.data_as(_L), idx.ctypes.data_as(_I32),
                                                     data.ctypes.data, self._dt, C.byref(h)))
        self._adopt(self.ctx, h)

    @classmethod
    def from_scipy_like(cls, obj, ctx: Optional["Context"] = None):
        """From any object with ``.data``, ``.indices``, ``.indptr`` and ``.shape`` laid out as CSR."""
        if isinstance(obj, cls):
            return obj
        return cls(obj.data, obj.indices, obj.indptr, obj.shape, ctx=ctx)

    def info(self) -> dict:
        out = (C.c_int64 * 8)()
        if self.ctx.lib.petal_csr_info(self._handle(), out) != PETAL_OK:
            raise InvalidInput("petal_csr_info failed")
        keys = ("rows", "cols", "nnz", "dtype", "resident", "items", "items_transposed", "item_nnz")
        return dict(zip(keys, (int(v) for v in out)))

    @property
    def resident(self) -> bool:
        return bool(self.info()["resident"])

    def image(self, transposed: bool = False):
        """Debug accessor of a handle that is not resident: (indptr, indices, values, items) of the matrix or of its transposed image as
        the library built them; items is an (n, 3) array of (image row, first position, one past the last)."""
        inf = self.info()
        rows = inf["cols"] if transposed else inf["rows"]
        ptr, idx = np.zeros(rows + 1, dtype=np.int64), np.zeros(self.nnz, dtype=np.int32)
        val = np.zeros(self.nnz, dtype=self.dtype)
        items = np.zeros((inf["items_transposed" if transposed else "items"], 3), dtype=np.int64)
        self.ctx.check(self.ctx.lib.petal_csr_image(self._handle(), int(bool(transposed)), ptr.ctypes.data_as(_L), idx.ctypes.data_as(_I32),
                                                    val.ctypes.data, items.ctypes.data_as(_L)))
        return ptr, idx, val, items


def csr_gemm(x: "CsrMatrix", p, transposed: bool = False, a=None, s=None):
    """Test aid (``petal_csr_gemm``): ``x @ p`` or ``x.T @ p`` through the sparse product, minus ``outer(a, s)`` when ``s`` is given
    (``a`` defaults to ones) -- the implicit centring.  float64 in and out; a float32 matrix rounds ``p`` and the result to float32."""
    p = _f64c(p)
    rows, inner = (x.shape[1], x.shape[0]) if transposed else x.shape
    if p.ndim != 2 or p.shape[0] != inner:
        raise InvalidInput(f"expected {inner} rows in p")
    N = p.shape[1]
    out = np.zeros((rows, N))
    a = None if a is None else _host(a, PETAL_F64, (rows,))
    s = None if s is None else _host(s, PETAL_F64, (N,))
    ctx = x.ctx
    ctx.check(ctx.lib.petal_csr_gemm(ctx._h, x._handle(), int(bool(transposed)), _dp(p), N, _dp(a), _dp(s), _dp(out)))
    return out


def row_gram(x, centre=None, ctx: Optional["Context"] = None, want_info: bool = False):
    """Test aid (``petal_row_gram``, include/petal_hip_wide.h): the float64 row Gram matrix ``(x - centre) @ (x - centre).T`` of exact
    Pca's dual route, ``x`` widened to float64 before ``centre`` (d float64 values, or None) is subtracted.  ``x``: numpy or a
    ``torch.cuda`` tensor, any strides.  ``want_info``: also returns ``{"kernel": k_row_gram ran, "chunks": feature chunks}``."""
    keep = []
    mx = describe(x, keep)
    ctx = ctx or default_context()
    cen = None if centre is None else _host(centre, PETAL_F64, (mx.cols,))
    out = np.zeros((mx.rows, mx.rows))
    info = (C.c_int64 * 2)()
    ctx.check(ctx.lib.petal_row_gram(ctx._h, C.byref(mx), _dp(cen), _dp(out), info))
    return _with_info(out, info, want_info, ("kernel", "chunks"))


def _kernel_spec(kernel, gamma, degree, coef0) -> petal_kernel_spec:
    if kernel not in KERNELS:
        raise InvalidInput(f"unknown kernel {kernel!r} (one of {', '.join(KERNELS)})")
    return petal_kernel_spec(KERNELS[kernel], int(degree), 0.0 if gamma is None else float(gamma), float(coef0))


def kernel_apply(xq, xt, a, kernel="linear", gamma=None, degree=3, coef0=1.0, centre=None, ctx: Optional["Context"] = None,
                 want_info: bool = False):
    """Test aid (``petal_kernel_apply``, include/petal_hip_kpca.h): ``phi((xq - centre) @ (xt - centre).T) @ a`` in float64, the fused
    pass of ``KernelPca.transform`` by itself -- no double centring, no epilogue.  ``xq`` (m x d), ``xt`` (n x d): numpy or
    ``torch.cuda``, the same dtype, any strides; ``a``: n x cols float64; ``centre``: d float64 values or None.  ``want_info``: also
    returns ``{"kernel": k_kapply ran}``."""
    keep = []
    mq, mt = describe(xq, keep), describe(xt, keep)
    ctx = ctx or default_context()
    spec = _kernel_spec(kernel, gamma, degree, coef0)
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] != mt.rows:
        raise InvalidInput(f"a should have {mt.rows} rows")
    a = np.ascontiguousarray(a)
    cen = None if centre is None else _host(centre, PETAL_F64, (mt.cols,))
    out = np.zeros((mq.rows, a.shape[1]))
    info = (C.c_int64 * 1)()
    ctx.check(ctx.lib.petal_kernel_apply(ctx._h, C.byref(mq), C.byref(mt), C.byref(spec), _dp(a), a.shape[1], _dp(cen), _dp(out), info))
    return _with_info(out, info, want_info)


class KernelPca(_HandleOwner, _FitsWithY):
    """Kernel PCA (``petal_kpca``, include/petal_hip_kpca.h; an extension beyond the crate, DESIGN.md sections 4 and 7) -- scikit-learn's
    ``KernelPCA`` with the kernels ``linear``, ``poly``, ``rbf``, ``sigmoid`` and ``cosine``.  ``gamma=None`` (or <= 0) means 1 / d.
    ``fit_transform`` = V sqrt(lambda); ``transform`` is one fused pass over the query rows whose m x n kernel matrix never touches
    memory.  Everything is float64 inside; outputs are rounded once to the data's type.  A component at or below the relative threshold
    (1e-6 float32, 1e-10 float64, on sqrt(lambda)) is a zero column of both outputs.  The fitted model lives with its ctx and keeps its
    own device copy of the training rows."""

    _destroy, _no_handle = "petal_kpca_destroy", "the model has not been fitted (or its ctx was closed)"

    def __init__(self, n_components: int, kernel: str = "linear", gamma=None, degree: int = 3, coef0: float = 1.0,
                 ctx: Optional[Context] = None):
        self._k = int(n_components)
        self.kernel, self.gamma, self.degree, self.coef0 = kernel, gamma, int(degree), float(coef0)
        self.ctx = ctx
        self._h = None

    def n_components(self):
        return self._k

    def _inner_fit(self, x, want_y: bool):
        keep = []
        mx = describe(x, keep)
        ctx = self._ctx()
        spec = _kernel_spec(self.kernel, self.gamma, self.degree, self.coef0)
        y, my = _out_like(x, mx.rows, self._k, mx.dtype, keep) if want_y else (None, None)
        h = C.c_void_p()
        ctx.check(ctx.lib.petal_kpca_fit(ctx._h, C.byref(mx), self._k, C.byref(spec), C.byref(h), _ref(my)))
        self._adopt(ctx, h)
        return y

    def transform(self, x):
        keep = []
        mx = describe(x, keep)
        ctx = self._ctx()
        y, my = _out_like(x, mx.rows, self._k, mx.dtype, keep)
        ctx.check(ctx.lib.petal_kpca_transform(ctx._h, self._handle(), C.byref(mx), C.byref(my)))
        return y

    def _get(self, lam=None, vec=None):
        h = self._handle()   # (first: an unfitted model may have no ctx yet)
        out = (C.c_int64 * 8)()
        if self._ctx().lib.petal_kpca_get(h, _dp(lam), _dp(vec), out) != PETAL_OK:
            raise InvalidInput("petal_kpca_get failed")
        return out

    def eigenvalues(self):
        """The k leading eigenvalues of the centred kernel matrix, float64, as computed (descending)."""
        lam = np.zeros(self._k)
        self._get(lam=lam)
        return lam

    def scaled_eigenvectors(self):
        """V lambda^(-1/2), n x k float64, signs applied; a zero column where the component is undetermined."""
        vec = np.zeros((self.info()["n"], self._k))
        self._get(vec=vec)
        return vec

    def info(self) -> dict:
        """n, d, k, ``fit_kernel`` (k_kmap ran on the fit's map), ``transform_kernel`` (k_kapply ran on the last transform; -1 before
        the first), ``order`` of the eigenproblem, kernel, ``topk_solver`` (1: the top-k subspace iteration delivered the eigenpairs; 0: the
        full eigen-solver of order n ran -- the slower fit)."""
        keys = ("n", "d", "k", "fit_kernel", "transform_kernel", "order", "kernel", "topk_solver")
        return dict(zip(keys, (int(v) for v in self._get())))


def _nmf_spec(max_iter, tol, l1_w, l2_w, l1_h=0.0, l2_h=0.0) -> petal_nmf_spec:
    return petal_nmf_spec(int(max_iter), float(tol), float(l1_w), float(l2_w), float(l1_h), float(l2_h))


def _nmf_pass_operands(x, w, h, ctx):
    """the operands the three dense pass aids share: (keep, x described, ctx, w and h as contiguous float64 of matching shapes, k)"""
    keep = []
    mx = describe(x, keep)
    ctx = ctx or default_context()
    w, h = _f64c(w), _f64c(h)
    if w.ndim != 2 or h.ndim != 2 or w.shape[0] != mx.rows or h.shape != (w.shape[1], mx.cols):
        raise InvalidInput(f"w should be {mx.rows} x k and h k x {mx.cols}")
    return keep, mx, ctx, w, h, w.shape[1]


def _nmf_sweep_operands(sx, g, f, transposed):
    """the operands the two sweep aids share: (rows of the image swept, g and f as contiguous float64 of matching shapes, k)"""
    rows, inner = (sx.shape[1], sx.shape[0]) if transposed else sx.shape
    g, f = _f64c(g), _f64c(f)
    if g.ndim != 2 or f.ndim != 2 or g.shape[0] != rows or f.shape != (inner, g.shape[1]):
        raise InvalidInput(f"g should be {rows} x k and f {inner} x k")
    return rows, g, f, g.shape[1]


def nmf_pass(x, w, h, l1_w=0.0, l2_w=0.0, inner_iters=1, want_ab=True, ctx: Optional["Context"] = None, want_info: bool = False):
    """Test aid (``petal_nmf_pass``, include/petal_hip_nmf.h): the fused pass of an ``Nmf`` iteration by itself, in float64.  ``x``
    (n x d): numpy or ``torch.cuda``, any strides; ``w`` (n x k), ``h`` (k x d): float64.  Z = x h^T once, then ``inner_iters`` times
    D = W (h h^T) + l1_w + l2_w W, D[D == 0] = 2^-23, W <- W o Z / D.  Returns ``(w_new, a, b)`` with a = w_new^T x and
    b = w_new^T w_new (``want_ab=False``: ``w_new`` alone).  ``want_info``: also ``{"kernel": k_nmf_pass ran}``."""
    keep, mx, ctx, w, h, k = _nmf_pass_operands(x, w, h, ctx)
    spec = _nmf_spec(1, 0.0, l1_w, l2_w)
    wo = np.zeros((mx.rows, k))
    a = np.zeros((k, mx.cols)) if want_ab else None
    b = np.zeros((k, k)) if want_ab else None
    info = (C.c_int64 * 1)()
    ctx.check(ctx.lib.petal_nmf_pass(ctx._h, C.byref(mx), k, _dp(w), _dp(h), C.byref(spec), int(inner_iters), _dp(wo), _dp(a), _dp(b), info))
    return _with_info((wo, a, b) if want_ab else wo, info, want_info)


def nmf_sweep(sx: "CsrMatrix", g, f, transposed: bool = False, l1=0.0, l2=0.0, inner_iters=1, want_gram=True, want_info: bool = False):
    """Test aid (``petal_nmf_sweep_csr``, include/petal_hip_nmf_sparse.h): one sweep of sparse ``Nmf`` by itself, in float64, over the
    matrix (``transposed=False``: R x C = ``sx.shape``) or its transposed image.  ``g`` (R x k) is updated, ``f`` (C x k) gathered:
    z_r = sum over the stored entries of row r of val f[idx], then ``inner_iters`` times D = g_r (f^T f) + l1 + l2 g_r,
    D[D == 0] = 2^-23, g_r <- g_r o z_r / D.  Returns ``(g_new, gram, dot)`` with gram = g_new^T g_new and dot = sum_r <z_r, g_new_r>
    (``want_gram=False``: ``g_new`` alone).  ``want_info``: also ``{"kernel": k_nmf_sweep ran}``."""
    rows, g, f, k = _nmf_sweep_operands(sx, g, f, transposed)
    spec = _nmf_spec(1, 0.0, l1, l2)
    go = np.zeros((rows, k))
    gram = np.zeros((k, k)) if want_gram else None
    dot = np.zeros(1) if want_gram else None
    info = (C.c_int64 * 1)()
    ctx = sx.ctx
    ctx.check(ctx.lib.petal_nmf_sweep_csr(ctx._h, sx._handle(), int(bool(transposed)), k, _dp(g), _dp(f), C.byref(spec), int(inner_iters),
                                          _dp(go), _dp(gram), _dp(dot), info))
    return _with_info((go, gram, float(dot[0])) if want_gram else go, info, want_info)


def nmf_kl_sweep(sx: "CsrMatrix", g, f, transposed: bool = False, l1=0.0, l2=0.0, inner_iters=1, want_term: Optional[bool] = None,
                 want_info: bool = False):
    """Test aid (``petal_nmf_kl_sweep_csr``, include/petal_hip_nmf_kl.h): one Kullback-Leibler sweep of sparse ``Nmf`` by itself, in
    float64, over the matrix (``transposed=False``: R x C = ``sx.shape``) or its transposed image.  ``g`` (R x k) is updated, ``f``
    (C x k) gathered, c = colsum(f): ``inner_iters`` times, for every stored entry of row r, wh = max(<g_r, f[idx]>, 2^-23),
    num = sum val / wh f[idx], den = c + l1 + l2 g_r, den[den == 0] = 2^-23, g_r <- g_r o num / den.  Returns ``(g_new, colsum)`` with
    colsum = the column sums of g_new; with ``inner_iters=0`` (``want_term`` defaults to that) ``(g, colsum, term)`` with
    term = sum [val > 2^-23] val log(val / wh).  ``want_info``: also ``{"kernel": k_nmf_kl_sweep ran}``."""
    rows, g, f, k = _nmf_sweep_operands(sx, g, f, transposed)
    if want_term is None:
        want_term = int(inner_iters) == 0
    spec = _nmf_spec(1, 0.0, l1, l2)
    go, colsum, term = np.zeros((rows, k)), np.zeros(k), np.zeros(1)
    info = (C.c_int64 * 1)()
    ctx = sx.ctx
    ctx.check(ctx.lib.petal_nmf_kl_sweep_csr(ctx._h, sx._handle(), int(bool(transposed)), k, _dp(g), _dp(f), C.byref(spec), int(inner_iters),
                                             _dp(go), _dp(colsum), _dp(term) if want_term else None, info))
    return _with_info((go, colsum, float(term[0])) if want_term else (go, colsum), info, want_info)


def nmf_kl_pass(x, w, h, l1_w=0.0, l2_w=0.0, inner_iters=1, want_a=True, want_term: Optional[bool] = None,
                ctx: Optional["Context"] = None, want_info: bool = False):
    """Test aid (``petal_nmf_kl_pass``, include/petal_hip_nmf_kl_dense.h): the fused pass of a dense Kullback-Leibler ``Nmf`` iteration
    by itself, in float64.  ``x`` (n x d): numpy or ``torch.cuda``, any strides; ``w`` (n x k), ``h`` (k x d): float64.
    ``inner_iters`` times WH = max(W h, 2^-23), den = rowsum(h) + l1_w + l2_w W, den[den == 0] = 2^-23,
    W <- W o (((x / WH) h^T) / den).  Returns ``(w_new, a, colsum)`` with a = w_new^T (x / max(w_new h, 2^-23)) and colsum = the column
    sums of w_new (``want_a=False``: ``w_new`` alone); with ``inner_iters=0`` (``want_term`` defaults to that) ``(w, a, colsum, term)``
    with term = sum [x > 2^-23] x log(x / WH).  ``want_info``: also ``{"kernel": k_nmf_kl_pass ran}``."""
    keep, mx, ctx, w, h, k = _nmf_pass_operands(x, w, h, ctx)
    if want_term is None:
        want_term = int(inner_iters) == 0
    spec = _nmf_spec(1, 0.0, l1_w, l2_w)
    wo, a, colsum, term = np.zeros((mx.rows, k)), np.zeros((k, mx.cols)), np.zeros(k), np.zeros(1)
    info = (C.c_int64 * 1)()
    ctx.check(ctx.lib.petal_nmf_kl_pass(ctx._h, C.byref(mx), k, _dp(w), _dp(h), C.byref(spec), int(inner_iters), _dp(wo),
                                        _dp(a) if want_a else None, _dp(colsum) if want_a else None, _dp(term) if want_term else None, info))
    out = ((wo, a, colsum, float(term[0])) if want_term else (wo, a, colsum)) if want_a or want_term else wo
    return _with_info(out, info, want_info)


def nmf_cd_pass(x, w, h, l1_w=0.0, l2_w=0.0, inner_iters=1, from_zero: bool = False, want_ab=True, ctx: Optional["Context"] = None,
                want_info: bool = False):
    """Test aid (``petal_nmf_cd_pass``, include/petal_hip_nmf_cd.h): the fused pass of a coordinate-descent ``Nmf`` iteration by
    itself, in float64.  ``x`` (n x d): numpy or ``torch.cuda``, any strides; ``w`` (n x k), ``h`` (k x d): float64.  Z = x h^T once,
    then ``inner_iters`` Gauss-Seidel sweeps of every row of W with S = h h^T + l2_w I and z = Z - l1_w (``from_zero``: W starts as
    zeros).  Returns ``(w_new, a, b, violation)`` with a = w_new^T x, b = w_new^T w_new and violation = one sum of |pg| per sweep
    (``want_ab=False``: ``(w_new, violation)``).  ``want_info``: also ``{"kernel": k_nmf_cd_pass ran}``."""
    keep, mx, ctx, w, h, k = _nmf_pass_operands(x, w, h, ctx)
    spec = _nmf_spec(1, 0.0, l1_w, l2_w)
    wo = np.zeros((mx.rows, k))
    a = np.zeros((k, mx.cols)) if want_ab else None
    b = np.zeros((k, k)) if want_ab else None
    viol = np.zeros(max(int(inner_iters), 0))
    info = (C.c_int64 * 1)()
    ctx.check(ctx.lib.petal_nmf_cd_pass(ctx._h, C.byref(mx), k, _dp(w), _dp(h), C.byref(spec), int(inner_iters), int(bool(from_zero)),
                                        _dp(wo), _dp(a), _dp(b), _dp(viol) if viol.size else None, info))
    return _with_info((wo, a, b, viol) if want_ab else (wo, viol), info, want_info)


def nmf_cd_sweep(sx: "CsrMatrix", g, f, transposed: bool = False, l1=0.0, l2=0.0, inner_iters=1, from_zero: bool = False, want_gram=True,
                 want_info: bool = False):
    """Test aid (``petal_nmf_cd_sweep_csr``, include/petal_hip_nmf_cd_sparse.h): one coordinate-descent sweep of sparse ``Nmf`` by
    itself, in float64, over the matrix (``transposed=False``: R x C = ``sx.shape``) or its transposed image.  ``g`` (R x k) is updated
    (``from_zero``: from zeros), ``f`` (C x k) gathered: z_r = sum over the stored entries of row r of val f[idx], then ``inner_iters``
    Gauss-Seidel sweeps of g_r with S = f^T f + l2 I and z = z_r - l1.  Returns ``(g_new, gram, dot, violation)`` with
    gram = g_new^T g_new, dot = sum_r <z_r, g_new_r> and one violation per sweep (``want_gram=False``: ``(g_new, violation)``).
    ``want_info``: also ``{"kernel": k_nmf_cd_sweep ran}``."""
    rows, g, f, k = _nmf_sweep_operands(sx, g, f, transposed)
    spec = _nmf_spec(1, 0.0, l1, l2)
    go = np.zeros((rows, k))
    gram = np.zeros((k, k)) if want_gram else None
    dot = np.zeros(1) if want_gram else None
    viol = np.zeros(max(int(inner_iters), 0))
    info = (C.c_int64 * 1)()
    ctx = sx.ctx
    ctx.check(ctx.lib.petal_nmf_cd_sweep_csr(ctx._h, sx._handle(), int(bool(transposed)), k, _dp(g), _dp(f), C.byref(spec), int(inner_iters),
                                             int(bool(from_zero)), _dp(go), _dp(gram), _dp(dot), _dp(viol), info))
    return _with_info((go, gram, float(dot[0]), viol) if want_gram else (go, viol), info, want_info)


def nmf_cd_hupdate(a, b, h, l1_h=0.0, l2_h=0.0, ctx: Optional["Context"] = None, want_info: bool = False):
    """Test aid (``petal_nmf_cd_hupdate``, include/petal_hip_nmf_cd.h): the H side of a coordinate-descent ``Nmf`` iteration by itself,
    in float64: one sweep of every row of h^T with S = b + l2_h I and z = a[:, j] - l1_h.  ``a``, ``h`` (k x d), ``b`` (k x k).
    Returns ``(h_new, violation)``.  ``want_info``: also ``{"kernel": k_nmf_cd_hrule ran}``."""
    ctx = ctx or default_context()
    a, b, h = _f64c(a), _f64c(b), _f64c(h)
    if a.ndim != 2 or a.shape != h.shape or b.shape != (a.shape[0], a.shape[0]):
        raise InvalidInput("a and h should be k x d and b k x k")
    k, d = a.shape
    spec = _nmf_spec(1, 0.0, 0.0, 0.0, l1_h, l2_h)
    ho, viol = np.zeros((k, d)), np.zeros(1)
    info = (C.c_int64 * 1)()
    ctx.check(ctx.lib.petal_nmf_cd_hupdate(ctx._h, k, d, _dp(a), _dp(b), _dp(h), C.byref(spec), _dp(ho), _dp(viol), info))
    return _with_info((ho, float(viol[0])), info, want_info)


def _like_input(x, w):
    """w (a numpy array computed on the host) where x lives: a torch tensor on x's device for a torch x"""
    if _is_torch(x):
        import torch
        return torch.from_numpy(w).to(x.device)
    return w


def _beta_loss_code(beta_loss) -> int:
    if isinstance(beta_loss, str):
        if beta_loss in ("frobenius", "kullback-leibler"):
            return NMF_LOSS_FROBENIUS if beta_loss == "frobenius" else NMF_LOSS_KL
    elif not isinstance(beta_loss, bool) and beta_loss in (1, 2):
        return NMF_LOSS_KL if beta_loss == 1 else NMF_LOSS_FROBENIUS
    raise InvalidInput(f"unknown beta_loss {beta_loss!r} ('frobenius' / 2 or 'kullback-leibler' / 1)")


class _DenseAsCsr:
    """the CSR of the non-zero entries of a dense array, row by row in column order (what the Kullback-Leibler loss reads of it)"""

    def __init__(self, x):
        if _is_torch(x):
            x = x.detach().cpu().numpy()   # (a device tensor is copied to the host: the compression runs there)
        x = np.asarray(x)
        if x.ndim != 2:
            raise InvalidInput("expected a 2-D array")
        if x.dtype not in (np.float32, np.float64):
            x = x.astype(np.float64)
        r, c = np.nonzero(x)
        self.indptr = np.zeros(x.shape[0] + 1, dtype=np.int64)
        np.cumsum(np.bincount(r, minlength=x.shape[0]), out=self.indptr[1:])
        self.data, self.indices, self.shape = x[r, c], c.astype(np.int32), x.shape


class Nmf(_HandleOwner):
    """Non-negative matrix factorisation X ~ W H (``petal_nmf``, include/petal_hip_nmf.h; an extension beyond the crate, DESIGN.md
    sections 4 and 7) -- scikit-learn's ``NMF(solver="mu", beta_loss="frobenius")``.  ``fit``, ``fit_transform`` and ``transform``
    also take a ``CsrMatrix`` or any object with ``.data / .indices / .indptr / .shape`` (include/petal_hip_nmf_sparse.h).  ``init="random"`` draws W0 and H0 from
    ``Pcg(seed)``; ``init="custom"`` takes them from ``fit_transform(x, W=..., H=...)``.  ``alpha_W``, ``alpha_H`` ("same": alpha_W)
    and ``l1_ratio`` are scikit-learn's penalties.  ``tol > 0`` stops at a check every 10th iteration; ``transform`` runs exactly
    ``max_iter`` W-updates in one pass over its input.  Everything is float64 inside; outputs are rounded once to the data's type.
    The fitted model lives with its ctx.

    ``beta_loss="kullback-leibler"`` (or 1; include/petal_hip_nmf_kl.h) fits the generalised Kullback-Leibler divergence instead of the
    Frobenius loss ("frobenius" or 2, the default).  It runs on sparse input at the stored entries alone: a dense array is compressed
    here, on the host, to the CSR of its non-zero entries (a ``torch.cuda`` tensor is copied to the host for that) and takes the same
    path; at most 64 components; ``transform`` then costs ``max_iter`` sweeps.  ``beta_loss`` is readable.

    ``dense_path`` chooses the route of DENSE input under that loss (include/petal_hip_nmf_kl_dense.h).  ``"compress"``, the default,
    is the route above; ``"fused"`` sends the array as it is to the fused dense pass k_nmf_kl_pass: a ``torch.cuda`` tensor goes
    zero-copy and the results stay on its device, ``transform`` reads its input once whatever ``max_iter`` is, there is no cap on the
    components (outside the kernel's envelope the library's composed path runs), and ``kernel_path`` says whether the kernel ran (1)
    or the composed path (0).  The default stays ``"compress"`` only because existing callers are pinned to its bytes; a measured
    crossover may move it in a later change.  Under the Frobenius loss the keyword is read and changes nothing.

    ``solver`` (include/petal_hip_nmf_cd.h): ``"mu"``, the default, is everything above, byte for byte; ``"cd"`` is scikit-learn's
    coordinate-descent solver (its default, ``shuffle=False``) on dense input under the Frobenius loss: one fused pass k_nmf_cd_pass
    per iteration, scikit-learn's stopping rule after every iteration when ``tol > 0`` (``tol = 0``: exactly ``max_iter``
    iterations), ``transform`` from W = 0 with exactly ``max_iter`` sweeps.  ``"cd"`` with the Kullback-Leibler loss or with sparse
    input is ``InvalidInput``.  ``solver`` is readable.

    ``sparse_path`` chooses what ``solver="cd"`` does with sparse input (include/petal_hip_nmf_cd_sparse.h).  ``"refuse"``, the
    default, is the refusal above; ``"sweep"`` lets ``fit``, ``fit_transform`` and ``transform`` take a ``CsrMatrix`` or an object with
    ``.data / .indices / .indptr / .shape``: two fused gather sweeps k_nmf_cd_sweep per iteration, X never densified, at most 64
    components on the kernel (more, or ``nmf_fallback``, densify), and ``kernel_path`` says whether the sweep ran (1) or the call
    densified (0).  The default stays ``"refuse"`` only because existing callers are pinned to its messages; it may move in a later
    change.  Under ``solver="mu"`` the keyword is read and changes nothing."""

    _destroy, _no_handle = "petal_nmf_destroy", "the model has not been fitted (or its ctx was closed)"

    def __init__(self, n_components: int, max_iter: int = 200, tol: float = 1e-4, init: str = "random", seed: int = 0,
                 alpha_W: float = 0.0, alpha_H="same", l1_ratio: float = 0.0, ctx: Optional[Context] = None, beta_loss="frobenius",
                 dense_path: str = "compress", solver: str = "mu", sparse_path: str = "refuse"):
        if init not in ("random", "custom"):
            raise InvalidInput(f"unknown init {init!r} (random or custom)")
        if dense_path not in ("compress", "fused"):
            raise InvalidInput(f"unknown dense_path {dense_path!r} (compress or fused)")
        if not isinstance(solver, str) or solver not in ("mu", "cd"):
            raise InvalidInput(f"unknown solver {solver!r} (mu or cd)")
        if not isinstance(sparse_path, str) or sparse_path not in ("refuse", "sweep"):
            raise InvalidInput(f"unknown sparse_path {sparse_path!r} (refuse or sweep)")
        self.dense_path = dense_path
        self.solver = solver
        self.sparse_path = sparse_path
        self._loss = _beta_loss_code(beta_loss)
        if solver == "cd" and self._loss != NMF_LOSS_FROBENIUS:
            raise InvalidInput("solver='cd' does not take the kullback-leibler loss (the coordinate-descent solver is for the frobenius loss)")
        self.beta_loss = "frobenius" if self._loss == NMF_LOSS_FROBENIUS else "kullback-leibler"
        self._k = int(n_components)
        self.max_iter, self.tol, self.init, self.seed = int(max_iter), float(tol), init, int(seed)
        self.alpha_W, self.alpha_H, self.l1_ratio = float(alpha_W), alpha_H, float(l1_ratio)
        self.ctx = ctx
        self._h = None
        self.kernel_path = None   # the last fit / transform on sparse input: 1 the sweep kernel ran, 0 the call densified

    def n_components(self):
        return self._k

    def _spec(self, n, d) -> petal_nmf_spec:
        a_w = self.alpha_W
        a_h = a_w if isinstance(self.alpha_H, str) else float(self.alpha_H)
        if isinstance(self.alpha_H, str) and self.alpha_H != "same":
            raise InvalidInput("alpha_H should be a number or 'same'")
        rho = self.l1_ratio
        return _nmf_spec(self.max_iter, self.tol, d * a_w * rho, d * a_w * (1.0 - rho), n * a_h * rho, n * a_h * (1.0 - rho))

    def _start(self, dtype_code, W, H, keep):
        """(w0, h0) as petal_matrix descriptions (init="custom") or (None, None)"""
        if self.init == "custom":
            if W is None or H is None:
                raise InvalidInput("init='custom' needs W and H")
            dt = _np_dtype(dtype_code)
            return (describe(W if _is_torch(W) else np.asarray(W, dtype=dt), keep),
                    describe(H if _is_torch(H) else np.asarray(H, dtype=dt), keep))
        if W is not None or H is not None:
            raise InvalidInput("W and H are read with init='custom' only")
        return None, None

    def _inner_fit_sparse(self, x, W, H, want_w: bool):
        """fit / fit_transform on sparse input (include/petal_hip_nmf_sparse.h): X is never densified where the sweep kernel runs;
        ``kernel_path`` says whether it did (1) or the library densified and ran the dense fit (0)."""
        with self._sparse(x) as sx:
            ctx = self._ctx()
            rows, cols = sx.shape
            spec = self._spec(rows, cols)
            keep = []
            mw, mh = self._start(sx._dt, W, H, keep)
            w, mo = None, None
            if want_w:
                w = np.empty((rows, self._k), dtype=_np_dtype(sx._dt))
                mo = describe(w, keep)
            h, path = C.c_void_p(), C.c_int64(0)
            args = (_ref(mw), _ref(mh), C.c_int64(self.seed & ((1 << 64) - 1)), C.byref(h), _ref(mo), C.byref(path))
            if self.solver == "cd":   # sparse_path="sweep" (include/petal_hip_nmf_cd_sparse.h)
                ctx.check(ctx.lib.petal_nmf_fit_csr_solver(ctx._h, sx._handle(), self._k, C.byref(spec), NMF_SOLVER_CD, *args))
            elif self._loss == NMF_LOSS_FROBENIUS:
                ctx.check(ctx.lib.petal_nmf_fit_csr(ctx._h, sx._handle(), self._k, C.byref(spec), *args))
            else:
                ctx.check(ctx.lib.petal_nmf_fit_csr_loss(ctx._h, sx._handle(), self._k, C.byref(spec), self._loss, *args))
            self._adopt(ctx, h)
            self.kernel_path = int(path.value)
            return w

    def _inner_fit(self, x, W, H, want_w: bool):
        if self.solver == "cd" and self.sparse_path != "sweep" and _is_sparse(x):
            raise InvalidInput("solver='cd' does not take sparse (CSR) input in this version")
        if _is_sparse(x):
            return self._inner_fit_sparse(x, W, H, want_w)
        if self._loss == NMF_LOSS_KL and self.dense_path == "compress":   # the CSR of the non-zero entries, the same path
            w = self._inner_fit_sparse(_DenseAsCsr(x), W, H, want_w)
            return _like_input(x, w) if want_w else None
        keep = []
        mx = describe(x, keep)
        ctx = self._ctx()
        spec = self._spec(mx.rows, mx.cols)
        mw, mh = self._start(mx.dtype, W, H, keep)
        w, mo = _out_like(x, mx.rows, self._k, mx.dtype, keep) if want_w else (None, None)
        h = C.c_void_p()
        args = (_ref(mw), _ref(mh), C.c_int64(self.seed & ((1 << 64) - 1)), C.byref(h), _ref(mo))
        if self.solver == "cd":   # include/petal_hip_nmf_cd.h
            ctx.check(ctx.lib.petal_nmf_fit_solver(ctx._h, C.byref(mx), self._k, C.byref(spec), NMF_SOLVER_CD, *args))
        elif self._loss == NMF_LOSS_FROBENIUS:
            ctx.check(ctx.lib.petal_nmf_fit(ctx._h, C.byref(mx), self._k, C.byref(spec), *args))
        else:   # dense_path="fused" (include/petal_hip_nmf_kl_dense.h)
            ctx.check(ctx.lib.petal_nmf_fit_loss(ctx._h, C.byref(mx), self._k, C.byref(spec), self._loss, *args))
        self._adopt(ctx, h)
        if self._loss != NMF_LOSS_FROBENIUS:
            self.kernel_path = self.info()["fit_kernel"]
        return w

    def fit(self, x, W=None, H=None):
        self._inner_fit(x, W, H, False)
        return self

    def fit_transform(self, x, W=None, H=None):
        return self._inner_fit(x, W, H, True)

    def transform(self, x):
        """``max_iter`` W-updates with H fixed; sparse input (a CsrMatrix or an object with .data / .indices / .indptr / .shape) goes
        through the sparse sweep and sets ``kernel_path``."""
        self._handle()
        dense_kl = not _is_sparse(x) and self._model_loss() == NMF_LOSS_KL
        if dense_kl and self.dense_path == "compress":
            return _like_input(x, self.transform(_DenseAsCsr(x)))
        if _is_sparse(x):
            with self._sparse(x) as sx:
                ctx = self._ctx()
                keep = []
                w = np.empty((sx.shape[0], self._k), dtype=_np_dtype(sx._dt))
                mo = describe(w, keep)
                path = C.c_int64(0)
                entry = ctx.lib.petal_nmf_transform_csr_solver if self.sparse_path == "sweep" else ctx.lib.petal_nmf_transform_csr
                ctx.check(entry(ctx._h, self._handle(), sx._handle(), C.byref(mo), C.byref(path)))
                self.kernel_path = int(path.value)
                return w
        keep = []
        mx = describe(x, keep)
        ctx = self._ctx()
        w, mo = _out_like(x, mx.rows, self._k, mx.dtype, keep)
        if dense_kl:   # dense_path="fused" (include/petal_hip_nmf_kl_dense.h)
            ctx.check(ctx.lib.petal_nmf_transform_loss(ctx._h, self._handle(), C.byref(mx), C.byref(mo)))
            self.kernel_path = self.info()["transform_kernel"] if mx.rows else self.kernel_path
        else:
            ctx.check(ctx.lib.petal_nmf_transform(ctx._h, self._handle(), C.byref(mx), C.byref(mo)))
        return w

    def inverse_transform(self, w):
        keep = []
        mw = describe(w, keep)
        ctx = self._ctx()
        x, mo = _out_like(w, mw.rows, self.info()["d"], mw.dtype, keep)
        ctx.check(ctx.lib.petal_nmf_inverse_transform(ctx._h, self._handle(), C.byref(mw), C.byref(mo)))
        return x

    def _get(self, comp=None, err=None):
        h = self._handle()   # (first: an unfitted model may have no ctx yet)
        out = (C.c_int64 * 6)()
        if self._ctx().lib.petal_nmf_get(h, _dp(comp), out, _dp(err)) != PETAL_OK:
            raise InvalidInput("petal_nmf_get failed")
        return out

    def _model_loss(self) -> int:
        out = C.c_int64(0)
        if self._ctx().lib.petal_nmf_get_loss(self._handle(), C.byref(out)) != PETAL_OK:
            raise InvalidInput("petal_nmf_get_loss failed")
        return int(out.value)

    def info(self) -> dict:
        """n, d, k, ``n_iter``, ``fit_kernel`` (k_nmf_pass ran in the fit; 0: the composed path), ``transform_kernel`` (the same for
        the last transform; -1 before the first)."""
        keys = ("n", "d", "k", "n_iter", "fit_kernel", "transform_kernel")
        return dict(zip(keys, (int(v) for v in self._get())))

    @property
    def components(self):
        """H, k x d float64."""
        i = self.info()
        comp = np.zeros((i["k"], i["d"]))
        self._get(comp=comp)
        return comp

    @property
    def n_iter(self) -> int:
        return self.info()["n_iter"]

    @property
    def reconstruction_err(self) -> float:
        err = np.zeros(2)
        self._get(err=err)
        return float(err[0])

    @property
    def err_init(self) -> float:
        err = np.zeros(2)
        self._get(err=err)
        return float(err[1])


# ------------------------------------------------------------------------------------------------
class _PcaModel(_CtxUser):
    """State shared by Pca and RandomizedPca (src/pca.rs:41-51, 317-329)."""

    def __init__(self, n_components: int, centering: bool = True, ctx: Optional[Context] = None):
        self._k = int(n_components)
        self.centering = bool(centering)
        self.ctx = ctx
        self._components = np.zeros((self._k, 0))
        self._means = np.zeros(0)
        self._singular = np.zeros(0)
        self._total_variance = 0.0
        self.n_samples = 0
        self._dt = PETAL_F64

    # accessors (src/pca.rs:78-105, 392-419)
    def components(self):
        return self._components

    def mean(self):
        return self._means

    def n_components(self):
        return self._k

    def singular_values(self):
        return self._singular

    def explained_variance_ratio(self):
        return self._singular * self._singular / self._total_variance

    # scores of rows against the fitted model: an extension beyond the crate (include/petal_hip_score.h)
    def explained_variance(self):
        """lambda_j = sigma_j^2 / (n_samples - 1), the variance along each kept component."""
        return self._singular * self._singular / (self.n_samples - 1)

    def noise_variance(self):
        """The mean variance of the min(n_samples, d) - k discarded directions, as scikit-learn defines it (0 when none is discarded)."""
        rest = min(self.n_samples, self._means.shape[0]) - self._k
        if rest <= 0:
            return np.asarray(0.0, dtype=self._singular.dtype)[()]
        s = self._singular.astype(np.float64)
        return np.asarray((float(self._total_variance) - float(np.sum(s * s))) / (self.n_samples - 1) / rest, dtype=self._singular.dtype)[()]

    def _score(self, x, weights):
        if _is_sparse(x):
            raise InvalidInput("row scores (reconstruction_error, hotelling_t2, score_samples) are not available for sparse input")
        return score_rows(x, self._components, self._means, weights=weights, centering=self.centering, ctx=self._ctx())[0]

    def reconstruction_error(self, x):
        """|xc - (xc V^T) V|^2 per row (the Q / SPE statistic), as |xc|^2 - |xc V^T|^2 from one pass over x.  A difference: below about
        1e-5 |xc|^2 it is rounding noise for float32 input (float64 input: 1e-14)."""
        return self._score(x, None)[:, 0]

    def hotelling_t2(self, x):
        """sum_j y_j^2 / lambda_j per row, y = transform(x)."""
        lam = np.asarray(self.explained_variance(), dtype=np.float64)
        if not np.all(lam > 0):
            raise InvalidInput("a kept component has zero variance")
        return self._score(x, 1.0 / lam)[:, 1]

    def score_samples(self, x):
        """Log-likelihood of each row under the probabilistic-PCA model (scikit-learn's score_samples), from one pass over x:
        -1/2 [d log 2 pi + sum_j log lambda_j + (d - k) log s2 + residual / s2 + T^2], s2 = noise_variance()."""
        lam = np.asarray(self.explained_variance(), dtype=np.float64)
        s2 = float(self.noise_variance())
        if not s2 > 0:
            raise InvalidInput("the noise variance is not positive (no discarded direction, or an exactly low-rank fit)")
        if not np.all(lam > 0):
            raise InvalidInput("a kept component has zero variance")
        d = self._means.shape[0]
        sc = self._score(x, 1.0 / lam)
        const = d * np.log(2.0 * np.pi) + float(np.sum(np.log(lam))) + (d - self._k) * np.log(s2)
        return -0.5 * (const + sc[:, 0] / s2 + sc[:, 1])

    def _serde_fields(self) -> dict:
        dt = self._components.dtype if self._components.size or self._means.size else np.dtype(_np_dtype(self._dt))
        return {"components": _nd_to_serde(self._components), "n_samples": int(self.n_samples),
                "means": _nd_to_serde(self._means), "total_variance": float(np.asarray(self._total_variance, dtype=dt)),
                "singular": _nd_to_serde(self._singular), "centering": bool(self.centering)}

    def _load_serde_fields(self, obj: dict, dtype):
        self._components = _nd_from_serde(obj["components"], dtype)
        self.n_samples = int(obj["n_samples"])
        self._means = _nd_from_serde(obj["means"], dtype)
        self._total_variance = np.asarray(obj["total_variance"], dtype=dtype)[()]
        self._singular = _nd_from_serde(obj["singular"], dtype)
        self.centering = bool(obj["centering"])
        self._k = int(self._components.shape[0])
        self._dt = PETAL_F32 if np.dtype(dtype) == np.float32 else PETAL_F64

    def to_json(self) -> str:
        """The JSON ``serde_json::to_string(&model)`` writes for the reference struct (src/pca.rs:941, 1035)."""
        import json
        return json.dumps(self._serde_fields())

    def _store(self, comp, means, sing, tv, n):
        self._components, self._means, self._singular = comp, means, sing
        self._total_variance = tv[0]
        self.n_samples = n

    def transform(self, x):
        """src/pca.rs:130-135 / 444-449."""
        keep = []
        mx = describe(x, keep)
        ctx = self._ctx()
        d = self._means.shape[0]
        if mx.cols != d:
            raise InvalidInput(f"# of columns should be {d}")
        y, my = _out_like(x, mx.rows, self._k, mx.dtype, keep)
        comp = _host(self._components, mx.dtype)
        mu = _host(self._means, mx.dtype)
        ctx.check(ctx.lib.petal_transform(ctx._h, C.byref(mx), comp.ctypes.data, mu.ctypes.data, self._k, d,
                                          int(self.centering), C.byref(my)))
        return y

    def inverse_transform(self, y):
        """src/pca.rs:176-184 / 490-498."""
        keep = []
        my = describe(y, keep)
        ctx = self._ctx()
        d = self._means.shape[0]
        if my.cols != self._k:
            raise InvalidInput(f"# of columns should be {self._k}")
        x, mx = _out_like(y, my.rows, d, my.dtype, keep)
        comp = _host(self._components, my.dtype)
        mu = _host(self._means, my.dtype)
        ctx.check(ctx.lib.petal_inverse_transform(ctx._h, C.byref(my), comp.ctypes.data, mu.ctypes.data, self._k, d,
                                                  int(self.centering), C.byref(mx)))
        return x


class Pca(_PcaModel, _FitsWithY):
    """``Pca<A>`` (src/pca.rs:41-232)."""

    @classmethod
    def new(cls, n_components: int, ctx: Optional[Context] = None):
        return cls(n_components, True, ctx)

    @classmethod
    def from_json(cls, text: str, dtype=np.float32, ctx: Optional[Context] = None):
        """``serde_json::from_str::<Pca<A>>`` (A = ``dtype``)."""
        import json
        obj = json.loads(text)
        m = cls(int(obj["components"]["dim"][0]), ctx=ctx)
        m._load_serde_fields(obj, dtype)
        return m

    def _inner_fit(self, x, want_y: bool):
        keep = []
        mx = describe(x, keep)
        ctx = self._ctx()
        npdt = _np_dtype(mx.dtype)
        comp = np.zeros((self._k, mx.cols), dtype=npdt)
        means = np.zeros(mx.cols, dtype=npdt)
        sing = np.zeros(self._k, dtype=npdt)
        tv = np.zeros(1, dtype=npdt)
        y, my = _out_like(x, mx.rows, self._k, mx.dtype, keep) if want_y else (None, None)
        ctx.check(ctx.lib.petal_pca_fit(ctx._h, C.byref(mx), self._k, int(self.centering), comp.ctypes.data,
                                        means.ctypes.data, sing.ctypes.data, tv.ctypes.data, _ref(my)))
        if not (self.centering and mx.rows == 0 and ctx.world_size == 1):
            self._store(comp, means, sing, tv, mx.rows)
        if want_y and mx.rows == 0 and self.centering:
            y = _alloc_like(x, 0, mx.cols if self._k else 0, mx.dtype)[:, : self._k]  # src/pca.rs:210
        return y

    def last_route(self) -> dict:
        """``petal_pca_last_route`` (include/petal_hip_wide.h): facts of the last ``Pca`` fit on this model's ctx -- ``route`` (0 the
        d x d Gram route, 1 the dual route of wide data), ``kernel`` (k_row_gram ran), ``order`` of the eigenproblem, feature ``chunks``."""
        ctx = self._ctx()
        out = (C.c_int64 * 4)()
        if ctx.lib.petal_pca_last_route(ctx._h, out) != PETAL_OK:
            raise InvalidInput("petal_pca_last_route failed")
        return {"route": int(out[0]), "kernel": int(out[1]), "order": int(out[2]), "chunks": int(out[3])}


def _lazy_field(name):
    """A model field of IncrementalPca: reading it brings the model up to date with the batches seen so far."""
    def get(self):
        self._refresh()
        return self.__dict__[name]

    def put(self, value):
        self.__dict__[name] = value
    return property(get, put)


class IncrementalPca(_HandleOwner, _PcaModel):
    """The exact ``Pca`` fitted batch by batch (``petal_ipca``, include/petal_hip_ipca.h; an extension beyond the crate, DESIGN.md
    section 7): ``partial_fit`` folds a batch into the float64 statistic (rows seen, mean, M2) resident with the ctx, and the model is
    what ``Pca.fit`` returns on the concatenation of the batches -- up to the SIGN of each component, which is decided from the
    component itself (its entry of largest magnitude is positive; scikit-learn's rule) because a streaming fit never holds U.

    The model is refreshed lazily: the first ``components()``, ``mean()``, ``singular_values()``, ``transform(...)`` ... after a batch
    solves the eigenproblem once; every member inherited from the Pca model then works unchanged.  d and dtype are fixed by the first
    batch.  Gram route only (no accurate small-sigma route): about eps64 (sigma_1 / sigma_j)^2 over the relative gap."""

    _components = _lazy_field("_components")
    _means = _lazy_field("_means")
    _singular = _lazy_field("_singular")
    _total_variance = _lazy_field("_total_variance")
    n_samples = _lazy_field("n_samples")

    def __init__(self, n_components: int, centering: bool = True, ctx: Optional[Context] = None):
        self._h, self._dirty, self._d = None, False, None
        super().__init__(n_components, centering, ctx)

    # ---- the handle -------------------------------------------------------------------------------------------------------------------
    _destroy, _no_handle = "petal_ipca_destroy", "no batch has been seen yet (or the model's ctx was closed)"

    def _open(self, d: int, dtype_code: int):
        ctx = self._ctx()
        h = C.c_void_p()
        ctx.check(ctx.lib.petal_ipca_create(ctx._h, int(d), int(dtype_code), int(self.centering), C.byref(h)))
        self._adopt(ctx, h)
        self._d, self._dt = int(d), int(dtype_code)

    def info(self) -> dict:
        """d, dtype, centering, rows seen, batches, batches the streaming kernel took, merges."""
        out = (C.c_int64 * 8)()
        if self.ctx.lib.petal_ipca_info(self._handle(), out) != PETAL_OK:
            raise InvalidInput("petal_ipca_info failed")
        keys = ("d", "dtype", "centering", "n_samples_seen", "batches", "kernel_batches", "merges")
        return dict(zip(keys, (int(v) for v in out)))

    @property
    def n_samples_seen(self) -> int:
        return self.info()["n_samples_seen"] if self._h else 0

    # ---- the statistic ----------------------------------------------------------------------------------------------------------------
    def partial_fit(self, x):
        """Fold one batch (host or device, float32 or float64; the first batch fixes d and dtype) into the statistic."""
        keep = []
        mx = describe(x, keep)
        if not self._h:
            self._open(mx.cols, mx.dtype)
        ctx = self._ctx()
        ctx.check(ctx.lib.petal_ipca_partial_fit(ctx._h, self._handle(), C.byref(mx)))
        self._dirty = True
        return self

    def fit(self, x, batch_size=None):
        """A fresh fit of x (host or device array) in row slices of ``batch_size`` (default 5 d, scikit-learn's)."""
        rows, cols = int(x.shape[0]), int(x.shape[1])
        if self._h:
            self.reset()
        step = max(int(batch_size) if batch_size else 5 * cols, 1)
        if rows == 0:
            self.partial_fit(x)
        for r in range(0, rows, step):
            self.partial_fit(x[r:r + step])
        return self

    def merge(self, other: "IncrementalPca"):
        """Add the statistic of another model (same ctx, d, dtype and centering), exactly: the pairwise form, free of the
        cancellation a drifting stream causes in ``partial_fit``.  ``other`` is unchanged."""
        if not other._h:
            return self
        if not self._h:
            if self.ctx is None:
                self.ctx = other.ctx
            self._open(other._d, other._dt)
        ctx = self._ctx()
        ctx.check(ctx.lib.petal_ipca_merge(ctx._h, self._handle(), other._handle()))
        self._dirty = True
        return self

    def reset(self):
        if self._h:
            self._ctx().check(self.ctx.lib.petal_ipca_reset(self._h))
        dt = self._dt
        _PcaModel.__init__(self, self._k, self.centering, self.ctx)
        self._dt, self._dirty = dt, False       # (the handle keeps its d and dtype)
        return self

    def state(self) -> dict:
        """The statistic as host float64 arrays: for checkpoints, and for combining the work of several processes or GPUs by hand."""
        ctx, d = self._ctx(), self._d
        self._handle()
        n, mean, m2 = C.c_double(0), np.zeros(d), np.zeros((d, d))
        ctx.check(ctx.lib.petal_ipca_get_state(ctx._h, self._h, C.byref(n), _dp(mean), _dp(m2)))
        return {"n": float(n.value), "mean": mean, "m2": m2, "dtype": _np_dtype(self._dt), "centering": self.centering}

    @classmethod
    def from_state(cls, state: dict, n_components: int, ctx: Optional[Context] = None):
        m = cls(n_components, bool(state["centering"]), ctx)
        mean = np.ascontiguousarray(state["mean"], dtype=np.float64)
        m2 = np.ascontiguousarray(state["m2"], dtype=np.float64)
        if m2.shape != (mean.shape[0], mean.shape[0]):
            raise InvalidInput("m2 should be d x d")
        m._open(mean.shape[0], PETAL_F32 if np.dtype(state["dtype"]) == np.float32 else PETAL_F64)
        c = m._ctx()
        c.check(c.lib.petal_ipca_set_state(c._h, m._h, float(state["n"]), _dp(mean), _dp(m2)))
        m._dirty = True
        return m

    # ---- the model --------------------------------------------------------------------------------------------------------------------
    def finalize(self, n_components=None):
        """(components, means, singular values, total variance) of the rows seen so far; the statistic is not modified."""
        ctx, d = self._ctx(), self._d
        h = self._handle()
        k = self._k if n_components is None else int(n_components)
        npdt = _np_dtype(self._dt)
        comp, means = np.zeros((max(k, 0), d), dtype=npdt), np.zeros(d, dtype=npdt)
        sing, tv = np.zeros(max(k, 0), dtype=npdt), np.zeros(1, dtype=npdt)
        ctx.check(ctx.lib.petal_ipca_finalize(ctx._h, h, k, comp.ctypes.data, means.ctypes.data, sing.ctypes.data, tv.ctypes.data))
        return comp, means, sing, tv

    def _refresh(self):
        if self.__dict__.get("_dirty") and self._h and self.n_samples_seen > 0:   # (nothing seen: the model stays empty, as an unfitted Pca's)
            comp, means, sing, tv = self.finalize()
            self._dirty = False   # (cleared first: _store assigns the fields this method guards)
            self._store(comp, means, sing, tv, self.info()["n_samples_seen"])


class SegmentedPca(_CtxUser):
    """One exact Pca per row segment of a row-sorted matrix, in one call (include/petal_hip_segments.h; an extension beyond the crate,
    DESIGN.md section 7).  Segment b is rows offsets[b] .. offsets[b + 1] - 1; it gets what ``Pca.fit`` gives on those rows alone.  For
    d <= 64 the batch is one launch, a workgroup per segment; a very long segment is correct and not fast (fit it with ``Pca``)."""

    def __init__(self, n_components: int, centering: bool = True, ctx: Optional[Context] = None):
        self._k = int(n_components)
        self.centering = bool(centering)
        self.ctx = ctx
        self._dt = PETAL_F64
        self._components = np.zeros((0, self._k, 0))
        self._means = np.zeros((0, 0))
        self._singular = np.zeros((0, self._k))
        self._total_variance = np.zeros(0)
        self._status = np.zeros(0, dtype=np.int32)
        self._kernel_segments = 0

    components = property(lambda self: self._components, doc="(B, k, d), svd_flip's sign applied")
    mean = property(lambda self: self._means, doc="(B, d)")
    singular_values = property(lambda self: self._singular, doc="(B, k)")
    status = property(lambda self: self._status, doc="(B) 0: fitted; 1: the segment held a NaN or an infinity, its results are NaN")
    kernel_segments = property(lambda self: self._kernel_segments, doc="how many segments of the last fit the segment kernel fitted")
    total_variance = property(lambda self: self._total_variance, doc="(B)")

    @property
    def explained_variance_ratio(self):
        return self._singular * self._singular / self._total_variance[:, None]

    @staticmethod
    def _rows(x, offsets, lengths):
        """(the 2-D matrix of all rows, offsets as int64[B + 1], the leading (B, n) of a 3-D input or None)"""
        shape = tuple(x.shape) if hasattr(x, "shape") else np.shape(x)
        lead = None
        if len(shape) == 3:
            if offsets is not None or lengths is not None:
                raise InvalidInput("a 3-D input has equal segments: no offsets / lengths")
            lead = (int(shape[0]), int(shape[1]))
            x = x.reshape(lead[0] * lead[1], shape[2]) if (_is_torch(x) or isinstance(x, np.ndarray)) else np.asarray(x).reshape(-1, shape[2])
            offsets = np.arange(lead[0] + 1, dtype=np.int64) * lead[1]
        elif lengths is not None:
            if offsets is not None:
                raise InvalidInput("give offsets or lengths, not both")
            offsets = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])
        elif offsets is None:
            raise InvalidInput("a 2-D input needs offsets or lengths")
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.int64).reshape(-1))
        if off.size < 1:
            raise InvalidInput("offsets needs n_segments + 1 values")
        return x, off, lead

    @staticmethod
    def _shaped(y, lead):
        return y if lead is None else y.reshape(lead[0], lead[1], y.shape[1])

    def _inner_fit(self, x, offsets, lengths, want_y: bool):
        x, off, lead = self._rows(x, offsets, lengths)
        keep = []
        mx = describe(x, keep)
        ctx = self._ctx()
        npdt = _np_dtype(mx.dtype)
        nseg, k, d = off.size - 1, self._k, mx.cols
        comp = np.zeros((nseg, k, d), dtype=npdt)
        means = np.zeros((nseg, d), dtype=npdt)
        sing = np.zeros((nseg, k), dtype=npdt)
        tv = np.zeros(nseg, dtype=npdt)
        status = np.zeros(nseg, dtype=np.int32)
        ks = C.c_int64(0)
        y, my = _out_like(x, mx.rows, k, mx.dtype, keep) if want_y else (None, None)
        ctx.check(ctx.lib.petal_pca_fit_segments(
            ctx._h, C.byref(mx), off.ctypes.data_as(_L), nseg, k, int(self.centering), comp.ctypes.data, means.ctypes.data,
            sing.ctypes.data, tv.ctypes.data, status.ctypes.data_as(C.POINTER(C.c_int32)), _ref(my), C.byref(ks)))
        self._components, self._means, self._singular, self._total_variance = comp, means, sing, tv
        self._status, self._kernel_segments, self._dt = status, int(ks.value), mx.dtype
        return None if y is None else self._shaped(y, lead)

    def fit(self, x, offsets=None, lengths=None):
        self._inner_fit(x, offsets, lengths, False)
        return self

    def fit_transform(self, x, offsets=None, lengths=None):
        return self._inner_fit(x, offsets, lengths, True)

    def _apply(self, entry, a, offsets, lengths, cols_in, cols_out):
        a, off, lead = self._rows(a, offsets, lengths)
        keep = []
        ma = describe(a, keep)
        ctx = self._ctx()
        nseg, d = self._means.shape
        if ma.cols != cols_in:
            raise InvalidInput(f"# of columns should be {cols_in}")
        if off.size - 1 != nseg:
            raise InvalidInput(f"the model holds {nseg} segments, offsets describe {off.size - 1}")
        out, mo = _out_like(a, ma.rows, cols_out, ma.dtype, keep)
        comp = _host(self._components, ma.dtype)
        mu = _host(self._means, ma.dtype)
        ctx.check(entry(ctx._h, C.byref(ma), off.ctypes.data_as(_L), nseg, comp.ctypes.data, mu.ctypes.data, self._k, d,
                        int(self.centering), C.byref(mo)))
        return self._shaped(out, lead)

    def transform(self, x, offsets=None, lengths=None):
        return self._apply(self._ctx().lib.petal_transform_segments, x, offsets, lengths, self._means.shape[1], self._k)

    def inverse_transform(self, y, offsets=None, lengths=None):
        return self._apply(self._ctx().lib.petal_inverse_transform_segments, y, offsets, lengths, self._k, self._means.shape[1])


class PcaBuilder:
    """``PcaBuilder`` (src/pca.rs:246-283)."""

    def __init__(self, n_components: int):
        self._k, self._centering, self._ctx = n_components, True, None

    @classmethod
    def new(cls, n_components: int):
        return cls(n_components)

    def centering(self, centering: bool):
        self._centering = centering
        return self

    def context(self, ctx: Context):
        self._ctx = ctx
        return self

    def build(self) -> Pca:
        return Pca(self._k, self._centering, self._ctx)


class RandomizedPca(_PcaModel):
    """``RandomizedPca<A, R>`` (src/pca.rs:317-551).  The model owns an RNG that advances on every
    fit (src/pca.rs:532); ``rng`` is anything with ``standard_normal(shape)`` filling in row-major order
    like src/pca.rs:701-705: the crate's ``Pcg`` (``with_seed`` / builder ``seed()``; restated PCG + Ziggurat,
    "stream parity unpinned") or a ``numpy.random.Generator`` (the default)."""

    N_OVERSAMPLE = 10  # src/pca.rs:679
    N_ITER = 7         # src/pca.rs:680

    def __init__(self, n_components, centering=True, rng=None, ctx=None, n_oversample=None, n_iter=None):
        super().__init__(n_components, centering, ctx)
        self.rng = rng if rng is not None else np.random.default_rng()
        self.n_oversample = self.N_OVERSAMPLE if n_oversample is None else int(n_oversample)
        self.n_iter = self.N_ITER if n_iter is None else int(n_iter)
        self.kernel_path = None   # sparse input: 1 when the sparse product kernel ran, 0 for the densifying fall-back

    @classmethod
    def new(cls, n_components: int, ctx=None):
        return cls(n_components, ctx=ctx)

    @classmethod
    def with_seed(cls, n_components: int, seed: int, ctx=None):
        """``Pcg::from_seed(seed.to_be_bytes())`` (src/pca.rs:356-359)."""
        return cls(n_components, rng=Pcg.from_seed_be_bytes(seed), ctx=ctx)

    def _serde_fields(self) -> dict:
        return {"rng": _rng_to_serde(self.rng), **super()._serde_fields()}

    @classmethod
    def from_json(cls, text: str, dtype=np.float32, ctx=None):
        """``serde_json::from_str::<RandomizedPca<A, Pcg>>``."""
        import json
        obj = json.loads(text)
        m = cls(int(obj["components"]["dim"][0]), rng=Pcg.from_serde(obj["rng"]), ctx=ctx)
        m._load_serde_fields(obj, dtype)
        return m

    @classmethod
    def with_rng(cls, n_components: int, rng, ctx=None):
        return cls(n_components, rng=rng, ctx=ctx)

    def draw_omega(self, d: int, dtype_code: int) -> np.ndarray:
        size = self._k + self.n_oversample
        return self.rng.standard_normal((d, size)).astype(_np_dtype(dtype_code))  # f64 draw cast to A::Real

    def _inner_fit_sparse(self, x, want_y: bool, omega=None):
        """fit / fit_transform on sparse input (include/petal_hip_sparse.h): X is never densified; ``kernel_path`` says whether the
        sparse product kernel ran (1) or the library's densifying fall-back (0: a device-op layer without the kernel)."""
        with self._sparse(x) as sx:
            ctx = self._ctx()
            rows, cols = sx.shape
            npdt = _np_dtype(sx._dt)
            if omega is None:
                omega = self.draw_omega(cols, sx._dt)
            omega = _host(omega, sx._dt, (cols, self._k + self.n_oversample))
            comp, means = np.empty((self._k, cols), dtype=npdt), np.zeros(cols, dtype=npdt)
            sing, tv = np.empty(self._k, dtype=npdt), np.zeros(1, dtype=npdt)
            keep, y, my = [], None, None
            if want_y:
                y = np.empty((rows, self._k), dtype=npdt)
                my = describe(y, keep)
            path = C.c_int64(0)
            ctx.check(ctx.lib.petal_rpca_fit_csr(ctx._h, sx._handle(), self._k, self.n_oversample, self.n_iter, int(self.centering),
                                                 omega.ctypes.data, comp.ctypes.data, means.ctypes.data, sing.ctypes.data, tv.ctypes.data,
                                                 _ref(my), C.byref(path)))
            self.kernel_path = int(path.value)
            if not (self.centering and rows == 0):
                self._store(comp, means, sing, tv, rows)
            return y

    def transform(self, x):
        """src/pca.rs:444-449; sparse input (a CsrMatrix or an object with .data / .indices / .indptr / .shape) goes through the sparse product."""
        if not _is_sparse(x):
            return super().transform(x)
        with self._sparse(x) as sx:
            ctx = self._ctx()
            d = self._means.shape[0]
            if sx.shape[1] != d:
                raise InvalidInput(f"# of columns should be {d}")
            keep = []
            y = np.empty((sx.shape[0], self._k), dtype=_np_dtype(sx._dt))
            my = describe(y, keep)
            comp, mu = _host(self._components, sx._dt), _host(self._means, sx._dt)
            path = C.c_int64(0)
            ctx.check(ctx.lib.petal_transform_csr(ctx._h, sx._handle(), comp.ctypes.data, mu.ctypes.data, self._k, d, int(self.centering),
                                                  C.byref(my), C.byref(path)))
            self.kernel_path = int(path.value)
            return y

    def _inner_fit(self, x, want_y: bool, omega=None):
        if _is_sparse(x):
            return self._inner_fit_sparse(x, want_y, omega)
        keep = []
        mx = describe(x, keep)
        ctx = self._ctx()
        npdt = _np_dtype(mx.dtype)
        if omega is None:
            omega = self.draw_omega(mx.cols, mx.dtype)
        omega = _host(omega, mx.dtype, (mx.cols, self._k + self.n_oversample))
        comp = np.empty((self._k, mx.cols), dtype=npdt)   # (every element is written by a successful fit; a failed one raises)
        means = np.zeros(mx.cols, dtype=npdt)            # (an empty input without centering returns before the means are written)
        sing = np.empty(self._k, dtype=npdt)
        tv = np.zeros(1, dtype=npdt)
        y, my = _out_like(x, mx.rows, self._k, mx.dtype, keep) if want_y else (None, None)
        ctx.check(ctx.lib.petal_rpca_fit(ctx._h, C.byref(mx), self._k, self.n_oversample, self.n_iter,
                                         int(self.centering), omega.ctypes.data, comp.ctypes.data, means.ctypes.data,
                                         sing.ctypes.data, tv.ctypes.data, _ref(my)))
        if not (self.centering and mx.rows == 0 and ctx.world_size == 1):
            self._store(comp, means, sing, tv, mx.rows)
        return y

    def fit(self, x, omega=None):
        self._inner_fit(x, False, omega)
        return self

    def fit_transform(self, x, omega=None):
        return self._inner_fit(x, True, omega)


class RandomizedPcaBuilder:
    """``RandomizedPcaBuilder<R>`` (src/pca.rs:564-663)."""

    def __init__(self, n_components: int, rng=None):
        self._k, self._rng, self._centering, self._ctx = n_components, rng, True, None
        self._n_iter, self._n_oversample = None, None

    @classmethod
    def new(cls, n_components: int):
        return cls(n_components)

    @classmethod
    def with_rng(cls, rng, n_components: int):
        return cls(n_components, rng)

    def seed(self, seed: int):
        """``Pcg::from_seed(seed.to_be_bytes())`` like the crate's builders (src/pca.rs:599-602, src/ica.rs:274-277)."""
        self._rng = Pcg.from_seed_be_bytes(seed)
        return self

    def centering(self, centering: bool):
        self._centering = centering
        return self

    def context(self, ctx: Context):
        self._ctx = ctx
        return self

    def n_iter(self, n_iter: int):  # extension: the crate hard-codes 7
        self._n_iter = n_iter
        return self

    def n_oversample(self, n: int):  # extension: the crate hard-codes 10
        self._n_oversample = n
        return self

    def build(self) -> RandomizedPca:
        return RandomizedPca(self._k, self._centering, self._rng, self._ctx, self._n_oversample, self._n_iter)


class FastIca(_CtxUser):
    """``FastIca<A, R>`` (src/ica.rs:41-221)."""

    TOL, MAX_ITER = 1e-4, 200  # src/ica.rs:216

    def __init__(self, rng=None, ctx=None, n_components: int = 0, mode: int = ICA_TEXTBOOK, tol=None, max_iter=None,
                 fun: str = "logcosh"):
        self.rng = rng if rng is not None else np.random.default_rng()
        self.ctx = ctx
        self.n_components = int(n_components)  # extension: the crate always uses min(n, d) (src/ica.rs:173)
        self.mode = mode
        # extension: "logcosh" (the crate's, src/ica.rs:383-398), "exp" or "cube".  `mode` is meant to carry the semantics; contrast bits
        # in it are passed on as they are with the default fun, and refused beside any other fun (_mode_word)
        self.fun = fun
        _ica_contrast(fun)
        self.tol = self.TOL if tol is None else tol
        self.max_iter = self.MAX_ITER if max_iter is None else max_iter
        self.components = np.zeros((0, 0))
        self.means = np.zeros(0)
        self.n_iter = 0

    @classmethod
    def new(cls, ctx=None):
        return cls(ctx=ctx)

    @classmethod
    def with_seed(cls, seed: int, ctx=None):
        """``Pcg::from_seed(seed.to_be_bytes())`` (src/ica.rs:75-78)."""
        return cls(Pcg.from_seed_be_bytes(seed), ctx)

    def to_json(self) -> str:
        """The JSON ``serde_json::to_string(&ica)`` writes for the reference struct (src/ica.rs:41-50, 428)."""
        import json
        return json.dumps({"rng": _rng_to_serde(self.rng), "components": _nd_to_serde(self.components),
                           "means": _nd_to_serde(self.means), "n_iter": int(self.n_iter)})

    @classmethod
    def from_json(cls, text: str, dtype=np.float64, ctx=None):
        """``serde_json::from_str::<FastIca<A>>``."""
        import json
        obj = json.loads(text)
        m = cls(Pcg.from_serde(obj["rng"]), ctx)
        m.components = _nd_from_serde(obj["components"], dtype)
        m.means = _nd_from_serde(obj["means"], dtype)
        m.n_iter = int(obj["n_iter"])
        return m

    @classmethod
    def with_rng(cls, rng, ctx=None):
        return cls(rng, ctx)

    def _mode_word(self) -> int:
        """the ABI's `mode`: the semantics with the contrast of `fun` in bits 4-7"""
        mode, g = int(self.mode), _ica_contrast(self.fun)
        if g != ICA_CONTRAST_LOGCOSH and mode >= 0 and mode & ICA_CONTRAST_MASK:
            raise InvalidInput(f"FastICA: mode = {mode} already carries a contrast function; give it either there or as fun = {self.fun!r}")
        return mode | g

    def _inner_fit(self, x, want_y: bool, w_init=None):
        keep = []
        mx = describe(x, keep)
        ctx = self._ctx()
        word = self._mode_word()
        npdt = _np_dtype(mx.dtype)
        if mx.rows == 0 and ctx.world_size == 1:  # src/ica.rs:174-176
            return _alloc_like(x, 0, mx.cols, mx.dtype) if want_y else None
        nc = self.n_components or min(mx.rows if ctx.world_size == 1 else 1 << 62, mx.cols)
        if w_init is None:
            w_init = self.rng.standard_normal((nc, nc))  # src/ica.rs:210-214
        w_init = _host(w_init, mx.dtype, (nc, nc))
        comp = np.zeros((nc, mx.cols), dtype=npdt)
        means = np.zeros(mx.cols, dtype=npdt)
        n_iter = C.c_int64(0)
        y, my = _out_like(x, mx.rows, nc, mx.dtype, keep) if want_y else (None, None)
        ctx.check(ctx.lib.petal_fastica_fit(ctx._h, C.byref(mx), self.n_components, float(self.tol),
                                            int(self.max_iter), word, w_init.ctypes.data, comp.ctypes.data,
                                            means.ctypes.data, C.byref(n_iter), _ref(my)))
        self.components, self.means, self.n_iter = comp, means, int(n_iter.value)
        return y

    def fit(self, x, w_init=None):
        self._inner_fit(x, False, w_init)
        return self

    def fit_transform(self, x, w_init=None):
        return self._inner_fit(x, True, w_init)

    def transform(self, x):
        """src/ica.rs:120-131 (always centres)."""
        keep = []
        mx = describe(x, keep)
        ctx = self._ctx()
        d = self.means.shape[0]
        if mx.cols != d:
            raise InvalidInput("too many columns")  # src/ica.rs:124-128
        nc = self.components.shape[0]
        y, my = _out_like(x, mx.rows, nc, mx.dtype, keep)
        comp = _host(self.components, mx.dtype)
        mu = _host(self.means, mx.dtype)
        ctx.check(ctx.lib.petal_transform(ctx._h, C.byref(mx), comp.ctypes.data, mu.ctypes.data, nc, d, 1, C.byref(my)))
        return y


class FastIcaBuilder:
    """``FastIcaBuilder<R>`` (src/ica.rs:244-308)."""

    def __init__(self, rng=None):
        self._rng, self._ctx, self._nc, self._mode, self._fun = rng, None, 0, ICA_TEXTBOOK, "logcosh"

    @classmethod
    def new(cls):
        return cls()

    @classmethod
    def with_rng(cls, rng):
        return cls(rng)

    def seed(self, seed: int):
        """``Pcg::from_seed(seed.to_be_bytes())`` like the crate's builders (src/pca.rs:599-602, src/ica.rs:274-277)."""
        self._rng = Pcg.from_seed_be_bytes(seed)
        return self

    def context(self, ctx: Context):
        self._ctx = ctx
        return self

    def n_components(self, nc: int):
        self._nc = nc
        return self

    def mode(self, mode: int):
        self._mode = mode
        return self

    def fun(self, name: str):
        """The contrast function: "logcosh" (the crate's), "exp" or "cube" (extensions)."""
        _ica_contrast(name)
        self._fun = name
        return self

    def build(self) -> FastIca:
        return FastIca(self._rng, self._ctx, self._nc, self._mode, fun=self._fun)


# ---- crate-private kernels that carry known-answer tests -------------------------------------------
def ica_par(x1, tol, max_iter, w_init, mode=ICA_TEXTBOOK, ctx: Optional[Context] = None):
    """``ica_par`` (src/ica.rs:319-361): x1 is nc x n.  Returns (W, n_iter).  mode: ICA_TEXTBOOK or ICA_REFERENCE_LITERAL, OR-ed
    with an ICA_CONTRAST_* (default: logcosh)."""
    ctx = ctx or default_context()
    keep = []
    mx = describe(x1, keep)
    w0 = _host(w_init, mx.dtype, (mx.rows, mx.rows))
    w = np.zeros_like(w0)
    n_iter = C.c_int64(0)
    ctx.check(ctx.lib.petal_ica_par(ctx._h, C.byref(mx), float(tol), int(max_iter), int(mode), w0.ctypes.data,
                                    w.ctypes.data, C.byref(n_iter)))
    return w, int(n_iter.value)


def symmetric_decorrelation(w, mode=ICA_TEXTBOOK, ctx: Optional[Context] = None):
    """``symmetric_decorrelation`` (src/ica.rs:363-381)."""
    ctx = ctx or default_context()
    w = np.ascontiguousarray(np.asarray(w))
    if w.dtype not in (np.float32, np.float64):
        w = w.astype(np.float64)
    dt = PETAL_F32 if w.dtype == np.float32 else PETAL_F64
    out = np.zeros_like(w)
    ctx.check(ctx.lib.petal_symmetric_decorrelation(ctx._h, w.ctypes.data, w.shape[0], dt, int(mode), out.ctypes.data))
    return out


def logcosh(x, ctx: Optional[Context] = None):
    """``logcosh`` (src/ica.rs:383-398): returns (tanh(x), mean_j(1 - tanh(x)_ij^2))."""
    ctx = ctx or default_context()
    keep = []
    mx = describe(x, keep)
    g, mg = _out_like(x, mx.rows, mx.cols, mx.dtype, keep)
    gp = np.zeros(mx.rows, dtype=_np_dtype(mx.dtype))
    ctx.check(ctx.lib.petal_logcosh(ctx._h, C.byref(mx), C.byref(mg), gp.ctypes.data))
    return g, gp


def svd_flip(u, vt, ctx: Optional[Context] = None):
    """``svd_flip`` (src/pca.rs:815-850): in place on u (n x m) and vt (m' x d)."""
    ctx = ctx or default_context()
    keep = []
    mu, mv = describe(u, keep), describe(vt, keep)
    ctx.check(ctx.lib.petal_svd_flip(ctx._h, C.byref(mu), C.byref(mv)))
    return u, vt


def gemm_xp(x, p, mu=None, bias=None, ctx: Optional[Context] = None):
    """z = (x - mu) . p + bias -- the K1 power-iteration GEMM kernel on its own (src/pca.rs:707, 714)."""
    ctx = ctx or default_context()
    keep = []
    mx = describe(x, keep)
    ph = _host(p, mx.dtype)
    if ph.shape[0] != mx.cols:
        raise InvalidInput(f"p should have {mx.cols} rows")
    N = ph.shape[1]
    muh = _host(mu, mx.dtype, (mx.cols,)) if mu is not None else None
    bh = _host(bias, mx.dtype, (N,)) if bias is not None else None
    z = _alloc_like(x, mx.rows, N, mx.dtype)
    mz = describe(z, keep)
    ctx.check(ctx.lib.petal_gemm_xp(ctx._h, C.byref(mx), muh.ctypes.data if muh is not None else None, ph.ctypes.data, N,
                                    bh.ctypes.data if bh is not None else None, C.byref(mz)))
    return z


def score_rows(x, components, means, weights=None, centering=True, want_y=False, ctx: Optional[Context] = None):
    """(scores, y): scores[:, 0] = max(|xc|^2 - sum_j y_j^2, 0) and scores[:, 1] = sum_j weights_j y_j^2 per row, with xc = x - means
    (when centering) and y = xc . components^T (k x d components) -- one pass over x (petal_score_rows, include/petal_hip_score.h);
    y = the projections as transform writes them if wanted, else None.  weights=None means all ones."""
    ctx = ctx or default_context()
    keep = []
    mx = describe(x, keep)
    comp = _host(components, mx.dtype)
    if comp.ndim != 2:
        raise InvalidInput("components should be a k x d matrix")
    k, d = comp.shape
    mu = _host(means, mx.dtype, (d,)) if means is not None else np.zeros(d, dtype=_np_dtype(mx.dtype))
    wh = _host(weights, mx.dtype, (k,)) if weights is not None else None
    out, mo = _out_like(x, mx.rows, 2, mx.dtype, keep)
    y, my = _out_like(x, mx.rows, k, mx.dtype, keep) if want_y else (None, None)
    ctx.check(ctx.lib.petal_score_rows(ctx._h, C.byref(mx), comp.ctypes.data, mu.ctypes.data, k, d, int(bool(centering)),
                                       wh.ctypes.data if wh is not None else None, C.byref(mo), _ref(my)))
    return out, y


def power_pass(x, p, mu=None, want_z=False, ctx: Optional[Context] = None):
    """(y, z, fused): y (fp64, host) = (x - mu)^T ((x - mu) p) -- one power iteration of the range finder as ONE pass over x
    (src/pca.rs:711 + 714) where the fused kernel exists (fused = True), the two GEMM kernels otherwise; z = (x - mu) p if wanted."""
    ctx = ctx or default_context()
    keep = []
    mx = describe(x, keep)
    ph = _host(p, mx.dtype)
    if ph.shape[0] != mx.cols:
        raise InvalidInput(f"p should have {mx.cols} rows")
    N = ph.shape[1]
    muh = _host(mu, mx.dtype, (mx.cols,)) if mu is not None else None
    y = np.zeros((mx.cols, N), dtype=np.float64)
    z, mz = _out_like(x, mx.rows, N, mx.dtype, keep) if want_z else (None, None)
    fused = C.c_int(0)
    ctx.check(ctx.lib.petal_power_pass(ctx._h, C.byref(mx), muh.ctypes.data if muh is not None else None, ph.ctypes.data, N,
                                       _dp(y), _ref(mz), C.byref(fused)))
    return y, z, bool(fused.value)


def gemm_atb(a, b=None, mu_a=None, mu_b=None, ctx: Optional[Context] = None):
    """c (fp64, host) = (a - mu_a)^T . (b - mu_b) -- the K2 power-iteration GEMM kernel on its own
    (src/pca.rs:711, 681); b=None means b = a."""
    ctx = ctx or default_context()
    keep = []
    ma = describe(a, keep)
    mb = describe(b, keep) if b is not None else None
    M, N = ma.cols, (mb.cols if mb is not None else ma.cols)
    mah = _host(mu_a, ma.dtype, (M,)) if mu_a is not None else None
    mbh = _host(mu_b, ma.dtype, (N,)) if mu_b is not None else None
    out = np.zeros((M, N), dtype=np.float64)
    ctx.check(ctx.lib.petal_gemm_atb(ctx._h, C.byref(ma), mah.ctypes.data if mah is not None else None,
                                     C.byref(mb) if mb is not None else None,
                                     mbh.ctypes.data if mbh is not None else None,
                                     out.ctypes.data_as(C.POINTER(C.c_double))))
    return out


# ---- include/petal_hip_probe.h: thin numpy wrappers (test aids) ---------------------------------------------------------------------
def _f64_2d(a):
    """a 2-D float64 array with unit column stride as it is (a row-sliced view keeps its leading dimension), else a contiguous copy"""
    a = np.asarray(a, dtype=np.float64)
    if a.ndim != 2:
        raise InvalidInput("expected a 2-D array")
    if a.shape[1] > 1 and a.strides[1] != 8 or a.strides[0] % 8 or a.strides[0] < 8 * a.shape[1]:
        a = np.ascontiguousarray(a)
    return a, (a.strides[0] // 8 if a.shape[0] > 1 else max(a.shape[1], 1))


def probe_chol(g, rel_tol, Lz=0, ndead_cols=0, route=0, b=None, ndead_in=0, ctx: Optional[Context] = None):
    """(out, ndead, rt) of petal_probe_chol: route 0 out = T (Lz x Lz); 1 out = b R^-1 (b: rows x Lz, None = identity); 2 out = R^-1 b"""
    ctx = ctx or default_context()
    g, ldg = _f64_2d(g)
    L = g.shape[0]
    lz = Lz or L
    bb, ldb, br, bc = None, 0, 0, 0
    if b is not None:
        bb, ldb = _f64_2d(b)
        br, bc = bb.shape
    shape = (lz, lz) if route == 0 else ((br if bb is not None else lz, lz) if route == 1 else (lz, bc))
    out = np.full(shape, np.nan)
    nd, rt = C.c_int(int(ndead_in)), C.c_int(-1)
    ctx.check(ctx.lib.petal_probe_chol(ctx._h, _dp(g), L, ldg, float(rel_tol), int(Lz), int(ndead_cols), int(route),
                                       _dp(bb), br, bc, ldb, _dp(out), shape[1], C.byref(nd), C.byref(rt)))
    return out, nd.value, rt.value


def probe_eigh(a, tol_rel=1e-15, clustered=False, Lz=0, ncheck=0, verdict_mode=0, verdict_in=0, gap_tol_override=0.0,
               ctx: Optional[Context] = None):
    """(w, V, verdict) of petal_probe_eigh; V is max(L, Lz) square"""
    ctx = ctx or default_context()
    a, lda = _f64_2d(a)
    L = a.shape[0]
    lm = max(L, int(Lz))
    w, v = np.full(L, np.nan), np.full((lm, lm), np.nan)
    vo = C.c_int(-2)
    ctx.check(ctx.lib.petal_probe_eigh(ctx._h, _dp(a), L, lda, float(tol_rel), int(bool(clustered)), int(Lz), int(ncheck), int(verdict_mode),
                                       int(verdict_in), float(gap_tol_override), _dp(w), _dp(v), lm, C.byref(vo)))
    return w, v, vo.value


def probe_ritz_residual(cv, vr, nc, theta, flag=None, flag2=None, w_len=None, ctx: Optional[Context] = None):
    """(out3, w_out) of petal_probe_ritz_residual: cv, vr (rows x leading dimension, the first nc columns count), theta (nc values);
    flag / flag2: None = no such word, else its starting value; w_out has w_len (default nc + 8) words, NaN where nothing was written"""
    ctx = ctx or default_context()
    cv, vr = np.ascontiguousarray(cv, dtype=np.float64), np.ascontiguousarray(vr, dtype=np.float64)
    if cv.ndim != 2 or vr.ndim != 2 or cv.shape[0] != vr.shape[0]:
        raise InvalidInput("cv and vr should be 2-D arrays with the same number of rows")
    th = np.ascontiguousarray(theta, dtype=np.float64).reshape(-1)
    if th.size < nc:
        raise InvalidInput(f"theta should hold {nc} values")
    w_len = int(nc + 8 if w_len is None else w_len)
    out3, w_out = np.full(3, np.nan), np.full(max(w_len, 1), np.nan)
    f1 = C.c_int(int(flag)) if flag is not None else None
    f2 = C.c_int(int(flag2)) if flag2 is not None else None
    ctx.check(ctx.lib.petal_probe_ritz_residual(ctx._h, _dp(cv), cv.shape[1], _dp(vr), vr.shape[1], cv.shape[0], int(nc),
                                                _dp(th) if nc > 0 else None, _ref(f1), _ref(f2), _dp(out3), _dp(w_out), w_len))
    return out3, w_out


def probe_topk_eigh(c, nc, dtype=PETAL_F64, mode=0, ctx: Optional[Context] = None):
    """petal_probe_topk_eigh on c (d x d float64).  Returns a dict: delivered, w, v, and by mode 0: checks; 1: r3, verdict; 2: diag
    (w: dp values, v: dp x dp; modes 0 / 1: nc values, dp x nc)"""
    ctx = ctx or default_context()
    c, ldc = _f64_2d(c)
    d = c.shape[0]
    dp = (d + 15) // 16 * 16
    cols = dp if mode == 2 else int(nc)
    w, v = np.full(max(cols, 1), np.nan), np.full((dp, max(cols, 1)), np.nan)
    r3, diag = np.full(3, np.nan), np.full(dp, np.nan)
    delivered, checks, verdict = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    ctx.check(ctx.lib.petal_probe_topk_eigh(ctx._h, _dp(c), d, ldc, int(nc), int(dtype), int(mode), C.byref(delivered), _dp(w), _dp(v),
                                            max(cols, 1), C.byref(checks), _dp(r3), C.byref(verdict), _dp(diag)))
    out = {"delivered": delivered.value, "w": w[:cols], "v": v[:, :cols]}
    if mode == 0:
        out["checks"] = checks.value
    elif mode == 1:
        out["r3"], out["verdict"] = r3, verdict.value
    else:
        out["diag"] = diag
    return out


def probe_jacobi_svd_rows(a, ctx: Optional[Context] = None):
    """(U, s_inv, nonconv) of petal_probe_jacobi_svd_rows"""
    ctx = ctx or default_context()
    a, lda = _f64_2d(a)
    L = a.shape[0]
    u, s = np.full((L, L), np.nan), np.full(L, np.nan)
    nc = C.c_int(-1)
    ctx.check(ctx.lib.petal_probe_jacobi_svd_rows(ctx._h, _dp(a), L, lda, _dp(u), L, _dp(s), C.byref(nc)))
    return u, s, nc.value


def probe_dgemm(ta, tb, M, N, K, alpha, a, b, beta, c, colscale=None, ctx: Optional[Context] = None):
    """petal_probe_dgemm in place on c (float64, unit column stride; a row-sliced view keeps its leading dimension); b is a: one buffer"""
    ctx = ctx or default_context()
    aa, lda = _f64_2d(a)
    bb, ldb = (aa, lda) if b is a else _f64_2d(b)
    if not (isinstance(c, np.ndarray) and c.dtype == np.float64 and c.ndim == 2 and c.shape == (M, N) and (N == 1 or c.strides[1] == 8)):
        raise InvalidInput("c should be an M x N float64 array with unit column stride")
    ldc = c.strides[0] // 8 if M > 1 else N
    cs = np.ascontiguousarray(colscale, dtype=np.float64) if colscale is not None else None
    ctx.check(ctx.lib.petal_probe_dgemm(ctx._h, int(bool(ta)), int(bool(tb)), M, N, K, float(alpha), _dp(aa), lda, _dp(bb), ldb, float(beta),
                                        _dp(c), ldc, _dp(cs)))
    return c


def _data_2d(x):
    """a 2-D float32 / float64 host array with unit column stride as it is (a row-sliced view keeps its leading dimension)"""
    x = np.asarray(x)
    if x.ndim != 2 or x.dtype not in (np.float32, np.float64):
        raise InvalidInput("expected a 2-D float32 / float64 array")
    es = x.dtype.itemsize
    if x.shape[1] > 1 and x.strides[1] != es or x.strides[0] % es or x.strides[0] < es * x.shape[1]:
        x = np.ascontiguousarray(x)
    return x, (x.strides[0] // es if x.shape[0] > 1 else max(x.shape[1], 1)), (PETAL_F32 if x.dtype == np.float32 else PETAL_F64)


def probe_power_pass_means(x, p, L, d=None, ctx: Optional[Context] = None):
    """petal_probe_power_pass_means: x (n x K, K a multiple of 16; columns d .. K - 1 zero), p (K x N float64).  Returns a dict:
    done, y (K x N), mu64, muT, mu0 (K each, float64; muT and mu0 hold values of x's dtype), tv."""
    ctx = ctx or default_context()
    x, ldx, dt = _data_2d(x)
    pp, ldp = _f64_2d(p)
    n, K = x.shape
    N = pp.shape[1]
    if pp.shape[0] != K:
        raise InvalidInput(f"p should have {K} rows")
    y = np.full((K, N), np.nan)
    mu64, muT, mu0, tv = np.full(K, np.nan), np.full(K, np.nan), np.full(K, np.nan), np.full(1, np.nan)
    done = C.c_int(-1)
    ctx.check(ctx.lib.petal_probe_power_pass_means(ctx._h, x.ctypes.data, dt, n, K, int(K if d is None else d), ldx, _dp(pp), N, ldp, int(L),
                                                   C.byref(done), _dp(y), N, _dp(mu64), _dp(muT), _dp(mu0), _dp(tv)))
    return {"done": done.value, "y": y, "mu64": mu64, "muT": muT, "mu0": mu0, "tv": float(tv[0])}


def probe_rebase(x, mu, g, a, rel_tol=1e-15, p_planes=2, steering=False, route=0, ndead_in=0, ctx: Optional[Context] = None):
    """petal_probe_rebase: x (n x K), mu (K, or None), g (L x L float64), a (K x M float64).  Returns a dict: done, p_out (K x M),
    z (n x M float64, None on route 1), y (K x M, None on route 0), ndead."""
    ctx = ctx or default_context()
    x, ldx, dt = _data_2d(x)
    gg, ldg = _f64_2d(g)
    aa, lda = _f64_2d(a)
    n, K = x.shape
    L, M = gg.shape[0], aa.shape[1]
    if aa.shape[0] != K:
        raise InvalidInput(f"a should have {K} rows")
    muh = _host(mu, dt, (K,)) if mu is not None else None
    p_out = np.full((K, M), np.nan)
    z = np.full((n, M), np.nan) if route != 1 else None
    y = np.full((K, M), np.nan) if route != 0 else None
    done, nd = C.c_int(-1), C.c_int(int(ndead_in))
    ctx.check(ctx.lib.petal_probe_rebase(ctx._h, x.ctypes.data, dt, n, K, ldx, muh.ctypes.data if muh is not None else None, _dp(gg), L, ldg,
                                         float(rel_tol), _dp(aa), M, lda, int(p_planes), int(bool(steering)), int(route), C.byref(done),
                                         _dp(p_out), M, _dp(z), M, _dp(y), M,
                                         C.byref(nd)))
    return {"done": done.value, "p_out": p_out, "z": z, "y": y, "ndead": nd.value}

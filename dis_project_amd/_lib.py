"""ctypes binding of ``liblfm.so`` (the C-ABI declared in ``include/lfm.h``).

This module is the only place that touches the shared library. There is no CPU
fallback: if ``liblfm.so`` is missing, or no HIP device is visible when a context is
requested, the calls raise :class:`LfmError` — loudly, by design.

HIP runtime note: ``liblfm.so`` needs ``libamdhip64.so.7``. When PyTorch is imported
*before* this module, the dynamic loader binds that name to the copy PyTorch already
loaded (same SONAME), so one process never holds two HIP runtimes. Processes that
use both must therefore import torch first (``bench.py`` does).
"""

from __future__ import annotations

import ctypes
import os
import threading
from ctypes import (POINTER, c_char, c_char_p, c_double, c_int, c_int64, c_size_t, c_uint64,
                    c_void_p)

import numpy as np

LIB_NAME = "liblfm.so"
LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), LIB_NAME)
# diagnostics (include/lfm_diag.h): a library of their own, linked against liblfm.so
DIAG_NAME = "liblfm_diag.so"
DIAG_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), DIAG_NAME)

LFM_OK = 0
LFM_E_ARG = 1
LFM_E_HIP = 2
LFM_E_NOT_PD = 3
LFM_E_OOM = 4
LFM_E_RCCL = 5
LFM_E_STATE = 6
LFM_E_TIMEOUT = 7
ABI_VERSION = 5

LFM_UPLO_FULL = 0
LFM_UPLO_LOWER = 1

_ERR_NAMES = {
    LFM_E_ARG: "LFM_E_ARG",
    LFM_E_HIP: "LFM_E_HIP",
    LFM_E_NOT_PD: "LFM_E_NOT_PD",
    LFM_E_OOM: "LFM_E_OOM",
    LFM_E_RCCL: "LFM_E_RCCL",
    LFM_E_STATE: "LFM_E_STATE",
    LFM_E_TIMEOUT: "LFM_E_TIMEOUT",
}

# double* arguments and struct fields as untyped pointers: ctypes then takes the array's address
# as a plain int (numpy's .ctypes.data, ~1 us) where POINTER(c_double) needed a data_as cast
# (~2.3 us each; a C5 step of 15 problems paid ~0.1 ms for them). byref() and pointer objects
# are accepted as before.
_dptr = c_void_p


class LfmError(RuntimeError):
    """A non-OK status from liblfm (code + the library's own message)."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"{_ERR_NAMES.get(code, code)}: {msg}")
        self.code = code


class LfmHyp(ctypes.Structure):
    _fields_ = [
        ("num_genes", c_int64),
        ("true_d", _dptr),
        ("true_s", _dptr),
        ("true_b", _dptr),
        ("l", c_double),
        ("obs_stddev", c_double),
        ("jitter", c_double),
    ]


class LfmProblem(ctypes.Structure):
    _fields_ = [("x", _dptr), ("y", _dptr), ("n", c_int64), ("hyp", LfmHyp)]


class LfmAdam(ctypes.Structure):
    """lfm_adam (include/lfm.h): optax.adam and JaxTrainer.fit's epoch handling."""
    _fields_ = [
        ("learning_rate", c_double),
        ("b1", c_double),
        ("b2", c_double),
        ("eps", c_double),
        ("eps_root", c_double),
        ("num_steps_per_epoch", c_int64),
        ("fix_params", c_int),
    ]


class LfmKstat(ctypes.Structure):
    _fields_ = [
        ("name", c_char * 32),
        ("launches", c_int64),
        ("total_ms", c_double),
        ("flops", c_double),
        ("bytes", c_double),
        ("issued_flops", c_double),
    ]


# (name, restype, argtypes) — every entry point of include/lfm.h
_c_ctx = c_void_p
PRODUCT_SIGNATURES = [
    ("lfm_abi_version", c_int, []),
    ("lfm_device_count", c_int, [POINTER(c_int)]),
    ("lfm_ctx_create", c_int, [c_int, POINTER(c_void_p)]),
    ("lfm_ctx_destroy", None, [_c_ctx]),
    ("lfm_last_error", c_char_p, [_c_ctx]),
    ("lfm_ctx_synchronize", c_int, [_c_ctx]),
    ("lfm_ctx_set_block", c_int, [_c_ctx, c_int]),
    ("lfm_ctx_set_schedule", c_int, [_c_ctx, c_int]),
    ("lfm_ctx_get_schedule", c_int, [_c_ctx, POINTER(c_int)]),
    ("lfm_ctx_fallbacks", c_int, [_c_ctx, POINTER(c_int64)]),
    ("lfm_mean_function_f64", c_int, [_c_ctx, _dptr, c_int64, POINTER(LfmHyp), _dptr]),
    ("lfm_cross_covariance_f64", c_int,
     [_c_ctx, _dptr, c_int64, _dptr, c_int64, POINTER(LfmHyp), _dptr, c_int64]),
    ("lfm_gram_f64", c_int,
     [_c_ctx, _dptr, c_int64, POINTER(LfmHyp), c_double, c_int, _dptr, c_int64]),
    ("lfm_gram_f32", c_int,
     [_c_ctx, _dptr, c_int64, POINTER(LfmHyp), c_double, c_int, POINTER(ctypes.c_float), c_int64]),
    ("lfm_mll_f64", c_int, [_c_ctx, _dptr, _dptr, c_int64, POINTER(LfmHyp), c_int, _dptr]),
    ("lfm_mll_grad_f64", c_int,
     [_c_ctx, _dptr, _dptr, c_int64, POINTER(LfmHyp), c_int, _dptr, _dptr]),
    ("lfm_loocv_f64", c_int,
     [_c_ctx, _dptr, _dptr, c_int64, POINTER(LfmHyp), c_int, _dptr, _dptr, _dptr]),
    ("lfm_loocv_grad_f64", c_int,
     [_c_ctx, _dptr, _dptr, c_int64, POINTER(LfmHyp), c_int, _dptr, _dptr]),
    ("lfm_posterior_f64", c_int,
     [_c_ctx, _dptr, _dptr, c_int64, _dptr, c_double, _dptr, c_int64, POINTER(LfmHyp), _dptr,
      _dptr]),
    ("lfm_mll_batch_f64", c_int,
     [_c_ctx, c_int64, POINTER(LfmProblem), c_int, _dptr, POINTER(c_int)]),
    ("lfm_batch_create", c_int, [_c_ctx, c_int64, POINTER(LfmProblem), POINTER(c_void_p)]),
    ("lfm_batch_destroy", c_int, [c_void_p]),
    ("lfm_batch_hyp_size", c_int, [c_void_p, POINTER(c_int64)]),
    ("lfm_batch_mll_f64", c_int, [_c_ctx, c_void_p, _dptr, c_int, _dptr, _dptr]),
    ("lfm_batch_mll_grad_f64", c_int, [_c_ctx, c_void_p, _dptr, c_int, _dptr, _dptr, _dptr]),
    ("lfm_batch_fit_f64", c_int,
     [_c_ctx, c_void_p, POINTER(LfmAdam), c_int, c_int64, c_int64, _dptr, _dptr, _dptr, _dptr,
      _dptr]),
    ("lfm_batch_posterior_f64", c_int,
     [_c_ctx, c_void_p, _dptr, _dptr, _dptr, _dptr, _dptr, _dptr, _dptr, _dptr, _dptr]),
    ("lfm_mbatch_create", c_int, [_c_ctx, c_int64, POINTER(LfmProblem), POINTER(c_void_p)]),
    ("lfm_mbatch_destroy", c_int, [c_void_p]),
    ("lfm_mbatch_hyp_size", c_int, [c_void_p, POINTER(c_int64)]),
    ("lfm_mbatch_mll_f64", c_int, [_c_ctx, c_void_p, _dptr, c_int, _dptr, _dptr]),
    ("lfm_mbatch_mll_grad_f64", c_int, [_c_ctx, c_void_p, _dptr, c_int, _dptr, _dptr, _dptr]),
    ("lfm_mbatch_posterior_f64", c_int,
     [_c_ctx, c_void_p, _dptr, _dptr, _dptr, _dptr, _dptr, _dptr, _dptr, _dptr, _dptr]),
    ("lfm_mbatch_predictive_f64", c_int,
     [_c_ctx, c_void_p, _dptr, _dptr, _dptr, _dptr, _dptr, _dptr, _dptr, _dptr, _dptr, c_int64,
      c_int64, _dptr, _dptr, _dptr]),
    ("lfm_mbatch_fit_f64", c_int,
     [_c_ctx, c_void_p, POINTER(LfmAdam), c_int, c_int64, c_int64, _dptr, _dptr, _dptr, _dptr,
      _dptr]),
    ("lfm_post_create", c_int,
     [_c_ctx, _dptr, _dptr, c_int64, _dptr, c_double, POINTER(LfmHyp), POINTER(c_void_p)]),
    ("lfm_post_destroy", c_int, [c_void_p]),
    ("lfm_post_set_chunk", c_int, [c_void_p, c_int64]),
    ("lfm_post_predict_f64", c_int, [_c_ctx, c_void_p, _dptr, c_int64, _dptr, _dptr, _dptr]),
    ("lfm_log_prob_f64", c_int, [_c_ctx, _dptr, _dptr, c_int64, c_int64, _dptr, _dptr]),
    ("lfm_randn_f64", c_int, [_c_ctx, c_uint64, c_int64, c_int64, c_int64, _dptr]),
    ("lfm_mvn_sample_f64", c_int,
     [_c_ctx, _dptr, _dptr, c_int64, c_int64, c_uint64, c_int64, c_int64, _dptr]),
    ("lfm_post_sample_f64", c_int,
     [_c_ctx, c_void_p, _dptr, c_int64, c_double, c_uint64, c_int64, c_int64, _dptr, _dptr]),
    ("lfm_post_log_prob_f64", c_int,
     [_c_ctx, c_void_p, _dptr, c_int64, c_double, _dptr, c_int64, _dptr, _dptr]),
    ("lfm_h_f64", c_int,
     [_c_ctx, POINTER(LfmHyp), POINTER(c_int64), POINTER(c_int64), _dptr, _dptr, c_int64, _dptr]),
    ("lfm_dev_alloc", c_int, [_c_ctx, c_size_t, POINTER(c_void_p)]),
    ("lfm_dev_free", c_int, [_c_ctx, c_void_p]),
    ("lfm_memcpy_h2d", c_int, [_c_ctx, c_void_p, c_void_p, c_size_t]),
    ("lfm_memcpy_d2h", c_int, [_c_ctx, c_void_p, c_void_p, c_size_t]),
    ("lfm_memset_dev", c_int, [_c_ctx, c_void_p, c_int, c_size_t]),
    ("lfm_mll_f64_dev", c_int, [_c_ctx, c_void_p, c_void_p, c_int64, POINTER(LfmHyp), c_int, _dptr]),
    ("lfm_data_create", c_int, [_c_ctx, c_void_p, c_void_p, c_int64, POINTER(c_void_p)]),
    ("lfm_data_destroy", c_int, [c_void_p]),
    ("lfm_mll_f64_data", c_int, [_c_ctx, c_void_p, POINTER(LfmHyp), c_int, _dptr]),
    ("lfm_mll_multi_f64", c_int,
     [_c_ctx, c_void_p, c_int64, POINTER(LfmHyp), c_int, _dptr, _dptr]),
    ("lfm_gram_f64_dev", c_int,
     [_c_ctx, c_void_p, c_int64, POINTER(LfmHyp), c_double, c_int, c_void_p, c_int64]),
    ("lfm_gram_f32_dev", c_int,
     [_c_ctx, c_void_p, c_int64, POINTER(LfmHyp), c_double, c_int, c_void_p, c_int64]),
    ("lfm_profile_enable", c_int, [_c_ctx, c_int]),
    ("lfm_profile_classes", c_int, [_c_ctx, ctypes.c_uint]),
    ("lfm_profile_reset", c_int, [_c_ctx]),
    ("lfm_profile_read", c_int, [_c_ctx, POINTER(LfmKstat), c_int, POINTER(c_int)]),
    ("lfm_farm_unique_id", c_int, [_c_ctx, POINTER(ctypes.c_ubyte)]),
    ("lfm_farm_init", c_int, [_c_ctx, POINTER(ctypes.c_ubyte), c_int, c_int]),
    ("lfm_farm_allgather_f64", c_int, [_c_ctx, _dptr, c_int64, _dptr]),
    ("lfm_farm_batch_mll_f64", c_int, [_c_ctx, c_void_p, _dptr, c_int, c_int64, _dptr, _dptr]),
    ("lfm_farm_destroy", c_int, [_c_ctx]),
]

# include/lfm_diag.h (liblfm_diag.so): probes, phase stamps and the schedule-3 tenancy state
# (measurement / known-answer tests only)
DIAG_SIGNATURES = [
    ("lfm_debug_stamps", c_int, [_c_ctx, c_int, POINTER(ctypes.c_ulonglong), c_int]),
    ("lfm_debug_last_schedule", c_int, [_c_ctx, POINTER(c_int)]),
    ("lfm_debug_trace", c_int, [_c_ctx, ctypes.c_int64, POINTER(ctypes.c_ulonglong),
                                ctypes.c_int64, POINTER(ctypes.c_int64)]),
    ("lfm_debug_lock_path", c_int, [_c_ctx, ctypes.c_char_p, c_int]),
    ("lfm_probe_rsq", c_int, [_c_ctx, c_void_p, c_int64, c_void_p]),
    ("lfm_probe_kxx_tab", c_int, [_c_ctx, _dptr, c_int64, POINTER(LfmHyp), _dptr]),
    ("lfm_probe_grad_tables", c_int, [_c_ctx, POINTER(LfmHyp), c_int, c_double, _dptr, _dptr]),
    ("lfm_probe_mfma_f64_layout", c_int, [_c_ctx, _dptr, _dptr, _dptr]),
    ("lfm_probe_mfma4_layout", c_int, [_c_ctx, _dptr, _dptr, _dptr, _dptr]),
    ("lfm_probe_mfma_f64", c_int, [_c_ctx, c_int, c_int, _dptr, _dptr]),
    ("lfm_probe_mfma_f64_cycles", c_int, [_c_ctx, c_int, c_int, _dptr, _dptr]),
    ("lfm_probe_rate", c_int, [_c_ctx, c_int, c_int, c_int, _dptr]),
    ("lfm_probe_syrk", c_int, [_c_ctx, c_int, c_int, c_int, c_int, _dptr]),
]

# kernel classes in lfm_profile_read order (lfm_internal.h KClass)
KCLASSES = ["tables", "gram_grid", "gram_direct", "augment", "potrf", "trsm", "syrk",
            "finalize", "small_mll", "mean", "grad", "panel", "syrk_side", "small_grad",
            "small_post", "post_panel", "post_update", "mid_fill", "mid_column", "mid_inverse",
            "mid_pairs", "mid_finish"]
# ... and the joint samples' two (lfm_sample.hip), entries 22 and 23 of that order
SAMPLE_KCLASSES = ["sample_randn", "sample_trmm"]
# ... and the leave-one-out gradient's product (lfm_loo.hip), entry 24
LOO_KCLASSES = ["loo_product"]

_lib = None
_diag = None
_lib_lock = threading.Lock()


def load_library(path: str | None = None) -> ctypes.CDLL:
    """Load liblfm.so (once) and declare every C-ABI signature. Raises if absent."""
    global _lib
    with _lib_lock:
        if _lib is not None and path is None:
            return _lib
        p = path or os.environ.get("LFM_LIBRARY", LIB_PATH)
        if not os.path.exists(p):
            raise LfmError(
                LFM_E_STATE,
                f"{p} not found: build it first (python -c 'import __graft_entry__ as g; g.build()'"
                " or make -C dis_project_amd/csrc). There is no CPU fallback.",
            )
        lib = ctypes.CDLL(p)
        for name, res, args in PRODUCT_SIGNATURES:
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.lfm_abi_version() != ABI_VERSION:
            raise LfmError(LFM_E_STATE, "liblfm ABI version mismatch")
        if path is None:
            _lib = lib
        return lib


def load_diag() -> ctypes.CDLL:
    """Load liblfm_diag.so (after liblfm.so, whose contexts it takes) and declare the
    include/lfm_diag.h signatures. Measurement scripts and tests only."""
    global _diag
    load_library()
    with _lib_lock:
        if _diag is None:
            if not os.path.exists(DIAG_PATH):
                raise LfmError(LFM_E_STATE, f"{DIAG_PATH} not found: make -C dis_project_amd/csrc")
            lib = ctypes.CDLL(DIAG_PATH)
            for name, res, args in DIAG_SIGNATURES:
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            _diag = lib
        return _diag


def as_f64(a, shape=None) -> np.ndarray:
    arr = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    if shape is not None:
        arr = arr.reshape(shape)
    return arr


def dptr(a: np.ndarray):
    return a.ctypes.data


class HypArgs:
    """Keeps the numpy buffers behind an LfmHyp alive for the duration of a call."""

    def __init__(self, true_d, true_s, true_b, l, obs_stddev, jitter):
        self.d = as_f64(true_d).reshape(-1)
        self.s = as_f64(true_s).reshape(-1)
        self.b = as_f64(true_b).reshape(-1)
        if not (self.d.size == self.s.size == self.b.size) or self.d.size == 0:
            raise ValueError("true_d, true_s, true_b must be non-empty and of equal length")
        self.struct = LfmHyp(
            self.d.size, self.d.ctypes.data, self.s.ctypes.data, self.b.ctypes.data,
            float(l), float(obs_stddev), float(jitter),
        )
        # the struct holds plain addresses: it keeps this object (and so the arrays) alive, so
        # a struct or a byref of it passed on alone never outlives its buffers
        self.struct._owner = self

    @property
    def ref(self):
        """byref(struct): the CArgObject keeps the struct, which keeps this object and its
        arrays alive for as long as the reference is held (e.g. across a call)."""
        return ctypes.byref(self.struct)


class Context:
    """One liblfm context = one device + one HIP stream + a reusable workspace."""

    def __init__(self, device: int = 0):
        self.lib = load_library()
        h = c_void_p()
        rc = self.lib.lfm_ctx_create(int(device), ctypes.byref(h))
        if rc != LFM_OK:
            n = c_int(0)
            self.lib.lfm_device_count(ctypes.byref(n))
            raise LfmError(rc, f"lfm_ctx_create(device={device}) failed; visible HIP devices: "
                               f"{n.value}. liblfm needs an MI355X (gfx950); there is no CPU fallback.")
        self.handle = h
        self.device = int(device)
        self.farm_ranks = 1  # ranks of this context's farm communicator (farm.RcclGather)

    # -- error plumbing
    def check(self, rc: int, allow_not_pd: bool = False) -> int:
        """Raise LfmError unless rc is LFM_OK (or LFM_E_NOT_PD with allow_not_pd: JAX's NaN
        on a failed Cholesky). LFM_E_TIMEOUT always raises: a stalled device-side hand-off is
        not a property of the input and must never read as a NaN likelihood."""
        if rc == LFM_OK or (allow_not_pd and rc == LFM_E_NOT_PD):
            return rc
        msg = self.lib.lfm_last_error(self.handle)
        raise LfmError(rc, msg.decode() if msg else "")

    def close(self):
        if getattr(self, "handle", None):
            self.lib.lfm_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def diag(self) -> ctypes.CDLL:
        """liblfm_diag.so (include/lfm_diag.h), loaded on first use."""
        return load_diag()

    # -- factorisation schedule (include/lfm.h: lfm_ctx_set_schedule)
    @property
    def schedule(self) -> int:
        out = c_int(0)
        self.check(self.lib.lfm_ctx_get_schedule(self.handle, ctypes.byref(out)))
        return out.value

    @schedule.setter
    def schedule(self, value: int):
        self.check(self.lib.lfm_ctx_set_schedule(self.handle, int(value)))

    @property
    def fallbacks(self) -> int:
        """Schedule-3 calls of this context re-run on schedule 1 after a device-side wait ran
        out (include/lfm.h ``lfm_ctx_fallbacks``); their results are valid."""
        out = c_int64(0)
        self.check(self.lib.lfm_ctx_fallbacks(self.handle, ctypes.byref(out)))
        return out.value

    # -- profiling
    def profile(self, on: bool = True, classes=None):
        """Event-time kernel launches; `classes` (names from profile_read) limits which."""
        if classes is not None:
            mask = 0
            for c in classes:
                mask |= 1 << (KCLASSES + SAMPLE_KCLASSES + LOO_KCLASSES).index(c)
            self.check(self.lib.lfm_profile_classes(self.handle, mask))
        else:
            self.check(self.lib.lfm_profile_classes(self.handle, 0xFFFFFFFF))
        self.check(self.lib.lfm_profile_enable(self.handle, int(on)))

    def profile_reset(self):
        self.check(self.lib.lfm_profile_reset(self.handle))

    def profile_read(self) -> dict:
        arr = (LfmKstat * 32)()
        cnt = c_int(0)
        self.check(self.lib.lfm_profile_read(self.handle, arr, 32, ctypes.byref(cnt)))
        out = {}
        for i in range(min(cnt.value, 32)):
            s = arr[i]
            out[s.name.decode()] = dict(launches=s.launches, total_ms=s.total_ms,
                                        flops=s.flops, bytes=s.bytes,
                                        issued_flops=s.issued_flops)
        return out


# one context per (host thread, device): a context's workspace, pinned buffer and streams are
# not thread-safe (include/lfm.h), so threads never share one
_tls = threading.local()


def default_device() -> int:
    for var in ("LFM_DEVICE", "LOCAL_RANK"):
        v = os.environ.get(var)
        if v is not None and v != "":
            return int(v)
    return 0


def get_context(device: int | None = None) -> Context:
    """The calling thread's context on `device` (created on first use)."""
    dev = default_device() if device is None else int(device)
    cache = getattr(_tls, "contexts", None)
    if cache is None:
        cache = _tls.contexts = {}
    ctx = cache.get(dev)
    if ctx is None:
        ctx = Context(dev)
        cache[dev] = ctx
    return ctx


def device_count() -> int:
    lib = load_library()
    n = c_int(0)
    lib.lfm_device_count(ctypes.byref(n))
    return n.value

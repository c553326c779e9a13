"""CPU checks of the leave-one-out CV calls (lfm_loocv_f64, lfm_loocv_grad_f64,
objectives.CustomConjLOOCV): their plan under AddressSanitizer + UBSan (tests/native/
loo_plan_check.cpp, a stand-alone program built here with the flags of tests/native/Makefile and
run directly), the entry points in the header and the ctypes table, the argument checks that need
no GPU, and the strict build."""

import os
import re
import shutil
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("lfm_loocv_f64", "lfm_loocv_grad_f64")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan")
def test_plan_loo_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "loo_plan_check")
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *san, "-pthread",
                        os.path.join(ROOT, "tests", "native", "loo_plan_check.cpp"),
                        os.path.join(ROOT, "dis_project_amd", "csrc", "lfm_host.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "loo_plan_check: all passed" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_header_and_signatures_agree():
    import ctypes

    from dis_project_amd import _lib
    from tests.test_abi import header_functions

    declared = header_functions()
    bound = {name: (res, args) for name, res, args in _lib.PRODUCT_SIGNATURES}
    assert set(bound) == set(declared)
    with open(os.path.join(ROOT, "include", "lfm.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    params = {}
    for name in NAMES:
        assert name in declared and name in bound
        m = re.search(r"int\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, "the header declares it"
        params[name] = [" ".join(p.split()) for p in m.group(1).split(",")]
    head = ["lfm_ctx* ctx", "const double* x", "const double* y", "int64_t n", "const lfm_hyp* hyp",
            "int negative", "double* value"]
    assert params["lfm_loocv_f64"] == head + ["double* loo_mean", "double* loo_var"]
    assert params["lfm_loocv_grad_f64"] == head + ["double* grad"]
    dp = _lib._dptr  # how the table passes a host double*
    hyp = ctypes.POINTER(_lib.LfmHyp)
    for name, tail in (("lfm_loocv_f64", [dp, dp, dp]), ("lfm_loocv_grad_f64", [dp, dp])):
        res, args = bound[name]
        assert res is ctypes.c_int
        assert args[1:] == [dp, dp, ctypes.c_int64, hyp, ctypes.c_int] + tail
    # the gradient call is lfm_mll_grad_f64's signature exactly
    assert bound["lfm_loocv_grad_f64"] == bound["lfm_mll_grad_f64"]
    lib = _lib.load_library()
    assert lib.lfm_abi_version() == 5
    assert all(hasattr(lib, name) for name in NAMES)
    # one new profile class, after the 24 there were, within lfm_profile_classes' mask
    assert _lib.LOO_KCLASSES == ["loo_product"]
    assert len(_lib.KCLASSES) + len(_lib.SAMPLE_KCLASSES) + len(_lib.LOO_KCLASSES) == 25 <= 32


def test_null_ctx_and_pointers_are_rejected_without_a_gpu():
    from dis_project_amd import _lib

    lib = _lib.load_library()
    d = _lib.dptr
    x, y = np.zeros((10, 3)), np.zeros(10)
    val, mean, var, grad = np.full(1, 7.0), np.full(10, 7.0), np.full(10, 7.0), np.full(17, 7.0)
    hyp = _lib.HypArgs(np.ones(5), np.ones(5), np.ones(5), 2.5, 1.0, 1e-4)
    # a NULL ctx: bare LFM_E_ARG, whatever else is given
    assert lib.lfm_loocv_f64(None, None, None, 0, None, 0, None, None, None) == _lib.LFM_E_ARG
    assert lib.lfm_loocv_f64(None, d(x), d(y), 10, hyp.ref, 0, d(val), d(mean),
                             d(var)) == _lib.LFM_E_ARG
    assert lib.lfm_loocv_grad_f64(None, None, None, 0, None, 0, None, None) == _lib.LFM_E_ARG
    assert lib.lfm_loocv_grad_f64(None, d(x), d(y), 10, hyp.ref, 1, d(val),
                                  d(grad)) == _lib.LFM_E_ARG
    for buf in (val, mean, var, grad):
        assert np.all(buf == 7.0)


def test_loocv_shape_errors_need_no_gpu():
    """Shapes are checked before the first device call (model.ctx would create a context)."""
    import dis_project_amd as lfm

    assert lfm.CustomConjLOOCV in (lfm.CustomConjLOOCV,) and "CustomConjLOOCV" in lfm.__all__
    obj = lfm.CustomConjLOOCV(negative=True)
    assert obj.constant == -1.0 and lfm.CustomConjLOOCV().constant == 1.0

    class NoDevice(lfm.ExactLFM):
        @property
        def ctx(self):
            raise AssertionError("a device call before the shapes were checked")

    model = NoDevice(jitter=1e-4, num_genes=5)
    # Dataset checks its own shapes; the objective must not rely on that (any object with X and y)
    data = lambda X, y: SimpleNamespace(X=X, y=y)  # noqa: E731
    for fn in (obj, obj.step, obj.value_and_grad, obj.pointwise):
        with pytest.raises(ValueError, match="same number of rows"):
            fn(model, data(np.ones((10, 3)), np.ones((9, 1))))
        with pytest.raises(ValueError, match="multiple of num_genes"):
            fn(model, lfm.Dataset(np.ones((7, 3)), np.ones((7, 1))))
        with pytest.raises(ValueError, match=r"\[n, 3\]"):
            fn(model, data(np.ones((10, 2)), np.ones((10, 1))))
        with pytest.raises(AssertionError, match="device call"):
            fn(model, lfm.Dataset(np.ones((10, 3)), np.ones((10, 1))))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_strict_build():
    """Every unit with warnings as errors."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "dis_project_amd", "csrc"),
                        "-j", str(min(16, os.cpu_count() or 4)), "strict"],
                       capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])

"""CPU checks of the held-out log density on the resident posterior (lfm_post_log_prob_f64,
predict.Posterior.log_prob): its plan under AddressSanitizer + UBSan (tests/native/
post_logp_plan_check.cpp, a stand-alone program built here with the flags of
tests/native/Makefile and run directly), the entry point in the header and the ctypes table, the
argument checks that need no GPU, and the strict build."""

import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "lfm_post_log_prob_f64"


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan")
def test_plan_post_logp_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "post_logp_plan_check")
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *san, "-pthread",
                        os.path.join(ROOT, "tests", "native", "post_logp_plan_check.cpp"),
                        os.path.join(ROOT, "dis_project_amd", "csrc", "lfm_host.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "post_logp_plan_check: all passed" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_header_and_signature_agree():
    import ctypes

    from dis_project_amd import _lib
    from tests.test_abi import header_functions

    declared = header_functions()
    bound = {name: (res, args) for name, res, args in _lib.PRODUCT_SIGNATURES}
    assert set(bound) == set(declared)
    assert NAME in declared and NAME in bound
    # the declaration, argument by argument, against the ctypes table
    with open(os.path.join(ROOT, "include", "lfm.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    m = re.search(r"int\s+" + NAME + r"\s*\(([^)]*)\)\s*;", text)
    assert m, "the header declares it"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["lfm_ctx* ctx", "lfm_post* post", "const double* t", "int64_t m",
                      "double diag_add", "const double* ystar", "int64_t k", "double* mean",
                      "double* logp"]
    res, args = bound[NAME]
    dp = _lib._dptr  # how the table passes a host double*
    assert res is ctypes.c_int
    assert args[1:] == [ctypes.c_void_p, dp, ctypes.c_int64, ctypes.c_double, dp, ctypes.c_int64,
                        dp, dp]
    assert args == bound["lfm_post_sample_f64"][1][:5] + [dp, ctypes.c_int64, dp, dp]
    lib = _lib.load_library()
    assert lib.lfm_abi_version() == 5
    assert hasattr(lib, NAME)
    assert len(_lib.KCLASSES) + len(_lib.SAMPLE_KCLASSES) <= 32  # no new profile class


def test_null_handle_and_pointers_are_rejected_without_a_gpu():
    from dis_project_amd import _lib

    lib = _lib.load_library()
    t, y = np.zeros((5, 3)), np.zeros((2, 5))
    mean, logp = np.full(5, 7.0), np.full(2, 7.0)
    d = _lib.dptr
    # a NULL ctx: bare LFM_E_ARG, whatever else is given
    call = lib.lfm_post_log_prob_f64
    assert call(None, None, None, 0, 0.0, None, 0, None, None) == _lib.LFM_E_ARG
    assert lib.lfm_post_log_prob_f64(None, None, d(t), 5, 1e-4, d(y), 2, d(mean),
                                     d(logp)) == _lib.LFM_E_ARG
    assert np.all(mean == 7.0) and np.all(logp == 7.0)


def test_posterior_log_prob_shape_errors_need_no_gpu():
    """Shapes are checked before the first device call; after a failed fit the result is NaN."""
    import dis_project_amd as lfm

    post = object.__new__(lfm.Posterior)
    post.num_genes, post.kind, post.jitter = 5, "gene", 1e-4
    post._handle, post._final, post.ctx = None, None, None
    t = np.ones((10, 3))
    with pytest.raises(ValueError, match=r"\[m, 3\]"):
        post.log_prob(np.zeros((10, 2)), np.zeros(10))
    with pytest.raises(ValueError, match="multiple"):
        post.log_prob(np.zeros((7, 3)), np.zeros(7))
    for bad in (np.zeros(9), np.zeros((2, 9)), np.zeros((10, 2)), np.zeros((0, 10)),
                np.zeros((1, 2, 10)), np.float64(1.0)):
        with pytest.raises(ValueError, match="y_star"):
            post.log_prob(t, bad)
    one = post.log_prob(t, np.zeros(10))
    assert isinstance(one, float) and np.isnan(one)
    many = post.log_prob(t, np.zeros((3, 10)), cov_add=0.3)
    assert many.shape == (3,) and np.all(np.isnan(many))
    post.close()


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_strict_build():
    """Every unit with warnings as errors."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "dis_project_amd", "csrc"),
                        "-j", str(min(16, os.cpu_count() or 4)), "strict"],
                       capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])

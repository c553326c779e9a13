"""CPU checks of the resident posterior (lfm_post_*, predict.Posterior): its launch plan under
AddressSanitizer + UBSan (tests/native/post_plan_check.cpp, a stand-alone program built here
with the flags of tests/native/Makefile), the shim's argument checks that need no GPU, the four
new entry points in the header and the ctypes table, and the strict build."""

import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lfm_post_create", "lfm_post_destroy", "lfm_post_predict_f64", "lfm_post_set_chunk"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan")
def test_plan_post_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "post_plan_check")
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *san, "-pthread",
                        os.path.join(ROOT, "tests", "native", "post_plan_check.cpp"),
                        os.path.join(ROOT, "dis_project_amd", "csrc", "lfm_host.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "post_plan_check: all passed" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_header_and_signatures_carry_the_new_entry_points():
    from dis_project_amd import _lib
    from tests.test_abi import header_functions

    declared = header_functions()
    bound = {name for name, _, _ in _lib.PRODUCT_SIGNATURES}
    assert bound == set(declared)
    for name in NEW:
        assert name in declared and name in bound
    lib = _lib.load_library()
    assert lib.lfm_abi_version() == 5
    for name in NEW:
        assert hasattr(lib, name)
    for cls in ("post_panel", "post_update"):
        assert cls in _lib.KCLASSES
    assert len(_lib.KCLASSES) <= 32  # lfm_profile_classes' mask


def test_null_handles_are_rejected_without_a_gpu():
    from dis_project_amd import _lib

    lib = _lib.load_library()
    assert lib.lfm_post_destroy(None) == _lib.LFM_E_ARG
    assert lib.lfm_post_set_chunk(None, 128) == _lib.LFM_E_ARG
    assert lib.lfm_post_predict_f64(None, None, None, 0, None, None, None) == _lib.LFM_E_ARG
    assert lib.lfm_post_create(None, None, None, 0, None, 0.0, None, None) == _lib.LFM_E_ARG


def test_posterior_argument_checks_need_no_gpu():
    """kind and the shapes are checked before any context is asked for."""
    import dis_project_amd as lfm
    from dis_project_amd import dataset as ds

    assert lfm.Posterior is lfm.predict.Posterior
    data = ds.SyntheticP53Data(replicate=0, seed=5)
    model = lfm.ExactLFM(num_genes=5)
    with pytest.raises(ValueError, match="kind"):
        lfm.Posterior(model, data, kind="both")
    with pytest.raises(ValueError, match="kind"):
        model.posterior(data, "cov")
    with pytest.raises(ValueError, match="num_genes"):
        lfm.Posterior(lfm.ExactLFM(num_genes=4), data, "gene")  # n = 35 rows, 4 genes

    # the test-input checks of a constructed object (no handle: as after a failed fit)
    post = object.__new__(lfm.Posterior)
    post.num_genes, post.kind, post.jitter = 5, "latent", 1e-4
    post._handle, post._final, post.ctx = None, None, None
    with pytest.raises(ValueError, match=r"\[m, 3\]"):
        post.predict(np.zeros((10, 2)))
    with pytest.raises(ValueError, match="multiple"):
        post.marginals(np.zeros((7, 3)))
    with pytest.raises(ValueError, match="multiple"):
        post.marginals(np.zeros((0, 3)))
    mean, var = post.marginals(np.ones((10, 3)))
    assert mean.shape == var.shape == (10,) and np.all(np.isnan(mean)) and np.all(np.isnan(var))
    post.close()


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="needs hipcc")
def test_strict_build():
    """Every unit, lfm_post.hip and lfm_post_api.hip included, with warnings as errors."""
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "dis_project_amd", "csrc"),
                        "-j", str(min(16, os.cpu_count() or 4)), "strict"],
                       capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])

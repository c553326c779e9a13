"""CPU checks of the on-device fit of the mid-size resident batch (lfm_mbatch_fit_f64,
farm.MidBatchEvaluator.fit_packed, trainer.MidBatchTrainer(on_device=True)): its third arena and
launch list under AddressSanitizer + UBSan (tests/native/mid_fit_plan_check.cpp, a stand-alone
program built here with the flags of tests/native/Makefile), the entry point in the header and
the ctypes table, the NULL checks that need no GPU, and the trainer's option: refused at
construction without a fit_packed, and off by default with the host loop's result unchanged."""

import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan")
def test_plan_mid_fit_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "mid_fit_plan_check")
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *san, "-pthread",
                        os.path.join(ROOT, "tests", "native", "mid_fit_plan_check.cpp"),
                        os.path.join(ROOT, "dis_project_amd", "csrc", "lfm_host.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "mid_fit_plan_check: all passed" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_header_declares_and_lib_binds_the_fit():
    from dis_project_amd import _lib
    from tests.test_abi import header_functions

    declared = header_functions()
    sigs = {name: args for name, _, args in _lib.PRODUCT_SIGNATURES}
    assert "lfm_mbatch_fit_f64" in declared and "lfm_mbatch_fit_f64" in sigs
    # the arguments are lfm_batch_fit_f64's, word for word
    assert sigs["lfm_mbatch_fit_f64"] == sigs["lfm_batch_fit_f64"]
    lib = _lib.load_library()
    assert lib.lfm_abi_version() == 5
    assert hasattr(lib, "lfm_mbatch_fit_f64")
    # timed under the existing finish class: no class was added
    assert _lib.KCLASSES[-1] == "mid_finish" and len(_lib.KCLASSES) == 22


def test_null_ctx_and_handle_are_rejected_without_a_gpu():
    from dis_project_amd import _lib

    lib = _lib.load_library()
    raw = np.zeros(6)
    opt = _lib.LfmAdam(0.01, 0.9, 0.999, 1e-8, 0.0, 1000, 1)
    assert lib.lfm_mbatch_fit_f64(None, None, None, 1, 0, 1, None, None, None, None,
                                  None) == _lib.LFM_E_ARG
    assert lib.lfm_mbatch_fit_f64(None, None, _lib.ctypes.byref(opt), 1, 0, 1, _lib.dptr(raw),
                                  _lib.dptr(raw), _lib.dptr(raw), _lib.dptr(raw),
                                  None) == _lib.LFM_E_ARG


def _problem(G, T, seed):
    from dis_project_amd.dataset import Dataset, grid_inputs
    from dis_project_amd.model import ExactLFM

    rng = np.random.default_rng(seed)
    D, S, B = rng.uniform(0.2, 1.0, G), rng.uniform(0.5, 1.5, G), rng.uniform(0.01, 0.1, G)
    y = np.repeat(B / D, T) + 0.5 * rng.standard_normal(G * T)
    model = ExactLFM(jitter=1e-4, num_genes=G, true_d=D, true_s=S, true_b=B, l=2.2,
                     obs_stddev=0.9)
    return model, Dataset(grid_inputs(G, T), y)


class _StubEvaluator:
    """value_and_grad(models) from a closed form of the models alone; no fit_packed."""

    calls = 0

    def value_and_grad(self, models):
        self.calls += 1
        vals = np.array([float(np.sum(m.true_d ** 2) + m.l * m.obs_stddev) for m in models])
        grads = [{"true_d": 2.0 * np.asarray(m.true_d), "true_s": np.cos(np.asarray(m.true_s)),
                  "true_b": -np.asarray(m.true_b), "l": float(m.obs_stddev),
                  "obs_stddev": float(m.l)} for m in models]
        return vals, grads


class _StubObjective:
    negative = True

    def __init__(self, stub, p):
        self.stub, self.p = stub, p

    def value_and_grad(self, model, data):
        vals, grads = self.stub.value_and_grad([model])
        return float(vals[0]), grads[0]


def test_on_device_needs_an_evaluator_with_fit_packed(monkeypatch):
    """Refused at construction, before any context is asked for."""
    from dis_project_amd import _lib
    from dis_project_amd import trainer as TR

    def no_context(*a, **k):
        raise AssertionError("a context was asked for")

    monkeypatch.setattr(_lib, "get_context", no_context)
    models, datasets = zip(*[_problem(4, 7, 11), _problem(3, 9, 12)])
    with pytest.raises(ValueError, match="fit_packed"):
        TR.MidBatchTrainer(models, _StubObjective(None, 0), datasets, TR.adam(0.01), num_iters=3,
                           evaluator=_StubEvaluator(), on_device=True)
    # the default stays the host loop: the same stub is accepted
    bt = TR.MidBatchTrainer(models, _StubObjective(None, 0), datasets, TR.adam(0.01), num_iters=3,
                            evaluator=_StubEvaluator())
    assert bt.on_device is False


@pytest.mark.parametrize("fix_params", [True, False])
def test_host_loop_is_the_default_and_unchanged(fix_params):
    """on_device=False (spelled out, and by default) with a stub evaluator: every problem gets
    exactly its own JaxTrainer loop on the same closed-form objective — today's host loop — from
    one value_and_grad call per step."""
    from dis_project_amd import trainer as TR

    models, datasets = zip(*[_problem(4, 7, 11), _problem(3, 9, 12)])
    want = []
    for p, (m, d) in enumerate(zip(models, datasets)):
        jt = TR.JaxTrainer(m, _StubObjective(_StubEvaluator(), p), d, TR.adam(0.01), num_iters=6)
        fitted, h = jt.fit(fix_params=fix_params, num_steps_per_epoch=4)
        want.append((fitted, h, jt.raw))
    for kwargs in ({"on_device": False}, {}):
        ev = _StubEvaluator()
        bt = TR.MidBatchTrainer(models, _StubObjective(None, 0), datasets, TR.adam(0.01),
                                num_iters=6, evaluator=ev, **kwargs)
        fitted, hist = bt.fit(fix_params=fix_params, num_steps_per_epoch=4)
        assert ev.calls == 6 and hist.shape == (2, 6)
        for p, (wm, wh, wraw) in enumerate(want):
            np.testing.assert_array_equal(hist[p], wh)
            for k in ("true_d", "true_s", "true_b"):
                np.testing.assert_array_equal(getattr(fitted[p], k), getattr(wm, k))
                np.testing.assert_array_equal(bt.raws[p][k], wraw[k])
            assert fitted[p].l == wm.l and fitted[p].obs_stddev == wm.obs_stddev
        bt.close()

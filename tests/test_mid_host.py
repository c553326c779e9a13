"""CPU checks of the mid-size resident batch (lfm_mbatch_*, farm.MidBatchEvaluator,
trainer.MidBatchTrainer): its arena and launch plan under AddressSanitizer + UBSan
(tests/native/mid_plan_check.cpp, a stand-alone program built here with the flags of
tests/native/Makefile), the five entry points in the header and the ctypes table, the NULL
checks that need no GPU, the trainer's host loop against per-problem JaxTrainer loops driven by
the oracle, and the evaluator's argument checks."""

import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["lfm_mbatch_create", "lfm_mbatch_destroy", "lfm_mbatch_hyp_size", "lfm_mbatch_mll_f64",
       "lfm_mbatch_mll_grad_f64"]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan")
def test_plan_mid_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "mid_plan_check")
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *san, "-pthread",
                        os.path.join(ROOT, "tests", "native", "mid_plan_check.cpp"),
                        os.path.join(ROOT, "dis_project_amd", "csrc", "lfm_host.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "mid_plan_check: all passed" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_header_and_signatures_carry_the_new_entry_points():
    from dis_project_amd import _lib
    from tests.test_abi import header_functions

    declared = header_functions()
    bound = {name for name, _, _ in _lib.PRODUCT_SIGNATURES}
    assert bound == set(declared)
    for name in NEW:
        assert name in declared and name in bound
    src = open(os.path.join(ROOT, "include", "lfm.h")).read()
    assert "#define LFM_MID_MAX_N 1024" in src
    lib = _lib.load_library()
    assert lib.lfm_abi_version() == 5
    for name in NEW:
        assert hasattr(lib, name)
    for cls in ("mid_fill", "mid_column", "mid_inverse", "mid_pairs", "mid_finish"):
        assert cls in _lib.KCLASSES
    assert _lib.KCLASSES[17:] == ["mid_fill", "mid_column", "mid_inverse", "mid_pairs",
                                  "mid_finish"]  # appended: the earlier classes keep their bits
    assert len(_lib.KCLASSES) <= 32  # lfm_profile_classes' mask


def test_null_handles_are_rejected_without_a_gpu():
    import ctypes

    from dis_project_amd import _lib

    lib = _lib.load_library()
    n = ctypes.c_int64(0)
    assert lib.lfm_mbatch_destroy(None) == _lib.LFM_E_ARG
    assert lib.lfm_mbatch_hyp_size(None, ctypes.byref(n)) == _lib.LFM_E_ARG
    assert lib.lfm_mbatch_create(None, 0, None, None) == _lib.LFM_E_ARG
    assert lib.lfm_mbatch_mll_f64(None, None, None, 0, None, None) == _lib.LFM_E_ARG
    assert lib.lfm_mbatch_mll_grad_f64(None, None, None, 0, None, None, None) == _lib.LFM_E_ARG


def _problem(G, T, seed):
    from dis_project_amd.dataset import Dataset, grid_inputs
    from dis_project_amd.model import ExactLFM

    rng = np.random.default_rng(seed)
    D, S, B = rng.uniform(0.2, 1.0, G), rng.uniform(0.5, 1.5, G), rng.uniform(0.01, 0.1, G)
    y = np.repeat(B / D, T) + 0.5 * rng.standard_normal(G * T)
    model = ExactLFM(jitter=1e-4, num_genes=G, true_d=D, true_s=S, true_b=B, l=2.2,
                     obs_stddev=0.9)
    return model, Dataset(grid_inputs(G, T), y)


class _OracleEvaluator:
    """value_and_grad(models) of a batch from oracle.mll_grad, one problem at a time."""

    def __init__(self, datasets, negative):
        self.datasets, self.negative, self.calls = datasets, negative, 0

    def value_and_grad(self, models):
        from tests.test_trainer import OracleObjective

        self.calls += 1
        obj = OracleObjective(self.negative)
        pairs = [obj.value_and_grad(m, d) for m, d in zip(models, self.datasets)]
        return np.array([v for v, _ in pairs]), [g for _, g in pairs]


@pytest.mark.parametrize("fix_params", [True, False])
def test_mid_batch_trainer_host_loop_matches_jax_trainer(fix_params):
    """Two problems, (4, 7) and (3, 9), 10 steps, after_epoch every 4: each problem gets the
    history and parameters of its own JaxTrainer loop on the oracle (1e-12 relative), from one
    value_and_grad call per step."""
    from dis_project_amd import trainer as TR
    from tests.test_trainer import OracleObjective

    models, datasets = zip(*[_problem(4, 7, 11), _problem(3, 9, 12)])
    ev = _OracleEvaluator(datasets, True)
    bt = TR.MidBatchTrainer(models, OracleObjective(True), datasets, TR.adam(0.01), num_iters=10,
                            evaluator=ev)
    fitted, hist = bt.fit(fix_params=fix_params, num_steps_per_epoch=4)
    assert ev.calls == 10 and hist.shape == (2, 10)
    for p, (m, d) in enumerate(zip(models, datasets)):
        jt = TR.JaxTrainer(m, OracleObjective(True), d, TR.adam(0.01), num_iters=10)
        want, h = jt.fit(fix_params=fix_params, num_steps_per_epoch=4)
        np.testing.assert_allclose(hist[p], h, rtol=1e-12, atol=0)
        for k in ("true_d", "true_s", "true_b"):
            np.testing.assert_allclose(getattr(fitted[p], k), getattr(want, k), rtol=1e-12, atol=0)
            np.testing.assert_allclose(bt.raws[p][k], jt.raw[k], rtol=1e-12, atol=0)
        assert fitted[p].l == pytest.approx(want.l, rel=1e-12)
        assert fitted[p].obs_stddev == pytest.approx(want.obs_stddev, rel=1e-12)
    bt.close()


def test_mid_batch_evaluator_argument_checks_need_no_gpu(monkeypatch):
    """Mismatched rows and an n that is no multiple of num_genes raise ValueError before any
    context is asked for."""
    import dis_project_amd as lfm
    from dis_project_amd import _lib, farm
    from dis_project_amd.dataset import Dataset, grid_inputs

    assert lfm.MidBatchEvaluator is farm.MidBatchEvaluator
    assert lfm.MidBatchTrainer is lfm.trainer.MidBatchTrainer

    def no_context(*a, **k):
        raise AssertionError("a context was asked for")

    monkeypatch.setattr(_lib, "get_context", no_context)
    x = grid_inputs(3, 43)

    class Ragged:
        X, y = x, np.zeros(128)

    with pytest.raises(ValueError, match="rows"):
        farm.MidBatchEvaluator(None, [Ragged])
    with pytest.raises(ValueError, match="1024"):
        farm.MidBatchEvaluator(None, [Dataset(grid_inputs(1, 1025), np.zeros(1025))])
    ev = farm.MidBatchEvaluator(None, [Dataset(x, np.zeros(129))])
    with pytest.raises(ValueError, match="multiple"):
        ev([lfm.ExactLFM(num_genes=2)])
    with pytest.raises(ValueError, match="multiple"):
        ev.value_and_grad([lfm.ExactLFM(num_genes=2)])
    with pytest.raises(ValueError, match="one model"):
        ev([])
    ev.close()

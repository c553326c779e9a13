"""CPU checks of the mid-size batched posterior (lfm_mbatch_posterior_f64,
predict.MidBatchPredictor): plan_mid_post's arena and launch list under AddressSanitizer + UBSan
(tests/native/mid_post_plan_check.cpp, a stand-alone program built here with the flags of
tests/test_mid_host.py), the entry point in the header and the ctypes table, the NULL check that
needs no GPU, the predictor's argument checks, and the oracle's own error at the inputs of
tests/test_gpu_mid_predict.py."""

import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import mid_predict_inputs as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan")
def test_plan_mid_post_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "mid_post_plan_check")
    san = ["-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", *san, "-pthread",
                        os.path.join(ROOT, "tests", "native", "mid_post_plan_check.cpp"),
                        os.path.join(ROOT, "dis_project_amd", "csrc", "lfm_host.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "mid_post_plan_check: all passed" in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr


def test_header_and_signatures_carry_the_entry_point():
    from dis_project_amd import _lib
    from tests.test_abi import header_functions

    declared = header_functions()
    bound = {name for name, _, _ in _lib.PRODUCT_SIGNATURES}
    assert bound == set(declared)
    assert "lfm_mbatch_posterior_f64" in declared and "lfm_mbatch_posterior_f64" in bound
    src = open(os.path.join(ROOT, "include", "lfm.h")).read()
    assert "#define LFM_MID_MAX_M 4096" in src
    lib = _lib.load_library()
    assert lib.lfm_abi_version() == 5 and _lib.ABI_VERSION == 5
    assert hasattr(lib, "lfm_mbatch_posterior_f64")
    assert _lib.KCLASSES[17:] == ["mid_fill", "mid_column", "mid_inverse", "mid_pairs",
                                  "mid_finish"] and len(_lib.KCLASSES) == 22  # no new class


def test_null_ctx_is_rejected_without_a_gpu():
    from dis_project_amd import _lib

    lib = _lib.load_library()
    assert lib.lfm_mbatch_posterior_f64(None, None, None, None, None, None, None, None, None,
                                        None, None) == _lib.LFM_E_ARG


def _datas():
    from dis_project_amd.dataset import SyntheticP53Data

    return [SyntheticP53Data(replicate=0, num_timepoints=30),
            SyntheticP53Data(replicate=0, num_timepoints=7)]


def test_mid_batch_predictor_argument_checks_need_no_gpu(monkeypatch):
    """A mismatched model count, an m that is no multiple of num_genes and an evaluator whose
    data differ raise ValueError before any context is asked for."""
    import dis_project_amd as lfm
    from dis_project_amd import _lib, farm, predict
    from dis_project_amd.dataset import Dataset, dataset_3d

    assert lfm.MidBatchPredictor is predict.MidBatchPredictor

    def no_context(*a, **k):
        raise AssertionError("a context was asked for")

    monkeypatch.setattr(_lib, "get_context", no_context)
    datas = _datas()
    bp = predict.MidBatchPredictor(datas)
    assert len(bp) == 2 and bp.status.shape == (2,)
    models = [lfm.ExactLFM(num_genes=5), lfm.ExactLFM(num_genes=5)]
    t = np.stack((np.linspace(0, 12, 10), np.repeat(np.arange(5.0), 2), np.ones(10)), -1)
    with pytest.raises(ValueError, match="one model"):
        bp.latent_predict(models[:1], t)
    with pytest.raises(ValueError, match="multiple"):
        bp.multi_gene_predict(models, t[:9])
    with pytest.raises(ValueError, match="multiple"):
        bp.marginals(models, [t, t[:3]])
    with pytest.raises(ValueError, match="4096"):
        bp.marginals(models, np.tile(t, (410, 1)))
    with pytest.raises(ValueError, match="kind"):
        bp.marginals(models, t, kind="other")
    bp.close()

    # an evaluator over the same data is taken as it is; one over other data is refused
    sets = []
    for d in datas:
        x, y, _ = dataset_3d(d)
        sets.append(Dataset(np.asarray(x, np.float64).reshape(-1, 3),
                            np.asarray(y, np.float64).reshape(-1)))
    ev = farm.MidBatchEvaluator(None, sets)
    bp = predict.MidBatchPredictor(datas, evaluator=ev)
    assert bp._ev is ev and len(bp) == 2
    bp.close()
    assert ev.datasets  # a borrowed evaluator is not closed
    y2 = np.array(sets[1].y, np.float64).reshape(-1)
    y2[3] += 1e-9
    other = farm.MidBatchEvaluator(None, [sets[0], Dataset(np.asarray(sets[1].X), y2)])
    with pytest.raises(ValueError, match="differ"):
        predict.MidBatchPredictor(datas, evaluator=other)
    with pytest.raises(ValueError, match="number of problems"):
        predict.MidBatchPredictor(datas[:1], evaluator=ev)
    with pytest.raises(ValueError, match="no training data"):
        predict.MidBatchPredictor([])


def test_batch_predictor_keeps_its_surface():
    """The assembly is shared, not copied: both predictors have BatchPredictor's methods from
    one place."""
    from dis_project_amd import predict

    for name in ("latent_predict", "multi_gene_predict", "marginals"):
        assert getattr(predict.BatchPredictor, name) is getattr(predict.MidBatchPredictor, name)
    for name in ("status", "close", "__len__"):
        assert name == "status" or callable(getattr(predict.MidBatchPredictor, name))


# ------------------------------------------------------------------ the oracle's own error
def _longdouble_posterior(p, obs, with_v):
    """mean and cov from the oracle's own gram entries by a Cholesky and forward solves in
    np.longdouble (the same algebra as the kernels: V = K(t,x) L^{-T}, z = L^{-1} r)."""
    from oracle import lfm_oracle as O

    ld = np.longdouble
    x, t, D, S, B = p["x"], p["t"], p["D"], p["S"], p["B"]
    n = p["n"]
    A = O.gram(x, D, S, I.L).astype(ld)
    if with_v:
        A[np.diag_indices(n)] += p["v"].astype(ld)
    A[np.diag_indices(n)] += ld(obs) ** 2
    Kxt = O.cross_covariance(x, t, D, S, I.L).astype(ld)
    Ktt = O.gram(t, D, S, I.L).astype(ld)
    r = (p["y"].reshape(-1, 1) - O.mean_function(x, D, B, p["G"])).astype(ld)
    Lf = np.zeros((n, n), ld)
    for j in range(n):  # left-looking, column by column
        c = A[j:, j] - Lf[j:, :j] @ Lf[j, :j]
        assert c[0] > 0
        Lf[j:, j] = c / np.sqrt(c[0])
    W = np.concatenate((Kxt, r), axis=1)  # forward solve of K(x,t) and the residual together
    for i in range(n):
        W[i] = (W[i] - Lf[i, :i] @ W[:i]) / Lf[i, i]
    V, z = W[:, :-1], W[:, -1:]
    mean = O.mean_function(t, D, B, p["G"]).astype(ld) + V.T @ z
    cov = Ktt - V.T @ V
    return mean.reshape(-1), cov, float(np.linalg.cond(A.astype(np.float64)))


@pytest.mark.parametrize("idx", range(len(I.parity_inputs())))
def test_oracle_is_within_a_hundredth_of_the_tolerance(idx):
    """At every input at which tests/test_gpu_mid_predict.py compares against
    O.multi_gene_predict, the oracle itself is within 1/100 of the tolerance
    (1e-9 max|ref| + 1e-12) of the long-double restatement on its own gram entries."""
    p, obs, with_v = I.parity_inputs()[idx]
    ref_m, ref_c = I.oracle(p, obs, with_v)
    mean, cov, cond = _longdouble_posterior(p, obs, with_v)
    figs = []
    for got, ref in ((mean, ref_m), (cov, ref_c)):
        bound = I.RTOL * float(np.max(np.abs(ref))) + I.ATOL
        figs.append(float(np.max(np.abs(ref.astype(np.longdouble) - got))) / bound)
    print(f"n = {p['n']} m = {p['m']} diag_add = {obs ** 2:.3g} diag_vec = {with_v}: oracle error / "
          f"bound mean {figs[0]:.2e} cov {figs[1]:.2e}, cond(S) {cond:.2e}")
    assert max(figs) <= 0.01, figs

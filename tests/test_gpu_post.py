"""The resident posterior (lfm_post_create / lfm_post_predict_f64, predict.Posterior): factor a
large model once, predict many times.

  1. exact truth: tests/golden/exact_posterior.npz (groups a and b of
     tests/test_gpu_exact_posterior.py) under that file's bound,
     max|d| <= post_rtol max|truth| + 1e-12, one handle per (restart, diagonal);
  2. several super-panels against oracle.multi_gene_predict and against lfm_posterior_f64 on the
     same inputs, bound 1e-9 max|ref| + 1e-12 (tests/test_gpu_predict.py);
  3. the split: chunks of 128 rows, a prefix of the test rows and a repeated call give the same
     bits;
  4. the handle owns its memory: other calls on the ctx between two predicts change nothing;
  5. the covariance: exactly symmetric, var = diag(cov) bit for bit;
  6. argument errors; 7. the Python shim against the predictors' goldens.
"""

import ctypes
import functools

import numpy as np
import pytest

from oracle import lfm_exact as E
from oracle import lfm_oracle as O
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

B_RESTARTS = (0, 7, 13, 19, 29)


# ------------------------------------------------------------------ plumbing
def ctx0():
    from dis_project_amd import _lib

    return _lib.get_context(0)


def post_create(ctx, x, y, v, dadd, hyp):
    """lfm_post_create -> (rc, handle or None)."""
    from dis_project_amd import _lib

    h = ctypes.c_void_p()
    rc = ctx.lib.lfm_post_create(ctx.handle, _lib.dptr(x), _lib.dptr(y), x.shape[0],
                                 None if v is None else _lib.dptr(v), float(dadd), hyp.ref,
                                 ctypes.byref(h))
    if rc not in (_lib.LFM_OK, _lib.LFM_E_NOT_PD):
        ctx.check(rc)
    return rc, (h if h.value else None)


def post_predict(ctx, h, t, want_var=True, want_cov=False):
    """lfm_post_predict_f64 -> (mean, var or None, cov or None); raises on a non-OK code."""
    from dis_project_amd import _lib

    m = t.shape[0]
    mean = np.full(m, 7.0)
    var = np.full(m, 7.0) if want_var else None
    cov = np.full((m, m), 7.0) if want_cov else None
    ctx.check(ctx.lib.lfm_post_predict_f64(ctx.handle, h, _lib.dptr(t), m, _lib.dptr(mean),
                                           _lib.dptr(var) if want_var else None,
                                           _lib.dptr(cov) if want_cov else None))
    return mean, var, cov


def destroy(ctx, h):
    assert ctx.lib.lfm_post_destroy(h) == 0


def close(a, b, rtol=1e-9):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape
    assert np.max(np.abs(a - b)) <= rtol * np.max(np.abs(b)) + 1e-12


def ratio(got, ref, rtol):
    """max|d| / (rtol max|truth| + 1e-12): at most 1 for a right answer."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    with np.errstate(invalid="ignore"):
        d = float(np.nan_to_num(np.max(np.abs(got - ref)), nan=np.inf))
    return d / (rtol * float(np.max(np.abs(ref))) + 1e-12)


def full_of(tril, m):
    out = np.empty((m, m))
    ii, jj = np.tril_indices(m)
    out[ii, jj] = tril
    out[jj, ii] = tril
    return out


# ------------------------------------------------------------------ 1. exact truth
@pytest.fixture(scope="module")
def fx():
    g = load_golden("exact_posterior")
    assert tuple(int(r) for r in g["b_restarts"]) == B_RESTARTS
    return g


@pytest.fixture(scope="module")
def restarts():
    from dis_project_amd import configs

    return configs.c3_restarts(configs.c2(), 32)


def check_group(fx, pre, models, labels, x, y, v, t):
    from dis_project_amd import _lib

    ctx = ctx0()
    m = t.shape[0]
    bad = []
    for q, (r, model) in enumerate(zip(labels, models)):
        figs = []
        for kind in (0, 1):
            dadd = model.jitter if kind == 0 else model.obs_stddev ** 2
            rc, h = post_create(ctx, x, y, v, dadd, model.hyp())
            if fx[pre + "_not_pd"][q, kind]:
                assert rc == _lib.LFM_E_NOT_PD and h is None
                continue
            assert rc == 0 and h is not None, (r, kind, rc)
            try:
                mean, var, cov = post_predict(ctx, h, t, True, True)
                mean1, var1, _ = post_predict(ctx, h, t, True, False)
            finally:
                destroy(ctx, h)
            if fx[pre + "_dropped"][q, kind]:
                continue
            np.testing.assert_array_equal(cov, cov.T)
            np.testing.assert_array_equal(var, np.diagonal(cov))
            np.testing.assert_array_equal(mean, mean1)
            rtol = float(fx[pre + "_rtol"][q, kind])
            ref = full_of(fx[pre + "_cov"][q, kind], m)
            figs += [ratio(mean, fx[pre + "_mean"][q, kind], rtol), ratio(cov, ref, rtol),
                     ratio(var1, np.diagonal(ref), rtol)]
        print(f"{pre} r{r}: resident |d| / bound mean, cov, var-only (latent | gene diagonal) = "
              + " ".join(f"{f:.2e}" for f in figs))
        if figs and not max(figs) <= 1.0:
            bad.append((r, [round(f, 3) for f in figs]))
    assert not bad, bad


def test_exact_a_all_restarts(fx, restarts):
    """Group a: n = 28, m = 20, all 32 restarts x both diagonals; one handle each, one predict
    with the covariance and one with the variances only."""
    models = [E.submodel(m, 4)[0] for m in restarts]
    check_group(fx, "a", models, range(32), fx["a_x"], fx["a_y"], fx["a_v"], fx["a_t"])


def test_exact_b_two_block_columns(fx, restarts):
    """Group b: n = 129, m = 45: two block columns with a ragged edge."""
    models = [E.submodel(restarts[r], 3)[0] for r in B_RESTARTS]
    check_group(fx, "b", models, B_RESTARTS, fx["b_x"], fx["b_y"], fx["b_v"], fx["b_t"])


# ------------------------------------------------------------------ 2. super-panels
@functools.lru_cache(maxsize=None)
def case(n_genes, T, m):
    """The recipe of tests/test_gpu_predict.py::test_posterior_schur_sizes, its oracle
    reference and lfm_posterior_f64's answer; computed once, never modified."""
    from dis_project_amd import _lib

    rng = np.random.default_rng(T)
    D = rng.uniform(0.2, 1.0, n_genes); S = rng.uniform(0.5, 1.5, n_genes)
    B = rng.uniform(0.01, 0.1, n_genes)
    n = n_genes * T
    x = np.stack((rng.uniform(0, 12, n), rng.integers(0, n_genes, n).astype(float),
                  np.ones(n)), -1)
    y = rng.normal(0.4, 0.5, n)
    v = rng.uniform(0.01, 0.05, n)
    mm = m - m % n_genes
    t = np.stack((rng.uniform(0, 13, mm), rng.integers(-1, n_genes + 1, mm).astype(float),
                  rng.integers(0, 2, mm).astype(float)), -1)
    ref_m, ref_v = O.multi_gene_predict(x, y, v, t, D, S, B, 1.8, 0.7, 0.0)
    hyp = _lib.HypArgs(D, S, B, 1.8, 0.7, 1e-4)
    ctx = ctx0()
    mean = np.empty(mm)
    cov = np.empty((mm, mm))
    ctx.check(ctx.lib.lfm_posterior_f64(ctx.handle, _lib.dptr(x), _lib.dptr(y), n, _lib.dptr(v),
                                        0.49, _lib.dptr(t), mm, hyp.ref, _lib.dptr(mean),
                                        _lib.dptr(cov)))
    out = dict(x=x, y=y, v=v, t=t, hyp=hyp, ref_m=np.asarray(ref_m), ref_v=np.asarray(ref_v),
               schur_m=mean, schur_v=cov)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def handle_of(c):
    rc, h = post_create(ctx0(), c["x"], c["y"], c["v"], 0.49, c["hyp"])
    assert rc == 0 and h is not None
    return h


@pytest.mark.parametrize("n_genes,T,m", [(4, 250, 300), (3, 215, 129), (3, 43, 129)])
def test_superpanels_vs_oracle(n_genes, T, m):
    """Np = 1024 (two full super-panels), Np = 768 (a ragged second super-panel) and n = 129:
    mixed flags, gene indices -1 .. G; against the oracle and against lfm_posterior_f64."""
    c = case(n_genes, T, m)
    ctx = ctx0()
    h = handle_of(c)
    try:
        mean, var, cov = post_predict(ctx, h, c["t"], True, True)
        mean1, var1, _ = post_predict(ctx, h, c["t"], True, False)
    finally:
        destroy(ctx, h)
    for ref_m, ref_v in ((c["ref_m"], c["ref_v"]), (c["schur_m"], c["schur_v"])):
        print("resident |d| mean, cov, var-only:", np.max(np.abs(mean - ref_m)),
              np.max(np.abs(cov - ref_v)), np.max(np.abs(var1 - np.diagonal(ref_v))),
              "bound", 1e-9 * np.max(np.abs(ref_v)) + 1e-12)
        close(mean, ref_m)
        close(cov, ref_v)
        close(mean1, ref_m)
        close(var1, np.diagonal(ref_v))
    np.testing.assert_array_equal(cov, cov.T)


# ------------------------------------------------------------------ 3. the split
def test_split_independence_bitwise():
    c = case(4, 250, 300)
    ctx = ctx0()
    t = c["t"]
    h = handle_of(c)
    try:
        mean, var, _ = post_predict(ctx, h, t)
        mean_again, var_again, _ = post_predict(ctx, h, t)
        assert ctx.lib.lfm_post_set_chunk(h, 128) == 0  # three passes, the last of 44 rows
        mean_c, var_c, _ = post_predict(ctx, h, t)
        assert ctx.lib.lfm_post_set_chunk(h, 0) == 0
        _, var_head, _ = post_predict(ctx, h, np.ascontiguousarray(t[:128]))
    finally:
        destroy(ctx, h)
    np.testing.assert_array_equal(mean_again, mean)
    np.testing.assert_array_equal(var_again, var)
    np.testing.assert_array_equal(mean_c, mean)
    np.testing.assert_array_equal(var_c, var)
    np.testing.assert_array_equal(var_head, var[:128])
    close(mean, c["ref_m"])
    close(var, np.diagonal(c["ref_v"]))


# ------------------------------------------------------------------ 4. ownership
def test_handle_owns_its_memory():
    """lfm_mll_f64 at n = 1000 and lfm_posterior_f64 at n = 645 regrow / overwrite the ctx
    workspace between two predicts on an n = 129 handle."""
    from dis_project_amd import _lib

    c, big, mid = case(3, 43, 129), case(4, 250, 300), case(3, 215, 129)
    ctx = ctx0()
    h = handle_of(c)
    try:
        first = post_predict(ctx, h, c["t"], True, True)
        out = np.zeros(1)
        ctx.check(ctx.lib.lfm_mll_f64(ctx.handle, _lib.dptr(big["x"]), _lib.dptr(big["y"]), 1000,
                                      big["hyp"].ref, 1, _lib.dptr(out)))
        assert np.isfinite(out[0])
        mm = mid["t"].shape[0]
        mean, cov = np.empty(mm), np.empty((mm, mm))
        ctx.check(ctx.lib.lfm_posterior_f64(ctx.handle, _lib.dptr(mid["x"]), _lib.dptr(mid["y"]),
                                            645, _lib.dptr(mid["v"]), 0.49, _lib.dptr(mid["t"]),
                                            mm, mid["hyp"].ref, _lib.dptr(mean), _lib.dptr(cov)))
        second = post_predict(ctx, h, c["t"], True, True)
    finally:
        destroy(ctx, h)
    for a, b in zip(first, second):
        np.testing.assert_array_equal(a, b)
    close(second[0], c["ref_m"])


# ------------------------------------------------------------------ 5. covariance
def test_covariance_symmetric_and_var_is_its_diagonal():
    c = case(3, 215, 129)
    ctx = ctx0()
    h = handle_of(c)
    try:
        _, var, cov = post_predict(ctx, h, c["t"], True, True)
        _, _, cov_only = post_predict(ctx, h, c["t"], False, True)
        _, var_only, _ = post_predict(ctx, h, c["t"], True, False)
    finally:
        destroy(ctx, h)
    np.testing.assert_array_equal(cov, cov.T)
    np.testing.assert_array_equal(var, np.diagonal(cov))
    np.testing.assert_array_equal(cov_only, cov)
    close(var_only, np.diagonal(cov))


# ------------------------------------------------------------------ 6. arguments
def test_argument_errors():
    from dis_project_amd import _lib

    c = case(3, 43, 129)
    ctx = ctx0()
    lib = ctx.lib
    t = c["t"]
    m = t.shape[0]
    mean, var, cov = np.empty(m), np.empty(m), np.empty((m, m))
    d = _lib.dptr

    def rejected(rc):
        assert rc == _lib.LFM_E_ARG, rc
        msg = lib.lfm_last_error(ctx.handle)
        assert msg and len(msg.decode()) > 8
        return msg.decode()

    h = handle_of(c)
    try:
        rejected(lib.lfm_post_predict_f64(ctx.handle, h, d(t), m - 1, d(mean), d(var), None))
        rejected(lib.lfm_post_predict_f64(ctx.handle, h, d(t), 0, d(mean), d(var), None))
        rejected(lib.lfm_post_predict_f64(ctx.handle, h, None, m, d(mean), d(var), None))
        rejected(lib.lfm_post_predict_f64(ctx.handle, h, d(t), m, None, d(var), None))
        rejected(lib.lfm_post_predict_f64(ctx.handle, h, d(t), m, d(mean), None, None))
        assert lib.lfm_post_set_chunk(h, 128) == 0
        msg = rejected(lib.lfm_post_predict_f64(ctx.handle, h, d(t), m, d(mean), None, d(cov)))
        assert "128" in msg  # m = 129 above the chunk: the message names the limit
        rejected(lib.lfm_post_set_chunk(h, 100))
        # the rejected chunk left the handle as it was, and it still predicts
        got = post_predict(ctx, h, t)[0]
        close(got, c["ref_m"])
    finally:
        destroy(ctx, h)
    assert lib.lfm_post_destroy(None) == _lib.LFM_E_ARG

    g = load_golden("grid_n64")
    hyp = _lib.HypArgs(g["D"], g["S"], g["B"], float(g["l"]), 1.0, 1e-4)
    rc, h = post_create(ctx, g["x"], g["y"], None, -50.0, hyp)
    assert rc == _lib.LFM_E_NOT_PD and h is None


# ------------------------------------------------------------------ 7. the shim
@pytest.mark.parametrize("tag", ["rep0", "all"])
def test_shim_vs_golden(tag):
    import dis_project_amd as lfm
    from dis_project_amd import dataset as ds

    g = load_golden(f"predict_p53_{tag}")
    data = ds.SyntheticP53Data(replicate=0 if tag == "rep0" else None, seed=5)
    model = lfm.ExactLFM(jitter=float(g["jitter"]), obs_stddev=float(g["obs_stddev"]),
                         num_genes=5, true_d=g["D"], true_s=g["S"], true_b=g["B"],
                         l=float(g["l"]))
    for kind, t, mean, scale in (("latent", g["t_lat"], g["lat_mean"], g["lat_var"]),
                                 ("gene", g["t_gene"], g["gene_mean"], g["gene_var"])):
        post = model.posterior(data, kind)
        try:
            assert post.status == 0
            dist = post.predict(t)
            close(dist.loc, mean)
            close(dist.scale, scale)
            mm, mv = post.marginals(t)
            close(mm, mean)
            close(mv, np.diagonal(dist.scale))
        finally:
            post.close()
        post.close()  # idempotent


def test_shim_not_pd_gives_nan():
    import dis_project_amd as lfm
    from dis_project_amd import _lib, dataset as ds

    g = load_golden("predict_p53_rep0")
    data = ds.SyntheticP53Data(replicate=0, seed=5)
    model = lfm.ExactLFM(jitter=-50.0, obs_stddev=float(g["obs_stddev"]), num_genes=5,
                         true_d=g["D"], true_s=g["S"], true_b=g["B"], l=float(g["l"]))
    post = lfm.Posterior(model, data, "latent")
    assert post.status == _lib.LFM_E_NOT_PD
    dist = post.predict(g["t_lat"])
    assert np.all(np.isnan(dist.loc)) and np.all(np.isnan(dist.scale[np.diag_indices(len(dist.loc))]))
    mean, var = post.marginals(g["t_lat"])
    assert np.all(np.isnan(mean)) and np.all(np.isnan(var))
    post.close()

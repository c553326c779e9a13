"""Held-out log density on the resident posterior (lfm_post_log_prob_f64,
predict.Posterior.log_prob).

  1. the truth: tests/golden/exact_predictive.npz (extended precision end to end) at a's 32
     restarts, b at m = 129 and 63 and c's round 15, both cov_add values, within the fixture's own
     bounds, |logp - truth| <= rtol max(1, |truth|) and the mean's form, rtol = 1e-9;
  2. the sweep's update launch: m = 520 on the n = 300 handle (Np' = 640: a panel, an update and a
     second panel; k = 130: three 64-row slabs, a second 128-row tile). The held-out rows are the
     handle's own draw X_s = mean + L z_s, so w_s = z_s up to rounding and
         |logp[s] - (base - 1/2 ||z_s||^2)| <= 50 kappa(scale) m eps max(1, ||z_s||^2)
     (test_gpu_sample.py's bound form), base the call's logp at ystar = mean; base itself against
     numpy's slogdet in the same form; the same at m = 100 and 130 on the p53 handle;
  3. bit identities: prefixes of a k-vector call, the pass size, repeats, the mean, a predict and
     a sample around the call, a NaN row;
  4. Posterior.log_prob against predict(t).log_prob(y) within twice the fixture's bound (each
     route is within it once, by 1. and test_gpu_exact_predictive.py), and its shapes;
  5. failures: not positive definite, and every argument violation with its word and the
     sentinels intact.
"""

import numpy as np
import pytest

from tests.test_gpu_exact_posterior import c5_datas, ratio
from tests.test_gpu_exact_predictive import (Resident, cadds_of, fx,  # noqa: F401 (fixture)
                                             labels_of, problems)
from tests.test_gpu_sample import EPS, posterior, randn, rows_of

pytestmark = pytest.mark.gpu

C_RESIDENT = range(30, 45)  # c's round-15 problems
SEED = 2 ** 35 + 17


def ctx0():
    from dis_project_amd import _lib

    return _lib.get_context(0)


def logp_call(handle, t, cadd, ystar, want_mean=True, expect=0):
    """lfm_post_log_prob_f64 -> (logp [k], mean [m]); sentinels of 7 where nothing is written."""
    from dis_project_amd import _lib

    ctx = ctx0()
    t = np.ascontiguousarray(t, dtype=np.float64)
    ys = np.ascontiguousarray(np.atleast_2d(ystar), dtype=np.float64)
    k, m = ys.shape
    assert m == t.shape[0]
    logp, mean = np.full(k, 7.0), np.full(m, 7.0)
    rc = ctx.lib.lfm_post_log_prob_f64(ctx.handle, handle, _lib.dptr(t), m, float(cadd),
                                       _lib.dptr(ys), k, _lib.dptr(mean) if want_mean else None,
                                       _lib.dptr(logp))
    assert rc == expect, (rc, ctx.lib.lfm_last_error(ctx.handle))
    return logp, mean


@pytest.fixture(scope="module")
def probs(fx):
    return problems(fx)


# ------------------------------------------------------------------ 1. the truth
@pytest.mark.parametrize("pre", ["a", "b129", "b63", "c"])
def test_truth(fx, probs, pre):
    labels = labels_of(pre)
    qs = list(C_RESIDENT) if pre == "c" else list(range(len(labels)))
    bad, worst, where = [], np.zeros(2), [None, None]
    for q in qs:
        p = probs[pre][q]
        with Resident(p) as post:
            for kind in (0, 1):
                logp, mean = logp_call(post.h, p[3], cadds_of(p[4])[kind],
                                       fx[pre + "_ystar"][q, kind])
                rtol = float(fx[pre + "_rtol"][q, kind])
                ref = float(fx[pre + "_logp"][q, kind])
                d = abs(float(logp[0]) - ref)
                figs = np.array([ratio(mean, fx[pre + "_mean"][q, kind], rtol),
                                 (d if np.isfinite(d) else np.inf) / (rtol * max(1.0, abs(ref)))])
                for i in range(2):
                    if not figs[i] <= worst[i]:
                        worst[i], where[i] = figs[i], (labels[q], kind)
                if not figs.max() <= 1.0:
                    bad.append((labels[q], kind, [float(f"{f:.3g}") for f in figs]))
    print(f"resident log_prob {pre}: worst |d| / bound mean, logp = "
          + " ".join(f"{f:.2e}" for f in worst) + f" at (case, cov_add) {where}")
    assert not bad, bad


# ------------------------------------------------------------------ 2. the sweep
@pytest.mark.parametrize("which,m", [("mixed", 520), ("p53", 100), ("p53", 130)])
def test_own_draw_scores_as_its_normals(which, m):
    post = posterior(which, "gene")
    t = rows_of(m, 5, m)
    k = 130
    cadd = post.jitter
    mean0, _, cov0 = post._predict(t, True)
    mean_s, x = post.sample(t, k, SEED)
    np.testing.assert_array_equal(mean_s, mean0)
    logp, mean = logp_call(post._handle, t, cadd, x)
    np.testing.assert_array_equal(mean, mean0)
    base = float(logp_call(post._handle, t, cadd, mean0)[0][0])
    scale = cov0.copy()
    scale[np.diag_indices(m)] += cadd
    kappa = float(np.linalg.cond(scale))
    sign, logdet = np.linalg.slogdet(scale)
    assert sign == 1.0
    ref_base = -0.5 * logdet - 0.5 * m * np.log(2.0 * np.pi)
    d_base, b_base = abs(base - ref_base), 50.0 * kappa * m * EPS * max(1.0, abs(ref_base))
    z2 = np.sum(randn(SEED, 0, k, m) ** 2, axis=1)
    d = np.abs(logp - (base - 0.5 * z2))
    bound = 50.0 * kappa * m * EPS * np.maximum(1.0, z2)
    print(f"{which} m {m} k {k}: kappa {kappa:.3g}; base {base:.6f}, |base - slogdet route| = "
          f"{d_base:.2e} (bound {b_base:.2e}); max |logp - (base - ||z||^2 / 2)| = {d.max():.2e}, "
          f"worst |d| / bound = {np.max(d / bound):.2e}")
    assert np.all(np.isfinite(logp)) and np.isfinite(base)
    assert d_base <= b_base
    assert np.all(d <= bound)


# ------------------------------------------------------------------ 3. bit identities
def test_bit_identities():
    post = posterior("p53", "gene")
    h, m, k, cadd = post._handle, 100, 130, post.jitter
    t = rows_of(m, 5, m)
    pred0 = post._predict(t, True)
    mean_s0, x = post.sample(t, k, SEED)
    logp, mean = logp_call(h, t, cadd, x)
    assert np.all(np.isfinite(logp))
    # prefixes of the k-vector call
    np.testing.assert_array_equal(logp_call(h, t, cadd, x[:64])[0], logp[:64])
    np.testing.assert_array_equal(logp_call(h, t, cadd, x[:1])[0], logp[:1])
    # the pass size: two passes of 128 rows against one of 256
    post.set_chunk(128)
    try:
        np.testing.assert_array_equal(logp_call(h, t, cadd, x)[0], logp)
    finally:
        post.set_chunk(0)
    # the same call twice; without the mean
    again, mean2 = logp_call(h, t, cadd, x)
    np.testing.assert_array_equal(again, logp)
    np.testing.assert_array_equal(mean2, mean)
    nomean, untouched = logp_call(h, t, cadd, x, want_mean=False)
    np.testing.assert_array_equal(nomean, logp)
    assert np.all(untouched == 7.0)
    # the mean is the predict's; a predict and a sample after the call are what they were
    np.testing.assert_array_equal(mean, pred0[0])
    for a, b in zip(post._predict(t, True), pred0):
        np.testing.assert_array_equal(a, b)
    mean_s1, x1 = post.sample(t, k, SEED)
    np.testing.assert_array_equal(x1, x)
    np.testing.assert_array_equal(mean_s1, mean_s0)
    # a NaN (an Inf) in one row: that row NaN, its neighbours' bits alone, LFM_OK
    for poison, col in ((np.nan, 37), (np.inf, 0), (-np.inf, 96)):
        y3 = x[:3].copy()
        y3[1, col] = poison
        got, _ = logp_call(h, t, cadd, y3)
        assert np.isnan(got[1]), (poison, got)
        np.testing.assert_array_equal(got[[0, 2]], logp[[0, 2]])
    np.testing.assert_array_equal(logp_call(h, t, cadd, x)[0], logp)


# ------------------------------------------------------------------ 4. the shim
def test_posterior_log_prob_vs_host_route(fx, probs):
    worst = 0.0
    datas = c5_datas()
    for q in C_RESIDENT:
        x_, y_, v_, t, model = probs["c"][q]
        ys = fx["c_ystar"][q, 0]
        rtol, ref = float(fx["c_rtol"][q, 0]), float(fx["c_logp"][q, 0])
        post = model.posterior(datas[q % 15], "gene")
        try:
            assert post.status == 0
            got = post.log_prob(t, ys)
            host = post.predict(t).log_prob(ys)
            if q == C_RESIDENT[0]:
                both = post.log_prob(t, np.stack((ys, ys + 0.25)))
                assert isinstance(got, float) and both.shape == (2,) and both[0] == got
                assert both[1] != got and np.isfinite(both[1])
                wide = post.log_prob(t, fx["c_ystar"][q, 1], cov_add=model.obs_stddev ** 2)
                ref1 = float(fx["c_logp"][q, 1])
                assert abs(wide - ref1) <= rtol * max(1.0, abs(ref1))
        finally:
            post.close()
        bound = 2.0 * rtol * max(1.0, abs(ref))
        worst = max(worst, abs(got - host) / bound)
        assert abs(got - host) <= bound, (q, got, host, bound)
    print(f"Posterior.log_prob - predict(t).log_prob(y) at c round 15: worst |d| / (2 bound) = "
          f"{worst:.2e}")


# ------------------------------------------------------------------ 5. failures
def test_failures_leave_everything_usable(fx, probs):
    from dis_project_amd import _lib

    ctx = ctx0()
    lib, d = ctx.lib, _lib.dptr
    r = int(fx["npd_restart"])
    bad_t = np.ascontiguousarray(fx["npd_t"])
    p5 = probs["a"][r]
    cadd = cadds_of(p5[4])[0]
    ys = np.ascontiguousarray(np.stack((fx["a_ystar"][r, 0], fx["a_ystar"][r, 1])))

    def message():
        return lib.lfm_last_error(ctx.handle).decode()

    with Resident(p5) as post:
        good, gmean = logp_call(post.h, p5[3], cadd, ys)
        assert np.all(np.isfinite(good))
        # latent test rows: the joint covariance is indefinite
        assert bad_t.shape[0] == ys.shape[1]
        logp, mean = logp_call(post.h, bad_t, cadd, ys, expect=_lib.LFM_E_NOT_PD)
        assert np.all(np.isnan(logp)) and np.all(np.isnan(mean))
        again, amean = logp_call(post.h, p5[3], cadd, ys)
        np.testing.assert_array_equal(again, good)
        np.testing.assert_array_equal(amean, gmean)

        # argument violations, in the documented order: the word, and nothing written
        t = np.ascontiguousarray(p5[3])
        m, G = t.shape[0], p5[4].num_genes
        big_t = np.ascontiguousarray(np.tile(t, (7, 1)))  # 140 rows: above a chunk of 128
        assert big_t.shape[0] % G == 0 and big_t.shape[0] > 128
        big_y = np.zeros((2, big_t.shape[0]))
        mean, logp = np.full(big_t.shape[0], 7.0), np.full(2, 7.0)
        h = post.h

        def call(c, p, tt, mm, yy, kk, lp=logp):
            return lib.lfm_post_log_prob_f64(c, p, d(tt) if tt is not None else None, mm, cadd,
                                             d(yy) if yy is not None else None, kk, d(mean),
                                             d(lp) if lp is not None else None)

        assert call(None, h, t, m, ys, 2) == _lib.LFM_E_ARG
        for args, word in (((ctx.handle, None, t, m, ys, 2), "post"),
                           ((ctx.handle, h, None, m, ys, 2), "NULL"),
                           ((ctx.handle, h, t, m, None, 2), "NULL"),
                           ((ctx.handle, h, t, m, ys, 2, None), "NULL"),
                           ((ctx.handle, h, t, 0, ys, 2), "num_genes"),
                           ((ctx.handle, h, t, m - 1, ys, 2), "num_genes"),
                           ((ctx.handle, h, t, m, ys, 0), "k must be"),
                           ((ctx.handle, h, t, m, ys, -2), "k must be"),
                           ((ctx.handle, h, t, m, ys, 2 ** 24 + 1), "split")):
            assert call(*args) == _lib.LFM_E_ARG, args[3:]
            assert word in message(), (word, message())
        assert (m - 1) % G != 0
        # m above the chunk names the limit, and comes before k
        assert lib.lfm_post_set_chunk(h, 128) == 0
        try:
            assert call(ctx.handle, h, big_t, big_t.shape[0], big_y, 0) == _lib.LFM_E_ARG
            assert "128" in message() and "chunk" in message()
        finally:
            assert lib.lfm_post_set_chunk(h, 0) == 0
        if _lib.device_count() > 1:
            other = _lib.get_context(1)
            assert call(other.handle, h, t, m, ys, 2) == _lib.LFM_E_ARG
            assert "another device" in other.lib.lfm_last_error(other.handle).decode()
        assert np.all(mean == 7.0) and np.all(logp == 7.0)
        final, fmean = logp_call(post.h, p5[3], cadd, ys)
        np.testing.assert_array_equal(final, good)
        np.testing.assert_array_equal(fmean, gmean)
    print("not PD and ten argument violations refused; the handle returned its earlier bits after "
          "each")

"""The posterior predictors against extended-precision truth at C3's restarts and C5's rounds.

tests/test_gpu_predict.py and test_gpu_batch_predict.py compare with oracle/lfm_oracle.py at
benign hyperparameters (cond(Sigma) <= 4e2). At the restarts' hyperparameters that oracle is off
by up to 2e-1 of the covariance (tests/test_exact_posterior.py), and the covariance
K(t,t) - K(t,x) S^{-1} K(x,t) is a cancellation of its own. Here the reference is
tests/golden/exact_posterior.npz (oracle/lfm_exact.posterior_exact: 60-digit entries carried in
long double, a long double Cholesky; make_golden_exact_posterior.py) and the bound is the
predictors' own with the fixture's per-case post_rtol,

    max|d| <= post_rtol * max|truth| + 1e-12    for the mean, the variance and the covariance,

post_rtol = 1e-9 wherever fp64 LAPACK on correctly rounded entries is 8 x better than that, which
is every case here (worst 1.3e-12).

  * a: n = 28 (the first C5 problem's data), all 32 restarts' 4-gene sub-models, both diagonals
    (latent_predict's jitter, multi_gene_predict's obs_stddev^2), m = 20 test rows of every flag
    pairing, t = 0 rows, a time past the data, gene indices -1 and G: through lfm_posterior_f64,
    as one lfm_batch_posterior_f64 batch of 32, and (restarts 5, 29) through ExactLFM.
  * b: n = 129, m = 45 (two block columns, a ragged edge) at restarts 0, 7, 13, 19, 29 through
    lfm_posterior_f64. chol_factor_solve keeps the Schur-complement posterior on schedule 1
    whatever the context's schedule is (lfm_chol_sched.hip: s3 = s3_on(ctx) && mode !=
    CHOL_SCHUR), so there is no LFM_SCHED=1 variant to run; the test asserts the schedule used.
  * c: the 15 C5 problems at rounds 0, 7, 15 through predict.BatchPredictor, one batch of 45 per
    predictor, the shim's jitter assembly included.
  * the entries behind a and b through the direct gram (cross_covariance of scattered copies)
    and, n = 28 at restarts 13 and 19, the small kernel's table path (lfm_probe_kxx_tab), held to
    k_direct eps M: M the magnitude of the terms of the cancellation-free form, which does not
    grow with the reference order's cancellation, k_direct 4 x what a numpy restatement needs.

Everything comes from the .npz files; mpmath is not needed here.
"""

import ctypes

import numpy as np
import pytest

from oracle import lfm_exact as E
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
B_RESTARTS = (0, 7, 13, 19, 29)
C_ROUNDS = (0, 7, 15)


@pytest.fixture(scope="module")
def fx():
    g = load_golden("exact_posterior")
    g.update(load_golden("exact_posterior_c5cov"))
    assert tuple(int(r) for r in g["b_restarts"]) == B_RESTARTS
    assert tuple(int(r) for r in g["c_rounds"]) == C_ROUNDS
    return g


@pytest.fixture(scope="module")
def restarts():
    from dis_project_amd import configs

    return configs.c3_restarts(configs.c2(), 32)


def c5_datas():
    from dis_project_amd import dataset as ds

    return [ds.SyntheticP53Data(replicate=0, seed=seed,
                                selected_genes=[g for g in ds.BARENCO_GENES if g != drop])
            for seed in (10, 11, 12) for drop in ds.BARENCO_GENES]


def full_of(tril, m):
    out = np.empty((m, m))
    ii, jj = np.tril_indices(m)
    out[ii, jj] = tril
    out[jj, ii] = tril
    return out


def ratio(got, ref, rtol):
    """max|d| / (rtol max|truth| + 1e-12): at most 1 for a right answer."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape
    with np.errstate(invalid="ignore"):
        d = float(np.nan_to_num(np.max(np.abs(got - ref)), nan=np.inf))
    return d / (rtol * float(np.max(np.abs(ref))) + 1e-12)


def posterior_call(ctx, x, y, v, dadd, t, model):
    """lfm_posterior_f64 -> (rc, mean, cov)."""
    from dis_project_amd import _lib

    m = t.shape[0]
    mean, cov = np.full(m, 7.0), np.full((m, m), 7.0)
    rc = ctx.lib.lfm_posterior_f64(ctx.handle, _lib.dptr(x), _lib.dptr(y), x.shape[0],
                                   _lib.dptr(v), float(dadd), _lib.dptr(t), m, model.hyp().ref,
                                   _lib.dptr(mean), _lib.dptr(cov))
    if rc not in (_lib.LFM_OK, _lib.LFM_E_NOT_PD):
        ctx.check(rc)
    return rc, mean, cov


def dadd_of(model, kind):
    return model.jitter if kind == 0 else model.obs_stddev ** 2


def check_group(fx, pre, ctx, models, labels, x, y, v, t):
    """Every case of group `pre` through lfm_posterior_f64; prints the worst ratio per restart."""
    from dis_project_amd import _lib

    m = t.shape[0]
    bad = []
    for q, (r, model) in enumerate(zip(labels, models)):
        figs = []
        for kind in (0, 1):
            rc, mean, cov = posterior_call(ctx, x, y, v, dadd_of(model, kind), t, model)
            if fx[pre + "_not_pd"][q, kind]:
                assert rc == _lib.LFM_E_NOT_PD and np.all(np.isnan(mean)) and np.all(np.isnan(cov))
                continue
            assert rc == 0, (r, kind, rc)
            if fx[pre + "_dropped"][q, kind]:
                continue
            np.testing.assert_array_equal(cov, cov.T)
            rtol = float(fx[pre + "_rtol"][q, kind])
            figs += [ratio(mean, fx[pre + "_mean"][q, kind], rtol),
                     ratio(cov, full_of(fx[pre + "_cov"][q, kind], m), rtol)]
        orc, la = fx[pre + "_oracle_err"][q], fx[pre + "_lapack_err"][q]
        print(f"{pre} r{r}: device |d| / bound mean, cov (latent diag | gene diag) = "
              + " ".join(f"{f:.2e}" for f in figs)
              + f"; relative errors mean, cov: lapack {np.nanmax(la[:, 0]):.1e} {np.nanmax(la[:, 1]):.1e}"
              f" oracle {np.nanmax(orc[:, 0]):.1e} {np.nanmax(orc[:, 1]):.1e}")
        if figs and not max(figs) <= 1.0:
            bad.append((r, [round(f, 3) for f in figs]))
    assert not bad, bad


def test_a_all_restarts_single(fx, restarts):
    """a through lfm_posterior_f64: 64 calls, mean and full covariance inside each case's bound,
    the covariance exactly symmetric."""
    from dis_project_amd import _lib

    assert np.sum(np.any(fx["a_dropped"], axis=1)) <= 2
    models = [E.submodel(m, 4)[0] for m in restarts]
    check_group(fx, "a", _lib.get_context(0), models, range(32), fx["a_x"], fx["a_y"], fx["a_v"],
                fx["a_t"])


def test_a_all_restarts_one_batch(fx, restarts):
    """a through lfm_batch_posterior_f64: the same data registered 32 times, one problem per
    restart; one call without cov (the latent diagonal), one with (the gene diagonal), var equal
    to diag(cov) bit for bit. A problem that is not PD in exact arithmetic carries its status and
    NaNs while the others are judged as usual."""
    from dis_project_amd import _lib, dataset as ds, farm, predict as P

    ctx = _lib.get_context(0)
    models = [E.submodel(m, 4)[0] for m in restarts]
    x, y, v, t = fx["a_x"], fx["a_y"], fx["a_v"], fx["a_t"]
    ev = farm.BatchEvaluator(ctx, [ds.Dataset(x, y.reshape(-1, 1))] * 32)
    bad = []
    try:
        hyp = ev.pack(models)
        tt, mm = P.pack_test_inputs([t] * 32, [4] * 32)
        dv = np.ascontiguousarray(np.tile(v, 32))
        for kind, want_cov in ((0, False), (1, True)):
            dadd = np.array([dadd_of(m, kind) for m in models])
            mean, var = np.full(int(mm.sum()), 7.0), np.full(int(mm.sum()), 7.0)
            cov = np.full(int((mm * mm).sum()), 7.0) if want_cov else None
            st = np.full(32, -9, np.int32)
            rc = ctx.lib.lfm_batch_posterior_f64(
                ctx.handle, ev.batch, _lib.dptr(hyp), _lib.dptr(dv), _lib.dptr(dadd),
                _lib.dptr(mm), _lib.dptr(tt), _lib.dptr(mean), _lib.dptr(var),
                _lib.dptr(cov) if want_cov else None, _lib.dptr(st))
            not_pd = fx["a_not_pd"][:, kind]
            assert rc == (_lib.LFM_E_NOT_PD if np.any(not_pd) else 0), rc
            assert np.array_equal(st, np.where(not_pd, _lib.LFM_E_NOT_PD, 0)), st
            worst = 0.0
            for r, (mean_r, var_r, cov_r) in enumerate(P.unpack_outputs(mm, mean, var, cov)):
                if not_pd[r]:
                    assert np.all(np.isnan(mean_r)) and np.all(np.isnan(var_r))
                    continue
                if fx["a_dropped"][r, kind]:
                    continue
                rtol = float(fx["a_rtol"][r, kind])
                ref = full_of(fx["a_cov"][r, kind], 20)
                figs = [ratio(mean_r, fx["a_mean"][r, kind], rtol),
                        ratio(var_r, np.diagonal(ref), rtol)]
                if want_cov:
                    np.testing.assert_array_equal(var_r, np.diagonal(cov_r))
                    np.testing.assert_array_equal(cov_r, cov_r.T)
                    figs.append(ratio(cov_r, ref, rtol))
                worst = max(worst, max(figs))
                if not max(figs) <= 1.0:
                    bad.append((r, kind, [round(f, 3) for f in figs]))
            print(f"a batch, {'gene' if kind else 'latent'} diagonal: worst |d| / bound = {worst:.3e}")
    finally:
        ev.close()
    assert not bad, bad


def test_a_through_exactlfm(fx, restarts):
    """Restarts 5 and 29 of a through ExactLFM.latent_predict / multi_gene_predict: the jitter
    assembly scale = diag(var + jitter) + jitter I, and cov + jitter I."""
    data = c5_datas()[0]
    t = fx["a_t"]
    for r in (5, 29):
        model = E.submodel(restarts[r], 4)[0]
        assert not np.any(fx["a_not_pd"][r]) and not np.any(fx["a_dropped"][r])
        jit = model.jitter
        lat = model.latent_predict(t, data)
        ref = full_of(fx["a_cov"][r, 0], 20)
        want = np.diag(np.diagonal(ref) + jit) + np.eye(20) * jit
        figs = [ratio(lat.loc, fx["a_mean"][r, 0], float(fx["a_rtol"][r, 0])),
                ratio(lat.scale, want, float(fx["a_rtol"][r, 0]))]
        gene = model.multi_gene_predict(t, data)
        want = full_of(fx["a_cov"][r, 1], 20) + np.eye(20) * jit
        figs += [ratio(gene.loc, fx["a_mean"][r, 1], float(fx["a_rtol"][r, 1])),
                 ratio(gene.scale, want, float(fx["a_rtol"][r, 1]))]
        print(f"ExactLFM r{r}: |d| / bound latent mean, scale, gene mean, scale = "
              + " ".join(f"{f:.2e}" for f in figs))
        assert max(figs) <= 1.0, (r, figs)


def test_b_blocked_ragged(fx, restarts):
    """b through lfm_posterior_f64 (n = 129: two block columns, a ragged edge; m = 45). The
    posterior's factorisation runs schedule 1 under every context schedule (asserted), so one
    run covers it."""
    from dis_project_amd import _lib

    ctx = _lib.get_context(0)
    models = [E.submodel(restarts[r], 3)[0] for r in B_RESTARTS]
    assert not np.any(fx["b_dropped"])
    check_group(fx, "b", ctx, models, B_RESTARTS, fx["b_x"], fx["b_y"], fx["b_v"], fx["b_t"])
    used = ctypes.c_int(-1)
    ctx.check(ctx.diag.lfm_debug_last_schedule(ctx.handle, ctypes.byref(used)))
    assert used.value == 1


def test_c_rounds_through_batchpredictor(fx):
    """c: the 15 C5 problems at rounds 0, 7 and 15 as one batch of 45 per predictor through
    predict.BatchPredictor: marginals(..., "latent") at generate_test_times(100) and
    multi_gene_predict at generate_test_times_pred(20, 4), the shim's jitter assembly included."""
    from dis_project_amd import configs, dataset as ds
    from dis_project_amd.predict import BatchPredictor

    works = configs.c5_ablations()
    allm = configs.c5_rounds([w.model for w in works], 16)
    models = [allm[15 * k + p] for k in C_ROUNDS for p in range(15)]
    t_lat, t_gene = ds.generate_test_times(100), ds.generate_test_times_pred(20, 4)
    bp = BatchPredictor(c5_datas() * 3)
    try:
        lat = bp.marginals(models, t_lat, "latent")
        assert not np.any(bp.status)
        gene = bp.multi_gene_predict(models, t_gene)
        assert not np.any(bp.status)
    finally:
        bp.close()
    u = fx["c_unique"]
    worst, bad = np.zeros(4), []
    for q, model in enumerate(models):
        jit = model.jitter
        rl, rg = float(fx["c_lat_rtol"][q]), float(fx["c_gene_rtol"][q])
        cov = full_of(fx["c_gene_cov"][q], 60)[np.ix_(u, u)]
        figs = np.array([ratio(lat[q][0], fx["c_lat_mean"][q], rl),
                         ratio(lat[q][1], (fx["c_lat_var"][q] + jit) + jit, rl),
                         ratio(gene[q].loc, fx["c_gene_mean"][q], rg),
                         ratio(gene[q].scale, cov + np.eye(80) * jit, rg)])
        worst = np.maximum(worst, figs)
        if not figs.max() <= 1.0:
            bad.append((q, figs.round(3).tolist()))
    print("c: worst |d| / bound latent mean, latent variance, gene mean, gene covariance = "
          + " ".join(f"{f:.2e}" for f in worst)
          + f"; oracle's worst relative error {max(fx['c_lat_oracle_err'].max(), fx['c_gene_oracle_err'].max()):.1e}")
    assert not bad, bad


# --------------------------------------------------------------- entry level
def entry_pairs(x, t, with_xx):
    """The rows behind ent_*_k: K(t,x) row-major, tril K(t,t) and, with_xx, tril K(x,x)."""
    m, n = len(t), len(x)
    ia, ib = np.divmod(np.arange(m * n), n)
    A, Bm = [t[ia]], [x[ib]]
    ii, jj = np.tril_indices(m)
    A.append(t[ii])
    Bm.append(t[jj])
    if with_xx:
        ii, jj = np.tril_indices(n)
        A.append(x[ii])
        Bm.append(x[jj])
    return np.concatenate(A), np.concatenate(Bm)


def entry_ratio(fx, got, val, rel):
    """|got - truth| / (k_direct eps M), M = rel |truth|; where the truth is 0 (a gene row at
    t = 0) the entry must be exactly 0."""
    assert np.all(got[val == 0] == 0.0)
    M = rel.astype(np.float64) * np.abs(val)
    live = val != 0
    assert np.all(M[live] > 0)
    out = np.zeros(val.shape)
    with np.errstate(invalid="ignore"):
        out[live] = np.nan_to_num(np.abs(got[live] - val[live]), nan=np.inf) / (
            float(fx["k_direct"]) * EPS * M[live])
    return out


def flags_of(xa, xb):
    return (xa[:, 2] != 0).astype(int) * 2 + (xb[:, 2] != 0).astype(int)  # ff, fx, xf, xx


def test_direct_entries_vs_truth_all_flag_pairings(fx, restarts):
    """The direct gram (kernel_ref: h_ref, kxf_ref, kff_ref) on the entries behind a (all 32
    restarts) and b, gene / gene, gene / latent on either side and latent / latent: every entry
    within k_direct eps M of the truth. This is the test that names the cause when a posterior
    above is off: its bound does not grow with the reference order's cancellation, unlike
    test_direct_path_vs_truth's 16 eps gram_error_scale."""
    k = float(fx["k_direct"])
    xa, xb = entry_pairs(fx["a_x"], fx["a_t"], True)
    kinds = flags_of(xa, xb)
    assert set(kinds.tolist()) == {0, 1, 2, 3}
    bad, worst = [], np.zeros(4)
    for r in range(32):
        model = E.submodel(restarts[r], 4)[0]
        K = model.cross_covariance(model.kernel, xa, xb)
        rr = entry_ratio(fx, K.diagonal(), fx["ent_a_k"][r], fx["ent_a_r"][r])
        per = np.array([rr[kinds == c].max() for c in range(4)])
        worst = np.maximum(worst, per)
        i = int(rr.argmax())
        print(f"direct a r{r}: worst |dK| / (k eps M) ff, fx, xf, xx = "
              + " ".join(f"{f:.2e}" for f in per) + f" (worst pair {xa[i].tolist()} {xb[i].tolist()},"
              f" |dK| = {abs(K[i, i] - fx['ent_a_k'][r][i]):.2e})")
        if not rr.max() <= 1.0:
            bad.append(("a", r, round(float(rr.max()), 2)))
    xa, xb = entry_pairs(fx["b_x"], fx["b_t"], False)
    xa, xb = xa[fx["b_pick"]], xb[fx["b_pick"]]
    for q, r in enumerate(B_RESTARTS):
        model = E.submodel(restarts[r], 3)[0]
        K = model.cross_covariance(model.kernel, xa, xb)
        rr = entry_ratio(fx, K.diagonal(), fx["ent_b_k"][q], fx["ent_b_r"][q])
        print(f"direct b r{r}: worst |dK| / (k eps M) = {rr.max():.2e}")
        if not rr.max() <= 1.0:
            bad.append(("b", r, round(float(rr.max()), 2)))
    print(f"direct: worst |dK| / (k_direct eps M) ff, fx, xf, xx = "
          + " ".join(f"{f:.2e}" for f in worst) + f" (k_direct = {k:.1f})")
    assert not bad, bad


def test_small_table_entries_vs_truth(fx, restarts):
    """The small kernel's table path (kxx_tab) and kernel_ref beside it (lfm_probe_kxx_tab) on
    all 406 lower entries of a's K(x,x) at restarts 13 and 19, under the same bound."""
    from dis_project_amd import _lib

    ctx = _lib.get_context(0)
    x = np.ascontiguousarray(fx["a_x"])
    ii, jj = np.tril_indices(28)
    off = 20 * 28 + 20 * 21 // 2  # tril K(x,x) follows K(t,x) and tril K(t,t) in ent_a_*
    bad = []
    for r in (13, 19):
        model = E.submodel(restarts[r], 4)[0]
        out = np.empty(2 * 28 * 28)
        ctx.check(ctx.diag.lfm_probe_kxx_tab(ctx.handle, _lib.dptr(x), 28, model.hyp().ref,
                                             _lib.dptr(out)))
        np.testing.assert_array_equal(out[:784], out[784:])
        rr = entry_ratio(fx, out[:784].reshape(28, 28)[ii, jj], fx["ent_a_k"][r][off:],
                         fx["ent_a_r"][r][off:])
        print(f"kxx_tab r{r}: worst |dK| / (k eps M) = {rr.max():.2e}")
        if not rr.max() <= 1.0:
            bad.append((r, round(float(rr.max()), 2)))
    assert not bad, bad

"""Joint samples and held-out log density of the multi_gene_predict distribution,
N(mean, cov + cov_add I), against extended-precision truth at C3's restarts and C5's rounds.

tests/test_gpu_mid_draw.py and test_gpu_sample.py take their reference mean and covariance from
the handle's own posterior call at benign hyperparameters (l = 1.8, kappa about 5) and bound the
difference by 50 kappa m eps, so an error in the covariance tiles, the copy into the padded matrix
or the addition on the diagonal moves reference and result together, and the log-determinant and
quadratic term are only seen as their sum. Here the reference is tests/golden/exact_predictive.npz
(oracle/lfm_exact.predictive_exact end to end in long double; make_golden_exact_predictive.py;
tests/test_exact_predictive.py holds it on the CPU) and the bounds are the fixture's,

    |logp - truth|      <= rtol max(1, |truth|)
    max|X - truth X|    <= rtol max|truth X| + 1e-12
    max|mean - truth|   <= rtol max|truth| + 1e-12        (test_gpu_exact_posterior's form)

with rtol = 1e-9 in every case (fp64 LAPACK on the rounded entries is within 5.4e-12). The truth
samples use the normals of tests/philox_ref.py; the device generator is held to them at 1e-13
absolute (test_gpu_sample.py), which through L with m <= 129 moves a sample by at most
sqrt(m scale_ii) 1e-13 < 1.2e-12 sqrt(scale_ii), below 1e-11 of max|X|: inside the bounds.

All test rows are gene rows, diag_add = obs_stddev^2; cov_add index 0 = jitter, 1 = obs_stddev^2.
Every draw is one call of nsamp = 130 at sample0 = 0, of which rows 0, 63, 64, 65 and 129 are
compared: the 64-row edges and the 128-row tile edge of the product.

  * a (n = 28, m = 20 with four t = 0 rows and a repeated block, all 32 restarts), b (n = 129 at
    restarts 0, 7, 13, 19, 29; m = 129: m + 1 = 130 rows, the residual row two rows into a third
    block column; m = 63: the residual row closes a block) and c (the 45 C5 problems, m = 80 with
    20 exactly repeated rows) through
      - the mid batch: lfm_mbatch_predictive_f64, logp and samples from one call (c through
        predict.MidBatchPredictor.sample / .log_prob), both cov_add values;
      - the host route: lfm_posterior_f64 -> one addition on the diagonal -> lfm_mvn_sample_f64 /
        lfm_log_prob_f64 (c: ExactLFM.multi_gene_predict(...).sample / .log_prob, cov_add 0);
      - the resident path: lfm_post_create + lfm_post_sample_f64 at cov_add 0 (c: round 15),
        which must also equal lfm_mvn_sample_f64 fed the handle's lfm_post_predict_f64 mean and
        cov + cov_add I bit for bit (include/lfm.h), here at the restarts.
  * mixed sizes in one mid handle: the bits of the homogeneous batches.
  * a's restart 5 with latent test rows (the truth scale's smallest eigenvalue is -0.96):
    LFM_E_NOT_PD and NaN on all three paths, which stay usable.
  * at the ill-conditioned restarts a line with the mid result's and the host route's distance
    from the truth in units of the bound: one path far off points at its factor or product, both
    at the covariance.

Every homogeneous batch is evaluated once per module (the fixture `runs`), its handle closed as
soon as the results are on the host; the tests judge them and print their worst |d| / bound.
"""

import ctypes

import numpy as np
import pytest

from oracle import lfm_exact as E
from tests.conftest import load_golden
from tests.test_gpu_exact_posterior import B_RESTARTS, C_ROUNDS, c5_datas, posterior_call, ratio

pytestmark = pytest.mark.gpu

ILL = (1, 5, 10, 29)
SAMPLES = (0, 63, 64, 65, 129)
NSAMP = 130
A_MIXED = (5, 29)
B_MIXED = 4       # index of restart 29 in B_RESTARTS
C5_MIXED = 15     # the first C5 problems (round 0) in the mixed-size handle
GROUPS = ("a", "b129", "b63", "c")


@pytest.fixture(scope="module")
def fx():
    g = load_golden("exact_predictive")
    assert tuple(int(r) for r in g["b_restarts"]) == B_RESTARTS
    assert tuple(int(r) for r in g["c_rounds"]) == C_ROUNDS
    assert tuple(int(s) for s in g["samples"]) == SAMPLES and B_RESTARTS[B_MIXED] == 29
    for pre in GROUPS:
        assert np.all(g[pre + "_rtol"] == 1e-9)  # nothing dropped, nothing widened
    return g


def ctx0():
    from dis_project_amd import _lib

    return _lib.get_context(0)


def cadds_of(model):
    return (model.jitter, model.obs_stddev ** 2)


# ------------------------------------------------------------------ problems
def problems(fx):
    """{group: [(x, y, v, t, model)]} in fixture order."""
    from dis_project_amd import configs, dataset as ds

    restarts = configs.c3_restarts(configs.c2(), 32)
    a = [(fx["a_x"], fx["a_y"], fx["a_v"], fx["a_t"], E.submodel(m, 4)[0]) for m in restarts]
    b = {m: [(fx["b_x"], fx["b_y"], fx["b_v"], np.ascontiguousarray(fx["b_t"][:m]),
              E.submodel(restarts[r], 3)[0]) for r in B_RESTARTS] for m in (129, 63)}
    works = configs.c5_ablations()
    allm = configs.c5_rounds([w.model for w in works], 16)
    c = []
    for k in C_ROUNDS:
        for p, data in enumerate(c5_datas()):
            x, y, v = ds.dataset_3d(data)
            c.append((np.ascontiguousarray(x, dtype=np.float64).reshape(-1, 3),
                      np.ascontiguousarray(y, dtype=np.float64).reshape(-1),
                      np.ascontiguousarray(v, dtype=np.float64).reshape(-1), fx["c_t"],
                      allm[15 * k + p]))
    return {"a": a, "b129": b[129], "b63": b[63], "c": c}


# ------------------------------------------------------------------ the three paths
def mid_predictive(probs, kind, ystars, seeds, ts=None):
    """One farm.MidBatchEvaluator over `probs` and one lfm_mbatch_predictive_f64 (logp and
    samples together) -> (rc, [(mean, logp, X[SAMPLES])], statuses). kind: the cov_add index, or
    a list of them for several calls on the one handle (then a list of such triples)."""
    import dis_project_amd as lfm
    from dis_project_amd import _lib, farm, predict as P

    ctx = ctx0()
    models = [p[4] for p in probs]
    ev = farm.MidBatchEvaluator(ctx, [lfm.Dataset(np.ascontiguousarray(p[0]), p[1].reshape(-1, 1))
                                      for p in probs])
    try:
        ev._pack(models)
        hyp = ev._buf.copy()
        dv = np.ascontiguousarray(np.concatenate([p[2] for p in probs]))
        dadd = np.array([m.obs_stddev ** 2 for m in models])
        sd = np.ascontiguousarray(seeds, dtype=np.uint64)
        out = []
        for call, k in enumerate(np.atleast_1d(kind)):
            tl = [p[3] for p in probs] if ts is None else ts[call]
            tt, mm = P.pack_test_inputs(tl, [m.num_genes for m in models])
            sm = int(mm.sum())
            cadd = np.array([cadds_of(m)[k] for m in models])
            ys = np.ascontiguousarray(np.concatenate([y[k] for y in ystars]))
            logp, mean, smp = np.full(len(probs), 7.0), np.full(sm, 7.0), np.full(NSAMP * sm, 7.0)
            st = np.full(len(probs), -9, np.int32)
            rc = ctx.lib.lfm_mbatch_predictive_f64(
                ctx.handle, ev.batch, _lib.dptr(hyp), _lib.dptr(dv), _lib.dptr(dadd),
                _lib.dptr(mm), _lib.dptr(tt), _lib.dptr(cadd), _lib.dptr(ys), _lib.dptr(logp),
                _lib.dptr(sd), 0, NSAMP, _lib.dptr(mean), _lib.dptr(smp), _lib.dptr(st))
            res, o = [], 0
            for q, m in enumerate(int(v) for v in mm):
                X = smp[NSAMP * o:NSAMP * (o + m)].reshape(NSAMP, m)
                res.append((mean[o:o + m].copy(), float(logp[q]), X[list(SAMPLES)].copy()))
                o += m
            out.append((rc, res, st))
        return out if np.ndim(kind) else out[0]
    finally:
        ev.close()


def host_route(p, kind, ystar, seed, t=None):
    """lfm_posterior_f64 -> cov + cov_add on the diagonal -> lfm_mvn_sample_f64 and
    lfm_log_prob_f64 -> (rc's, (mean, logp, X[SAMPLES]))."""
    from dis_project_amd import _lib

    ctx = ctx0()
    x, y, v, t0, model = p
    t = np.ascontiguousarray(t0 if t is None else t)
    m = t.shape[0]
    rc0, mean, cov = posterior_call(ctx, np.ascontiguousarray(x), y, v, model.obs_stddev ** 2, t,
                                    model)
    scale = cov.copy()
    scale[np.diag_indices(m)] += cadds_of(model)[kind]
    X, logp = np.full((NSAMP, m), 7.0), np.full(1, 7.0)
    rc1 = ctx.lib.lfm_mvn_sample_f64(ctx.handle, _lib.dptr(mean), _lib.dptr(scale), m, m,
                                     int(seed), 0, NSAMP, _lib.dptr(X))
    rc2 = ctx.lib.lfm_log_prob_f64(ctx.handle, _lib.dptr(mean), _lib.dptr(scale), m, m,
                                   _lib.dptr(np.ascontiguousarray(ystar)), _lib.dptr(logp))
    return (rc0, rc1, rc2), (mean, float(logp[0]), X[list(SAMPLES)].copy())


class Resident:
    """lfm_post_create at diag_add = obs_stddev^2, closed by the with-block."""

    def __init__(self, p):
        from dis_project_amd import _lib

        self.ctx = ctx0()
        x, y, v, _, model = p
        self.h = ctypes.c_void_p()
        self.ctx.check(self.ctx.lib.lfm_post_create(
            self.ctx.handle, _lib.dptr(np.ascontiguousarray(x)), _lib.dptr(y), x.shape[0],
            _lib.dptr(v), model.obs_stddev ** 2, model.hyp().ref, ctypes.byref(self.h)))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.lib.lfm_post_destroy(self.h)

    def sample(self, t, cadd, seed):
        """lfm_post_sample_f64 -> (rc, mean, X [NSAMP, m])."""
        from dis_project_amd import _lib

        t = np.ascontiguousarray(t)
        m = t.shape[0]
        mean, X = np.full(m, 7.0), np.full((NSAMP, m), 7.0)
        rc = self.ctx.lib.lfm_post_sample_f64(self.ctx.handle, self.h, _lib.dptr(t), m,
                                              float(cadd), int(seed), 0, NSAMP, _lib.dptr(mean),
                                              _lib.dptr(X))
        return rc, mean, X

    def via_predict(self, t, cadd, seed):
        """lfm_mvn_sample_f64 fed this handle's lfm_post_predict_f64 mean and cov + cadd I."""
        from dis_project_amd import _lib

        t = np.ascontiguousarray(t)
        m = t.shape[0]
        mean, var, cov = np.full(m, 7.0), np.full(m, 7.0), np.full((m, m), 7.0)
        self.ctx.check(self.ctx.lib.lfm_post_predict_f64(
            self.ctx.handle, self.h, _lib.dptr(t), m, _lib.dptr(mean), _lib.dptr(var),
            _lib.dptr(cov)))
        cov[np.diag_indices(m)] += cadd
        X = np.full((NSAMP, m), 7.0)
        self.ctx.check(self.ctx.lib.lfm_mvn_sample_f64(
            self.ctx.handle, _lib.dptr(mean), _lib.dptr(cov), m, m, int(seed), 0, NSAMP,
            _lib.dptr(X)))
        return mean, X


class Runs:
    """Each path's results on each group, evaluated once and then left unchanged."""

    def __init__(self, fx):
        self.fx = fx
        self.probs = problems(fx)
        self._mid, self._host, self._res = {}, {}, {}

    def ystars(self, pre, qs=None):
        ys = self.fx[pre + "_ystar"]
        return [ys[q] for q in (range(len(ys)) if qs is None else qs)]

    def mid(self, pre):
        """[kind] -> (rc, [(mean, logp, X)], statuses)."""
        if pre not in self._mid:
            probs, seeds = self.probs[pre], self.fx[pre + "_seed"]
            if pre == "c":
                self._mid[pre] = self._mid_c(probs, seeds)
            else:
                self._mid[pre] = mid_predictive(probs, [0, 1], self.ystars(pre), seeds)
        return self._mid[pre]

    def _mid_c(self, probs, seeds):
        from dis_project_amd.predict import MidBatchPredictor

        models = [p[4] for p in probs]
        bp = MidBatchPredictor(c5_datas() * 3)
        out = []
        try:
            for k in (0, 1):
                cadd = [cadds_of(m)[k] for m in models]
                lp = bp.log_prob(models, self.fx["c_t"], [y[k] for y in self.ystars("c")],
                                 cov_add=cadd)
                st = bp.status.copy()
                drawn = bp.sample(models, self.fx["c_t"], NSAMP, 0, cov_add=cadd,
                                  seeds=[int(s) for s in seeds])
                st = np.maximum(st, bp.status)
                out.append((int(st.max()), [(mean, float(lp[q]), X[list(SAMPLES)].copy())
                                            for q, (mean, X) in enumerate(drawn)], st))
        finally:
            bp.close()
        return out

    def host(self, pre):
        """[kind][q] -> (mean, logp, X); c: the ExactLFM shim, cov_add 0 alone."""
        if pre not in self._host:
            probs, seeds, ys = self.probs[pre], self.fx[pre + "_seed"], self.fx[pre + "_ystar"]
            out = []
            for k in ((0,) if pre == "c" else (0, 1)):
                row = []
                for q, p in enumerate(probs):
                    if pre == "c":
                        dist = p[4].multi_gene_predict(p[3], c5_datas()[q % 15])
                        X = dist.sample(int(seeds[q]), (NSAMP,))
                        row.append((np.asarray(dist.loc), dist.log_prob(ys[q, k]),
                                    X[list(SAMPLES)].copy()))
                    else:
                        rcs, got = host_route(p, k, ys[q, k], seeds[q])
                        assert rcs == (0, 0, 0), (pre, q, k, rcs)
                        row.append(got)
                out.append(row)
            self._host[pre] = out
        return self._host[pre]

    def resident(self, pre):
        """[q] -> (mean, X [NSAMP, m], the same through lfm_post_predict_f64) at cov_add 0; c: the
        round-15 problems (q = 30..44) alone, None elsewhere."""
        if pre not in self._res:
            out = []
            for q, p in enumerate(self.probs[pre]):
                if pre == "c" and q < 30:
                    out.append(None)
                    continue
                seed, cadd = self.fx[pre + "_seed"][q], cadds_of(p[4])[0]
                with Resident(p) as post:
                    rc, mean, X = post.sample(p[3], cadd, seed)
                    assert rc == 0, (pre, q, rc)
                    out.append((mean, X, post.via_predict(p[3], cadd, seed)))
            self._res[pre] = out
        return self._res[pre]


@pytest.fixture(scope="module")
def runs(fx):
    return Runs(fx)


# ------------------------------------------------------------------ judging
def figures(fx, pre, q, kind, got):
    """|d| / bound of (mean, logp, samples) of case (q, kind) of group `pre`."""
    mean, logp, X = got
    rtol = float(fx[pre + "_rtol"][q, kind])
    ref = float(fx[pre + "_logp"][q, kind])
    d = abs(logp - ref)
    return np.array([ratio(mean, fx[pre + "_mean"][q, kind], rtol),
                     (d if np.isfinite(d) else np.inf) / (rtol * max(1.0, abs(ref))),
                     ratio(X, fx[pre + "_smp"][q, kind], rtol)])


def labels_of(pre):
    if pre == "a":
        return [f"a r{r}" for r in range(32)]
    if pre == "c":
        return [f"c round {C_ROUNDS[q // 15]} problem {q % 15}" for q in range(45)]
    return [f"{pre} r{r}" for r in B_RESTARTS]


def judge(fx, pre, path, results, kinds=(0, 1), qs=None, verbose=None):
    """results[kind][q] -> (mean, logp, X): prints the group's worst figures (and each case of
    `verbose`), returns what is outside its bound."""
    labels = labels_of(pre)
    qs = range(len(labels)) if qs is None else qs
    bad, worst, where = [], np.zeros(3), [None] * 3
    for kind in kinds:
        for q in qs:
            figs = figures(fx, pre, q, kind, results[kind][q])
            if verbose is not None and q in verbose:
                print(f"{path} {labels[q]} cov_add {kind}: |d| / bound mean, logp, samples = "
                      + " ".join(f"{f:.2e}" for f in figs))
            for k in range(3):
                if not figs[k] <= worst[k]:
                    worst[k], where[k] = figs[k], (labels[q], kind)
            if not figs.max() <= 1.0:
                bad.append((path, labels[q], kind, [float(f"{f:.3g}") for f in figs]))
    print(f"{path} {pre}: worst |d| / bound mean, logp, samples = "
          + " ".join(f"{f:.2e}" for f in worst) + f" at (case, cov_add) {where}")
    return bad


def mid_results(runs, pre):
    out = []
    for kind, (rc, res, st) in enumerate(runs.mid(pre)):
        assert rc == 0 and np.all(st == 0), (pre, kind, rc, st)
        out.append(res)
    return out


# ------------------------------------------------------------------ the mid batch
def test_mid_a_all_restarts_one_handle(fx, runs):
    """a: the data registered 32 times, one model per restart, logp and samples of one
    lfm_mbatch_predictive_f64 per cov_add."""
    assert fx["a_mean"].shape == (32, 2, 20) and fx["a_smp"].shape == (32, 2, 5, 20)
    bad = judge(fx, "a", "mid", mid_results(runs, "a"), verbose=ILL)
    assert not bad, bad


@pytest.mark.parametrize("m", [129, 63])
def test_mid_b_one_handle_per_m(fx, runs, m):
    """b at restarts 0, 7, 13, 19, 29: m = 129 (m + 1 = 130: three block columns of the scale's
    factor, the residual row second in the third) and m = 63 (m + 1 = 64: the residual row is the
    last of the only block)."""
    pre = f"b{m}"
    assert fx[pre + "_smp"].shape == (5, 2, 5, m)
    bad = judge(fx, pre, "mid", mid_results(runs, pre), verbose=range(5))
    assert not bad, bad


def test_mid_c_through_midbatchpredictor(fx, runs):
    """c: the 15 C5 problems at rounds 0, 7, 15 as one batch of 45 through
    predict.MidBatchPredictor.log_prob and .sample, both cov_add values; rows 60..79 of the test
    inputs repeat rows 40..59."""
    assert fx["c_smp"].shape == (45, 2, 5, 80)
    bad = judge(fx, "c", "mid", mid_results(runs, "c"))
    assert not bad, bad


def test_mid_mixed_sizes_in_one_handle(fx, runs):
    """a at restarts 5 and 29, b at restart 29 with m = 129 and the first 15 C5 problems in one
    handle (1 and 3 block columns of S; 1, 3 and 2 of the scale): every result the homogeneous
    batch's bit for bit, and inside its bound."""
    members = ([("a", r) for r in A_MIXED] + [("b129", B_MIXED)]
               + [("c", q) for q in range(C5_MIXED)])
    probs = [runs.probs[pre][q] for pre, q in members]
    ys = [fx[pre + "_ystar"][q] for pre, q in members]
    seeds = [int(fx[pre + "_seed"][q]) for pre, q in members]
    got = mid_predictive(probs, [0, 1], ys, seeds)
    bad, wrong_bits, worst = [], [], 0.0
    for kind, (rc, res, st) in enumerate(got):
        assert rc == 0 and np.all(st == 0), (kind, rc, st)
        for i, (pre, q) in enumerate(members):
            ref = runs.mid(pre)[kind][1][q]
            same = (np.array_equal(res[i][0], ref[0]) and res[i][1] == ref[1]
                    and np.array_equal(res[i][2], ref[2]))
            figs = figures(fx, pre, q, kind, res[i])
            worst = max(worst, float(figs.max()))
            if not same:
                wrong_bits.append((labels_of(pre)[q], kind))
            if not figs.max() <= 1.0:
                bad.append((labels_of(pre)[q], kind, figs.round(3).tolist()))
    print(f"mixed handle: {len(members)} problems, "
          f"{'every result' if not wrong_bits else 'NOT every result'} the homogeneous batch's "
          f"bits; worst |d| / bound = {worst:.2e}")
    assert not wrong_bits, wrong_bits
    assert not bad, bad


# ------------------------------------------------------------------ the host route
@pytest.mark.parametrize("pre", ["a", "b129", "b63"])
def test_host_route_a_b(fx, runs, pre):
    """lfm_posterior_f64 -> lfm_mvn_sample_f64 / lfm_log_prob_f64, both cov_add values."""
    bad = judge(fx, pre, "host", runs.host(pre), verbose=ILL if pre == "a" else range(5))
    assert not bad, bad


def test_host_route_c_through_exactlfm(fx, runs):
    """ExactLFM.multi_gene_predict(...).sample / .log_prob on the 45 C5 problems (the shim's
    scale = cov + jitter I: cov_add 0)."""
    bad = judge(fx, "c", "host", runs.host("c"), kinds=(0,))
    assert not bad, bad


# ------------------------------------------------------------------ the resident path
@pytest.mark.parametrize("pre", GROUPS)
def test_resident_path(fx, runs, pre):
    """lfm_post_create + lfm_post_sample_f64 at cov_add = jitter: mean and samples inside the
    truth's bounds, and the bits of lfm_mvn_sample_f64 fed the handle's own lfm_post_predict_f64
    mean and cov + jitter I (include/lfm.h), at the restarts. Against the lfm_posterior_f64 route
    (a factorisation of its own) the largest difference is printed."""
    res = runs.resident(pre)
    labels = labels_of(pre)
    qs = [q for q, r in enumerate(res) if r is not None]
    assert qs == (list(range(30, 45)) if pre == "c" else list(range(len(labels))))
    bad, wrong_bits, worst, far = [], [], np.zeros(2), 0.0
    for q in qs:
        mean, X, (pmean, pX) = res[q]
        if not (np.array_equal(mean, pmean) and np.array_equal(X, pX)):
            wrong_bits.append(labels[q])
        rtol = float(fx[pre + "_rtol"][q, 0])
        figs = np.array([ratio(mean, fx[pre + "_mean"][q, 0], rtol),
                         ratio(X[list(SAMPLES)], fx[pre + "_smp"][q, 0], rtol)])
        worst = np.maximum(worst, figs)
        if not figs.max() <= 1.0:
            bad.append((labels[q], figs.round(3).tolist()))
        host = runs.host(pre)[0][q]
        far = max(far, ratio(X[list(SAMPLES)], host[2], rtol))
    print(f"resident {pre}: worst |d| / bound mean, samples = "
          + " ".join(f"{f:.2e}" for f in worst)
          + f"; resident - host route in units of the bound: {far:.2e}")
    assert not wrong_bits, wrong_bits
    assert not bad, bad


# ------------------------------------------------------------------ not positive definite
def test_not_pd_on_all_three_paths(fx, runs):
    """a's restart 5 with latent test rows at cov_add = jitter (the truth scale's smallest
    eigenvalue is -0.96): LFM_E_NOT_PD, NaN in every output and a non-zero status on the mid
    batch, the resident path and the host route; a neighbour in the same batch keeps its bits
    and every path works afterwards."""
    from dis_project_amd import _lib

    r = int(fx["npd_restart"])
    assert float(fx["npd_min_eig"]) < -1e-3 and r == 5
    bad_t = np.ascontiguousarray(fx["npd_t"])
    p5, p29 = runs.probs["a"][r], runs.probs["a"][29]
    ys, seeds = [fx["a_ystar"][r], fx["a_ystar"][29]], [int(fx["a_seed"][r]), int(fx["a_seed"][29])]
    clean = runs.mid("a")[0][1]
    # the mid batch: a failed call, then a clean one on the same handle
    (rc, res, st), (rc2, res2, st2) = mid_predictive(
        [p5, p29], [0, 0], ys, seeds, ts=[[bad_t, p29[3]], [p5[3], p29[3]]])
    assert rc == _lib.LFM_E_NOT_PD and st.tolist() == [_lib.LFM_E_NOT_PD, 0], (rc, st)
    assert np.all(np.isnan(res[0][0])) and np.isnan(res[0][1]) and np.all(np.isnan(res[0][2]))
    assert rc2 == 0 and not st2.any()
    for got in (res[1], res2[1]):
        assert np.array_equal(got[0], clean[29][0]) and got[1] == clean[29][1]
        assert np.array_equal(got[2], clean[29][2])
    assert np.array_equal(res2[0][0], clean[r][0]) and res2[0][1] == clean[r][1]
    assert np.array_equal(res2[0][2], clean[r][2])
    # the resident path
    cadd = cadds_of(p5[4])[0]
    with Resident(p5) as post:
        rc, mean, X = post.sample(bad_t, cadd, seeds[0])
        assert rc == _lib.LFM_E_NOT_PD and np.all(np.isnan(mean)) and np.all(np.isnan(X))
        rc, mean, X = post.sample(p5[3], cadd, seeds[0])
        assert rc == 0
        np.testing.assert_array_equal(mean, runs.resident("a")[r][0])
        np.testing.assert_array_equal(X, runs.resident("a")[r][1])
    # the host route: S is definite, the scale is not
    rcs, (mean, logp, X) = host_route(p5, 0, ys[0], seeds[0], t=bad_t)
    assert rcs == (0, _lib.LFM_E_NOT_PD, _lib.LFM_E_NOT_PD), rcs
    assert np.all(np.isfinite(mean)) and np.isnan(logp) and np.all(np.isnan(X))
    rcs, got = host_route(p5, 0, ys[0], seeds[0])
    assert rcs == (0, 0, 0)
    ref = runs.host("a")[0][r]
    assert np.array_equal(got[0], ref[0]) and got[1] == ref[1] and np.array_equal(got[2], ref[2])
    print(f"not PD (smallest eigenvalue {float(fx['npd_min_eig']):.3f}): refused on the mid batch, "
          "the resident path and the host route; all three usable afterwards")


# ------------------------------------------------------------------ diagnostics
def test_diagnostics_at_ill_conditioned_restarts(fx, runs):
    """a at restarts 1, 5, 10 and 29 (and b129 at restart 29): the mid result's and the host
    route's distance from the truth, and from each other, in units of the bound. Nothing new is
    asserted; the lines name the suspect when a test above fails."""
    worst = 0.0
    for pre, qs in (("a", ILL), ("b129", (B_MIXED,))):
        mid, host = mid_results(runs, pre), runs.host(pre)
        for q in qs:
            for kind in (0, 1):
                fm = figures(fx, pre, q, kind, mid[kind][q])
                fh = figures(fx, pre, q, kind, host[kind][q])
                rtol = float(fx[pre + "_rtol"][q, kind])
                apart = ratio(mid[kind][q][2], host[kind][q][2], rtol)
                worst = max(worst, float(fm.max()), float(fh.max()))
                print(f"{labels_of(pre)[q]} cov_add {kind}: |d| / bound mean, logp, samples: mid "
                      + " ".join(f"{f:.2e}" for f in fm) + "; host "
                      + " ".join(f"{f:.2e}" for f in fh) + f"; mid - host samples {apart:.2e}")
    print(f"ill-conditioned restarts: worst |d| / bound = {worst:.2e}")
    assert np.isfinite(worst)

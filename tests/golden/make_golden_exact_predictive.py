"""Extended-precision golden joint samples and held-out log densities at C3's restarts and C5's
rounds.

    python tests/golden/make_golden_exact_predictive.py    # exact_predictive.npz

The predictive distribution of multi_gene_predict, N(mean, cov + cov_add I), is drawn from and
scored by lfm_mbatch_predictive_f64, lfm_post_sample_f64 and lfm_posterior_f64 ->
lfm_mvn_sample_f64 / lfm_log_prob_f64. tests/test_gpu_mid_draw.py and test_gpu_sample.py take
their reference mean and covariance from the device at benign hyperparameters; here the truth is
lfm_exact.predictive_exact end to end: entries of the reference formula at 60 digits carried in
long double, a long double Cholesky of S, the covariance never rounded before cov_add joins its
diagonal, a long double Cholesky of the scale, a forward solve and a product.

All test rows are gene rows (flag 1); diag_add = obs_stddev^2 (multi_gene_predict's); cov_add
index 0 = the model's jitter (what the shim passes), 1 = obs_stddev^2.

  a_*   n = 28: the first C5 problem, the 4-gene sub-models of all 32 restarts; a_t (m = 20): the
        times 0, 0.9, 3.3, 7.7, 12.5 under each of the gene indices -1, 1, 2, G (they wrap and
        clamp to 3, 1, 2, 3: the last block's kernel rows repeat the first's). A t = 0 row has
        K(t, .) = 0, so its row of the scale is cov_add on the diagonal and 0 elsewhere.
  b_*   n = 129, 3 genes: make_golden_exact_posterior.b_problem()'s x, y, v at restarts
        B_RESTARTS; b_t: 129 gene rows (times U(0, 13), gene indices -1..3) from
        default_rng(B_T_SEED). b129_*: all of them (m + 1 = 130: the residual row is the second
        of a third 64-row block; 256-row padding for the 128-row product). b63_*: the first 63
        (m + 1 = 64: the residual row closes a block).
  c_*   the 15 C5 problems at rounds C_ROUNDS, generate_test_times_pred(20, 4) (m = 80): rows
        60..79 repeat rows 40..59, so the scale has cov_add as an exact 20-fold eigenvalue.
  per case [and cov_add]:
        *_mean    the truth mean
        *_ystar   truth mean + L_truth zeta, zeta = default_rng([m, case, 11]).standard_normal(m),
                  rounded to fp64: log-determinant and quadratic term of comparable size
        *_logp    log N(ystar; mean, scale)
        *_seed, *_z, *_smp the case's seed, the normals tests/philox_ref.randn(seed, s, 1, m) at
                  the absolute sample indices SAMPLES and the truth samples mean + L_truth z
        *_rtol    max(1e-9, 8 x the worst relative error of scipy's Cholesky and triangular solves
                  on the correctly rounded entries, plain and with every entry moved one ulp up or
                  down with probability 1/2), capped at 1e-5; the error is |d| / max(1, |logp|)
                  for the log density and max|d| / max|truth| for mean and samples. No case is
                  beyond the cap (asserted).
        *_lapack_err, *_oracle_err   (mean, logp, samples): those errors, and the same of
                  oracle.multi_gene_predict -> numpy's Cholesky (inf where that fails)
  every case is computed a second way (a seeded permutation of the training rows) and the two
  agree to 1e-3 of the case's bound.
  npd_*  a's restart NPD_RESTART with every test row's flag 0 (latent rows) at cov_add = jitter:
        the truth scale's smallest eigenvalue (npd_min_eig) is below -1e-3, so every path must
        refuse it whatever its rounding. (Whether the flag-switched kernel's latent covariance is
        indefinite depends on the hyperparameters: at restart 0 these rows give a positive
        semi-definite covariance, smallest eigenvalue of the scale +1e-4; at restart 5, -0.96.)
"""

from __future__ import annotations

import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_golden_exact as GE  # noqa: E402
from make_golden_exact_posterior import (B_RESTARTS, C_ROUNDS, b_problem, c5_datas,  # noqa: E402
                                         hyp_of, perturbed, rel_errs, rtol_of, xyv)
from dis_project_amd import configs, dataset as ds  # noqa: E402
from oracle import lfm_exact as E  # noqa: E402
from oracle import lfm_oracle as O  # noqa: E402
from tests import philox_ref  # noqa: E402

TIE = 1e-3
A_TIMES = (0.0, 0.9, 3.3, 7.7, 12.5)
SAMPLES = (0, 63, 64, 65, 129)  # absolute sample indices: the 64- and 128-row tile edges
B_T_SEED = 12900
B_MS = (129, 63)
NPD_RESTART = 5
OUT = os.path.join(HERE, "exact_predictive.npz")


# ----------------------------------------------------------------- problems
def a_inputs(G=4, flag=1.0):
    tm = np.asarray(A_TIMES)
    return np.concatenate([np.stack((tm, np.full(5, float(g)), np.full(5, flag)), -1)
                           for g in (-1, 1, 2, G)])


def b_inputs():
    rng = np.random.default_rng(B_T_SEED)
    return np.stack((rng.uniform(0, 13, 129), rng.integers(-1, 4, 129).astype(float),
                     np.ones(129)), -1)


def seed_of(group, case):
    """The case's generator seed; b's are above 2^32, so both key words are in use."""
    return {"a": 7000, "b129": 2 ** 40 + 129000, "b63": 2 ** 40 + 63000, "c": 9000}[group] + case


def normals(seed, m):
    return np.concatenate([philox_ref.randn(seed, s, 1, m) for s in SAMPLES])


# ------------------------------------------------------------------- one case
def errs(got, ref):
    """(mean, logp, samples) errors of a restatement: inf where it failed."""
    if got[0] is None:
        return [np.inf] * 3
    em, ex = rel_errs((got[0], got[2]), (ref[0], ref[2]))
    return [em, abs(got[1] - ref[1]) / max(1.0, abs(ref[1])), ex]


def case(ent, x, y, v, dadd, cadd, t, D, B, key, seed, z=None):
    """The stored record of one predictive distribution from its long double entries. key: the
    case's index (zeta and the tie's permutation derive from it); z: the normals, philox_ref's
    when None."""
    m = t.shape[0]
    z = normals(seed, m) if z is None else z
    zeta = np.random.default_rng([m, key, 11]).standard_normal(m)
    head = (ent, x, y, v, dadd, t, D, B, cadd)
    _, _, ys = E.predictive_exact(*head, None, zeta)
    if ys is None:
        return dict(not_pd=True)
    ystar = ys[0]
    ref = E.predictive_exact(*head, ystar, z)
    perm = np.random.default_rng([m, key, 12]).permutation(x.shape[0])
    again = E.predictive_exact(*head, ystar, z, perm=perm)
    ent64 = tuple(np.asarray(q).astype(np.float64) for q in ent)
    la = [errs(E.predictive_exact(e, *head[1:], ystar, z, dtype=np.float64), ref)
          for e in (ent64, perturbed(ent, 1000 * m + key))]
    lapack_err = np.max(np.array(la), axis=0)
    rtol, dropped = rtol_of(float(lapack_err.max()))
    assert not dropped, (m, key, lapack_err)
    tie = max(errs(again, ref))
    assert tie <= TIE * rtol, (m, key, tie)
    return dict(not_pd=False, mean=ref[0], ystar=ystar, logp=ref[1], smp=ref[2], z=z, seed=seed,
                rtol=rtol, lapack_err=lapack_err, tie=tie)


def oracle_errs(rec, x, y, v, t, D, S, B, l, sd, jit, cadd):
    """oracle.multi_gene_predict -> numpy's Cholesky against the truth."""
    with np.errstate(all="ignore"):
        om, ov = O.multi_gene_predict(x, y, v, t, D, S, B, l, sd, jit)
        scale = ov + np.eye(len(om)) * (cadd - jit)
        try:
            L = np.linalg.cholesky(scale)
        except np.linalg.LinAlgError:
            return [np.inf] * 3
        w = np.linalg.solve(L, rec["ystar"] - om)
        logp = -(len(om) * np.log(2 * np.pi) + 2 * np.sum(np.log(np.diagonal(L))) + w @ w) / 2
        got = (om, float(logp), om + rec["z"] @ L.T)
    ref = (rec["mean"], rec["logp"], rec["smp"])
    return [e if np.isfinite(e) else np.inf for e in errs(got, ref)]


def both(ent, x, y, v, t, D, S, B, l, sd, jit, key, seed, zs=None):
    """The records of both cov_add values."""
    recs = []
    for kind, cadd in enumerate((jit, sd * sd)):
        rec = case(ent, x, y, v, sd * sd, cadd, t, D, B, key, seed, zs)
        assert not rec["not_pd"], (t.shape[0], key, kind)
        rec["oracle_err"] = oracle_errs(rec, x, y, v, t, D, S, B, l, sd, jit, cadd)
        recs.append(rec)
    return recs


def line(label, recs, t0):
    print(f"{label}: " + " | ".join(
        f"lapack={max(q['lapack_err']):.1e} oracle={max(q['oracle_err']):.1e} rtol={q['rtol']:.0e} "
        f"logp={q['logp']:.3f}" for q in recs) + f" ({time.perf_counter() - t0:.1f} s)", flush=True)


def a_case(r, z=None):
    t0 = time.perf_counter()
    x, y, v = xyv(c5_datas()[0])
    t = a_inputs()
    D, S, B, l, sd, jit = hyp_of(E.submodel(GE.restart_models()[r], 4)[0])
    ent = E.posterior_entries(x, t, D, S, l)
    recs = both(ent, x, y, v, t, D, S, B, l, sd, jit, r, seed_of("a", r), z)
    # the t = 0 rows: K(t, .) = 0, so the truth scale's diagonal there is 0 + cov_add
    assert np.all(np.asarray(ent[1])[::5] == 0) and np.all(np.asarray(ent[2])[::5] == 0)
    _, cov = E.posterior_from_entries(ent, x, y, v, sd * sd, t, D, B)
    for kind, cadd in enumerate((jit, sd * sd)):
        recs[kind]["scale_diag"] = np.diagonal(cov) + cadd
    line(f"a r{r}", recs, t0)
    return recs


def b_case(r, ms=B_MS, zs=None):
    """{m: records} of restart r; the m = 63 entries are a block of the m = 129 ones."""
    t0 = time.perf_counter()
    x, y, v, _ = b_problem()
    t = b_inputs()[:max(ms)]
    D, S, B, l, sd, jit = hyp_of(E.submodel(GE.restart_models()[r], 3)[0])
    Kxx, Ktx, Ktt = E.posterior_entries(x, t, D, S, l)
    out = {}
    for m in ms:
        ent = (Kxx, Ktx[:m], Ktt[:m, :m])
        out[m] = both(ent, x, y, v, t[:m], D, S, B, l, sd, jit, r, seed_of(f"b{m}", r),
                      None if zs is None else zs[m])
        line(f"b r{r} m={m}", out[m], t0)
    return out


def c_case(q, z=None):
    """q = 15 * (index into C_ROUNDS) + problem."""
    t0 = time.perf_counter()
    k, p = divmod(q, 15)
    x, y, v = xyv(c5_datas()[p])
    works = configs.c5_ablations()
    model = configs.c5_rounds([w.model for w in works], 16)[15 * C_ROUNDS[k] + p]
    D, S, B, l, sd, jit = hyp_of(model)
    t = np.asarray(ds.generate_test_times_pred(20, 4), np.float64)
    assert np.array_equal(t[60:, 0], t[40:60, 0]) and np.all(t[:, 2] == 1)
    ent = E.posterior_entries(x, t, D, S, l)
    assert np.array_equal(ent[2][60:], ent[2][40:60])
    recs = both(ent, x, y, v, t, D, S, B, l, sd, jit, q, seed_of("c", q), z)
    line(f"c round {C_ROUNDS[k]} problem {p}", recs, t0)
    return recs


def npd_case():
    """a's restart NPD_RESTART with latent test rows: (t, the truth scale's smallest
    eigenvalue)."""
    x, y, v = xyv(c5_datas()[0])
    t = a_inputs(flag=0.0)
    D, S, B, l, sd, jit = hyp_of(E.submodel(GE.restart_models()[NPD_RESTART], 4)[0])
    ent = E.posterior_entries(x, t, D, S, l)
    _, cov = E.posterior_from_entries(ent, x, y, v, sd * sd, t, D, B)
    eig = float(np.linalg.eigvalsh(cov + jit * np.eye(20))[0])
    assert eig < -1e-3, eig
    got = E.predictive_exact(ent, x, y, v, sd * sd, t, D, B, jit, np.zeros(20), np.zeros((1, 20)))
    assert got == (None, None, None)
    return t, eig


# --------------------------------------------------------------------- stacking
def stack(out, pre, cases):
    """cases[q][kind] -> arrays [Q, 2, ...]; seed and z per case."""
    for key in ("mean", "ystar", "logp", "smp", "rtol", "lapack_err", "oracle_err", "tie"):
        out[f"{pre}_{key}"] = np.array([[np.asarray(rec[key], np.float64) for rec in recs]
                                        for recs in cases])
    for recs in cases:
        assert recs[0]["seed"] == recs[1]["seed"] and np.array_equal(recs[0]["z"], recs[1]["z"])
    out[f"{pre}_seed"] = np.array([recs[0]["seed"] for recs in cases], np.uint64)
    out[f"{pre}_z"] = np.stack([recs[0]["z"] for recs in cases])


def make():
    with ProcessPoolExecutor(int(os.environ.get("GOLDEN_THREADS", "8"))) as ex:
        b = ex.map(b_case, B_RESTARTS)
        c = ex.map(c_case, range(15 * len(C_ROUNDS)))
        a = ex.map(a_case, range(GE.RESTARTS))
        a, b, c = list(a), list(b), list(c)
    out = {"b_restarts": np.array(B_RESTARTS, np.int64), "c_rounds": np.array(C_ROUNDS, np.int64),
           "samples": np.array(SAMPLES, np.int64)}
    out["a_x"], out["a_y"], out["a_v"] = xyv(c5_datas()[0])
    out["a_t"] = a_inputs()
    out["b_x"], out["b_y"], out["b_v"], _ = b_problem()
    out["b_t"] = b_inputs()
    out["c_t"] = np.asarray(ds.generate_test_times_pred(20, 4), np.float64)
    stack(out, "a", a)
    for m in B_MS:
        stack(out, f"b{m}", [q[m] for q in b])
    stack(out, "c", c)
    out["npd_t"], eig = npd_case()
    out["npd_min_eig"], out["npd_restart"] = np.float64(eig), np.int64(NPD_RESTART)
    pres = ("a", "b129", "b63", "c")
    print("worst lapack "
          + " ".join(f"{p}={out[p + '_lapack_err'].max(axis=(0, 1))}" for p in pres))
    print("worst rtol " + " ".join(f"{p}={out[p + '_rtol'].max():.0e}" for p in pres)
          + f" worst tie / rtol {max((out[p + '_tie'] / out[p + '_rtol']).max() for p in pres):.1e}"
          f" not-PD case's smallest eigenvalue {eig:.3e}")
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT))
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    make()

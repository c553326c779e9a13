"""Extended-precision truth for the small-problem batch (lfm_batch_*) at C3's restarts.

    python tests/golden/make_golden_exact_small.py        # tests/golden/exact_small.npz

The small batch (one workgroup per problem, n <= 128, lfm_small.hip) picks its factor, its sweep,
its entry code and its derivative code by n, by the layout and by what else is in the launch. Away
from n = 28 on the 7-time grid it was compared with oracle.mll_grad / multi_gene_predict at benign
hyperparameters only; at the restarts those oracles are wrong (the *_oracle_err columns). This
fixture holds the truth at the edges of every variant. The cases, their inputs and their seeds are
tests/small_exact_inputs.py's (CASES, POST); nothing that can be rebuilt from them is stored, only
a checksum of each problem's x and y (*_crc).

  <case>_*  per restart of the case, by make_golden_exact_grad's hyp_of / finish / stack on
            lfm_exact.mll_grad_exact's direct route: *_grad, *_scale, *_grad_fp64, *_grad_rtol,
            *_mll, *_mll_rtol, *_oracle_err (packed [d (G), s (G), b (G), l, obs_stddev]; the
            value-only cases carry the same columns), *_grad_dropped, and *_restarts.
  <post>_*  per restart of ILL and diagonal (0: jitter, latent_predict's; 1: obs_stddev^2,
            multi_gene_predict's) by make_golden_exact_posterior's PairCache / posterior_entries /
            case (with its second, permuted computation and TIE rule): *_mean, *_cov (lower
            triangle), *_rtol, *_lapack_err, *_oracle_err, *_not_pd, *_dropped.

The generator asserts: no case dropped, none not PD, every rtol at the project's floor (1e-8 for
the gradient, 1e-9 for the value and the posterior), the file under 1 MiB.

A shuffled copy's truth is computed from its own x and y, and tied to its grid copy (COPIES) in
what a permutation of the rows leaves unchanged. The mean function goes by block position, so with
G > 1 the shuffled problem has the grid copy's Sigma, permuted, and another residual: tied are
Sigma entry by entry, the value through the grid copy's Sigma and the shuffled residual carried
back, and the posterior's covariance. With G = 1 (1 x 127) it is the same problem: the value, the
gradient, the posterior mean and covariance are tied (the posterior's grid copy, which the device
cannot hold, is computed here for the tie alone). Every tie is 1e-3 of the quantity's bound.
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

import make_golden_exact_grad as GG  # noqa: E402
import make_golden_exact_posterior as GP  # noqa: E402
from oracle import lfm_exact as E  # noqa: E402
from tests import small_exact_inputs as I  # noqa: E402

TIE = 1e-3
OUT = os.path.join(HERE, "exact_small.npz")
TIED = {name for pair in I.COPIES for name in pair}


def grad_case(job):
    name, r = job
    t0 = time.perf_counter()
    _, G, T, shuffled, _, _ = I.case_of(name)
    x, y, model = I.problem(G, T, shuffled, r)
    D, S, B, l, sd, jit = GG.hyp_of(model)
    ex = E.mll_grad_exact(x, y, D, S, B, l, sd, jit)
    assert not ex.get("not_pd"), (name, r)
    rec = GG.finish(ex, x, y, D, S, B, l, sd, jit)
    rec["crc"] = I.checksum(x, y)
    if name in TIED:
        rec["Sigma"], rec["r"] = ex["Sigma"], ex["r"]
    print(f"{name} r{r}: fp64 lapack err/scale={rec['fp64_err']:.1e} oracle err/scale="
          f"{rec['oracle_err']:.1e} grad_rtol={rec['grad_rtol']:.0e} mll_rtol={rec['mll_rtol']:.0e}"
          f" ({time.perf_counter() - t0:.0f} s)", flush=True)
    return rec


def post_case(job):
    name, G, T, shuffled, r = job
    t0 = time.perf_counter()
    x, y, model = I.problem(G, T, shuffled, r)
    v, t = I.post_extra(G, T, shuffled, r)
    assert np.array_equal(t, GP.a_inputs(G))
    D, S, B, l, sd, jit = GP.hyp_of(model)
    ent = E.posterior_entries(x, t, D, S, l, cache=E.PairCache(D, S, l))
    recs = []
    for kind, dadd in enumerate((jit, sd * sd)):
        rec = GP.case(ent, x, y, v, dadd, t, D, B, 8 * ((1000 * G + T) * 32 + r) + 4 * shuffled
                      + 2 * kind)
        assert not rec["not_pd"], (name, r, kind)
        rec["oracle_err"] = GP.oracle_errs(kind, rec, x, y, v, t, D, S, B, l, sd, jit)
        recs.append(rec)
    print(f"{name} r{r}: " + " ".join(
        f"lapack={max(q['lapack_err']):.1e} oracle={max(q['oracle_err']):.1e} rtol={q['rtol']:.0e}"
        for q in recs) + f" ({time.perf_counter() - t0:.1f} s)", flush=True)
    return dict(recs=recs, crc=I.checksum(x, y, v))


def stack_post(out, pre, cases, m=20):
    ii, jj = np.tril_indices(m)
    for key, fn in (("mean", lambda q: q["mean"]), ("cov", lambda q: q["cov"][ii, jj]),
                    ("rtol", lambda q: q["rtol"]), ("lapack_err", lambda q: q["lapack_err"]),
                    ("oracle_err", lambda q: q["oracle_err"])):
        out[f"{pre}_{key}"] = np.array([[fn(q) for q in c["recs"]] for c in cases], np.float64)
    for key in ("not_pd", "dropped"):
        out[f"{pre}_{key}"] = np.array([[q[key] for q in c["recs"]] for c in cases], bool)
    for c in cases:
        for q in c["recs"]:
            assert np.array_equal(q["cov"], q["cov"].T)
    out[f"{pre}_crc"] = np.array([c["crc"] for c in cases], np.int64)


def tie_grad(shuf, grid, recs):
    """The shuffled copy against its grid copy at every restart of ILL (the module docstring)."""
    _, G, T, _, rs_s, _ = I.case_of(shuf)
    rs_g = I.case_of(grid)[4]
    worst = np.zeros(3)
    for q, r in enumerate(rs_s):
        a, b = recs[shuf][q], recs[grid][rs_g.index(r)]
        p = I.permutation(G, T, r)
        Sg, Ss = b["Sigma"], a["Sigma"]
        dS = float(np.max(np.abs(Ss - Sg[np.ix_(p, p)])) / np.max(np.abs(Sg)))
        back = np.empty_like(a["r"])
        back[p] = a["r"]
        val = E.mll_exact(Sg, back)[0]
        dv = abs(val - a["mll"]) / (a["mll_rtol"] * abs(a["mll"]))
        dg = 0.0
        if G == 1:
            np.testing.assert_array_equal(back, b["r"])
            dv = max(dv, abs(b["mll"] - a["mll"]) / (a["mll_rtol"] * abs(a["mll"])))
            bound = a["grad_rtol"] * a["scale"] + 1e-10 * np.abs(a["grad"])
            dg = float(np.max(np.abs(a["grad"] - b["grad"]) / bound))
        worst = np.maximum(worst, (dS, dv, dg))
        assert dS <= 1e-15 and dv <= TIE and dg <= TIE, (shuf, r, dS, dv, dg)
    print(f"tie {shuf} ~ {grid}: |dSigma| / max|Sigma| = {worst[0]:.1e}, value / bound = "
          f"{worst[1]:.1e}, gradient / bound = {worst[2]:.1e}"
          + ("" if G == 1 else " (G > 1: none)"))


def tie_post(shuf, grid, G, posts):
    worst = np.zeros(2)
    for a, b in zip(posts[shuf], posts[grid]):
        for qa, qb in zip(a["recs"], b["recs"]):
            dc = float(np.max(np.abs(qa["cov"] - qb["cov"]))
                       / (qa["rtol"] * np.max(np.abs(qb["cov"])) + 1e-12))
            dm = float(np.max(np.abs(qa["mean"] - qb["mean"]))
                       / (qa["rtol"] * np.max(np.abs(qb["mean"])) + 1e-12)) if G == 1 else 0.0
            worst = np.maximum(worst, (dc, dm))
            assert dc <= TIE and dm <= TIE, (shuf, dc, dm)
    print(f"tie {shuf} ~ {grid}: covariance / bound = {worst[0]:.1e}, mean / bound = "
          f"{worst[1]:.1e}" + ("" if G == 1 else " (G > 1: none)"))


def make():
    # the largest problems first, so that the pool's tail is short
    gjobs = sorted(((c[0], r) for c in I.CASES for r in c[4]),
                   key=lambda j: -I.case_of(j[0])[1] * I.case_of(j[0])[2])
    pjobs = [(name, G, T, sh, r) for name, G, T, sh in I.POST + (("p1x127", 1, 127, False),)
             for r in I.ILL]
    with ProcessPoolExecutor(int(os.environ.get("GOLDEN_THREADS", "8"))) as ex:
        gres = ex.map(grad_case, gjobs)
        pres = ex.map(post_case, pjobs)
        gres, pres = list(gres), list(pres)
    recs = {c[0]: [None] * len(c[4]) for c in I.CASES}
    for (name, r), rec in zip(gjobs, gres):
        recs[name][I.case_of(name)[4].index(r)] = rec
    posts = {}
    for job, rec in zip(pjobs, pres):
        posts.setdefault(job[0], []).append(rec)

    out = {"ill": np.array(I.ILL, np.int64)}
    for name, _, _, _, restarts, _ in I.CASES:
        GG.stack(out, name, recs[name])
        out[f"{name}_restarts"] = np.array(restarts, np.int64)
        out[f"{name}_crc"] = np.array([s["crc"] for s in recs[name]], np.int64)
        # the conditions of the fixture: nothing dropped (not PD is asserted per case), every
        # bound at the project's floor
        assert out[f"{name}_grad_dropped"].size == 0, (name, out[f"{name}_grad_dropped"])
        assert np.all(out[f"{name}_grad_rtol"] == GG.PROJECT_GRAD_RTOL), name
        assert np.all(out[f"{name}_mll_rtol"] == 1e-9), name
    for name, _, _, _ in I.POST:
        stack_post(out, name, posts[name])
        assert not np.any(out[f"{name}_dropped"]) and not np.any(out[f"{name}_not_pd"]), name
        assert np.all(out[f"{name}_rtol"] == GP.PROJECT_RTOL), name
    for shuf, grid in I.COPIES:
        if shuf in recs:
            tie_grad(shuf, grid, recs)
        else:
            tie_post(shuf, grid, I.case_of(shuf)[1], posts)
    tie_post("p1x127s", "p1x127", 1, posts)
    worst = {k: max(float(np.max(out[f"{c[0]}_{k}"])) for c in I.CASES)
             for k in ("oracle_err",)}
    print(f"{sum(len(c[4]) for c in I.CASES)} value / gradient problems, "
          f"{2 * len(I.ILL) * len(I.POST)} posteriors; worst oracle err / scale = "
          f"{worst['oracle_err']:.1e}; fp64 restatement's worst err / scale = "
          f"{max(s['fp64_err'] for v in recs.values() for s in v):.1e}, posterior "
          f"{max(float(np.max(out[p[0] + '_lapack_err'])) for p in I.POST):.1e}")
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT))
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    make()

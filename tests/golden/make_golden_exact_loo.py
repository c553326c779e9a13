"""Extended-precision golden values of the leave-one-out CV objective (gpjax 0.8.2
ConjugateLOOCV.step, Rasmussen & Williams 5.4.2) at C3's restarts and on the C1 problem.

    python tests/golden/make_golden_exact_loo.py          # tests/golden/exact_loo.npz

With S = K + (jitter + obs_stddev^2) I, r = y - m, a = S^{-1} r and k_i = [S^{-1}]_ii:

    mu_i = y_i - a_i / k_i,   var_i = 1 / k_i,
    value = sum_i (-1/2 log 2 pi + 1/2 log k_i - 1/2 a_i^2 / k_i),
    d value / d theta = 1/2 tr(W_loo dS/dtheta) + u^T dm/dtheta,
    W_loo = -2 S^{-1} diag(c) S^{-1} + u a^T + a u^T,   c_i = (1 + a_i^2 / k_i) / (2 k_i),
    u = S^{-1} b,   b_i = a_i / k_i.

Everything is built from what oracle/lfm_exact.py offers: mll_grad_exact gives the long double
Sigma, r and the derivative blocks, w_exact gives a and S^{-1} (as a a^T - W), contract_grad
contracts W_loo and u with the blocks. The fp64 restatement is scipy's Cholesky and inverse on
the correctly rounded Sigma and r (as lfm_exact.mll_grad_fp64). The truth's own uncertainty is the
long double algebra repeated under the reversed pivot order; it is asserted within 1e-3 of every
bound stored here.

  sub_*   restarts 0..31 on the 4 x 256 grid of make_golden_exact.sub_problem (N = 1024)
  una_*   make_golden_exact_grad.una_problem at restarts ILL (N = 129, y = exact_grad's una_y)
  mix_*   mixed_mll_n48 at restarts ILL; Sigma is not PD at restarts 1 and 5 (NaN entries)
  c1_*    configs.c1_p53() (n = 35) at its base model: case 0 as it is, case 1 with observation
          OUTLIER moved by 30 obs_stddev (c1_y holds both)
  per problem of each group:
    *_loo, *_loo_fp64, *_loo_fp64_err, *_loo_rtol
                                      exact value, the restatement's, its relative error and
                                      make_golden_exact.rtol_of's rule on it
    *_mean, *_var                     exact per-point LOO mean and variance [n]
    *_mean_fp64_err, *_mean_rtol      the restatement's worst |error| / (|y_i| + |a_i| / k_i) and
                                      the value rule on it
    *_var_fp64_err, *_var_rtol        the same, relative
    *_grad, *_scale, *_grad_fp64, *_grad_fp64_err, *_grad_rtol
                                      as make_golden_exact_grad ([d, s, b, l, obs_stddev])
    *_truth_err                       the reversed-order repeat's worst |difference| / bound
    *_max_z2                          max a_i^2 / k_i, the cancellation in -Bt_ii - a_i^2
  sub_dropped   restarts whose restatement is outside 1e-5 (at most MAX_DROPPED)
  fit_*   five Adam steps (learning rate 0.01) on the negative LOO value of the C1 problem,
          trainer.JaxTrainer driven from the host: fit_losses from the long double value and
          gradient, fit_losses_fp64 from the restatement's, fit_dev their worst relative
          difference and fit_rtol the value rule on it.
"""

from __future__ import annotations

import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import scipy.linalg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import make_golden_exact as GE  # noqa: E402
import make_golden_exact_grad as GG  # noqa: E402
from oracle import lfm_exact as E  # noqa: E402

LD = E.LD
ILL = GG.ILL
MAX_DROPPED = GE.MAX_DROPPED
OUTLIER = 17          # the observation of the C1 problem moved by 30 obs_stddev
FIT_ITERS = 5
FIT_LR = 0.01
OUT = os.path.join(HERE, "exact_loo.npz")


def value_rule(rel):
    """make_golden_exact.rtol_of on a relative error: (rtol, dropped)."""
    if not rel <= GE.NORTH_STAR:
        return float("nan"), True
    return min(GE.NORTH_STAR, max(GE.PROJECT_RTOL, 8 * rel)), False


def loo_parts(a, Sinv, y, dtype):
    """(value, mean, var, c, b, u, W_loo, max z^2) from a = S^{-1} r and S^{-1} in `dtype`."""
    a, Sinv = np.asarray(a, dtype=dtype), np.asarray(Sinv, dtype=dtype)
    y = np.asarray(y, dtype=dtype).reshape(-1)
    k = np.diagonal(Sinv).copy()
    z2 = a * a / k
    half = dtype(1) / 2
    value = np.sum(-half * np.log(2 * dtype(np.pi)) + half * np.log(k) - half * z2)
    b = a / k
    c = (1 + z2) / (2 * k)
    u = Sinv @ b
    M = (Sinv * c[None, :]) @ Sinv
    W = -2 * M + np.outer(u, a) + np.outer(a, u)
    return value, y - b, 1 / k, c, b, u, W, float(np.max(z2))


def loo_exact(ex, x, y, D, B, sd, perm=None):
    """The LOO record of mll_grad_exact's result `ex` in long double; `perm` repeats the
    factorisation and inverse on the symmetric permutation (the same numbers in exact arithmetic,
    through different roundings)."""
    Sig, r = ex["Sigma"], ex["r"]
    if perm is not None:
        Sig, r = Sig[np.ix_(perm, perm)], r[perm]
    a, W, _, _ = E.w_exact(Sig, r)
    Sinv = np.outer(a, a) - W
    if perm is not None:
        inv = np.argsort(perm)
        a, Sinv = a[inv], Sinv[np.ix_(inv, inv)]
    value, mean, var, _, b, u, Wl, z2 = loo_parts(a, Sinv, y, LD)
    g = E.contract_grad(ex["blocks"], Wl, u, x, D, B, sd)
    return dict(value=float(value), mean=mean.astype(np.float64), var=var.astype(np.float64),
                babs=np.abs(b).astype(np.float64), grad=g, max_z2=z2)


def loo_fp64(ex, x, y, D, B, sd):
    """The fp64 restatement: scipy's Cholesky and inverse on the correctly rounded Sigma and r."""
    Sig, r = ex["Sigma"].astype(np.float64), ex["r"].astype(np.float64)
    cf = scipy.linalg.cho_factor(Sig, lower=True, check_finite=False)
    a = scipy.linalg.cho_solve(cf, r, check_finite=False)
    Sinv = scipy.linalg.cho_solve(cf, np.eye(Sig.shape[0]), check_finite=False)
    value, mean, var, _, _, u, Wl, _ = loo_parts(a, Sinv, y, np.float64)
    g = E.contract_grad(ex["blocks"], Wl, u, x, D, B, sd, dtype=np.float64)
    return dict(value=float(value), mean=mean, var=var, grad=g)


def nan_record(n, G):
    nan = np.full(3 * G + 2, np.nan)
    row = np.full(n, np.nan)
    return dict(loo=np.nan, loo_fp64=np.nan, loo_fp64_err=np.nan, loo_rtol=np.nan, mean=row,
                var=row, mean_fp64_err=np.nan, mean_rtol=np.nan, var_fp64_err=np.nan,
                var_rtol=np.nan,
                grad=nan, scale=nan, grad_fp64=nan, grad_fp64_err=np.nan, grad_rtol=np.nan,
                truth_err=np.nan, max_z2=np.nan, dropped=False)


def finish(ex, x, y, D, B, sd):
    """The stored record of one problem from mll_grad_exact's result."""
    y = np.asarray(y, np.float64).reshape(-1)
    n = x.shape[0]
    t = loo_exact(ex, x, y, D, B, sd)
    t2 = loo_exact(ex, x, y, D, B, sd, perm=np.arange(n)[::-1].copy())
    la = loo_fp64(ex, x, y, D, B, sd)
    mscale = np.abs(y) + t["babs"]
    errs = dict(loo=abs(la["value"] - t["value"]) / abs(t["value"]),
                mean=float(np.max(np.abs(la["mean"] - t["mean"]) / mscale)),
                var=float(np.max(np.abs(la["var"] - t["var"]) / t["var"])),
                grad=E.grad_error(la["grad"], t["grad"]))
    rt = {k: value_rule(v) for k, v in errs.items() if k != "grad"}
    rt["grad"] = GG.grad_rtol_of(errs["grad"])
    dropped = any(d for _, d in rt.values())
    tol = {k: (1e-9 if dropped else v[0]) for k, v in rt.items()}
    tol["grad"] = GG.PROJECT_GRAD_RTOL if dropped else rt["grad"][0]
    g, g2, sc = GG.pack(t["grad"]), GG.pack(t2["grad"]), GG.pack(t["grad"], "scale_")
    truth = max(abs(t["value"] - t2["value"]) / (tol["loo"] * abs(t["value"])),
                float(np.max(np.abs(t["mean"] - t2["mean"]) / (tol["mean"] * mscale))),
                float(np.max(np.abs(t["var"] - t2["var"]) / (tol["var"] * t["var"]))),
                float(np.max(np.abs(g - g2) / (tol["grad"] * sc + 1e-10 * np.abs(g)))))
    # extended precision was sufficient: two elimination orders agree to 1e-3 of every bound
    assert truth <= 1e-3, truth
    return dict(loo=t["value"], loo_fp64=la["value"], loo_rtol=rt["loo"][0], mean=t["mean"],
                var=t["var"], mean_fp64_err=errs["mean"], mean_rtol=rt["mean"][0],
                var_fp64_err=errs["var"], var_rtol=rt["var"][0], grad=g, scale=sc,
                grad_fp64=GG.pack(la["grad"]), grad_fp64_err=errs["grad"],
                grad_rtol=rt["grad"][0], truth_err=truth, max_z2=t["max_z2"], dropped=dropped,
                loo_fp64_err=errs["loo"])


def say(tag, rec, t0):
    print(f"{tag}: loo={rec['loo']!r} fp64 err value={rec['loo_fp64_err']:.1e} "
          f"mean={rec['mean_fp64_err']:.1e} var={rec['var_fp64_err']:.1e} "
          f"grad={rec['grad_fp64_err']:.1e} truth={rec['truth_err']:.1e} "
          f"max z2={rec['max_z2']:.0f} ({time.perf_counter() - t0:.0f} s)", flush=True)


def sub_case(r):
    t0 = time.perf_counter()
    x, y, sub = GE.sub_problem(GE.restart_models()[r])
    D, S, B, l, sd, jit = GG.hyp_of(sub)
    tabs = E.GridTables(x[:256, 0], D, S, l, range(4), grad=True)
    ex = E.mll_grad_exact(x, y, D, S, B, l, sd, jit, tables=tabs)
    rec = finish(ex, x, y, D, B, sd)
    say(f"sub r{r}", rec, t0)
    return rec


def una_case(q):
    t0 = time.perf_counter()
    x, _, (D, S, B, l, sd, jit) = GG.una_problem(ILL[q])
    with np.load(os.path.join(HERE, "exact_grad.npz"), allow_pickle=False) as g:
        y = np.ascontiguousarray(g["una_y"][q])
    rec = finish(E.mll_grad_exact(x, y, D, S, B, l, sd, jit), x, y, D, B, sd)
    say(f"una r{ILL[q]}", rec, t0)
    return rec


def mix_case(q):
    t0 = time.perf_counter()
    x, y, (D, S, B, l, sd, jit) = GG.mix_problem(ILL[q])
    ex = E.mll_grad_exact(x, y, D, S, B, l, sd, jit)
    if ex.get("not_pd"):
        print(f"mix r{ILL[q]}: Sigma is not PD", flush=True)
        return nan_record(x.shape[0], len(D))
    rec = finish(ex, x, y, D, B, sd)
    say(f"mix r{ILL[q]}", rec, t0)
    return rec


def c1_problem(outlier):
    from dis_project_amd import configs

    w = configs.c1_p53()
    x = np.ascontiguousarray(w.data.X)
    y = np.ascontiguousarray(w.data.y.reshape(-1)).copy()
    if outlier:
        y[OUTLIER] += 30.0 * float(w.model.obs_stddev)
    return x, y, w.model


def c1_case(outlier):
    t0 = time.perf_counter()
    x, y, model = c1_problem(outlier)
    D, S, B, l, sd, jit = GG.hyp_of(model)
    rec = finish(E.mll_grad_exact(x, y, D, S, B, l, sd, jit), x, y, D, B, sd)
    rec["y"] = y
    say(f"c1 outlier={outlier}", rec, t0)
    return rec


class HostLOO:
    """CustomConjLOOCV(negative=True).value_and_grad restated on the host: the long double truth
    or the fp64 restatement, for trainer.JaxTrainer."""

    def __init__(self, exact):
        self.exact = exact

    def value_and_grad(self, model, data):
        x = np.ascontiguousarray(data.X)
        y = np.ascontiguousarray(data.y.reshape(-1))
        D, S, B, l, sd, jit = GG.hyp_of(model)
        G = len(D)
        ex = E.mll_grad_exact(x, y, D, S, B, l, sd, jit)
        got = loo_exact(ex, x, y, D, B, sd) if self.exact else loo_fp64(ex, x, y, D, B, sd)
        g = -GG.pack(got["grad"])
        return -got["value"], {"true_d": g[:G], "true_s": g[G:2 * G], "true_b": g[2 * G:3 * G],
                               "l": float(g[3 * G]), "obs_stddev": float(g[3 * G + 1])}


def fit_case(exact):
    from dis_project_amd import configs
    from dis_project_amd.trainer import JaxTrainer, adam

    w = configs.c1_p53()
    tr = JaxTrainer(w.model, HostLOO(exact), w.data, adam(FIT_LR), num_iters=FIT_ITERS)
    _, hist = tr.fit(fix_params=False)
    print(f"fit exact={exact}: {hist.tolist()}", flush=True)
    return np.asarray(hist, np.float64)


def make():
    with ProcessPoolExecutor(int(os.environ.get("GOLDEN_THREADS", "8"))) as ex:
        sub = ex.map(sub_case, range(GE.RESTARTS))
        una = ex.map(una_case, range(len(ILL)))
        mix = ex.map(mix_case, range(len(ILL)))
        c1 = ex.map(c1_case, (False, True))
        fit = ex.map(fit_case, (True, False))
        groups = {"sub": list(sub), "una": list(una), "mix": list(mix), "c1": list(c1)}
        fit = list(fit)
    out = {"ill": np.array(ILL, np.int64), "outlier": np.int64(OUTLIER)}
    keys = [k for k in nan_record(1, 1) if k != "dropped"]
    for pre, recs in groups.items():
        for key in keys:
            out[f"{pre}_{key}"] = np.array([s[key] for s in recs], np.float64)
        bad = np.array([i for i, s in enumerate(recs) if s["dropped"]], np.int64)
        if pre == "sub":
            out["sub_dropped"] = bad
            assert bad.size <= MAX_DROPPED and not set(bad) & {0, 1, 5, 10, 29}, bad
        else:
            assert bad.size == 0, (pre, bad)
    out["c1_y"] = np.stack([s["y"] for s in groups["c1"]])
    assert np.isnan(out["mix_loo"]).tolist() == [True, True, False, False]
    out["fit_losses"], out["fit_losses_fp64"] = fit
    dev = float(np.max(np.abs(fit[1] - fit[0]) / np.abs(fit[0])))
    rtol, dropped = value_rule(dev)
    assert not dropped
    out["fit_dev"], out["fit_rtol"] = np.float64(dev), np.float64(rtol)
    print(f"dropped sub={out['sub_dropped'].tolist()} worst loo_rtol="
          f"{np.nanmax(out['sub_loo_rtol']):.0e} grad_rtol={np.nanmax(out['sub_grad_rtol']):.0e} "
          f"fit dev={dev:.1e}")
    np.savez_compressed(OUT, **out)
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    make()

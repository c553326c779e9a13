"""The mid-size batched posterior (lfm_mbatch_posterior_f64) against the path such problems took
before it: 15 problems on 5-gene grids at n = 160, 320, 640 and 1020 (T = 32, 64, 128, 204; the
problems of scripts/mid_batch_rate.py, data variances v ~ U(0.01, 0.05)).
  latent  latent marginals at generate_test_times(100): diag_add = jitter, cov == NULL
  gene    gene predictions with the covariance at generate_test_times_pred(20, 5): diag_add =
          obs_stddev^2
  (a) ONE lfm_mbatch_posterior_f64 call on the resident batch, all problems at once;
  (b) the per-problem loop of lfm_posterior_f64 over the same problems — what predicting after
      a MidBatchTrainer fit did (one synchronous call per problem, x / y uploaded each time; it
      always forms the m x m covariance).
(a) and (b) alternate in one process: warm-up calls, then the median of synchronous calls by the
host clock. The kernel time per class (lfm_profile_read) of one batched call comes from a
separate profiled pass. Results: one JSON document (--out, default profiles/mid_predict.json).
    python scripts/mid_predict_rate.py [--reps 20] [--problems 15] [--sizes 160,320,640,1020]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dis_project_amd import _lib  # noqa: E402
from dis_project_amd.dataset import (generate_test_times, generate_test_times_pred,  # noqa: E402
                                     grid_inputs)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--problems", type=int, default=15)
ap.add_argument("--genes", type=int, default=5)
ap.add_argument("--sizes", default="160,320,640,1020")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.out is None:
    name = "mid_predict.json" if args.problems == 15 else f"mid_predict_p{args.problems}.json"
    args.out = os.path.join(ROOT, "profiles", name)

ctx = _lib.get_context(0)
lib, h, dptr = ctx.lib, ctx.handle, _lib.dptr
MID = ["mid_fill", "mid_column", "mid_inverse", "mid_pairs", "mid_finish"]
L, OBS, JIT = 2.2, 0.9, 1e-4


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def one_size(n):
    G, P = args.genes, args.problems
    assert n % G == 0
    T = n // G
    xs, ys, vs, hyps, vecs = [], [], [], [], []
    for p in range(P):
        rng = np.random.default_rng(n * 100 + p)
        D, S, B = rng.uniform(0.2, 1.0, G), rng.uniform(0.5, 1.5, G), rng.uniform(0.01, 0.1, G)
        xs.append(np.ascontiguousarray(grid_inputs(G, T)))
        ys.append(np.repeat(B / D, T) + 0.5 * rng.standard_normal(n))
        vs.append(rng.uniform(0.01, 0.05, n))
        hyps.append(_lib.HypArgs(D, S, B, L, OBS, JIT))
        vecs.append(np.concatenate([D, S, B]))
    packed = np.concatenate(vecs + [np.tile([L, OBS, JIT], P)])
    dv = np.concatenate(vs)
    probs = (_lib.LfmProblem * P)()
    for p in range(P):
        probs[p].x, probs[p].y, probs[p].n = xs[p].ctypes.data, ys[p].ctypes.data, n
        probs[p].hyp.num_genes = G
    mb = ctypes.c_void_p()
    ctx.check(lib.lfm_mbatch_create(h, P, probs, ctypes.byref(mb)))
    st = np.zeros(P, np.int32)
    res = dict(n=n, num_genes=G, problems=P)
    try:
        for name, t1, dadd, want_cov in (
                ("latent", generate_test_times(100), JIT, False),
                ("gene", generate_test_times_pred(20, G), OBS ** 2, True)):
            t1 = np.ascontiguousarray(t1, np.float64)
            m = t1.shape[0]
            tt = np.ascontiguousarray(np.tile(t1, (P, 1)))
            ms = np.full(P, m, np.int64)
            dadds = np.full(P, dadd)
            mean_b, var_b = np.empty(P * m), np.empty(P * m)
            cov_b = np.empty(P * m * m) if want_cov else None
            mean_l, cov_l = np.empty((P, m)), np.empty((P, m, m))

            def batch():
                ctx.check(lib.lfm_mbatch_posterior_f64(
                    h, mb, dptr(packed), dptr(dv), dptr(dadds), dptr(ms), dptr(tt), dptr(mean_b),
                    dptr(var_b), dptr(cov_b) if want_cov else None, dptr(st)))

            def loop():
                for p in range(P):
                    ctx.check(lib.lfm_posterior_f64(h, dptr(xs[p]), dptr(ys[p]), n, dptr(vs[p]),
                                                    float(dadd), dptr(t1), m, hyps[p].ref,
                                                    dptr(mean_l[p]), dptr(cov_l[p])))

            for _ in range(args.warmup):
                batch()
                loop()
            tb, tl = [], []
            for _ in range(args.reps):  # alternating
                tb.append(timed(batch))
                tl.append(timed(loop))
            b_ms, l_ms = float(np.median(tb)), float(np.median(tl))
            ctx.profile(True, classes=MID)
            ctx.profile_reset()
            batch()
            stats = ctx.profile_read()
            ctx.profile(False)
            kern = {k: dict(ms=stats[k]["total_ms"], launches=stats[k]["launches"])
                    for k in MID if k in stats}
            var_l = np.diagonal(cov_l, axis1=1, axis2=2)
            r = dict(m=m, with_cov=want_cov, batch_ms=b_ms, loop_ms=l_ms,
                     ratio_loop_over_batch=l_ms / b_ms, batch_us_per_problem=1e3 * b_ms / P,
                     loop_us_per_problem=1e3 * l_ms / P,
                     max_diff_mean_over_largest=float(np.max(np.abs(mean_b.reshape(P, m) - mean_l))
                                                      / np.max(np.abs(mean_l))),
                     max_diff_var_over_largest=float(np.max(np.abs(var_b.reshape(P, m) - var_l))
                                                     / np.max(np.abs(var_l))),
                     kernels=kern, kernel_ms=sum(k["ms"] for k in kern.values()),
                     launches=sum(k["launches"] for k in kern.values()))
            if want_cov:
                r["max_diff_cov_over_largest"] = float(
                    np.max(np.abs(cov_b.reshape(P, m, m) - cov_l)) / np.max(np.abs(cov_l)))
            res[name] = r
        print(json.dumps(res), flush=True)
    finally:
        lib.lfm_mbatch_destroy(mb)
    return res


out = dict(what="mid-size batched posterior (lfm_mbatch_posterior_f64) against the per-problem "
                f"loop of lfm_posterior_f64; {args.problems} problems per size; latent marginals "
                "at generate_test_times(100), gene predictions with the covariance at "
                f"generate_test_times_pred(20, {args.genes}); medians of {args.reps} alternating "
                "synchronous calls by the host clock; kernel times from HIP events "
                "(lfm_profile_*) in a separate pass",
           sizes=[one_size(int(n)) for n in args.sizes.split(",")])
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print("wrote", args.out)

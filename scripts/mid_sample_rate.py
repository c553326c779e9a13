"""Joint samples and held-out log density on the mid-size resident batch
(lfm_mbatch_predictive_f64) against the route the same work took before it: problems on 5-gene
grids at n = 160, 320, 640 and 1020 (the problems of scripts/mid_predict_rate.py), gene rows at
generate_test_times_pred(20, 5) and (80, 5): m = 100 and 400; S's diagonal obs_stddev^2,
cov_add = jitter (multi_gene_predict's distribution).
  draw16 / draw1024  nsamp = 16 and 1024 joint samples of every problem
  logp               the log density of one held-out vector per problem
  (a) ONE lfm_mbatch_predictive_f64 call: the covariance never leaves the device;
  (b) lfm_mbatch_posterior_f64 with the covariance, the jitter added on the host, then per
      problem one lfm_mvn_sample_f64 (for logp: lfm_log_prob_f64), each of which uploads the
      m x m matrix again and runs the large-N blocked factorisation on it.
(a) and (b) alternate in one process: warm-up calls, then the median of synchronous calls by the
host clock. The kernel time per class (lfm_profile_read) of one batched call comes from a
separate profiled pass; the product's share of the call and its fraction of the 78.6 TFLOP/s
fp64 matrix peak on nsamp sum m^2 flops are derived from it. Results: one JSON document (--out,
default profiles/mid_sample.json).
    python scripts/mid_sample_rate.py [--reps 20] [--problems 15] [--sizes 160,320,640,1020]"""
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
from dis_project_amd.dataset import generate_test_times_pred, grid_inputs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--problems", type=int, default=15)
ap.add_argument("--genes", type=int, default=5)
ap.add_argument("--sizes", default="160,320,640,1020")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.out is None:
    name = "mid_sample.json" if args.problems == 15 else f"mid_sample_p{args.problems}.json"
    args.out = os.path.join(ROOT, "profiles", name)

ctx = _lib.get_context(0)
lib, h, dptr = ctx.lib, ctx.handle, _lib.dptr
CLASSES = ["mid_fill", "mid_column", "mid_inverse", "mid_finish", "sample_randn", "sample_trmm"]
L, OBS, JIT = 2.2, 0.9, 1e-4
PEAK = 78.6e12  # fp64 matrix, FLOP/s


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def one_size(n):
    G, P = args.genes, args.problems
    assert n % G == 0
    T = n // G
    xs, ys, vs, vecs = [], [], [], []
    for p in range(P):
        rng = np.random.default_rng(n * 100 + p)
        D, S, B = rng.uniform(0.2, 1.0, G), rng.uniform(0.5, 1.5, G), rng.uniform(0.01, 0.1, G)
        xs.append(np.ascontiguousarray(grid_inputs(G, T)))
        ys.append(np.repeat(B / D, T) + 0.5 * rng.standard_normal(n))
        vs.append(rng.uniform(0.01, 0.05, n))
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
    res = dict(n=n, num_genes=G, problems=P, shapes=[])
    try:
        for per_gene in (20, 80):
            t1 = np.ascontiguousarray(generate_test_times_pred(per_gene, G), np.float64)
            m = t1.shape[0]
            tt = np.ascontiguousarray(np.tile(t1, (P, 1)))
            ms = np.full(P, m, np.int64)
            dadds, cadds = np.full(P, OBS ** 2), np.full(P, JIT)
            seeds = np.arange(1, P + 1, dtype=np.uint64)
            mean_b, mean_l = np.empty(P * m), np.empty(P * m)
            cov_l = np.empty(P * m * m)
            eye = np.eye(m) * JIT
            ystar = np.empty(P * m)
            for nsamp in (16, 1024, 0):
                key = f"draw{nsamp}" if nsamp else "logp"
                x_b = np.empty(max(nsamp, 1) * P * m)
                x_l = np.empty((P, max(nsamp, 1), m))
                lp_b, lp_l = np.empty(P), np.empty(P)

                def batch():
                    ctx.check(lib.lfm_mbatch_predictive_f64(
                        h, mb, dptr(packed), dptr(dv), dptr(dadds), dptr(ms), dptr(tt),
                        dptr(cadds), None if nsamp else dptr(ystar), None if nsamp else dptr(lp_b),
                        dptr(seeds) if nsamp else None, 0, nsamp, dptr(mean_b),
                        dptr(x_b) if nsamp else None, dptr(st)))

                def loop():
                    ctx.check(lib.lfm_mbatch_posterior_f64(
                        h, mb, dptr(packed), dptr(dv), dptr(dadds), dptr(ms), dptr(tt),
                        dptr(mean_l), None, dptr(cov_l), dptr(st)))
                    for p in range(P):
                        scale = cov_l[p * m * m:(p + 1) * m * m].reshape(m, m) + eye
                        loc = mean_l[p * m:(p + 1) * m]
                        if nsamp:
                            ctx.check(lib.lfm_mvn_sample_f64(h, dptr(loc), dptr(scale), m, m,
                                                             int(seeds[p]), 0, nsamp,
                                                             dptr(x_l[p])))
                        else:
                            out = ctypes.c_double(0.0)
                            ctx.check(lib.lfm_log_prob_f64(h, dptr(loc), dptr(scale), m, m,
                                                           dptr(ystar[p * m:(p + 1) * m]),
                                                           ctypes.byref(out)))
                            lp_l[p] = out.value

                if not nsamp:  # held-out values: the mean + 0.5 N(0, 1)
                    loop_mean = np.empty(P * m)
                    ctx.check(lib.lfm_mbatch_posterior_f64(
                        h, mb, dptr(packed), dptr(dv), dptr(dadds), dptr(ms), dptr(tt),
                        dptr(loop_mean), None, dptr(cov_l), dptr(st)))
                    ystar[:] = loop_mean + 0.5 * np.random.default_rng(n + m).standard_normal(P * m)
                for _ in range(args.warmup):
                    batch()
                    loop()
                tb, tl = [], []
                for _ in range(args.reps):  # alternating
                    tb.append(timed(batch))
                    tl.append(timed(loop))
                b_ms, l_ms = float(np.median(tb)), float(np.median(tl))
                ctx.profile(True, classes=CLASSES)
                ctx.profile_reset()
                batch()
                stats = ctx.profile_read()
                ctx.profile(False)
                kern = {k: dict(ms=stats[k]["total_ms"], launches=stats[k]["launches"])
                        for k in CLASSES if k in stats}
                r = dict(what=key, m=m, nsamp=nsamp, batch_ms=b_ms, loop_ms=l_ms,
                         ratio_loop_over_batch=l_ms / b_ms, kernels=kern,
                         kernel_ms=sum(k["ms"] for k in kern.values()),
                         launches=sum(k["launches"] for k in kern.values()))
                if nsamp:
                    xb = x_b.reshape(P, nsamp, m)
                    r["max_diff_samples_over_largest"] = float(np.max(np.abs(xb - x_l))
                                                               / np.max(np.abs(x_l)))
                    prod_ms = kern["sample_trmm"]["ms"]
                    r["product_ms"] = prod_ms
                    r["product_share_of_call"] = prod_ms / b_ms
                    r["product_fraction_of_fp64_matrix_peak"] = \
                        (nsamp * P * m * m) / (prod_ms * 1e-3) / PEAK if prod_ms > 0 else None
                else:
                    r["max_diff_logp_over_largest"] = float(np.max(np.abs(lp_b - lp_l))
                                                            / np.max(np.abs(lp_l)))
                res["shapes"].append(r)
        print(json.dumps(res), flush=True)
    finally:
        lib.lfm_mbatch_destroy(mb)
    return res


out = dict(what="joint samples and held-out log density on the mid-size resident batch "
                "(lfm_mbatch_predictive_f64) against lfm_mbatch_posterior_f64 with the covariance "
                "followed by one lfm_mvn_sample_f64 / lfm_log_prob_f64 per problem; "
                f"{args.problems} problems per size; gene rows, m = 100 and 400; nsamp = 16 and "
                f"1024, and logp alone; medians of {args.reps} alternating synchronous calls by "
                "the host clock; kernel times from HIP events (lfm_profile_*) in a separate pass; "
                "the product's fraction of the 78.6 TFLOP/s fp64 matrix peak on nsamp sum m^2 flops",
           sizes=[one_size(int(n)) for n in args.sizes.split(",")])
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print("wrote", args.out)

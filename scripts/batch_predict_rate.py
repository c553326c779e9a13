"""Batched posterior predictors against the per-problem loop, on the 15 C5 ablation problems
(configs.c5_ablations: n = 28, G = 4):
  (a) latent marginals at generate_test_times(100) (m = 100, no covariance);
  (b) gene prediction at generate_test_times_pred(100, G) (m = 400) with the covariance.
Each case is timed as ONE lfm_batch_posterior_f64 call on the resident batch and as the loop of
15 lfm_posterior_f64 calls that ExactLFM._posterior makes (x / y / t uploaded per call, the
large-N Schur-complement chain), in the same process, the two alternating: warm-up calls, then
the median of synchronous calls by the host clock (both calls synchronise before they return).
The batched call's kernel time (HIP events around its launches) comes from a separate profiled
pass. Results: one JSON document (--out, default profiles/batch_predict.json).
    python scripts/batch_predict_rate.py [--reps 40] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dis_project_amd import _lib, configs, dataset as ds, farm, predict  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_predict.json"))
args = ap.parse_args()

ctx = _lib.get_context(0)
lib, h, dptr = ctx.lib, ctx.handle, _lib.dptr
datas = [ds.SyntheticP53Data(replicate=0, seed=seed,
                             selected_genes=[g for g in ds.BARENCO_GENES if g != drop])
         for seed in (10, 11, 12) for drop in ds.BARENCO_GENES]
models = [w.model for w in configs.c5_ablations()]
xyv = []
for d in datas:
    x, y, v = ds.dataset_3d(d)
    xyv.append((np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y).reshape(-1),
                np.ascontiguousarray(v).reshape(-1)))
genes = [int(m.num_genes) for m in models]
ev = farm.BatchEvaluator(ctx, [ds.Dataset(x, y) for x, y, _ in xyv])
hyp = ev.pack(models)  # registers the batch for this gene layout
batch = ev.batch
dv = np.concatenate([v for _, _, v in xyv])
hyps = [m.hyp() for m in models]


def case(name, t, dadd, want_cov):
    t = np.ascontiguousarray(t)
    m = t.shape[0]
    tp, mp = predict.pack_test_inputs(t, genes)
    dadd = np.ascontiguousarray(dadd, dtype=np.float64)
    mean, var = np.empty(int(mp.sum())), np.empty(int(mp.sum()))
    cov = np.empty(int((mp * mp).sum())) if want_cov else None
    st = np.zeros(len(genes), np.int32)
    lm, lc = np.empty((len(genes), m)), np.empty((len(genes), m, m))

    def batched():
        ctx.check(lib.lfm_batch_posterior_f64(h, batch, dptr(hyp), dptr(dv), dptr(dadd), dptr(mp),
                                              dptr(tp), dptr(mean), dptr(var),
                                              dptr(cov) if want_cov else None, dptr(st)))

    def loop():
        for k, ((x, y, v), hp) in enumerate(zip(xyv, hyps)):
            ctx.check(lib.lfm_posterior_f64(h, dptr(x), dptr(y), x.shape[0], dptr(v),
                                            float(dadd[k]), dptr(t), m, hp.ref, dptr(lm[k]),
                                            dptr(lc[k])))

    for _ in range(args.warmup):
        batched()
        loop()
    tb, tl = [], []
    for _ in range(args.reps):  # alternating: the same conditions for both
        t0 = time.perf_counter()
        batched()
        t1 = time.perf_counter()
        loop()
        t2 = time.perf_counter()
        tb.append(t1 - t0)
        tl.append(t2 - t1)
    # the two paths computed the same thing (the tests' tolerance)
    ref_var = np.stack([np.diag(c) for c in lc]).reshape(-1)
    assert np.max(np.abs(mean - lm.reshape(-1))) <= 1e-9 * np.max(np.abs(lm)) + 1e-12
    assert np.max(np.abs(var - ref_var)) <= 1e-9 * np.max(np.abs(ref_var)) + 1e-12
    if want_cov:
        assert np.max(np.abs(cov - lc.reshape(-1))) <= 1e-9 * np.max(np.abs(lc)) + 1e-12
    ctx.profile(True, classes=["small_post"])
    ctx.profile_reset()
    for _ in range(10):
        batched()
    kern = ctx.profile_read()["small_post"]
    ctx.profile(False)
    us = lambda a: float(np.median(a)) * 1e6  # noqa: E731
    res = dict(case=name, problems=len(genes), n=int(xyv[0][0].shape[0]), m=m, cov=bool(want_cov),
               reps=args.reps, batched_us=us(tb), loop_us=us(tl),
               batched_us_min=float(np.min(tb)) * 1e6, loop_us_min=float(np.min(tl)) * 1e6,
               batched_us_p90=float(np.percentile(tb, 90)) * 1e6,
               loop_us_p90=float(np.percentile(tl, 90)) * 1e6,
               speedup=us(tl) / us(tb),
               batched_kernel_us=kern["total_ms"] * 1e3 / max(1, kern["launches"]))
    print(json.dumps(res), flush=True)
    return res


try:
    out = [case("latent_marginals", ds.generate_test_times(100), [m.jitter for m in models], False),
           case("gene_predict_cov", ds.generate_test_times_pred(100, 4),
                [m.obs_stddev ** 2 for m in models], True)]
finally:
    ev.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(dict(script="scripts/batch_predict_rate.py", device="MI355X", cases=out), f, indent=1)
    f.write("\n")

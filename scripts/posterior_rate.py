"""The resident posterior against the call it replaces, at N = 16384 (the C2 data and base point)
and N = 4096 (the same recipe, 16 genes):
  (a) lfm_posterior_f64 — the yardstick: the whole Schur-complement factorisation per call — at
      m = 128 and m = 384 gene rows (the multiples of num_genes next to the notebooks' 100 and
      400 test times; mean_function needs m % num_genes == 0);
  (b) lfm_post_create once, then lfm_post_predict_f64 at the same m with the covariance;
  (c) var-only predicts at m = 128, 384, 16384 and 65536 (lfm_posterior_f64 has no counterpart
      for the last two: n + m <= 131072 and an m x m output).
(a) and (b) alternate in one process: warm-up calls, then the median of synchronous calls by the
host clock. The event time of the two solve kernels (post_panel, post_update), summed over one
predict, comes from a separate profiled pass (lfm_profile_*); their share of the fp64 matrix spec
is taken from the algorithmic N^2 m flop. Beside each measured ratio stands the flop ceiling
N / 3m. Results: one JSON document (--out, default profiles/posterior_solve.json).
    python scripts/posterior_rate.py [--reps 5] [--sizes 16384,4096] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dis_project_amd import _lib, configs  # noqa: E402

SPEC_F64_MATRIX = 78.6e12  # MI355X dense fp64 matrix, flop/s

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--sizes", default="16384,4096")
ap.add_argument("--cov-m", default="128,384")
ap.add_argument("--var-m", default="128,384,16384,65536")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "posterior_solve.json"))
args = ap.parse_args()

ctx = _lib.get_context(0)
lib, h, dptr = ctx.lib, ctx.handle, _lib.dptr


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def test_rows(m, G, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack((rng.uniform(0, 12, m),
                                          np.repeat(np.arange(G), m // G).astype(float),
                                          np.ones(m)), -1))


def one_size(N):
    G = N // 256
    w = configs.c2(G=G, T=256)
    x = np.ascontiguousarray(w.data.X, dtype=np.float64).reshape(-1, 3)
    y = np.ascontiguousarray(w.data.y, dtype=np.float64).reshape(-1)
    assert x.shape[0] == N
    hyp = w.model.hyp()
    dadd = float(w.model.obs_stddev) ** 2
    res = dict(N=N, num_genes=G, cov=[], var_only=[])

    post = ctypes.c_void_p()
    t0 = time.perf_counter()
    ctx.check(lib.lfm_post_create(h, dptr(x), dptr(y), N, None, dadd, hyp.ref, ctypes.byref(post)))
    res["create_ms_first"] = (time.perf_counter() - t0) * 1e3

    def kernels(fn):
        """post_panel + post_update event time of one call of fn, ms, and their launches."""
        ctx.profile(True, classes=["post_panel", "post_update"])
        ctx.profile_reset()
        fn()
        st = ctx.profile_read()
        ctx.profile(False)
        return (st["post_panel"]["total_ms"], st["post_update"]["total_ms"],
                st["post_panel"]["launches"] + st["post_update"]["launches"])

    try:
        for m in (int(v) for v in args.cov_m.split(",")):
            t = test_rows(m, G, m)
            mean, cov = np.empty(m), np.empty((m, m))
            mean2, var2, cov2 = np.empty(m), np.empty(m), np.empty((m, m))

            def yard():
                ctx.check(lib.lfm_posterior_f64(h, dptr(x), dptr(y), N, None, dadd, dptr(t), m,
                                                hyp.ref, dptr(mean), dptr(cov)))

            def resident():
                ctx.check(lib.lfm_post_predict_f64(h, post, dptr(t), m, dptr(mean2), dptr(var2),
                                                   dptr(cov2)))

            for _ in range(args.warmup):
                yard()
                resident()
            ty, tr = [], []
            for _ in range(args.reps):  # alternating
                ty.append(median_ms(yard, 1))
                tr.append(median_ms(resident, 1))
            yard_ms, res_ms = float(np.median(ty)), float(np.median(tr))
            pan, upd, launches = kernels(resident)
            flop = float(N) * N * m
            err = float(np.max(np.abs(cov2 - cov)) / np.max(np.abs(cov)))
            res["cov"].append(dict(
                m=m, posterior_f64_ms=yard_ms, predict_ms=res_ms, ratio=yard_ms / res_ms,
                flop_ceiling_N_over_3m=N / (3.0 * m), panel_ms=pan, update_ms=upd,
                solve_launches=launches, other_ms=res_ms - pan - upd,
                solve_frac_of_spec=flop / ((pan + upd) * 1e-3) / SPEC_F64_MATRIX,
                max_rel_diff_cov=err))
            print(json.dumps(res["cov"][-1]), flush=True)
        for m in (int(v) for v in args.var_m.split(",")):
            t = test_rows(m, G, m)
            mean2, var2 = np.empty(m), np.empty(m)

            def marg():
                ctx.check(lib.lfm_post_predict_f64(h, post, dptr(t), m, dptr(mean2), dptr(var2),
                                                   None))

            marg()
            ms = median_ms(marg, max(2, args.reps if m <= 16384 else 2))
            pan, upd, launches = kernels(marg)
            flop = float(N) * N * m
            res["var_only"].append(dict(
                m=m, predict_ms=ms, panel_ms=pan, update_ms=upd, solve_launches=launches,
                other_ms=ms - pan - upd,
                solve_frac_of_spec=flop / ((pan + upd) * 1e-3) / SPEC_F64_MATRIX))
            print(json.dumps(res["var_only"][-1]), flush=True)
    finally:
        lib.lfm_post_destroy(post)
    return res


out = dict(what="resident posterior (lfm_post_*) against lfm_posterior_f64; medians of "
                f"{args.reps} alternating synchronous calls by the host clock; kernel times from "
                "HIP events (lfm_profile_*) in a separate pass",
           spec_f64_matrix_flops=SPEC_F64_MATRIX,
           sizes=[one_size(int(n)) for n in args.sizes.split(",")])
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print("wrote", args.out)

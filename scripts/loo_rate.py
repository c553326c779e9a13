"""The leave-one-out CV calls on the C2 grid layout at N in {1024, 4096, 16384} (G = N / 256 genes,
the C2 base point): lfm_loocv_f64 and lfm_loocv_grad_f64 against lfm_mll_grad_f64 on the same
problem (before these calls the only one that paid the bordered factorisation) and, at
N = 4096, against the route that existed without them: lfm_gram_f64 to the host, then scipy's
cho_factor and cho_solve on the identity for diag(S^{-1}) and S^{-1} r.
One process; per case a warm-up call, then the median of synchronous calls by the host clock. The
event time of the product launch alone (kernel class loo_product) and of the small LOO kernels
plus the reductions (class grad) come from a separate profiled pass of lfm_loocv_grad_f64
(lfm_profile_*); the product's share of the fp64 matrix spec is taken from its algorithmic n^3
flop (the lower triangle of an n x n x n product), its issued share from the whole tiles at depth
Np it runs. Results: one JSON document (--out, default profiles/loo_rate.json).
    python scripts/loo_rate.py [--reps 7] [--N 1024,4096,16384] [--host-N 4096] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dis_project_amd import _lib, configs  # noqa: E402

SPEC_F64_MATRIX = 78.6e12  # MI355X dense fp64 matrix, flop/s
FACTOR = ["tables", "gram_grid", "augment", "potrf", "trsm", "syrk", "panel", "syrk_side",
          "finalize"]

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--N", default="1024,4096,16384")
ap.add_argument("--host-N", type=int, default=4096, help="the host route is timed at this N")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loo_rate.json"))
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


cases = []
for N in (int(v) for v in args.N.split(",")):
    G = N // 256
    w = configs.c2(G=G, T=256)
    x = np.ascontiguousarray(w.data.X, dtype=np.float64).reshape(-1, 3)
    y = np.ascontiguousarray(w.data.y, dtype=np.float64).reshape(-1)
    assert x.shape[0] == N
    hyp = w.model.hyp()
    val, gv = np.empty(1), np.empty(3 * G + 2)
    mean, var = np.empty(N), np.empty(N)

    def loo():
        ctx.check(lib.lfm_loocv_f64(h, dptr(x), dptr(y), N, hyp.ref, 1, dptr(val), dptr(mean),
                                    dptr(var)))

    def loo_grad():
        ctx.check(lib.lfm_loocv_grad_f64(h, dptr(x), dptr(y), N, hyp.ref, 1, dptr(val), dptr(gv)))

    def mll_grad():
        ctx.check(lib.lfm_mll_grad_f64(h, dptr(x), dptr(y), N, hyp.ref, 1, dptr(val), dptr(gv)))

    row = dict(N=N, num_genes=G)
    for name, fn in (("mll_grad_ms", mll_grad), ("loocv_ms", loo), ("loocv_grad_ms", loo_grad)):
        fn()
        row[name] = median_ms(fn, args.reps)
    row["loo_value"] = float(val[0])
    ctx.profile(True, classes=FACTOR + ["grad", "loo_product"])
    ctx.profile_reset()
    loo_grad()
    st = ctx.profile_read()
    ctx.profile(False)
    prod = st["loo_product"]["total_ms"]
    row.update(product_ms=prod, product_launches=int(st["loo_product"]["launches"]),
               small_and_reductions_ms=st["grad"]["total_ms"],
               factor_ms=sum(st[k]["total_ms"] for k in FACTOR),
               product_flops=float(N) ** 3,
               product_frac_of_spec=float(N) ** 3 / (prod * 1e-3) / SPEC_F64_MATRIX,
               product_issued_frac_of_spec=st["loo_product"]["issued_flops"] / (prod * 1e-3)
               / SPEC_F64_MATRIX,
               fallbacks=int(ctx.fallbacks))
    if N == args.host_N:
        import scipy.linalg

        def host():
            K = np.empty((N, N))
            d = float(w.model.jitter) + float(w.model.obs_stddev) ** 2
            ctx.check(lib.lfm_gram_f64(h, dptr(x), N, hyp.ref, d, _lib.LFM_UPLO_FULL, dptr(K), N))
            m = np.empty(N)
            ctx.check(lib.lfm_mean_function_f64(h, dptr(x), N, hyp.ref, dptr(m)))
            c = scipy.linalg.cho_factor(K, lower=True, check_finite=False)
            Sinv = scipy.linalg.cho_solve(c, np.eye(N), check_finite=False)
            a = scipy.linalg.cho_solve(c, y - m, check_finite=False)
            k = np.diagonal(Sinv)
            return float(np.sum(-0.5 * np.log(2 * np.pi) + 0.5 * np.log(k) - 0.5 * a * a / k))

        hv = host()
        row["host_route_ms"] = median_ms(host, max(1, min(3, args.reps)))
        row["host_value_rel_diff"] = abs(-hv - row["loo_value"]) / abs(hv)
        row["host_download_bytes"] = 8 * (N * N + N)
        row["ratio_host_over_loocv"] = row["host_route_ms"] / row["loocv_ms"]
    cases.append(row)
    print(json.dumps(row), flush=True)

doc = dict(what="lfm_loocv_f64 and lfm_loocv_grad_f64 against lfm_mll_grad_f64 on the C2 grid "
                "layout; medians of %d synchronous calls by the host clock after a warm-up call; "
                "kernel-class times from HIP events in a separate profiled pass of "
                "lfm_loocv_grad_f64; the host route (lfm_gram_f64 + scipy cho_factor / "
                "cho_solve(I)) at N = %d" % (args.reps, args.host_N),
           spec_f64_matrix_flops=SPEC_F64_MATRIX, cases=cases)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print("wrote", args.out)

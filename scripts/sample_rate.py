"""Joint samples from a resident posterior at N = 16384 (the C2 data and base point):
lfm_post_sample_f64 against the route that exists without it — lfm_post_predict_f64 with the
covariance, then numpy's cholesky and a matmul on the host — for m in {384, 4096, 16384} gene rows
and nsamp in {16, 1024}, on N(mean(t), cov(t) + diag_add I) with diag_add = obs_stddev^2.
One process; per case a warm-up call, then the median of synchronous calls by the host clock (the
host route at m = 16384 is timed once: its factorisation alone takes tens of seconds). The event
times of the kernel classes of one lfm_post_sample_f64 come from a separate profiled pass
(lfm_profile_*): the solve (post_panel, post_update, gram_direct), the factorisation (potrf, trsm,
syrk, panel, augment, finalize), sample_randn and sample_trmm; what is left of the call (the
covariance's own kernel, which has no class, the strided copy, the download and the host side) is
`other_ms`. The product's share of the fp64 matrix spec is taken from its algorithmic
nsamp m^2 flop. Results: one JSON document (--out, default profiles/post_sample.json).
    python scripts/sample_rate.py [--reps 5] [--m 384,4096,16384] [--nsamp 16,1024] [--out FILE]"""
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
SOLVE = ["post_panel", "post_update", "gram_direct"]
FACTOR = ["potrf", "trsm", "syrk", "panel", "augment", "finalize"]
SAMPLE = ["sample_randn", "sample_trmm"]

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--N", type=int, default=16384)
ap.add_argument("--m", default="384,4096,16384")
ap.add_argument("--nsamp", default="16,1024")
ap.add_argument("--host-max-m", type=int, default=16384, help="skip the host route above this m")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "post_sample.json"))
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


N = args.N
G = N // 256
w = configs.c2(G=G, T=256)
x = np.ascontiguousarray(w.data.X, dtype=np.float64).reshape(-1, 3)
y = np.ascontiguousarray(w.data.y, dtype=np.float64).reshape(-1)
assert x.shape[0] == N
hyp = w.model.hyp()
dadd = float(w.model.obs_stddev) ** 2
post = ctypes.c_void_p()
ctx.check(lib.lfm_post_create(h, dptr(x), dptr(y), N, None, dadd, hyp.ref, ctypes.byref(post)))
ctx.check(lib.lfm_post_set_chunk(post, 16384))  # the covariance at m = 16384 in one chunk
cases = []
try:
    for m in (int(v) for v in args.m.split(",")):
        rng = np.random.default_rng(m)
        t = np.ascontiguousarray(np.stack((rng.uniform(0, 12, m),
                                           np.repeat(np.arange(G), m // G).astype(float),
                                           np.ones(m)), -1))
        for nsamp in (int(v) for v in args.nsamp.split(",")):
            mean, out = np.empty(m), np.empty((nsamp, m))
            rcs = []

            def device():
                rcs.append(lib.lfm_post_sample_f64(h, post, dptr(t), m, dadd, 7, 0, nsamp,
                                                   dptr(mean), dptr(out)))

            def host():
                mu, var, cov = np.empty(m), np.empty(m), np.empty((m, m))
                ctx.check(lib.lfm_post_predict_f64(h, post, dptr(t), m, dptr(mu), dptr(var),
                                                   dptr(cov)))
                cov[np.diag_indices(m)] += dadd
                z = np.random.default_rng(7).standard_normal((nsamp, m))
                return mu + z @ np.linalg.cholesky(cov).T

            device()
            ctx.check(rcs[-1])
            dev_ms = median_ms(device, args.reps)
            ctx.profile(True, classes=SOLVE + FACTOR + SAMPLE)
            ctx.profile_reset()
            device()
            st = ctx.profile_read()
            ctx.profile(False)
            ms = {k: st[k]["total_ms"] for k in SOLVE + FACTOR + SAMPLE}
            solve, factor = sum(ms[k] for k in SOLVE), sum(ms[k] for k in FACTOR)
            trmm = ms["sample_trmm"]
            row = dict(m=m, nsamp=nsamp, rc=int(rcs[-1]), finite=bool(np.all(np.isfinite(out))),
                       post_sample_ms=dev_ms, solve_ms=solve, factor_ms=factor,
                       randn_ms=ms["sample_randn"], trmm_ms=trmm,
                       other_ms=dev_ms - solve - factor - ms["sample_randn"] - trmm,
                       trmm_flops=float(nsamp) * m * m,
                       trmm_frac_of_spec=float(nsamp) * m * m / (trmm * 1e-3) / SPEC_F64_MATRIX,
                       trmm_issued_frac_of_spec=st["sample_trmm"]["issued_flops"] / (trmm * 1e-3)
                       / SPEC_F64_MATRIX,
                       download_bytes=8 * (nsamp * m + m))
            if m <= args.host_max_m:
                if m <= 4096:
                    host()
                    row["host_route_ms"] = median_ms(host, max(1, min(3, args.reps)))
                else:
                    row["host_route_ms"] = median_ms(host, 1)  # one call, no warm-up
                row["host_download_bytes"] = 8 * (m * m + 2 * m)
                row["ratio_host_over_device"] = row["host_route_ms"] / dev_ms
            cases.append(row)
            print(json.dumps(row), flush=True)
finally:
    lib.lfm_post_destroy(post)

doc = dict(what="lfm_post_sample_f64 on a resident N = %d model against lfm_post_predict_f64 with "
                "the covariance + numpy cholesky and matmul on the host; medians of %d synchronous "
                "calls by the host clock after a warm-up call (the host route at m > 4096: one "
                "call); kernel-class times from HIP events in a separate pass" % (N, args.reps),
           N=N, num_genes=G, diag_add=dadd, spec_f64_matrix_flops=SPEC_F64_MATRIX, cases=cases)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print("wrote", args.out)

"""Held-out log density on a resident posterior at N = 16384 (the C2 data and base point):
lfm_post_log_prob_f64 against the route that exists without it — lfm_post_predict_f64 with the
covariance, one addition on the diagonal on the host, then lfm_log_prob_f64 once per held-out
vector — for m in {384, 4096, 16384} gene rows and k in {1, 16, 1024} vectors, under
N(mean(t), cov(t) + diag_add I) with diag_add = obs_stddev^2.

Each m is one child process of this script (--case M) under its own time limit; the first child
that fails or runs out of time ends the run with its exit status, and nothing more is started.
Per case a warm-up call, then the median of synchronous calls by the host clock. The host route's
predict and its per-vector lfm_log_prob_f64 are timed apart; above a cap on the vectors timed (1024
up to m = 512, 16 up to m = 4096, 2 above: one vector at m = 16384 uploads 2.1 GB and factors it)
the route's time is composed as predict + k x the median vector, and the row says so
(host_route_composed). The event times of the kernel classes of one lfm_post_log_prob_f64 come from
a separate profiled pass (lfm_profile_*): the solve (post_panel, post_update, gram_direct: the
predict's sweep and the residual rows' sweep share their classes, so `predict_solve_ms`, the same
classes of a profiled lfm_post_predict_f64 with the covariance, stands beside it; the two passes
differ by more than the residual sweep costs at small m, so no difference is reported) and the
factorisation (potrf, trsm, syrk, panel, augment, finalize); what is left of the call (the
covariance's own kernel, the copies, the small kernels without a class, the upload of ystar, the
downloads and the host side) is `other_ms`. Results: one JSON document (--out, default
profiles/post_logp.json).
    python scripts/post_logp_rate.py [--reps 5] [--m 384,4096,16384] [--k 1,16,1024] [--out FILE]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SOLVE = ["post_panel", "post_update", "gram_direct"]
FACTOR = ["potrf", "trsm", "syrk", "panel", "augment", "finalize"]

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--N", type=int, default=16384)
ap.add_argument("--m", default="384,4096,16384")
ap.add_argument("--k", default="1,16,1024")
ap.add_argument("--case", type=int, default=0, help="child: measure this m alone")
ap.add_argument("--rows-out", default="", help="child: where its rows go")
ap.add_argument("--limit", type=int, default=420, help="seconds a child may take")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "post_logp.json"))
args = ap.parse_args()
ks = [int(v) for v in args.k.split(",")]


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def child(m):
    from dis_project_amd import _lib, configs

    ctx = _lib.get_context(0)
    lib, h, dptr = ctx.lib, ctx.handle, _lib.dptr
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
    rows = []
    try:
        rng = np.random.default_rng(m)
        t = np.ascontiguousarray(np.stack((rng.uniform(0, 12, m),
                                           np.repeat(np.arange(G), m // G).astype(float),
                                           np.ones(m)), -1))
        mu, var, cov = np.empty(m), np.empty(m), np.empty((m, m))

        def predict():
            ctx.check(lib.lfm_post_predict_f64(h, post, dptr(t), m, dptr(mu), dptr(var),
                                               dptr(cov)))

        def shift():
            cov[np.diag_indices(m)] += dadd

        # the host route's pieces: the predict with its download, the addition, one vector
        big = m > 4096
        if not big:
            predict()
        predict_ms = median_ms(predict, 1 if big else max(1, min(3, args.reps)))
        t0 = time.perf_counter()
        shift()
        add_ms = (time.perf_counter() - t0) * 1e3
        # held-out vectors drawn from the predictive distribution itself: plausible log densities
        ystar = np.empty((max(ks), m))
        ctx.check(lib.lfm_post_sample_f64(h, post, dptr(t), m, dadd, 7, 0, max(ks), None,
                                          dptr(ystar)))
        cap = 1024 if m <= 512 else 16 if m <= 4096 else 2
        one = np.empty(1)

        def vector(r):
            ctx.check(lib.lfm_log_prob_f64(h, dptr(mu), dptr(cov), m, m, dptr(ystar[r]), dptr(one)))
            return float(one[0])

        host_first = vector(0)  # warm-up
        vec_ts = []
        for r in range(min(max(ks), cap)):
            t0 = time.perf_counter()
            vector(r)
            vec_ts.append((time.perf_counter() - t0) * 1e3)
        vector_ms = float(np.median(vec_ts))

        # the predict's kernel classes alone
        ctx.profile(True, classes=SOLVE + FACTOR)
        ctx.profile_reset()
        predict()
        st = ctx.profile_read()
        ctx.profile(False)
        pred_solve = sum(st[c]["total_ms"] for c in SOLVE)

        for k in ks:
            ys = np.ascontiguousarray(ystar[:k])
            mean, logp = np.empty(m), np.empty(k)
            rcs = []

            def device():
                rcs.append(lib.lfm_post_log_prob_f64(h, post, dptr(t), m, dadd, dptr(ys), k,
                                                     dptr(mean), dptr(logp)))

            device()
            ctx.check(rcs[-1])
            dev_ms = median_ms(device, args.reps)
            ctx.profile(True, classes=SOLVE + FACTOR)
            ctx.profile_reset()
            device()
            st = ctx.profile_read()
            ctx.profile(False)
            ms = {c: st[c]["total_ms"] for c in SOLVE + FACTOR}
            solve, factor = sum(ms[c] for c in SOLVE), sum(ms[c] for c in FACTOR)
            row = dict(m=m, k=k, rc=int(rcs[-1]), finite=bool(np.all(np.isfinite(logp))),
                       post_log_prob_ms=dev_ms, solve_ms=solve, factor_ms=factor,
                       other_ms=dev_ms - solve - factor, predict_solve_ms=pred_solve,
                       sweep_launches=int(st["post_panel"]["launches"]
                                          + st["post_update"]["launches"]),
                       logp0=float(logp[0]), host_logp0=host_first,
                       upload_bytes=8 * (k * m + 3 * m), download_bytes=8 * (k + m))
            composed = k > cap
            if composed:
                host_ms = predict_ms + add_ms + k * vector_ms
            else:
                def host():
                    predict()
                    shift()
                    for r in range(k):
                        vector(r)

                host_ms = median_ms(host, 1 if big or k > 16 else max(1, min(3, args.reps)))
            row.update(host_route_ms=host_ms, host_route_composed=composed,
                       host_predict_ms=predict_ms, host_add_ms=add_ms, host_vector_ms=vector_ms,
                       host_vectors_timed=len(vec_ts),
                       host_upload_bytes=8 * k * (m * m + 2 * m),
                       host_download_bytes=8 * (m * m + 2 * m + k),
                       ratio_host_over_device=host_ms / dev_ms)
            rows.append(row)
            print(json.dumps(row), flush=True)
    finally:
        lib.lfm_post_destroy(post)
    with open(args.rows_out, "w") as f:
        json.dump(dict(rows=rows, G=G, diag_add=dadd), f)


if args.case:
    child(args.case)
    sys.exit(0)

cases, G, dadd = [], None, None
with tempfile.TemporaryDirectory() as tmp:
    for m in (int(v) for v in args.m.split(",")):
        part = os.path.join(tmp, f"rows_{m}.json")
        cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__),
               "--case", str(m), "--rows-out", part, "--reps", str(args.reps), "--N", str(args.N),
               "--k", args.k]
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"m = {m}: the child ended with status {rc}; nothing more is started",
                  flush=True)
            sys.exit(rc)
        with open(part) as f:
            got = json.load(f)
        cases += got["rows"]
        G, dadd = got["G"], got["diag_add"]

doc = dict(what="lfm_post_log_prob_f64 on a resident N = %d model against lfm_post_predict_f64 "
                "with the covariance + one addition on the diagonal + lfm_log_prob_f64 per "
                "held-out vector; medians of %d synchronous calls by the host clock after a "
                "warm-up call; host routes marked host_route_composed are predict + k x the "
                "median of host_vectors_timed vectors; kernel-class times from HIP events in a "
                "separate pass" % (args.N, args.reps),
           N=args.N, num_genes=G, diag_add=dadd, cases=cases)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(doc, f, indent=1)
    f.write("\n")
print("wrote", args.out)

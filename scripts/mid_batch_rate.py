"""The mid-size resident batch (lfm_mbatch_*) against the path such problems took before it: 15
problems on 5-gene grids at n = 160, 320, 640 and 1020 (T = 32, 64, 128, 204; the hyperparameter
recipe of tests/test_gpu_grad.py::test_grad_block_edges, one seed per problem).
  (a) the batched value call and the batched value-and-gradient call, all 15 problems at once;
  (b) the per-problem loop of lfm_mll_f64 / lfm_mll_grad_f64 over the same 15 problems — what
      lfm_mll_batch_f64 and a training step did for n > 128 (one synchronous call per problem,
      x / y uploaded each time).
(a) and (b) alternate in one process: warm-up calls, then the median of synchronous calls by the
host clock. The kernel time per class (lfm_profile_read) of one batched call comes from a
separate profiled pass. Results: one JSON document (--out, default profiles/mid_batch.json).
    python scripts/mid_batch_rate.py [--reps 20] [--sizes 160,320,640,1020] [--out FILE]"""
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
from dis_project_amd.dataset import grid_inputs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--problems", type=int, default=15)
ap.add_argument("--genes", type=int, default=5)
ap.add_argument("--sizes", default="160,320,640,1020")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mid_batch.json"))
args = ap.parse_args()

ctx = _lib.get_context(0)
lib, h, dptr = ctx.lib, ctx.handle, _lib.dptr
MID = ["mid_fill", "mid_column", "mid_inverse", "mid_pairs", "mid_finish"]


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def one_size(n):
    G, P = args.genes, args.problems
    assert n % G == 0
    T = n // G
    xs, ys, hyps, vecs, scs = [], [], [], [], []
    for p in range(P):
        rng = np.random.default_rng(n * 100 + p)
        D, S, B = rng.uniform(0.2, 1.0, G), rng.uniform(0.5, 1.5, G), rng.uniform(0.01, 0.1, G)
        xs.append(np.ascontiguousarray(grid_inputs(G, T)))
        ys.append(np.repeat(B / D, T) + 0.5 * rng.standard_normal(n))
        hyps.append(_lib.HypArgs(D, S, B, 2.2, 0.9, 1e-4))
        vecs.append(np.concatenate([D, S, B]))
        scs.append([2.2, 0.9, 1e-4])
    packed = np.concatenate(vecs + [np.asarray(scs).reshape(-1)])
    probs = (_lib.LfmProblem * P)()
    for p in range(P):
        probs[p].x, probs[p].y, probs[p].n = xs[p].ctypes.data, ys[p].ctypes.data, n
        probs[p].hyp.num_genes = G
    mb = ctypes.c_void_p()
    ctx.check(lib.lfm_mbatch_create(h, P, probs, ctypes.byref(mb)))
    out_b, grad_b, st = np.empty(P), np.empty(packed.size), np.zeros(P, np.int32)
    out_l, one, grad_l = np.empty(P), np.empty(1), np.empty((P, 3 * G + 2))

    def batch_value():
        ctx.check(lib.lfm_mbatch_mll_f64(h, mb, dptr(packed), 1, dptr(out_b), dptr(st)))

    def batch_grad():
        ctx.check(lib.lfm_mbatch_mll_grad_f64(h, mb, dptr(packed), 1, dptr(out_b), dptr(grad_b),
                                              dptr(st)))

    def loop_value():
        for p in range(P):
            ctx.check(lib.lfm_mll_f64(h, dptr(xs[p]), dptr(ys[p]), n, hyps[p].ref, 1, dptr(one)))
            out_l[p] = one[0]

    def loop_grad():
        for p in range(P):
            ctx.check(lib.lfm_mll_grad_f64(h, dptr(xs[p]), dptr(ys[p]), n, hyps[p].ref, 1,
                                           dptr(one), dptr(grad_l[p])))
            out_l[p] = one[0]

    def kernels(fn):
        ctx.profile(True, classes=MID)
        ctx.profile_reset()
        fn()
        stats = ctx.profile_read()
        ctx.profile(False)
        return {k: dict(ms=stats[k]["total_ms"], launches=stats[k]["launches"]) for k in MID}

    res = dict(n=n, num_genes=G, problems=P)
    try:
        for name, batch, loop in (("value", batch_value, loop_value),
                                  ("value_and_grad", batch_grad, loop_grad)):
            for _ in range(args.warmup):
                batch()
                loop()
            tb, tl = [], []
            for _ in range(args.reps):  # alternating
                tb.append(timed(batch))
                tl.append(timed(loop))
            b_ms, l_ms = float(np.median(tb)), float(np.median(tl))
            agree = float(np.max(np.abs(out_b - out_l) / np.abs(out_l)))
            res[name] = dict(batch_ms=b_ms, loop_ms=l_ms, ratio_loop_over_batch=l_ms / b_ms,
                             batch_us_per_problem=1e3 * b_ms / P, loop_us_per_problem=1e3 * l_ms / P,
                             max_rel_diff_value=agree, kernels=kernels(batch))
            if name == "value_and_grad":
                # the batch's gradient against the loop's, per problem, over its largest component
                gb = np.concatenate([grad_b[:3 * G * P].reshape(P, 3 * G),
                                     grad_b[3 * G * P:].reshape(P, 3)[:, :2]], axis=1)
                res[name]["max_grad_diff_over_largest"] = float(np.max(
                    np.max(np.abs(gb - grad_l), axis=1) / np.max(np.abs(grad_l), axis=1)))
            res[name]["kernel_ms"] = sum(k["ms"] for k in res[name]["kernels"].values())
            res[name]["launches"] = sum(k["launches"] for k in res[name]["kernels"].values())
        print(json.dumps(res), flush=True)
    finally:
        lib.lfm_mbatch_destroy(mb)
    return res


out = dict(what="mid-size resident batch (lfm_mbatch_*) against the per-problem loop of "
                f"lfm_mll_f64 / lfm_mll_grad_f64; {args.problems} problems per size; medians of "
                f"{args.reps} alternating synchronous calls by the host clock; kernel times from "
                "HIP events (lfm_profile_*) in a separate pass",
           sizes=[one_size(int(n)) for n in args.sizes.split(",")])
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print("wrote", args.out)

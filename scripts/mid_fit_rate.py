"""A whole fit of the mid-size resident batch, on the host loop and on the device: P problems on
5-gene grids at n = 160, 320, 640 and 1020 (T = 32, 64, 128, 204; the hyperparameter recipe of
tests/test_gpu_grad.py::test_grad_block_edges, one seed per problem), 150 steps of adam(0.01) on
-MLL, after_epoch every 1000 steps.
  (a) trainer.MidBatchTrainer.fit on the host loop: one lfm_mbatch_mll_grad_f64 call per step,
      the constrain, the chain rule and Adam per problem in Python between the calls;
  (b) the same trainer with on_device=True: one lfm_mbatch_fit_f64 call for the whole fit;
  (c) for 15 problems of n = 35 (5 genes x 7 times), trainer.BatchTrainer.fit (lfm_batch_fit_f64,
      the whole loop inside one launch) beside (b) on the same problems.
(a) and (b) alternate in one process, each from the same start: warm-up fits, then the median of
synchronous fits by the host clock. The kernel time per class (lfm_profile_read) of a 10-step
on-device fit comes from a separate profiled pass. One JSON document per problem count:
profiles/mid_fit.json for 15 problems, profiles/mid_fit_p<P>.json otherwise.
    python scripts/mid_fit_rate.py [--reps 5] [--problems 15,4] [--sizes 160,320,640,1020]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dis_project_amd as lfm  # noqa: E402
from dis_project_amd import _lib  # noqa: E402
from dis_project_amd import trainer as TR  # noqa: E402
from dis_project_amd.dataset import Dataset, grid_inputs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--steps", type=int, default=150)
ap.add_argument("--problems", default="15,4")
ap.add_argument("--genes", type=int, default=5)
ap.add_argument("--sizes", default="160,320,640,1020")
ap.add_argument("--outdir", default=os.path.join(ROOT, "profiles"))
args = ap.parse_args()

ctx = _lib.get_context(0)
MID = ["mid_fill", "mid_column", "mid_inverse", "mid_pairs", "mid_finish"]


def problems(n, P, G):
    T = n // G
    out = []
    for p in range(P):
        rng = np.random.default_rng(n * 100 + p)
        D, S, B = rng.uniform(0.2, 1.0, G), rng.uniform(0.5, 1.5, G), rng.uniform(0.01, 0.1, G)
        y = np.repeat(B / D, T) + 0.5 * rng.standard_normal(n)
        m = lfm.ExactLFM(jitter=1e-4, num_genes=G, true_d=D, true_s=S, true_b=B, l=2.2,
                         obs_stddev=0.9)
        out.append((m, Dataset(np.ascontiguousarray(grid_inputs(G, T)), y)))
    return out


def timed_fit(bt, start):
    bt.raws = [dict(r) for r in start]  # every fit from the same start
    t0 = time.perf_counter()
    _, hist = bt.fit(fix_params=True, num_steps_per_epoch=1000)
    return (time.perf_counter() - t0) * 1e3, hist


def alternate(first, second, start):
    """Medians (ms) of alternating fits of two trainers, and their last histories."""
    for _ in range(args.warmup):
        timed_fit(first, start)
        timed_fit(second, start)
    t1, t2 = [], []
    for _ in range(args.reps):
        ms, h1 = timed_fit(first, start)
        t1.append(ms)
        ms, h2 = timed_fit(second, start)
        t2.append(ms)
    return float(np.median(t1)), float(np.median(t2)), h1, h2


def kernels(ev, probs, nsteps=10):
    """Kernel time per class of one on-device fit of nsteps steps (HIP events)."""
    raw = TR.pack_raw([TR.unconstrain(m) for m, _ in probs], [m.jitter for m, _ in probs])
    mu, nu = np.zeros_like(raw), np.zeros_like(raw)
    ctx.profile(True, classes=MID)
    ctx.profile_reset()
    ev.fit_packed(raw, mu, nu, TR.adam(0.01), True, 1000, 0, nsteps)
    stats = ctx.profile_read()
    ctx.profile(False)
    per = {k: dict(ms=stats[k]["total_ms"], launches=stats[k]["launches"]) for k in MID}
    return dict(steps=nsteps, classes=per,
                kernel_ms_per_step=sum(k["ms"] for k in per.values()) / nsteps,
                launches_per_step=(sum(k["launches"] for k in per.values()) - 1) / nsteps)


def mid_trainer(probs, on_device, evaluator=None):
    return TR.MidBatchTrainer([m for m, _ in probs], lfm.CustomConjMLL(negative=True),
                              [d for _, d in probs], TR.adam(0.01), num_iters=args.steps,
                              ctx=ctx, evaluator=evaluator, on_device=on_device)


def one_size(n, P):
    probs = problems(n, P, args.genes)
    host, dev = mid_trainer(probs, False), mid_trainer(probs, True)
    start = [dict(r) for r in host.raws]
    try:
        a_ms, b_ms, ha, hb = alternate(host, dev, start)
        res = dict(n=n, num_genes=args.genes, problems=P, steps=args.steps,
                   host_loop_ms=a_ms, on_device_ms=b_ms, ratio_host_over_device=a_ms / b_ms,
                   host_loop_ms_per_step=a_ms / args.steps, on_device_ms_per_step=b_ms / args.steps,
                   host_gap_ms_per_step=(a_ms - b_ms) / args.steps,
                   max_rel_diff_history=float(np.max(np.abs(ha - hb) / np.abs(ha))),
                   profiled=kernels(dev.evaluator, probs))
    finally:
        host.close()
        dev.close()
    print(json.dumps(res), flush=True)
    return res


def small_set():
    """(c): 15 problems of n = 35, the one-launch small fit beside the mid path's fit."""
    probs = problems(35, 15, 5)
    small = TR.BatchTrainer([m for m, _ in probs], lfm.CustomConjMLL(negative=True),
                            [d for _, d in probs], TR.adam(0.01), num_iters=args.steps, ctx=ctx)
    dev = mid_trainer(probs, True)
    start = [dict(r) for r in dev.raws]
    try:
        s_ms, b_ms, hs, hb = alternate(small, dev, start)
        res = dict(n=35, num_genes=5, problems=15, steps=args.steps, batch_trainer_ms=s_ms,
                   on_device_ms=b_ms, batch_trainer_us_per_step=1e3 * s_ms / args.steps,
                   on_device_us_per_step=1e3 * b_ms / args.steps,
                   ratio_mid_over_small=b_ms / s_ms,
                   max_rel_diff_history=float(np.max(np.abs(hs - hb) / np.abs(hs))))
    finally:
        small.close()
        dev.close()
    print(json.dumps(res), flush=True)
    return res


os.makedirs(args.outdir, exist_ok=True)
for P in (int(p) for p in args.problems.split(",")):
    out = dict(what="a whole fit of the mid-size resident batch: trainer.MidBatchTrainer.fit on "
                    "the host loop (one lfm_mbatch_mll_grad_f64 call per step) against "
                    f"on_device=True (one lfm_mbatch_fit_f64 call); {P} problems per size, "
                    f"{args.steps} steps of adam(0.01) on -MLL; medians of {args.reps} "
                    "alternating synchronous fits by the host clock after "
                    f"{args.warmup} warm-up fit(s); kernel times from HIP events "
                    "(lfm_profile_*) of a 10-step fit in a separate pass",
               sizes=[one_size(int(n), P) for n in args.sizes.split(",")])
    if P == 15:
        out["small_n35"] = small_set()
    path = os.path.join(args.outdir, "mid_fit.json" if P == 15 else f"mid_fit_p{P}.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)

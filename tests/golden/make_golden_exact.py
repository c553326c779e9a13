"""Extended-precision golden values at C3's restarts and C5's rounds (oracle/lfm_exact.py).

    python tests/golden/make_golden_exact.py              # tests/golden/exact_reduced.npz
    python tests/golden/make_golden_exact.py --full 5     # one full-size restart (resumable)
    python tests/golden/make_golden_exact.py --full all   # the missing ones of FULL_RESTARTS

The existing goldens come from the fp64 oracle, which cancels where the reference does; these
come from mpmath / long double and do not. Inputs are not stored: configs rebuilds them from
their seeds. Two files, because no committed file may exceed 1 MiB:

exact_reduced.npz
  sub_*   restart r = 0..31 of configs.c3_restarts(configs.c2(), 32) reduced to the 4-gene
          sub-model of lfm_exact.submodel on grid_inputs(4, 256) (N = 1024: the smallest layout on
          the aligned, fused, schedule-3 path). Per restart SAMPLES lower-triangle (row, col)
          pairs with the exact value and M_tab, and the exact MLL / logdet / quadratic form of
          y = configs.grid_workload("exact", 4, 256, 2, 3).data.y (long double Cholesky of the
          long double Sigma), scipy's on the correctly rounded Sigma, and the oracle's.
  una_*   the same entry data on the unaligned layout grid_inputs(3, 43) (3-gene sub-model),
          restarts UNALIGNED_RESTARTS.
  c5_*    configs.c5_rounds rounds 0..15 of the 15 C5 problems (n = 28): exact MLL parts of all
          240, all 406 lower entries of the problems C5_ENTRY_PROBLEMS.
  k_tab64 / k_tab32   4 x the largest |dK| / (eps M_tab) of a numpy/scipy restatement of the
          device's table form (fp64; tables rounded to fp32 and combined in fp32) over every
          sub_* and una_* entry.
  *_mll_rtol   max(1e-9, 8 |mll_fp64_lapack - exact| / |exact|), capped at 1e-5; a problem whose
          LAPACK value is already outside 1e-5 is listed in *_dropped instead (at most 2 of 32).

exact_full.npz (N = 16384, the real 64-gene restarts FULL_RESTARTS)
  sigma_exact rounded to fp64, then scipy's Cholesky: mll / logdet / quad. No extended
  factorisation is feasible at this size; mll_rtol is max(1e-9, 8 x the relative change of
  that MLL when the entries of the rounded Sigma are moved by one ulp up or down with
  probability 1/2 (seeded; fp64 holds no half ulp, so the mean displacement is half an ulp))
  with the same cap and drop rule. For FULL_ROW_RESTARTS, 16 rows x FULL_COLS sampled columns
  of exact K and M_tab.
"""

from __future__ import annotations

import math
import os
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import scipy.linalg
import scipy.special

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from dis_project_amd import configs  # noqa: E402
from dis_project_amd.dataset import grid_inputs  # noqa: E402
from oracle import lfm_exact as E  # noqa: E402
from oracle import lfm_oracle as O  # noqa: E402

EPS = np.finfo(np.float64).eps
EPS32 = float(np.finfo(np.float32).eps)
RESTARTS = 32
SAMPLES = 768
UNALIGNED_RESTARTS = (1, 5, 10, 29)
C5_ROUNDS = 16
C5_ENTRY_PROBLEMS = tuple(range(0, 240, 5))  # 48 problems: 3 per round, every ablation
FULL_RESTARTS = (0, 1, 5, 8, 10, 18, 21, 27, 29)
FULL_ROW_RESTARTS = (5, 29)
FULL_COLS = 1024
NORTH_STAR = 1e-5
PROJECT_RTOL = 1e-9
MAX_DROPPED = 2
REDUCED = os.path.join(HERE, "exact_reduced.npz")
FULL = os.path.join(HERE, "exact_full.npz")


# ----------------------------------------------------------------- problems
def restart_models():
    return configs.c3_restarts(configs.c2(), RESTARTS)


def sub_problem(model, G=4, T=256):
    """(x, y, sub-model) of one restart's reduced problem."""
    sub, _ = E.submodel(model, G)
    work = configs.grid_workload("exact", G, T, seed_params=2, seed_y=3)
    return (np.ascontiguousarray(work.data.X), np.ascontiguousarray(work.data.y.reshape(-1)),
            sub)


def c5_problems():
    works = configs.c5_ablations()
    models = configs.c5_rounds([w.model for w in works], C5_ROUNDS)
    return works, models


# ------------------------------------------------------------------ sampling
def sample_pairs(D, l, G, T, seed, count=SAMPLES, row_tile=64, col_tile=256):
    """Seeded lower-triangle (row >= col) pairs of the G x T block layout on linspace(0, 12, T):
    the diagonal, tau = 0 rows, tau = T - 1 columns, d = +-(T - 1), both sides of the row / column
    tile edges, both sides of the exp_erfc branch of Wt (gamma - delta / l changing sign) and of
    Qt (gamma - t / l), every gene pair; filled to exactly `count` with uniform pairs."""
    rng = np.random.default_rng(seed)
    n = G * T
    dt = 12.0 / (T - 1)
    pairs = []

    def add(r, c):
        r, c = int(r), int(c)
        if 0 <= c <= r < n:
            pairs.append((r, c))

    for i in (0, T - 1, T, n - 1):
        add(i, i)
    for i in rng.choice(n, min(n, 44), replace=False):
        add(i, i)
    for bi in range(G):                       # tau = 0 rows, tau' = T - 1 columns
        for c in rng.integers(0, bi * T + 1, 6):
            add(bi * T, c)
        c = bi * T + T - 1
        for r in rng.integers(c, n, 6):
            add(r, c)
    for bi in range(G):                       # d = +(T - 1) and -(T - 1)
        for bk in range(bi + 1):
            add(bi * T + T - 1, bk * T)       # d = -(T - 1)
            if bk < bi:
                add(bi * T, bk * T + T - 1)   # d = +(T - 1)
    redges = [e for m in range(row_tile, n, row_tile) for e in (m - 1, m)]
    cedges = [e for m in range(col_tile, n, col_tile) for e in (m - 1, m)] or [0, n - 1]
    for r in redges:
        add(r, rng.integers(0, r + 1))
        for c in cedges:
            add(r, c)
    for c in cedges:
        add(rng.integers(c, n), c)
    # exp_erfc's branch: z = gamma_g - delta / l changes sign at delta* = D_g l^2 / 2
    for g in range(G):
        ds = D[g] * l * l / 2 / dt
        for d in (math.floor(ds), math.floor(ds) + 1):
            if not 0 < d <= T - 1:
                continue
            for _ in range(6):
                lo = int(rng.integers(0, T - d))
                bo = int(rng.integers(0, G))
                if g < bo:                    # gene g as the column gene: d = tau' - tau > 0
                    add(bo * T + lo, g * T + lo + d)
                if bo <= g:                   # gene g as the row gene: -d
                    add(g * T + lo + d, bo * T + lo)
            for bo in range(G):               # Qt's branch at t = delta*
                add(max(g, bo) * T + (d if g >= bo else int(rng.integers(0, T))),
                    min(g, bo) * T + (d if g < bo else int(rng.integers(0, T))))
    for bi in range(G):                       # every gene pair
        for bk in range(bi + 1):
            for _ in range(12):
                add(bi * T + rng.integers(0, T), bk * T + rng.integers(0, T))
    seen, out = set(), []
    for p in pairs:
        if p not in seen:
            seen.add(p)
            out.append(p)
    while len(out) < count:
        r = int(rng.integers(0, n))
        p = (r, int(rng.integers(0, r + 1)))
        if p not in seen:
            seen.add(p)
            out.append(p)
    out = np.array(out[:count], np.int32)
    return out[:, 0].copy(), out[:, 1].copy()


# ---------------------------------- the device's table form, restated in numpy
def exp_erfc_np(A, z):
    """e^A erfc(z), through erfcx once z > 0."""
    zp = np.where(z > 0, z, 0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(z > 0, scipy.special.erfcx(zp) * np.exp(A - zp * zp),
                        np.exp(A) * scipy.special.erfc(z))


def table_form_np(t, D, S, l, jr, tau, kc, tp, fp32=False):
    """kxx of rows (gene jr, time index tau) and columns (gene kc, tp) on the uniform grid t
    through the tables of the structured gram (Wt, Xt, Pt, Et, Qt, Cm and their combine), in
    fp64 numpy / scipy.special; with ``fp32`` every table entry is rounded to fp32 and the
    combine runs in fp32. Written from the identities, not from the HIP source's code."""
    t = np.asarray(t, np.float64)
    T = t.size
    dt = (t[-1] - t[0]) / (T - 1)
    d = (tp - tau).astype(np.float64)

    def WX(g, dd):
        gam = D[g] * l / 2.0
        delta = dd * dt
        A = gam * gam - D[g] * delta
        return exp_erfc_np(A, gam - delta / l), np.exp(A)

    def PEQ(g, ti):
        gam = D[g] * l / 2.0
        tt = t[ti]
        return (scipy.special.erfc(tt / l + gam), np.exp(-D[g] * tt),
                exp_erfc_np(gam * gam, gam - tt / l) - scipy.special.erfcx(gam))

    Wk, Xk = WX(kc, d)
    Wj, Xj = WX(jr, -d)
    Pk, _, Qj = PEQ(kc, tau)[0], None, PEQ(jr, tau)[2]
    Pj, Ej = PEQ(jr, tp)[0], PEQ(jr, tau)[1]
    Ek, Qk = PEQ(kc, tp)[1], PEQ(kc, tp)[2]
    Cm = S[jr] * S[kc] * l * math.sqrt(math.pi) * 0.5 / (D[jr] + D[kc])
    if fp32:
        Wk, Xk, Wj, Xj, Pk, Pj, Ej, Ek, Qj, Qk, Cm = (
            np.asarray(v, np.float64).astype(np.float32)
            for v in (Wk, Xk, Wj, Xj, Pk, Pj, Ej, Ek, Qj, Qk, Cm))
    with np.errstate(over="ignore", invalid="ignore"):
        v = Wk + Wj
        v = v - Xk * Pk
        v = v - Xj * Pj
        v = v - (Ek * Ej) * (Qk + Qj)
        return Cm * v


def table_form_pairs(x, rows, cols, D, S, l, fp32=False):
    t, bg = E.grid_of(x)
    T = t.size
    bg = bg.astype(np.int64)
    return table_form_np(t, D, S, l, bg[rows // T], rows % T, bg[cols // T], cols % T, fp32)


# ------------------------------------------------------------------- pieces
def mll_parts_lapack(Sig, r):
    n = Sig.shape[0]
    c = scipy.linalg.cholesky(Sig, lower=True, check_finite=False)
    logdet = 2.0 * float(np.sum(np.log(np.diag(c))))
    z = scipy.linalg.solve_triangular(c, r, lower=True, check_finite=False)
    quad = float(z @ z)
    return -0.5 * (n * math.log(2 * math.pi) + logdet + quad), logdet, quad


def rtol_of(lapack, exact):
    """(mll_rtol, dropped): max(1e-9, 8 |lapack - exact| / |exact|) capped at 1e-5; dropped
    when LAPACK on exactly rounded inputs is itself outside 1e-5."""
    rel = abs(lapack - exact) / abs(exact)
    if not rel <= NORTH_STAR:
        return float("nan"), True
    return min(NORTH_STAR, max(PROJECT_RTOL, 8 * rel)), False


def entry_block(x, D, S, l, rows, cols, tables):
    """Exact sampled entries and M_tab; asserts the long double table route agrees with the
    direct mpmath formula far below fp64 eps M_tab (2^-8 of it) and restatement ratios."""
    val, mt = E.exact_pairs(x, rows, cols, D, S, l)
    T = tables.T
    _, bg = E.grid_of(x)
    got = np.array([tables.block(int(bg[r // T]), int(bg[c // T]), [r % T])[0][c % T]
                    for r, c in zip(rows, cols)], dtype=E.LD)
    dev = np.abs(got - val.astype(E.LD)).astype(np.float64)
    # val is itself rounded to fp64: half an ulp of |K| is the floor of this comparison
    assert np.all(dev <= EPS * mt / 256 + 0.5 * EPS * np.abs(val)), float((dev / (EPS * mt)).max())
    r64 = np.abs(table_form_pairs(x, rows, cols, D, S, l) - val) / (EPS * mt)
    k32 = table_form_pairs(x, rows, cols, D, S, l, fp32=True).astype(np.float64)
    r32 = np.abs(k32 - val) / (EPS32 * mt)
    return val, mt, float(r64.max()), float(np.nan_to_num(r32, nan=np.inf).max())


def sub_case(r):
    t0 = time.perf_counter()
    model = restart_models()[r]
    x, y, sub = sub_problem(model)
    D, S, B = (np.asarray(v, np.float64) for v in (sub.true_d, sub.true_s, sub.true_b))
    l = float(sub.l)
    T, G = 256, 4
    tabs = E.GridTables(x[:T, 0], D, S, l, range(G))
    rows, cols = sample_pairs(D, l, G, T, 7000 + r)
    val, mt, r64, r32 = entry_block(x, D, S, l, rows, cols, tabs)
    diag = (sub.jitter, sub.obs_stddev ** 2)
    SigL = E.sigma_exact(x, D, S, l, diag, dtype=E.LD, tables=tabs)
    Sig = E.sigma_exact(x, D, S, l, diag, tables=tabs)
    assert np.all(Sig == SigL.astype(np.float64))
    res = y - O.mean_function(x, D, B, G).reshape(-1)
    ex = E.mll_exact(SigL, res)
    ex2 = E.mll_exact(SigL, res, perm=np.random.default_rng(8000 + r).permutation(x.shape[0]))
    la = mll_parts_lapack(Sig, res)
    rtol, dropped = rtol_of(la[0], ex[0])
    # extended precision was sufficient: two elimination orders agree to 1e-3 of the tolerance
    assert abs(ex[0] - ex2[0]) <= 1e-3 * (PROJECT_RTOL if dropped else rtol) * abs(ex[0]), (ex, ex2)
    orc = O.mll(x, y, D, S, B, l, sub.obs_stddev, sub.jitter)
    print(f"sub r{r}: mll={ex[0]!r} lapack rel={abs(la[0] - ex[0]) / abs(ex[0]):.2e} "
          f"oracle rel={abs(orc - ex[0]) / abs(ex[0]):.2e} rtol={rtol:.2e} r64={r64:.1f} "
          f"r32={r32:.1f} ({time.perf_counter() - t0:.1f} s)", flush=True)
    return dict(rows=rows, cols=cols, k=val, mtab=mt.astype(np.float32), mll=ex[0], logdet=ex[1],
                quad=ex[2], mll_fp64_lapack=la[0], mll_oracle=orc, mll_rtol=rtol,
                dropped=dropped, r64=r64, r32=r32)


def una_case(r):
    model = restart_models()[r]
    G, T = 3, 43
    sub, _ = E.submodel(model, G)
    x = grid_inputs(G, T)
    D, S = np.asarray(sub.true_d, np.float64), np.asarray(sub.true_s, np.float64)
    l = float(sub.l)
    tabs = E.GridTables(x[:T, 0], D, S, l, range(G))
    rows, cols = sample_pairs(D, l, G, T, 7100 + r, row_tile=32)
    val, mt, r64, r32 = entry_block(x, D, S, l, rows, cols, tabs)
    print(f"una r{r}: r64={r64:.1f} r32={r32:.1f}", flush=True)
    return dict(rows=rows, cols=cols, k=val, mtab=mt.astype(np.float32), r64=r64, r32=r32)


def c5_case(p):
    works, models = c5_problems()
    m, w = models[p], works[p % len(works)]
    x = np.ascontiguousarray(w.data.X)
    y = np.ascontiguousarray(w.data.y.reshape(-1))
    D, S, B = (np.asarray(v, np.float64) for v in (m.true_d, m.true_s, m.true_b))
    n = x.shape[0]
    ii, jj = np.tril_indices(n)
    val, mt = E.exact_pairs(x, ii, jj, D, S, m.l)
    # long double Sigma from the table route, tied to the direct formula entry by entry
    SigL = E.sigma_exact(x, D, S, m.l, (m.jitter, m.obs_stddev ** 2), dtype=E.LD)
    KL = E.sigma_exact(x, D, S, m.l, 0.0, dtype=E.LD)
    dev = np.abs(KL[ii, jj] - val.astype(E.LD)).astype(np.float64)
    assert np.all(dev <= EPS * mt / 256 + 0.5 * EPS * np.abs(val)), float((dev / (EPS * mt)).max())
    Sig = SigL.astype(np.float64)
    res = y - O.mean_function(x, D, B, m.num_genes).reshape(-1)
    ex = E.mll_exact(SigL, res)
    ex2 = E.mll_exact(SigL, res, perm=np.random.default_rng(9000 + p).permutation(n))
    la = mll_parts_lapack(Sig, res)
    rtol, dropped = rtol_of(la[0], ex[0])
    assert abs(ex[0] - ex2[0]) <= 1e-3 * (PROJECT_RTOL if dropped else rtol) * abs(ex[0])
    return dict(k=val, mll=ex[0], logdet=ex[1], quad=ex[2], mll_fp64_lapack=la[0],
                mll_rtol=rtol, dropped=dropped)


def make_reduced():
    with ProcessPoolExecutor(int(os.environ.get("GOLDEN_THREADS", "8"))) as ex:
        sub = list(ex.map(sub_case, range(RESTARTS)))
        una = list(ex.map(una_case, UNALIGNED_RESTARTS))
        c5 = list(ex.map(c5_case, range(15 * C5_ROUNDS), chunksize=8))
    out = {}
    for key in ("rows", "cols", "k", "mtab"):
        out[f"sub_{key}"] = np.stack([s[key] for s in sub])
        out[f"una_{key}"] = np.stack([s[key] for s in una])
    for key in ("mll", "logdet", "quad", "mll_fp64_lapack", "mll_oracle", "mll_rtol"):
        out[f"sub_{key}"] = np.array([s[key] for s in sub], np.float64)
    out["sub_dropped"] = np.array([r for r, s in enumerate(sub) if s["dropped"]], np.int64)
    assert out["sub_dropped"].size <= MAX_DROPPED, out["sub_dropped"]
    out["una_restarts"] = np.array(UNALIGNED_RESTARTS, np.int64)
    out["k_tab64"] = np.float64(4 * max(s["r64"] for s in sub + una))
    out["k_tab32"] = np.float64(4 * max(s["r32"] for s in sub + una))
    for key in ("mll", "logdet", "quad", "mll_fp64_lapack", "mll_rtol"):
        out[f"c5_{key}"] = np.array([s[key] for s in c5], np.float64)
    out["c5_dropped"] = np.array([p for p, s in enumerate(c5) if s["dropped"]], np.int64)
    out["c5_entry_problems"] = np.array(C5_ENTRY_PROBLEMS, np.int64)
    out["c5_k"] = np.stack([c5[p]["k"] for p in C5_ENTRY_PROBLEMS])
    print(f"k_tab64={float(out['k_tab64']):.1f} k_tab32={float(out['k_tab32']):.1f} "
          f"dropped sub={out['sub_dropped'].tolist()} c5={out['c5_dropped'].tolist()}")
    np.savez_compressed(REDUCED, **out)


# ---------------------------------------------------------------- full size
def full_columns(n, T=256):
    rng = np.random.default_rng(2025)
    fixed = [0, 1, T - 1, T, T + 1, 8191, 8192, n - T, n - 2, n - 1]
    rest = rng.choice(np.setdiff1d(np.arange(n), fixed), FULL_COLS - len(fixed), replace=False)
    return np.sort(np.concatenate([fixed, rest])).astype(np.int64)


def half_ulp_perturbed(Sig, seed):
    """Sig with each lower entry moved one ulp up or down with probability 1/2 (in place,
    mirrored: the perturbed matrix stays symmetric)."""
    rng = np.random.default_rng(seed)
    n = Sig.shape[0]
    for i0 in range(0, n, 512):
        blk = Sig[i0:i0 + 512]
        u = rng.integers(0, 4, blk.shape, dtype=np.int8)
        step = np.where(u == 0, 1.0, np.where(u == 1, -1.0, 0.0))
        blk += step * np.spacing(np.abs(blk))
    for i0 in range(0, n, 512):               # mirror the lower triangle
        Sig[i0:i0 + 512, i0 + 512:] = Sig[i0 + 512:, i0:i0 + 512].T
        d = Sig[i0:i0 + 512, i0:i0 + 512]
        d[:] = np.tril(d) + np.tril(d, -1).T
    return Sig


def full_case(r):
    t0 = time.perf_counter()
    base = configs.c2()
    model = restart_models()[r]
    x = np.ascontiguousarray(base.data.X)
    y = np.ascontiguousarray(base.data.y.reshape(-1))
    D, S, B = (np.asarray(v, np.float64) for v in (model.true_d, model.true_s, model.true_b))
    l, G, T = float(model.l), model.num_genes, 256
    n = x.shape[0]
    tabs = E.GridTables(x[:T, 0], D, S, l, range(G))
    print(f"full r{r}: tables {time.perf_counter() - t0:.0f} s", flush=True)
    res = {}
    if r in FULL_ROW_RESTARTS:
        rng = np.random.default_rng(2024)
        rows = np.sort(np.concatenate([[0, 127, 128, 8191, n - 1],
                                       rng.choice(n, 11, replace=False)])).astype(np.int64)
        cols = full_columns(n)
        K, M = E.sigma_rows_exact(x, rows, D, S, l, tables=tabs)
        # tie the table route to the direct formula on a few of these entries
        pick = np.random.default_rng(r).integers(0, cols.size, 8)
        for i in (0, 7, 15):
            v, mt = E.exact_pairs(x, np.full(8, rows[i]), cols[pick], D, S, l)
            assert np.all(np.abs(K[i, cols[pick]] - v) <= EPS * mt / 256 + EPS * np.abs(v))
        res.update({f"r{r}_rows": rows, f"r{r}_cols": cols, f"r{r}_krows": K[:, cols],
                    f"r{r}_mtab": M[:, cols]})
    Sig = E.sigma_exact(x, D, S, l, (model.jitter, model.obs_stddev ** 2), tables=tabs)
    print(f"full r{r}: sigma {time.perf_counter() - t0:.0f} s", flush=True)
    resid = y - O.mean_function(x, D, B, G).reshape(-1)
    la = mll_parts_lapack(Sig, resid)
    pert = mll_parts_lapack(half_ulp_perturbed(Sig, 6000 + r), resid)
    rel = abs(pert[0] - la[0]) / abs(la[0])
    dropped = not rel <= NORTH_STAR
    rtol = float("nan") if dropped else min(NORTH_STAR, max(PROJECT_RTOL, 8 * rel))
    print(f"full r{r}: mll={la[0]!r} logdet={la[1]!r} quad={la[2]!r} perturbed rel={rel:.2e} "
          f"rtol={rtol:.2e} ({time.perf_counter() - t0:.0f} s)", flush=True)
    res.update({f"r{r}_mll": np.float64(la[0]), f"r{r}_logdet": np.float64(la[1]),
                f"r{r}_quad": np.float64(la[2]), f"r{r}_mll_rtol": np.float64(rtol),
                f"r{r}_perturbed_rel": np.float64(rel)})
    return res


def make_full(which):
    out = {}
    if os.path.exists(FULL):
        with np.load(FULL, allow_pickle=False) as z:
            out = {k: z[k] for k in z.files}
    todo = [r for r in (FULL_RESTARTS if which == "all" else (int(which),))
            if f"r{r}_mll" not in out]
    # a case holds ~7 GB; GOLDEN_FULL_PROCS of them run side by side
    with ProcessPoolExecutor(int(os.environ.get("GOLDEN_FULL_PROCS", "1"))) as ex:
        for res in ex.map(full_case, todo):
            out.update(res)
            done = sorted(int(k[1:-4]) for k in out if k.endswith("_mll"))
            out["restarts"] = np.array(done, np.int64)
            out["dropped"] = np.array([q for q in done if np.isnan(out[f"r{q}_mll_rtol"])],
                                      np.int64)
            np.savez_compressed(FULL, **out)


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--full":
        make_full(sys.argv[2])
    else:
        make_reduced()

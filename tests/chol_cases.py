"""Matrices whose Cholesky factor is known exactly, the cases that walk the blocked factorisation's
step plans with them, and a numpy restatement of the blocked algorithm that can inject one fault.
Shared by tests/test_chol_cases_host.py (CPU) and tests/test_gpu_chol_exact.py. Nothing here needs
a GPU.

The family. Li is lower triangular with integer entries: strict lower part in (-2^18, 2^18),
diagonal in [2^24, 2^25). L0 = Li 2^-24 (off-diagonal magnitudes below 1/64, diagonal in [1, 2)) and
Sigma = (Li Li^T) 2^-48. Every partial sum of Li Li^T is an integer below 2^53, so the fp64 product
is exact in any order: Sigma's Cholesky factor is L0 to the last bit, its entries carry about 50
significant bits, and kappa(Sigma) grows from 4.2 at n = 129 to 7.3 at n = 2559.
With integer w in [-3, 3], loc a multiple of 1/4 and y = loc + L0 w (exact again) the truth needs no
arithmetic beyond logs of the diagonal:
    log N(y; loc, Sigma) = -1/2 (n log 2 pi + 2 sum log L0_ii + w.w).

The bounds. c(n, kappa) = (8 n eps + 4e-14) kappa: n eps is the backward error of an n-term fp64
accumulation, the 8 covers the factor, the solve and the two reductions, and 4e-14 is four times the
pivot reciprocal square root's pinned error (test_pivot_rsqrt_one_newton_step, <= 1e-14).
    log density:  |logp - truth| <= c max(1, |truth|)
    draws:        |X - (loc + Z L0^T)| <= c (|Z| |L0|^T) + 4 eps |loc|, element by element.

The cases. Each names the regime it reaches; `widths` and `steps` are what plan_steps and plan_s3
(lfm_host.cpp) give for it, as tests/native/chol_plan_check.cpp prints them, and
tests/test_chol_cases_host.py compares the two, so a case stops reaching its regime loudly when the
plan changes. A step field is T:wn:R:hu (T trailing 128-tiles past the super-panel, wn the next
super-panel's width, R = S supertiled / B bands / - no update, hu the side-CU helper's units).

The restatement (blocked_cholesky) is the same algorithm in numpy with one injectable fault; what
each fault does to the bounds is measured in tests/test_chol_cases_host.py (its docstring has the
figures). The structural faults move the log density by more than 10^4 bounds. An fp32 rounding of
Sigma does not do so reliably: its 10^6 rounding errors enter the scalar with random signs, and the
sum lands anywhere between 0.3 and 700 bounds depending on n (FP32_SCALAR_UNDER_10 lists the sizes
of the table where it stays under 10). The factor's entries move by at least 890 bounds at every
size, which is why every case also draws (draw_widths): an fp32 step is the element-wise check's to
catch, not the scalar's.
"""

import functools
import math
from collections import namedtuple

import numpy as np

EPS = 2.0 ** -52
NB = 128      # block column
SLAB = 64     # rows of one update unit
SEED = 7
CUS = 256     # an MI355X
# The library's defaults that knobs_of restates: the environment knobs as lfm_ctx.hip reads them
# (env_int_api("NAME", default)), the bulk widths (lfm_chol.h WBULK; 4 on schedule 1) and
# LFM_W2_MIN's per-schedule default (lfm_chol_sched.hip). tests/test_chol_cases_host.py compares
# them with those sources' text; the helper's and the partition's are also S3Params' own defaults
# (lfm_host.h), which chol_plan_check uses for a "-".
DEFAULTS = {"LFM_SCHED": 3, "LFM_W4_MIN": 6144, "LFM_W2_MIN": -1, "LFM_W0": 1, "LFM_HELPER": 1,
            "LFM_HELPER_TC": 700, "LFM_HELPER_MIN": 1200, "LFM_SIDE_CUS": 32}
WBULK_S3, WBULK_S1 = 5, 4
W2MIN_S3, W2MIN_S1 = 5120, 4096


def round_up(a, b):
    return (a + b - 1) // b * b


# ------------------------------------------------------------------ the exact-factor family
@functools.lru_cache(maxsize=None)
def exact_factor(n, seed=SEED):
    """dict(Sigma, L0, loc, w, y, kappa, logdet, truth, c) of the family above. Cached per
    (n, seed); the arrays are read-only."""
    rng = np.random.default_rng(seed)
    li = np.tril(rng.integers(-(2 ** 18) + 1, 2 ** 18, size=(n, n)).astype(np.float64), -1)
    li[np.diag_indices(n)] = rng.integers(2 ** 24, 2 ** 25, size=n).astype(np.float64)
    prod = li @ li.T
    assert float(np.max(np.abs(prod))) < 2.0 ** 53
    # every partial sum is an integer below 2^53: a second summation order gives the same bits
    h = n // 2
    assert np.array_equal(prod, li[:, :h] @ li[:, :h].T + li[:, h:] @ li[:, h:].T)
    assert np.array_equal(prod, prod.T)
    l0 = li * 2.0 ** -24
    sigma = prod * 2.0 ** -48
    w = rng.integers(-3, 4, size=n).astype(np.float64)
    loc = rng.integers(-20, 21, size=n).astype(np.float64) / 4.0
    y = loc + l0 @ w
    # exact: multiples of 2^-24 far below 2^53 of them, in either order
    assert np.array_equal(y - loc, l0[:, ::-1] @ w[::-1])
    ev = np.linalg.eigvalsh(sigma)
    kappa = float(ev[-1] / ev[0])
    logdet = 2.0 * math.fsum(float(v) for v in np.log(np.diag(l0).astype(np.longdouble)))
    truth = -0.5 * (n * math.log(2.0 * math.pi) + logdet + float(w @ w))
    for arr in (sigma, l0, loc, w, y):
        arr.setflags(write=False)
    return dict(n=n, Sigma=sigma, L0=l0, loc=loc, w=w, y=y, kappa=kappa, logdet=logdet,
                truth=truth, c=bound_c(n, kappa))


def bound_c(n, kappa):
    return (8.0 * n * EPS + 4e-14) * kappa


def logp_bound(p):
    return p["c"] * max(1.0, abs(p["truth"]))


def draw_bound(p, z):
    """Element-wise bound of a draw X = loc + Z L^T with normals z (nsamp x n)."""
    return p["c"] * (np.abs(z) @ np.abs(p["L0"]).T) + 4.0 * EPS * np.abs(p["loc"])


# ------------------------------------------------------------------ the cases
# draw_widths: the width list of the case's draw, whose factorisation is schedule 1's whatever the
# context's (bulk width 4, a wide first super-panel, LFM_W0 ignored). Every case has one; the
# device test draws once per distinct (n, draw_widths) (draw_cases)
Case =namedtuple("Case", "name n env sched widths steps draw_widths")

WIDE = {"LFM_W4_MIN": "128", "LFM_W2_MIN": "128"}
W2 = {"LFM_W4_MIN": "1073741824", "LFM_W2_MIN": "128"}
HELPER = {"LFM_HELPER_MIN": "0", "LFM_HELPER_TC": "0"}
W0 = {"LFM_W0": "2"}
EVENTS = {"LFM_S3_EVENTS": "1"}
SIDE8 = {"LFM_SIDE_CUS": "8"}
S1 = {"LFM_SCHED": "1"}


def _env(*parts):
    out = {}
    for p in parts:
        out.update(p)
    return out


def knobs_of(env):
    """The plan's inputs as lfm_ctx.hip reads the environment and chol_factor_solve passes them on
    (CHOL_MLL on the context's schedule)."""
    g = lambda k: int(env.get(k, DEFAULTS[k]))  # noqa: E731
    s3 = g("LFM_SCHED") != 1
    w2 = g("LFM_W2_MIN")
    return dict(s3=int(s3), wbulk=WBULK_S3 if s3 else WBULK_S1, w4min=g("LFM_W4_MIN"),
                w2min=w2 if w2 >= 0 else (W2MIN_S3 if s3 else W2MIN_S1), w0=max(1, g("LFM_W0")),
                helper=g("LFM_HELPER"), tc=g("LFM_HELPER_TC"), hmin=g("LFM_HELPER_MIN"), cus=CUS,
                side=g("LFM_SIDE_CUS"))


def plan_input(name, n, env):
    """The case's line of chol_plan_check's stdin. A knob the environment does not set goes as "-"
    where S3Params has a default of its own (the helper's three, the side CUs)."""
    k = knobs_of(env)
    own = lambda key, v: v if key in env else "-"  # noqa: E731
    return (f"{name} {n} {k['s3']} {k['wbulk']} {k['w4min']} {k['w2min']} {k['w0']} "
            f"{own('LFM_HELPER', k['helper'])} {own('LFM_HELPER_TC', k['tc'])} "
            f"{own('LFM_HELPER_MIN', k['hmin'])} {k['cus']} {own('LFM_SIDE_CUS', k['side'])}")


def draw_plan_input(name, n, env):
    """... and of the draw's factorisation (CHOL_RESIDENT: schedule 1 whatever the context's)."""
    return plan_input(name, n, _env(env, {"LFM_SCHED": "1"}))


_RAW = []


def _add(name, n, env, widths, steps, draw_widths):
    sched = 1 if env.get("LFM_SCHED") == "1" else 3
    _RAW.append(Case(name, n, dict(env), sched, widths, steps, draw_widths))


# the w = 1 steps that end every default plan: bands from 9 trailing tiles down
_T9 = "9:1:B:0 8:1:B:0 7:1:B:0 6:1:B:0 5:1:B:0 4:1:B:0 3:1:B:0 2:1:B:0 "
_T8 = _T9[len("9:1:B:0 "):]
_END = "1:1:B:0 0:0:-:0"   # the last pivot block holds rows past it (the residual row at least)
_END0 = "1:0:-:0"          # n a multiple of 128: the residual row alone in a block of its own
_W12, _W13 = ",".join("1" * 12), ",".join("1" * 13)

# Default knobs: w = 1 throughout. 1471 / 1473: one row either side of a 64-row slab edge; 1535:
# the residual row inside the last pivot block; 1536: alone in a block of its own; from 1409 the
# first steps run the supertiled enumeration and the later ones bands.
_add("default_n129", 129, {}, "1,1", _END, "1,1")
_add("default_n1025", 1025, {}, ",".join("1" * 9), _T8 + _END, ",".join("1" * 9))
_add("default_n1409", 1409, {}, _W12, "11:1:S:0 10:1:S:0 " + _T9 + _END, _W12)
_add("default_n1471", 1471, {}, _W12, "11:1:S:0 10:1:S:0 " + _T9 + _END, _W12)
_add("default_n1473", 1473, {}, _W12, "11:1:S:0 10:1:S:0 " + _T9 + _END, _W12)
_add("default_n1535", 1535, {}, _W12, "11:1:S:0 10:1:S:0 " + _T9 + _END, _W12)
_add("default_n1536", 1536, {}, _W12, "12:1:S:0 11:1:S:0 10:1:S:0 " + _T9 + _END0, _W12)
_add("default_n1537", 1537, {}, _W13, "12:1:S:0 11:1:S:0 10:1:S:0 " + _T9 + _END, _W13)
# LFM_W4_MIN=128 LFM_W2_MIN=128: every fall-through of plan_steps (5 does not fit -> 4, -> 2,
# -> 1), per nblk at n = 128 nblk - 127, 128 nblk - 1 and 128 nblk; nblk = 13 also either side of
# the last block row's slab edge
_add("wide_b9_n1025", 1025, WIDE, "1,4,4", "8:4:B:0 4:4:B:0 0:0:-:0", "4,4,1")
_add("wide_b9_n1151", 1151, WIDE, "1,4,4", "8:4:B:0 4:4:B:0 0:0:-:0", "4,4,1")
_add("wide_b9_n1152", 1152, WIDE, "1,4,4", "9:4:B:0 5:4:B:0 1:0:-:0", "4,4,1")
_add("wide_b11_n1281", 1281, WIDE, "1,4,5,1", "10:4:B:0 6:5:B:0 1:1:B:0 0:0:-:0", "4,4,2,1")
_add("wide_b11_n1407", 1407, WIDE, "1,4,5,1", "10:4:B:0 6:5:B:0 1:1:B:0 0:0:-:0", "4,4,2,1")
_add("wide_b11_n1408", 1408, WIDE, "1,4,5,1", "11:4:B:0 7:5:B:0 2:1:B:0 1:0:-:0", "4,4,2,1")
_add("wide_b12_n1409", 1409, WIDE, "1,4,5,2", "11:4:B:0 7:5:B:0 2:2:B:0 0:0:-:0", "4,4,4")
_add("wide_b12_n1535", 1535, WIDE, "1,4,5,2", "11:4:B:0 7:5:B:0 2:2:B:0 0:0:-:0", "4,4,4")
_add("wide_b12_n1536", 1536, WIDE, "1,4,5,2", "12:4:B:0 8:5:B:0 3:2:B:0 1:0:-:0", "4,4,4")
_B13 = "12:4:B:0 8:5:B:0 3:2:B:0 1:1:B:0 0:0:-:0"
_add("wide_b13_n1537", 1537, WIDE, "1,4,5,2,1", _B13, "4,4,4,1")
_add("wide_b13_n1599", 1599, WIDE, "1,4,5,2,1", _B13, "4,4,4,1")
_add("wide_b13_n1601", 1601, WIDE, "1,4,5,2,1", _B13, "4,4,4,1")
_add("wide_b13_n1663", 1663, WIDE, "1,4,5,2,1", _B13, "4,4,4,1")
_add("wide_b13_n1664", 1664, WIDE, "1,4,5,2,1", "13:4:S:0 9:5:B:0 4:2:B:0 2:1:B:0 1:0:-:0",
     "4,4,4,1")
_add("wide_b14_n1665", 1665, WIDE, "1,4,5,4", "13:4:S:0 9:5:B:0 4:4:B:0 0:0:-:0", "4,4,4,2")
_add("wide_b14_n1791", 1791, WIDE, "1,4,5,4", "13:4:S:0 9:5:B:0 4:4:B:0 0:0:-:0", "4,4,4,2")
_add("wide_b14_n1792", 1792, WIDE, "1,4,5,4", "14:4:S:0 10:5:B:0 5:4:B:0 1:0:-:0", "4,4,4,2")
_add("wide_b15_n1793", 1793, WIDE, "1,4,5,5", "14:4:S:0 10:5:B:0 5:5:B:0 0:0:-:0", "4,4,4,2,1")
_add("wide_b15_n1919", 1919, WIDE, "1,4,5,5", "14:4:S:0 10:5:B:0 5:5:B:0 0:0:-:0", "4,4,4,2,1")
_add("wide_b15_n1920", 1920, WIDE, "1,4,5,5", "15:4:S:0 11:5:B:0 6:5:B:0 1:0:-:0", "4,4,4,2,1")
# LFM_W4_MIN=2^30 LFM_W2_MIN=128: w = 2 throughout, nblk = 8 and 9, ragged and full
_add("w2_b8_n897", 897, W2, "1,2,2,2,1", "7:2:B:0 5:2:B:0 3:2:B:0 1:1:B:0 0:0:-:0", "2,2,2,2")
_add("w2_b8_n1024", 1024, W2, "1,2,2,2,1", "8:2:B:0 6:2:B:0 4:2:B:0 2:1:B:0 1:0:-:0", "2,2,2,2")
_add("w2_b9_n1025", 1025, W2, "1,2,2,2,2", "8:2:B:0 6:2:B:0 4:2:B:0 2:2:B:0 0:0:-:0",
     "2,2,2,2,1")
_add("w2_b9_n1152", 1152, W2, "1,2,2,2,2", "9:2:B:0 7:2:B:0 5:2:B:0 3:2:B:0 1:0:-:0",
     "2,2,2,2,1")
# LFM_W0=2 (schedule 3's first super-panel two block columns wide), alone and with the wide knobs
_add("w0_b2_n255", 255, W0, "2", "0:0:-:0", "1,1")
_add("w0wide_b2_n129", 129, _env(WIDE, W0), "2", "0:0:-:0", "2")
_add("w0_b3_n383", 383, W0, "2,1", _END, "1,1,1")
_add("w0wide_b3_n257", 257, _env(WIDE, W0), "2,1", _END, "2,1")
_add("w0_b12_n1535", 1535, W0, "2" + ",1" * 10, "10:1:S:0 " + _T9 + _END, _W12)
_add("w0wide_b12_n1409", 1409, _env(WIDE, W0), "2,4,5,1", "10:4:B:0 6:5:B:0 1:1:B:0 0:0:-:0",
     "4,4,4")
# The side-CU helper forced (LFM_HELPER_MIN=0 LFM_HELPER_TC=0): n = 1408 is the smallest n whose
# default plan has a helped step (a supertiled rest region at a step s >= 1: Mp >= 1536), 2304 the
# smallest with the wide knobs (14 - 5 > 8 tile columns at step 1: Mp >= 2432); 1535, 2433 and 2559
# are ragged sizes of the same plans
_add("helper_n1408", 1408, HELPER, ",".join("1" * 11), "11:1:S:0 10:1:S:15 " + _T9 + _END0,
     ",".join("1" * 11))
_add("helper_n1535", 1535, HELPER, _W12, "11:1:S:0 10:1:S:15 " + _T9 + _END, _W12)
_add("helperwide_n2304", 2304, _env(WIDE, HELPER), "1,4,5,5,2,1",
     "18:4:S:0 14:5:S:30 9:5:B:0 4:2:B:0 2:1:B:0 1:0:-:0", "4,4,4,4,2")
_add("helperwide_n2433", 2433, _env(WIDE, HELPER), "1,4,5,5,5",
     "19:4:S:0 15:5:S:35 10:5:B:0 5:5:B:0 0:0:-:0", "4,4,4,4,4")
_add("helperwide_n2559", 2559, _env(WIDE, HELPER), "1,4,5,5,5",
     "19:4:S:0 15:5:S:35 10:5:B:0 5:5:B:0 0:0:-:0", "4,4,4,4,4")
# one wide ragged case with the launches ordered by events, one with a chain partition of 8 CUs
_add("events_b13_n1599", 1599, _env(WIDE, EVENTS), "1,4,5,2,1", _B13, "4,4,4,1")
_add("side8_b13_n1601", 1601, _env(WIDE, SIDE8), "1,4,5,2,1", _B13, "4,4,4,1")
# LFM_SCHED=1: look-ahead on every CU, bulk width 4, a wide first super-panel
_add("s1_b9_n1151", 1151, S1, ",".join("1" * 9), _T8 + _END, ",".join("1" * 9))
_add("s1wide_b9_n1025", 1025, _env(WIDE, S1), "4,4,1", "5:4:B:0 1:1:B:0 0:0:-:0", "4,4,1")
_add("s1_b12_n1535", 1535, S1, _W12, "11:1:S:0 10:1:S:0 " + _T9 + _END, _W12)
_add("s1wide_b12_n1409", 1409, _env(WIDE, S1), "4,4,4", "8:4:B:0 4:4:B:0 0:0:-:0", "4,4,4")
_add("s1_b13_n1663", 1663, S1, _W13, "12:1:S:0 11:1:S:0 10:1:S:0 " + _T9 + _END, _W13)
_add("s1wide_b13_n1537", 1537, _env(WIDE, S1), "4,4,4,1", "9:4:B:0 5:4:B:0 1:1:B:0 0:0:-:0",
     "4,4,4,1")

CASES = tuple(_RAW)
CASE = {c.name: c for c in CASES}
assert len(CASE) == len(CASES)

# Fault (d), Sigma rounded to fp32 on input, against the scalar's bound: the sizes of the table
# where the log density moves by fewer than 10 bounds, with the measured |d| / bound (numpy's
# Cholesky of the rounded matrix; every other size of the table is at 11 or more, n = 129 at 690).
# The rounding errors enter the scalar with random signs, so the figure swings with n (2.1 at 2559,
# 21 at 2433) and is no margin. The rows at these sizes — w2_b8_n897; wide_b9_n1152 and w2_b9_n1152;
# default_n1536 and wide_b12_n1536; default_n1537, wide_b13_n1537 and s1wide_b13_n1537;
# wide_b14_n1665; wide_b14_n1792; wide_b15_n1793; helperwide_n2304; helperwide_n2559 — see an fp32
# step through their draws alone, where the worst entry of L moves by 890 bounds or more.
FP32_SCALAR_UNDER_10 = {897: 4.9, 1152: 4.7, 1536: 9.0, 1537: 0.29, 1665: 6.5, 1792: 2.9,
                        1793: 1.9, 2304: 4.0, 2559: 2.1}


def draw_cases(cases=None):
    """One case per distinct (n, draw_widths), the first in the given order: the draws the device
    test makes. Every n of the table has at least one."""
    seen, out = set(), []
    for c in (CASES if cases is None else cases):
        if (c.n, c.draw_widths) not in seen:
            seen.add((c.n, c.draw_widths))
            out.append(c)
    return out


def env_key(env):
    return tuple(sorted(env.items()))


def cases_by_env():
    """The cases grouped by environment, in table order: [(env, [cases])]."""
    groups = {}
    for c in CASES:
        groups.setdefault(env_key(c.env), (c.env, []))[1].append(c)
    return list(groups.values())


# ------------------------------------------------------------------ the numpy restatement
Fault = namedtuple("Fault", "kind step ti tj k", defaults=(None, 0, 0, 0, 0))
# kind: "slice"  (a) the depth-4 slice [k, k + 4) of step `step`'s update of the 128 x 128 tile
#                    (block row ti, block column tj of the whole matrix, ti > tj) dropped
#       "slab"   (b) step `step`'s update of the 64-row slab ti (of the whole matrix) x block
#                    column tj skipped
#       "twice"  (c) step `step`'s update of tile (ti, tj) applied twice
#       "fp32"   (d) Sigma rounded to fp32 on input
#       "short"  (e) step `step` (a super-panel of w > 1) updates the next super-panel's diagonal
#                    block with depth kd - 128: its last block column left out


def blocked_cholesky(sigma, resid, widths, fault=None):
    """Right-looking blocked Cholesky of the augmented matrix as launch_augment lays it out
    (Mp = round_up(n + 1, 128); row n: the residual, unit pivot; rows past n: identity), over
    super-panels of the given widths (block columns of 128), the trailing update in units of one
    64-row slab x one 128-column tile. Returns (L, z, logp): the n x n factor, z = L^-1 resid and
    the log density. One fault (Fault) may be injected."""
    fault = fault or Fault()
    n = sigma.shape[0]
    Mp = round_up(n + 1, NB)
    nblk = (n + NB - 1) // NB
    assert sum(widths) == nblk, (widths, nblk)
    A = np.zeros((Mp, Mp))
    src = sigma.astype(np.float32).astype(np.float64) if fault.kind == "fp32" else sigma
    A[:n, :n] = np.tril(src)
    A[n, :n] = resid
    A[np.arange(n, Mp), np.arange(n, Mp)] = 1.0
    rows_end = n + 1  # the rows anything reads: pivots and the residual row
    k0 = 0
    for s, w in enumerate(widths):
        K0, K1 = k0 * NB, (k0 + w) * NB
        p1 = min(K1, n)  # pivots of this super-panel: columns [K0, p1)
        # the diagonal block's factor; the rows below (the residual row included) against it
        D = np.tril(A[K0:p1, K0:p1])
        L11 = np.linalg.cholesky(D + np.tril(D, -1).T)
        A[K0:p1, K0:p1] = L11
        if rows_end > p1:
            A[p1:rows_end, K0:p1] = np.linalg.solve(L11, A[p1:rows_end, K0:p1].T).T
        # trailing update from K1 with depth kd = p1 - K0 (columns past n hold no pivot)
        if K1 < rows_end:
            X = A[:, K0:p1]
            wn = widths[s + 1] if s + 1 < len(widths) else 0
            for tj in range(k0 + w, Mp // NB):
                c0, c1 = tj * NB, min((tj + 1) * NB, rows_end)
                if c0 >= rows_end:
                    break
                for ti in range(2 * tj, (rows_end + SLAB - 1) // SLAB):
                    r0, r1 = ti * SLAB, min((ti + 1) * SLAB, rows_end)
                    P, Q = X[r0:r1], X[c0:c1]
                    times = 1.0
                    if fault.step == s and fault.tj == tj:
                        if fault.kind == "slab" and fault.ti == ti:
                            times = 0.0
                        elif fault.kind == "twice" and fault.ti == ti // 2:
                            times = 2.0
                        elif fault.kind == "slice" and fault.ti == ti // 2:
                            k = fault.k
                            A[r0:r1, c0:c1] += P[:, k:k + 4] @ Q[:, k:k + 4].T
                    if (fault.kind == "short" and fault.step == s and w > 1 and
                            k0 + w <= tj < k0 + w + wn and ti // 2 < k0 + w + wn):
                        P, Q = P[:, :-NB], Q[:, :-NB]
                    A[r0:r1, c0:c1] -= times * (P @ Q.T)
        k0 += w
    L = np.tril(A[:n, :n])
    z = A[n, :n].copy()
    logdet = 2.0 * math.fsum(float(v) for v in np.log(np.diag(L).astype(np.longdouble)))
    logp = -0.5 * (n * math.log(2.0 * math.pi) + logdet + float(z @ z))
    return L, z, logp


def widths_of(case):
    return tuple(int(v) for v in case.widths.split(","))

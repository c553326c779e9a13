"""The blocked Cholesky (chol_factor_solve: lfm_chol.hip, lfm_chol_sched.hip) against matrices whose
factor is known exactly (tests/chol_cases.py), across its step plans: every case of the table that
tests/test_chol_cases_host.py pins to plan_steps / plan_s3.

  1. the log density through the context's schedule (lfm_log_prob_f64: CHOL_MLL), twice per case:
     both values within c max(1, |truth|) of the truth and equal bit for bit, on the schedule the
     case names, with no schedule-1 re-run; a NaN upper triangle changes no bit.
  2. the factor, element by element, through three joint draws (lfm_mvn_sample_f64: CHOL_RESIDENT on
     schedule 1, L left in A), once per distinct (n, draw width list) of the table, so at every
     size of it, the helper cases' included:
     |X - (loc + Z L0^T)| <= c (|Z| |L0|^T) + 4 eps |loc| with Z from lfm_randn_f64. The sample
     product's deep tiles (sample_depth above 384) run here. This is the check that sees an fp32
     step: an fp32-rounded Sigma moves the worst element of a draw with unit normals by 636 bounds or more at every size,
     but the log density by as little as 0.3 to 5 bounds at nine sizes of the table
     (chol_cases.FP32_SCALAR_UNDER_10).
  3. a failing pivot inside a wide panel: LFM_E_NOT_PD, NaN, the pivot named; the context then
     returns the unmodified matrix's value with its earlier bits.

c = (8 n eps + 4e-14) kappa (chol_cases.bound_c). Schedule 3 is observable only through the scalar:
its X_s lives in the double-buffered xbuf and is not kept, so the element-wise check is schedule
1's.

What the device run does not observe. The profiled third call of part 1 counts launches: one chain
launch per super-panel and one helper launch per helped step. That shows the knobs reached the
device and the plan has the expected number of steps; it does not show the widths themselves
(1,4,5,2 and 1,5,4,2 count alike) nor the helper's unit counts. Those are held on the CPU alone, by
the table against plan_steps / plan_s3 from the same knob values. The draws' schedule-1 width lists
(draw_widths) are not observed on the device at all; they too are the CPU check's word.

One context per environment (the knobs are read when a context is created), closed when the
next one is made and when the module ends. Every test prints its worst |d| / bound.

Measured on an MI355X, worst |d| / bound over the cases: log density 1.2e-4 on schedule 3
(w0wide_b3_n257) and 1.3e-5 on schedule 1 (s1wide_b12_n1409); draws 1.9e-3 (default_n129).
"""

import ctypes
import os

import numpy as np
import pytest

from tests import chol_cases as C

pytestmark = pytest.mark.gpu

KNOBS = ("LFM_SCHED", "LFM_S3_EVENTS", "LFM_W4_MIN", "LFM_W2_MIN", "LFM_W0", "LFM_HELPER",
         "LFM_HELPER_TC", "LFM_HELPER_MIN", "LFM_SIDE_CUS", "LFM_S3_FALLBACK")
SEED, SAMPLE0, NSAMP = 11, 2, 3

# the cases in table order, grouped by environment: one context per group
ORDERED = [c for _, group in C.cases_by_env() for c in group]
DRAWN = C.draw_cases(ORDERED)  # one draw per distinct (n, draw width list): every size draws


class _Current:
    key = None
    ctx = None
    worst = {}


def _close():
    if _Current.ctx is not None:
        _Current.ctx.close()
    _Current.ctx = _Current.key = None


def context_for(env):
    """A context created under `env` (and no other knob of KNOBS); the previous one is closed."""
    from dis_project_amd import _lib

    key = C.env_key(env)
    if _Current.key == key and _Current.ctx is not None:
        return _Current.ctx
    _close()
    saved = {k: os.environ.pop(k) for k in KNOBS if k in os.environ}
    try:
        os.environ.update(env)
        _Current.ctx = _lib.Context(0)
        _Current.key = key
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(saved)
    return _Current.ctx


@pytest.fixture(scope="module", autouse=True)
def contexts():
    try:
        yield
    finally:
        _close()
        for what, (ratio, name) in sorted(_Current.worst.items()):
            print(f"\nworst |d| / bound, {what}: {ratio:.3e} ({name})")


def note(what, name, ratio):
    if ratio > _Current.worst.get(what, (-1.0, ""))[0]:
        _Current.worst[what] = (ratio, name)


def log_prob(ctx, p, scale=None, expect=0):
    from dis_project_amd import _lib

    n = p["n"]
    scale = p["Sigma"] if scale is None else scale
    out = np.full(1, 7.0)
    rc = ctx.lib.lfm_log_prob_f64(ctx.handle, _lib.dptr(p["loc"]), _lib.dptr(scale), n, n,
                                  _lib.dptr(p["y"]), _lib.dptr(out))
    assert rc == expect, (rc, ctx.lib.lfm_last_error(ctx.handle))
    return float(out[0])


def last_schedule(ctx):
    out = ctypes.c_int(0)
    ctx.check(ctx.diag.lfm_debug_last_schedule(ctx.handle, ctypes.byref(out)))
    return out.value


# ------------------------------------------------------------------ 1. the log density
@pytest.mark.parametrize("case", ORDERED, ids=[c.name for c in ORDERED])
def test_log_density_on_the_case_schedule(case):
    p = C.exact_factor(case.n)
    ctx = context_for(case.env)
    fallbacks = ctx.fallbacks
    bound = C.logp_bound(p)
    got = [log_prob(ctx, p), log_prob(ctx, p)]  # the second reuses workspace, flags and counters
    ratio = max(abs(v - p["truth"]) for v in got) / bound
    print(f"{case.name} (widths {case.widths}): logp {got[0]!r}, truth {p['truth']!r}, "
          f"|d| / bound = {ratio:.3e} (bound {bound:.2e}, kappa {p['kappa']:.2f})")
    note(f"log density, schedule {case.sched}", case.name, ratio if ratio == ratio else np.inf)
    assert last_schedule(ctx) == case.sched
    assert ctx.fallbacks == fallbacks  # no silent schedule-1 re-run
    assert np.isfinite(got[0]) and ratio <= 1.0
    assert got[0] == got[1]
    if case.sched == 3:
        # the knobs reached the device: one chain launch per super-panel of the case's width list,
        # one helper launch per helped step (none when the launches are ordered by events)
        ctx.profile(True, classes=["potrf", "syrk_side"])
        try:
            ctx.profile_reset()
            third = log_prob(ctx, p)
            st = ctx.profile_read()
        finally:
            ctx.profile(False)
            ctx.profile_reset()
        helped = sum(not f.endswith(":0") for f in case.steps.split())
        assert st["potrf"]["launches"] == len(C.widths_of(case)), st["potrf"]
        assert st.get("syrk_side", {}).get("launches", 0) == helped
        assert third == got[0]


def test_nan_upper_triangle_changes_no_bit():
    case = C.CASE["wide_b13_n1599"]
    p = C.exact_factor(case.n)
    ctx = context_for(case.env)
    full = log_prob(ctx, p)
    upper = p["Sigma"].copy()
    upper[np.triu_indices(case.n, 1)] = np.nan
    assert log_prob(ctx, p, upper) == full  # only the lower triangle is read
    assert last_schedule(ctx) == 3


# ------------------------------------------------------------------ 2. the factor, through draws
@pytest.mark.parametrize("case", DRAWN, ids=[c.name for c in DRAWN])
def test_factor_element_by_element_through_draws(case):
    from dis_project_amd import _lib

    p = C.exact_factor(case.n)
    n = case.n
    ctx = context_for(case.env)
    z = np.full((NSAMP, n), 7.0)
    ctx.check(ctx.lib.lfm_randn_f64(ctx.handle, SEED, SAMPLE0, NSAMP, n, _lib.dptr(z)))
    x = np.full((NSAMP, n), 7.0)
    ctx.check(ctx.lib.lfm_mvn_sample_f64(ctx.handle, _lib.dptr(p["loc"]), _lib.dptr(p["Sigma"]),
                                         n, n, SEED, SAMPLE0, NSAMP, _lib.dptr(x)))
    assert last_schedule(ctx) == 1
    ref = p["loc"] + z @ p["L0"].T
    r = np.abs(x - ref) / C.draw_bound(p, z)
    assert np.all(np.isfinite(x))
    s, j = np.unravel_index(int(np.argmax(r)), r.shape)
    ratio = float(r[s, j])
    print(f"{case.name} (draw widths {case.draw_widths}): worst |d| / bound = {ratio:.3e} at "
          f"sample {s}, element {j} (128-block {j // 128}, row {j % 128})")
    note("draws, schedule 1", case.name, ratio)
    assert ratio <= 1.0


# ------------------------------------------------------------------ 3. failures in a wide panel
def test_failing_pivot_inside_a_wide_panel():
    from dis_project_amd import _lib

    case = C.CASE["wide_b13_n1537"]
    assert case.widths == "1,4,5,2,1"  # block columns 0 | 1-4 | 5-9 | 10-11 | 12
    p = C.exact_factor(case.n)
    n = case.n
    ctx = context_for(case.env)
    good = log_prob(ctx, p)
    assert abs(good - p["truth"]) <= C.logp_bound(p)
    # the first and the last column of the w = 5 panel, a column of the w = 2 panel, the last pivot
    for j in (5 * 128, 10 * 128 - 1, 10 * 128 + 120, n - 1):
        bad = p["Sigma"].copy()
        bad[j, j] -= 1.5 * p["L0"][j, j] ** 2  # pivot j: L0_jj^2 - 1.5 L0_jj^2 < 0, exactly
        out = log_prob(ctx, p, bad, expect=_lib.LFM_E_NOT_PD)
        msg = ctx.lib.lfm_last_error(ctx.handle).decode()
        print(f"pivot {j}: {msg}")
        assert np.isnan(out)
        assert msg.endswith(f"index {j}"), msg
        assert log_prob(ctx, p) == good  # the same context, the earlier bits
    assert last_schedule(ctx) == 3

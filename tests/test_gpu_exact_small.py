"""The small-problem batch (lfm_batch_mll_f64, lfm_batch_mll_grad_f64, lfm_batch_fit_f64,
lfm_batch_posterior_f64; the kernels of lfm_small.hip) against extended-precision truth at C3's
restarts, at the edges of every variant the kernels choose between.

tests/test_gpu_batch_grad.py and test_gpu_batch_predict.py compare with oracle.mll_grad and
oracle.multi_gene_predict at benign hyperparameters; at the restarts those oracles are wrong by
up to 9e-2 of the gradient's scale at these very shapes (tests/test_exact_small_host.py). Until
now the small batch met the truth at n = 28 on the 7-time grid (the C5 rounds, fixture a of the
posterior) and at n = 48 off the grid alone. Which code runs depends on n (the factor on two lanes
a row, one wave or two waves; the sweep on two lanes a row, one wave or four waves), on the
layout (grid tables, KxxTab, kernel_ref; derivative tables or per-pair duals), and on the launch
(KxxTab in the value call only when every problem has n + 1 <= 64; the problem table in the kernel
arguments up to 16 problems, else in memory); the fit wraps all of it in a kernel of its own.
tests/small_exact_inputs.py lists the cases and says which edge each one is.

The truth is tests/golden/exact_small.npz (make_golden_exact_small.py), the bounds the fixture's,

    |value - truth| <= mll_rtol |truth|                        (mll_rtol = 1e-9)
    |g - g_exact|   <= grad_rtol scale + 1e-10 |g_exact|       (grad_rtol = 1e-8)
    max|d|          <= post_rtol max|truth| + 1e-12            (post_rtol = 1e-9)

in the helper forms of tests/test_gpu_exact_grad.py and test_gpu_exact_posterior.py. Every batch
is evaluated once per module (the fixture `runs`); the tests judge the results, print their worst
figure and where it occurs, and check status 0 everywhere and both signs of `negative`.

The diagnostic lines (not assertions) give, at the ill-conditioned restarts, the batch's distance
from lfm_mll_grad_f64 / lfm_posterior_f64 on the same inputs in units of the bound: far from both
the single call and the truth points to this kernel, near the single call and far from the truth
to the entry code the two share.

On the MI355X every case is within 3.3e-4 of its bound. One check found a bug, which is fixed:
test_gradient_calls_value_is_the_value_calls (the header's "the same bits").
"""

import numpy as np
import pytest

from tests import small_exact_inputs as I
from tests.conftest import load_golden
from tests.test_gpu_exact_grad import figures, grad_call, pack_dict, ratio_of
from tests.test_gpu_exact_posterior import dadd_of, full_of, posterior_call, ratio

pytestmark = pytest.mark.gpu

LE63 = tuple(c for c in I.CASES if c[1] * c[2] <= 63)
# exactly 16 problems: group S at restarts ILL and 4 x 24 (one wave and four waves in one launch)
ARGS16 = tuple((c[0], c[1], c[2], c[3], I.ILL, c[5]) for c in I.FIT_CASES) + \
    (I.case_of("e4x24"),)
COMPOSITIONS = {"values": {"all": I.CASES, "le63": LE63},
                "grads": {"all": I.GRAD_CASES, "le63": LE63, "args16": ARGS16}}


@pytest.fixture(scope="module")
def sx():
    g = load_golden("exact_small")
    assert tuple(int(r) for r in g["ill"]) == I.ILL
    return g


def members(cases):
    """[(case name, index into the case's fixture rows, restart, x, y, model)] of `cases`."""
    out = []
    for name, G, T, shuffled, restarts, _ in cases:
        every = I.case_of(name)[4]
        out += [(name, every.index(r), r) + I.problem(G, T, shuffled, r) for r in restarts]
    return out


def evaluator(mem, negative=False):
    import dis_project_amd as lfm
    from dis_project_amd import _lib, farm

    return farm.BatchEvaluator(_lib.get_context(0),
                               [lfm.Dataset(m[3], m[4].reshape(-1, 1)) for m in mem],
                               negative=negative)


class Runs:
    """The batches' results, each evaluated once and then left unchanged."""

    def __init__(self):
        self._done = {}

    def _once(self, key, fn):
        if key not in self._done:
            self._done[key] = fn()
        return self._done[key]

    def values(self, comp):
        """(members, {negative: (values, statuses)}) of lfm_batch_mll_f64 on one handle."""
        def run():
            mem = members(COMPOSITIONS["values"][comp])
            ev = evaluator(mem)
            try:
                out = {}
                for negative in (False, True):
                    ev.negative = negative
                    vals = ev([m[5] for m in mem])
                    out[negative] = (vals, ev.status.copy())
                return mem, out
            finally:
                ev.close()
        return self._once(("values", comp), run)

    def grads(self, comp):
        """(members, {negative: (values, packed gradients, statuses, the value call's values on
        the same handle)}) of lfm_batch_mll_grad_f64."""
        def run():
            mem = members(COMPOSITIONS["grads"][comp])
            models = [m[5] for m in mem]
            ev = evaluator(mem)
            try:
                out = {}
                for negative in (False, True):
                    ev.negative = negative
                    vals, grads = ev.value_and_grad(models)
                    status = ev.status.copy()
                    out[negative] = (vals, [pack_dict(g) for g in grads], status, ev(models))
                return mem, out
            finally:
                ev.close()
        return self._once(("grads", comp), run)

    def fit(self):
        """(members, {negative: (history [1, P], the gradients recovered from mu, statuses)}) of
        one lfm_batch_fit_f64 step of group S from zero moments."""
        def run():
            from dis_project_amd import farm, trainer as tr

            mem = members(I.FIT_CASES)
            models = [m[5] for m in mem]
            genes = [int(m.num_genes) for m in models]
            ev = evaluator(mem)
            try:
                ev.registered(genes)
                out = {}
                for negative in (False, True):
                    ev.negative = negative
                    raw = tr.pack_raw([tr.unconstrain(m) for m in models],
                                      [m.jitter for m in models])
                    raw0 = raw.copy()
                    mu, nu = np.zeros_like(raw), np.zeros_like(raw)
                    hist, st = ev.fit_packed(raw, mu, nu, tr.adam(0.01, 0.9, 0.999, 1e-8, 0.0),
                                             False, 1000, 0, 1)
                    # fit_update: mu = (1 - b1) g c, c the bijector's derivative at raw (softplus:
                    # sigmoid; l = 0.5 + 3 sigmoid: 3 sigmoid (1 - sigmoid)); the jitter slot is
                    # static (mu stays 0)
                    c = tr.sigmoid(raw0)
                    nvec = 3 * sum(genes)
                    c[nvec::3] = 3.0 * c[nvec::3] * (1.0 - c[nvec::3])
                    c[nvec + 2::3] = 1.0
                    assert np.all(mu[nvec + 2::3] == 0.0)
                    g = mu / ((1.0 - 0.9) * c)
                    out[negative] = (hist, [pack_dict(d) for d in farm.unpack_grads(g, genes)], st)
                return mem, out
            finally:
                ev.close()
        return self._once("fit", run)

    def post(self):
        """(members with v and t, {kind: ([(mean, var, cov)], statuses, rc)}) of group P: one
        lfm_batch_posterior_f64 per diagonal, the latent one without the covariance."""
        def run():
            from dis_project_amd import _lib, predict as P

            mem = []
            for name, G, T, shuffled in I.POST:
                for q, r in enumerate(I.ILL):
                    mem.append((name, q, r) + I.problem(G, T, shuffled, r)
                               + I.post_extra(G, T, shuffled, r))
            models = [m[5] for m in mem]
            ctx = _lib.get_context(0)
            ev = evaluator(mem)
            try:
                hyp = ev.pack(models)
                tt, mm = P.pack_test_inputs([m[7] for m in mem], [m.num_genes for m in models])
                dv = np.ascontiguousarray(np.concatenate([m[6] for m in mem]))
                out = {}
                for kind, want_cov in ((0, False), (1, True)):
                    dadd = np.array([dadd_of(m, kind) for m in models])
                    mean, var = np.full(int(mm.sum()), 7.0), np.full(int(mm.sum()), 7.0)
                    cov = np.full(int((mm * mm).sum()), 7.0) if want_cov else None
                    st = np.full(len(mem), -9, np.int32)
                    rc = ctx.lib.lfm_batch_posterior_f64(
                        ctx.handle, ev.batch, _lib.dptr(hyp), _lib.dptr(dv), _lib.dptr(dadd),
                        _lib.dptr(mm), _lib.dptr(tt), _lib.dptr(mean), _lib.dptr(var),
                        _lib.dptr(cov) if want_cov else None, _lib.dptr(st))
                    out[kind] = (P.unpack_outputs(mm, mean, var, cov), st, rc)
                return mem, out
            finally:
                ev.close()
        return self._once("post", run)


@pytest.fixture(scope="module")
def runs():
    return Runs()


def label(m):
    return f"{m[0]} r{m[2]} (n = {m[3].shape[0]})"


def judge(sx, mem, vals, grads, negative, what):
    """Every member's figures (tests/test_gpu_exact_grad.figures; the gradient's only with
    `grads`), the worst of each printed with its place, and the list of what is outside."""
    bad, worst = [], [(-1.0, None), (-1.0, None)]
    for i, m in enumerate(mem):
        # without gradients the truth's own stands in: only the value's figure is then read
        truth = sx[m[0] + "_grad"][m[1]] * (-1.0 if negative else 1.0)
        gv = grads[i] if grads is not None else truth
        figs = figures(sx, m[0], m[1], float(vals[i]), gv, negative)
        figs = [np.nan_to_num(f, nan=np.inf) for f in figs][:2 if grads is not None else 1]
        for k, f in enumerate(figs):
            if f > worst[k][0]:
                worst[k] = (f, label(m))
            if not f <= 1.0:
                bad.append((label(m), ("value", "gradient")[k], float(f)))
        if grads is not None and not np.all(np.isfinite(grads[i])):
            bad.append((label(m), "non-finite gradient", float("inf")))
    print(f"{what} negative={bool(negative)}: worst |dvalue| / (mll_rtol |value|) = "
          f"{worst[0][0]:.3e} at {worst[0][1]}"
          + (f", worst |dg| / bound = {worst[1][0]:.3e} at {worst[1][1]}" if grads is not None
             else "") + f" over {len(mem)} problems")
    for b in bad:
        print(f"  OUTSIDE: {b[0]} {b[1]} {b[2]:.3e}")
    return bad


# ------------------------------------------------------------------------- values
@pytest.mark.parametrize("comp", ["all", "le63"])
def test_values_vs_truth(sx, runs, comp):
    """lfm_batch_mll_f64. "all": every case in one batch; with n up to 128 in it the launch has no
    KxxTab (the off-grid n = 63 problems take kernel_ref) and reads the problem table from memory.
    "le63": the n <= 63 cases alone, KxxTab on. The n <= 63 problems are judged against the truth
    in both (nothing is asserted between the two compositions' bits)."""
    mem, out = runs.values(comp)
    sizes = sorted({m[3].shape[0] for m in mem})
    assert sizes[-1] == (128 if comp == "all" else 63) and len(mem) > 16
    bad = []
    for negative in (False, True):
        vals, status = out[negative]
        assert np.all(status == 0), [(label(m), s) for m, s in zip(mem, status) if s]
        bad += judge(sx, mem, vals, None, negative, f"values[{comp}]")
    assert not bad, bad


# ------------------------------------------------------------- value and gradient
def against_single(sx, mem, vals, grads, what):
    """The diagnostic lines at restarts ILL (negative = False): the batch's distance from
    lfm_mll_grad_f64 on the same inputs, and that call's from the truth, in units of the bound."""
    from dis_project_amd import _lib

    ctx = _lib.get_context(0)
    for i, m in enumerate(mem):
        name, q, r, x, y, model = m
        if r not in I.ILL:
            continue
        bval, bgv = grad_call(ctx, x, y, model, 0)
        mll = float(sx[name + "_mll"][q])
        bound = float(sx[name + "_grad_rtol"][q]) * sx[name + "_scale"][q] + \
            1e-10 * np.abs(sx[name + "_grad"][q])
        big = figures(sx, name, q, bval, bgv, False)
        print(f"{what} {label(m)}: batch - lfm_mll_grad_f64 in units of the bound: value "
              f"{abs(vals[i] - bval) / (float(sx[name + '_mll_rtol'][q]) * abs(mll)):.3e}, "
              f"gradient {float(np.max(np.abs(grads[i] - bgv) / bound)):.3e}; lfm_mll_grad_f64 - "
              f"truth: value {big[0]:.3e}, gradient {big[1]:.3e}")


@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("comp", ["all", "le63", "args16"])
def test_value_and_gradient_vs_truth(sx, runs, comp, negative):
    """lfm_batch_mll_grad_f64. "all": every gradient case, 128 problems, the problem table read
    from memory; "le63": the n <= 63 cases alone; "args16": exactly 16 problems (group S at
    restarts ILL and 4 x 24), the table in the kernel arguments. Every status 0, every value and
    every gradient component inside its bound."""
    mem, out = runs.grads(comp)
    assert (len(mem) == 16) == (comp == "args16") and (comp == "args16" or len(mem) > 16)
    vals, grads, status, _ = out[negative]
    assert np.all(status == 0), [(label(m), s) for m, s in zip(mem, status) if s]
    bad = judge(sx, mem, vals, grads, negative, f"grads[{comp}]")
    if comp == "all" and not negative:
        against_single(sx, mem, vals, grads, "grads[all]")
    assert not bad, bad
    for i, m in enumerate(mem):  # the helper's own assertions, problem by problem
        assert ratio_of(sx, m[0], m[1], float(vals[i]), grads[i], negative) <= 1.0, label(m)


def test_gradient_calls_value_is_the_value_calls(sx, runs):
    """include/lfm.h on lfm_batch_mll_grad_f64: "value[p] as its [lfm_batch_mll_f64's] out[p]
    (the same bits)". Both calls on one handle, the three compositions, both signs.

    This test found a bug. 116 of the 256 values of "all" (38 of 160 of "le63", 20 of 32 of
    "args16") differed from the value call's, by at most 2.0e-14 relative (3 x 21 at restart 1,
    n = 63), both within 8.7e-5 of mll_rtol |truth| of the truth: since the sweep operator went
    in, the gradient and the fit took logdet and the quadratic form from its pivots
    (small_sweep_half / small_sweep_regs / small_sweep4) and the value call from a Cholesky factor
    in registers (small_factor_regs / small_factor_regs2); two eliminations of the same Sigma do
    not round alike, and the header's sentence is older than the sweep. small_value_grad now
    takes the value from the value call's own factor: wave 1 runs it beside wave 0's sweep when
    n + 1 <= 64, every wave before the four-wave sweep above that. The gradients kept their
    bits."""
    bad = []
    for comp in ("all", "le63", "args16"):
        mem, out = runs.grads(comp)
        worst, where, count = 0.0, None, 0
        for negative in (False, True):
            vals, _, _, only = out[negative]
            for i, m in enumerate(mem):
                rel = abs(vals[i] - only[i]) / abs(only[i])
                count += int(vals[i] != only[i])
                if rel > worst:
                    worst, where = rel, label(m)
        print(f"grads[{comp}]: {count} of {2 * len(mem)} values differ from the value call's; "
              f"largest relative difference {worst:.3e} at {where}")
        if count:
            bad.append((comp, count, worst, where))
    assert not bad, bad


# ---------------------------------------------------------------- the fit's first step
@pytest.mark.parametrize("negative", [False, True])
def test_fit_first_step_vs_truth(sx, runs, negative):
    """lfm_batch_fit_f64 on group S (96 problems): one step from raw = unconstrain(model) and
    zero moments under adam(0.01, 0.9, 0.999, 1e-8, 0), fix_params = 0. history[0] is the value,
    held to its bound; the returned mu is (1 - b1) g c with c the bijector's derivative, so
    g = mu / ((1.0 - 0.9) c), recovered on the host, is the fit kernel's own gradient and is held
    to the gradient's bound (the recovery and the device's constrain of raw cost a few ulp, orders
    inside the 1e-10 |g| and 1e-8 scale terms). The parameter update from zero moments is
    -lr sign(g) and is not judged."""
    mem, out = runs.fit()
    hist, grads, status = out[negative]
    assert hist.shape == (1, len(mem)) and len(mem) == 96
    assert np.all(status == 0), [(label(m), s) for m, s in zip(mem, status) if s]
    bad = judge(sx, mem, hist[0], grads, negative, "fit step 0")
    assert not bad, bad


# ------------------------------------------------------------------------ posterior
def test_posterior_vs_truth(sx, runs):
    """lfm_batch_posterior_f64 on group P (4 x 16 on and off the grid, 1 x 127 off the grid with
    the narrowest panel, 16 columns; restarts ILL; m = 20 with t = 0 rows, gene indices -1 and G,
    latent and mixed rows): one batch per diagonal, the latent one without the covariance. Mean,
    var and cov inside post_rtol of the truth, var equal to diag(cov) bit for bit, cov exactly
    symmetric."""
    from dis_project_amd import _lib

    mem, out = runs.post()
    assert len(mem) == 12
    bad, worst, where = [], np.zeros(3), [None] * 3
    for kind, (res, st, rc) in sorted(out.items()):
        assert rc == 0 and np.all(st == 0), (kind, rc, st)
        for m, (mean, var, cov) in zip(mem, res):
            name, q = m[0], m[1]
            assert not sx[name + "_dropped"][q, kind] and not sx[name + "_not_pd"][q, kind]
            rtol = float(sx[name + "_rtol"][q, kind])
            ref = full_of(sx[name + "_cov"][q, kind], 20)
            figs = [ratio(mean, sx[name + "_mean"][q, kind], rtol),
                    ratio(var, np.diagonal(ref), rtol)]
            if kind == 1:
                np.testing.assert_array_equal(var, np.diagonal(cov))
                np.testing.assert_array_equal(cov, cov.T)
                figs.append(ratio(cov, ref, rtol))
            else:
                assert cov is None
            print(f"{label(m)}, {'gene' if kind else 'latent'} diagonal: |d| / bound mean, var"
                  f"{', cov' if kind else ''} = " + " ".join(f"{f:.2e}" for f in figs))
            for k, f in enumerate(figs):
                if not f <= worst[k]:
                    worst[k], where[k] = f, (label(m), "gene" if kind else "latent")
            if not max(figs) <= 1.0:
                bad.append((label(m), kind, [round(f, 3) for f in figs]))
    print("posterior: worst |d| / bound mean, var, cov = " + " ".join(f"{f:.2e}" for f in worst)
          + f" at {where}")
    # the diagnostic lines: the batch against lfm_posterior_f64 on the same inputs
    ctx = _lib.get_context(0)
    for i, m in enumerate(mem):
        name, q, _, x, y, model, v, t = m
        for kind in (0, 1):
            rc, smean, scov = posterior_call(ctx, x, y, v, dadd_of(model, kind), t, model)
            rtol = float(sx[name + "_rtol"][q, kind])
            ref = full_of(sx[name + "_cov"][q, kind], 20)
            mean, var, _ = out[kind][0][i]
            print(f"{label(m)}, {'gene' if kind else 'latent'} diagonal: batch - "
                  f"lfm_posterior_f64 in units of the bound: mean "
                  f"{ratio(mean, smean, rtol) if rc == 0 else float('nan'):.2e}, var "
                  f"{ratio(var, np.diagonal(scov), rtol) if rc == 0 else float('nan'):.2e}; "
                  f"lfm_posterior_f64 - truth: mean "
                  f"{ratio(smean, sx[name + '_mean'][q, kind], rtol):.2e}, cov "
                  f"{ratio(scov, ref, rtol):.2e} (rc {rc})")
    assert not bad, bad

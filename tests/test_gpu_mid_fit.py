"""The on-device fit of the mid-size resident batch on the GPU (lfm_mbatch_fit_f64,
farm.MidBatchEvaluator.fit_packed, trainer.MidBatchTrainer(on_device=True)): every problem's Adam
loop with no host round trip between steps.

One mixed batch crosses every edge: n = 28, 63, 128, 129, 192, 320 (1, 1, 3, 3, 4 and 6 block
rows), G <= 3 (after_epoch is a no-op) and G > 3 (index 3 is pinned), 10 steps of adam(0.01) on
-MLL with after_epoch every 4 steps. It is held to each problem's own JaxTrainer loop on the
oracle (complex-step derivatives of the reference kernel, on the CPU) and to the host loop on the
same GPU evaluator, at the bounds of test_mid_batch_trainer_matches_oracle_loops: the history
within 1e-9 relative, the fitted parameters within 1e-8. The oracle loops and the batch's fit are
computed once per process and shared."""

import functools

import numpy as np
import pytest

from tests.test_gpu_mid_batch import _edge

pytestmark = pytest.mark.gpu

BATCH = ((4, 7), (1, 63), (2, 64), (3, 43), (3, 64), (5, 64))
STEPS, SPE = 10, 4
PARAMS = ("true_d", "true_s", "true_b", "l")


def _problems():
    return [_edge(G, T) for G, T in BATCH]


@functools.lru_cache(maxsize=None)
def _oracle_loop(G, T):
    """(fitted model, history) of the problem's own JaxTrainer loop on the oracle."""
    from dis_project_amd import trainer as TR
    from tests.test_trainer import OracleObjective

    m, d = _edge(G, T)
    jt = TR.JaxTrainer(m, OracleObjective(True), d, TR.adam(0.01), num_iters=STEPS)
    return jt.fit(fix_params=True, num_steps_per_epoch=SPE)


def _evaluator(problems, negative=True):
    from dis_project_amd import _lib, farm

    return farm.MidBatchEvaluator(_lib.get_context(), [d for _, d in problems], negative)


def _start(problems):
    """raw, mu, nu of a fit's start in the packed layout."""
    from dis_project_amd import trainer as TR

    raw = TR.pack_raw([TR.unconstrain(m) for m, _ in problems], [m.jitter for m, _ in problems])
    return raw, np.zeros_like(raw), np.zeros_like(raw)


def _call(ev, problems, state, nsteps, step0=0, fix=True, spe=SPE, lr=0.01):
    """One lfm_mbatch_fit_f64 call on ev's handle: (rc, history, status); state in place."""
    from dis_project_amd import _lib

    ev.registered([m.num_genes for m, _ in problems])
    raw, mu, nu = state
    hist = np.full((nsteps, len(problems)), -7.0)
    st = np.full(len(problems), -7, np.int32)
    opt = _lib.LfmAdam(lr, 0.9, 0.999, 1e-8, 0.0, spe, int(fix))
    rc = ev.ctx.lib.lfm_mbatch_fit_f64(ev.ctx.handle, ev.batch, _lib.ctypes.byref(opt),
                                       int(ev.negative), step0, nsteps, _lib.dptr(raw),
                                       _lib.dptr(mu), _lib.dptr(nu), _lib.dptr(hist),
                                       _lib.dptr(st))
    return rc, hist, st


def _fit(problems, nsteps=STEPS, negative=True, **kw):
    """A fresh handle, one call from the start: (rc, history, status, (raw, mu, nu))."""
    ev = _evaluator(problems, negative)
    try:
        state = _start(problems)
        rc, hist, st = _call(ev, problems, state, nsteps, **kw)
        return rc, hist, st, state
    finally:
        ev.close()


@functools.lru_cache(maxsize=None)
def _batch_fit():
    """The mixed batch's clean 10-step fit, once."""
    from dis_project_amd import _lib

    rc, hist, st, state = _fit(_problems())
    assert rc == _lib.LFM_OK and not st.any()
    return hist, state


def _per_problem(packed, problems):
    from dis_project_amd import trainer as TR

    return TR.unpack_raw(packed, [m.num_genes for m, _ in problems])


def _same_problem_bits(a, b):
    for k in ("true_d", "true_s", "true_b", "l", "obs_stddev"):
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]))


def _worst(got, want):
    got, want = np.atleast_1d(np.asarray(got, float)), np.atleast_1d(np.asarray(want, float))
    return float(np.max(np.abs(got - want) / np.abs(want)))


def _check_fit(fitted, hist, want, what):
    """want: [(model, history)] per problem; the worst ratios are printed before they are held
    to rtol 1e-9 (history) and 1e-8 (parameters)."""
    for p, (wm, wh) in enumerate(want):
        eh = _worst(hist[p], wh)
        ep = max(_worst(getattr(fitted[p], k), getattr(wm, k)) for k in PARAMS)
        print(f"{what}, problem {p} (G = {wm.num_genes}): history worst rel err {eh:.3e} "
              f"(/1e-9 = {eh / 1e-9:.3e}), parameters {ep:.3e} (/1e-8 = {ep / 1e-8:.3e})")
    for p, (wm, wh) in enumerate(want):
        np.testing.assert_allclose(hist[p], wh, rtol=1e-9, atol=0)
        for k in ("true_d", "true_s", "true_b"):
            np.testing.assert_allclose(getattr(fitted[p], k), getattr(wm, k), rtol=1e-8, atol=0)
        assert fitted[p].l == pytest.approx(wm.l, rel=1e-8)


@functools.lru_cache(maxsize=None)
def _trainer_fit(on_device):
    """The mixed batch through MidBatchTrainer on the GPU evaluator: (fitted, history, status)."""
    import dis_project_amd as lfm
    from dis_project_amd import trainer as TR

    probs = _problems()
    bt = TR.MidBatchTrainer([m for m, _ in probs], lfm.CustomConjMLL(negative=True),
                            [d for _, d in probs], TR.adam(0.01), num_iters=STEPS,
                            on_device=on_device)
    try:
        fitted, hist = bt.fit(fix_params=True, num_steps_per_epoch=SPE)
        return fitted, hist, bt.status
    finally:
        bt.close()


# ------------------------------------------------------------------ 1. the oracle's loops
def test_on_device_fit_matches_oracle_loops():
    fitted, hist, status = _trainer_fit(True)
    assert hist.shape == (len(BATCH), STEPS) and not np.asarray(status).any()
    _check_fit(fitted, hist, [_oracle_loop(G, T) for G, T in BATCH], "vs the oracle loop")
    # after_epoch once more on the constrained model (G > 3: index 3 pinned)
    for m in fitted:
        if m.num_genes > 3:
            assert m.true_s[3] == 1.0 and m.true_d[3] == 0.8
    # the trainer's one call is the C call on the same start
    ref_hist, _ = _batch_fit()
    np.testing.assert_array_equal(hist, ref_hist.T)


# ------------------------------------------------------------------ 2. the host loop
def test_on_device_fit_matches_the_host_loop():
    """The same batch through the host loop on the GPU evaluator: the gradient kernels are the
    same code, so a mismatch isolates the update kernel."""
    fitted, hist, _ = _trainer_fit(True)
    host, host_hist, _ = _trainer_fit(False)
    _check_fit(fitted, hist, list(zip(host, host_hist)), "vs the host loop")


# ------------------------------------------------------------------ 3. bits
def test_resumed_fit_equals_the_one_call_fit():
    """4 + 6 steps with step0 = 4: the epoch boundary at step 4 lies exactly on the split."""
    from dis_project_amd import _lib

    probs = _problems()
    ref_hist, ref_state = _batch_fit()
    ev = _evaluator(probs)
    try:
        state = _start(probs)
        rc, h1, s1 = _call(ev, probs, state, 4)
        assert rc == _lib.LFM_OK and not s1.any()
        rc, h2, s2 = _call(ev, probs, state, 6, step0=4)
        assert rc == _lib.LFM_OK and not s2.any()
    finally:
        ev.close()
    np.testing.assert_array_equal(np.concatenate([h1, h2]), ref_hist)
    for got, want in zip(state, ref_state):
        np.testing.assert_array_equal(got, want)


def test_bits_do_not_depend_on_the_batch():
    from dis_project_amd import _lib

    probs = _problems()
    ref_hist, ref_state = _batch_fit()
    ref = [_per_problem(a, probs) for a in ref_state]
    # a second identical call
    rc, hist, st, state = _fit(probs)
    assert rc == _lib.LFM_OK
    np.testing.assert_array_equal(hist, ref_hist)
    for got, want in zip(state, ref_state):
        np.testing.assert_array_equal(got, want)
    # each problem alone in its own handle
    for p, prob in enumerate(probs):
        rc, hist, st, state = _fit([prob])
        assert rc == _lib.LFM_OK and not st.any()
        np.testing.assert_array_equal(hist[:, 0], ref_hist[:, p])
        for got, want in zip(state, ref):
            _same_problem_bits(_per_problem(got, [prob])[0], want[p])
    # the batch in reversed order
    rc, hist, st, state = _fit(probs[::-1])
    assert rc == _lib.LFM_OK and not st.any()
    np.testing.assert_array_equal(hist[:, ::-1], ref_hist)
    for got, want in zip(state, ref):
        for a, b in zip(_per_problem(got, probs[::-1])[::-1], want):
            _same_problem_bits(a, b)


# ------------------------------------------------------------------ 4. 3 G + 2 > 256
def test_more_parameters_than_threads():
    """G = 128, T = 2: n = 256 and 386 trainable parameters, two passes of the update's 256
    threads. 3 steps against the host loop on the GPU evaluator."""
    import dis_project_amd as lfm
    from dis_project_amd import trainer as TR

    m, d = _edge(128, 2)
    out = {}
    for on_device in (True, False):
        bt = TR.MidBatchTrainer([m], lfm.CustomConjMLL(negative=True), [d], TR.adam(0.01),
                                num_iters=3, on_device=on_device)
        try:
            out[on_device] = bt.fit(fix_params=True, num_steps_per_epoch=2)
        finally:
            bt.close()
    (fitted, hist), (host, host_hist) = out[True], out[False]
    assert np.all(np.isfinite(hist)) and hist.shape == (1, 3)
    # every pass moved its parameters
    assert np.all(fitted[0].true_b != m.true_b) and np.all(fitted[0].true_d != m.true_d)
    _check_fit(fitted, hist, list(zip(host, host_hist)), "G = 128 vs the host loop")


# ------------------------------------------------------------------ 5. not positive definite
def test_not_pd_at_step_0():
    from dis_project_amd import _lib

    probs = _problems()
    ref_hist, ref_state = _batch_fit()
    ref = [_per_problem(a, probs) for a in ref_state]
    bad = BATCH.index((3, 64))
    probs[bad] = (probs[bad][0].replace(jitter=-50.0), probs[bad][1])
    rc, hist, st, state = _fit(probs)
    assert rc == _lib.LFM_E_NOT_PD
    want = np.zeros(len(probs), np.int32)
    want[bad] = 1
    np.testing.assert_array_equal(st, want)
    assert np.all(np.isnan(hist[:, bad]))
    got = [_per_problem(a, probs) for a in state]
    for k in ("true_d", "true_s", "true_b", "l", "obs_stddev"):
        assert np.all(np.isnan(np.atleast_1d(got[0][bad][k]))), k
    assert state[0][-3 * len(probs) + 3 * bad + 2] == -50.0  # the jitter slot passes through
    for p in range(len(probs)):
        if p != bad:
            np.testing.assert_array_equal(hist[:, p], ref_hist[:, p])
            for g, w in zip(got, ref):
                _same_problem_bits(g[p], w[p])


def test_not_pd_at_a_later_step():
    """K(0, 0) = 0 on these grids, so pivot 0 is exactly sigma^2 + jitter: 0.81 - 0.805 = 0.005 at
    step 0; Adam's first update lowers sigma by lr sigmoid(raw), and step 1's pivot is -0.0056.
    +MLL (negative=False), fix_params off (after_epoch would pin index 3 of the G = 4 problem to
    a number again); a good problem shares the call."""
    from dis_project_amd import _lib
    from tests.test_trainer import OracleObjective

    bads = [_edge(3, 43), _edge(3, 64), _edge(4, 7)]
    bads = [(m.replace(jitter=-0.805, obs_stddev=0.9), d) for m, d in bads]
    good = _edge(2, 64)
    probs = bads + [good]
    rc, hist, st, state = _fit(probs, nsteps=4, negative=False, fix=False)
    assert rc == _lib.LFM_E_NOT_PD
    np.testing.assert_array_equal(st, [2, 2, 2, 0])
    got = _per_problem(state[0], probs)
    for p, (m, d) in enumerate(bads):
        want = OracleObjective(False).value_and_grad(m, d)[0]
        err = abs(hist[0, p] - want) / abs(want)
        print(f"n = {d.X.shape[0]}: step-0 loss {hist[0, p]:.6f}, oracle {want:.6f}, "
              f"rel err {err:.3e}")
        assert np.isfinite(hist[0, p]) and err <= 1e-9
        assert np.all(np.isnan(hist[1:, p]))
        for k in ("true_d", "true_s", "true_b", "l", "obs_stddev"):
            assert np.all(np.isnan(np.atleast_1d(got[p][k]))), k
    rc, alone, st1, state1 = _fit([good], nsteps=4, negative=False, fix=False)
    assert rc == _lib.LFM_OK and not st1.any()
    np.testing.assert_array_equal(hist[:, 3], alone[:, 0])
    _same_problem_bits(got[3], _per_problem(state1[0], [good])[0])


# ------------------------------------------------------------------ 6. interleaving
def test_a_fit_leaves_the_handle_usable():
    """After an on-device fit, value_and_grad and the predictor's marginals on the trainer's
    handle are the bits of a fresh evaluator at the same models."""
    import dis_project_amd as lfm
    from dis_project_amd import farm
    from dis_project_amd import trainer as TR
    from dis_project_amd.dataset import (Dataset, SyntheticP53Data, dataset_3d,
                                         generate_test_times)

    datas = [SyntheticP53Data(replicate=0, num_timepoints=30),
             SyntheticP53Data(replicate=0, num_timepoints=64)]
    sets = []
    for d in datas:
        x, y, _ = dataset_3d(d)
        sets.append(Dataset(np.asarray(x, np.float64).reshape(-1, 3),
                            np.asarray(y, np.float64).reshape(-1)))
    models = [lfm.ExactLFM(jitter=1e-4, num_genes=5, device=0) for _ in datas]
    bt = TR.MidBatchTrainer(models, lfm.CustomConjMLL(negative=True), sets, TR.adam(0.01),
                            num_iters=3, on_device=True)
    fresh = farm.MidBatchEvaluator(bt.evaluator.ctx, sets, True)
    t = generate_test_times(20)
    try:
        fitted, hist = bt.fit(fix_params=False)
        assert np.all(np.isfinite(hist)) and not bt.status.any()
        v, g = bt.evaluator.value_and_grad(fitted)
        used = lfm.MidBatchPredictor(datas, evaluator=bt.evaluator).marginals(fitted, t)
        v0, g0 = fresh.value_and_grad(fitted)
        new = lfm.MidBatchPredictor(datas, evaluator=fresh).marginals(fitted, t)
        # and a second fit on the used handle repeats the first
        bt2 = TR.MidBatchTrainer(models, lfm.CustomConjMLL(negative=True), sets, TR.adam(0.01),
                                 num_iters=3, evaluator=bt.evaluator, on_device=True)
        _, hist2 = bt2.fit(fix_params=False)
    finally:
        fresh.close()
        bt.close()
    np.testing.assert_array_equal(v, v0)
    for a, b in zip(g, g0):
        _same_problem_bits(a, b)
    for (ma, va), (mb, vb) in zip(used, new):
        np.testing.assert_array_equal(ma, mb)
        np.testing.assert_array_equal(va, vb)
    np.testing.assert_array_equal(hist2, hist)


# ------------------------------------------------------------------ 7. arguments
def test_bad_arguments_are_refused_with_a_message():
    from dis_project_amd import _lib
    from dis_project_amd import trainer as TR

    probs = [_edge(4, 7)]
    ev = _evaluator(probs)
    ctx = ev.ctx
    try:
        ev.registered([4])
        raw, mu, nu = _start(probs)
        before = raw.copy()
        hist, st = np.empty((2, 1)), np.zeros(1, np.int32)
        opt = _lib.LfmAdam(0.01, 0.9, 0.999, 1e-8, 0.0, 4, 1)
        bad_opt = _lib.LfmAdam(0.01, 0.9, 0.999, 1e-8, 0.0, 0, 1)
        o, bo = _lib.ctypes.byref(opt), _lib.ctypes.byref(bad_opt)
        d = _lib.dptr
        fit = ctx.lib.lfm_mbatch_fit_f64
        cases = {
            "raw": lambda: fit(ctx.handle, ev.batch, o, 1, 0, 2, None, d(mu), d(nu), d(hist), d(st)),
            "history": lambda: fit(ctx.handle, ev.batch, o, 1, 0, 2, d(raw), d(mu), d(nu), None,
                                   d(st)),
            "opt": lambda: fit(ctx.handle, ev.batch, None, 1, 0, 2, d(raw), d(mu), d(nu), d(hist),
                               d(st)),
            "nsteps": lambda: fit(ctx.handle, ev.batch, o, 1, 0, -1, d(raw), d(mu), d(nu), d(hist),
                                  d(st)),
            "num_steps_per_epoch": lambda: fit(ctx.handle, ev.batch, bo, 1, 0, 2, d(raw), d(mu),
                                               d(nu), d(hist), d(st)),
            "batch": lambda: fit(ctx.handle, None, o, 1, 0, 2, d(raw), d(mu), d(nu), d(hist),
                                 d(st)),
        }
        for what, call in cases.items():
            assert call() == _lib.LFM_E_ARG, what
            msg = ctx.lib.lfm_last_error(ctx.handle)
            assert msg and what.encode() in msg, (what, msg)
        np.testing.assert_array_equal(raw, before)
        # nsteps == 0: LFM_OK, nothing touched (as lfm_batch_fit_f64), with or without a history
        assert fit(ctx.handle, ev.batch, o, 1, 0, 0, d(raw), d(mu), d(nu), None,
                   d(st)) == _lib.LFM_OK
        np.testing.assert_array_equal(raw, before)
        assert not mu.any() and not nu.any()
        # fit_packed checks its arrays before the call
        with pytest.raises(ValueError, match="packed"):
            ev.fit_packed(raw[:-1].copy(), mu, nu, TR.adam(0.01), True, 4, 0, 2)
    finally:
        ev.close()


def test_ctx_of_another_device_is_refused():
    from dis_project_amd import _lib

    if _lib.device_count() < 2:
        pytest.skip("needs a second visible device")
    probs = [_edge(4, 7)]
    ev = _evaluator(probs)
    other = _lib.Context(1)
    try:
        ev.registered([4])
        raw, mu, nu = _start(probs)
        hist, st = np.empty((2, 1)), np.zeros(1, np.int32)
        opt = _lib.LfmAdam(0.01, 0.9, 0.999, 1e-8, 0.0, 4, 1)
        assert other.lib.lfm_mbatch_fit_f64(other.handle, ev.batch, _lib.ctypes.byref(opt), 1, 0,
                                            2, _lib.dptr(raw), _lib.dptr(mu), _lib.dptr(nu),
                                            _lib.dptr(hist), _lib.dptr(st)) == _lib.LFM_E_ARG
        assert other.lib.lfm_last_error(other.handle)
    finally:
        other.close()
        ev.close()

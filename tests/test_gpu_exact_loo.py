"""The leave-one-out CV objective (lfm_loocv_f64, lfm_loocv_grad_f64, CustomConjLOOCV) against
extended-precision truth.

The reference is tests/golden/exact_loo.npz (make_golden_exact_loo.py: oracle/lfm_exact.py's long
double Sigma, inverse and derivative blocks). The bounds are the project's own: the value within
loo_rtol (make_golden_exact.rtol_of: 1e-9 wherever fp64 LAPACK on correctly rounded inputs is that
good, which is everywhere here), every gradient component within

    |g - g_exact| <= grad_rtol * scale + 1e-10 * |g_exact|      (grad_rtol 1e-8 here),

the per-point mean within mean_rtol of |y_i| + |a_i| / k_i and the per-point variance within
var_rtol, relatively. Both signs of CustomConjLOOCV(negative) are checked in every case.

  * N = 1024 (4 x 256): the table reductions over W_loo, schedule 3's bordered inverse, 9 x 9
    product tiles (Mp = 1152); all 32 restarts, the ill-conditioned ones again on schedule 1 and
    through grad_pairs_kernel.
  * N = 129 (3 x 43): a ragged last tile, the pair reduction, two product tile rows.
  * n = 48 with latent rows: Sigma is not PD at restarts 1 and 5 (LFM_E_NOT_PD, NaN everywhere);
    restarts 10 and 29 carry values.
  * the C1 problem (n = 35, one tile) as it is and with one observation moved by 30 obs_stddev:
    the cancellation in k_i = -Bt_ii - a_i^2.

Everything comes from the .npz; mpmath is not needed here.
"""

import numpy as np
import pytest

from oracle import lfm_exact as E
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

ILL = (1, 5, 10, 29)


@pytest.fixture(scope="module")
def fx():
    g = load_golden("exact_loo")
    assert tuple(int(r) for r in g["ill"]) == ILL
    return g


@pytest.fixture(scope="module")
def restarts():
    from dis_project_amd import configs

    return configs.c3_restarts(configs.c2(), 32)


@pytest.fixture(scope="module")
def sub(restarts):
    from dis_project_amd import configs

    work = configs.grid_workload("exact", 4, 256, seed_params=2, seed_y=3)
    x = np.ascontiguousarray(work.data.X)
    y = np.ascontiguousarray(work.data.y.reshape(-1))
    return x, y, [E.submodel(m, 4)[0] for m in restarts]


def bits(v):
    return np.asarray(v, np.float64).view(np.uint64)


def loo_call(ctx, x, y, model, negative, want_mean=True, want_var=True):
    """lfm_loocv_f64: (rc, value, loo_mean or None, loo_var or None); NaN-prefilled outputs."""
    from dis_project_amd import _lib

    n = x.shape[0]
    val = np.full(1, 7.0)
    mean = np.full(n, 7.0) if want_mean else None
    var = np.full(n, 7.0) if want_var else None
    rc = ctx.lib.lfm_loocv_f64(ctx.handle, _lib.dptr(x), _lib.dptr(y), n, model.hyp().ref,
                               int(negative), _lib.dptr(val),
                               _lib.dptr(mean) if want_mean else None,
                               _lib.dptr(var) if want_var else None)
    return rc, float(val[0]), mean, var


def loo_grad_call(ctx, x, y, model, negative):
    """lfm_loocv_grad_f64: (rc, value, packed [d, s, b, l, obs_stddev])."""
    from dis_project_amd import _lib

    val, gv = np.full(1, 7.0), np.full(3 * model.num_genes + 2, 7.0)
    rc = ctx.lib.lfm_loocv_grad_f64(ctx.handle, _lib.dptr(x), _lib.dptr(y), x.shape[0],
                                    model.hyp().ref, int(negative), _lib.dptr(val), _lib.dptr(gv))
    return rc, float(val[0]), gv


def figures(fx, pre, q, y, val, mean, var, gv, negative):
    """|error| / bound of the value, the per-point mean, the per-point variance and the gradient
    of problem q of group `pre`: each at most 1 for a right answer."""
    sign = -1.0 if negative else 1.0
    exact, m, v = float(fx[pre + "_loo"][q]), fx[pre + "_mean"][q], fx[pre + "_var"][q]
    mscale = np.abs(y) + np.abs(y - m)  # |y_i| + |a_i| / k_i
    ref = sign * fx[pre + "_grad"][q]
    bound = float(fx[pre + "_grad_rtol"][q]) * fx[pre + "_scale"][q] + 1e-10 * np.abs(ref)
    assert np.all(bound > 0) and np.all(mscale > 0) and np.all(v > 0)
    with np.errstate(invalid="ignore"):
        out = (abs(val - sign * exact) / (float(fx[pre + "_loo_rtol"][q]) * abs(exact)),
               np.max(np.abs(mean - m) / (float(fx[pre + "_mean_rtol"][q]) * mscale)),
               np.max(np.abs(var - v) / (float(fx[pre + "_var_rtol"][q]) * v)),
               np.max(np.abs(gv - ref) / bound))
    return tuple(float(np.nan_to_num(f, nan=np.inf)) for f in out)


def case_figures(ctx, fx, pre, q, x, y, model):
    """Both calls, both signs, of one case: the worst of `figures` per quantity. The gradient
    call's value has the value call's bits."""
    worst = np.zeros(4)
    for negative in (0, 1):
        rc, val, mean, var = loo_call(ctx, x, y, model, negative)
        rc2, val2, gv = loo_grad_call(ctx, x, y, model, negative)
        assert rc == 0 and rc2 == 0, (pre, q, rc, rc2)
        assert bits(val) == bits(val2), (pre, q, val, val2)
        assert np.all(np.isfinite(gv)) and np.all(np.isfinite(mean)) and np.all(np.isfinite(var))
        worst = np.maximum(worst, figures(fx, pre, q, y, val, mean, var, gv, negative))
    return worst


def report(tag, w):
    print(f"{tag}: |error| / bound  value {w[0]:.3e}  mean {w[1]:.3e}  var {w[2]:.3e}  "
          f"grad {w[3]:.3e}")


@pytest.mark.parametrize("env,which", [({}, "all"), ({"LFM_SCHED": "1"}, "ill"),
                                       ({"LFM_GRAD_DIRECT": "1"}, "ill")],
                         ids=["default", "sched1", "direct"])
def test_loo_n1024_restarts_vs_truth(fx, sub, monkeypatch, env, which):
    """The 4 x 256 sub-model: all 32 restarts on the default path (the table reductions over
    W_loo, schedule 3's bordered inverse, 9 x 9 product tiles), the ill-conditioned ones again on
    schedule 1 and through grad_pairs_kernel. No schedule fallback."""
    from dis_project_amd import _lib

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    x, y, models = sub
    keep = np.setdiff1d(np.arange(32), fx["sub_dropped"])
    assert keep.size >= 30 and {0, 1, 5, 10, 29} <= set(keep.tolist())
    todo = [int(r) for r in keep if which == "all" or int(r) in ILL]
    ctx = _lib.Context(0)  # knobs are read when a context is created
    worst, bad = np.zeros(4), []
    try:
        for r in todo:
            w = case_figures(ctx, fx, "sub", r, x, y, models[r])
            report(f"sub r{r} {env}", w)
            worst = np.maximum(worst, w)
            if not np.all(w <= 1.0):
                bad.append((r, w.tolist()))
        assert ctx.fallbacks == 0
    finally:
        ctx.close()
    report(f"N = 1024 {env}: worst over {len(todo)} restarts", worst)
    assert not bad, bad


def una_cases(fx, restarts):
    from dis_project_amd.dataset import grid_inputs

    x = np.ascontiguousarray(grid_inputs(3, 43))
    ys = load_golden("exact_grad")["una_y"]
    return [(q, x, np.ascontiguousarray(ys[q]), E.submodel(restarts[r], 3)[0])
            for q, r in enumerate(ILL)]


def mix_cases(restarts):
    g = load_golden("mixed_mll_n48")
    x, y = np.ascontiguousarray(g["x"]), np.ascontiguousarray(g["y"].reshape(-1))
    return [(q, x, y, E.submodel(restarts[r], 4)[0]) for q, r in enumerate(ILL)]


def test_loo_unaligned_vs_truth(fx, restarts):
    """3 x 43 (N = 129: a ragged last tile in every kernel, the pair reduction, two product tile
    rows) at restarts ILL."""
    from dis_project_amd import _lib

    ctx = _lib.get_context(0)
    before = ctx.fallbacks
    for q, x, y, model in una_cases(fx, restarts):
        w = case_figures(ctx, fx, "una", q, x, y, model)
        report(f"una r{ILL[q]}", w)
        assert np.all(w <= 1.0), (ILL[q], w.tolist())
    assert ctx.fallbacks == before


def test_loo_mixed_flags_vs_truth(fx, restarts):
    """The latent / gene rows of mixed_mll_n48 at the two PD restarts of ILL, 10 and 29."""
    from dis_project_amd import _lib

    ctx = _lib.get_context(0)
    assert np.isfinite(fx["mix_loo"]).tolist() == [False, False, True, True]
    for q, x, y, model in mix_cases(restarts)[2:]:
        w = case_figures(ctx, fx, "mix", q, x, y, model)
        report(f"mix r{ILL[q]}", w)
        assert np.all(w <= 1.0), (ILL[q], w.tolist())


def test_loo_mixed_flags_not_pd_restarts(fx, restarts):
    """At restarts 1 and 5 the mixed layout's Sigma is not PD in exact arithmetic (exact_grad's
    mix_min_eig: -0.15, -0.69): LFM_E_NOT_PD and NaN in every output, the per-point arrays
    included, from both calls and from CustomConjLOOCV."""
    import dis_project_amd as lfm
    from dis_project_amd import _lib

    ctx = _lib.get_context(0)
    assert np.all(load_golden("exact_grad")["mix_min_eig"][:2] < -0.1)
    for q, x, y, model in mix_cases(restarts)[:2]:
        for negative in (0, 1):
            rc, val, mean, var = loo_call(ctx, x, y, model, negative)
            assert rc == _lib.LFM_E_NOT_PD and np.isnan(val), ILL[q]
            assert np.all(np.isnan(mean)) and np.all(np.isnan(var)), ILL[q]
            rc, val, gv = loo_grad_call(ctx, x, y, model, negative)
            assert rc == _lib.LFM_E_NOT_PD and np.isnan(val) and np.all(np.isnan(gv)), ILL[q]
        obj = lfm.CustomConjLOOCV(negative=True)
        data = lfm.Dataset(x, y.reshape(-1, 1))
        assert np.isnan(obj(model, data))
        val, grads = obj.value_and_grad(model, data)
        assert np.isnan(val) and all(np.all(np.isnan(v)) for v in grads.values())
        val, mean, var = obj.pointwise(model, data)
        assert np.isnan(val) and np.all(np.isnan(mean)) and np.all(np.isnan(var))


def c1_cases(fx):
    from dis_project_amd import configs

    w = configs.c1_p53()
    x = np.ascontiguousarray(w.data.X)
    assert np.array_equal(fx["c1_y"][0], w.data.y.reshape(-1))
    return w, [(q, x, np.ascontiguousarray(fx["c1_y"][q]), w.model) for q in (0, 1)]


def test_loo_c1_and_outlier_vs_truth(fx):
    """The C1 problem (n = 35, one tile) at its base model, and once more with one observation
    moved by 30 obs_stddev: max z^2 = a_i^2 / k_i is then 787, the cancellation in
    k_i = -Bt_ii - a_i^2."""
    from dis_project_amd import _lib

    ctx = _lib.get_context(0)
    _, cases = c1_cases(fx)
    assert float(fx["c1_max_z2"][1]) > 100 * float(fx["c1_max_z2"][0])
    for q, x, y, model in cases:
        w = case_figures(ctx, fx, "c1", q, x, y, model)
        report(f"c1 outlier={bool(q)}", w)
        assert np.all(w <= 1.0), (q, w.tolist())


def test_loo_bits_signs_and_optional_outputs(fx, sub, restarts):
    """The same call twice gives the same value and per-point bits; loo_mean / loo_var NULL in
    any combination does not change the value's bits (nor the other array's); `negative` flips
    the value and the gradient exactly and leaves the per-point arrays alone. On N = 1024
    (schedule 3) and N = 129."""
    from dis_project_amd import _lib

    ctx = _lib.get_context(0)
    x, y, models = sub
    _, xu, yu, mu = una_cases(fx, restarts)[0]
    for xx, yy, model, scale in ((x, y, models[0], fx["sub_scale"][0]),
                                 (xu, yu, mu, fx["una_scale"][0])):
        rc, val, mean, var = loo_call(ctx, xx, yy, model, 0)
        assert rc == 0
        for _ in range(2):
            rc, v2, m2, s2 = loo_call(ctx, xx, yy, model, 0)
            assert rc == 0 and bits(v2) == bits(val)
            assert np.array_equal(bits(m2), bits(mean)) and np.array_equal(bits(s2), bits(var))
        for wm, wv in ((False, False), (True, False), (False, True)):
            rc, v2, m2, s2 = loo_call(ctx, xx, yy, model, 0, wm, wv)
            assert rc == 0 and bits(v2) == bits(val), (wm, wv)
            assert m2 is None or np.array_equal(bits(m2), bits(mean))
            assert s2 is None or np.array_equal(bits(s2), bits(var))
        rc, vn, mn, sn = loo_call(ctx, xx, yy, model, 1)
        assert rc == 0 and bits(vn) == bits(-val)
        assert np.array_equal(bits(mn), bits(mean)) and np.array_equal(bits(sn), bits(var))
        # the value flips exactly, and so do the gradient's components that are summed in a
        # fixed order (the mean terms and the trace). The kernel-derivative components are joined
        # with atomics in whatever order the workgroups arrive (at most a few thousand partial
        # sums, each bounded by the component's scale): two calls differ by rounding of that
        # order only, far below 1e-12 of the scale
        rc, gval, gv = loo_grad_call(ctx, xx, yy, model, 0)
        rc2, gvaln, gvn = loo_grad_call(ctx, xx, yy, model, 1)
        assert rc == 0 and rc2 == 0
        assert bits(gval) == bits(val) and bits(gvaln) == bits(-val)
        G = model.num_genes
        # the mean terms (true_b) and the trace (obs_stddev) are summed in a fixed order
        fixed = list(range(2 * G, 3 * G)) + [3 * G + 1]
        assert np.array_equal(bits(gvn[fixed]), bits(-gv[fixed]))
        assert np.all(np.abs(gvn + gv) <= 1e-12 * scale), (gvn + gv) / scale


def test_null_pointers_and_bad_n_carry_a_message():
    """A NULL required pointer or a bad n gives LFM_E_ARG with a message, and no caller buffer is
    touched (the NULL-ctx half needs no context: tests/test_loo_host.py)."""
    from dis_project_amd import _lib

    ctx = _lib.get_context(0)
    lib, h, d = ctx.lib, ctx.handle, _lib.dptr
    x, y = np.zeros((10, 3)), np.zeros(10)
    val, mean, var, grad = np.full(1, 7.0), np.full(10, 7.0), np.full(10, 7.0), np.full(17, 7.0)
    hyp = _lib.HypArgs(np.ones(5), np.ones(5), np.ones(5), 2.5, 1.0, 1e-4)
    bad = [lambda: lib.lfm_loocv_f64(h, None, d(y), 10, hyp.ref, 0, d(val), d(mean), d(var)),
           lambda: lib.lfm_loocv_f64(h, d(x), None, 10, hyp.ref, 0, d(val), d(mean), d(var)),
           lambda: lib.lfm_loocv_f64(h, d(x), d(y), 10, hyp.ref, 0, None, d(mean), d(var)),
           lambda: lib.lfm_loocv_f64(h, d(x), d(y), 10, None, 0, d(val), d(mean), d(var)),
           lambda: lib.lfm_loocv_f64(h, d(x), d(y), 0, hyp.ref, 0, d(val), d(mean), d(var)),
           lambda: lib.lfm_loocv_f64(h, d(x), d(y), 9, hyp.ref, 0, d(val), d(mean), d(var)),
           lambda: lib.lfm_loocv_grad_f64(h, d(x), d(y), 10, hyp.ref, 0, d(val), None),
           lambda: lib.lfm_loocv_grad_f64(h, d(x), d(y), 10, hyp.ref, 0, None, d(grad)),
           lambda: lib.lfm_loocv_grad_f64(h, d(x), d(y), 7, hyp.ref, 0, d(val), d(grad))]
    for call in bad:
        assert call() == _lib.LFM_E_ARG
        assert lib.lfm_last_error(h)
    for buf in (val, mean, var, grad):
        assert np.all(buf == 7.0)


def mll_grad_value(ctx, x, y, model):
    from dis_project_amd import _lib

    val, gv = np.empty(1), np.empty(3 * model.num_genes + 2)
    ctx.check(ctx.lib.lfm_mll_grad_f64(ctx.handle, _lib.dptr(x), _lib.dptr(y), x.shape[0],
                                       model.hyp().ref, 0, _lib.dptr(val), _lib.dptr(gv)))
    return float(val[0])


def test_loo_leaves_nothing_behind_in_the_shared_matrix(fx, sub, restarts):
    """lfm_mll_grad_f64 immediately before and after the leave-one-out calls on one context
    returns the bits it returns as a fresh context's second call: Bs and W_loo, written into the
    bordered matrix's free blocks, are nothing the next factorisation reads. (The value only: the
    gradient's components are summed with atomics.)"""
    from dis_project_amd import _lib

    x, y, models = sub
    _, xu, yu, mu = una_cases(fx, restarts)[0]
    for xx, yy, model in ((x, y, models[0]), (xu, yu, mu)):
        fresh = _lib.Context(0)
        try:
            mll_grad_value(fresh, xx, yy, model)
            ref = mll_grad_value(fresh, xx, yy, model)
        finally:
            fresh.close()
        ctx = _lib.Context(0)
        try:
            mll_grad_value(ctx, xx, yy, model)
            before = mll_grad_value(ctx, xx, yy, model)
            assert loo_grad_call(ctx, xx, yy, model, 0)[0] == 0
            after = mll_grad_value(ctx, xx, yy, model)
            assert loo_call(ctx, xx, yy, model, 1)[0] == 0
            after2 = mll_grad_value(ctx, xx, yy, model)
            assert ctx.fallbacks == 0
        finally:
            ctx.close()
        assert bits(before) == bits(ref) and bits(after) == bits(ref) and bits(after2) == bits(ref)


def test_trainer_fits_on_loocv(fx):
    """JaxTrainer trains on CustomConjLOOCV unchanged: five Adam steps on the negative LOO value
    of the C1 problem against the same loop driven from the host by the fixture's long double
    value and gradient (fit_losses), within the value rule on the fp64-driven loop's own
    deviation (fit_rtol)."""
    import dis_project_amd as lfm
    from dis_project_amd.trainer import JaxTrainer, adam

    w, _ = c1_cases(fx)
    tr = JaxTrainer(w.model, lfm.CustomConjLOOCV(negative=True), w.data, adam(0.01), num_iters=5)
    model, hist = tr.fit(fix_params=False)
    ref, rtol = fx["fit_losses"], float(fx["fit_rtol"])
    assert hist.shape == ref.shape == (5,) and np.all(np.diff(ref) < 0)
    ratio = np.abs(hist - ref) / (rtol * np.abs(ref))
    print(f"fit on -LOO: losses {hist.tolist()}, worst |error| / bound = {ratio.max():.3e} "
          f"(fp64-driven host loop: {float(fx['fit_dev']):.1e} relative)")
    assert np.all(ratio <= 1.0), ratio.tolist()
    assert float(fx["fit_losses"][0]) == -float(fx["c1_loo"][0])

"""CPU checks of the leave-one-out truth fixture (tests/golden/exact_loo.npz,
make_golden_exact_loo.py) against an independent numpy restatement of gpjax 0.8.2's
ConjugateLOOCV.step: Sigma and its explicit inverse, loocv_means = mx + (y - mx) - K_inv_y /
K_inv_diag, loocv_stds = sqrt(1 / K_inv_diag), and Normal(loc, scale).log_prob written out term by
term, all in fp64 numpy. K is the correctly rounded gram (lfm_exact.kernel_exact_pairs, mpmath):
the fp64 oracle's gram cancels at C3's restarts (its LOO value at restart 10 on the 3 x 43 grid is
off by 1.9e-6, relative), and what is checked here is the formula, not that cancellation."""

import math

import numpy as np
import pytest

from oracle import lfm_exact as E
from oracle import lfm_oracle as O
from tests.conftest import load_golden

ILL = (1, 5, 10, 29)


@pytest.fixture(scope="module")
def fx():
    return load_golden("exact_loo")


def hyp_of(model):
    return (np.asarray(model.true_d, np.float64), np.asarray(model.true_s, np.float64),
            np.asarray(model.true_b, np.float64), float(model.l), float(model.obs_stddev),
            float(model.jitter))


def gram_rounded(x, D, S, l):
    """K(x, x), every entry correctly rounded to fp64 (the lower triangle, mirrored)."""
    n = x.shape[0]
    ii, jj = np.tril_indices(n)
    K = np.empty((n, n))
    K[ii, jj] = E.kernel_exact_pairs(x, ii, jj, D, S, l)
    K[jj, ii] = K[ii, jj]
    return K


def gpjax_loocv(x, y, D, S, B, l, sd, jit, gram=gram_rounded):
    """(value, loocv_means, loocv_stds^2) as ConjugateLOOCV.step computes them (constant = 1)."""
    n, G = x.shape[0], len(D)
    Kxx = gram(x, D, S, l) + jit * np.eye(n)
    Sigma = Kxx + sd * sd * np.eye(n)
    mx = O.mean_function(x, D, B, G).reshape(-1)
    Sinv = np.linalg.inv(Sigma)
    K_inv_diag = np.diag(Sinv)
    K_inv_y = Sinv @ (y - mx)
    means = mx + (y - mx) - K_inv_y / K_inv_diag
    stds = np.sqrt(1.0 / K_inv_diag)
    # tfd.Normal(loc, scale).log_prob(y)
    z = (y - means) / stds
    scores = -0.5 * z * z - np.log(stds) - 0.5 * math.log(2.0 * math.pi)
    return float(np.sum(scores)), means, stds * stds


def c1_problem(fx, q):
    from dis_project_amd import configs

    w = configs.c1_p53()
    return np.ascontiguousarray(w.data.X), np.ascontiguousarray(fx["c1_y"][q]), w.model


def small_cases(fx):
    """(group, index, x, y, model) of the small cases: C1 and the PD restarts of una and mix."""
    from dis_project_amd import configs
    from dis_project_amd.dataset import grid_inputs

    restarts = configs.c3_restarts(configs.c2(), 32)
    out = [("c1", q) + c1_problem(fx, q) for q in (0, 1)]
    xu = np.ascontiguousarray(grid_inputs(3, 43))
    yu = load_golden("exact_grad")["una_y"]
    g = load_golden("mixed_mll_n48")
    xm, ym = np.ascontiguousarray(g["x"]), np.ascontiguousarray(g["y"].reshape(-1))
    for q in (2, 3):
        out.append(("una", q, xu, np.ascontiguousarray(yu[q]), E.submodel(restarts[ILL[q]], 3)[0]))
        out.append(("mix", q, xm, ym, E.submodel(restarts[ILL[q]], 4)[0]))
    return out


def test_fixture_against_gpjax_formula_restated(fx):
    """Value, per-point means and variances of the fixture against the restatement. The
    restatement inverts an fp64 Sigma of condition number up to ~1e5 with numpy's inv: it loses
    ~1e-11, and is held to 1e-8, far above that and far below any error of the formula."""
    for pre, q, x, y, model in small_cases(fx):
        val, means, var = gpjax_loocv(x, y, *hyp_of(model))
        assert abs(val - fx[pre + "_loo"][q]) <= 1e-8 * abs(val), (pre, q, val)
        scale = np.abs(y) + np.abs(y - fx[pre + "_mean"][q])
        assert np.all(np.abs(means - fx[pre + "_mean"][q]) <= 1e-8 * scale), (pre, q)
        np.testing.assert_allclose(var, fx[pre + "_var"][q], rtol=1e-8, err_msg=f"{pre} {q}")
    # the outlier moved one observation by 30 obs_stddev and nothing else
    d = fx["c1_y"][1] - fx["c1_y"][0]
    k = int(fx["outlier"])
    sd = c1_problem(fx, 0)[2].obs_stddev
    assert d[k] == pytest.approx(30.0 * sd) and np.count_nonzero(d) == 1
    assert np.array_equal(fx["c1_var"][0], fx["c1_var"][1])  # the variances do not depend on y


@pytest.mark.parametrize("q", [0, 1], ids=["base", "outlier"])
def test_fixture_gradient_against_central_differences_at_c1(fx, q):
    """Every one of the 3G + 2 components of the fixture's gradient at the C1 problem against
    central differences of the restatement (on the fp64 oracle's gram, which is accurate to 1e-13
    at the C1 base model and smooth in the parameters), step 1e-5: truncation ~1e-10 of the third
    derivative, round-off ~1e-16 |value| / 1e-5 ~ 5e-9 (outlier), so 1e-6 of the component's
    scale separates a wrong formula (errors of order the scale) from a right one by a wide margin
    either way."""
    x, y, model = c1_problem(fx, q)
    D, S, B, l, sd, jit = hyp_of(model)
    G = len(D)
    theta = np.concatenate([D, S, B, [l, sd]])

    def value(t):
        return gpjax_loocv(x, y, t[:G], t[G:2 * G], t[2 * G:3 * G], float(t[3 * G]),
                           float(t[3 * G + 1]), jit, gram=O.gram)[0]

    h = 1e-5
    fd = np.empty(theta.size)
    for i in range(theta.size):
        up, dn = theta.copy(), theta.copy()
        up[i] += h
        dn[i] -= h
        fd[i] = (value(up) - value(dn)) / (2 * h)
    g, scale = fx["c1_grad"][q], fx["c1_scale"][q]
    assert g.shape == (3 * G + 2,) and np.all(scale > 0)
    ratio = np.abs(fd - g) / scale
    print(f"c1 case {q}: worst |central difference - fixture| / scale = {ratio.max():.2e}")
    assert np.all(ratio <= 1e-6), ratio.tolist()
    assert np.max(np.abs(g) / scale) > 1e-3  # the comparison is not one of zeros


def test_fixture_bookkeeping(fx):
    """No drops beyond the cap, the pinned restarts kept, every tolerance finite and the
    project's own, the truth's uncertainty recorded and small, the not-PD cases NaN."""
    assert tuple(int(r) for r in fx["ill"]) == ILL
    drop = fx["sub_dropped"]
    assert drop.size <= 2 and not set(drop.tolist()) & {0, 1, 5, 10, 29}
    keep = np.setdiff1d(np.arange(32), drop)
    assert keep.size >= 30
    assert fx["sub_loo"].shape == (32,) and fx["sub_mean"].shape == (32, 1024)
    assert fx["una_mean"].shape == (4, 129) and fx["mix_mean"].shape == (4, 48)
    assert fx["c1_mean"].shape == (2, 35) and fx["sub_grad"].shape == (32, 14)
    pd = {"sub": keep, "una": np.arange(4), "mix": np.array([2, 3]), "c1": np.arange(2)}
    for pre, idx in pd.items():
        for key, floor in (("loo_rtol", 1e-9), ("mean_rtol", 1e-9), ("var_rtol", 1e-9),
                           ("grad_rtol", 1e-8)):
            r = fx[f"{pre}_{key}"][idx]
            assert np.all(np.isfinite(r)) and np.all(r >= floor) and np.all(r <= 1e-5), (pre, key)
        # each tolerance is the rule on the restatement's own error
        for key, err, floor in (("loo_rtol", "loo_fp64_err", 1e-9),
                                ("mean_rtol", "mean_fp64_err", 1e-9),
                                ("var_rtol", "var_fp64_err", 1e-9),
                                ("grad_rtol", "grad_fp64_err", 1e-8)):
            e = fx[f"{pre}_{err}"][idx]
            assert np.all(e <= 1e-5), (pre, err)
            rule = np.minimum(1e-5, np.maximum(floor, 8 * e))
            assert np.array_equal(fx[f"{pre}_{key}"][idx], rule), (pre, key)
        assert np.all(fx[f"{pre}_truth_err"][idx] <= 1e-3), pre
        assert np.all(np.isfinite(fx[f"{pre}_grad"][idx])) and np.all(fx[f"{pre}_var"][idx] > 0)
    assert np.all(np.isnan(fx["mix_loo"][:2])) and np.all(np.isnan(fx["mix_mean"][:2]))
    assert np.all(np.isnan(fx["mix_grad"][:2])) and np.all(np.isnan(fx["mix_grad_rtol"][:2]))
    # the outlier is the cancellation case: z^2 in the hundreds, against ~1 without it
    assert fx["c1_max_z2"][1] > 100 * fx["c1_max_z2"][0]
    # the fit: five decreasing losses, the first the base value, a finite bound
    assert fx["fit_losses"].shape == (5,) and np.all(np.diff(fx["fit_losses"]) < 0)
    assert float(fx["fit_losses"][0]) == -float(fx["c1_loo"][0])
    assert 1e-9 <= float(fx["fit_rtol"]) <= 1e-5 and float(fx["fit_dev"]) <= 1e-5

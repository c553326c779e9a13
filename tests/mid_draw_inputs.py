"""Inputs of the mid-size batch's predictive call (lfm_mbatch_predictive_f64), shared by
tests/test_gpu_mid_draw.py and tests/test_mid_draw_host.py. The training draws are
tests/mid_predict_inputs.problem's (l = 1.8, obs_stddev = 0.7, diag_vec = v); the test rows are
replaced by gene rows (flag 1): a joint covariance over latent rows (flag 0) is indefinite under
the reference's flag-switched kernel, and that is the not-PD case below. Nothing here needs a
GPU."""

import functools

import numpy as np

from tests import mid_predict_inputs as I

L = I.L
OBS = 0.7  # S's diagonal is obs_stddev ** 2 = 0.49 (kind "gene")
COV_ADDS = (1e-4, 0.49)

# (G, T, m): the m's 63 / 64 / 65 and 128 / 129 / 130 / 320 put the residual row at the last row
# of a block, the first row of a new block, and several columns deep
EDGE = ((4, 7, 20), (1, 63, 63), (1, 64, 64), (1, 64, 65), (2, 64, 128), (3, 43, 129),
        (5, 64, 130), (5, 64, 320))
CAP = (4, 256, 1024)
LATENT = (5, 64, 130)  # with flag 0 and cov_add = 1e-4: smallest eigenvalue -0.38, not PD


@functools.lru_cache(maxsize=None)
def problem(G, T, m, flag=1.0):
    """mid_predict_inputs.problem(G, T, m) with the test rows replaced: times U(0, 13), genes
    integers(-1, G + 1), every flag `flag`."""
    p = dict(I.problem(G, T, m))
    rng = np.random.default_rng([G, T, m, 7])
    t = np.stack((rng.uniform(0, 13, m), rng.integers(-1, G + 1, m).astype(float),
                  np.full(m, float(flag))), -1)
    t.setflags(write=False)
    p["t"] = t
    return p


def edge_problems():
    return [problem(*s) for s in EDGE]


def ystar(mean, key):
    """mean + 0.5 N(0, 1) from a fixed rng."""
    rng = np.random.default_rng([len(mean), key, 11])
    return mean + 0.5 * rng.standard_normal(len(mean))


def chol_log_prob(y, mean, scale):
    """log N(y; mean, scale) through numpy's Cholesky factor."""
    Lc = np.linalg.cholesky(scale)
    z = np.linalg.solve(Lc, y - mean)
    return float(-0.5 * (len(y) * np.log(2.0 * np.pi) + 2.0 * np.sum(np.log(np.diagonal(Lc)))
                         + z @ z))


def bound_factor(scale):
    """50 kappa m eps of the GPU checks (the form tests/test_gpu_sample.py uses)."""
    w = np.linalg.eigvalsh(scale)
    return 50.0 * (w[-1] / w[0]) * scale.shape[0] * np.finfo(np.float64).eps

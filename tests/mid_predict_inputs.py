"""Inputs of the mid-size batched posterior's tests, shared by tests/test_gpu_mid_predict.py (the
GPU parity checks) and tests/test_mid_predict_host.py (the oracle's own error at the same
inputs). The draws are those of tests/test_gpu_predict.py::test_posterior_schur_sizes: scattered
times and random genes, v ~ U(0.01, 0.05), l = 1.8, test rows with out-of-range genes and every
flag. Nothing here needs a GPU."""

import functools

import numpy as np

L = 1.8
RTOL, ATOL = 1e-9, 1e-12  # the predictors' tolerance (tests/test_gpu_predict.py)

# (G, T, m): n = 28, 63, 64, 128, 129, 192, 193, 320; the m's give 1, 3, 1, 2, 3, 2, 2, 3 blocks of
# 64 test rows (G k < 64, 64, 68 and 130 each rounded down to a multiple of G)
EDGE = ((4, 7, 20), (1, 63, 130), (1, 64, 64), (2, 64, 68), (3, 43, 129), (3, 64, 66),
        (1, 193, 68), (5, 64, 130))
CAP = (4, 256, 68)  # n = 1024, nb = 17
# (obs_stddev, with the covariance): diag_add = obs_stddev ** 2 = 0.49 and 1e-4
MODES = ((0.7, True), (1e-2, False))


@functools.lru_cache(maxsize=None)
def problem(G, T, m):
    """One problem's draws: dict of D S B x y v t (t [m, 3])."""
    rng = np.random.default_rng([G, T])
    D, S, B = rng.uniform(0.2, 1.0, G), rng.uniform(0.5, 1.5, G), rng.uniform(0.01, 0.1, G)
    n = G * T
    x = np.stack((rng.uniform(0, 12, n), rng.integers(0, G, n).astype(float), np.ones(n)), -1)
    y = rng.normal(0.4, 0.5, n)
    v = rng.uniform(0.01, 0.05, n)
    assert m % G == 0
    t = np.stack((rng.uniform(0, 13, m), rng.integers(-1, G + 1, m).astype(float),
                  rng.integers(0, 2, m).astype(float)), -1)
    out = dict(G=G, n=n, m=m, D=D, S=S, B=B, x=x, y=y, v=v, t=t)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def parity_inputs():
    """Every (problem, obs_stddev, with diag_vec) at which a GPU test compares against the
    oracle: the edge batch at both diagonals, the cap, and the edge batch's n = 129 problem
    without diag_vec."""
    out = []
    for obs, _ in MODES:
        out += [(problem(*s), obs, True) for s in EDGE]
    out.append((problem(*CAP), MODES[0][0], True))
    out.append((problem(*EDGE[4]), MODES[0][0], False))
    return out


@functools.lru_cache(maxsize=None)
def _oracle(G, T, m, obs, with_v):
    from oracle import lfm_oracle as O

    p = problem(G, T, m)
    v = p["v"] if with_v else np.zeros(p["n"])
    mean, cov = O.multi_gene_predict(p["x"], p["y"], v, p["t"], p["D"], p["S"], p["B"], L,
                                     obs, 0.0)
    mean.setflags(write=False)
    cov.setflags(write=False)
    return mean, cov


def oracle(p, obs, with_v=True):
    """(mean [m], cov [m, m]) of O.multi_gene_predict(..., jitter = 0), computed once."""
    return _oracle(p["G"], p["n"] // p["G"], p["m"], float(obs), bool(with_v))

"""``GaussianDistribution`` — the part of gpjax 0.8.2 ``gpjax.distributions`` on the
hot path (called at src/objectives.py:76-78): ``log_prob(y)`` of a dense SPD scale,

    log N(y; loc, S) = -1/2 ( n log 2pi + logdet S + (y - loc)^T S^{-1} (y - loc) ),

with logdet and solve through a Cholesky factor, computed by ``lfm_log_prob_f64``.
A scale that is not positive definite gives NaN (JAX semantics).

The rest of what the reference calls on the object its predictors return (src/plotter.py:63,
src/utils.py:176-179): ``stddev()``, ``variance()`` and ``covariance()`` on the host, and
``sample(seed, sample_shape)`` through ``lfm_mvn_sample_f64``. The samples come from the
library's own counter-based generator (include/lfm.h), not from JAX's threefry key: they equal
gpjax's in distribution, not bit for bit.
"""

from __future__ import annotations

import numpy as np

from ._lib import as_f64, dptr, get_context
from .model import DenseOperator


def seed_to_u64(seed) -> int:
    """An int seed as it is (mod 2^64), or a pair of uint32 words laid out like a JAX key,
    combined hi << 32 | lo."""
    if np.ndim(seed) == 0:
        return int(seed) & 0xFFFFFFFFFFFFFFFF
    words = np.asarray(seed).reshape(-1)
    if words.shape[0] != 2:
        raise ValueError("seed must be an int or a pair of uint32 words (hi, lo)")
    hi, lo = (int(w) for w in words)
    if not (0 <= hi < 2 ** 32 and 0 <= lo < 2 ** 32):
        raise ValueError("the words of a key must be uint32")
    return hi << 32 | lo


def randn(seed, num_samples: int, n: int, sample0: int = 0, device: int | None = None):
    """``[num_samples, n]`` standard normals of the library's generator (``lfm_randn_f64``):
    element ``[s, j]`` depends on ``(seed, sample0 + s, j)`` alone."""
    out = np.empty((int(num_samples), int(n)))
    ctx = get_context(device)
    ctx.check(ctx.lib.lfm_randn_f64(ctx.handle, seed_to_u64(seed), int(sample0),
                                    int(num_samples), int(n), dptr(out)))
    return out


class GaussianDistribution:
    def __init__(self, loc, scale, device: int | None = None):
        self.loc = as_f64(np.atleast_1d(loc)).reshape(-1)
        s = scale.to_dense() if isinstance(scale, DenseOperator) else scale
        self.scale = as_f64(s)
        n = self.loc.shape[0]
        if self.scale.shape != (n, n):
            raise ValueError(f"scale must be {n} x {n}")
        self.device = device

    def mean(self) -> np.ndarray:
        return self.loc

    def log_prob(self, y) -> float:
        y = as_f64(np.atleast_1d(y)).reshape(-1)
        n = self.loc.shape[0]
        if y.shape[0] != n:
            raise ValueError("y has the wrong length")
        out = np.empty(1)
        ctx = get_context(self.device)
        rc = ctx.lib.lfm_log_prob_f64(ctx.handle, dptr(self.loc), dptr(self.scale), n, n,
                                      dptr(y), dptr(out))
        ctx.check(rc, allow_not_pd=True)
        return float(out[0])

    def covariance(self) -> np.ndarray:
        return self.scale

    def variance(self) -> np.ndarray:
        return np.diagonal(self.scale).copy()

    def stddev(self) -> np.ndarray:
        return np.sqrt(np.diagonal(self.scale))

    def sample(self, seed, sample_shape=(), sample0: int = 0) -> np.ndarray:
        """``loc + L z`` per sample, ``L L^T = scale`` (gpjax 0.8.2 ``sample(seed,
        sample_shape)``): ``sample_shape=(k,)`` returns ``[k, n]``, ``()`` returns ``[n]``.
        ``seed`` is an int or a JAX-style pair of uint32 words; sample ``sample0 + s`` depends on
        the seed and its own index alone, so a draw can be continued with ``sample0``. A scale
        that is not positive definite gives NaN (JAX semantics)."""
        shape = tuple(int(k) for k in np.atleast_1d(np.asarray(sample_shape, dtype=np.int64)))
        if len(shape) > 1:
            raise ValueError("sample_shape must be () or (k,)")
        k = shape[0] if shape else 1
        n = self.loc.shape[0]
        out = np.empty((k, n))
        ctx = get_context(self.device)
        rc = ctx.lib.lfm_mvn_sample_f64(ctx.handle, dptr(self.loc), dptr(self.scale), n, n,
                                        seed_to_u64(seed), int(sample0), k, dptr(out))
        ctx.check(rc, allow_not_pd=True)
        return out if shape else out[0]

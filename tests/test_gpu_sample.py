"""Joint samples on the device (lfm_randn_f64, lfm_mvn_sample_f64, lfm_post_sample_f64,
GaussianDistribution.sample, predict.Posterior.sample).

  1. the generator against its numpy restatement (tests/philox_ref.py), |d| <= 1e-13: |z| <= 8.6,
     ln / sqrt / sin / cos are a few ulp each and the rounding of 2 pi u2 is <= 7e-16, together
     about 1e-14; a wrong constant or word order is off by O(1);
  2. splits of the generator: rows and prefixes of a larger call, bit for bit;
  3. the product against numpy's loc + Z cholesky(scale)^T with Z from lfm_randn_f64, bound
     1e-11 max|X| (kappa n eps is about 2e-13 at n = 300), the full matrix and a NaN upper triangle;
  4. the distribution: second moments within 5 SE, means within 4.5 sqrt(C_ii / S);
  5. bit identities over repeats and splits of a draw;
  6. the resident path against lfm_mvn_sample_f64 fed the same handle's predict, bit for bit, and
     against numpy within 50 kappa(scale) m eps max|X|; a predict before and after is unchanged;
  7. failures leave the ctx and the handle usable.

The end-to-end bound against an extended-precision truth: tests/test_gpu_exact_predictive.py.
"""

import ctypes
import functools

import numpy as np
import pytest

from tests import philox_ref

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52


def ctx0():
    from dis_project_amd import _lib

    return _lib.get_context(0)


def randn(seed, sample0, nsamp, n):
    from dis_project_amd import _lib

    ctx = ctx0()
    out = np.full((nsamp, n), 7.0)
    ctx.check(ctx.lib.lfm_randn_f64(ctx.handle, seed, sample0, nsamp, n, _lib.dptr(out)))
    return out


def mvn(loc, scale, seed, sample0, nsamp, expect=0):
    from dis_project_amd import _lib

    ctx = ctx0()
    loc = np.ascontiguousarray(loc, dtype=np.float64)
    scale = np.ascontiguousarray(scale, dtype=np.float64)
    n = loc.shape[0]
    out = np.full((nsamp, n), 7.0)
    rc = ctx.lib.lfm_mvn_sample_f64(ctx.handle, _lib.dptr(loc), _lib.dptr(scale), n, n, seed,
                                    sample0, nsamp, _lib.dptr(out))
    assert rc == expect, (rc, ctx.lib.lfm_last_error(ctx.handle))
    return out


@functools.lru_cache(maxsize=None)
def scale_of(n):
    """A A^T / n + I from default_rng(3): kappa about 5. Computed once, never modified."""
    a = np.random.default_rng(3).standard_normal((n, n))
    c = a @ a.T / n + np.eye(n)
    c = 0.5 * (c + c.T)
    loc = np.random.default_rng(4).normal(0.0, 2.0, n)
    chol = np.linalg.cholesky(c)
    for arr in (c, loc, chol):
        arr.setflags(write=False)
    return c, loc, chol


# ------------------------------------------------------------------ 1. the generator
@pytest.mark.parametrize("sample0", [0, 7, 2 ** 33 + 1])
def test_generator_vs_reference(sample0):
    for seed in (42, 2 ** 40 + 5):
        for nsamp, n in ((1, 1), (1, 2), (3, 5), (2, 129), (130, 127)):
            got = randn(seed, sample0, nsamp, n)
            ref = philox_ref.randn(seed, sample0, nsamp, n)
            d = float(np.max(np.abs(got - ref)))
            print(f"randn seed {seed} sample0 {sample0} ({nsamp}, {n}): max|d| = {d:.2e}")
            assert d <= 1e-13


# ------------------------------------------------------------------ 2. its splits
def test_generator_splits_bitwise():
    seed = 42
    big = randn(seed, 5, 130, 127)
    for s in (0, 1, 64, 129):
        np.testing.assert_array_equal(big[s], randn(seed, 5 + s, 1, 127)[0])
    for n1 in (1, 2, 5, 126):
        np.testing.assert_array_equal(big[3, :n1], randn(seed, 8, 1, n1)[0])
    assert np.all(np.isfinite(big)) and np.max(np.abs(big)) <= 8.6


# ------------------------------------------------------------------ 3. the product
@pytest.mark.parametrize("n", [1, 5, 127, 128, 129, 300])
def test_product_vs_numpy(n):
    c, loc, chol = scale_of(n)
    nan_upper = c.copy()
    nan_upper[np.triu_indices(n, 1)] = np.nan
    for nsamp in (1, 3, 130):
        z = randn(11, 2, nsamp, n)
        ref = loc + z @ chol.T
        bound = 1e-11 * float(np.max(np.abs(ref)))
        full = mvn(loc, c, 11, 2, nsamp)
        lower = mvn(loc, nan_upper, 11, 2, nsamp)
        d = float(np.max(np.abs(full - ref)))
        print(f"mvn n {n} nsamp {nsamp}: max|d| = {d:.2e}, bound {bound:.2e}")
        assert d <= bound
        np.testing.assert_array_equal(lower, full)  # only the lower triangle is read


# ------------------------------------------------------------------ 4. the distribution
def test_distribution_moments():
    n, S = 130, 2048
    c, _, _ = scale_of(n)
    x = mvn(np.zeros(n), c, 7, 0, S)
    second = x.T @ x / S
    se = np.sqrt((c * c + np.outer(np.diag(c), np.diag(c))) / S)
    zmom = float(np.max(np.abs(second - c) / se))
    zmean = float(np.max(np.abs(x.mean(0)) / np.sqrt(np.diag(c) / S)))
    print(f"second moments: max |d| / SE = {zmom:.2f}; means: {zmean:.2f}")
    assert zmom <= 5.0
    assert zmean <= 4.5


# ------------------------------------------------------------------ 5. bit identities
def test_bit_identities():
    n, nsamp, k = 300, 130, 37
    c, loc, _ = scale_of(n)
    a = mvn(loc, c, 99, 0, nsamp)
    np.testing.assert_array_equal(mvn(loc, c, 99, 0, nsamp), a)
    np.testing.assert_array_equal(mvn(loc, c, 99, 0, k), a[:k])
    np.testing.assert_array_equal(mvn(loc, c, 99, k, nsamp - k), a[k:])
    assert not np.array_equal(mvn(loc, c, 100, 0, k), a[:k])


def test_distribution_object_samples():
    import dis_project_amd as lfm

    c, loc, _ = scale_of(129)
    d = lfm.GaussianDistribution(loc, c, device=0)
    x = d.sample(5, sample_shape=(4,))
    assert x.shape == (4, 129)
    np.testing.assert_array_equal(x, mvn(loc, c, 5, 0, 4))
    one = d.sample(5)
    assert one.shape == (129,)
    np.testing.assert_array_equal(one, x[0])
    np.testing.assert_array_equal(d.sample([0, 5], (2,)), x[:2])  # a JAX-style key: hi, lo
    np.testing.assert_array_equal(lfm.randn(42, 3, 5), randn(42, 0, 3, 5))


# ------------------------------------------------------------------ 6. the resident path
def _close_handle(lib, handle):
    lib.lfm_post_destroy(handle)


@functools.lru_cache(maxsize=None)
def posterior(which, kind):
    """"p53": the synthetic p53 data with 3 replicates (n = 105) through the shim. "mixed":
    n = 300 scattered times and genes (no grid), on a handle made with lfm_post_create and wrapped
    in the same class."""
    import weakref

    import dis_project_amd as lfm
    from dis_project_amd import _lib, dataset as ds

    if which == "p53":
        data = ds.SyntheticP53Data(replicate=None, seed=5)
        model = lfm.ExactLFM(jitter=1e-4, obs_stddev=0.4, num_genes=5, device=0)
        post = model.posterior(data, kind)
        assert post.status == 0 and post.n == 105
        return post
    rng = np.random.default_rng(300)
    G, n = 5, 300
    D, S, B = rng.uniform(0.2, 1.0, G), rng.uniform(0.5, 1.5, G), rng.uniform(0.01, 0.1, G)
    x = np.stack((rng.uniform(0, 12, n), rng.integers(0, G, n).astype(float),
                  np.ones(n)), -1)
    y = rng.normal(0.4, 0.5, n)
    v = rng.uniform(0.01, 0.05, n)
    hyp = _lib.HypArgs(D, S, B, 1.8, 0.7, 1e-4)
    ctx = ctx0()
    h = ctypes.c_void_p()
    ctx.check(ctx.lib.lfm_post_create(ctx.handle, _lib.dptr(x), _lib.dptr(y), n, _lib.dptr(v),
                                      1e-4 if kind == "latent" else 0.49, hyp.ref,
                                      ctypes.byref(h)))
    post = object.__new__(lfm.Posterior)
    post.num_genes, post.kind, post.jitter, post.n = G, kind, 1e-4, n
    post._handle, post.ctx, post._keep, post.status = h, ctx, ctx, 0
    post._final = weakref.finalize(post, _close_handle, ctx.lib, h)
    return post


def rows_of(m, G, seed, flag=1.0):
    """Test rows at scattered times, gene indices -1 .. G (they wrap and clamp). flag 1: gene
    rows, whose joint covariance is positive semi-definite to rounding (its smallest eigenvalue
    was measured at -2e-14 for these designs, against the jitter of 1e-4). flag 0: latent rows,
    whose joint covariance under the reference's flag-switched kernel is indefinite (smallest
    eigenvalue -3 to -4 at m = 100, 130 on the p53 data): test_failures_leave_everything_usable."""
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack((rng.uniform(0, 13, m),
                                          rng.integers(-1, G + 1, m).astype(float),
                                          np.full(m, flag)), -1))



@pytest.mark.parametrize("m", [5, 100, 130])
@pytest.mark.parametrize("kind", ["latent", "gene"])
@pytest.mark.parametrize("which", ["p53", "mixed"])
def test_resident_path_vs_host_route(which, kind, m):
    post = posterior(which, kind)
    t = rows_of(m, 5, m)
    nsamp, seed = 131, 2 ** 35 + 17
    mean0, var0, cov0 = post._predict(t, True)
    mean_s, x = post.sample(t, nsamp, seed)
    mean1, var1, cov1 = post._predict(t, True)
    for a, b in ((mean0, mean1), (var0, var1), (cov0, cov1)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(mean_s, mean0)
    assert x.shape == (nsamp, m) and np.all(np.isfinite(x))
    # the host route: the same one addition on the diagonal, then lfm_mvn_sample_f64
    scale = cov0.copy()
    scale[np.diag_indices(m)] += post.jitter
    np.testing.assert_array_equal(x, mvn(mean0, scale, seed, 0, nsamp))
    # a continued draw
    _, tail = post.sample(t, nsamp - 40, seed, sample0=40)
    np.testing.assert_array_equal(tail, x[40:])
    # numpy
    ref = mean0 + randn(seed, 0, nsamp, m) @ np.linalg.cholesky(scale).T
    kappa = float(np.linalg.cond(scale))
    bound = 50.0 * kappa * m * EPS * float(np.max(np.abs(ref)))
    d = float(np.max(np.abs(x - ref)))
    print(f"{which} {kind} m {m}: kappa {kappa:.3g}, max|d| = {d:.2e}, bound {bound:.2e}")
    assert d <= bound


# ------------------------------------------------------------------ 7. failures
def test_failures_leave_everything_usable():
    import dis_project_amd as lfm
    from dis_project_amd import _lib

    ctx = ctx0()
    lib = ctx.lib
    c, loc, _ = scale_of(129)
    good = mvn(loc, c, 1, 0, 3)

    def message():
        return lib.lfm_last_error(ctx.handle).decode()

    # not positive definite: a negative eigenvalue
    bad = c - 3.0 * np.eye(129)
    assert np.linalg.eigvalsh(bad)[0] < 0
    out = mvn(loc, bad, 1, 0, 3, expect=_lib.LFM_E_NOT_PD)
    assert np.all(np.isnan(out))
    assert np.all(np.isnan(lfm.GaussianDistribution(loc, bad, device=0).sample(1, (3,))))
    np.testing.assert_array_equal(mvn(loc, c, 1, 0, 3), good)
    # arguments
    out = np.full((3, 129), 7.0)
    d = _lib.dptr
    for s0, ns, word in ((0, 0, "nsamp"), (-1, 3, "sample0"), (2 ** 63 - 2, 3, "overflow")):
        assert lib.lfm_mvn_sample_f64(ctx.handle, d(loc), d(c), 129, 129, 1, s0, ns,
                                      d(out)) == _lib.LFM_E_ARG
        assert word in message()
        assert lib.lfm_randn_f64(ctx.handle, 1, s0, ns, 129, d(out)) == _lib.LFM_E_ARG
    assert lib.lfm_mvn_sample_f64(ctx.handle, None, d(c), 129, 129, 1, 0, 3,
                                  d(out)) == _lib.LFM_E_ARG
    assert "NULL" in message()
    assert np.all(out == 7.0)
    np.testing.assert_array_equal(mvn(loc, c, 1, 0, 3), good)

    # the handle: m over the chunk names the limit; nsamp = 0; then it still samples
    post = posterior("mixed", "gene")
    t = rows_of(130, 5, 130)
    _, before = post.sample(t, 4, 9)
    post.set_chunk(128)
    with pytest.raises(lfm.LfmError, match="128") as e:
        post.sample(t, 4, 9)
    assert e.value.code == _lib.LFM_E_ARG
    post.set_chunk(0)
    mean, out = np.empty(130), np.empty((4, 130))
    assert lib.lfm_post_sample_f64(ctx.handle, post._handle, d(t), 130, 1e-4, 9, 0, 0, d(mean),
                                   d(out)) == _lib.LFM_E_ARG
    assert "nsamp" in message()
    assert lib.lfm_post_sample_f64(ctx.handle, post._handle, d(t), 130, 1e-4, 9, 0, 4, d(mean),
                                   None) == _lib.LFM_E_ARG
    # not positive definite through the handle: every output NaN, the handle unharmed
    assert lib.lfm_post_sample_f64(ctx.handle, post._handle, d(t), 130, -50.0, 9, 0, 4, d(mean),
                                   d(out)) == _lib.LFM_E_NOT_PD
    assert np.all(np.isnan(out)) and np.all(np.isnan(mean))
    _, after = post.sample(t, 4, 9)
    np.testing.assert_array_equal(after, before)

    # latent rows: the reference's kernel gives an indefinite joint covariance, so the draw is
    # JAX's NaN Cholesky on both routes; the marginals and the handle are unharmed
    lat = posterior("p53", "latent")
    t0 = rows_of(100, 5, 100, flag=0.0)
    mean0, var0, cov0 = lat._predict(t0, True)
    scale = cov0 + 1e-4 * np.eye(100)
    assert np.linalg.eigvalsh(scale)[0] < -1.0
    mean_s, x = lat.sample(t0, 3, 9)
    assert np.all(np.isnan(x)) and np.all(np.isnan(mean_s))
    assert np.all(np.isnan(mvn(mean0, scale, 9, 0, 3, expect=_lib.LFM_E_NOT_PD)))
    for a, b in zip(lat._predict(t0, True), (mean0, var0, cov0)):
        np.testing.assert_array_equal(a, b)
    assert np.all(np.isfinite(lat.sample(rows_of(100, 5, 100), 3, 9)[1]))

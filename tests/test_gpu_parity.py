"""GPU parity: every value comes from liblfm.so on the MI355X (through the C-ABI / the
Python shim) and is compared with the oracle / golden fixtures on the same inputs.

Tolerances (stated per test):
  * MLL: 1e-5 relative is the north_star bar; the fp64 paths are held to 1e-9.
  * gram / cross-covariance fp64: |dK| <= 16 eps M + 1e-14 max|K| element-wise, where M is
    the magnitude of the reference formula's intermediate terms (oracle.gram_error_scale):
    the reference's own fp64 evaluation is only accurate to ~eps * M where its erf sums
    cancel under a large e^{gamma^2 - D delta} factor (numerics).
  * gram fp32: |dK| <= 16 eps64 M + 4e-6 max|K| (fp32 arithmetic on cancellation-free tables).
"""

import math

import numpy as np
import pytest

from oracle import lfm_exact as E
from oracle import lfm_oracle as O
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu

MLL_RTOL = 1e-9          # fp64 end-to-end; north_star requires <= 1e-5
NORTH_STAR_RTOL = 1e-5


@pytest.fixture(scope="module")
def lfm():
    import dis_project_amd as m
    from dis_project_amd import _lib

    assert _lib.device_count() >= 1, "no HIP device visible"
    return m


def model_from(g, lfm, **kw):
    return lfm.ExactLFM(jitter=float(g["jitter"]), obs_stddev=float(g["obs_stddev"]),
                        num_genes=g["D"].shape[0], true_d=g["D"], true_s=g["S"], true_b=g["B"],
                        l=float(g["l"]), **kw)


# ----------------------------------------------------------- matrix cores
def test_mfma_f64_layout(lfm):
    """v_mfma_f64_16x16x4_f64 lane maps, A = arbitrary, B asymmetric (guide §3)."""
    from dis_project_amd._lib import dptr, get_context

    rng = np.random.default_rng(0)
    a = rng.integers(-4, 5, (16, 4)).astype(np.float64)
    b = rng.integers(-4, 5, (4, 16)).astype(np.float64) + np.arange(16) * 0.5
    d = np.empty((16, 16))
    ctx = get_context()
    ctx.check(ctx.diag.lfm_probe_mfma_f64_layout(ctx.handle, dptr(a), dptr(b), dptr(d)))
    np.testing.assert_array_equal(d, a @ b)


def test_mfma4_layout(lfm):
    """v_mfma_f64_4x4x4_4b_f64 lane maps the trailing update relies on (lfm_chol.hip
    gemm_accumulate): block g = (lane >> 2) & 3 holds A_g[i][k] at lane 16k + 4g + i,
    B_g[k][j] at lane 16k + 4g + j, C/D_g[i][j] at lane 16i + 4g + j. (The CBSZ / ABID
    A-broadcast fields do not broadcast on the f64 form: one-hot probes of every mode give
    this same map, scripts/probe_mfma4_layout.py — so A is replicated in registers.)"""
    from dis_project_amd._lib import dptr, get_context

    rng = np.random.default_rng(4)
    a, b, c = (rng.integers(-4, 5, 64).astype(np.float64) for _ in range(3))
    d = np.empty(5 * 64)
    ctx = get_context()
    ctx.check(ctx.diag.lfm_probe_mfma4_layout(ctx.handle, dptr(a), dptr(b), dptr(c), dptr(d)))
    d = d.reshape(5, 64)
    for g in range(4):
        A = np.array([[a[16 * k + 4 * g + i] for k in range(4)] for i in range(4)])
        B = np.array([[b[16 * k + 4 * g + j] for j in range(4)] for k in range(4)])
        C = np.array([[c[16 * i + 4 * g + j] for j in range(4)] for i in range(4)])
        got = np.array([[d[0, 16 * i + 4 * g + j] for j in range(4)] for i in range(4)])
        np.testing.assert_array_equal(got, A @ B + C, err_msg=f"block {g}")


# --------------------------------------------------------------- kernel
def test_h_vs_oracle_and_mpmath(lfm):
    rng = np.random.default_rng(1)
    D = rng.uniform(0.2, 1.0, 5)
    m = lfm.ExactLFM(num_genes=5, true_d=D, l=2.3)
    j = rng.integers(0, 5, 400)
    k = rng.integers(0, 5, 400)
    t1 = rng.uniform(0, 12, 400)
    t2 = rng.uniform(0, 12, 400)
    got = m.h(j, k, t1, t2)
    # the reference is the 50-digit value at every point: O.h keeps the reference's operation
    # order and is itself 1.8e-12 (absolute) off it here, 181 x this tolerance, which the device
    # reproduced digit for digit while it kept that order (tests/test_gpu_exact_posterior.py)
    hm = np.array([O.h_mpmath(D, 2.3, j[q], k[q], t1[q], t2[q]) for q in range(400)])
    np.testing.assert_allclose(got, hm, rtol=1e-13, atol=1e-14)
    ref = O.h(D, 2.3, j, k, t1, t2)
    assert np.max(np.abs(ref - hm)) <= 16 * EPS * np.max(np.exp((D * 2.3 / 2) ** 2 + 12 * D))


def test_h_t0_vanishes_exactly(lfm):
    """KAT: erf is odd on the device too, so h(., ., 0, t2) and h(., ., t1, 0) are 0."""
    rng = np.random.default_rng(2)
    D = rng.uniform(0.1, 2.0, 4)
    m = lfm.ExactLFM(num_genes=4, true_d=D)
    t = rng.uniform(0, 12, 200)
    j = rng.integers(0, 4, 200)
    k = rng.integers(0, 4, 200)
    assert np.all(m.h(j, k, np.zeros(200), t) == 0.0)


EPS = np.finfo(np.float64).eps


def assert_gram_close(K, Kref, x, y, D, S, l, extra_rel=1e-14):
    M = O.gram_error_scale(x, y, D, S, l)
    tol = 16 * EPS * M + extra_rel * max(1.0, np.abs(Kref).max())
    bad = np.abs(K - Kref) > tol
    assert not bad.any(), (int(bad.sum()), float(np.abs(K - Kref).max()),
                           float((np.abs(K - Kref) / tol).max()))


def test_cross_covariance_mixed_flags(lfm, golden):
    """Against the 80-digit value of every pair (lfm_exact.kernel_exact), under the tolerance the
    golden was held to. The golden's own K comes from the oracle, whose gene / latent entries
    carry the reference order's cancellation: up to 1.1e-11 here, 479 x this tolerance (for
    such pairs gram_error_scale is |K| + 1, which does not grow with that cancellation)."""
    g = golden("mixed_flags_cross")
    m = lfm.ExactLFM(num_genes=3, true_d=g["D"], true_s=g["S"], l=float(g["l"]))
    K = m.cross_covariance(m.kernel, g["xa"], g["xb"])
    truth = np.array([[E.kernel_exact(a, b, g["D"], g["S"], float(g["l"])) for b in g["xb"]]
                      for a in g["xa"]])
    assert np.max(np.abs(g["K"] - truth)) <= 2e-11  # the fixture is the oracle's, not the truth
    assert_gram_close(K, truth, g["xa"], g["xb"], g["D"], g["S"], float(g["l"]))


def test_kernel_scalar_surface(lfm):
    D = np.array([0.3, 0.9])
    S = np.array([1.1, 0.7])
    m = lfm.ExactLFM(num_genes=2, true_d=D, true_s=S, l=1.9)
    a, b = np.array([3.0, 1.0, 1.0]), np.array([7.5, 0.0, 0.0])
    assert abs(m.kernel(a, b) - O.kernel_scalar(a, b, D, S, 1.9)) < 1e-13
    assert abs(m.kernel_xx(a, b) - O.kernel_scalar(a, [7.5, 0.0, 1.0], D, S, 1.9)) < 1e-13
    assert abs(m.kernel_ff(a, b) - math.exp(-(4.5**2) / (2 * 1.9))) < 1e-15
    assert abs(m.kernel_xf(a, b) - O.kernel_scalar(a, b, D, S, 1.9)) < 1e-13
    assert m.gamma(1) == 0.9 * 1.9 / 2


@pytest.mark.parametrize("name", ["c1_p53_n35", "p53_3rep_n105", "grid_n64", "grid_n512",
                                  "scattered_n200", "kat_zero_times_n32"])
def test_gram_vs_golden(lfm, name):
    g = load_golden(name)
    m = model_from(g, lfm)
    K = m.gram(m.kernel, g["x"]).to_dense()
    assert_gram_close(K, g["K"], g["x"], g["x"], g["D"], g["S"], float(g["l"]))


def test_mean_function_vs_golden(lfm):
    for name in ["c1_p53_n35", "p53_3rep_n105", "grid_n512"]:
        g = load_golden(name)
        m = model_from(g, lfm)
        np.testing.assert_array_equal(m.mean_function(g["x"]).reshape(-1), g["m"])


# ------------------------------------------------------------------ MLL
@pytest.mark.parametrize("name", ["c1_p53_n35", "p53_3rep_n105", "grid_n64", "grid_n512",
                                  "scattered_n200", "kat_zero_times_n32"])
@pytest.mark.parametrize("negative", [False, True])
def test_mll_vs_golden(lfm, name, negative):
    g = load_golden(name)
    m = model_from(g, lfm)
    v = lfm.CustomConjMLL(negative=negative)(m, lfm.Dataset(g["x"], g["y"]))
    ref = float(g["neg_mll"] if negative else g["mll"])
    assert abs(v - ref) <= MLL_RTOL * abs(ref), (v, ref)
    assert abs(v - ref) <= NORTH_STAR_RTOL * abs(ref)


def test_mll_batch_c5(lfm):
    """3 replicates x leave-one-gene-out, one fused launch (one workgroup per problem)."""
    models, data, refs = [], [], []
    for r in range(3):
        g = load_golden(f"c5_rep{r}_loo")
        for drop in range(5):
            keep = [q for q in range(5) if q != drop]
            x = np.stack((np.tile(np.linspace(0, 12, 7), 4), np.repeat(np.arange(4), 7),
                          np.ones(28)), -1)
            models.append(lfm.ExactLFM(jitter=1e-4, num_genes=4))
            data.append(lfm.Dataset(x, g["expr"][keep].reshape(-1)))
            refs.append(g["neg_mll"][drop])
    got = lfm.CustomConjMLL(negative=True).batch(models, data)
    np.testing.assert_allclose(got, np.array(refs), rtol=MLL_RTOL)


def test_mll_batch_mixed_sizes(lfm):
    names = ["c1_p53_n35", "grid_n512", "grid_n64", "scattered_n200"]
    gs = [load_golden(n) for n in names]
    got = lfm.CustomConjMLL().batch([model_from(g, lfm) for g in gs],
                                    [lfm.Dataset(g["x"], g["y"]) for g in gs])
    np.testing.assert_allclose(got, [float(g["mll"]) for g in gs], rtol=MLL_RTOL)


@pytest.mark.parametrize("n_genes,T", [(2, 64), (3, 43), (2, 129), (1, 257)])
def test_mll_block_edges(lfm, n_genes, T):
    """n around the 128-row panel edges: n = 128, 129, 258, 257 (augmented row placement)."""
    rng = np.random.default_rng(n_genes * 1000 + T)
    D = rng.uniform(0.2, 1.0, n_genes)
    S = rng.uniform(0.5, 1.5, n_genes)
    B = rng.uniform(0.01, 0.1, n_genes)
    x = np.stack((np.tile(np.linspace(0, 12, T), n_genes), np.repeat(np.arange(n_genes), T),
                  np.ones(n_genes * T)), -1)
    y = rng.normal(0.3, 0.5, n_genes * T)
    ref = O.mll(x, y, D, S, B, 2.5, 1.0, 1e-4)
    m = lfm.ExactLFM(jitter=1e-4, num_genes=n_genes, true_d=D, true_s=S, true_b=B)
    v = lfm.CustomConjMLL()(m, lfm.Dataset(x, y))
    assert abs(v - ref) <= MLL_RTOL * abs(ref), (v, ref)


def test_mll_not_pd_is_nan(lfm):
    """JAX returns NaN on a failed Cholesky; so does the device path (small and blocked)."""
    for T in (8, 300):
        x = np.stack((np.linspace(0, 12, T), np.zeros(T), np.ones(T)), -1)
        m = lfm.ExactLFM(jitter=-5.0, obs_stddev=0.0, num_genes=1)
        v = lfm.CustomConjMLL(negative=True)(m, lfm.Dataset(x, np.zeros(T)))
        assert math.isnan(v)
        assert math.isnan(O.mll(x, np.zeros(T), [0.4], [1.0], [0.05], 2.5, 0.0, -5.0))


def test_log_prob_dense(lfm):
    g = load_golden("grid_n512")
    Sig = O.sigma(g["x"], g["D"], g["S"], float(g["l"]), float(g["obs_stddev"]),
                  float(g["jitter"]))
    dist = lfm.GaussianDistribution(g["m"], Sig)
    v = dist.log_prob(g["y"])
    assert abs(v - float(g["mll"])) <= MLL_RTOL * abs(float(g["mll"]))


def test_gram_f32(lfm):
    g = load_golden("grid_n512")
    m = model_from(g, lfm)
    K32 = m.gram_f32(g["x"])
    assert K32.dtype == np.float32
    assert_gram_close(K32.astype(np.float64), g["K"], g["x"], g["x"], g["D"], g["S"],
                      float(g["l"]), extra_rel=4e-6)


def test_structured_and_direct_paths_agree(lfm):
    """The grid (table) path and the direct erf path give the same gram: shuffling the
    rows defeats layout detection, so the permuted gram comes from the direct kernel."""
    g = load_golden("grid_n512")
    m = model_from(g, lfm)
    K_grid = m.gram(m.kernel, g["x"]).to_dense()
    perm = np.random.default_rng(0).permutation(g["x"].shape[0])
    K_dir = m.gram(m.kernel, g["x"][perm]).to_dense()
    assert_gram_close(K_grid[np.ix_(perm, perm)], K_dir, g["x"][perm], g["x"][perm], g["D"],
                      g["S"], float(g["l"]))
    # C3 restart 29 (sub-model of oracle.lfm_exact.submodel, 4 x 128 grid): e^{gamma^2 + 12 D}
    # reaches ~1e23 and the direct path, which keeps the reference's operation order, is off
    # the truth by up to ~1e-2 on entries of order 10 while the table path is right to
    # ~1e-14 (tests/test_gpu_exact.py). The two paths' expected disagreement is therefore the
    # direct path's error: bounded by 16 eps gram_error_scale and nothing tighter.
    from dis_project_amd import configs
    from dis_project_amd.dataset import grid_inputs
    from oracle import lfm_exact

    m29, _ = lfm_exact.submodel(configs.c3_restarts(configs.c2(), 30)[29], 4)
    x = np.ascontiguousarray(grid_inputs(4, 128))
    K_grid = m29.gram(m29.kernel, x).to_dense()
    K_dir = m29.gram(m29.kernel, x[perm]).to_dense()
    print(f"restart 29: max |grid - direct| = {np.abs(K_grid[np.ix_(perm, perm)] - K_dir).max():.2e}"
          f" on max |K| = {np.abs(K_grid).max():.2f}")
    assert_gram_close(K_grid[np.ix_(perm, perm)], K_dir, x[perm], x[perm], m29.true_d, m29.true_s,
                      m29.l, extra_rel=0.0)


def grid_problem(G, T, seed, l=2.5, sd=1.0, jitter=1e-4):
    rng = np.random.default_rng(seed)
    D = rng.uniform(0.2, 1.0, G)
    S = rng.uniform(0.5, 1.5, G)
    B = rng.uniform(0.01, 0.1, G)
    x = np.stack((np.tile(np.linspace(0, 12, T), G), np.repeat(np.arange(G), T), np.ones(G * T)),
                 -1)
    y = np.repeat(B / D, T) + 0.5 * rng.standard_normal(G * T)
    return x, y, D, S, B, l, sd, jitter


@pytest.mark.parametrize("G", [2, 3])
def test_gram_aligned_T256(lfm, G):
    """T = 256: the LDS-staged aligned grid kernel (configs 2-4 use it)."""
    x, y, D, S, B, l, sd, jit = grid_problem(G, 256, 40 + G, l=1.8)
    m = lfm.ExactLFM(jitter=jit, obs_stddev=sd, num_genes=G, true_d=D, true_s=S, true_b=B, l=l)
    Kref = O.gram(x, D, S, l)
    assert_gram_close(m.gram(m.kernel, x).to_dense(), Kref, x, x, D, S, l)
    assert_gram_close(m.gram_f32(x).astype(np.float64), Kref, x, x, D, S, l, extra_rel=4e-6)


def test_mll_aligned_T256_permuted_genes(lfm):
    """Blocks in a shuffled gene order (an ablation-style layout) on the aligned path."""
    x, y, D, S, B, l, sd, jit = grid_problem(4, 256, 77)
    order = np.array([2, 0, 3, 1])
    x2 = x.copy()
    x2[:, 1] = np.repeat(order, 256)
    ref = O.mll(x2, y, D, S, B, l, sd, jit)
    m = lfm.ExactLFM(jitter=jit, obs_stddev=sd, num_genes=4, true_d=D, true_s=S, true_b=B, l=l)
    v = lfm.CustomConjMLL()(m, lfm.Dataset(x2, y))
    assert abs(v - ref) <= MLL_RTOL * abs(ref), (v, ref)


@pytest.mark.slow
def test_mll_n4096_vs_oracle(lfm):
    """N = 4096 (16 genes x 256 timepoints): 32 block columns through the look-ahead
    pipeline, compared with the scipy oracle. Tolerance: the north_star 1e-5, held to 1e-9."""
    x, y, D, S, B, l, sd, jit = grid_problem(16, 256, 4096)
    ref = O.mll(x, y, D, S, B, l, sd, jit, negative=True)
    m = lfm.ExactLFM(jitter=jit, obs_stddev=sd, num_genes=16, true_d=D, true_s=S, true_b=B, l=l)
    v = lfm.CustomConjMLL(negative=True)(m, lfm.Dataset(x, y))
    assert abs(v - ref) <= MLL_RTOL * abs(ref), (v, ref)


def test_pivot_rsqrt_one_newton_step(lfm):
    """The diagonal factor's pivot reciprocal square root (v_rsq_f64 + one Newton step) stays
    within 1e-14 relative of 1/sqrt over 24 decades (measured max 4.1e-15, typical 1e-15): a
    backward error of that size in the pivot's column (numerics)."""
    from dis_project_amd import _lib

    rng = np.random.default_rng(7)
    x = np.concatenate([10.0 ** rng.uniform(-12, 12, 200000), rng.uniform(0.5, 4.0, 100000),
                        np.array([1.0, 2.0, 1e-300, 1e300])])
    y = np.empty_like(x)
    ctx = _lib.get_context(0)
    ctx.check(ctx.diag.lfm_probe_rsq(ctx.handle, x.ctypes.data, x.size, y.ctypes.data))
    ref = 1.0 / np.sqrt(x)
    rel = np.abs(y - ref) / ref
    assert rel.max() <= 1e-14, rel.max()


@pytest.mark.parametrize("G,n,seed", [(4, 28, 1), (5, 35, 2), (7, 63, 3), (1, 9, 4)])
def test_small_kernel_tables_are_bit_identical(lfm, G, n, seed):
    """small_mll_kernel forms gene-gene pairs from per-row / per-gene tables (KxxTab, round 4):
    every entry bit-identical to the reference restatement kernel_ref on the same device, over
    random times (t = 0 included), gene indices that need the JAX clamp / wrap (-1, G + 2.7) and
    mixed flags (latent rows, a flag of 2: kernel_ref's generic switch)."""
    from dis_project_amd import _lib

    rng = np.random.default_rng(seed)
    x = np.stack([rng.uniform(0, 12, n), rng.integers(0, G, n).astype(np.float64),
                  np.ones(n)], -1)
    x[0, 0] = 0.0
    x[1 % n, 1] = -1.0
    x[2 % n, 1] = G + 2.7
    if n > 8:
        x[3::7, 2] = 0.0
        x[5, 2] = 2.0
    m = lfm.ExactLFM(num_genes=G, true_d=rng.uniform(0.2, 1.0, G), true_s=rng.uniform(0.5, 1.5, G),
                     true_b=rng.uniform(0.01, 0.1, G), l=rng.uniform(1.0, 4.0))
    x = np.ascontiguousarray(x)
    out = np.empty(2 * n * n)
    hp = m.hyp()
    ctx = _lib.get_context(0)
    ctx.check(ctx.diag.lfm_probe_kxx_tab(ctx.handle, _lib.dptr(x), n, hp.ref, _lib.dptr(out)))
    ref, tab = out[: n * n], out[n * n:]
    assert np.array_equal(ref.view(np.uint64), tab.view(np.uint64)), \
        np.flatnonzero(ref.view(np.uint64) != tab.view(np.uint64))[:8]
    # and the restatement against the formula's 60-digit value (rows with flags 0 / 1; the
    # oracle's own gene / latent entries are off by more than this tolerance, see
    # test_cross_covariance_mixed_flags)
    ok = np.isin(x[:, 2], (0.0, 1.0))
    xs = x[ok]
    K = E.PairCache(m.true_d, m.true_s, m.l).matrix(xs).astype(np.float64)
    scale = O.gram_error_scale(xs, xs, m.true_d, m.true_s, m.l)
    got = ref.reshape(n, n)[np.ix_(ok, ok)]
    assert np.all(np.abs(got - K) <= 16 * np.finfo(float).eps * scale + 1e-300)


@pytest.mark.parametrize("env", [{"LFM_SCHED": "3"}, {"LFM_SCHED": "3", "LFM_S3_EVENTS": "1"},
                                 {"LFM_SCHED": "3", "LFM_W4_MIN": "1024"},
                                 {"LFM_SCHED": "3", "LFM_W4_MIN": "1024", "LFM_S3_EVENTS": "1"},
                                 {"LFM_SCHED": "3", "LFM_W4_MIN": "1073741824", "LFM_W2_MIN": "1024"},
                                 {"LFM_SCHED": "1"}, {"LFM_SCHED": "3", "LFM_SIDE_CUS": "8"}])
def test_mll_schedules_agree(lfm, env, monkeypatch):
    """N = 2560 (10 genes x 256): schedule 3 device-ordered (default), schedule 3 event-ordered
    (profiling mode), both with w = 4 super-panels (LFM_W4_MIN=1024), w = 2 super-panels,
    schedule 1 and a smaller chain partition all match the oracle to 1e-9."""
    from dis_project_amd import _lib, configs

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    work = configs.grid_workload("sched", 10, 256, seed_params=5, seed_y=6)
    x = np.ascontiguousarray(work.data.X)
    y = np.ascontiguousarray(work.data.y.reshape(-1))
    m = work.model
    ref = O.mll(x, y, m.true_d, m.true_s, m.true_b, m.l, m.obs_stddev, m.jitter)
    ctx = _lib.Context(0)  # schedule / partition knobs are read when a context is created
    try:
        out = np.empty(1)
        hp = m.hyp()
        for _ in range(2):  # a second call reuses the workspace and the device counters
            ctx.check(ctx.lib.lfm_mll_f64(ctx.handle, _lib.dptr(x), _lib.dptr(y), x.shape[0],
                                          hp.ref, 0, _lib.dptr(out)))
            assert abs(out[0] - ref) <= MLL_RTOL * abs(ref), (env, out[0], ref)
    finally:
        ctx.close()

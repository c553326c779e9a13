"""``BatchPredictor`` — the predict half of the reference's small-problem workflow, batched.

The reference fits every replicate x leave-one-gene-out model (src/notebook.py:33-75) and then
calls ``latent_predict`` and ``multi_gene_predict`` (src/model.py:420-514) on each fitted model
(src/notebook.py:91-110, src/utils.py:144-172). ``trainer.BatchTrainer`` runs the fits of the
whole farm in one launch; this class does the same for the predictors: the training data of
every problem is registered in HBM once (``lfm_batch_create``) and one
``lfm_batch_posterior_f64`` call evaluates every problem at its own test inputs. The assembly of
the returned ``GaussianDistribution`` is ``ExactLFM.latent_predict`` / ``multi_gene_predict``'s.

``MidBatchPredictor`` is the same for problems of up to 1024 rows each
(``lfm_mbatch_posterior_f64`` on ``farm.MidBatchEvaluator``'s handle).

``Posterior`` is the large-N counterpart: one fitted model whose factor stays resident in HBM
(``lfm_post_create``) and is evaluated at many sets of test inputs (``lfm_post_predict_f64``).
"""

from __future__ import annotations

from typing import Sequence

import numpy as np

from . import _lib
from ._lib import as_f64, dptr


# ------------------------------------------------------------------ pure helpers
def pack_test_inputs(test_inputs, genes: Sequence[int]):
    """Test inputs of P problems as lfm_batch_posterior_f64 takes them: (t [sum m_p, 3] packed in
    problem order, m [P] int64). ``test_inputs`` is one [m, 3] array shared by every problem or a
    sequence of P such arrays. Every m_p must be >= 1 and a multiple of that problem's num_genes
    (mean_function's broadcast, model.py:145-149), else ValueError."""
    genes = [int(g) for g in genes]
    if isinstance(test_inputs, np.ndarray) and test_inputs.ndim == 2:
        per = [test_inputs] * len(genes)
    else:
        per = list(test_inputs)
        if len(per) != len(genes):
            raise ValueError("one test-input array per problem (or one shared [m, 3] array)")
    ts = []
    for p, (t, G) in enumerate(zip(per, genes)):
        t = as_f64(t)
        if t.ndim != 2 or t.shape[1] != 3:
            raise ValueError(f"problem {p}: test inputs must be [m, 3]")
        if t.shape[0] < 1 or t.shape[0] % G != 0:
            raise ValueError(f"problem {p}: m = {t.shape[0]} test rows is not a positive multiple "
                             f"of num_genes = {G} (mean_function, model.py:145-149)")
        ts.append(t)
    m = np.asarray([t.shape[0] for t in ts], np.int64)
    return np.ascontiguousarray(np.concatenate(ts, axis=0)), m


def unpack_outputs(m, mean, var=None, cov=None):
    """lfm_batch_posterior_f64's packed outputs as per-problem arrays: a list of (mean [m_p],
    var [m_p] or None, cov [m_p, m_p] or None)."""
    m = np.asarray(m, np.int64)
    if np.any(m < 1):
        raise ValueError("every m must be >= 1")
    mean = np.asarray(mean)
    if mean.shape != (int(m.sum()),) or (var is not None and np.shape(var) != mean.shape) or \
            (cov is not None and np.shape(cov) != (int((m * m).sum()),)):
        raise ValueError("packed outputs do not match m")
    out, o1, o2 = [], 0, 0
    for k in (int(v) for v in m):
        out.append((mean[o1:o1 + k].copy(),
                    None if var is None else np.asarray(var)[o1:o1 + k].copy(),
                    None if cov is None else np.asarray(cov)[o2:o2 + k * k].reshape(k, k).copy()))
        o1 += k
        o2 += k * k
    return out


# ------------------------------------------------------------------ the predictors
class _Assembly:
    """The ``GaussianDistribution``s and marginals of ``ExactLFM.latent_predict`` /
    ``multi_gene_predict`` from a batched posterior: ``_posterior(models, test_inputs, diag_add,
    want_cov)`` returns per problem (mean, var, cov or None). ``_ev`` is the evaluator that
    holds the registered batch (``farm.BatchEvaluator`` / ``farm.MidBatchEvaluator``), ``ENTRY``
    the posterior entry point on its handle and ``MAX_M`` that entry point's bound on a
    problem's test rows, if it has one (``TOO_MANY_ROWS``: the message past it)."""

    ENTRY = None
    MAX_M = TOO_MANY_ROWS = None

    def __len__(self):
        return len(self._ev.datasets)

    def _posterior(self, models, test_inputs, diag_add, want_cov):
        models = list(models)
        if len(models) != len(self):
            raise ValueError("one model per registered problem")
        genes = [int(mm.num_genes) for mm in models]
        t, m = pack_test_inputs(test_inputs, genes)
        if self.MAX_M is not None and np.any(m > self.MAX_M):
            raise ValueError(self.TOO_MANY_ROWS)
        self._ev._pack(models)  # the packed hyperparameters; registers this gene layout
        self.ctx = self.ctx or self._ev.ctx
        dadd = as_f64(diag_add).reshape(-1)
        mean = np.empty(int(m.sum()))
        var = np.empty_like(mean)
        cov = np.empty(int((m * m).sum())) if want_cov else None
        self.status = np.zeros(len(models), np.int32)
        rc = getattr(self.ctx.lib, self.ENTRY)(
            self.ctx.handle, self._ev.batch, dptr(self._ev._buf), dptr(self.variances),
            dptr(dadd), dptr(m), dptr(t), dptr(mean), dptr(var),
            dptr(cov) if want_cov else None, dptr(self.status))
        self.ctx.check(rc, allow_not_pd=True)
        return unpack_outputs(m, mean, var, cov)

    def latent_predict(self, models, test_inputs):
        """model.py:420-465 per problem: S = K(x,x) + diag(variances) + jitter I;
        scale = diag(var + jitter) + jitter I. No covariance is computed."""
        from .distributions import GaussianDistribution

        models = list(models)
        res = self._posterior(models, test_inputs, [mm.jitter for mm in models], False)
        out = []
        for (mean, var, _), mm in zip(res, models):
            scale = np.diag(var + mm.jitter) + np.eye(mean.shape[0]) * mm.jitter
            out.append(GaussianDistribution(mean, scale, device=self.ctx.device))
        return out

    def multi_gene_predict(self, models, test_inputs):
        """model.py:467-514 per problem: S = K(x,x) + diag(variances) + obs_stddev^2 I;
        scale = K(t,t) - K(t,x) S^{-1} K(x,t) + jitter I."""
        from .distributions import GaussianDistribution

        models = list(models)
        res = self._posterior(models, test_inputs, [mm.obs_stddev ** 2 for mm in models], True)
        out = []
        for (mean, _, cov), mm in zip(res, models):
            scale = cov + np.eye(mean.shape[0]) * mm.jitter
            out.append(GaussianDistribution(mean, scale, device=self.ctx.device))
        return out

    def marginals(self, models, test_inputs, kind: str = "latent"):
        """(mean, var) per problem — the diagonal of ``latent_predict``'s (kind "latent") or
        ``multi_gene_predict``'s (kind "gene") scale — without forming any covariance: what the
        plots of utils.py:144-172 read."""
        models = list(models)
        if kind == "latent":
            res = self._posterior(models, test_inputs, [mm.jitter for mm in models], False)
            return [(mean, (var + mm.jitter) + mm.jitter) for (mean, var, _), mm in zip(res, models)]
        if kind == "gene":
            res = self._posterior(models, test_inputs, [mm.obs_stddev ** 2 for mm in models],
                                  False)
            return [(mean, var + mm.jitter) for (mean, var, _), mm in zip(res, models)]
        raise ValueError('kind must be "latent" or "gene"')


def _training_sets(train_datas):
    """``dataset_3d`` of every data object: ([Dataset], the variances packed in problem order)."""
    from .dataset import Dataset, dataset_3d

    datasets, var = [], []
    for d in train_datas:
        x, y, v = dataset_3d(d)
        datasets.append(Dataset(as_f64(x).reshape(-1, 3), as_f64(y).reshape(-1, 1)))
        var.append(as_f64(v).reshape(-1))
    if not datasets:
        raise ValueError("no training data")
    return datasets, np.ascontiguousarray(np.concatenate(var))


class BatchPredictor(_Assembly):
    """``latent_predict`` / ``multi_gene_predict`` of P (model, training data) problems in one
    call each. ``train_datas``: the P53-style data objects ``ExactLFM.latent_predict`` takes
    (``dataset_3d`` is applied to each; n <= 127 per problem). ``models`` (one ExactLFM per
    problem, e.g. ``BatchTrainer.fit``'s) are read at every call. ``status`` holds the last
    call's per-problem codes (LFM_E_NOT_PD: that problem's outputs are NaN, as under JAX)."""

    ENTRY = "lfm_batch_posterior_f64"

    def __init__(self, train_datas, ctx=None):
        from .farm import BatchEvaluator

        self.ctx = ctx or _lib.get_context()
        datasets, self.variances = _training_sets(train_datas)
        self._ev = BatchEvaluator(self.ctx, datasets)
        self.status = np.zeros(len(datasets), np.int32)

    def close(self):
        self._ev.close()


class MidBatchPredictor(_Assembly):
    """``BatchPredictor`` for problems of any size 1 <= n <= 1024 — the predict half of
    ``trainer.MidBatchTrainer``'s workflow: one ``lfm_mbatch_posterior_f64`` call evaluates every
    problem at its own test inputs (at most 4096 rows each), in a number of launches that depends
    on the largest n alone. ``train_datas`` as ``BatchPredictor``'s; the problems are registered
    through ``farm.MidBatchEvaluator``. With ``evaluator=`` (``MidBatchTrainer.evaluator``) that
    handle is used and the data is not uploaded a second time; its x / y must be the data's,
    else ValueError. The context may be asked for as late as the first call. ``sample`` and
    ``log_prob`` draw from, and score held-out values under, every problem's predictive
    distribution on the same handle (``lfm_mbatch_predictive_f64``, at most 1024 test rows each)."""

    ENTRY = "lfm_mbatch_posterior_f64"
    MAX_M = 4096  # LFM_MID_MAX_M
    TOO_MANY_ROWS = (f"at most {MAX_M} test rows per problem (LFM_MID_MAX_M); use Posterior for "
                     "more on one model")

    def __init__(self, train_datas, ctx=None, evaluator=None):
        from .farm import MidBatchEvaluator

        datasets, self.variances = _training_sets(train_datas)
        self._own = evaluator is None
        if evaluator is None:
            evaluator = MidBatchEvaluator(ctx, datasets)
        else:
            if len(evaluator.datasets) != len(datasets):
                raise ValueError("the evaluator holds another number of problems")
            for i, (d, e) in enumerate(zip(datasets, evaluator.datasets)):
                ex = np.asarray(e.X, np.float64)
                ey = np.asarray(e.y, np.float64).reshape(-1)
                if ex.shape != d.X.shape or not np.array_equal(ex, d.X) or \
                        not np.array_equal(ey, np.asarray(d.y).reshape(-1)):
                    raise ValueError(f"problem {i}: the evaluator's x / y differ from the data's")
        self._ev = evaluator
        self.ctx = ctx or evaluator.ctx
        self.status = np.zeros(len(datasets), np.int32)

    MAX_DRAW_M = 1024       # LFM_MID_MAX_N: the covariance goes through the mid factorisation
    MAX_DRAW_SAMPLES = 65536  # per call; sample0 continues a draw

    def _predictive(self, models, test_inputs, kind, cov_add, y_star=None, num_samples=0,
                    seeds=None, sample0=0):
        """One ``lfm_mbatch_predictive_f64``; every argument is checked before the first device
        call. Returns (m, mean, logp or None, samples or None), packed."""
        models = list(models)
        if len(models) != len(self):
            raise ValueError("one model per registered problem")
        if kind == "latent":
            dadd = as_f64([mm.jitter for mm in models]).reshape(-1)
        elif kind == "gene":
            dadd = as_f64([mm.obs_stddev ** 2 for mm in models]).reshape(-1)
        else:
            raise ValueError('kind must be "latent" or "gene"')
        P = len(models)
        genes = [int(mm.num_genes) for mm in models]
        t, m = pack_test_inputs(test_inputs, genes)
        if np.any(m > self.MAX_DRAW_M):
            raise ValueError(f"at most {self.MAX_DRAW_M} test rows per problem (LFM_MID_MAX_N: the "
                             "covariance is factored on the handle); use Posterior.sample for "
                             "more on one model")
        if cov_add is None:
            cadd = as_f64([mm.jitter for mm in models]).reshape(-1)
        else:
            cadd = as_f64(cov_add).reshape(-1)
            if cadd.size == 1:
                cadd = np.full(P, cadd[0])
            if cadd.size != P:
                raise ValueError("cov_add: one value, or one per problem")
        ys = None
        if y_star is not None:
            if isinstance(y_star, np.ndarray) and y_star.ndim == 1 and P == 1:
                y_star = [y_star]
            per = [as_f64(y).reshape(-1) for y in y_star]
            if len(per) != P or any(y.size != k for y, k in zip(per, m)):
                raise ValueError("y_star: one array of m_p values per problem")
            ys = np.ascontiguousarray(np.concatenate(per))
        k = int(num_samples)
        sd = None
        if k > 0:
            if k > self.MAX_DRAW_SAMPLES:
                raise ValueError(f"at most {self.MAX_DRAW_SAMPLES} samples per call; continue "
                                 "the draw with sample0")
            if int(sample0) < 0:
                raise ValueError("sample0 must be >= 0")
            sd = np.ascontiguousarray(np.asarray(seeds, np.uint64).reshape(-1))
            if sd.size != P:
                raise ValueError("seeds: one per problem")
        self._ev._pack(models)  # the packed hyperparameters; registers this gene layout
        self.ctx = self.ctx or self._ev.ctx
        sm = int(m.sum())
        mean = np.empty(sm)
        logp = np.empty(P) if ys is not None else None
        out = np.empty(k * sm) if k > 0 else None
        self.status = np.zeros(P, np.int32)
        rc = self.ctx.lib.lfm_mbatch_predictive_f64(
            self.ctx.handle, self._ev.batch, dptr(self._ev._buf), dptr(self.variances), dptr(dadd),
            dptr(m), dptr(t), dptr(cadd), dptr(ys) if ys is not None else None,
            dptr(logp) if logp is not None else None, dptr(sd) if sd is not None else None,
            int(sample0), k, dptr(mean), dptr(out) if out is not None else None,
            dptr(self.status))
        self.ctx.check(rc, allow_not_pd=True)
        return m, mean, logp, out

    def sample(self, models, test_inputs, num_samples, seed, sample0: int = 0,
               kind: str = "gene", cov_add=None, seeds=None):
        """Joint draws from every fitted model's predictive distribution in one
        ``lfm_mbatch_predictive_f64``: a list of ``(mean [m_p], samples [num_samples, m_p])`` from
        N(mean_p, cov_p + cov_add_p I), the covariance formed, factored and multiplied on the
        handle (at most 1024 test rows per problem). ``kind`` picks S's diagonal as ``Posterior``
        does ("latent": jitter; "gene": obs_stddev**2); ``cov_add`` defaults to each model's
        jitter, which with ``kind="gene"`` is ``multi_gene_predict(...)[p].sample(...)``'s
        distribution. Problem p's seed is ``seeds[p]``, or ``(seed_to_u64(seed) + p) mod 2^64``;
        sample ``sample0 + s`` depends on that seed and its own index alone. A problem that is
        not positive definite gives NaN (``status`` holds the codes)."""
        from .distributions import seed_to_u64

        k = int(num_samples)
        if k < 1:
            raise ValueError("num_samples must be >= 1")
        if seeds is None:
            key = seed_to_u64(seed)
            seeds = [(key + p) % (1 << 64) for p in range(len(self))]
        m, mean, _, out = self._predictive(models, test_inputs, kind, cov_add, None, k, seeds,
                                           sample0)
        res, o = [], 0
        for mp in (int(v) for v in m):
            res.append((mean[o:o + mp].copy(), out[k * o:k * (o + mp)].reshape(k, mp).copy()))
            o += mp
        return res

    def log_prob(self, models, test_inputs, y_star, kind: str = "gene", cov_add=None):
        """``[P]``: log N(y_star_p; mean_p, cov_p + cov_add_p I) of every problem in one
        ``lfm_mbatch_predictive_f64`` — with the defaults ``multi_gene_predict(...)[p].log_prob(
        y_star_p)``, the held-out log density of, say, replicate 2's measurements under a model
        fitted on replicate 1. A caller scoring noisy replicates passes ``cov_add =
        obs_stddev**2 + jitter``. ``y_star``: one array of m_p values per problem. NaN where not
        positive definite (``status`` holds the codes)."""
        if y_star is None:
            raise ValueError("y_star: one array of m_p values per problem")
        _, _, logp, _ = self._predictive(models, test_inputs, kind, cov_add, y_star)
        return logp

    def close(self):
        if self._own:
            self._ev.close()


# ------------------------------------------------------------------ the resident posterior
def _destroy_post(lib, handle):
    lib.lfm_post_destroy(handle)


class Posterior:
    """One large fitted model, conditioned once and evaluated at many sets of test inputs.

    ``latent_predict`` / ``multi_gene_predict`` (src/model.py:420-514) condition on the training
    data at every call; the notebooks then evaluate the fitted model at several sets of test
    times. ``Posterior(model, train_data, kind)`` applies ``dataset_3d`` and that predictor's
    diagonal (``kind="latent"``: ``jitter``; ``kind="gene"``: ``obs_stddev**2``), factors S once
    (``lfm_post_create``: the factor stays in HBM) and every ``predict`` / ``marginals`` is one
    ``lfm_post_predict_f64``: a multi-right-hand-side solve against the resident factor. The
    model's hyperparameters are read at construction. ``status`` holds the fit's code
    (LFM_E_NOT_PD: every output is NaN, as under JAX)."""

    KINDS = ("latent", "gene")

    def __init__(self, model, train_data, kind: str = "latent", ctx=None):
        import ctypes
        import weakref

        from .dataset import dataset_3d

        if kind not in self.KINDS:
            raise ValueError('kind must be "latent" or "gene"')
        x, y, variances = dataset_3d(train_data)
        x = as_f64(x).reshape(-1, 3)
        y = as_f64(y).reshape(-1)
        v = as_f64(variances).reshape(-1)
        self.num_genes = int(model.num_genes)
        if x.shape[0] < 1 or x.shape[0] % self.num_genes != 0:
            raise ValueError(f"n = {x.shape[0]} training rows is not a positive multiple of "
                             f"num_genes = {self.num_genes} (mean_function, model.py:145-149)")
        if y.shape[0] != x.shape[0] or v.shape[0] != x.shape[0]:
            raise ValueError("x, y and the variances must have one row per observation")
        self.kind = kind
        self.jitter = float(model.jitter)
        self.n = x.shape[0]
        diag_add = self.jitter if kind == "latent" else float(model.obs_stddev) ** 2
        self.ctx = ctx or model.ctx
        hp = model.hyp()
        handle = ctypes.c_void_p()
        rc = self.ctx.lib.lfm_post_create(self.ctx.handle, dptr(x), dptr(y), self.n, dptr(v),
                                          float(diag_add), hp.ref, ctypes.byref(handle))
        self.status = self.ctx.check(rc, allow_not_pd=True)
        self._handle = handle if rc == _lib.LFM_OK else None
        # the fallback of close(): the context (kept alive by the finaliser) outlives the handle
        self._final = (weakref.finalize(self, _destroy_post, self.ctx.lib, handle)
                       if self._handle else None)
        self._keep = self.ctx

    def _test(self, test_inputs):
        t = as_f64(test_inputs)
        if t.ndim != 2 or t.shape[1] != 3:
            raise ValueError("test inputs must be [m, 3]")
        if t.shape[0] < 1 or t.shape[0] % self.num_genes != 0:
            raise ValueError(f"m = {t.shape[0]} test rows is not a positive multiple of "
                             f"num_genes = {self.num_genes} (mean_function, model.py:145-149)")
        return t

    def set_chunk(self, rows: int = 0):
        """Test rows solved per pass (a multiple of 128; 0: the default)."""
        if self._handle:
            self.ctx.check(self.ctx.lib.lfm_post_set_chunk(self._handle, int(rows)))

    def _predict(self, t, want_cov):
        m = t.shape[0]
        mean = np.full(m, np.nan)
        var = np.full(m, np.nan)
        cov = np.full((m, m), np.nan) if want_cov else None
        if self._handle:  # a failed fit: NaN, as under JAX
            self.ctx.check(self.ctx.lib.lfm_post_predict_f64(
                self.ctx.handle, self._handle, dptr(t), m, dptr(mean), dptr(var),
                dptr(cov) if want_cov else None))
        return mean, var, cov

    def marginals(self, test_inputs):
        """(mean, var), var the diagonal of ``predict``'s scale, for any m: nothing of size m^2
        is formed (what the plots of utils.py:144-172 read)."""
        mean, var, _ = self._predict(self._test(test_inputs), False)
        if self.kind == "latent":
            return mean, (var + self.jitter) + self.jitter
        return mean, var + self.jitter

    def predict(self, test_inputs):
        """The ``GaussianDistribution`` of ``ExactLFM.latent_predict`` (kind "latent": the scale
        is diagonal, model.py:420-465, so only the variances are computed) or
        ``multi_gene_predict`` (kind "gene": the dense covariance, model.py:467-514)."""
        from .distributions import GaussianDistribution

        t = self._test(test_inputs)
        m = t.shape[0]
        if self.kind == "latent":
            mean, var, _ = self._predict(t, False)
            scale = np.diag(var + self.jitter) + np.eye(m) * self.jitter
        else:
            mean, _, cov = self._predict(t, True)
            scale = cov + np.eye(m) * self.jitter
        return GaussianDistribution(mean, scale, device=self.ctx.device)

    def sample(self, test_inputs, num_samples, seed, sample0: int = 0):
        """``(mean [m], samples [num_samples, m])``: joint draws from N(mean(t), cov(t) +
        jitter I), one ``lfm_post_sample_f64``: the covariance is formed, factored and multiplied
        on the device and only the samples come back. Both kinds use the DENSE covariance. For
        ``kind="gene"`` that is ``predict(t).sample(...)``. For ``kind="latent"`` it is the joint
        posterior, which the reference's ``latent_predict`` discards by diagonalising
        (model.py:420-465); ``predict(t).sample(...)`` still reproduces the reference's diagonal
        distribution exactly. Gene rows (flag 1) can be drawn jointly under either kind. Latent
        rows (flag 0) cannot: the joint covariance the reference's flag-switched kernel gives them
        is indefinite, and the draw is NaN with ``LFM_E_NOT_PD`` swallowed,
        as JAX's Cholesky would return NaN. m must fit one chunk (``set_chunk``). ``seed`` as
        ``GaussianDistribution.sample``; sample ``sample0 + s`` depends on the seed and its own
        index alone. The bits are not JAX's threefry bits. After a failed fit: NaN, as
        ``predict``."""
        from .distributions import seed_to_u64

        t = self._test(test_inputs)
        k = int(num_samples)
        if k < 1:
            raise ValueError("num_samples must be >= 1")
        if int(sample0) < 0:
            raise ValueError("sample0 must be >= 0")
        key = seed_to_u64(seed)
        m = t.shape[0]
        mean = np.full(m, np.nan)
        out = np.full((k, m), np.nan)
        if self._handle:
            rc = self.ctx.lib.lfm_post_sample_f64(
                self.ctx.handle, self._handle, dptr(t), m, self.jitter, key, int(sample0), k,
                dptr(mean), dptr(out))
            self.ctx.check(rc, allow_not_pd=True)
        return mean, out

    def log_prob(self, test_inputs, y_star, cov_add=None):
        """log N(y_star; mean(t), cov(t) + cov_add I), one ``lfm_post_log_prob_f64``: the
        covariance is formed and factored on the device and the held-out vectors are solved
        against its factor there; only the log densities come back. ``y_star`` is ``[m]`` (returns
        a float) or ``[k, m]`` (returns ``[k]``: k vectors scored under the one factorisation).
        ``cov_add`` defaults to the model's jitter, as in ``sample``; a caller scoring noisy
        replicates passes ``obs_stddev**2 + jitter``. Both kinds use the DENSE covariance. For
        ``kind="gene"`` with the default ``cov_add`` that is ``predict(t).log_prob(y_star)``. For
        ``kind="latent"`` it is the joint posterior, which the reference's ``latent_predict``
        discards by diagonalising (model.py:420-465); ``predict(t).log_prob(...)`` still
        reproduces the reference's diagonal distribution exactly. Gene rows (flag 1) can be
        scored jointly under either kind. Latent rows (flag 0) cannot: their joint covariance is
        indefinite, and the result is NaN with ``LFM_E_NOT_PD``
        swallowed, as JAX's Cholesky would return NaN. A row of ``y_star`` with a NaN or Inf is
        NaN alone. m must fit one chunk (``set_chunk``). After a failed fit: NaN, as
        ``predict``."""
        t = self._test(test_inputs)
        m = t.shape[0]
        y = as_f64(y_star)
        if y.ndim not in (1, 2) or y.shape[-1] != m or y.shape[0] < 1:
            raise ValueError(f"y_star must be [m] or [k, m] with m = {m} test rows and k >= 1")
        single = y.ndim == 1
        y = np.ascontiguousarray(y.reshape(-1, m))
        k = y.shape[0]
        cadd = self.jitter if cov_add is None else float(cov_add)
        logp = np.full(k, np.nan)
        if self._handle:
            rc = self.ctx.lib.lfm_post_log_prob_f64(
                self.ctx.handle, self._handle, dptr(t), m, cadd, dptr(y), k, None, dptr(logp))
            self.ctx.check(rc, allow_not_pd=True)
        return float(logp[0]) if single else logp

    def close(self):
        if self._final is not None:
            self._final()  # runs lfm_post_destroy once
            self._final = None
        self._handle = None

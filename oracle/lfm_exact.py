"""Extended-precision ground truth for the SIM kernel and the MLL — TEST INFRASTRUCTURE ONLY.

``oracle/lfm_oracle.py`` restates the reference's ``h()`` term for term and therefore cancels
where the reference cancels (absolute error ~ eps e^{gamma^2 + 12 D}). This module evaluates
the same mathematical function without that loss, so a device result can be compared with a
value that is right to fp64 rounding at any hyperparameters:

  * ``kxx_exact`` / ``kernel_exact``: the reference formula (model.py:197-235, 315-365 and the
    xf / ff branches, 237-312) in mpmath at ``dps`` digits, rounded to fp64 at the end.
  * ``mtab_scale``: M_tab = |Cm| sum |term| over the five terms of the cancellation-free table
    form (lfm_gram.hip's header); the forward error of a correct table kernel is a small
    multiple of eps M_tab.
  * ``sigma_exact``: the full Sigma of a grid layout from mpmath tables combined in long
    double (64-bit mantissa). The tables depend on d = tau' - tau through the nominal
    difference d dt; the actual difference t_tau' - t_tau of the fp64 grid differs from it by a
    few ulp, which a first-order term restores (the second-order term is ~1e-28 relative).
  * ``mll_exact``: logdet, quadratic form and MLL from a long double column Cholesky.

mpmath is needed by the generator (tests/golden/make_golden_exact.py) and by the CPU tests that
regenerate a subsample; nothing here runs on a GPU box at test time.
"""

from __future__ import annotations

import math

import numpy as np

LD = np.longdouble


def _mp():
    import mpmath

    return mpmath


# ------------------------------------------------------------ direct formula
def _h(mp, Dj, Dk, L, t1, t2):
    """model.py:315-365 on mpf operands."""
    gk = Dk * L / 2
    td = t2 - t1
    mult = mp.exp(gk * gk) / (Dj + Dk)
    a = mp.exp(-Dk * td) * (mp.erf(td / L - gk) + mp.erf(t1 / L + gk))
    b = mp.exp(-(Dk * t2 + Dj * t1)) * (mp.erf(t2 / L - gk) + mp.erf(gk))
    return mult * (a - b)


def _kxx(mp, D, S, l, j, ta, k, tb):
    Dj, Dk, L = mp.mpf(float(D[j])), mp.mpf(float(D[k])), mp.mpf(float(l))
    Ta, Tb = mp.mpf(float(ta)), mp.mpf(float(tb))
    mult = mp.mpf(float(S[j])) * mp.mpf(float(S[k])) * L * mp.sqrt(mp.pi) / 2
    return mult * (_h(mp, Dk, Dj, L, Tb, Ta) + _h(mp, Dj, Dk, L, Ta, Tb))


def kxx_exact(D, S, l, j, ta, k, tb, dps=80):
    """kernel_xx (model.py:197-235) of rows (ta, gene j) and (tb, gene k), rounded to fp64."""
    mp = _mp()
    with mp.workdps(dps):
        return float(_kxx(mp, D, S, l, int(j), ta, int(k), tb))


def _gene(g, G):
    g = math.trunc(g)
    if g < 0:
        g += G
    return int(min(max(g, 0), G - 1))


def kernel_exact(xa, xb, D, S, l, dps=80):
    """The flag-switched kernel (model.py:152-312) of two rows (t, gene, flag), rounded to
    fp64; only the branch whose switch is non-zero is evaluated."""
    mp = _mp()
    G = len(D)
    f1, f2 = math.trunc(xa[2]), math.trunc(xb[2])
    with mp.workdps(dps):
        val = mp.mpf(0)
        if f1 * f2:
            val += f1 * f2 * _kxx(mp, D, S, l, _gene(xa[1], G), xa[0], _gene(xb[1], G), xb[0])
        if (1 - f1) * (1 - f2):
            d = mp.mpf(float(xa[0])) - mp.mpf(float(xb[0]))
            val += (1 - f1) * (1 - f2) * mp.exp(-(d * d) / (2 * mp.mpf(float(l))))
        for sw, ra, rb in ((f1 * (1 - f2), xa, xb), ((1 - f1) * f2, xb, xa)):
            if sw:
                gene, lat = (rb, ra) if ra[2] == 0 else (ra, rb)
                j = _gene(gene[1], G)
                L, Dj = mp.mpf(float(l)), mp.mpf(float(D[j]))
                tl = mp.mpf(float(lat[0]))
                td = mp.mpf(float(gene[0])) - tl
                gj = Dj * L / 2
                val += sw * (L * mp.sqrt(mp.pi) / 2 * mp.mpf(float(S[j])) * mp.exp(gj * gj)
                             * mp.exp(-Dj * td) * (mp.erf(td / L - gj) + mp.erf(tl / L + gj)))
        return float(val)


def kernel_exact_pairs(x, rows, cols, D, S, l, y=None, dps=80):
    """kernel_exact(x[rows[i]], y[cols[i]]) for every i (y defaults to x)."""
    y = x if y is None else y
    return np.array([kernel_exact(x[int(r)], y[int(c)], D, S, l, dps)
                     for r, c in zip(rows, cols)])


# ------------------------------------------------------------------ table form
def _table_terms(mp, D, S, l, j, ta, k, tb):
    """Cm and the five terms of the table form for kxx(j, ta; k, tb), as mpf."""
    Dj, Dk, L = mp.mpf(float(D[j])), mp.mpf(float(D[k])), mp.mpf(float(l))
    Ta, Tb = mp.mpf(float(ta)), mp.mpf(float(tb))
    gj, gk = Dj * L / 2, Dk * L / 2
    delta = Tb - Ta
    Cm = mp.mpf(float(S[j])) * mp.mpf(float(S[k])) * L * mp.sqrt(mp.pi) / 2 / (Dj + Dk)
    Xk = mp.exp(gk * gk - Dk * delta)
    Xj = mp.exp(gj * gj + Dj * delta)
    Wk = Xk * mp.erfc(gk - delta / L)
    Wj = Xj * mp.erfc(gj + delta / L)
    Pk = mp.erfc(Ta / L + gk)
    Pj = mp.erfc(Tb / L + gj)
    Ek, Ej = mp.exp(-Dk * Tb), mp.exp(-Dj * Ta)
    Qk = mp.exp(gk * gk) * (mp.erfc(gk - Tb / L) - mp.erfc(gk))
    Qj = mp.exp(gj * gj) * (mp.erfc(gj - Ta / L) - mp.erfc(gj))
    return Cm, (Wk, Wj, -Xk * Pk, -Xj * Pj, -Ek * Ej * (Qk + Qj))


def mtab_scale(D, S, l, j, ta, k, tb, dps=80):
    """M_tab = |Cm| (|Wt_k| + |Wt_j| + |Xt_k Pt_k| + |Xt_j Pt_j| + |Et_k Et_j (Qt_k + Qt_j)|)."""
    mp = _mp()
    with mp.workdps(dps):
        Cm, terms = _table_terms(mp, D, S, l, int(j), ta, int(k), tb)
        return float(abs(Cm) * sum(abs(t) for t in terms))


def kxx_table_form(D, S, l, j, ta, k, tb, dps=80):
    """kxx through the table identity in mpmath (equals kxx_exact; tests pin the identity)."""
    mp = _mp()
    with mp.workdps(dps):
        Cm, terms = _table_terms(mp, D, S, l, int(j), ta, int(k), tb)
        return float(Cm * sum(terms))


def exact_pairs(x, rows, cols, D, S, l, dps=80):
    """(kxx_exact, mtab_scale) of the gene/gene pairs (x[rows[i]], x[cols[i]])."""
    G = len(D)
    val = np.empty(len(rows))
    mt = np.empty(len(rows))
    for i, (r, c) in enumerate(zip(rows, cols)):
        r, c = int(r), int(c)
        j, k = _gene(x[r, 1], G), _gene(x[c, 1], G)
        val[i] = kxx_exact(D, S, l, j, x[r, 0], k, x[c, 0], dps)
        mt[i] = mtab_scale(D, S, l, j, x[r, 0], k, x[c, 0], dps)
    return val, mt


# --------------------------------------------------------- full Sigma (grid)
def _to_ld(v):
    """mpf -> long double (hi + lo of two fp64 roundings: 64 mantissa bits survive)."""
    hi = float(v)
    return LD(hi) + LD(float(v - hi))


def grid_of(x):
    """(times [T], block genes [nblk]) of x in the dataset_3d block layout, all flags 1."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    T = 1
    while T < n and x[T, 1] == x[0, 1] and x[T, 0] > x[T - 1, 0]:
        T += 1
    assert n % T == 0, "not a block layout"
    t = x[:T, 0].copy()
    blocks = x.reshape(n // T, T, 3)
    assert np.all(blocks[:, :, 0] == t) and np.all(blocks[:, :, 2] == 1)
    assert np.all(blocks[:, :, 1] == blocks[:, :1, 1])
    return t, blocks[:, 0, 1].copy()


class GridTables:
    """The gram tables of lfm_gram.hip's header at extended precision, for the genes in
    ``genes`` only: mpmath entries rounded to long double, plus the first-order term that
    restores the actual time differences of the fp64 grid."""

    def __init__(self, t, D, S, l, genes, dps=50):
        mp = _mp()
        t = np.asarray(t, np.float64)
        T = t.size
        self.T, self.genes = T, [int(g) for g in genes]
        with mp.workdps(dps):
            L = mp.mpf(float(l))
            tm = [mp.mpf(float(v)) for v in t]
            dt = (tm[-1] - tm[0]) / (T - 1) if T > 1 else mp.mpf(0)
            # eps[tau, tau'] = (t_tau' - t_tau) - (tau' - tau) dt, a few ulp of the grid
            self.eps = np.array([[float((tm[b] - tm[a]) - (b - a) * dt) for b in range(T)]
                                 for a in range(T)], dtype=LD)
            ds = [(d, d * dt) for d in range(-(T - 1), T)]
            # d/d delta of Wt is -D Wt + 2 / (l sqrt(pi)) e^{-delta^2 / l^2} (2 gamma / l = D)
            self.Gt = np.array([_to_ld(2 / (L * mp.sqrt(mp.pi)) * mp.exp(-(dl / L) ** 2))
                                for _, dl in ds], dtype=LD)
            self.W, self.X, self.P, self.E, self.Q, self.D = {}, {}, {}, {}, {}, {}
            for g in self.genes:
                Dg = mp.mpf(float(D[g]))
                gam = Dg * L / 2
                X = [mp.exp(gam * gam - Dg * dl) for _, dl in ds]
                self.X[g] = np.array([_to_ld(v) for v in X], dtype=LD)
                self.W[g] = np.array([_to_ld(X[i] * mp.erfc(gam - dl / L))
                                      for i, (_, dl) in enumerate(ds)], dtype=LD)
                self.P[g] = np.array([_to_ld(mp.erfc(v / L + gam)) for v in tm], dtype=LD)
                self.E[g] = np.array([_to_ld(mp.exp(-Dg * v)) for v in tm], dtype=LD)
                eg = mp.exp(gam * gam)
                self.Q[g] = np.array([_to_ld(eg * (mp.erfc(gam - v / L) - mp.erfc(gam)))
                                      for v in tm], dtype=LD)
                self.D[g] = _to_ld(Dg)
            self.Cm = {(j, k): _to_ld(mp.mpf(float(S[j])) * mp.mpf(float(S[k])) * L
                                      * mp.sqrt(mp.pi) / 2 / (mp.mpf(float(D[j])) + mp.mpf(float(D[k]))))
                       for j in self.genes for k in self.genes}

    def block(self, j, k, taus=None, scale=False):
        """Rows (gene j, taus) x columns (gene k, all tau') of K in long double; with ``scale``
        the M_tab of the same entries instead."""
        T = self.T
        taus = np.arange(T) if taus is None else np.asarray(taus)
        tp = np.arange(T)
        d = tp[None, :] - taus[:, None]
        eps = self.eps[taus]
        ik, ij = d + (T - 1), -d + (T - 1)
        Wk, Xk = self.W[k][ik], self.X[k][ik]
        Wj, Xj = self.W[j][ij], self.X[j][ij]
        Pk = self.P[k][taus][:, None]
        Pj = self.P[j][None, :]
        EE = self.E[k][None, :] * self.E[j][taus][:, None]
        QQ = self.Q[k][None, :] + self.Q[j][taus][:, None]
        if scale:
            return np.abs(self.Cm[j, k]) * (np.abs(Wk) + np.abs(Wj) + np.abs(Xk * Pk)
                                            + np.abs(Xj * Pj) + np.abs(EE * QQ))
        # gene k's term moves with +eps, gene j's (argument -delta) with -eps
        fk = (Wk - Xk * Pk) * (1 - eps * self.D[k]) + eps * self.Gt[ik]
        fj = (Wj - Xj * Pj) * (1 + eps * self.D[j]) - eps * self.Gt[ij]
        return self.Cm[j, k] * ((fk + fj) - EE * QQ)


def sigma_exact(x, D, S, l, diag=0.0, dps=50, dtype=np.float64, tables=None):
    """Sigma = K + diag I of a grid layout (dataset_3d blocks on one time grid, all flags 1),
    every entry rounded once from long double to ``dtype`` (fp64 by default; pass
    ``np.longdouble`` to keep the extended values for ``mll_exact``). The lower block triangle
    is computed and mirrored, so the result is exactly symmetric."""
    t, bg = grid_of(x)
    G = len(D)
    bg = [_gene(g, G) for g in bg]
    T, nb = t.size, len(bg)
    tabs = tables or GridTables(t, D, S, l, sorted(set(bg)), dps)
    out = np.empty((nb * T, nb * T), dtype=dtype)
    for bi in range(nb):
        for bk in range(bi + 1):
            blk = tabs.block(bg[bi], bg[bk])
            if bi == bk:
                blk = np.tril(blk) + np.tril(blk, -1).T
            out[bi * T:(bi + 1) * T, bk * T:(bk + 1) * T] = blk
            if bi != bk:
                out[bk * T:(bk + 1) * T, bi * T:(bi + 1) * T] = blk.T
    if np.any(np.atleast_1d(diag) != 0):
        idx = np.diag_indices(nb * T)
        dsum = LD(0)
        for v in np.atleast_1d(diag):
            dsum = dsum + LD(float(v))
        if dtype == np.float64:
            # round once: rebuild the diagonal in long double
            for bi in range(nb):
                dg = np.diagonal(tabs.block(bg[bi], bg[bi])) + dsum
                out[idx[0][bi * T:(bi + 1) * T], idx[1][bi * T:(bi + 1) * T]] = dg
        else:
            out[idx] = out[idx] + dsum
    return out


def sigma_rows_exact(x, rows, D, S, l, tables=None, dps=50):
    """(K[rows, :], M_tab[rows, :]) of a grid layout, fp64 / fp32."""
    t, bg = grid_of(x)
    G = len(D)
    bg = [_gene(g, G) for g in bg]
    T, nb = t.size, len(bg)
    tabs = tables or GridTables(t, D, S, l, sorted(set(bg)), dps)
    K = np.empty((len(rows), nb * T))
    M = np.empty((len(rows), nb * T), dtype=np.float32)
    for i, r in enumerate(rows):
        bi, tau = divmod(int(r), T)
        for bk in range(nb):
            K[i, bk * T:(bk + 1) * T] = tabs.block(bg[bi], bg[bk], [tau])[0]
            M[i, bk * T:(bk + 1) * T] = tabs.block(bg[bi], bg[bk], [tau], scale=True)[0]
    return K, M


# ------------------------------------------------------------------------ MLL
def mll_exact(Sigma, r, perm=None):
    """(mll, logdet, quad) of N(r; 0, Sigma) from a long double column Cholesky (eps 1.1e-19).
    ``perm`` factors the symmetric permutation Sigma[perm][:, perm] instead: the same three
    numbers in exact arithmetic, through different roundings."""
    A = np.array(Sigma, dtype=LD)
    r = np.asarray(r, dtype=LD).reshape(-1)
    if perm is not None:
        A = A[np.ix_(perm, perm)]
        r = r[perm]
    n = A.shape[0]
    Lm = np.zeros((n, n), dtype=LD)
    for j in range(n):
        col = A[j:, j] - Lm[j:, :j] @ Lm[j, :j]
        if not col[0] > 0:
            return float("nan"), float("nan"), float("nan")
        piv = np.sqrt(col[0])
        Lm[j:, j] = col / piv
    z = np.empty(n, dtype=LD)
    for i in range(n):
        z[i] = (r[i] - Lm[i, :i] @ z[:i]) / Lm[i, i]
    logdet = 2 * np.sum(np.log(np.diagonal(Lm)))
    quad = z @ z
    mll = -(n * np.log(2 * LD(np.pi)) + logdet + quad) / 2
    # log(2 pi) from the fp64 pi: n * 1e-17 absolute, far below the tolerances in use
    return float(mll), float(logdet), float(quad)


# ------------------------------------------------------------ reduced problems
def submodel(model, genes=4):
    """The reduced model of the fixtures: genes {argmax D, argmin D, then the lowest-index
    genes not already chosen} of ``model`` with its l, sigma and jitter. Returns
    (sub-model, chosen gene indices)."""
    D = np.asarray(model.true_d, np.float64)
    pick = [int(np.argmax(D)), int(np.argmin(D))]
    for g in range(D.size):
        if len(pick) >= genes:
            break
        if g not in pick:
            pick.append(g)
    pick = pick[:genes]
    sub = model.replace(num_genes=len(pick), true_d=D[pick],
                        true_s=np.asarray(model.true_s, np.float64)[pick],
                        true_b=np.asarray(model.true_b, np.float64)[pick])
    return sub, pick

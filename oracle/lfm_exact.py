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
  * ``mll_grad_exact``: the gradient of log N(y; m, Sigma) in true_d, true_s, true_b, l and
    obs_stddev, g = 1/2 tr(W dSigma) + a^T dm with a = Sigma^{-1} r and W = a a^T - Sigma^{-1}
    from the long double Cholesky and a long double inverse, and the per-component scale
    1/2 sum |W| |dSigma| + |a| |dm| of the same exact quantities. dK/dtheta comes by one of two
    routes, which ``grid_vs_direct`` ties to each other:
      - direct (``pair_grad_exact``): central differences of the reference formula itself in
        mpmath at DIFF_DPS = 100 digits with step DIFF_H = 1e-25. The formula loses up to
        e^{gamma^2 + 12 D} ~ 1e25 to cancellation, so a difference carries 1e-75 / 1e-25
        = 1e-50 of round-off relative to its largest term and h^2 f''' / 6 = 1e-50 times a
        ratio of derivatives (below 1e6 here) of truncation: both far below 1e-30. Any layout,
        any flags; K is homogeneous in S, so dK/dS_g = K (multiplicity of g) / S_g.
      - grid (``GridTables(..., grad=True)``): the D- and l-derivatives of the W, X, P, E, Q
        tables and of Cm and Gt, differenced in mpmath the same way before rounding to long
        double, combined by the product rule in long double. With f_k = Wt_k - Xt_k Pt_k,
        d f_k / d delta = -D_k f_k + Gt, so the first-order grid-spacing term is
        eps (-D_k f_k + Gt); its derivatives eps (-f_k - D_k df_k/dD_k) and
        eps (-D_k df_k/dl + dGt/dl) are carried as well (gene j: the opposite sign).
  * ``grad_tables_exact``: every entry of the 14 derivative tables of the grid gradient (the
    layout of lfm_dual.h's grad_tables_doubles: Wt Xt dWt/dD dXt/dD dWt/dl dXt/dl per
    (gene, d), then Pt dPt/dD dPt/dl Et dEt/dD Qt dQt/dD dQt/dl per (gene, tau)), differenced
    in mpmath, and the magnitude M of the terms an evaluation from the identities sums. With
    g = D l / 2, A = g^2 - D delta, z = g - delta / l, y = t / l + g, u = g - t / l,
    c = 2 / sqrt(pi) (A - z^2 = -delta^2 / l^2, g^2 - u^2 = D t - t^2 / l^2):
        dWt/dD = Wt (g l - delta) - c e^{-delta^2/l^2} l / 2
        dWt/dl = Wt g D - c e^{-delta^2/l^2} (D / 2 + delta / l^2)
        dXt/dD = Xt (g l - delta),   dXt/dl = Xt g D
        dPt/dD = -c e^{-y^2} l / 2,  dPt/dl = -c e^{-y^2} (D / 2 - t / l^2)
        dEt/dD = -t Et
        dQt/dD = g l Qt - c (l / 2) (e^{D t - t^2/l^2} - 1)
        dQt/dl = g D Qt - c ((D / 2 + t / l^2) e^{D t - t^2/l^2} - D / 2)
    M is the sum of the absolute values of the products on the right, with g l - delta taken
    as g l + |delta|, D / 2 -+ x as D / 2 + |x| and Qt as e^{g^2} (erfc(u) + erfc(g)).

  * ``posterior_exact``: the posterior predictors' mean and covariance (model.py:420-514) from
    entries of the reference formula in mpmath carried in long double (never rounded to fp64),
    a long double Cholesky and forward solves; ``PairCache.scale`` gives the magnitude M of the
    cancellation-free form's terms for any flag pairing (``mtab_scale``'s analogue for xf / ff).
  * ``predictive_exact``: joint samples and the held-out log density of
    N(mean, cov + cov_add I) from the same posterior, the covariance never rounded to fp64 before
    its own long double Cholesky.

mpmath is needed by the generators (tests/golden/make_golden_exact.py, make_golden_exact_grad.py,
make_golden_exact_posterior.py and make_golden_exact_predictive.py) and by the CPU tests that
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


def _kxx_m(mp, Dj, Dk, Sj, Sk, L, Ta, Tb):
    """kernel_xx (model.py:197-235) on mpf operands."""
    mult = Sj * Sk * L * mp.sqrt(mp.pi) / 2
    return mult * (_h(mp, Dk, Dj, L, Tb, Ta) + _h(mp, Dj, Dk, L, Ta, Tb))


def _kxx(mp, D, S, l, j, ta, k, tb):
    Dj, Dk, L = mp.mpf(float(D[j])), mp.mpf(float(D[k])), mp.mpf(float(l))
    Ta, Tb = mp.mpf(float(ta)), mp.mpf(float(tb))
    return _kxx_m(mp, Dj, Dk, mp.mpf(float(S[j])), mp.mpf(float(S[k])), L, Ta, Tb)


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
    with mp.workdps(dps):
        return float(_kernel_m(mp, xa, xb, [mp.mpf(float(v)) for v in D],
                               [mp.mpf(float(v)) for v in S], mp.mpf(float(l))))


def _kernel_m(mp, xa, xb, Dm, Sm, L):
    """kernel_exact on mpf hyperparameters (the lists Dm, Sm and L), unrounded."""
    G = len(Dm)
    f1, f2 = math.trunc(xa[2]), math.trunc(xb[2])
    val = mp.mpf(0)
    if f1 * f2:
        j, k = _gene(xa[1], G), _gene(xb[1], G)
        val += f1 * f2 * _kxx_m(mp, Dm[j], Dm[k], Sm[j], Sm[k], L, mp.mpf(float(xa[0])),
                                mp.mpf(float(xb[0])))
    if (1 - f1) * (1 - f2):
        d = mp.mpf(float(xa[0])) - mp.mpf(float(xb[0]))
        val += (1 - f1) * (1 - f2) * mp.exp(-(d * d) / (2 * L))
    for sw, ra, rb in ((f1 * (1 - f2), xa, xb), ((1 - f1) * f2, xb, xa)):
        if sw:
            gene, lat = (rb, ra) if ra[2] == 0 else (ra, rb)
            j = _gene(gene[1], G)
            Dj = Dm[j]
            tl = mp.mpf(float(lat[0]))
            td = mp.mpf(float(gene[0])) - tl
            gj = Dj * L / 2
            val += sw * (L * mp.sqrt(mp.pi) / 2 * Sm[j] * mp.exp(gj * gj)
                         * mp.exp(-Dj * td) * (mp.erf(td / L - gj) + mp.erf(tl / L + gj)))
    return val


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
    restores the actual time differences of the fp64 grid. With ``grad`` also their D- and
    l-derivatives (``dW[g] = (dWt/dD_g, dWt/dl)`` and so on, ``GtL``, ``CmD = dCm/dD_j =
    dCm/dD_k``, ``CmL``), differenced in mpmath at DIFF_DPS digits before rounding, which
    ``block_grad`` combines by the product rule."""

    def __init__(self, t, D, S, l, genes, dps=50, grad=False):
        mp = _mp()
        t = np.asarray(t, np.float64)
        T = t.size
        self.T, self.genes = T, [int(g) for g in genes]
        if grad:
            self._init_grad(mp, t, D, S, l)
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

    def _init_grad(self, mp, t, D, S, l):
        T = self.T
        with mp.workdps(DIFF_DPS):
            h = mp.mpf(DIFF_H)
            L = mp.mpf(float(l))
            tm = [mp.mpf(float(v)) for v in t]
            dt = (tm[-1] - tm[0]) / (T - 1) if T > 1 else mp.mpf(0)
            deltas = [d * dt for d in range(-(T - 1), T)]

            def ld(plus, minus):
                return np.array([_to_ld((p - m) / (2 * h)) for p, m in zip(plus, minus)], dtype=LD)

            def gt(Lv):
                return [2 / (Lv * mp.sqrt(mp.pi)) * mp.exp(-(dl / Lv) ** 2) for dl in deltas]

            self.GtL = ld(gt(L + h), gt(L - h))
            self.dW, self.dX, self.dP, self.dE, self.dQ = {}, {}, {}, {}, {}
            for g in self.genes:
                Dg = mp.mpf(float(D[g]))
                dp, dm = _gene_tables_m(mp, Dg + h, L, deltas, tm), _gene_tables_m(mp, Dg - h, L, deltas, tm)
                lp, lm = _gene_tables_m(mp, Dg, L + h, deltas, tm), _gene_tables_m(mp, Dg, L - h, deltas, tm)
                for name, store in (("W", self.dW), ("X", self.dX), ("P", self.dP),
                                    ("E", self.dE), ("Q", self.dQ)):
                    store[g] = (ld(dp[name], dm[name]), ld(lp[name], lm[name]))
            self.CmD, self.CmL = {}, {}
            for j in self.genes:
                for k in self.genes:
                    cm = (mp.mpf(float(S[j])) * mp.mpf(float(S[k])) * L * mp.sqrt(mp.pi) / 2
                          / (mp.mpf(float(D[j])) + mp.mpf(float(D[k]))))
                    # Cm = const l / (D_j + D_k)
                    self.CmD[j, k] = _to_ld(-cm / (mp.mpf(float(D[j])) + mp.mpf(float(D[k]))))
                    self.CmL[j, k] = _to_ld(cm / L)

    def block_grad(self, j, k, taus=None, scale=False):
        """(K, dK/dD_j, dK/dD_k, dK/dl) of the rows (gene j, taus) x columns (gene k, all tau')
        in long double, the D-derivatives as partials (for j == k their sum is dK/dD_j); with
        ``scale`` the sums of the absolute values of the product-rule terms instead."""
        T = self.T
        taus = np.arange(T) if taus is None else np.asarray(taus)
        d = np.arange(T)[None, :] - taus[:, None]
        eps = self.eps[taus]
        ik, ij = d + (T - 1), -d + (T - 1)
        col, row = (lambda v: v[None, :]), (lambda v: v[taus][:, None])
        Wk, Xk, Wj, Xj = self.W[k][ik], self.X[k][ik], self.W[j][ij], self.X[j][ij]
        WkD, Wkl, XkD, Xkl = self.dW[k][0][ik], self.dW[k][1][ik], self.dX[k][0][ik], self.dX[k][1][ik]
        WjD, Wjl, XjD, Xjl = self.dW[j][0][ij], self.dW[j][1][ij], self.dX[j][0][ij], self.dX[j][1][ij]
        Pk, PkD, Pkl = row(self.P[k]), row(self.dP[k][0]), row(self.dP[k][1])
        Pj, PjD, Pjl = col(self.P[j]), col(self.dP[j][0]), col(self.dP[j][1])
        Ek, EkD = col(self.E[k]), col(self.dE[k][0])
        Ej, EjD = row(self.E[j]), row(self.dE[j][0])
        Qk, QkD, Qkl = col(self.Q[k]), col(self.dQ[k][0]), col(self.dQ[k][1])
        Qj, QjD, Qjl = row(self.Q[j]), row(self.dQ[j][0]), row(self.dQ[j][1])
        EE, QQ = Ek * Ej, Qk + Qj
        Cm, CmD, CmL = self.Cm[j, k], self.CmD[j, k], self.CmL[j, k]
        if scale:
            a = np.abs
            MV = a(Wk) + a(Wj) + a(Xk * Pk) + a(Xj * Pj) + a(EE * QQ)
            mk = a(WkD) + a(XkD * Pk) + a(Xk * PkD) + a(EkD * Ej * QQ) + a(EE * QkD)
            mj = a(WjD) + a(XjD * Pj) + a(Xj * PjD) + a(Ek * EjD * QQ) + a(EE * QjD)
            ml = (a(Wkl) + a(Xkl * Pk) + a(Xk * Pkl) + a(Wjl) + a(Xjl * Pj) + a(Xj * Pjl)
                  + a(EE * Qkl) + a(EE * Qjl))
            return (a(Cm) * MV, a(CmD) * MV + a(Cm) * mj, a(CmD) * MV + a(Cm) * mk,
                    a(CmL) * MV + a(Cm) * ml)
        Dk, Dj = self.D[k], self.D[j]
        fk, fkD, fkl = Wk - Xk * Pk, WkD - XkD * Pk - Xk * PkD, Wkl - Xkl * Pk - Xk * Pkl
        fj, fjD, fjl = Wj - Xj * Pj, WjD - XjD * Pj - Xj * PjD, Wjl - Xjl * Pj - Xj * Pjl
        # gene k's term moves with +eps along delta, gene j's (argument -delta) with -eps
        ck = fk + eps * (self.Gt[ik] - Dk * fk)
        ckD = fkD - eps * (fk + Dk * fkD)
        ckl = fkl + eps * (self.GtL[ik] - Dk * fkl)
        cj = fj - eps * (self.Gt[ij] - Dj * fj)
        cjD = fjD + eps * (fj + Dj * fjD)
        cjl = fjl - eps * (self.GtL[ij] - Dj * fjl)
        V = (ck + cj) - EE * QQ
        Vk = ckD - EkD * Ej * QQ - EE * QkD
        Vj = cjD - Ek * EjD * QQ - EE * QjD
        Vl = (ckl + cjl) - EE * (Qkl + Qjl)
        return Cm * V, CmD * V + Cm * Vj, CmD * V + Cm * Vk, CmL * V + Cm * Vl


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
def _chol_ld(A):
    """Lower Cholesky factor of the long double matrix A by columns; None when not PD."""
    n = A.shape[0]
    Lm = np.zeros((n, n), dtype=LD)
    for j in range(n):
        col = A[j:, j] - Lm[j:, :j] @ Lm[j, :j]
        if not col[0] > 0:
            return None
        piv = np.sqrt(col[0])
        Lm[j:, j] = col / piv
    return Lm


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
    Lm = _chol_ld(A)
    if Lm is None:
        return float("nan"), float("nan"), float("nan")
    z = np.empty(n, dtype=LD)
    for i in range(n):
        z[i] = (r[i] - Lm[i, :i] @ z[:i]) / Lm[i, i]
    logdet = 2 * np.sum(np.log(np.diagonal(Lm)))
    quad = z @ z
    mll = -(n * np.log(2 * LD(np.pi)) + logdet + quad) / 2
    # log(2 pi) from the fp64 pi: n * 1e-17 absolute, far below the tolerances in use
    return float(mll), float(logdet), float(quad)


# ------------------------------------------------------------------- gradient
DIFF_DPS = 100   # digits of every differenced evaluation
DIFF_H = "1e-25"  # central-difference step (see the module docstring for the error budget)
GRAD_KEYS = ("d", "s", "b", "l", "obs_stddev")


def _gene_tables_m(mp, Dg, L, deltas, tm):
    """One gene's W, X (per delta) and P, E, Q (per time) tables as mpf lists."""
    gam = Dg * L / 2
    X = [mp.exp(gam * gam - Dg * dl) for dl in deltas]
    W = [X[i] * mp.erfc(gam - dl / L) for i, dl in enumerate(deltas)]
    eg = mp.exp(gam * gam)
    return dict(W=W, X=X, P=[mp.erfc(v / L + gam) for v in tm], E=[mp.exp(-Dg * v) for v in tm],
                Q=[eg * (mp.erfc(gam - v / L) - mp.erfc(gam)) for v in tm])


def _pair_grad_m(mp, xa, xb, Dm, Sm, L, h):
    """(K, {g: dK/dD_g}, {g: dK/dS_g}, dK/dl) of one pair as mpf, by central differences."""
    G = len(Dm)
    f1, f2 = math.trunc(xa[2]), math.trunc(xb[2])
    assert f1 in (0, 1) and f2 in (0, 1), "flags 0 / 1: exactly one branch is live"
    K = _kernel_m(mp, xa, xb, Dm, Sm, L)
    mult = {}
    for f, row in ((f1, xa), (f2, xb)):
        if f:
            g = _gene(row[1], G)
            mult[g] = mult.get(g, 0) + 1
    dD, dS = {}, {}
    for g, cnt in mult.items():
        up, dn = list(Dm), list(Dm)
        up[g], dn[g] = Dm[g] + h, Dm[g] - h
        dD[g] = (_kernel_m(mp, xa, xb, up, Sm, L) - _kernel_m(mp, xa, xb, dn, Sm, L)) / (2 * h)
        dS[g] = K * cnt / Sm[g]
    dl = (_kernel_m(mp, xa, xb, Dm, Sm, L + h) - _kernel_m(mp, xa, xb, Dm, Sm, L - h)) / (2 * h)
    return K, dD, dS, dl


def pair_grad_exact(xa, xb, D, S, l):
    """The direct route for one pair of rows (t, gene, flag): K, dK/dD [G], dK/dS [G] and
    dK/dl, each rounded once to long double."""
    mp = _mp()
    G = len(D)
    with mp.workdps(DIFF_DPS):
        K, dD, dS, dl = _pair_grad_m(mp, xa, xb, [mp.mpf(float(v)) for v in D],
                                     [mp.mpf(float(v)) for v in S], mp.mpf(float(l)),
                                     mp.mpf(DIFF_H))
        oD, oS = np.zeros(G, dtype=LD), np.zeros(G, dtype=LD)
        for g in dD:
            oD[g], oS[g] = _to_ld(dD[g]), _to_ld(dS[g])
        return _to_ld(K), oD, oS, _to_ld(dl)


def dk_direct(x, D, S, l):
    """One block in ``mll_grad_exact``'s form holding the whole of K and its derivatives by
    the direct route: the lower triangle pair by pair, mirrored."""
    x = np.asarray(x, np.float64)
    n, G = x.shape[0], len(D)
    K, dl = np.zeros((n, n), dtype=LD), np.zeros((n, n), dtype=LD)
    dD, dS = np.zeros((G, n, n), dtype=LD), np.zeros((G, n, n), dtype=LD)
    for i in range(n):
        for c in range(i + 1):
            K[i, c], dD[:, i, c], dS[:, i, c], dl[i, c] = pair_grad_exact(x[i], x[c], D, S, l)
            K[c, i], dD[:, c, i], dS[:, c, i], dl[c, i] = K[i, c], dD[:, i, c], dS[:, i, c], dl[i, c]
    sl = slice(0, n)
    return [(sl, sl, 1, K, {g: dD[g] for g in range(G)}, {g: dS[g] for g in range(G)}, dl)]


def dk_grid(x, D, S, l, tables):
    """K and its derivatives of a grid layout by the grid route, block by block (a generator
    of ``mll_grad_exact`` blocks: the lower block triangle, the off-diagonal blocks counted
    twice, the diagonal ones mirrored from their lower triangle as sigma_exact's are)."""
    t, bg = grid_of(x)
    G = len(D)
    bg = [_gene(g, G) for g in bg]
    T = t.size
    for bi in range(len(bg)):
        for bk in range(bi + 1):
            j, k = bg[bi], bg[bk]
            Kb, dj, dk, dl = tables.block_grad(j, k)
            if bi == bk:
                Kb, dj, dk, dl = (np.tril(v) + np.tril(v, -1).T for v in (Kb, dj, dk, dl))
            dD = {j: dj + dk} if j == k else {j: dj, k: dk}
            Sj, Sk = LD(float(S[j])), LD(float(S[k]))
            dS = {j: 2 * Kb / Sj} if j == k else {j: Kb / Sj, k: Kb / Sk}
            yield (slice(bi * T, (bi + 1) * T), slice(bk * T, (bk + 1) * T),
                   1 if bi == bk else 2, Kb, dD, dS, dl)


def w_exact(Sigma, r):
    """(a = Sigma^{-1} r, W = a a^T - Sigma^{-1}, logdet, quad) in long double: the column
    Cholesky of ``mll_exact``, the factor's inverse by forward substitution on the identity,
    Sigma^{-1} = L^{-T} L^{-1}. None when Sigma is not PD."""
    A = np.array(Sigma, dtype=LD)
    r = np.asarray(r, dtype=LD).reshape(-1)
    n = A.shape[0]
    Lm = _chol_ld(A)
    if Lm is None:
        return None
    Li = np.zeros((n, n), dtype=LD)
    for i in range(n):
        row = -(Lm[i, :i] @ Li[:i, :i + 1])
        row[i] += 1
        Li[i, :i + 1] = row / Lm[i, i]
    Sinv = Li.T @ Li
    z = Li @ r
    a = Li.T @ z
    return a, np.outer(a, a) - Sinv, 2 * np.sum(np.log(np.diagonal(Lm))), z @ z


def contract_grad(blocks, W, a, x, D, B, obs_stddev, dtype=LD):
    """The gradient dict (GRAD_KEYS and scale_* in oracle.mll_grad's layout, fp64 arrays) of
    g = 1/2 sum W dSigma + a^T dm over ``blocks`` = (row slice, column slice, weight, K,
    {g: dK/dD_g}, {g: dK/dS_g}, dK/dl), with every operand cast to ``dtype`` first (long
    double: the truth; fp64: the restatement on correctly rounded inputs)."""
    G, n = len(D), x.shape[0]
    W, a = np.asarray(W, dtype=dtype), np.asarray(a, dtype=dtype)
    g = {k: np.zeros(G, dtype=dtype) for k in ("d", "s")}
    sc = {k: np.zeros(G, dtype=dtype) for k in ("d", "s")}
    gl = sl = dtype(0)
    for rs, cs, wgt, _, dD, dS, dl in blocks:
        Wb = W[rs, cs]
        aW = np.abs(Wb)
        half = dtype(wgt) / 2
        for key, parts in (("d", dD), ("s", dS)):
            for q, m in parts.items():
                m = np.asarray(m, dtype=dtype)
                g[key][q] += half * np.sum(Wb * m)
                sc[key][q] += half * np.sum(aW * np.abs(m))
        m = np.asarray(dl, dtype=dtype)
        gl += half * np.sum(Wb * m)
        sl += half * np.sum(aW * np.abs(m))
    # mean: m_i = (B / D)[i // (n / G)] flag_i (model.py:124-149: the block position)
    bs = n // G
    f = np.trunc(x[:, 2]).astype(dtype)
    Dt, Bt = np.asarray(D, dtype=dtype), np.asarray(B, dtype=dtype)
    af = np.array([np.sum((a * f)[q * bs:(q + 1) * bs]) for q in range(G)], dtype=dtype)
    aabs = np.array([np.sum(np.abs(a * f)[q * bs:(q + 1) * bs]) for q in range(G)], dtype=dtype)
    sd = dtype(float(obs_stddev))
    dg = np.diagonal(W)
    out = {"d": g["d"] - Bt / (Dt * Dt) * af, "s": g["s"], "b": af / Dt, "l": gl,
           "obs_stddev": sd * np.sum(dg),
           "scale_d": sc["d"] + np.abs(Bt / (Dt * Dt)) * aabs, "scale_s": sc["s"],
           "scale_b": aabs / np.abs(Dt), "scale_l": sl,
           "scale_obs_stddev": np.abs(sd) * np.sum(np.abs(dg))}
    return {k: np.asarray(v, dtype=np.float64) for k, v in out.items()}


def residual_ld(x, y, D, B):
    """r = y - m in long double, m_i = (B / D)[i // (n / G)] flag_i."""
    n, G = x.shape[0], len(D)
    m = (np.asarray(B, dtype=LD) / np.asarray(D, dtype=LD))[np.arange(n) // (n // G)]
    return np.asarray(y, dtype=LD).reshape(-1) - m * np.trunc(x[:, 2]).astype(LD)


def mll_grad_exact(x, y, D, S, B, l, obs_stddev, jitter, tables=None, blocks=None):
    """Exact value and gradient of log N(y; m, K + (jitter + obs_stddev^2) I): a dict with
    value, logdet, quad, GRAD_KEYS and scale_* (oracle.mll_grad's layout), plus ``blocks``
    (the long double K and derivative blocks), ``Sigma`` (long double) and ``r`` for a
    restatement on rounded inputs. The grid route with ``tables`` (GridTables(grad=True)),
    else the direct route. Where Sigma is not positive definite: {"not_pd": True, Sigma, r}."""
    x = np.asarray(x, np.float64)
    n = x.shape[0]
    if blocks is None:
        blocks = list(dk_grid(x, D, S, l, tables)) if tables is not None else dk_direct(x, D, S, l)
    Sig = np.zeros((n, n), dtype=LD)
    for rs, cs, _, Kb, _, _, _ in blocks:
        Sig[rs, cs] = Kb
        Sig[cs, rs] = Kb.T
    idx = np.diag_indices(n)
    Sig[idx] = Sig[idx] + (LD(float(jitter)) + LD(float(obs_stddev)) * LD(float(obs_stddev)))
    r = residual_ld(x, y, D, B)
    got = w_exact(Sig, r)
    if got is None:  # not positive definite: no gradient; the caller gets Sigma to say by how much
        return {"not_pd": True, "Sigma": Sig, "r": r}
    a, W, logdet, quad = got
    out = contract_grad(blocks, W, a, x, D, B, obs_stddev)
    out.update(value=float(-(n * np.log(2 * LD(np.pi)) + logdet + quad) / 2),
               logdet=float(logdet), quad=float(quad), blocks=blocks, Sigma=Sig, r=r)
    return out


def mll_grad_fp64(ex, x, D, B, obs_stddev):
    """The fp64 restatement of ``mll_grad_exact``'s result ``ex``: scipy's Cholesky and inverse
    on the correctly rounded Sigma and residual, the exact dSigma rounded to fp64."""
    import scipy.linalg

    Sig, r = ex["Sigma"].astype(np.float64), ex["r"].astype(np.float64)
    c = scipy.linalg.cho_factor(Sig, lower=True, check_finite=False)
    a = scipy.linalg.cho_solve(c, r, check_finite=False)
    W = np.outer(a, a) - scipy.linalg.cho_solve(c, np.eye(Sig.shape[0]), check_finite=False)
    return contract_grad(ex["blocks"], W, a, x, D, B, obs_stddev, dtype=np.float64)


def grad_error(got, ex, sign=1.0):
    """The largest |got - sign exact| / scale over the components of two gradient dicts."""
    worst = 0.0
    for k in GRAD_KEYS:
        e = np.abs(np.atleast_1d(got[k]) - sign * np.atleast_1d(ex[k]))
        worst = max(worst, float(np.max(e / np.atleast_1d(ex["scale_" + k]))))
    return worst


def grid_vs_direct(x, rows, cols, D, S, l, tables):
    """The tie between the routes on the pairs (x[rows[i]], x[cols[i]]) of a grid layout: the
    largest |grid - direct| / (sum of the absolute values of the product-rule terms) over K,
    dK/dD_row, dK/dD_col and dK/dl."""
    t, bg = grid_of(x)
    G, T = len(D), t.size
    worst = 0.0
    for r, c in zip(rows, cols):
        r, c = int(r), int(c)
        j, k = _gene(bg[r // T], G), _gene(bg[c // T], G)
        K, dD, _, dl = pair_grad_exact(x[r], x[c], D, S, l)
        got = [v[0][c % T] for v in tables.block_grad(j, k, [r % T])]
        mag = [v[0][c % T] for v in tables.block_grad(j, k, [r % T], scale=True)]
        if j == k:
            ref = (K, dD[j], dl)
            got, mag = (got[0], got[1] + got[2], got[3]), (mag[0], mag[1] + mag[2], mag[3])
        else:
            ref = (K, dD[j], dD[k], dl)
        worst = max(worst, max(float(abs(g - v) / m) for g, v, m in zip(got, ref, mag)))
    return worst


def grad_tables_exact(t, D, l):
    """(exact, M), each a flat fp64 array in the layout of the device's 14 derivative tables
    (grad_tables_doubles: six Toeplitz tables G x (2T - 1), eight time tables G x T) on the
    uniform grid t: the derivative tables by central differences in mpmath, M from the
    identities in the module docstring."""
    mp = _mp()
    t = np.asarray(t, np.float64)
    T, G = t.size, len(D)
    with mp.workdps(DIFF_DPS):
        h = mp.mpf(DIFF_H)
        L = mp.mpf(float(l))
        tm = [mp.mpf(float(v)) for v in t]
        dt = (tm[-1] - tm[0]) / (T - 1)
        deltas = [d * dt for d in range(-(T - 1), T)]
        c = 2 / mp.sqrt(mp.pi)
        toe = [[] for _ in range(6)]
        tim = [[] for _ in range(8)]
        mtoe = [[] for _ in range(6)]
        mtim = [[] for _ in range(8)]
        for g in range(G):
            Dg = mp.mpf(float(D[g]))
            b = _gene_tables_m(mp, Dg, L, deltas, tm)
            dp, dm = _gene_tables_m(mp, Dg + h, L, deltas, tm), _gene_tables_m(mp, Dg - h, L, deltas, tm)
            lp, lm = _gene_tables_m(mp, Dg, L + h, deltas, tm), _gene_tables_m(mp, Dg, L - h, deltas, tm)

            def dif(p, m, name):
                return [(u - v) / (2 * h) for u, v in zip(p[name], m[name])]

            for w, vals in enumerate((b["W"], b["X"], dif(dp, dm, "W"), dif(dp, dm, "X"),
                                      dif(lp, lm, "W"), dif(lp, lm, "X"))):
                toe[w] += [float(v) for v in vals]
            for w, vals in enumerate((b["P"], dif(dp, dm, "P"), dif(lp, lm, "P"), b["E"],
                                      dif(dp, dm, "E"), b["Q"], dif(dp, dm, "Q"),
                                      dif(lp, lm, "Q"))):
                tim[w] += [float(v) for v in vals]
            gam = Dg * L / 2
            for i, dl in enumerate(deltas):
                Wv, Xv = abs(b["W"][i]), abs(b["X"][i])
                ez = c * mp.exp(-(dl / L) ** 2)
                lin = gam * L + abs(dl)
                for w, v in enumerate((Wv, Xv, Wv * lin + ez * L / 2, Xv * lin,
                                       Wv * gam * Dg + ez * (Dg / 2 + abs(dl) / (L * L)),
                                       Xv * gam * Dg)):
                    mtoe[w].append(float(v))
            eg = mp.exp(gam * gam)
            for i, tv in enumerate(tm):
                ey = c * mp.exp(-(tv / L + gam) ** 2)
                MQ = eg * (mp.erfc(gam - tv / L) + mp.erfc(gam))
                eq = mp.exp(Dg * tv - tv * tv / (L * L))
                Ev = b["E"][i]
                for w, v in enumerate((b["P"][i], ey * L / 2, ey * (Dg / 2 + tv / (L * L)), Ev,
                                       tv * Ev, MQ, gam * L * MQ + c * (L / 2) * (eq + 1),
                                       gam * Dg * MQ + c * ((Dg / 2 + tv / (L * L)) * eq + Dg / 2))):
                    mtim[w].append(float(v))
    flat = [v for tab in toe + tim for v in tab]
    mflat = [v for tab in mtoe + mtim for v in tab]
    return np.array(flat), np.array(mflat)


# ------------------------------------------------------------------ posterior
def _row_key(row, G):
    """A row (t, gene, flag) as the kernel reads it: a latent row's gene index is not read."""
    f = math.trunc(row[2])
    return (float(row[0]), _gene(row[1], G) if f else 0, f)


def _pair_scale_m(mp, xa, xb, Dm, Sm, L):
    """The magnitude M of the terms of the cancellation-free form of ``_kernel_m`` for rows with
    flags 0 / 1: gene / gene |Cm| sum |term| (``mtab_scale``); gene / latent
    l sqrt(pi) / 2 S_j (|Wt_j| + |Xt_j Pt_j|) with delta = t_gene - t_latent and Pt at the latent
    time; latent / latent the value itself."""
    G = len(Dm)
    f1, f2 = math.trunc(xa[2]), math.trunc(xb[2])
    assert f1 in (0, 1) and f2 in (0, 1)
    if f1 and f2:
        j, k = _gene(xa[1], G), _gene(xb[1], G)
        Ta, Tb = mp.mpf(float(xa[0])), mp.mpf(float(xb[0]))
        gj, gk = Dm[j] * L / 2, Dm[k] * L / 2
        delta = Tb - Ta
        Cm = Sm[j] * Sm[k] * L * mp.sqrt(mp.pi) / 2 / (Dm[j] + Dm[k])
        Xk, Xj = mp.exp(gk * gk - Dm[k] * delta), mp.exp(gj * gj + Dm[j] * delta)
        Qk = mp.exp(gk * gk) * (mp.erfc(gk - Tb / L) - mp.erfc(gk))
        Qj = mp.exp(gj * gj) * (mp.erfc(gj - Ta / L) - mp.erfc(gj))
        terms = (Xk * mp.erfc(gk - delta / L), Xj * mp.erfc(gj + delta / L),
                 Xk * mp.erfc(Ta / L + gk), Xj * mp.erfc(Tb / L + gj),
                 mp.exp(-Dm[k] * Tb) * mp.exp(-Dm[j] * Ta) * (Qk + Qj))
        return abs(Cm) * sum(abs(v) for v in terms)
    if not f1 and not f2:
        return abs(_kernel_m(mp, xa, xb, Dm, Sm, L))
    gene, lat = (xa, xb) if f1 else (xb, xa)
    j = _gene(gene[1], G)
    tl = mp.mpf(float(lat[0]))
    td = mp.mpf(float(gene[0])) - tl
    gj = Dm[j] * L / 2
    X = mp.exp(gj * gj - Dm[j] * td)
    return abs(L * mp.sqrt(mp.pi) / 2 * Sm[j]) * (X * mp.erfc(gj - td / L) + X * mp.erfc(tl / L + gj))


class PairCache:
    """kernel(xa, xb) of rows (t, gene, flag) with flags 0 / 1 at ``dps`` digits, each distinct
    pair evaluated once (the kernel is symmetric) and carried as a long double; ``scale`` gives
    ``_pair_scale_m`` of the same pair as fp64. A pair whose terms are far below the cancelling
    ones of the reference formula is evaluated at as many more digits as that takes."""

    def __init__(self, D, S, l, dps=60):
        self.mp = _mp()
        self.dps = dps
        with self.mp.workdps(dps):
            self.Dm = [self.mp.mpf(float(v)) for v in D]
            self.Sm = [self.mp.mpf(float(v)) for v in S]
            self.L = self.mp.mpf(float(l))
        self.G = len(D)
        self.val, self.mag = {}, {}

    def _key(self, xa, xb):
        ka, kb = _row_key(xa, self.G), _row_key(xb, self.G)
        return (ka, kb) if ka <= kb else (kb, ka)

    def _digits(self, key, mag):
        """Digits at which the reference formula, which loses e^{gamma^2 + D |dt|} to
        cancellation, is still right to 1e-30 of ``mag`` (prefactors are below 1e3)."""
        (ta, ja, fa), (tb, jb, fb) = key
        if mag == 0 or not (fa or fb):
            return self.dps
        mp = self.mp
        A = max((self.Dm[g] * self.L / 2) ** 2 + self.Dm[g] * abs(ta - tb)
                for g, f in ((ja, fa), (jb, fb)) if f)
        return max(self.dps, 33 + int(math.ceil(float(A / mp.log(10) - mp.log10(mag)))))

    def _mag(self, key):
        if key not in self.mag:
            with self.mp.workdps(self.dps):
                self.mag[key] = _pair_scale_m(self.mp, key[0], key[1], self.Dm, self.Sm, self.L)
        return self.mag[key]

    def value(self, xa, xb):
        key = self._key(xa, xb)
        if key not in self.val:
            with self.mp.workdps(self._digits(key, self._mag(key))):
                self.val[key] = _to_ld(_kernel_m(self.mp, key[0], key[1], self.Dm, self.Sm, self.L))
        return self.val[key]

    def scale(self, xa, xb):
        return float(self._mag(self._key(xa, xb)))

    def matrix(self, xa, xb=None, scale=False):
        """kernel (or its scale) of every row of xa against every row of xb; with xb None the
        lower triangle of xa against itself, mirrored."""
        fn = self.scale if scale else self.value
        dt = np.float64 if scale else LD
        if xb is None:
            n = len(xa)
            out = np.zeros((n, n), dtype=dt)
            for i in range(n):
                for c in range(i + 1):
                    out[i, c] = out[c, i] = fn(xa[i], xa[c])
            return out
        return np.array([[fn(a, b) for b in xb] for a in xa], dtype=dt).reshape(len(xa), len(xb))


def posterior_entries(x, t, D, S, l, dps=60, diag_only=False, cache=None):
    """(K(x,x), K(t,x), K(t,t)) in long double from ``_kernel_m`` at ``dps`` digits, never
    rounded to fp64; with ``diag_only`` the third is the diagonal of K(t,t) alone."""
    x, t = np.asarray(x, np.float64), np.asarray(t, np.float64)
    pc = cache or PairCache(D, S, l, dps)
    Ktt = (np.array([pc.value(r, r) for r in t], dtype=LD) if diag_only else pc.matrix(t))
    return pc.matrix(x), pc.matrix(t, x), Ktt


def _posterior_parts(ent, x, y, diag_vec, diag_add, t, D, B, dtype, perm):
    """(m(t), V = L^{-1} K(x,t), z = L^{-1} (y - m(x)), K(t,t)) in ``dtype`` behind
    ``posterior_from_entries`` and ``predictive_exact``; None when S is not positive definite."""
    Kxx, Ktx, Ktt = ent
    x, t = np.asarray(x, np.float64), np.asarray(t, np.float64)
    n, m, G = x.shape[0], t.shape[0], len(D)
    dv = np.zeros(n) if diag_vec is None else np.asarray(diag_vec, np.float64).reshape(-1)
    Sig = np.array(Kxx, dtype=LD)
    idx = np.diag_indices(n)
    Sig[idx] = Sig[idx] + (dv.astype(LD) + LD(float(diag_add)))
    r = residual_ld(x, y, D, B)
    Kxt = np.array(Ktx, dtype=LD).T
    if perm is not None:
        Sig, r, Kxt = Sig[np.ix_(perm, perm)], r[perm], Kxt[perm]
    mt = ((np.asarray(B, dtype=LD) / np.asarray(D, dtype=LD))[np.arange(m) // (m // G)]
          * np.trunc(t[:, 2]).astype(LD))
    if dtype == LD:
        Lm = _chol_ld(Sig)
        if Lm is None:
            return None
        W = np.concatenate([Kxt, r[:, None]], axis=1)
        for i in range(n):
            W[i] = (W[i] - Lm[i, :i] @ W[:i]) / Lm[i, i]
    else:
        import scipy.linalg

        try:
            Lm = scipy.linalg.cholesky(Sig.astype(dtype), lower=True, check_finite=False)
        except (np.linalg.LinAlgError, scipy.linalg.LinAlgError):
            return None
        W = scipy.linalg.solve_triangular(
            Lm, np.concatenate([Kxt, r[:, None]], axis=1).astype(dtype), lower=True,
            check_finite=False)
        mt, Ktt = mt.astype(dtype), np.asarray(Ktt).astype(dtype)
    return mt, W[:, :m], W[:, m], Ktt


def posterior_from_entries(ent, x, y, diag_vec, diag_add, t, D, B, dtype=LD, perm=None):
    """(mean, cov) of the posterior from the entries ``ent`` of ``posterior_entries`` (cov is the
    variance vector when ent[2] is K(t,t)'s diagonal): S = K(x,x) + diag(diag_vec) + diag_add I,
    V = L^{-1} K(x,t), z = L^{-1} (y - m(x)), mean = m(t) + V^T z, cov = K(t,t) - V^T V, in
    ``dtype`` (long double: the truth, by ``_chol_ld``; fp64: scipy's Cholesky and triangular
    solves on the entries rounded once). ``perm`` factors the symmetric permutation instead.
    (None, None) when S is not positive definite."""
    parts = _posterior_parts(ent, x, y, diag_vec, diag_add, t, D, B, dtype, perm)
    if parts is None:
        return None, None
    mt, V, z, Ktt = parts
    mean = mt + V.T @ z
    cov = Ktt - np.sum(V * V, axis=0) if np.ndim(Ktt) == 1 else Ktt - V.T @ V
    return mean.astype(np.float64), cov.astype(np.float64)


def predictive_exact(ent, x, y, diag_vec, diag_add, t, D, B, cov_add, ystar, z, dtype=LD,
                     perm=None):
    """(mean [m], logp, X [len(z), m]) of the predictive distribution N(mean, cov + cov_add I)
    behind ``multi_gene_predict(...).log_prob`` / ``.sample``: the posterior as
    ``posterior_from_entries`` forms it, with the covariance kept in ``dtype`` (long double: it is
    not rounded to fp64 before ``cov_add`` joins its diagonal), the scale's Cholesky factor L
    (``_chol_ld``), logp = -(m log 2 pi + 2 sum log L_ii + |L^{-1} (ystar - mean)|^2) / 2 from a
    forward solve and the factor's diagonal, and X = mean + z L^T for the normals ``z``; rounded
    to fp64 at the end. ``ent`` holds the full K(t,t). ``ystar`` None: logp is None; ``z`` None:
    X is None. ``dtype=np.float64``: scipy's Cholesky and triangular solves on the entries rounded
    once. ``perm`` permutes the training rows. (None, None, None) where S or the scale is not
    positive definite."""
    parts = _posterior_parts(ent, x, y, diag_vec, diag_add, t, D, B, dtype, perm)
    if parts is None:
        return None, None, None
    mt, V, zr, Ktt = parts
    assert np.ndim(Ktt) == 2, "the full K(t,t)"
    m = mt.shape[0]
    mean = mt + V.T @ zr
    scale = Ktt - V.T @ V
    idx = np.diag_indices(m)
    scale[idx] = scale[idx] + dtype(float(cov_add))
    if dtype == LD:
        Lc = _chol_ld(scale)
        if Lc is None:
            return None, None, None
    else:
        import scipy.linalg

        try:
            Lc = scipy.linalg.cholesky(scale, lower=True, check_finite=False)
        except (np.linalg.LinAlgError, scipy.linalg.LinAlgError):
            return None, None, None
    logp = None
    if ystar is not None:
        d = np.asarray(ystar, np.float64).reshape(-1).astype(dtype) - mean
        if dtype == LD:
            w = np.empty(m, dtype=LD)
            for i in range(m):
                w[i] = (d[i] - Lc[i, :i] @ w[:i]) / Lc[i, i]
        else:
            w = scipy.linalg.solve_triangular(Lc, d, lower=True, check_finite=False)
        logdet = 2 * np.sum(np.log(np.diagonal(Lc)))
        # log(2 pi) from the fp64 pi: m * 1e-17 absolute, as in mll_exact
        logp = float(-(m * np.log(2 * dtype(np.pi)) + logdet + w @ w) / 2)
    X = None
    if z is not None:
        X = (mean + np.atleast_2d(np.asarray(z, np.float64)).astype(dtype) @ Lc.T).astype(np.float64)
    return mean.astype(np.float64), logp, X


def posterior_exact(x, y, diag_vec, diag_add, t, D, S, B, l, dps=60, perm=None, diag_only=False,
                    entries=None):
    """The exact posterior (mean [m], cov [m, m]) of model.py:420-514's predictors before their
    jitter assembly, mean = m(t) + K(t,x) S^{-1} (y - m(x)), cov = K(t,t) - K(t,x) S^{-1} K(x,t),
    S = K(x,x) + diag(diag_vec) + diag_add I: entries from the reference formula in mpmath at
    ``dps`` digits carried in long double, a long double Cholesky and forward solves, rounded to
    fp64 at the end. ``diag_only``: the variances instead of cov. (None, None) where S is not
    positive definite in this arithmetic."""
    ent = entries or posterior_entries(x, t, D, S, l, dps, diag_only)
    return posterior_from_entries(ent, x, y, diag_vec, diag_add, t, D, B, perm=perm)


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

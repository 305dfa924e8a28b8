"""NumPy restatement of the leave-one-out pass over the Cholesky factor (csrc/loo.hip) and its error bounds.
Test helper only: the package never imports it.

Conventions are the project's: K the un-negated kernel matrix, A = -K + lam I (n x n, n = 3N M), y the labels normalised by
std, a = A^-1 y (the library's coefficients are alphas = -a).  With blk_j the 3N indices of training point j, G_j the
diagonal block j of A^-1 (Rasmussen & Williams 5.4.2 in block form):
    r_j = G_j^-1 a_j   = y_j - (prediction at x_j of the model trained without point j)
    C_j = G_j^-1       = predictive covariance of the left-out label, noise lam included
    log det A = 2 sum log L_ii
"""
import numpy as np
import scipy.linalg as sla

import _uncertainty_ref as ur

TAU = ur.TAU  # the project's assembly contract: max|dA| <= 1e-12 max|A|
EPS = ur.EPS


def loo_identity(A, y, n3):
    """(r (M,3N), C (M,3N,3N), log det A) by scipy's Cholesky -> L^-1 -> block Gram -> block Cholesky solve."""
    n = len(A)
    M = n // n3
    L = sla.cholesky(A, lower=True, check_finite=False)
    Linv = sla.solve_triangular(L, np.eye(n), lower=True, check_finite=False)
    a = sla.cho_solve((L, True), y, check_finite=False)
    r, C = np.empty((M, n3)), np.empty((M, n3, n3))
    for j in range(M):
        Z = Linv[:, j * n3:(j + 1) * n3]  # = (E_j^T L^-T)^T; zero above row 3N j
        cG = sla.cho_factor(Z.T @ Z, lower=True, check_finite=False)
        r[j] = sla.cho_solve(cG, a[j * n3:(j + 1) * n3], check_finite=False)
        C[j] = sla.cho_solve(cG, np.eye(n3), check_finite=False)
    return r, C, 2.0 * np.sum(np.log(np.diag(L)))


def loo_brute(A, y, n3, folds):
    """r_j for the given folds by deleting block j and solving each fold by Cholesky: (r (len(folds),3N), list of the folds'
    coefficients beta_j (n - 3N))."""
    n = len(A)
    r, betas = [], []
    for j in folds:
        keep = np.r_[0:j * n3, (j + 1) * n3:n]
        blk = np.arange(j * n3, (j + 1) * n3)
        beta = sla.cho_solve(sla.cho_factor(A[np.ix_(keep, keep)], lower=True, check_finite=False), y[keep], check_finite=False)
        r.append(y[blk] - A[np.ix_(blk, keep)] @ beta)
        betas.append(beta)
    return np.array(r), betas


class Bounds(object):
    """The elementwise error bounds of one system (A, y), with A^-1 formed once.

    A Cholesky factor is the exact factor of A + dA with ||dA||_2 <~ eps ||A||_2, and the assembled matrix differs from the
    reference's by max|dA| <= tau max|A|.  To first order in dA, with V_j = A^-1[:, blk_j] G_j^-1 (n x 3N) and beta_j the
    coefficients of fold j padded with zeros at blk_j (beta_j = a - V_j a_j):
        d r_j = -V_j^T dA beta_j        d C_j = V_j^T dA V_j        d log det A = tr(A^-1 dA)
    (d G_j = -E_j^T A^-1 dA A^-1 E_j, d C_j = -C_j dG_j C_j, d a = -A^-1 dA a).  Hence
        tol_j     = 4 eps ||A||_2 ||V_j||_2 ||beta_j||_2  +  tau max|A| max_col ||V_j||_1 ||beta_j||_1
        cov_tol_j = 4 eps ||A||_2 ||V_j||_2^2             +  tau max|A| (max_col ||V_j||_1)^2
        logdet_tol = 4 eps ||A||_2 tr(A^-1)               +  tau max|A| sum|A^-1|
    the form and the factor 4 of _uncertainty_ref.cov_tol.  The two CPU routes (loo_identity, loo_brute) differ by at most
    0.028 of the first term of tol_j on the fixtures of tests/test_loo_cpu.py."""

    def __init__(self, A, y, n3):
        self.n3 = n3
        self.Ainv = sla.cho_solve(sla.cho_factor(A, lower=True, check_finite=False), np.eye(len(A)), check_finite=False)
        self.a = self.Ainv @ y
        self.nA = float(sla.eigvalsh(A, subset_by_index=[len(A) - 1, len(A) - 1])[0])  # ||A||_2, A symmetric positive definite
        self.maxA = float(np.abs(A).max())

    def _V_beta(self, j):
        blk = slice(j * self.n3, (j + 1) * self.n3)
        V = sla.solve(self.Ainv[blk, blk], self.Ainv[blk, :], assume_a='pos', check_finite=False).T  # (n,3N), G_j symmetric
        beta = self.a - V @ self.a[blk]
        beta[blk] = 0.0
        return V, beta

    def terms(self, j):
        """(first term of tol_j, second term of tol_j, cov_tol_j)."""
        V, beta = self._V_beta(j)
        nV, cV = np.linalg.norm(V, 2), np.abs(V).sum(axis=0).max()
        return (4.0 * EPS * self.nA * nV * np.linalg.norm(beta), TAU * self.maxA * cV * np.abs(beta).sum(),
                4.0 * EPS * self.nA * nV * nV + TAU * self.maxA * cV * cV)

    def logdet_tol(self):
        return 4.0 * EPS * self.nA * np.trace(self.Ainv) + TAU * self.maxA * np.abs(self.Ainv).sum()


def loo_tol(A, y, n3, j, bounds=None):
    """Elementwise bound on |r_gpu - r_ref| for point j (derivation: Bounds)."""
    t = (bounds or Bounds(A, y, n3)).terms(j)
    return t[0] + t[1]


def system(g, lam=None):
    """(A, y, n3, std) of a golden fixture at its stored lam (or the given one); y = F_train / std."""
    R_train, x, gd, tp, _ = ur.fixture_tables(g)
    lam = float(g['lam']) if lam is None else float(lam)
    A = ur.system_matrix(x, gd, tp, float(g['sig']), lam)
    std = float(g['model_std'])
    y = np.asarray(g['F_train'], dtype=np.float64).ravel() / std
    return A, y, R_train.shape[1], std

"""NumPy restatement of the gradient of the model evidence in sig and lam (csrc/evidence.hip) and its error
bounds.  Test helper only: the package never imports it.

Conventions are the project's: K the un-negated kernel matrix (oracle._full_K), A = -K + lam I (n x n, n = 3N M), y the labels
normalised by std, a = A^-1 y (the library's coefficients are alphas = -a), model y ~ N(0, s^2 A), s^2 = y^T a / n:
    lml = -1/2 y^T a / s^2 - 1/2 (log det A + n log s^2) - n/2 log 2 pi
    d lml / d sig = 1/2 (<A^-1, K'> - a^T K' a / s^2),   d lml / d lam = 1/2 (a^T a / s^2 - tr A^-1),   K' = dK/dsig.
For a pair of points, a permutation p, d = x_i - P_p x_j, r = sqrt(5) |d|, e = exp(-r / sig) the block of K is
    J_i^T [f1 d d^T - f2 I] J_j^p,   f1 = 25 e / (3 sig^4),   f2 = 5 e (sig + r) / (3 sig^3),
and that of K' has f1' = f1 (r - 4 sig) / sig^2, f2' = 5 e (r^2 - 2 sig r - 2 sig^2) / (3 sig^5) in their place.
"""
import numpy as np
import scipy.linalg as sla

import _uncertainty_ref as ur
from oracle import gdml_oracle as orc

TAU = ur.TAU
EPS = ur.EPS
TERMS = ('tr_Ainv', 'Ainv_dK', 'a_dK_a', 'a_a', 'log_det_A')


def dK_dsig(R_desc, R_d_desc, tril_perms, sig):
    """K' = dK/dsig (n x n, forces only), the loop of oracle._full_K with f1', f2' in the place of f1, f2."""
    R_desc = np.asarray(R_desc, dtype=np.float64)
    M, D = R_desc.shape
    n3 = 3 * orc.n_atoms_from_dim_d(D)
    sig = float(sig)
    J = orc.d_desc_from_comp(np.asarray(R_d_desc, dtype=np.float64))  # (M,D,3N)
    Jt = np.ascontiguousarray(J.transpose(0, 2, 1))
    Kp = np.zeros((M * n3, M * n3))
    for j in range(M):
        xj_p = R_desc[j][tril_perms]  # (P,D)
        Jj_p = J[j][tril_perms]  # (P,D,3N)
        d = R_desc[:, None, :] - xj_p[None]  # (M,P,D)
        r = np.sqrt(5.0) * np.sqrt(np.sum(d * d, axis=-1))  # (M,P)
        e = np.exp(-r / sig)
        f1p = 25.0 * e / (3.0 * sig**4) * (r - 4.0 * sig) / sig**2
        f2p = 5.0 * e * (r * r - 2.0 * sig * r - 2.0 * sig * sig) / (3.0 * sig**5)
        u = np.matmul(d.transpose(1, 0, 2), Jj_p).transpose(1, 0, 2)  # (M,P,3N): d_p^T J_j^p
        B = np.matmul((f1p[..., None] * d).transpose(0, 2, 1), u)  # (M,D,3N)
        B -= np.tensordot(f2p, Jj_p, axes=([1], [0]))
        Kp[:, j * n3:(j + 1) * n3] = np.matmul(Jt, B).reshape(M * n3, n3)
    return Kp


def tables(g):
    """(R_desc, R_d_desc, tril_perms, y, n3, std) of a golden fixture; y = F_train / std."""
    R_train, x, gd, tp, _ = ur.fixture_tables(g)
    std = float(g['model_std'])
    return x, gd, tp, np.asarray(g['F_train'], dtype=np.float64).ravel() / std, R_train.shape[1], std


def evidence(A, y, s2=None):
    """lml at the maximum-likelihood signal variance s^2 = y^T A^-1 y / n, or at the given one."""
    n = len(A)
    cA = sla.cho_factor(A, lower=True, check_finite=False)
    a = sla.cho_solve(cA, y, check_finite=False)
    s2 = np.dot(y, a) / n if s2 is None else s2
    logdet = 2.0 * np.sum(np.log(np.diag(cA[0])))
    return -0.5 * np.dot(y, a) / s2 - 0.5 * (logdet + n * np.log(s2)) - 0.5 * n * np.log(2.0 * np.pi)


def evidence_at(x, gd, tp, y, sig, lam, s2=None):
    return evidence(ur.system_matrix(x, gd, tp, sig, lam), y, s2)


class Bounds(object):
    """The five terms, the two derivatives and their error bounds for one system (A, K', y), with A^-1 formed once.

    A Cholesky factor is the exact factor of A + dA with ||dA||_2 <~ eps ||A||_2 (factor 4 as in _uncertainty_ref.cov_tol), and the
    assembled matrices differ from the reference's by max|dA| <= tau max|A|, max|dK'| <= tau max|K'|.  To first order, with
    d A^-1 = -A^-1 dA A^-1, d a = -A^-1 dA a, B = A^-1 K' A^-1, w = A^-1 K' a, z = A^-1 a:
        d tr A^-1      = -tr(A^-2 dA)                    <= 4 eps ||A||_2 tr(A^-2) + tau max|A| sum|A^-2|
        d <A^-1, K'>   = -<B, dA> + <A^-1, dK'>          <= 4 eps ||A||_2 ||B||_* + tau max|A| sum|B| + tau max|K'| sum|A^-1|
        d a^T K' a     = -2 w^T dA a + a^T dK' a         <= 8 eps ||A||_2 ||w|| ||a|| + 2 tau max|A| ||w||_1 ||a||_1 + tau max|K'| ||a||_1^2
        d a^T a        = -2 z^T dA a                     <= 8 eps ||A||_2 ||z|| ||a|| + 2 tau max|A| ||z||_1 ||a||_1
        d log det A    = tr(A^-1 dA)                     <= 4 eps ||A||_2 tr(A^-1) + tau max|A| sum|A^-1|   (_loo_ref.Bounds.logdet_tol)
        d s^2          = -a^T dA a / n                   <= (4 eps ||A||_2 ||a||^2 + tau max|A| ||a||_1^2) / n
    and the derivatives get the propagated sums
        d_sig_tol = 1/2 (tol[<A^-1, K'>] + tol[a K' a] / s^2 + |a K' a| tol[s^2] / s^4)
        d_lam_tol = 1/2 (tol[a a] / s^2 + a^T a tol[s^2] / s^4 + tol[tr A^-1]).
    No free constants."""

    def __init__(self, A, Kp, y):
        n = len(A)
        self.n = n
        cA = sla.cho_factor(A, lower=True, check_finite=False)
        Ainv = sla.cho_solve(cA, np.eye(n), check_finite=False)
        a = sla.cho_solve(cA, y, check_finite=False)
        nA = float(sla.eigvalsh(A, subset_by_index=[n - 1, n - 1])[0])
        maxA, maxK = float(np.abs(A).max()), float(np.abs(Kp).max())
        A2 = Ainv @ Ainv
        B = Ainv @ Kp @ Ainv
        w, z = Ainv @ (Kp @ a), Ainv @ a
        n1 = lambda v: float(np.abs(v).sum())
        n2 = lambda v: float(np.linalg.norm(v))
        self.a = a
        self.s2 = float(np.dot(y, a) / n)
        logdet = 2.0 * float(np.sum(np.log(np.diag(cA[0]))))
        self.terms = np.array([np.trace(Ainv), np.sum(Ainv * Kp), a @ Kp @ a, a @ a, logdet])
        self.tol = np.array([
            4.0 * EPS * nA * np.trace(A2) + TAU * maxA * n1(A2),
            4.0 * EPS * nA * n1(sla.eigvalsh(0.5 * (B + B.T))) + TAU * maxA * n1(B) + TAU * maxK * n1(Ainv),
            8.0 * EPS * nA * n2(w) * n2(a) + 2.0 * TAU * maxA * n1(w) * n1(a) + TAU * maxK * n1(a) ** 2,
            8.0 * EPS * nA * n2(z) * n2(a) + 2.0 * TAU * maxA * n1(z) * n1(a),
            4.0 * EPS * nA * np.trace(Ainv) + TAU * maxA * n1(Ainv),
        ])
        self.s2_tol = (4.0 * EPS * nA * n2(a) ** 2 + TAU * maxA * n1(a) ** 2) / n
        tr, ik, aka, aa, _ = self.terms
        s2 = self.s2
        self.d_sig = 0.5 * (ik - aka / s2)
        self.d_lam = 0.5 * (aa / s2 - tr)
        self.d_sig_tol = 0.5 * (self.tol[1] + self.tol[2] / s2 + abs(aka) * self.s2_tol / s2**2)
        self.d_lam_tol = 0.5 * (self.tol[3] / s2 + aa * self.s2_tol / s2**2 + self.tol[0])
        self.lml = -0.5 * n - 0.5 * (logdet + n * np.log(s2)) - 0.5 * n * np.log(2.0 * np.pi)


def bounds_of(g, lam=None, sig=None):
    """Bounds of a golden fixture at its stored sig and lam (or the given ones)."""
    x, gd, tp, y, _, _ = tables(g)
    sig = float(g['sig']) if sig is None else float(sig)
    lam = float(g['lam']) if lam is None else float(lam)
    return Bounds(ur.system_matrix(x, gd, tp, sig, lam), dK_dsig(x, gd, tp, sig), y)

"""NumPy restatement of the posterior force covariance of the sGDML Gaussian process (csrc/uncert.hip), on top
of the oracle's descriptors.  Test helper only: the package never imports it.

Conventions are the project's: K is the un-negated kernel matrix (oracle._full_K), A = -K + lam I, labels normalised by std.
For a query geometry q
    Kx_q (3N, n)   block j = the kernel block of row point q (un-permuted) and training point j (permuted column point)
    k_qq (3N, 3N)  the same formula with i = j = q
    Sig_q = -k_qq - (-Kx_q) A^-1 (-Kx_q)^T
"""
import numpy as np
import scipy.linalg as sla

from oracle import gdml_oracle as orc

TAU = 1e-12  # the project's assembly contract: max|dK| <= 1e-12 max|K|
EPS = 2.0 ** -52


def _block(xq, Jq, xj, Jj, tril_perms, sig):
    """One 3N x 3N block, directly from the formula of the kernel's Hessian (train.py:97-232): row point (xq, Jq) un-permuted,
    column point (xj, Jj) under every permutation.  J: full (D,3N) Jacobians."""
    blk = np.zeros((Jq.shape[1], Jj.shape[1]))
    for tp in tril_perms:
        d = xq - xj[tp]  # (D,)
        Jp = Jj[tp]  # (D,3N)
        nrm = np.sqrt(5.0) * np.sqrt(np.sum(d * d))
        b = 5.0 * np.exp(-nrm / sig) / (3.0 * sig**4)
        A = 5.0 * b * np.outer(d, d @ Jp) - (sig**2 + sig * nrm) * b * Jp  # (D,3N)
        blk += Jq.T @ A
    return blk


def cross_rows(R, R_desc, R_d_desc, tril_perms, sig, lat_and_inv=None):
    """Un-negated Kx (B,3N,n) and k_qq (B,3N,3N) of geometries R (B,3N) against the training set R_desc (M,D), R_d_desc (M,D,3)."""
    R = np.asarray(R, dtype=np.float64)
    R = R.reshape(1 if R.ndim == 1 else R.shape[0], -1)
    sig = float(sig)
    xq, gq = orc.desc_from_R(R, lat_and_inv)
    Jq = orc.d_desc_from_comp(gq)
    Jt = orc.d_desc_from_comp(R_d_desc)
    B, M, n3 = R.shape[0], R_desc.shape[0], R.shape[1]
    Kx = np.zeros((B, n3, M * n3))
    kqq = np.zeros((B, n3, n3))
    for q in range(B):
        for j in range(M):
            Kx[q][:, j * n3:(j + 1) * n3] = _block(xq[q], Jq[q], R_desc[j], Jt[j], tril_perms, sig)
        kqq[q] = _block(xq[q], Jq[q], xq[q], Jq[q], tril_perms, sig)
    return Kx, kqq


def system_matrix(R_desc, R_d_desc, tril_perms, sig, lam):
    A = -orc._full_K(np.asarray(R_desc, dtype=np.float64), np.asarray(R_d_desc, dtype=np.float64), tril_perms, float(sig), False)
    A[np.diag_indices_from(A)] += float(lam)
    return A


def posterior_cov(Kx, kqq, A):
    """Sig_q (B,3N,3N) in normalised units, by scipy's Cholesky and triangular solve."""
    L = sla.cholesky(A, lower=True, check_finite=False)
    out = np.empty_like(kqq)
    for q in range(Kx.shape[0]):
        Z = sla.solve_triangular(L, -Kx[q].T, lower=True, check_finite=False)  # (n,3N)
        out[q] = -kqq[q] - Z.T @ Z
    return out


def cov_tol(Kx_q, kqq_q, A, norm_A=None):
    """Elementwise bound on |Sig_gpu - Sig_ref| for one query:

        tol_q = 4 eps ||A||_2 ||X_q||_2^2  +  2 tau max|Kx_q| max_col ||X_q||_1  +  tau max|k_qq|,     X_q = A^-1 Kx_q^T.

    First term: a Cholesky factor is the exact factor of A + dA with ||dA|| <~ eps ||A||; to first order k^T A^-1 k then moves
    by x^T dA x <= eps ||A||_2 ||x||^2 with x = A^-1 k.  On the CPU two fp64 summation orders and an 80-bit evaluation differ
    by at most 0.56 of that 1x bound; the factor 4 leaves about 7x.  Second and third term: the assembly contract tau of the
    cross-kernel (each entry of Kx_q and k_qq off by up to tau times the largest entry) carried through Sig: d(k^T x) =
    2 dk^T x <= 2 tau max|Kx_q| ||x||_1 per column x of X_q, and dk_qq directly."""
    X = sla.cho_solve(sla.cho_factor(A, lower=True, check_finite=False), Kx_q.T, check_finite=False)  # (n,3N)
    nA = np.linalg.norm(A, 2) if norm_A is None else norm_A
    return (4.0 * EPS * nA * np.linalg.norm(X, 2) ** 2 + 2.0 * TAU * np.abs(Kx_q).max() * np.abs(X).sum(axis=0).max()
            + TAU * np.abs(kqq_q).max())


# ---- fixtures


def fixture_tables(g):
    """(R_train (M,3N), R_desc, R_d_desc, tril_perms, lat_and_inv) of a golden fixture, descriptors by the oracle."""
    M = g['R_train'].shape[0]
    lat_and_inv = (np.asarray(g['lattice']), np.linalg.inv(g['lattice'])) if 'lattice' in g else None
    R_train = np.asarray(g['R_train'], dtype=np.float64).reshape(M, -1)
    x, gd = orc.desc_from_R(R_train, lat_and_inv)
    tp = orc.tril_perms_from_atom_perms(np.asarray(g['perms']))
    return R_train, x, gd, tp, lat_and_inv


def model_from_fixture(g):
    """Model dict for GDMLPredict with the keys a trained model carries (train.py create_model): the prediction tables plus
    lam, alphas_F and use_E_cstr."""
    R_train, x, gd, tp, lat_and_inv = fixture_tables(g)
    M = x.shape[0]
    perms = np.asarray(g['perms'])
    use_E = bool(g['use_E_cstr']) if 'use_E_cstr' in g else False
    n_ff = M * R_train.shape[1]
    alphas_F = np.asarray(g['alphas'], dtype=np.float64)[:n_ff]
    model = {
        'type': 'm', 'z': np.ones(perms.shape[1], dtype=np.int64), 'R_desc': np.ascontiguousarray(x.T),
        'R_d_desc_alpha': orc.d_desc_dot_vec(gd, alphas_F.reshape(M, -1)), 'sig': float(g['sig']), 'lam': float(g['lam']),
        'std': float(g['model_std']), 'c': float(g['model_c']), 'perms': perms, 'alphas_F': alphas_F, 'use_E_cstr': use_E,
        'tril_perms_lin': orc.tril_perms_lin_from_tril_perms(tp),
    }
    if lat_and_inv is not None:
        model['lattice'] = lat_and_inv[0]
    if use_E:
        model['alphas_E'] = np.asarray(g['alphas'], dtype=np.float64)[n_ff:]
    return model


def queries(g):
    """The first six test geometries and the first training geometry."""
    Rt = np.asarray(g['R_test'], dtype=np.float64)
    Rt = Rt.reshape(len(Rt), -1)
    return np.concatenate([Rt[:6], np.asarray(g['R_train'], dtype=np.float64)[:1].reshape(1, -1)])


def cancel_floor(model, gd):
    """The prediction sum's round-off floor of tests/test_oracle_golden.cancel_floor, from a model dict."""
    M, P, sig = model['R_desc'].shape[1], len(model['perms']), float(model['sig'])
    return (50 * np.finfo(float).eps * float(model['std']) * np.abs(model['R_d_desc_alpha']).max() * 5.0 / (3 * sig**2)
            * np.sqrt(M * P) * max(1.0, np.abs(gd).max()))

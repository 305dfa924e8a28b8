"""NumPy/SciPy restatement of appending training points to a Cholesky factor by bordering (csrc/extend.hip),
and the reference values of the enlarged system that the GPU tests compare against.  Test helper only: the package never
imports it.

Conventions are the project's (tests/_uncertainty_ref.py, tests/_loo_ref.py): A = -K + lam I, labels normalised by std.  With
A = L L^T of order n and m new rows
    A' = | A  C^T |     L' = | L  0   |     W = C L^-T,   S = D - W W^T = L_S L_S^T.
         | C  D   |          | W  L_S |
"""
import numpy as np
import scipy.linalg as sla

import _loo_ref as lr
import _uncertainty_ref as ur
from oracle import gdml_oracle as orc


def border(L, C, D):
    """Factor of [[A, C^T], [C, D]] from the factor L of A: (n + m) x (n + m) lower triangular."""
    n, m = len(L), len(D)
    W = sla.solve_triangular(L, C.T, lower=True, check_finite=False).T
    LS = sla.cholesky(D - W @ W.T, lower=True, check_finite=False)
    out = np.zeros((n + m, n + m))
    out[:n, :n] = L
    out[n:, :n] = W
    out[n:, n:] = LS
    return out


def extend(A_full, n0, steps):
    """Factor of the leading block of order n0 + sum(steps) of A_full, grown from the factor of its leading n0 x n0 block by
    one bordering per entry of `steps` (rows per step)."""
    L = sla.cholesky(A_full[:n0, :n0], lower=True, check_finite=False)
    n = n0
    for m in steps:
        L = border(L, A_full[n:n + m, :n], A_full[n:n + m, n:n + m])
        n += m
    return L


def cov_from_factor(L, Kx, kqq):
    """Sig_q (B,3N,3N) in normalised units from a given factor (posterior_cov of _uncertainty_ref with L handed in)."""
    out = np.empty_like(kqq)
    for q in range(Kx.shape[0]):
        Z = sla.solve_triangular(L, -Kx[q].T, lower=True, check_finite=False)
        out[q] = -kqq[q] - Z.T @ Z
    return out


SPLITS = {'b1': [1], 'b3': [3], 'seq': [2, 1, 4]}
SPLITS_SMALL = {'b1': [1], 'b3': [3], 'seq': [1, 1]}  # the fixtures of 9 - 10 points


def splits_of(M):
    return SPLITS_SMALL if M <= 10 else SPLITS


def tables(g):
    """Everything of a fixture-like dict the tests need: geometries, labels, descriptors by the oracle, permutations."""
    R_train, x, gd, tp, lat = ur.fixture_tables(g)
    M = len(R_train)
    return {'R': R_train, 'F': np.asarray(g['F_train'], dtype=np.float64).reshape(M, -1),
            'E': np.asarray(g['E_train'], dtype=np.float64).ravel(), 'x': x, 'gd': gd, 'tp': tp, 'lat': lat,
            'sig': float(g['sig']), 'lam': float(g['lam']), 'std': float(g['model_std']), 'c': float(g['model_c']),
            'perms': np.asarray(g['perms'])}


def model_dict(t, M, alphas_F):
    """Model dict (the keys train.py create_model sets) of the first M points of tables t with the given coefficients."""
    n3 = t['R'].shape[1]
    alphas_F = np.asarray(alphas_F, dtype=np.float64).ravel()
    m = {'type': 'm', 'z': np.ones(t['perms'].shape[1], dtype=np.int64), 'R_desc': np.ascontiguousarray(t['x'][:M].T),
         'R_d_desc_alpha': orc.d_desc_dot_vec(t['gd'][:M], alphas_F.reshape(M, n3)), 'sig': t['sig'], 'lam': t['lam'],
         'std': t['std'], 'c': t['c'], 'perms': t['perms'], 'alphas_F': alphas_F, 'use_E_cstr': False,
         'tril_perms_lin': orc.tril_perms_lin_from_tril_perms(t['tp']), 'idxs_train': np.arange(M),
         'f_err': {'mae': 0.25, 'rmse': 0.5}}
    if t['lat'] is not None:
        m['lattice'] = t['lat'][0]
    return m


def full_reference(t, Rq, with_loo=True):
    """Reference values of the FULL system of tables t (all M points) for queries Rq: A, y, the covariances and their bounds,
    the solve, the leave-one-out residuals and log det A with theirs.  Nothing here comes from the code under test."""
    n3 = t['R'].shape[1]
    A = ur.system_matrix(t['x'], t['gd'], t['tp'], t['sig'], t['lam'])
    y = t['F'].ravel() / t['std']
    Kx, kqq = ur.cross_rows(Rq, t['x'], t['gd'], t['tp'], t['sig'], t['lat'])
    Sig = ur.posterior_cov(Kx, kqq, A)
    nA = float(sla.eigvalsh(A, subset_by_index=[len(A) - 1, len(A) - 1])[0])
    tol = np.array([ur.cov_tol(Kx[q], kqq[q], A, nA) for q in range(len(Rq))])
    a = sla.cho_solve(sla.cho_factor(A, lower=True, check_finite=False), y, check_finite=False)
    out = {'A': A, 'nA': nA, 'y': y, 'n3': n3, 'Kx': Kx, 'kqq': kqq, 'Sig': Sig, 'tol': tol, 'scale': float(np.dot(y, a) / y.size)}
    if with_loo:
        r, _, logdet = lr.loo_identity(A, y, n3)
        b = lr.Bounds(A, y, n3)
        T = np.array([b.terms(j) for j in range(len(A) // n3)])
        out.update({'r': r, 'logdet': logdet, 'loo_tol': T[:, 0] + T[:, 1], 'logdet_tol': b.logdet_tol()})
    return out


def solve_tol(nA, x, y):
    """_tol.solve_tol with ||A||_2 handed in (the largest eigenvalue of the positive definite A, already known)."""
    return max(1e-10, np.finfo(np.float64).eps * nA * np.linalg.norm(x) / np.linalg.norm(y))


# ---- the synthetic case at panel and tile boundaries: P = 1, 3N = 18, 100 points -> n = 1800; the base of 84 points ends at
# column 1512, so the 288 new rows and columns run across column 1536 = 3 x 512 (a panel boundary of the triangular solve)
# and the chunk's rows fill more than two 128-row tiles.  sig and lam were chosen on the CPU so that the meaningfulness cap
# of the covariance bound holds for the seven queries (tests/test_extend_cpu.py asserts it).
SYNTH = {'N': 6, 'M': 100, 'b': 16, 'seed': 5, 'jitter': 0.3, 'sig': 10.0, 'lam': 1e-6, 'n_test': 7}


def synth_fixture():
    """A fixture-like dict (the keys of tests/golden/*.npz that tables() and _uncertainty_ref.queries() read)."""
    s = SYNTH
    ds = orc.synth_dataset(s['N'], s['M'] + s['n_test'], seed=s['seed'], jitter=s['jitter'])
    R = np.asarray(ds['R'], dtype=np.float64).reshape(s['M'] + s['n_test'], s['N'], 3)
    F = np.asarray(ds['F'], dtype=np.float64).reshape(s['M'] + s['n_test'], s['N'], 3)
    E = np.asarray(ds['E'], dtype=np.float64).ravel()
    M = s['M']
    return {'R_train': R[:M], 'F_train': F[:M], 'E_train': E[:M], 'R_test': R[M:], 'F_test': F[M:].reshape(s['n_test'], -1),
            'E_test': E[M:], 'perms': np.arange(s['N'])[None], 'sig': s['sig'], 'lam': s['lam'],
            'model_std': float(np.std(F[:M])), 'model_c': 0.0}

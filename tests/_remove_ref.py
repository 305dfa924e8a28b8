"""NumPy restatement of removing training points from a Cholesky factor (csrc/remove.hip), the removal sets
of the tests and the helper that cuts a fixture's tables down to the kept points.  Test helper only: the package never
imports it.  The reference values the tests compare against are _extend_ref.full_reference(subset(t, keep), Rq): SciPy on
the kept points alone.

With A = L L^T, L_c = L[kept, kept] and V = L[kept, removed]:  A_kept = L_c L_c^T + V V^T, and an orthogonal Q with
[L_c V] Q = [L' 0] gives the factor L' of A_kept.  Q is built 64 columns at a time: a Householder LQ of [L_kk V_k] (reflector
i = e_i + [0; v_i]), kept as the pair (U, T) with Q_k = I - [I; U^T] T [I, U], applied to the rows below; columns whose diagonal
entry comes out negative are negated.  V goes through in column slices, highest first; a slice's sweep does not touch the
other slices' columns."""
import numpy as np

BLOCK = 64
WIDTH = 128  # widest slice of V (columns)


def sets_of(M):
    """Removal sets of a fixture of M points: indices in the CURRENT order, one list per call.  Point 0 is never removed: it is
    the seventh query of _uncertainty_ref.queries, and the tightest one."""
    return {'one': [[M // 2]], 'three': [[1, M // 2, M - 1]], 'seq': [[2, 5], [1]] if M > 10 else [[2], [1]]}


SYNTH_SET = [[28, 29, 57]]  # the synthetic case of _extend_ref (3N = 18, M = 100): columns 504 .. 539 and 1026 .. 1043 leave


def keep_after(M, calls):
    """Original indices of the points that are left after the calls, in order."""
    keep = np.arange(M)
    for idx in calls:
        mask = np.ones(len(keep), dtype=bool)
        mask[np.asarray(idx)] = False
        keep = keep[mask]
    return keep


def subset(t, keep):
    """The tables of _extend_ref.tables for the points `keep` only."""
    out = dict(t)
    for k in ('R', 'F', 'E', 'x', 'gd'):
        out[k] = np.ascontiguousarray(t[k][keep])
    return out


def reduced_reference(full, t, keep, with_loo=True):
    """_extend_ref.full_reference(subset(t, keep), Rq) without assembling again: A of the kept points is the principal
    submatrix of the full system's A and their cross-kernel rows are columns of the full Kx, both from the oracle (a block of
    the kernel matrix depends on its two points alone; tests/test_remove_cpu.py checks the submatrix against a fresh
    assembly).  Everything else -- SciPy's factor, solve, covariances, leave-one-out values and the bounds -- is computed on
    the kept points only, with the formulas of full_reference.  Nothing here comes from the code under test."""
    import scipy.linalg as sla

    import _loo_ref as lr
    import _uncertainty_ref as ur

    n3 = full['n3']
    rows = (np.repeat(keep, n3) * n3 + np.tile(np.arange(n3), len(keep))).astype(np.int64)
    A = np.ascontiguousarray(full['A'][np.ix_(rows, rows)])
    y = t['F'][keep].ravel() / t['std']
    Kx, kqq = np.ascontiguousarray(full['Kx'][:, :, rows]), full['kqq']
    # One factorisation serves the covariances, the bounds and the solve (posterior_cov, cov_tol and full_reference factor
    # A once each, nine times in all: minutes at n = 7500); the formulas are theirs, test_remove_cpu compares the results.
    c = sla.cho_factor(A, lower=True, check_finite=False)
    Sig = np.empty_like(kqq)
    for q in range(len(Kx)):
        Z = sla.solve_triangular(c[0], -Kx[q].T, lower=True, check_finite=False)
        Sig[q] = -kqq[q] - Z.T @ Z
    bounds = lr.Bounds(A, y, n3) if with_loo else None
    nA = bounds.nA if with_loo else float(sla.eigvalsh(A, subset_by_index=[len(A) - 1, len(A) - 1])[0])
    tol = np.empty(len(Kx))
    for q in range(len(Kx)):
        X = sla.cho_solve(c, Kx[q].T, check_finite=False)
        tol[q] = (4.0 * ur.EPS * nA * np.linalg.norm(X, 2) ** 2 + 2.0 * ur.TAU * np.abs(Kx[q]).max() * np.abs(X).sum(axis=0).max()
                  + ur.TAU * np.abs(kqq[q]).max())
    a = sla.cho_solve(c, y, check_finite=False)
    out = {'A': A, 'nA': nA, 'y': y, 'n3': n3, 'Kx': Kx, 'kqq': kqq, 'Sig': Sig, 'tol': tol, 'scale': float(np.dot(y, a) / y.size)}
    if with_loo:
        r, _, logdet = lr.loo_identity(A, y, n3)
        T = np.array([bounds.terms(j) for j in range(len(A) // n3)])
        out.update({'r': r, 'logdet': logdet, 'loo_tol': T[:, 0] + T[:, 1], 'logdet_tol': bounds.logdet_tol()})
    return out


def _panel(Lkk, Vk):
    """Householder LQ of [Lkk Vk] in place: returns (U, T, sgn).  Lkk becomes the new diagonal block (not yet sign-fixed:
    the caller multiplies its columns by sgn), Vk becomes zero."""
    w = len(Lkk)
    U = np.zeros_like(Vk)
    tau = np.zeros(w)
    for i in range(w):
        x = Vk[i].copy()
        s = float(x @ x)
        alpha = Lkk[i, i]
        if s > 0.0:
            nrm = np.sqrt(alpha * alpha + s)
            beta = -nrm if alpha > 0.0 else nrm
            tau[i] = (beta - alpha) / beta
            U[i] = x / (alpha - beta)
            Lkk[i, i] = beta
            ww = Lkk[i + 1:, i] + Vk[i + 1:] @ U[i]
            Lkk[i + 1:, i] -= tau[i] * ww
            Vk[i + 1:] -= tau[i] * np.outer(ww, U[i])
        Vk[i] = 0.0
    G = U @ U.T
    T = np.zeros((w, w))
    for i in range(w):
        T[i, i] = tau[i]
        T[:i, i] = -tau[i] * (T[:i, :i] @ G[:i, i])
    sgn = np.where(np.diag(Lkk) < 0.0, -1.0, 1.0)
    return U, T, sgn


def remove(L, n3, idx, chunk=64):
    """Factor of A[kept, kept] from the factor L of A after removing the points idx (n3 rows and columns each)."""
    n = len(L)
    gone = np.zeros(n // n3, dtype=bool)
    gone[np.asarray(idx)] = True
    rows = np.repeat(gone, n3)
    Lc = np.ascontiguousarray(L[np.ix_(~rows, ~rows)])
    V = np.ascontiguousarray(L[np.ix_(~rows, rows)])
    n1, m = V.shape
    rem = np.flatnonzero(gone)
    w = min(chunk * n3, WIDTH, m)
    for g in reversed(range((m + w - 1) // w)):
        sl = slice(g * w, min((g + 1) * w, m))
        t0 = g * w // n3
        cstart = (rem[t0] - t0) * n3
        if cstart >= n1:
            continue
        for k in range(cstart // BLOCK * BLOCK, n1, BLOCK):
            e = min(k + BLOCK, n1)
            Lkk, Vk = Lc[k:e, k:e].copy(), V[k:e, sl].copy()
            U, T, sgn = _panel(Lkk, Vk)
            Lc[k:e, k:e] = np.tril(Lkk) * sgn
            V[k:e, sl] = 0.0
            if e < n1:
                X1, X2 = Lc[e:, k:e], V[e:, sl]
                Z = (X1 + X2 @ U.T) @ T
                Lc[e:, k:e] = (X1 - Z) * sgn
                V[e:, sl] = X2 - Z @ U
    assert not V.any()
    return Lc

"""NumPy/SciPy reference of the greedy selection of training points by joint information gain (csrc/select.hip, DESIGN.md
3.5f) and the bounds the GPU values are held to.  Test helper only: the package never imports it, and nothing in it comes from
the code under test.

Conventions are the project's (tests/_uncertainty_ref.py, tests/_loo_ref.py): A = -K + lam I, T the training set.  The
descriptors of T and of the pool come from the oracle, A_U = system_matrix of their UNION; for an index set I of points A_I is
the principal submatrix of A_U.  With S_t the candidates picked before step t,
    gain_t(q) = log det A_{T+S_t+q} - log det A_{T+S_t} - n3 log lam,      log det = 2 sum log diag chol,
step t picks the largest gain, ties to the lowest pool index.  Both determinants share the factor of the leading block
A_{T+S_t}, so their difference is 2 sum log of the trailing n3 diagonal entries of chol(A_{T+S_t+q}) (greedy()); the
second formulation (schur_sweep()) is the block-pivoted Cholesky of the pool's joint posterior covariance that the device code
runs, and full_logdet_gain() the literal difference of two full factorisations (tests/test_select_cpu.py compares the three).

Bound of one gain, the sum of the two log det bounds of _loo_ref.Bounds.logdet_tol:
    tol_t(q) = logdet_tol(A_{T+S_t+q}) + logdet_tol(A_{T+S_t}),   logdet_tol(A) = 4 EPS ||A||_2 tr A^-1 + TAU max|A| sum|A^-1|.
A^-1 of a bordered matrix comes from the inverse of its leading block (block inversion), never from the code under test.

Cap, a condition on the reference alone: at every step gain(best) - gain(second) >= 10 (tol(best) + tol(second)), an exact
duplicate of the best candidate left out as "second" -- otherwise the order of the picks would not be decided by the bounds.
The fixtures stored with lam = 1e-10 do not pass it (cfg0_n9_p6: a bound near 9e2 against gaps below 10), so they run with lam
overridden.  CASES records the value per fixture, chosen on the CPU so that the cap holds, the pool and the number of picks."""
import functools
import os

import numpy as np
import scipy.linalg as sla
import scipy.sparse.linalg as ssl

import _extend_ref as er
import _uncertainty_ref as ur
from oracle import gdml_oracle as orc

TAU = ur.TAU
EPS = ur.EPS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

# the synthetic case of the GLOBAL-scratch score form: n3 = 132 > 128
SYNTH132 = {'N': 44, 'M': 12, 'seed': 3, 'jitter': 0.3, 'sig': 30.0, 'n_test': 6}

# name -> lam (None: the fixture's stored value), number of test geometries in the pool, picks.
# cfg0_n9_p6 and cfg3_n42_p27_m60 need lam = 1e-3: at 1e-4 the smallest cap ratio (gap over the sum of the two bounds; 10 is
# required) is 6.7 on cfg0 (step 3; 0.49 at 1e-5) and 4.2 on cfg3 (step 2; 2.0 at 1e-5), at 1e-3 it is 49.7 and 14.3 --
# n = 5400 and 7560 make sum|A^-1|, hence the bounds, two orders larger than on the small fixtures while the gaps are not.
CASES = {
    'n10_p2_pbc': {'lam': None, 'n_test': 7, 'b': 3},
    'n4_p6_pbc': {'lam': 1e-5, 'n_test': 6, 'b': 3},
    'n5_p4': {'lam': 1e-5, 'n_test': 6, 'b': 4},
    'cfg0_n9_p6': {'lam': 1e-3, 'n_test': 8, 'b': 4},
    'cfg3_n42_p27_m60': {'lam': 1e-3, 'n_test': 6, 'b': 3},
    'synth132': {'lam': 1e-5, 'n_test': 6, 'b': 3},
    'synth': {'lam': None, 'n_test': 6, 'b': 3},
}


def synth132_fixture():
    s = SYNTH132
    ds = orc.synth_dataset(s['N'], s['M'] + s['n_test'], seed=s['seed'], jitter=s['jitter'])
    n = s['M'] + s['n_test']
    R = np.asarray(ds['R'], dtype=np.float64).reshape(n, s['N'], 3)
    F = np.asarray(ds['F'], dtype=np.float64).reshape(n, s['N'], 3)
    E = np.asarray(ds['E'], dtype=np.float64).ravel()
    M = s['M']
    return {'R_train': R[:M], 'F_train': F[:M], 'E_train': E[:M], 'R_test': R[M:], 'F_test': F[M:].reshape(s['n_test'], -1),
            'E_test': E[M:], 'perms': np.arange(s['N'])[None], 'sig': s['sig'], 'lam': 1e-5,
            'model_std': float(np.std(F[:M])), 'model_c': 0.0}


def load(name):
    if name == 'synth':
        return er.synth_fixture()
    if name == 'synth132':
        return synth132_fixture()
    return dict(np.load(os.path.join(GOLDEN, name + '.npz')))


def pool_of(g, n_test):
    """The fixture's first n_test test geometries, a duplicate of pool[0], and the first training geometry."""
    Rt = np.asarray(g['R_test'], dtype=np.float64)
    Rt = Rt.reshape(len(Rt), -1)
    assert len(Rt) >= n_test
    return np.ascontiguousarray(np.concatenate([Rt[:n_test], Rt[:1], np.asarray(g['R_train'], dtype=np.float64)[:1].reshape(1, -1)]))


def duplicate_case():
    """The pool of the issue's CPU observation: n10_p2_pbc at its stored lam, R_test[:7] + [R_test[0], R_train[0]], b = 3."""
    return 'n10_p2_pbc'


def logdet_tol_parts(nA, maxA, tr_inv, sumabs_inv):
    return 4.0 * EPS * nA * tr_inv + TAU * maxA * sumabs_inv


def _norm2_sub(A_U, sub):
    """||A_sub||_2 of the principal submatrix on the indices `sub` (symmetric positive definite: its largest eigenvalue), by
    Lanczos on the union matrix with the other entries held at zero -- no copy of the submatrix, no O(n^3) reduction."""
    if len(sub) < 64:
        return float(sla.eigvalsh(A_U[np.ix_(sub, sub)])[-1])
    buf = np.zeros(len(A_U))

    def mv(v):
        buf[:] = 0.0
        buf[sub] = np.ravel(v)
        return (A_U @ buf)[sub]

    op = ssl.LinearOperator((len(sub), len(sub)), matvec=mv, dtype=np.float64)
    return float(ssl.eigsh(op, k=1, which='LA', tol=1e-10, v0=np.ones(len(sub)))[0][0])


class Sweep(object):
    """State of the greedy loop on the union matrix A_U: the factor and the inverse of A_{T+S_t}, grown by bordering."""

    def __init__(self, A_U, nT, n3):
        self.A, self.n3, self.nT = A_U, n3, nT
        self.idx = np.arange(nT)
        self.L = sla.cholesky(A_U[:nT, :nT], lower=True, check_finite=False)
        self.inv = sla.cho_solve((self.L, True), np.eye(nT), check_finite=False)
        self.maxTT = float(np.abs(A_U[:nT, :nT]).max())
        self.base_tol = self._tol_of(self.idx, np.trace(self.inv), np.abs(self.inv).sum())

    def _tol_of(self, sub, tr_inv, sumabs_inv):
        extra = sub[self.nT:]  # max|A_sub|: the training block, and the rows of the appended points (A is symmetric)
        maxA = max(self.maxTT, float(np.abs(self.A[np.ix_(extra, sub)]).max())) if len(extra) else self.maxTT
        return logdet_tol_parts(_norm2_sub(self.A, sub), maxA, tr_inv, sumabs_inv)

    def blk(self, q, nT):
        return np.arange(nT + q * self.n3, nT + (q + 1) * self.n3)

    def border(self, rows):
        """(gain + n3 log lam, logdet_tol of the bordered matrix, pieces for commit) for the rows `rows` of A_U appended."""
        A, base = self.A, self.idx
        C = A[np.ix_(rows, base)]
        D = A[np.ix_(rows, rows)]
        W = sla.solve_triangular(self.L, C.T, lower=True, check_finite=False).T
        LS = sla.cholesky(D - W @ W.T, lower=True, check_finite=False)
        ld = 2.0 * np.sum(np.log(np.diag(LS)))
        # inverse of the bordered matrix by blocks: X = B^-1 C^T, S = D - C X
        X = self.inv @ C.T
        Sinv = sla.cho_solve((LS, True), np.eye(len(rows)), check_finite=False)
        XS = X @ Sinv
        # trace and sum of moduli of the leading block B^-1 + X S^-1 X^T in row slabs (the block itself is formed at a commit only)
        tr_inv, sumabs = np.trace(Sinv), 2.0 * np.abs(XS).sum() + np.abs(Sinv).sum()
        for i in range(0, len(base), 512):
            slab = self.inv[i:i + 512] + XS[i:i + 512] @ X.T
            tr_inv += np.trace(slab[:, i:i + 512])
            sumabs += np.abs(slab).sum()
        tol = self._tol_of(np.concatenate([base, rows]), tr_inv, sumabs)
        return ld, tol, (W, LS, X, XS, Sinv)

    def commit(self, rows, pieces, tol):
        W, LS, X, XS, Sinv = pieces
        top = self.inv + XS @ X.T
        n, m = len(self.idx), len(rows)
        L = np.zeros((n + m, n + m))
        L[:n, :n], L[n:, :n], L[n:, n:] = self.L, W, LS
        inv = np.empty((n + m, n + m))
        inv[:n, :n], inv[:n, n:], inv[n:, :n], inv[n:, n:] = top, -XS, -XS.T, Sinv
        self.L, self.inv, self.idx, self.base_tol = L, inv, np.concatenate([self.idx, rows]), tol


def greedy(A_U, nT, n3, B, b, lam, dup_of=None):
    """The greedy loop by log det differences.  Returns a dict: idx (b,), gain (b,), tol (b,), gain0 (B,), tol0 (B,), per step
    the gains and bounds of every remaining candidate ('steps': list of {q: (gain, tol)}), and the cap's ratios
    (gap / (tol(best) + tol(second)), None where every other candidate is an exact duplicate of the best), and logdet_tol of
    A_T ('tol_T') and of A_{T+S_b} ('tol_final')."""
    sw = Sweep(A_U, nT, n3)
    tol_T = sw.base_tol
    shift = n3 * np.log(lam)
    picked, idx, gains, tols, steps, cap = [], [], [], [], [], []
    for t in range(b):
        cur, keep = {}, {}
        for q in range(B):
            if q in picked:
                continue
            ld, tol_sub, pieces = sw.border(sw.blk(q, nT))
            cur[q] = (ld - shift, tol_sub + sw.base_tol)
            keep[q] = (pieces, tol_sub)
        best = max(cur, key=lambda q: (cur[q][0], -q))  # ties: the lowest index
        others = [q for q in cur if q != best and not (dup_of is not None and dup_of(q, best))]
        if others:
            second = max(others, key=lambda q: cur[q][0])
            cap.append((cur[best][0] - cur[second][0]) / (cur[best][1] + cur[second][1]))
        else:
            cap.append(None)
        steps.append(cur)
        idx.append(best)
        gains.append(cur[best][0])
        tols.append(cur[best][1])
        picked.append(best)
        sw.commit(sw.blk(best, nT), keep[best][0], keep[best][1])
    return {'idx': np.array(idx), 'gain': np.array(gains), 'tol': np.array(tols), 'gain0': np.array([steps[0][q][0] for q in range(B)]),
            'tol0': np.array([steps[0][q][1] for q in range(B)]), 'steps': steps, 'cap': cap,
            'tol_T': tol_T, 'tol_final': sw.base_tol}


def schur_sweep(A_U, nT, n3, B, b, lam):
    """The second formulation: Sig = D_pool - C A_TT^-1 C^T (the pool's joint posterior covariance + lam I on its diagonal
    blocks), then b steps of block-pivoted Cholesky with the lazily updated diagonal blocks.  Returns (idx, gain, gain0)."""
    L = sla.cholesky(A_U[:nT, :nT], lower=True, check_finite=False)
    W = sla.solve_triangular(L, A_U[nT:, :nT].T, lower=True, check_finite=False).T
    P = A_U[nT:, nT:] - W @ W.T  # = Sig_joint + lam I
    blocks = [P[q * n3:(q + 1) * n3, q * n3:(q + 1) * n3].copy() for q in range(B)]
    shift = n3 * np.log(lam)
    Vs, idx, gains, gain0 = [], [], [], None
    for t in range(b):
        g = np.full(B, -np.inf)
        for q in range(B):
            if q not in idx:
                g[q] = 2.0 * np.sum(np.log(np.diag(sla.cholesky(blocks[q], lower=True, check_finite=False)))) - shift
        if t == 0:
            gain0 = g.copy()
        best = int(np.argmax(g))  # the first of equal maxima
        idx.append(best)
        gains.append(g[best])
        sl = slice(best * n3, (best + 1) * n3)
        C = P[:, sl].copy()
        for V in Vs:
            C -= V @ V[sl].T
        G = sla.cholesky(blocks[best], lower=True, check_finite=False)
        V = sla.solve_triangular(G, C.T, lower=True, check_finite=False).T
        Vs.append(V)
        for q in range(B):
            Vq = V[q * n3:(q + 1) * n3]
            blocks[q] = blocks[q] - Vq @ Vq.T
    return np.array(idx), np.array(gains), gain0


def full_logdet_gain(A_U, nT, n3, S, q, lam):
    """gain of candidate q given the picked candidates S, literally: two full factorisations over index subsets."""
    def ld(cands):
        I = np.concatenate([np.arange(nT)] + [np.arange(nT + c * n3, nT + (c + 1) * n3) for c in cands]).astype(int)
        return 2.0 * np.sum(np.log(np.diag(sla.cholesky(A_U[np.ix_(I, I)], lower=True, check_finite=False))))
    return ld(list(S) + [q]) - ld(list(S)) - n3 * np.log(lam)


@functools.lru_cache(maxsize=None)
def case(name):
    """Everything of one case, computed once per session: the fixture's tables at the case's lam, the pool, the union matrix
    and the reference sweep."""
    c = CASES[name]
    g = load(name)
    if c['lam'] is not None:
        g['lam'] = c['lam']
    t = er.tables(g)
    pool = pool_of(g, c['n_test'])
    B, n3 = len(pool), t['R'].shape[1]
    x_all, gd_all = orc.desc_from_R(np.concatenate([t['R'], pool]), t['lat'])
    A_U = ur.system_matrix(x_all, gd_all, t['tp'], t['sig'], t['lam'])
    nT = len(t['R']) * n3

    def dup_of(a, b_):
        return np.array_equal(pool[a], pool[b_])

    ref = greedy(A_U, nT, n3, B, c['b'], t['lam'], dup_of)
    return {'g': g, 't': t, 'pool': pool, 'B': B, 'b': c['b'], 'n3': n3, 'nT': nT, 'lam': t['lam'], 'A_U': A_U, 'ref': ref,
            'dup': c['n_test'], 'train0': c['n_test'] + 1}

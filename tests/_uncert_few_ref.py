"""NumPy restatement of the few-row forward solve of csrc/uncert_few.hip: the same block sizes and the same
order of operations, so that what the inverted 64 x 64 diagonal blocks cost in accuracy shows without a GPU.  Test helper only.

    Z = X L^-T for r rows X (r, n) and the lower Cholesky factor L (n, n):
      1. every 64 x 64 diagonal block of L (the last one completed by an identity) is inverted by forward substitution,
         column by column, sums over k ascending;
      2. steps of W = 256 columns.  Diagonal part of a step, per 64-column sub-block jb in ascending order:
             X_jb <- X_jb inv(L_jb,jb)^T
             X_kb <- X_kb - X_jb L[kb, jb]^T      for the later sub-blocks kb of the step
         then the trailing update X[:, c] <- X[:, c] - X_step L[c, step]^T for every column c right of the step.
"""
import numpy as np

W = 256   # step width of few_diag_kernel / few_update_kernel
SB = 64   # sub-block whose diagonal block is inverted
LIMIT = 256  # rows the kernels take (GDML_COV_FEW_ROWS)


def invert_diag_blocks(L):
    """inv(L_bb) of every 64 x 64 diagonal block b, the last one padded by an identity: (nb, 64, 64)."""
    n = L.shape[0]
    nb = (n + SB - 1) // SB
    out = np.zeros((nb, SB, SB))
    for b in range(nb):
        D = np.eye(SB)
        w = min(SB, n - b * SB)
        D[:w, :w] = np.tril(L[b * SB:b * SB + w, b * SB:b * SB + w])
        Y = np.zeros((SB, SB))
        eye = np.eye(SB)
        for i in range(SB):  # row i of every column's substitution at once
            Y[i] = (eye[i] - D[i, :i] @ Y[:i]) / D[i, i]
        out[b] = Y
    return out


def few_solve(L, X):
    """Z = X L^-T by the blocked scheme above; X (r, n)."""
    n = L.shape[0]
    Z = np.array(X, dtype=np.float64)
    inv = invert_diag_blocks(L)
    for c0 in range(0, n, W):
        c1 = min(n, c0 + W)
        for j0 in range(c0, c1, SB):
            j1 = min(c1, j0 + SB)
            Z[:, j0:j1] = Z[:, j0:j1] @ inv[j0 // SB][:j1 - j0, :j1 - j0].T
            if j1 < c1:
                Z[:, j1:c1] -= Z[:, j0:j1] @ L[j1:c1, j0:j1].T
        if c1 < n:
            Z[:, c1:] -= Z[:, c0:c1] @ L[c1:, c0:c1].T
    return Z


def posterior_cov_few(Kx, kqq, L):
    """Sig_q (B,3N,3N) = -k_qq - Z_q Z_q^T with Z_q from few_solve, every query on its own."""
    out = np.empty_like(kqq)
    for q in range(Kx.shape[0]):
        Z = few_solve(L, -Kx[q])
        out[q] = -0.5 * (kqq[q] + kqq[q].T) - Z @ Z.T
    return out

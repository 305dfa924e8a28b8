"""Helper and references of the Nystroem edge tests (tests/test_nys_edges_cpu.py, tests/test_nys_edges_gpu.py,
tools/nys_edges_parity.py): plain NumPy / SciPy, no GPU import at module level.  Test helper only: the package never
imports it.  It builds on tests/_chol_ref.py (reachable, _dummy_set, gamma, U, spd).

The code under test is csrc/nystroem.hip (on gram_tn.hip and tall_trsm of chol_solve.hip): gdml_nystroem_factor
(K_mm = -K_nm[idx] + eps I = L_mm L_mm^T; X1 = K_nm L_mm^-T; X1^T X1 + lam I = L L^T; X2 = X1 L^-T) and
gdml_nystroem_lev_scores (row sums of X2^2), and csrc/precon_apply.hip: gdml_precon_apply
(P v = (X2 X2^T v - v) / lam in three forms).  The tests want THEIR matrix at THEIR shape: load_nystroem uploads a dummy
training set of n rows, lets the library allocate the (n + m) x m buffer and overwrites it.

Stage checks (u = 2^-53, gamma_k = k u / (1 - k u); derived, componentwise, valid for any order of summation; every stage
reads its inputs back from the device, so no conditioning enters; residuals are evaluated in long double):
  S1  Gram + second Cholesky   |X1^T X1 + lam I - L L^T| <= gamma_{n+1} |X1|^T |X1| + 2 gamma_{m+1} |L||L^T|   (lower triangle)
      an inner product of n terms and the addition of lam, then Higham's Theorem 10.3 for the factor, doubled for the
      Newton reciprocal square root as in _chol_ref.py
  S2  second solve             |X2 L^T - X1| <= gamma_{m+1} |X2| |L^T|
      substitution with at most m terms per entry and a multiplication by a reciprocal pivot
  S3  leverage scores          |lev - sum_c X2^2| <= gamma_m sum_c X2^2   per row
  S4  fp64 application         |out - (X2 (X2^T v) - v) / lam| <= [gamma_{m+1} |X2||t| + gamma_{n+1} |X2| (|X2|^T |v|)
                                                                   + 2 u (|s| + |v|)] / lam,   t = X2^T v, s = X2 t
      the two inner products, the subtraction and the multiplication by 1 / lam (itself rounded)
  S5  rounding                 bit comparisons of the in-place fp32 overlay with the separate fp32 copy
Measured checks (no simple derived bound): M1 form-0 application, M2 form 3, M3 the CholeskyQR branch, M4 the first solve,
M5 the matrix-free form, each against the long-double reference, error relative to max |reference|.  The allowance of a
case is 10 x the largest error that the float64 restatement of these files (nys_f64, f32_form_f64, ...) makes against the same
reference over three seeds of the matrix and of v: restatement and kernel perform the same roundings in another order,
the seeds sample the spread between orders, 10 sits an order of magnitude above that spread.  No allowance is ever sized
from the device's output.
"""
import ctypes as C
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import scipy.linalg as sla

from _chol_ref import U, _dummy_set, gamma, spd  # noqa: F401  (reachable is wrapped below)
import _chol_ref as cr

LD = np.longdouble
EPS = 2.220446049250313e-16  # the pre-regularisation of K_mm (cho_factor_stable_dev, pre_reg = true)
TT, TBK = 128, 16            # Gram tile and k-tile of csrc/gram_tn.hip (precon_plan.h)
SEEDS = (0, 1, 2)
_POOL = ThreadPoolExecutor(8)


def round16(m):
    return (int(m) + 15) // 16 * 16


def reachable(n):
    """_chol_ref.reachable with a preference for a training set WITHOUT energy constraints where one exists."""
    n = int(n)
    for N in range(2, 7):
        if n >= 3 * N and n % (3 * N) == 0:
            return N, False, n // (3 * N)
    return cr.reachable(n)


# ------------------------------------------------------------------ test matrices

def spd6(n, seed):
    """Family 'b'-style: Q diag(s) Q^T with s log-spaced over 6 decades."""
    rs = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rs.normal(size=(n, n)))
    A = (Q * np.logspace(-6.0, 0.0, n)) @ Q.T
    return 0.5 * (A + A.T)


@functools.lru_cache(maxsize=8)
def case_matrix(n, m, family='a', seed=0):
    """(K_nm, idx): K_nm = -A[:, idx], A symmetric positive definite of order n, idx a sorted seeded sample of m columns, so
    that K_mm = -K_nm[idx] is symmetric positive definite.  Family 'a': _chol_ref.spd('a') (condition number ~ 10); beyond
    n = 4096, where that n x (n + 20) product is too slow for a test, the same form with an n x (m + 20) factor
    (B B^T / (m + 20) + 0.5 I restricted to the columns: condition number of order n / m).  Family 'b': K_mm = spd6(m)."""
    s = 1000 + n + 7919 * seed
    rs = np.random.RandomState(5000 + 31 * n + m + 104729 * seed)
    idx = np.sort(rs.choice(n, m, replace=False)).astype(np.int64)
    if family == 'b':
        # a principal submatrix of spd6(n) is far better conditioned than spd6(n) (interlacing: 2e2 at m = 130 of 594), so the
        # six decades are put where the factorisations see them: A = [[B, B G], [G^T B, G^T B G + D]] on (idx, the rest) with
        # B = spd6(m) and any D > 0 is positive definite, K_mm = B, and X1^T X1 = L_mm^T (I + G G^T) L_mm spans them too
        B = spd6(m, s)
        G = rs.normal(size=(m, n - m)) / np.sqrt(m)
        K = np.empty((n, m))
        K[idx] = -B
        K[np.setdiff1d(np.arange(n), idx)] = -(G.T @ B)
    elif n <= 4096:
        A = spd('a', n, seed=s)
        A = 0.5 * (A + A.T)
        K = -A[:, idx]
    else:
        B = np.random.RandomState(s).normal(size=(n, m + 20))
        K = -(B @ B[idx].T) / (m + 20)
        K[idx, np.arange(m)] -= 0.5
        K[idx] = 0.5 * (K[idx] + K[idx].T)
    K = np.ascontiguousarray(K)
    K.setflags(write=False)
    idx.setflags(write=False)
    return K, idx


def vec(n, seed=0):
    return np.random.RandomState(77 + n + 15485863 * seed).normal(size=n)


# ------------------------------------------------------------------ long-double primitives, written out plainly

def _row_blocks(n, k=8):
    return [(b[0], b[-1] + 1) for b in np.array_split(np.arange(n), k) if len(b)]


def mm_ld(A, B):
    """A @ B on long doubles (NumPy has no BLAS for them); row blocks of A on a few threads, each a plain np.dot."""
    A = np.ascontiguousarray(A, dtype=LD)
    B = np.ascontiguousarray(B, dtype=LD)
    if B.ndim == 1 or A.shape[0] * B.shape[1] < 4096:
        return np.dot(A, B)
    out = np.empty((A.shape[0], B.shape[1]), dtype=LD)

    def f(r):
        out[r[0]:r[1]] = np.dot(A[r[0]:r[1]], B)

    list(_POOL.map(f, _row_blocks(A.shape[0])))
    return out


def chol_ld(A):
    """Lower Cholesky factor, column by column; reads the lower triangle of A."""
    A = np.asarray(A, dtype=LD)
    m = len(A)
    L = np.zeros((m, m), dtype=LD)
    for j in range(m):
        c = A[j:, j] - np.dot(L[j:, :j], L[j, :j])
        if not c[0] > 0:
            raise np.linalg.LinAlgError('not positive definite at %d' % j)
        L[j:, j] = c / np.sqrt(c[0])
    return L


def trsm_ld(X, L):
    """X L^-T for the rows of X: substitution column by column (row blocks on a few threads)."""
    X = np.asarray(X, dtype=LD)
    L = np.asarray(L, dtype=LD)
    m = L.shape[0]
    out = np.empty_like(X)

    def f(r):
        Y = out[r[0]:r[1]]
        Xr = X[r[0]:r[1]]
        for j in range(m):
            Y[:, j] = (Xr[:, j] - np.dot(Y[:, :j], L[j, :j])) / L[j, j]

    list(_POOL.map(f, _row_blocks(len(X))))
    return out


def sym_from_lower(A):
    A = np.tril(A)
    return A + np.tril(A, -1).T


def nys_ld(K_nm, idx, lam, upto='X2'):
    """(L_mm, X1, L, X2) of the Nystroem factor in long double (upto='X1': the first two only, the rest None)."""
    assert np.finfo(LD).eps < 1e-18, 'no extended precision on this host'
    K = np.asarray(K_nm, dtype=LD)
    m = len(idx)
    K_mm = sym_from_lower(-K[np.asarray(idx)]) + LD(EPS) * np.eye(m, dtype=LD)
    L_mm = chol_ld(K_mm)
    X1 = trsm_ld(K, L_mm)
    if upto == 'X1':
        return L_mm, X1, None, None
    inner = mm_ld(X1.T, X1) + LD(lam) * np.eye(m, dtype=LD)
    L = chol_ld(inner)
    return L_mm, X1, L, trsm_ld(X1, L)


def precon_ld(X2, lam, v):
    v = np.asarray(v, dtype=LD)
    return (np.dot(X2, np.dot(X2.T, v)) - v) / LD(lam)


def f32_form_ld(X2, L, lam):
    """The definition above build_f32_form (csrc/nystroem.hip): X32 = float32(X2); G0 = I - lam L^-1 L^-T; M0 = L0^T L0 with
    L0 L0^T = G0; G = X32^T X32 = L_G L_G^T; T0 = L_G^-T M0 L_G^-1.  Returns (X32 as long double, T0)."""
    m = L.shape[0]
    I = np.eye(m, dtype=LD)
    X32 = np.asarray(X2, dtype=np.float64).astype(np.float32).astype(LD)
    R = trsm_ld(I, L)                      # L^-T
    G0 = I - LD(lam) * mm_ld(R.T, R)       # I - lam L^-1 L^-T
    L0 = chol_ld(G0)
    M0 = mm_ld(L0.T, L0)
    L_G = chol_ld(mm_ld(X32.T, X32))
    Zt = trsm_ld(I, L_G)                   # L_G^-T
    return X32, mm_ld(mm_ld(Zt, M0), Zt.T)


def precon_f32_ld(X32, T0, lam, v):
    """P3 v = (X32 T0 X32^T v - v) / lam."""
    v = np.asarray(v, dtype=LD)
    return (np.dot(X32, np.dot(T0, np.dot(X32.T, v))) - v) / LD(lam)


# ------------------------------------------------------------------ the host's branch arithmetic, restated
# (written from the inline code before csrc/precon_plan.h existed; tests/test_precon_plan_cpu.py holds the header to it)

def gram_plan(n, m, split=1, ldc=None):
    """gram_tn + syrk_tn_kernel: the lower tiles with FULL / ragged per tile (buffers are 16-byte aligned and the pitch is
    even, so a tile is FULL exactly when it lies inside m), the split count S and the row ranges."""
    ldc = round16(m) if ldc is None else ldc
    tiles = (m + TT - 1) // TT
    T = tiles * (tiles + 1) // 2
    S = 1
    if split and T < 8192:
        S = min((8192 + T - 1) // T, 8)
        while S > 1 and n // S < 8192:
            S -= 1
        while S > 1 and S * m * ldc * 8 > (2 << 30):
            S -= 1
    full = {(ti, tj): (ti * TT + TT <= m and tj * TT + TT <= m) for ti in range(tiles) for tj in range(ti + 1)}
    rows_per = n if S == 1 else ((n + S - 1) // S + TBK - 1) // TBK * TBK
    ranges = [(s * rows_per, max(s * rows_per, min(n, (s + 1) * rows_per))) for s in range(S)]
    return dict(tiles=tiles, T=T, full=full, S=S, rows_per=rows_per, ranges=ranges,
                whole_k_tiles=[(b - a) // TBK for a, b in ranges], k_tail=[(b - a) % TBK for a, b in ranges])


def trsm_plan(m, left=1):
    """tall_trsm: per 512-column strip (k0, nb, branch, widths of the trsm64 steps, update before ('left'), update after
    ('right')); ld is a multiple of 16 and the buffers are aligned, so the panel branch is taken exactly when nb % 64 == 0."""
    out = []
    for k0 in range(0, m, 512):
        nb = min(512, m - k0)
        panel = nb % 64 == 0
        widths = [] if panel else [min(64, nb - jj) for jj in range(0, nb, 64)]
        out.append(dict(k0=k0, nb=nb, branch='panel' if panel else 'trsm64', widths=widths,
                        left_update=bool(left and k0 > 0), right_update=bool(not left and k0 + nb < m)))
    return out


def apply_plan(n, m, form, f32_rows_per=1024, f32_rw=4):
    """precon_apply_device: row parts of X^T v with the unroll remainder of each, column blocks, remainders of X t."""
    if form == 0:
        rows_per, cols_per_block = 2048, 512
    else:
        rows_per, cols_per_block = max(int(f32_rows_per), 64), 1024
    nparts = max((n + rows_per - 1) // rows_per, 1)
    parts = [min(n, (p + 1) * rows_per) - p * rows_per for p in range(nparts)]
    d = dict(nparts=nparts, parts=parts, rem8=[p % 8 for p in parts], col_blocks=(m + cols_per_block - 1) // cols_per_block)
    # the column loops of X t, walked lane by lane: iterations of the unrolled loop and of the tail loop over the wavefront
    per, width, mm = (2, 128, m & ~1) if form == 0 else (4, 256, (m + 3) & ~3)
    unrolled = tail = 0
    for lane in range(64):
        c = per * lane
        while c + (3 * width if form == 0 else width) < mm:
            unrolled += 1
            c += (4 if form == 0 else 2) * width
        while c < mm:
            tail += 1
            c += width
    d.update(unrolled=unrolled, tail=tail)
    if form == 0:
        d.update(odd_col=m % 2, threads_in_last_block=((m - (d['col_blocks'] - 1) * 512) + 1) // 2)
    else:
        rw = 4 if f32_rw >= 4 else (2 if f32_rw >= 2 else 1)
        d.update(rw=rw, mod4=m % 4, rem_rows=n % (4 * rw), rem_rw=n % rw)
    return d


# ------------------------------------------------------------------ float64 restatements of nystroem.hip / precon_apply.hip (defects on request)

def _trsm_f64(X, L, defect=None):
    """tall_trsm.  defect 'trsm_last_block': the last, ragged 64-block receives its updates but is never solved."""
    m = L.shape[0]
    if defect == 'trsm_last_block' and m % 64:
        c0 = m // 64 * 64
        Y = np.empty_like(X)
        if c0:
            Y[:, :c0] = sla.solve_triangular(L[:c0, :c0], X[:, :c0].T, lower=True, check_finite=False).T
        Y[:, c0:] = X[:, c0:] - Y[:, :c0] @ L[c0:, :c0].T
        return Y
    return np.ascontiguousarray(sla.solve_triangular(L, X.T, lower=True, check_finite=False).T)


def _gram_f64(X, defect=None):
    """gram_tn.  defects: 'gram_tail16' the last n % 16 rows are not summed; 'gram_split2' the second row range of the split
    is not summed."""
    n, m = X.shape
    if defect == 'gram_tail16':
        X = X[:n - n % TBK]
    elif defect == 'gram_split2':
        p = gram_plan(n, m)
        assert p['S'] >= 2
        X = np.concatenate([X[a:b] for k, (a, b) in enumerate(p['ranges']) if k != 1])
    return X.T @ X


def nys_f64(K_nm, idx, lam, force_qr=False, defect=None):
    """gdml_nystroem_factor in float64, statement for statement.  Returns dict(L_mm, X1, L, X2, info)."""
    K = np.asarray(K_nm, dtype=np.float64)
    n, m = K.shape
    K_mm = sym_from_lower(-K[np.asarray(idx)])
    K_mm[np.diag_indices(m)] += EPS
    L_mm = np.linalg.cholesky(K_mm)  # raises where the device would climb the jitter ladder
    X1 = _trsm_f64(K, L_mm, defect)
    inner = _gram_f64(X1, defect)
    inner[np.diag_indices(m)] += lam
    L = np.linalg.cholesky(inner)
    if not force_qr:
        return dict(L_mm=L_mm, X1=X1, L=L, X2=_trsm_f64(X1, L, defect), info=0)
    # shifted CholeskyQR3 on [X1; sqrt(lam) I]
    X = np.vstack([X1, np.sqrt(lam) * np.eye(m)])
    for p in range(3):
        G = X.T @ X
        if p == 0:
            tr = 0.0
            for d in np.diag(G):
                tr += d
            G[np.diag_indices(m)] += 11.0 * (m * float(n + m) + m * (m + 1.0)) * EPS * tr
        X = _trsm_f64(X, np.linalg.cholesky(G))
    return dict(L_mm=L_mm, X1=X1, L=L, X2=np.ascontiguousarray(X[:n]), info=1)


def precon_f64(X2, lam, v, defect=None):
    """precon_apply_device, form 0.  defects: 'gemv_t_tail8' the last rows % 8 rows of every part are not summed into
    X^T v; 'gemv_t_oddcol' / 'gemv_n_oddcol' the odd last column is missing from X^T v / from X t."""
    n, m = X2.shape
    t = np.zeros(m)
    for r0 in range(0, n, 2048):
        r1 = min(n, r0 + 2048)
        if defect == 'gemv_t_tail8':
            r1 -= (r1 - r0) % 8
        t += X2[r0:r1].T @ v[r0:r1]
    if defect == 'gemv_t_oddcol' and m % 2:
        t[m - 1] = 0.0
    mc = m - 1 if (defect == 'gemv_n_oddcol' and m % 2) else m
    return (X2[:, :mc] @ t[:mc] - v) * (1.0 / lam)


def _kahan_rows(X, v):
    """sum_r X[r] v[r] with Kahan's compensation, vectorised over the columns."""
    s = np.zeros(X.shape[1])
    c = np.zeros(X.shape[1])
    for r in range(X.shape[0]):
        y = X[r] * v[r] - c
        t = s + y
        c = (t - s) - y
        s = t
    return s


def f32_form_f64(X2, L, lam, gram_rows=2048, defect=None):
    """build_f32_form in float64: (X32 float32, T0, smallest squared pivot of L_G).  The same formation order for T0
    (G0 + W1 + W1^T + W1 E_z^T), a Kahan sum over the chunk Gram matrices.  defects: 'gram_kahan_chunk' the last, ragged
    chunk is not summed; 'T0_L0L0T' M0 is taken as G0 = L0 L0^T.  'no_kahan' (plain chunk sum) is NOT a defect."""
    n, m = X2.shape
    I = np.eye(m)
    Rb = _trsm_f64(I, L) * np.sqrt(lam)
    G0 = I - Rb.T @ Rb
    X32 = X2.astype(np.float32)
    chunk = 256 if gram_rows < 256 else int(gram_rows) // 16 * 16
    chunk = min(chunk, n)
    G = np.zeros((m, m))
    Gc = np.zeros((m, m))
    for r0 in range(0, n, chunk):
        rows = min(chunk, n - r0)
        if defect == 'gram_kahan_chunk' and rows < chunk:
            continue
        D = X32[r0:r0 + rows].astype(np.float64)
        Gp = D.T @ D
        if r0 == 0 or defect == 'no_kahan':
            G = G + Gp
        else:
            y = Gp - Gc
            t = G + y
            Gc = (t - G) - y
            G = t
    L_G = np.linalg.cholesky(G)
    piv = float(np.diag(L_G).min() ** 2)
    if defect != 'T0_L0L0T':
        Cm = I - np.linalg.cholesky(G0)
        G0 = G0 + (Cm.T @ Cm - Cm @ Cm.T)  # M0
    Ez = _trsm_f64(I, L_G) - I
    H = -(Ez @ G0.T)
    S = -(H @ Ez.T)
    return X32, ((G0 - H) - H.T) + S, piv


def precon_f32_f64(X32, T0, lam, v, rows_per=1024, rw=4, defect=None):
    """precon_apply_device, form 3.  defects: 'gemv_t_f32_mod4' the last m % 4 columns are missing from X32^T v;
    'gemv_n_tail' the last n % (4 rw) rows of X32 u are missing."""
    n, m = X32.shape
    X = X32.astype(np.float64)
    rows_per = max(int(rows_per), 64)
    parts = [_kahan_rows(X[r0:r0 + rows_per], v[r0:r0 + rows_per]) for r0 in range(0, n, rows_per)]
    t = _kahan_rows(np.array(parts), np.ones(len(parts)))
    if defect == 'gemv_t_f32_mod4' and m % 4:
        t[m - m % 4:] = 0.0
    s = X @ (T0 @ t)
    if defect == 'gemv_n_tail' and n % (4 * rw):
        s[n - n % (4 * rw):] = 0.0
    return (s - v) * (1.0 / lam)


def mf_f64(K_nm, idx, lam, Kv, v):
    """precon_apply_mf in float64: Z = L_mm^-T L^-T built by the solves X receives; (K_nm Z Z^T K_mn v - v) / lam with
    K_mn v = (K v)[idx] (Kv: the kernel mat-vec, a function) and K_nm t = K e, e the scatter of t."""
    r = nys_f64(K_nm, idx, lam)
    m = len(idx)
    Z = _trsm_f64(_trsm_f64(np.eye(m), r['L_mm']), r['L'])
    t = Z @ (Z.T @ Kv(v)[idx])
    e = np.zeros(len(v))
    e[idx] = t
    return (Kv(e) - v) * (1.0 / lam)


# ------------------------------------------------------------------ stage checks (ratios error / bound)

def _ratio(err, bound):
    err = np.asarray(err, dtype=LD)
    bound = np.asarray(bound, dtype=LD)
    if not np.isfinite(err.astype(np.float64)).all():
        return float('inf')
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(err == 0, LD(0), err / bound)
    return float(q.max()) if q.size else 0.0


def s1_ratio(X1, L, lam):
    n, m = X1.shape
    X = np.asarray(X1, dtype=LD)
    Ll = np.tril(np.asarray(L, dtype=LD))
    res = np.abs(mm_ld(X.T, X) + LD(lam) * np.eye(m, dtype=LD) - mm_ld(Ll, Ll.T))
    aX, aL = np.abs(np.asarray(X1, dtype=np.float64)), np.abs(np.tril(np.asarray(L, dtype=np.float64)))
    bound = gamma(n + 1) * (aX.T @ aX) + 2.0 * gamma(m + 1) * (aL @ aL.T)
    low = np.tril(np.ones((m, m), dtype=bool))
    return _ratio(res[low], bound[low])


def s2_ratio(X1, L, X2):
    m = L.shape[0]
    Ll = np.tril(np.asarray(L, dtype=LD))
    res = np.abs(mm_ld(np.asarray(X2, dtype=LD), Ll.T) - np.asarray(X1, dtype=LD))
    bound = gamma(m + 1) * (np.abs(X2) @ np.abs(np.tril(L)).T)
    return _ratio(res, bound)


def s3_ratio(X2, lev):
    m = X2.shape[1]
    X = np.asarray(X2, dtype=LD)
    ref = (X * X).sum(axis=1)
    return _ratio(np.abs(np.asarray(lev, dtype=LD) - ref), gamma(m) * ref)


def s4_ratio(X2, lam, v, out):
    n, m = X2.shape
    X = np.asarray(X2, dtype=LD)
    vl = np.asarray(v, dtype=LD)
    t = np.dot(X.T, vl)
    s = np.dot(X, t)
    ref = (s - vl) / LD(lam)
    aX = np.abs(X)
    bound = (gamma(m + 1) * np.dot(aX, np.abs(t)) + gamma(n + 1) * np.dot(aX, np.dot(aX.T, np.abs(vl)))
             + 2.0 * U * (np.abs(s) + np.abs(vl))) / LD(lam)
    return _ratio(np.abs(np.asarray(out, dtype=LD) - ref), bound)


def rel_err(x, ref):
    """max |x - ref| / max |ref| (the error of the measured checks)."""
    x = np.asarray(x)
    if not np.isfinite(x.astype(np.float64)).all():
        return float('inf')
    ref = np.asarray(ref, dtype=LD)
    return float(np.abs(np.asarray(x, dtype=LD) - ref).max() / np.abs(ref).max())


# ------------------------------------------------------------------ the grid (shared by the CPU and the GPU module)

LAM = 0.1
SOLVE_N = 594       # n % 16 = 2
F32_N = 594         # 594 % 8 = 2, % 16 = 2; 256-row Gram chunks 256, 256, 82; 64-row parts: 10, the last 18 rows
GRAM_TILES = ((12, 5), (63, 5), (144, 127), (144, 128), (150, 129), (270, 257))
GRAM_SPLIT = (16392, 129)
SOLVE_M = (63, 64, 65, 128, 512, 513, 525, 576)
SOLVE_SMALL = ((12, 1), (12, 2))
# (594, 525): at m = 513 the even part is 512 columns = exactly one round of the 4 x 128 unroll, so the 128-stride tail loop
# of gemv_n_precon_kernel does not run there; 525 has the unroll, the tail loop and the odd column together
GEMV64 = ((2100, 131), (594, 513), (594, 512), (594, 525), (63, 2), (13, 1))
F32_M = (129, 130, 131, 132, 525)
# (options of the build, options of the application) of the fp32 form; every build runs with pcg.f32_inplace 0 and 1
F32_BUILDS = ({}, {'pcg.f32_gram_rows': 256})
F32_APPLY = ({}, {'pcg.f32_rows_per': 64}, {'pcg.f32_rw': 1}, {'pcg.f32_rw': 2}, {'pcg.gemv_plain': 1})
QR = ((150, 129), (594, 513))
COND = (594, 130, 'b', 1e-6)
# The matrix-free case.  A force kernel matrix of M frames with N atoms has rank M (3N - 6) (translations and rotations of a
# frame are in its null space): 30 frames of 6 atoms (n = 540) carry rank 360, so no 513 columns of it are independent.
# Hence 90 frames (n = 1620) and at most 6 columns per frame, sig = 0.25.  The coordinates of one frame stay coupled
# through the descriptor Jacobian at any sig: cond(K_mm) comes out at 1e4 ... 2e5 (test_nys_edges_cpu.py holds <= 1e6).
MF = dict(N=6, M=90, m=513, cols_per_frame=6, sig=0.25, lam=LAM)


def grid_cases():
    """Every (n, m, family, lam) the GPU module loads."""
    s = [(n, m, 'a', LAM) for n, m in GRAM_TILES + (GRAM_SPLIT,) + SOLVE_SMALL + GEMV64 + QR]
    s += [(SOLVE_N, m, 'a', LAM) for m in SOLVE_M] + [(F32_N, m, 'a', LAM) for m in F32_M] + [COND]
    return sorted(set(s))


@functools.lru_cache(maxsize=None)
def mf_system(seed=0):
    """The matrix-free case: a real kernel matrix from the oracle.  (R_desc, R_d_desc, tril_perms, K_nm, idx, Kv)."""
    from oracle import gdml_oracle as orc

    ds = orc.synth_dataset(MF['N'], MF['M'], seed=seed + 1)
    xd, gd = orc.desc_from_R(ds['R'].reshape(MF['M'], -1))
    tp = orc.tril_perms_from_atom_perms(np.arange(MF['N'])[None])
    K = orc.assemble_K(xd, gd, orc.tril_perms_lin_from_tril_perms(tp), MF['sig'])
    K = 0.5 * (K + K.T)
    n = K.shape[0]
    rs = np.random.RandomState(4243 + seed)
    d = 3 * MF['N']
    assert n == MF['M'] * d
    cand = np.concatenate([f * d + rs.permutation(d)[:MF['cols_per_frame']] for f in range(MF['M'])])
    idx = np.sort(rs.choice(cand, MF['m'], replace=False)).astype(np.int64)
    K_nm = np.ascontiguousarray(K[:, idx])
    return xd, gd, tp, K_nm, idx, (lambda v: K @ v)


# ------------------------------------------------------------------ references and allowances, cached per case

@functools.lru_cache(maxsize=4)
def ref_ld(n, m, family='a', lam=LAM, seed=0, upto='X2'):
    K, idx = case_matrix(n, m, family, seed)
    return nys_ld(K, idx, lam, upto)


@functools.lru_cache(maxsize=2)
def ref_f32_ld(n, m, lam=LAM, seed=0):
    _, _, L, X2 = ref_ld(n, m, 'a', lam, seed)
    return f32_form_ld(X2.astype(np.float64), L, lam)


def restatement_errors(check, n, m, family='a', lam=LAM, seed=0, defect=None, **opt):
    """Error of the float64 restatement against the long-double reference for one measured check and one seed."""
    K, idx = case_matrix(n, m, family, seed)
    v = vec(n, seed)
    if check == 'M4':
        _, X1, _, _ = ref_ld(n, m, family, lam, seed, 'X1')
        L_mm = np.linalg.cholesky(sym_from_lower(-K[idx]) + EPS * np.eye(m))
        return rel_err(_trsm_f64(K, L_mm, defect), X1)
    _, _, L, X2 = ref_ld(n, m, family, lam, seed)
    if check in ('M1', 'M3'):
        r = nys_f64(K, idx, lam, force_qr=(check == 'M3'), defect=defect)
        return rel_err(precon_f64(r['X2'], lam, v, defect), precon_ld(X2, lam, v))
    if check == 'M2':
        r = nys_f64(K, idx, lam)
        X32, T0, _ = f32_form_f64(r['X2'], r['L'], lam, gram_rows=opt.get('gram_rows', 2048), defect=defect)
        out = precon_f32_f64(X32, T0, lam, v, opt.get('rows_per', 1024), opt.get('rw', 4), defect)
        return rel_err(out, precon_f32_ld(*ref_f32_ld(n, m, lam, seed), lam, v))
    raise ValueError(check)


@functools.lru_cache(maxsize=None)
def allowance(check, n, m, family='a', lam=LAM):
    """10 x the largest restatement error over SEEDS (module docstring).  Returns (allowance, the errors)."""
    errs = tuple(restatement_errors(check, n, m, family, lam, s) for s in SEEDS)
    return 10.0 * max(errs), errs


def mf_ref(seed=0):
    """(restatement error, long-double reference of P v, v) of the matrix-free case for one seed."""
    xd, gd, tp, K_nm, idx, Kv = mf_system(seed)
    v = vec(len(K_nm), seed)
    _, _, _, X2 = nys_ld(K_nm, idx, MF['lam'])
    ref = precon_ld(X2, MF['lam'], v)
    return rel_err(mf_f64(K_nm, idx, MF['lam'], Kv, v), ref), ref, v


@functools.lru_cache(maxsize=None)
def mf_allowance():
    refs = [mf_ref(s) for s in SEEDS]
    errs = tuple(r[0] for r in refs)
    return 10.0 * max(errs), errs, refs[0][1], refs[0][2]


# ------------------------------------------------------------------ the device side (ctypes through sgdml_amd._lib only)

def _buffer(ctx):
    rows, cols, extra = ctx.K_shape()
    p, ld = C.c_void_p(), C.c_int64()
    ctx._check(ctx._lib.gdml_K_dev(ctx._h, C.byref(p), C.byref(ld)))
    return p, ld.value, rows + extra


def raw_buffer(ctx):
    """The whole (n + m) x ld buffer, pitch padding included."""
    p, ld, r = _buffer(ctx)
    buf = np.empty((r, ld))
    ctx._check(ctx._lib.gdml_memcpy_d2h(ctx._h, buf.ctypes.data_as(C.c_void_p), p, buf.nbytes))
    return buf


def load_nystroem(ctx, n, idx, K_nm, sig=10.0):
    """Make K_nm (n x m) the resident, unfactored Nystroem matrix of ctx: a dummy training set with n rows is uploaded and
    assembled with m extra rows, then the whole (n + m) x ld buffer is overwritten: rows [0, n) hold K_nm in columns [0, m),
    everything else -- the pitch padding [m, ld) and the m-row work block -- is NaN.  The padding holds whatever the
    allocator left there in production, so a kernel that lets it into a result shows.  Returns ld."""
    N, use_E, M = reachable(n)
    xd, gd, tp = _dummy_set(N, M)
    m = len(idx)
    ctx.train_upload(xd, gd, tp)
    ctx.assemble_K(sig, use_E, idx=np.asarray(idx, dtype=np.int64), alloc_extra_rows=m)
    assert ctx.K_shape() == (n, m, m), (ctx.K_shape(), n, m)
    p, ld, rows = _buffer(ctx)
    assert ld == round16(m) and rows == n + m
    buf = np.full((n + m, ld), np.nan)
    buf[:n, :m] = K_nm
    ctx._check(ctx._lib.gdml_memcpy_h2d(ctx._h, p, buf.ctypes.data_as(C.c_void_p), buf.nbytes))
    return ld


class options(object):
    """with options(ctx, {...}): set, and restore the defaults (the values named in csrc) on the way out."""
    DEFAULTS = {'pcg.precon_form': 2, 'pcg.f32_inplace': 1, 'pcg.gemv_plain': 0, 'pcg.f32_gram_rows': 2048,
                'pcg.f32_rows_per': 1024, 'pcg.f32_rw': 4, 'nys.syrk_split': 1, 'nys.trsm_left': 1, 'nys.force_qr': 0}

    def __init__(self, ctx, opts):
        self.ctx, self.opts = ctx, dict(opts)

    def __enter__(self):
        for k, v in self.opts.items():
            self.ctx.set_option(k, v)
        return self.ctx

    def __exit__(self, *exc):
        for k in self.opts:
            self.ctx.set_option(k, self.DEFAULTS[k])
        return False


def dev_stages(ctx, n, m, family='a', lam=LAM, opts=None, checks=('S1', 'S2', 'S3', 'M4')):
    """Stage 1 on the device (pcg.precon_form = 1 without scores or host copy leaves X1 and L in the buffer), then the
    second solve and the scores through nystroem_lev_scores.  Returns the ratios of the checks asked for."""
    K, idx = case_matrix(n, m, family, 0)
    out = {}
    with options(ctx, dict(opts or {}, **{'pcg.precon_form': 1})):
        load_nystroem(ctx, n, idx, K)
        lev0, fac, info = ctx.nystroem_factor(lam, idx, want_factor=False, want_lev=False)
        assert lev0 is None and fac is None
        out['info'] = info
        H = ctx.K_to_host()
        X1, L = H[:n].copy(), np.tril(H[n:n + m])
        out['finite'] = bool(np.isfinite(X1).all() and np.isfinite(L).all())
        if 'S1' in checks:
            out['S1'] = s1_ratio(X1, L, lam)
        if 'M4' in checks:
            a, errs = allowance('M4', n, m, family, lam)
            e = rel_err(X1, ref_ld(n, m, family, lam, 0, 'X1')[1])
            out['M4'] = e / a
            out['M4_allowance'], out['M4_restatement'], out['M4_error'] = a, max(errs), e
        if 'S2' in checks or 'S3' in checks:
            lev = ctx.nystroem_lev_scores()
            H2 = ctx.K_to_host()
            X2 = H2[:n].copy()
            out['finite'] = bool(out['finite'] and np.isfinite(X2).all() and np.isfinite(lev).all())
            out['L_kept'] = bool(np.array_equal(np.tril(H2[n:n + m]), L))
            if 'S2' in checks:
                out['S2'] = s2_ratio(X1, L, X2)
            if 'S3' in checks:
                out['S3'] = s3_ratio(X2, lev)
    return out


def dev_apply(ctx, n, m, family='a', lam=LAM, opts=None, checks=('S4', 'M1')):
    """Form 0 on the device: S4 on the factor read back (pcg.gemv_plain 0 and 1 bit-equal), M1 / M3 against nys_ld."""
    K, idx = case_matrix(n, m, family, 0)
    v = vec(n, 0)
    out = {}
    with options(ctx, dict({'pcg.precon_form': 0}, **(opts or {}))):
        load_nystroem(ctx, n, idx, K)
        _, _, info = ctx.nystroem_factor(lam, idx, want_factor=False, want_lev=False)
        out['info'] = info
        X2 = ctx.K_to_host()[:n].copy()
        pv = ctx.precon_apply(lam, v)
        with options(ctx, {'pcg.gemv_plain': 1}):
            pv1 = ctx.precon_apply(lam, v)
        out['finite'] = bool(np.isfinite(X2).all() and np.isfinite(pv).all())
        out['plain_equal'] = bool(np.array_equal(pv, pv1))
        if 'S4' in checks:
            out['S4'] = s4_ratio(X2, lam, v, pv)
        if 'S3' in checks:
            out['S3'] = s3_ratio(X2, ctx.nystroem_lev_scores())
        for chk in ('M1', 'M3'):
            if chk in checks:
                a, errs = allowance(chk, n, m, family, lam)
                e = rel_err(pv, precon_ld(ref_ld(n, m, family, lam, 0)[3], lam, v))
                out[chk] = e / a
                out[chk + '_allowance'], out[chk + '_restatement'], out[chk + '_error'] = a, max(errs), e
    return out


def _f32_overlay(ctx, n, m):
    """(X32 (n x m float32), the floats [m, ld) of every row) of the in-place overlay (row pitch 2 ld floats)."""
    raw = raw_buffer(ctx)
    ld = raw.shape[1]
    f = raw.view(np.float32).reshape(raw.shape[0], 2 * ld)[:n]
    return f[:, :m].copy(), f[:, m:ld].copy()


def dev_f32(ctx, m, n=F32_N, lam=LAM):
    """Form 3 on the device at every build and application variant: S5 and one M2 ratio per variant."""
    K, idx = case_matrix(n, m, 'a', 0)
    v = vec(n, 0)
    a, errs = allowance('M2', n, m, 'a', lam)
    ref = precon_f32_ld(*ref_f32_ld(n, m, lam, 0), lam, v)
    out = {'M2': {}, 'M2_allowance': a, 'M2_restatement': max(errs), 'S5': True, 'S5_detail': {}}
    for build in F32_BUILDS:
        bkey = ','.join('%s=%g' % kv for kv in sorted(build.items())) or 'default'
        kept = {}
        for inplace in (0, 1):
            with options(ctx, dict(build, **{'pcg.precon_form': 3, 'pcg.f32_inplace': inplace})):
                load_nystroem(ctx, n, idx, K)
                _, _, info = ctx.nystroem_factor(lam, idx, want_factor=False, want_lev=False)
                d = {'info4': bool(info & 4), 'piv': ctx.get_option('pcg.f32_last_min_pivot')}
                if inplace == 0:
                    d['X2'] = ctx.K_to_host()[:n].copy()
                else:
                    d['X32'], d['pad'] = _f32_overlay(ctx, n, m)
                d['lev'] = ctx.nystroem_lev_scores()
                for ap in F32_APPLY:
                    akey = ','.join('%s=%g' % kv for kv in sorted(ap.items())) or 'default'
                    with options(ctx, ap):
                        pv = ctx.precon_apply(lam, v)
                    d[akey] = pv
                    out['M2']['%s|inplace=%d|%s' % (bkey, inplace, akey)] = rel_err(pv, ref) / a
                kept[inplace] = d
        det = {'info4': kept[0]['info4'] and kept[1]['info4'],
               'overlay_equal': bool(np.array_equal(kept[1]['X32'], kept[0]['X2'].astype(np.float32))),
               'pad_zero': bool((kept[1]['pad'].view(np.uint32) == 0).all()),
               'lev_equal': bool(np.array_equal(kept[0]['lev'], kept[1]['lev'])),
               'apply_equal': all(np.array_equal(kept[0][k], kept[1][k]) for k in kept[0]
                                  if k not in ('info4', 'piv', 'X2', 'lev')),
               'min_pivot': kept[0]['piv']}
        out['S5_detail'][bkey] = det
        out['S5'] = bool(out['S5'] and all(det[k] for k in ('info4', 'overlay_equal', 'pad_zero', 'lev_equal', 'apply_equal')))
    return out


def dev_mf(ctx):
    """The matrix-free form on a really assembled system (no overwrite): M5 against nys_ld on the oracle's K_nm."""
    xd, gd, tp, K_nm, idx, _ = mf_system(0)
    a, errs, ref, v = mf_allowance()
    with options(ctx, {'pcg.precon_form': 1}):
        ctx.train_upload(xd, gd, tp)
        ctx.assemble_K(MF['sig'], False, idx=idx, alloc_extra_rows=len(idx))
        dK = rel_err(ctx.K_to_host()[:len(K_nm)], K_nm)
        _, _, info = ctx.nystroem_factor(MF['lam'], idx, want_factor=False, want_lev=False)
        pv = ctx.precon_apply(MF['lam'], v)
    e = rel_err(pv, ref)
    return {'info': info, 'M5': e / a, 'M5_allowance': a, 'M5_restatement': max(errs), 'M5_error': e, 'assembly_vs_oracle': dK}


def still_usable(ctx):
    """After a group: default options, a fresh assembly, one application inside its M1 allowance."""
    n, m = GRAM_TILES[1]
    r = dev_apply(ctx, n, m, checks=('M1',), opts={'pcg.precon_form': 2})
    return r['finite'] and r['M1'] <= 1.0


# ------------------------------------------------------------------ the GPU grid: one list for the test module and the record

def _info_plain(info, form_bits):
    """No jitter escalation, no QR branch, the form bits as expected."""
    return info >> 8 == 0 and info & 1 == 0 and (info & 6) == form_bits


def _run_gram_tiles(ctx, n, m):
    s = dev_stages(ctx, n, m, checks=('S1',))
    a = dev_apply(ctx, n, m, checks=('M1',))
    return {'stages': s, 'apply': a, 'info_ok': _info_plain(s['info'], 2) and _info_plain(a['info'], 0)}


def _run_gram_split(ctx, split):
    n, m = GRAM_SPLIT
    s = dev_stages(ctx, n, m, opts={'nys.syrk_split': split}, checks=('S1', 'S2'))
    return {'stages': s, 'info_ok': _info_plain(s['info'], 2)}


def _run_solve(ctx, n, m, left):
    checks = ('S2', 'M4') + (('S1',) if m in (513, 576) else ())
    s = dev_stages(ctx, n, m, opts={'nys.trsm_left': left}, checks=checks)
    return {'stages': s, 'info_ok': _info_plain(s['info'], 2)}


def _run_gemv64(ctx, n, m):
    a = dev_apply(ctx, n, m, checks=('S3', 'S4'))
    return {'apply': a, 'info_ok': _info_plain(a['info'], 0)}


def _run_qr(ctx, n, m):
    a = dev_apply(ctx, n, m, opts={'nys.force_qr': 1}, checks=('M3',))
    return {'apply': a, 'info_ok': a['info'] >> 8 == 0 and a['info'] & 1 == 1 and (a['info'] & 6) == 0}


def _run_cond(ctx):
    n, m, fam, lam = COND
    s = dev_stages(ctx, n, m, fam, lam, checks=('S1', 'S2'))
    a = dev_apply(ctx, n, m, fam, lam, checks=('S4',))
    return {'stages': s, 'apply': a, 'info_ok': _info_plain(s['info'], 2) and _info_plain(a['info'], 0)}


def _run_mf(ctx):
    r = dev_mf(ctx)
    return {'mf': r, 'info_ok': _info_plain(r['info'], 2)}


def gpu_cases():
    """[(group, key, run(ctx) -> result)] in the order they run."""
    c = [('gram_tiles', 'gram_tiles-%d-%d' % nm, functools.partial(_run_gram_tiles, n=nm[0], m=nm[1])) for nm in GRAM_TILES]
    c += [('gram_split', 'gram_split-%d-%d-split%d' % (GRAM_SPLIT + (s,)), functools.partial(_run_gram_split, split=s)) for s in (1, 0)]
    for n, m in [(SOLVE_N, m) for m in SOLVE_M] + list(SOLVE_SMALL):
        c += [('solves', 'solves-%d-%d-left%d' % (n, m, lf), functools.partial(_run_solve, n=n, m=m, left=lf)) for lf in (1, 0)]
    c += [('gemv64', 'gemv64-%d-%d' % nm, functools.partial(_run_gemv64, n=nm[0], m=nm[1])) for nm in GEMV64]
    c += [('f32_form', 'f32_form-%d-%d' % (F32_N, m), functools.partial(dev_f32, m=m)) for m in F32_M]
    c += [('qr', 'qr-%d-%d' % nm, functools.partial(_run_qr, n=nm[0], m=nm[1])) for nm in QR]
    c += [('conditioning', 'conditioning-%d-%d-%s-%g' % COND, _run_cond)]
    c += [('matrix_free', 'matrix_free-%d-%d' % (MF['M'] * 3 * MF['N'], MF['m']), _run_mf)]
    return c


RATIO_KEYS = ('S1', 'S2', 'S3', 'S4', 'M1', 'M2', 'M3', 'M4', 'M5')
FLAG_KEYS = ('finite', 'plain_equal', 'L_kept', 'S5', 'info_ok')


def ratios(result, prefix=''):
    """Flat {path: ratio} of every stage / measured ratio in a case's result."""
    out = {}
    for k, v in result.items():
        if isinstance(v, dict) and k != 'S5_detail':
            if k in RATIO_KEYS:
                out.update({'%s%s[%s]' % (prefix, k, kk): vv for kk, vv in v.items()})
            else:
                out.update(ratios(v, prefix + k + '.'))
        elif k in RATIO_KEYS:
            out[prefix + k] = v
    return out


def failures(result, prefix=''):
    """What a case's result violates: a ratio above 1 (or not finite), a flag that is not set."""
    bad = ['%s = %.3g' % kv for kv in sorted(ratios(result).items()) if not kv[1] <= 1.0]
    for k, v in result.items():
        if isinstance(v, dict) and k not in RATIO_KEYS and k != 'S5_detail':
            bad += failures({kk: vv for kk, vv in v.items() if kk in FLAG_KEYS or (isinstance(vv, dict) and kk not in RATIO_KEYS)},
                            prefix + k + '.')
        elif k in FLAG_KEYS and v is not True:
            bad.append('%s%s is %r' % (prefix, k, v))
    if 'S5_detail' in result and not result.get('S5', True):
        bad.append('S5 detail: %r' % (result['S5_detail'],))
    return bad

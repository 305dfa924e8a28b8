"""Helper and reference of the Cholesky edge tests (tests/test_chol_edges_cpu.py, tests/test_chol_edges_gpu.py): plain
NumPy / SciPy, no GPU import.  Test helper only: the package never imports it.

The resident matrix of a context is the kernel matrix of the uploaded training set, n = M 3N (+ M with energy constraints)
rows.  The tests want a factorisation of THEIR matrix at THEIR size, so they upload a dummy training set of the right
shape (reachable), let the library allocate its matrix and overwrite the buffer (load_spd).

Bounds (u = 2^-53, gamma_k = k u / (1 - k u), Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed.):
  factor  |A - L L^T| <= gamma_{n+1} |L| |L^T|  componentwise (Theorem 10.3).  It is derived from the error of an inner
          product of at most n terms plus one square root / division, holds for ANY order of summation and therefore for any
          tiling, panel width or schedule.
  solve   the computed solution of L L^T x = y satisfies (A + dA) x = y with |dA| <= gamma_{3n+1} |L| |L^T| (Theorem 10.4:
          gamma_{n+1} of the factor and gamma_n per substitution, cross terms included).  The kernels differ from the
          theorem's model in two places: pivots come from a reciprocal square root by Newton steps, for which the tests
          grant the factor twice its bound (one more gamma_{n+1}), and both substitutions multiply by a reciprocal pivot
          instead of dividing (one more rounding on the diagonal: gamma_{n+1} per substitution instead of gamma_n).  The
          residual itself is evaluated in floating point (gamma_n |A| |x|, |A| <= |L||L^T| up to the factor's own error).
          Together:  |y - A x| <= gamma_{5n+8} (|L| |L^T|) |x|  componentwise: solve_bound.  This is the backward-error form
          of tests/_tol.py (eps ||A|| ||x||) and tests/_loo_ref.py, componentwise and with a derived constant.
  Two computed solutions x1, x2 of the same system are compared through the same bound: A (x1 - x2) is the difference of
  their residuals, so |A (x1 - x2)| <= solve_bound(x1) + solve_bound(x2).
"""
import ctypes as C
import functools

import numpy as np
import scipy.linalg as sla

U = 2.0 ** -53


def gamma(k):
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------ sizes the public path can allocate

def reachable(n):
    """(N, use_E_cstr, M): a training set of M points with N atoms (2 <= N <= 6) whose kernel matrix has exactly n rows,
    n = M 3N or n = M (3N + 1).  The smallest N that divides wins (cheapest dummy assembly).  ValueError if there is none."""
    n = int(n)
    for N in range(2, 7):
        for use_E in (False, True):
            d = 3 * N + (1 if use_E else 0)
            if n >= d and n % d == 0:
                return N, use_E, n // d
    raise ValueError('no training set with 2 <= N <= 6 atoms has a kernel matrix of %d rows' % n)


# ------------------------------------------------------------------ matrices

def spd(family, n, seed=None):
    """Seeded symmetric positive definite test matrix.
      'a'  B B^T / n + 0.5 I, B n x (n + 20) normal: condition number ~ 10 (the family of tests/test_hip_parity.py)
      'b'  Q diag(s) Q^T, s log-spaced over 8 decades (1e-8 .. 1), Q from the QR of a normal matrix: the conditioning of the
           real -K + lam I at lam = 1e-10 relative to its largest eigenvalues.  Symmetrised exactly."""
    rs = np.random.RandomState(1000 + n if seed is None else seed)
    if family == 'a':
        B = rs.normal(size=(n, n + 20))
        return B @ B.T / n + 0.5 * np.eye(n)
    if family == 'b':
        Q, _ = np.linalg.qr(rs.normal(size=(n, n)))
        s = np.logspace(-8.0, 0.0, n)
        A = (Q * s) @ Q.T
        return 0.5 * (A + A.T)
    raise ValueError(family)


def rhs(n, seed=None):
    return np.random.RandomState(77 + n if seed is None else seed).normal(size=n)


def abs_gram(L):
    """|L| |L^T| (n x n)."""
    aL = np.abs(np.tril(L))
    return aL @ aL.T


def factor_bound(L, n):
    """Componentwise bound on |A - L L^T| of a Cholesky factor computed in fp64 with correctly rounded operations, any
    summation order: gamma_{n+1} (|L| |L^T|)_ij."""
    return gamma(n + 1) * abs_gram(L)


def factor_ratio(A, L, G=None):
    """max over the lower triangle of |A - L L^T|_ij / factor_bound_ij (G = abs_gram(L) if already at hand)."""
    n = len(A)
    L = np.tril(L)
    if G is None:
        G = abs_gram(L)
    low = np.tril(np.ones((n, n), dtype=bool))
    return float((np.abs(A - L @ L.T)[low] / (gamma(n + 1) * G[low])).max())


def solve_bound(G, x):
    """Componentwise bound on |y - A x| (module docstring); G = abs_gram(L)."""
    return gamma(5 * len(x) + 8) * (G @ np.abs(x))


def solve_ratio(A, G, x, y):
    return float((np.abs(y - A @ x) / solve_bound(G, x)).max())


def agree_ratio(A, G, x1, x2):
    """max |A (x1 - x2)| / (solve_bound(x1) + solve_bound(x2))."""
    return float((np.abs(A @ (x1 - x2)) / (solve_bound(G, x1) + solve_bound(G, x2))).max())


@functools.lru_cache(maxsize=3)
def reference(family, n):
    """(A, y, L_ref, G_ref = |L_ref||L_ref^T|, x_ref) of a case, by SciPy; computed once and shared (read only)."""
    A = spd(family, n)
    y = rhs(n)
    L = sla.cholesky(A, lower=True, check_finite=False)
    x = sla.cho_solve((L, True), y, check_finite=False)
    out = (A, y, L, abs_gram(L), x)
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------ the schedule of chol_factor_device, restated

def schedule(n, rhs_row, nb=512, outer=1024, fused_min_rows=12288, outer_min_rows=16384):
    """The host-side decisions of chol_factor_device (csrc/chol.hip) for a matrix of order n: the list of
    (arm, first column, width) of the panels after the first one, arm in 'pair' (two fused launches, K = 2 nb), 'single'
    (one fused launch), 'tail' (two streams) and 'last' (the final panel, step chain on the main stream), and the launch
    counts the per-kernel timers of the main stream report for it:
      gemm_nt_sub_diag  2 per pair, 1 per single                       (launches that carry a diagonal-block workgroup)
      gemm_nt_sub       1 per single, 2 per tail panel, 1 per last     (plain trailing updates on the main stream)
      panel_trsm        first panel if rows lie below it and its width is a multiple of 64; 2 per pair, 1 per single;
                        the last panel if it carries the right-hand-side row and its width is a multiple of 64
    (the tail arm's step chain and solve run on the second stream, which the timers do not see).  The tests compare these
    counts with gdml_kernel_stat, so that a threshold which quietly routes to another arm fails them."""
    n_rows = n + (1 if rhs_row else 0)
    NB = int(nb)
    if NB < 64 or NB % 64 or NB > 512:
        NB = 512
    OB = int(outer)
    if OB != 2 * NB or NB % 128 != 0:
        OB = NB
    min_rows = max(int(fused_min_rows), 1)

    def width_at(c0):
        left = n - (c0 + OB)
        w = OB if (OB > NB and left > 0 and left >= outer_min_rows) else NB
        return min(w, n - c0)

    w0 = min(n, NB)  # first panel: nothing to hide its diagonal block behind
    arms = []
    stat = {'gemm_nt_sub_diag': 0, 'gemm_nt_sub': 0, 'panel_trsm': 1 if (w0 % 64 == 0 and n_rows - w0 > 0) else 0}
    t0 = w0
    while t0 < n:
        nb2 = width_at(t0)
        t1 = t0 + nb2
        fuse = nb2 % 64 == 0 and n - t1 >= min_rows and n_rows - t1 > 0
        if fuse and nb2 == 2 * NB:
            arms.append(('pair', t0, nb2))
            stat['gemm_nt_sub_diag'] += 2
            stat['panel_trsm'] += 2
        elif fuse:
            arms.append(('single', t0, nb2))
            stat['gemm_nt_sub'] += 1
            stat['gemm_nt_sub_diag'] += 1
            stat['panel_trsm'] += 1
        elif t1 < n:
            arms.append(('tail', t0, nb2))
            stat['gemm_nt_sub'] += 2
        else:
            arms.append(('last', t0, nb2))
            stat['gemm_nt_sub'] += 1
            if nb2 % 64 == 0 and n_rows - t1 > 0:
                stat['panel_trsm'] += 1
        t0 = t1
    return arms, stat


def solve_launches(n, persist):
    """Kernel launches the 'solve' phase counts for chol_solve(y): one forward kernel per 64-block, then ONE persistent
    backward launch (n >= 2048 and trsv.persist != 0) or one backward kernel per 64-block."""
    nbk = (n + 63) // 64
    return nbk + (1 if (persist and n >= 2048) else nbk)


# ------------------------------------------------------------------ the cases (shared by the CPU and the GPU module)

# default options: a first panel narrower than 64, exactly one / two / eight 64-blocks, one past them, the tail arm with 1, 2
# and 3 panels.  127 is prime: 126 stands for it (128 is in the list anyway).
BLOCK_EDGE_SIZES = (6, 7, 63, 64, 65, 126, 128, 130, 511, 512, 513, 576, 1022, 1024, 1026)
# rows below the first 64-block, right-hand-side row included: 2048 (n = 2112 without the row) and 2049 (with it)
SWITCH_N = 2112
NB_SWEEP_N = 1026  # ragged against every panel width (1026 = 16 * 64 + 2)
NB_PAIR_N = 1542   # a pair of 384-wide panels needs n > 3 * 384; 1542 = 24 * 64 + 6 = 4 * 384 + 6
NB_SINGLE = (64, 128, 192, 256, 384, 448)
NB_PAIR = (128, 256, 384)
BWD_SIZES = (2046, 2048, 2070)  # below the persistent kernel's threshold, at it, above it with a ragged last block (22)

# (id, n, options, the arms schedule() must report).  chol.nb = 512 throughout; first panel = columns 0..511.
ARM_EDGES = (
    # n - t1 == chol.fused_min_rows exactly (t1 = 1024): fused; the next panels fall short of it -> tail, last (ragged)
    ('fused_min_equal', 1548, {'chol.outer': 512, 'chol.fused_min_rows': 524}, ('single', 'tail', 'last')),
    # one 6-step below: nothing is fused
    ('fused_min_below', 1542, {'chol.outer': 512, 'chol.fused_min_rows': 524}, ('tail', 'tail', 'last')),
    # trailing matrix behind the pair == chol.outer_min_rows exactly: pair, then the ragged last panel (12 columns)
    ('outer_min_equal', 1548, {'chol.outer': 1024, 'chol.outer_min_rows': 12, 'chol.fused_min_rows': 1}, ('pair', 'last')),
    # one 6-step below: single panels; the last panel (6 columns, nb2 % 64 != 0) follows a FUSED predecessor
    ('outer_min_below', 1542, {'chol.outer': 1024, 'chol.outer_min_rows': 12, 'chol.fused_min_rows': 1},
     ('single', 'single', 'last')),
    # a pair whose trailing update has 2 super-tile rows (n_rows - t0 <= 2048): s_split = 3 / 2 = 1 is clamped to sm = 2;
    # ragged last panel behind the pair
    ('pair_split_clamped', 1542, {'chol.outer': 1024, 'chol.outer_min_rows': 1, 'chol.fused_min_rows': 1}, ('pair', 'last')),
    # a last panel of exactly 64 columns behind fused predecessors
    ('last_panel_64', 1600, {'chol.outer': 512, 'chol.fused_min_rows': 1}, ('single', 'single', 'last')),
    # chol.fused_min_rows = 0 (tools/diag_role_probe.py sets it): the last panel has NO trailing matrix to ride in; it must
    # take the step chain, not a fused launch with an empty update
    ('fused_min_zero', 1600, {'chol.outer': 512, 'chol.fused_min_rows': 0}, ('single', 'single', 'last')),
)

# (id, n, options, 0-based index of the -1 on the diagonal of the identity, where it is found)
NOT_PD = (
    ('first_block_0', 130, {}, 0),        # potrf_trsm64_kernel, c0 = 0
    ('first_block_63', 130, {}, 63),      # last pivot of the first 64-block
    ('second_block_64', 130, {}, 64),     # first pivot of the second step of the chain (c0 = 64)
    ('lone_last_block', 130, {}, 129),    # potrf64_kernel on the ragged last block (w = 2)
    ('tail_second_panel', 1026, {}, 700),  # step chain on the second stream, default options
    ('fused_single', 1542, {'chol.outer': 512, 'chol.fused_min_rows': 1}, 700),  # diag_block_role, c0 = 128 of the block at 512
    ('fused_pair_a', 1548, {'chol.outer': 1024, 'chol.outer_min_rows': 1, 'chol.fused_min_rows': 1}, 700),
    ('fused_pair_b', 1548, {'chol.outer': 1024, 'chol.outer_min_rows': 1, 'chol.fused_min_rows': 1}, 1224),
)


def gpu_sizes():
    """Every matrix order tests/test_chol_edges_gpu.py factors."""
    s = set(BLOCK_EDGE_SIZES) | {SWITCH_N, NB_SWEEP_N, NB_PAIR_N} | set(BWD_SIZES)
    s |= {c[1] for c in ARM_EDGES} | {c[1] for c in NOT_PD}
    return sorted(s)


# ------------------------------------------------------------------ loading a matrix into a context (GPU side, ctypes only)

@functools.lru_cache(maxsize=None)
def _dummy_set(N, M):
    from oracle import gdml_oracle as orc

    ds = orc.synth_dataset(N, M, seed=1)
    xd, gd = orc.desc_from_R(ds['R'].reshape(M, -1))
    return xd, gd, orc.tril_perms_from_atom_perms(np.arange(N)[None])


def load_spd(ctx, n, A, rhs=None):
    """Make A (n x n, symmetric positive definite) the resident, unfactored matrix of ctx, so that ctx.chol_factor(0.0)
    factors it: a dummy training set of the right shape is uploaded and assembled (alloc_extra_rows = 1 with a right-hand
    side), then the buffer is overwritten with -A (gdml_chol_factor negates the lower triangle: negate_shift_kernel
    touches row r only in its columns c <= r).  The strict upper triangle and the pitch padding (K_ld = n rounded up to 16)
    are filled with NaN: csrc/chol.hip declares the upper triangle scratch, so a kernel that lets it into a result
    shows.  With rhs the extra row is handed over through chol_set_rhs (its padding is NaN too).  Returns K_ld."""
    N, use_E, M = reachable(n)
    xd, gd, tp = _dummy_set(N, M)
    ctx.train_upload(xd, gd, tp)
    extra = 1 if rhs is not None else 0
    ctx.assemble_K(10.0, use_E, alloc_extra_rows=extra)
    rows, cols, ex = ctx.K_shape()
    assert (rows, cols, ex) == (n, n, extra), (rows, cols, ex, n)
    p, ld = C.c_void_p(), C.c_int64()
    ctx._check(ctx._lib.gdml_K_dev(ctx._h, C.byref(p), C.byref(ld)))
    assert ld.value == (n + 15) // 16 * 16
    buf = np.full((n + extra, ld.value), np.nan)
    buf[:n, :n] = np.where(np.tril(np.ones((n, n), dtype=bool)), -np.asarray(A), np.nan)
    ctx._check(ctx._lib.gdml_memcpy_h2d(ctx._h, p, buf.ctypes.data_as(C.c_void_p), buf.nbytes))
    if rhs is not None:
        ctx.chol_set_rhs(rhs)  # copies n values into row n; the padding behind them stays NaN
    return ld.value

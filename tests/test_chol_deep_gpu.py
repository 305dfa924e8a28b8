"""The deep schedule of the Cholesky factorisation (chol.deep, csrc/tile_sched.h + csrc/chol.hip) on the GPU at the smallest
sizes where each of its arms exists: chol.nb = 128 (outer panels of 256 columns), chol.deep = 512 and 768, thresholds lowered.

  case        n     blocks                         leaves the deep regime                    then
  w512_in    2100   [0, 640) [640, 1152)           at 1408, inside [1152, 1664) (cut block)  fused single, tail, tail, ragged last
  w768_in    2700   [0, 896) [896, 1664)           at 1920, inside [1664, 2432)              one panel pair, tail, tail, last
  w768_blk   2700   [0, 896) [896, 1664)           at 1664, after a whole block              two panel pairs, tail, tail, last
  w512_blk   2304   [0, 640) [640, 1152) [1152, 1664)  at 1664, after a whole block; n is a multiple of the tile: no ragged
                                                   row without the carried one, the carried row alone in the last tile row

Every case runs both matrix families of tests/_chol_ref.py, with and without the carried right-hand side, upper triangle and
pitch padding NaN, and asserts: factor and carried row BITWISE equal to chol.deep = 0 (a deep pass accumulates the same
products in the same order; a ragged last tile row stays in the near band because its guarded body rounds differently); the
componentwise bounds of _chol_ref; through gdml_kernel_stat that far tiles ran and that the composed launches replace the
paired ones one for one.  (tests/test_chol_deep_cpu.py checks the plans themselves.)"""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _chol_ref as cr  # noqa: E402

pytestmark = pytest.mark.gpu

BASE = {'chol.nb': 128, 'chol.outer': 256, 'chol.outer_min_rows': 200, 'chol.fused_min_rows': 200}
CASES = {
    'w512_in': (2100, 512, 800),
    'w768_in': (2700, 768, 900),
    'w768_blk': (2700, 768, 1100),
    'w512_blk': (2304, 512, 800),
}
STAT = ('gemm_nt_sub_diag', 'gemm_nt_sub', 'panel_trsm')


def _ctx(opts):
    from sgdml_amd import _lib

    c = _lib.Context()
    for k, v in opts.items():
        c.set_option(k, v)
    return c


def _factor(opts, n, A, y):
    c = _ctx(opts)
    try:
        cr.load_spd(c, n, A, y)
        c.profile(True)
        assert c.chol_factor(0.0) == 0
        stat = {k: c.kernel_stat(k)[1] for k in STAT}
        stat['deep'] = c.kernel_stat('gemm_nt_sub_deep')
        c.profile(False)
        buf = c.K_to_host()
        xs = [-c.chol_solve(y if y is not None else cr.rhs(n))]
        if y is not None:
            xs.append(-c.chol_solve(None))
        return buf, stat, xs
    finally:
        c.close()


@pytest.mark.parametrize('with_rhs', [False, True], ids=['norhs', 'rhs'])
@pytest.mark.parametrize('family', ['a', 'b'])
@pytest.mark.parametrize('case', sorted(CASES))
def test_deep_factor_is_bitwise_the_one_level_factor(case, family, with_rhs):
    n, W, deep_min = CASES[case]
    A, y, Lref, Gref, _ = cr.reference(family, n)
    rhs = y if with_rhs else None
    buf0, stat0, _ = _factor(dict(BASE, **{'chol.deep': 0}), n, A, rhs)
    buf1, stat1, xs = _factor(dict(BASE, **{'chol.deep': W, 'chol.deep_min_rows': deep_min}), n, A, rhs)
    low = np.tril(np.ones((n, n), dtype=bool))
    L0, L1 = buf0[:n, :n][low], buf1[:n, :n][low]
    assert np.isfinite(L1).all()
    n_diff = int((L0.view(np.uint64) != L1.view(np.uint64)).sum())
    print('%s %s rhs=%d: %d of %d entries of L differ from chol.deep = 0; launches %s' % (case, family, with_rhs, n_diff, L0.size, stat1))
    assert n_diff == 0
    if with_rhs:
        assert np.array_equal(buf0[n, :n].view(np.uint64), buf1[n, :n].view(np.uint64)), 'carried row'
    # the far tiles ran, and the composed launches stand where the paired ones stood
    assert stat0['deep'][1] == 0 and stat1['deep'][1] > 0 and stat1['deep'][2] > 0
    assert {k: stat1[k] for k in STAT} == {k: stat0[k] for k in STAT}
    L = np.tril(buf1[:n, :n])
    G = cr.abs_gram(L)
    q = cr.factor_ratio(A, L, G)
    q_x = max(cr.solve_ratio(A, G, x, y) for x in xs)
    print('factor %.3g of factor_bound, solve %.3g of solve_bound' % (q, q_x))
    assert q <= 2.0 and q_x <= 1.0
    if family == 'a':
        assert np.abs(L - Lref).max() <= 1e-11 * np.abs(Lref).max()


@pytest.mark.parametrize('p', [700, 1153], ids=['near_band', 'behind_block_boundary'])
def test_not_positive_definite_index(p):
    """Identity with a -1 at p: inside the near band of block [640, 1152), and just behind the block boundary 1152 (the block
    workgroup 0 factors behind the first share of a far pass): the reported index is the one chol.deep = 0 reports."""
    n, W, deep_min = CASES['w512_in']
    A = np.eye(n)
    A[p, p] = -1.0
    got = []
    for deep in (0, W):
        c = _ctx(dict(BASE, **{'chol.deep': deep, 'chol.deep_min_rows': deep_min}))
        try:
            cr.load_spd(c, n, A)
            with pytest.raises(np.linalg.LinAlgError) as e:
                c.chol_factor(0.0)
            m = re.search(r'(\d+)-th leading minor of the array is not positive definite', str(e.value))
            assert m, str(e.value)
            got.append(int(m.group(1)))
        finally:
            c.close()
    assert got == [p + 1, p + 1]

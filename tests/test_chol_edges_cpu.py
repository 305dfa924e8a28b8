"""The inputs, bounds and case tables of the Cholesky edge tests (tests/_chol_ref.py) are sound before a kernel is blamed:
every size the GPU module factors can be allocated through the public path, SciPy's own factor and solve stay within the
bounds on both matrix families at every one of those sizes, and each schedule case walks the arms it is named after."""
import os
import sys

import numpy as np
import pytest
import scipy.linalg as sla

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _chol_ref as cr  # noqa: E402


def test_reachable_covers_every_gpu_size():
    for n in cr.gpu_sizes():
        N, use_E, M = cr.reachable(n)
        assert 2 <= N <= 6 and M >= 1 and M * (3 * N + (1 if use_E else 0)) == n
    # the examples of the size rule (divisors 6, 7, 9, 10, 12, 13, 15, 16, 18, 19)
    for n, d in ((63, 7), (64, 16), (65, 13), (128, 16), (130, 10), (511, 7), (512, 16), (513, 9), (1022, 7), (1024, 16),
                 (2046, 6), (2048, 16)):
        N, use_E, M = cr.reachable(n)
        assert 3 * N + (1 if use_E else 0) == d and M == n // d


@pytest.mark.parametrize('n', [1, 5, 8, 11, 127, 1023, 2111, 2113])
def test_reachable_raises_for_sizes_without_a_training_set(n):
    with pytest.raises(ValueError):
        cr.reachable(n)


@pytest.mark.parametrize('family', ['a', 'b'])
@pytest.mark.parametrize('n', cr.gpu_sizes())
def test_scipy_meets_the_bounds(n, family):
    """|A - L L^T| <= factor_bound componentwise (ratio <= 1) and |y - A x| <= solve_bound for LAPACK's factor and solve: a
    condition on the inputs and the bounds, not a measurement.  Family 'b' spans 8 decades of eigenvalues."""
    A, y, L, G, x = cr.reference(family, n)
    assert np.array_equal(A, A.T)
    ev = sla.eigvalsh(A, subset_by_index=[0, 0])[0], sla.eigvalsh(A, subset_by_index=[n - 1, n - 1])[0]
    assert ev[0] > 0
    if family == 'b' and n >= 63:
        assert 1e7 <= ev[1] / ev[0] <= 2e8
    assert np.array_equal(cr.factor_bound(L, n), cr.gamma(n + 1) * G)
    q_f, q_s = cr.factor_ratio(A, L, G), cr.solve_ratio(A, G, x, y)
    print('n = %d family %s: factor %.3g, solve %.3g of their bounds' % (n, family, q_f, q_s))
    assert q_f <= 1.0
    assert q_s <= 1.0
    assert cr.agree_ratio(A, G, x, x) == 0.0


def test_bounds_notice_a_wrong_entry():
    """One entry of L off by 1e-7 relative (far below what the 1e-11 max-norm comparisons of family 'a' can see in family 'b')
    breaks the factor bound the GPU module asserts (ratio <= 2), in both families: the bound is tight enough to mean
    something."""
    for family in 'ab':
        A, y, L, G, x = cr.reference(family, 130)
        L2 = L.copy()
        L2[100, 70] *= 1.0 + 1e-7
        assert cr.factor_ratio(A, L2) > 2.0


@pytest.mark.parametrize('case', cr.ARM_EDGES, ids=[c[0] for c in cr.ARM_EDGES])
def test_arm_edge_cases_walk_the_arms_they_name(case):
    _, n, opts, want = case
    for rhs_row in (False, True):
        arms, stat = cr.schedule(n, rhs_row, 512, opts.get('chol.outer', 1024), opts.get('chol.fused_min_rows', 12288),
                                 opts.get('chol.outer_min_rows', 16384))
        assert tuple(a[0] for a in arms) == want
        assert sum(a[2] for a in arms) == n - 512
        assert stat['gemm_nt_sub_diag'] == 2 * want.count('pair') + want.count('single')


def test_schedule_of_the_other_cases():
    # default options: nothing below n = 12288 + 1024 is fused
    for n in cr.BLOCK_EDGE_SIZES + (cr.SWITCH_N,):
        for rhs_row in (False, True):
            arms, stat = cr.schedule(n, rhs_row)
            assert stat['gemm_nt_sub_diag'] == 0 and all(a[0] in ('tail', 'last') for a in arms)
    assert [a[0] for a in cr.schedule(513, False)[0]] == ['last']
    assert [a[0] for a in cr.schedule(1026, False)[0]] == ['tail', 'last']
    assert [a[0] for a in cr.schedule(cr.SWITCH_N, True)[0]] == ['tail', 'tail', 'tail', 'last']
    # panel widths: every one runs the fused single-panel arm; 128, 256 and 384 pair, 192 (not a multiple of 128) does not
    for nb in cr.NB_SINGLE:
        arms, _ = cr.schedule(cr.NB_SWEEP_N, True, nb, nb, 1, 16384)
        assert arms[0][0] == 'single' and arms[-1][0] == 'last' and arms[-1][2] % 64 != 0
        assert all(a[0] != 'pair' for a in arms)
    for nb in cr.NB_PAIR:
        arms, _ = cr.schedule(cr.NB_PAIR_N, True, nb, 2 * nb, 1, 1)
        assert arms[0] == ('pair', nb, 2 * nb) and arms[-1] == ('last', 1536, 6)
    assert all(a[0] != 'pair' for a in cr.schedule(cr.NB_PAIR_N, True, 192, 384, 1, 1)[0])
    # out-of-range widths fall back to 512
    assert cr.schedule(1542, False, 100, 1024, 1, 1) == cr.schedule(1542, False, 512, 1024, 1, 1)
    assert cr.schedule(1542, False, 576, 1024, 1, 1) == cr.schedule(1542, False, 512, 1024, 1, 1)


def test_not_pd_cases_lie_where_they_say():
    for name, n, opts, p in cr.NOT_PD:
        assert 0 <= p < n
        arms, _ = cr.schedule(n, False, 512, opts.get('chol.outer', 1024), opts.get('chol.fused_min_rows', 12288),
                              opts.get('chol.outer_min_rows', 16384))
        hit = [a for a in arms if a[1] <= p < a[1] + a[2]]
        if name.startswith('fused_pair'):
            assert hit and hit[0][0] == 'pair' and (p - hit[0][1]) // 512 == (0 if name.endswith('_a') else 1)
        elif name == 'fused_single':
            assert hit and hit[0][0] == 'single'
        elif name == 'tail_second_panel':
            assert hit and hit[0][0] == 'tail'
        else:
            assert not hit and n < 512  # inside the first panel = the whole matrix


def test_solve_launch_counts():
    assert cr.solve_launches(2046, 1) == 64 and cr.solve_launches(2048, 1) == 33 and cr.solve_launches(2048, 0) == 64
    assert cr.solve_launches(2070, 1) == 34 and cr.solve_launches(2070, 0) == 66

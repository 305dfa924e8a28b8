"""The inputs, bounds, allowances and case tables of the Nystroem edge tests (tests/_nys_ref.py) are sound before a kernel
is blamed: the float64 restatements of csrc/nystroem.hip and csrc/precon_apply.hip stay inside every stage bound on every grid case, each seeded defect of
a kernel branch breaks the check that is meant to see it (stage checks: ratio > 1; measured checks: more than 100 x the
allowance), the grid reaches every branch its table names -- and does not reach what is declared out of scope -- and the
inputs meet the conditions the device code needs to stay on the path under test.  No GPU."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _nys_ref as nr  # noqa: E402


def test_extended_precision_and_reachable_sizes():
    assert np.finfo(nr.LD).eps < 1e-18, 'no extended precision on this host'
    for n, m, _, _ in nr.grid_cases():
        N, use_E, M = nr.reachable(n)
        assert 2 <= N <= 6 and M >= 1 and M * (3 * N + (1 if use_E else 0)) == n and 1 <= m <= n
    assert nr.reachable(63) == (3, False, 7)   # _chol_ref.reachable would take 9 points of 2 atoms WITH energy constraints
    assert nr.reachable(13) == (4, True, 1)    # 13 rows exist only with them
    assert nr.MF['M'] * 3 * nr.MF['N'] == 1620


@functools.lru_cache(maxsize=None)
def _restated(n, m, family, lam):
    K, idx = nr.case_matrix(n, m, family, 0)
    return nr.nys_f64(K, idx, lam)


@pytest.mark.parametrize('n,m,family,lam', nr.grid_cases())
def test_restatement_inside_the_stage_bounds(n, m, family, lam):
    """S1-S4 on the float64 restatement: ratio <= 1.  A condition on the bounds and the inputs, not a measurement.  That
    nys_f64 returns at all means the first Cholesky needed no jitter (np.linalg.cholesky raises where the device climbs
    the ladder) and the second one succeeded (no QR branch unless forced)."""
    K, idx = nr.case_matrix(n, m, family, 0)
    assert np.array_equal(-K[idx], (-K[idx]).T) and np.array_equal(idx, np.unique(idx))
    r = _restated(n, m, family, lam)
    v = nr.vec(n, 0)
    q = dict(S1=nr.s1_ratio(r['X1'], r['L'], lam), S2=nr.s2_ratio(r['X1'], r['L'], r['X2']),
             S3=nr.s3_ratio(r['X2'], (r['X2'] ** 2).sum(axis=1)), S4=nr.s4_ratio(r['X2'], lam, v, nr.precon_f64(r['X2'], lam, v)))
    print('n = %d m = %d family %s: ' % (n, m, family) + ', '.join('%s %.3g' % kv for kv in sorted(q.items())) + ' of the bounds')
    for k, x in q.items():
        assert x <= 1.0, (k, x)
    if family == 'b':
        for A in (-K[idx], r['L'] @ r['L'].T):  # what the first and the second Cholesky factor: six decades each
            ev = np.linalg.eigvalsh(A)
            assert 3e5 <= ev[-1] / ev[0] <= 3e6, ev[-1] / ev[0]


MEASURED = ([('M1', n, m) for n, m in nr.GRAM_TILES] + [('M4', n, m) for n, m in nr.SOLVE_SMALL]
            + [('M4', nr.SOLVE_N, m) for m in nr.SOLVE_M] + [('M2', nr.F32_N, m) for m in nr.F32_M] + [('M3', n, m) for n, m in nr.QR])


@pytest.mark.parametrize('check,n,m', MEASURED)
def test_measured_allowances(check, n, m):
    """The allowance of every measured check: 10 x the largest restatement error over three seeds; the restatement of the
    seed the device runs sits inside it by construction.  Printed for the record."""
    a, errs = nr.allowance(check, n, m)
    print('%s n = %d m = %d: allowance %.3g (restatement errors %s)' % (check, n, m, a, ', '.join('%.3g' % e for e in errs)))
    assert 0.0 < a < 1e-12 and errs[0] <= a
    if check == 'M2':
        for opt in (dict(gram_rows=256), dict(rows_per=64), dict(rw=1), dict(rw=2)):
            assert nr.restatement_errors('M2', n, m, **opt) <= a, opt


def _stage_defect(n, m, defect, check):
    K, idx = nr.case_matrix(n, m, 'a', 0)
    v = nr.vec(n, 0)
    if check in ('S1', 'S2'):
        r = nr.nys_f64(K, idx, nr.LAM, defect=defect)
        return nr.s1_ratio(r['X1'], r['L'], nr.LAM) if check == 'S1' else nr.s2_ratio(r['X1'], r['L'], r['X2'])
    X2 = _restated(n, m, 'a', nr.LAM)['X2']
    return nr.s4_ratio(X2, nr.LAM, v, nr.precon_f64(X2, nr.LAM, v, defect))


# (defect, check, n, m, options of the restatement): each at the smallest grid case that reaches its branch
STAGE_DEFECTS = (
    ('gram_tail16', 'S1', 63, 5),            # 63 % 16 = 15 rows in the guarded k tail
    ('gram_split2', 'S1') + nr.GRAM_SPLIT,   # the second row range (8184 rows)
    ('gemv_t_tail8', 'S4', 2100, 131),       # second part: 52 rows, 52 % 8 = 4
    ('gemv_t_oddcol', 'S4', 13, 1),
    ('gemv_n_oddcol', 'S4', 13, 1),
    ('trsm_last_block', 'S2', 12, 1),        # one block of width 1
    ('trsm_last_block', 'S2', nr.SOLVE_N, 65),
)
MEASURED_DEFECTS = (
    ('gram_kahan_chunk', 'M2', nr.F32_N, 129, dict(gram_rows=256)),  # chunks 256, 256, 82
    ('gemv_t_f32_mod4', 'M2', nr.F32_N, 129, {}),
    ('gemv_n_tail', 'M2', nr.F32_N, 129, {}),                        # 594 % 16 = 2 rows
    ('T0_L0L0T', 'M2', nr.F32_N, 129, {}),
    ('trsm_last_block', 'M4', 12, 1, {}),
    ('trsm_last_block', 'M4', nr.SOLVE_N, 65, {}),
)


@pytest.mark.parametrize('defect,check,n,m', STAGE_DEFECTS)
def test_seeded_defect_breaks_its_stage_check(defect, check, n, m):
    q0, q = _stage_defect(n, m, None, check), _stage_defect(n, m, defect, check)
    print('%s at n = %d m = %d: %s %.3g of the bound (%.3g without the defect)' % (defect, n, m, check, q, q0))
    assert q0 <= 1.0 < q


@pytest.mark.parametrize('defect,check,n,m,opt', MEASURED_DEFECTS)
def test_seeded_defect_exceeds_its_allowance_a_hundredfold(defect, check, n, m, opt):
    a, _ = nr.allowance(check, n, m)
    e = nr.restatement_errors(check, n, m, defect=defect, **opt)
    print('%s at n = %d m = %d: %s error %.3g = %.3g x the allowance %.3g' % (defect, n, m, check, e, e / a, a))
    assert e > 100.0 * a


def test_plain_chunk_sum_is_not_a_defect():
    """Kahan's compensation of the chunk Gram sum replaced by nothing: a different order of the same sums, inside M2."""
    a, _ = nr.allowance('M2', nr.F32_N, 129)
    e = nr.restatement_errors('M2', nr.F32_N, 129, defect='no_kahan', gram_rows=256)
    print('no_kahan: %.3g of the allowance' % (e / a))
    assert e <= a


def test_grid_reaches_every_branch():
    """The host's branch arithmetic (gram_tn, tall_trsm, precon_apply_device) restated and walked over the grid."""
    g = {c: nr.gram_plan(*c) for c in nr.GRAM_TILES}
    assert all(p['S'] == 1 for p in g.values())
    assert g[(12, 5)]['whole_k_tiles'] == [0] and g[(12, 5)]['k_tail'] == [12] and g[(12, 5)]['full'] == {(0, 0): False}
    assert g[(63, 5)]['whole_k_tiles'] == [3] and g[(63, 5)]['k_tail'] == [15]
    assert g[(144, 127)]['full'] == {(0, 0): False} and g[(144, 127)]['k_tail'] == [0]
    assert g[(144, 128)]['full'] == {(0, 0): True} and g[(144, 128)]['k_tail'] == [0]     # syrk_tn_tile<true>, no guarded k-tile
    assert g[(150, 129)]['full'] == {(0, 0): True, (1, 0): False, (1, 1): False} and g[(150, 129)]['k_tail'] == [6]
    p = g[(270, 257)]
    assert p['tiles'] == 3 and p['T'] == 6 and sorted(k for k, f in p['full'].items() if f) == [(0, 0), (1, 0), (1, 1)]
    # the split
    n, m = nr.GRAM_SPLIT
    p = nr.gram_plan(n, m, 1)
    assert p['S'] == 2 and p['rows_per'] == 8208 and p['ranges'] == [(0, 8208), (8208, 16392)] and p['k_tail'] == [0, 8]
    assert p['full'] == {(0, 0): True, (1, 0): False, (1, 1): False}
    assert nr.gram_plan(n, m, 0)['S'] == 1
    # the fp32 form's chunk Gram matrices and the CholeskyQR Gram over the stacked rows run syrk_tn_kernel too
    assert [min(256, nr.F32_N - r) for r in range(0, nr.F32_N, 256)] == [256, 256, 82]
    assert [(n + m) % 16 for n, m in nr.QR] == [7, 3]
    # solves
    t = {m: nr.trsm_plan(m, 1) for m in nr.SOLVE_M + (1, 2)}
    assert [t[m][0]['branch'] for m in (64, 128, 512)] == ['panel'] * 3 and all(len(t[m]) == 1 for m in (63, 64, 65, 128, 512))
    assert t[63][0]['widths'] == [63] and t[65][0]['widths'] == [64, 1] and t[1][0]['widths'] == [1] and t[2][0]['widths'] == [2]
    assert [(s['branch'], s['widths']) for s in t[513]] == [('panel', []), ('trsm64', [1])]
    assert [(s['branch'], s['widths']) for s in t[525]] == [('panel', []), ('trsm64', [13])]
    assert [(s['branch'], s['nb']) for s in t[576]] == [('panel', 512), ('panel', 64)]
    for m in (513, 525, 576):
        assert [s['left_update'] for s in nr.trsm_plan(m, 1)] == [False, True]
        assert [s['right_update'] for s in nr.trsm_plan(m, 0)] == [True, False]
        assert not any(s['right_update'] for s in nr.trsm_plan(m, 1)) and not any(s['left_update'] for s in nr.trsm_plan(m, 0))
    assert nr.SOLVE_N % 16 == 2
    # fp64 GEMVs
    a = {c: nr.apply_plan(c[0], c[1], 0) for c in nr.GEMV64}
    p = a[(2100, 131)]
    assert p['parts'] == [2048, 52] and p['rem8'] == [0, 4] and p['odd_col'] == 1 and 2100 % 4 == 0
    p = a[(594, 513)]
    assert p['col_blocks'] == 2 and p['threads_in_last_block'] == 1 and p['odd_col'] == 1 and p['unrolled'] == 64 and p['tail'] == 0
    p = a[(594, 512)]
    assert p['col_blocks'] == 1 and p['odd_col'] == 0 and p['unrolled'] == 64 and p['tail'] == 0
    p = a[(594, 525)]
    assert p['unrolled'] == 64 and p['tail'] == 6 and p['odd_col'] == 1 and p['rem8'] == [594 % 8]
    assert a[(63, 2)]['unrolled'] == 0 and a[(63, 2)]['tail'] == 1 and 63 % 4 == 3
    assert a[(13, 1)]['unrolled'] == 0 and a[(13, 1)]['tail'] == 0 and a[(13, 1)]['odd_col'] == 1
    # fp32 form
    assert [nr.apply_plan(nr.F32_N, m, 3)['mod4'] for m in nr.F32_M[:4]] == [1, 2, 3, 0]
    for m in nr.F32_M[:4]:
        p = nr.apply_plan(nr.F32_N, m, 3)
        assert p['unrolled'] == 0 and p['tail'] == 33 and p['parts'] == [594] and p['rem8'] == [2]
    p = nr.apply_plan(nr.F32_N, 525, 3)
    assert p['unrolled'] == 64 and p['tail'] == 4 and p['mod4'] == 1
    p = nr.apply_plan(nr.F32_N, 129, 3, f32_rows_per=64)
    assert p['nparts'] == 10 and p['parts'][-1] == 18 and p['rem8'][-1] == 2
    assert [nr.apply_plan(nr.F32_N, 129, 3, f32_rw=rw)['rem_rows'] for rw in (1, 2, 4)] == [2, 2, 2]
    assert [nr.apply_plan(nr.F32_N, 129, 3, f32_rw=rw)['rem_rw'] for rw in (1, 2, 4)] == [0, 0, 2]
    # matrix-free: Z is m x m, 512 rows per part
    assert (nr.MF['m'] + 511) // 512 == 2 and nr.apply_plan(nr.MF['m'], nr.MF['m'], 0)['col_blocks'] == 2


def test_what_the_grid_does_not_reach():
    """Out of scope, stated in DESIGN.md: the 1024-column block boundary of gemv_t_part_f32_kernel and m > 576 (long-double
    references too slow for a test of a few seconds); the empty row range of the split Gram (unreachable: rows_per <=
    n / S + 16, so the last range starts at (S - 1) rows_per < n whenever 16 (S - 1) < n / S, and gram_tn keeps
    n / S >= 8192 with S <= 8)."""
    assert max(m for _, m, _, _ in nr.grid_cases()) == 576 and nr.MF['m'] <= 576
    assert all(nr.apply_plan(nr.F32_N, m, 3)['col_blocks'] == 1 for m in nr.F32_M)
    for n, m, _, _ in nr.grid_cases():
        assert all(b > a for a, b in nr.gram_plan(n, m)['ranges'])
    for S in range(2, 9):  # the smallest n that splits S ways, and one row more than a multiple of 16 S
        for n in (8192 * S, 8192 * S + 1, 8192 * S + 16 * S + 1):
            p = nr.gram_plan(n, 129 * S)  # (T < 8192 for any of these m)
            if p['S'] >= 2:
                assert all(b > a for a, b in p['ranges']), (n, p['S'])


@pytest.mark.parametrize('m', nr.F32_M)
def test_fp32_form_is_accepted_on_the_grid(m):
    """build_f32_form keeps the form only if the smallest squared pivot of L_G reaches pcg.f32_min_pivot = 1e-7."""
    r = _restated(nr.F32_N, m, 'a', nr.LAM)
    for rows in (2048, 256):
        _, _, piv = nr.f32_form_f64(r['X2'], r['L'], nr.LAM, gram_rows=rows)
        assert piv >= 1e-7
    print('m = %d: smallest squared pivot of L_G %.3g' % (m, piv))


def test_matrix_free_case():
    """The matrix-free case runs on a really assembled kernel matrix: its K_mm must be factorable without jitter and well
    enough conditioned that the form's own error (eps cond(K_mm)) leaves the allowance far below any defect.  30 frames of
    6 atoms, n = 540, cannot supply 513 independent columns (rank 360)."""
    from oracle import gdml_oracle as orc

    ds = orc.synth_dataset(6, 30, seed=1)
    xd, gd = orc.desc_from_R(ds['R'].reshape(30, -1))
    tp = orc.tril_perms_from_atom_perms(np.arange(6)[None])
    K30 = orc.assemble_K(xd, gd, orc.tril_perms_lin_from_tril_perms(tp), nr.MF['sig'])
    assert np.linalg.matrix_rank(K30) == 30 * 12
    for s in nr.SEEDS:
        _, _, _, K_nm, idx, _ = nr.mf_system(s)
        ev = np.linalg.eigvalsh(-K_nm[idx])
        print('seed %d: cond(K_mm) = %.3g' % (s, ev[-1] / ev[0]))
        assert ev[0] > 0 and ev[-1] / ev[0] <= 1e6
        assert np.bincount(idx // 18).max() <= nr.MF['cols_per_frame']
    a, errs, _, _ = nr.mf_allowance()
    print('M5 allowance %.3g (restatement errors %s)' % (a, ', '.join('%.3g' % e for e in errs)))
    assert a < 1e-8
    # a defect of the matrix-free path: the second row part of Z^T t (row 512) dropped
    xd, gd, tp, K_nm, idx, Kv = nr.mf_system(0)
    v = nr.vec(len(K_nm), 0)
    r = nr.nys_f64(K_nm, idx, nr.MF['lam'])
    Z = nr._trsm_f64(nr._trsm_f64(np.eye(len(idx)), r['L_mm']), r['L'])
    t = Z[:512].T @ Kv(v)[idx][:512]
    e = np.zeros(len(v))
    e[idx] = Z @ t
    bad = (Kv(e) - v) / nr.MF['lam']
    assert nr.rel_err(bad, nr.mf_allowance()[2]) > 100.0 * a

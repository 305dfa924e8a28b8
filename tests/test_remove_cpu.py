"""Removing training points from a Cholesky factor without a GPU: the blocked Householder sweep of tests/_remove_ref.py (what
csrc/remove.hip does) against SciPy's Cholesky of the system of the kept points -- the factor, the posterior covariances, the
solve -- the meaningfulness cap of every fixture / removal set on the reduced reference, and the binding."""
import functools
import os
import sys

import numpy as np
import pytest
import scipy.linalg as sla

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _extend_ref as er  # noqa: E402
import _remove_ref as rr  # noqa: E402
import _tol  # noqa: E402
import _uncertainty_ref as ur  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
CASES = ['n5_p4', 'n10_p2_pbc', 'n4_p6_pbc', 'cfg0_n9_p6']  # (the two largest fixtures of the GPU test cost minutes on a CPU)
SET_KEYS = ['one', 'three', 'seq']


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name + '.npz')))


@functools.lru_cache(maxsize=None)
def _fix(name):
    """Tables, queries, the oracle's matrices of the full system and SciPy's factor of it, once per fixture."""
    g = er.synth_fixture() if name == 'synth' else _load(name)
    t = er.tables(g)
    Rq = ur.queries(g)
    full = er.full_reference(t, Rq, with_loo=False)
    return t, Rq, full, sla.cholesky(full['A'], lower=True, check_finite=False)


def _check(name, calls, chunk=64, fresh=False):
    """The sweep, one call after another, against SciPy on the kept points; returns the swept factor.  fresh: the reference
    is _extend_ref.full_reference on the kept points' tables, assembled anew, and the principal submatrix that
    _remove_ref.reduced_reference takes instead (every other case, the GPU tests) is compared with it."""
    t, Rq, full, L = _fix(name)
    n3 = t['R'].shape[1]
    M = len(t['R'])
    for idx in calls:
        L = rr.remove(L, n3, idx, chunk)
    keep = rr.keep_after(M, calls)
    ref = rr.reduced_reference(full, t, keep, with_loo=False)
    if fresh:
        sub = ref
        ref = er.full_reference(rr.subset(t, keep), Rq, with_loo=False)
        assert np.abs(ref['A'] - sub['A']).max() <= 1e-12 * np.abs(ref['A']).max()
        assert np.abs(ref['Kx'] - sub['Kx']).max() <= 1e-12 * np.abs(ref['Kx']).max()
        assert np.abs(ref['tol'] / sub['tol'] - 1.0).max() <= 1e-6 and np.array_equal(ref['y'], sub['y'])
    A, y = ref['A'], ref['y']
    n = len(A)
    assert n == n3 * len(keep) and L.shape == (n, n) and np.array_equal(L, np.tril(L))
    cap = max(ref['tol'][q] / np.diag(ref['Sig'][q]).min() for q in range(len(Rq)))
    for q in range(len(Rq)):  # a condition on the reference values, not a measurement
        assert ref['tol'][q] <= 0.1 * np.diag(ref['Sig'][q]).min(), (q, cap)
    assert (np.diag(L) > 0.0).all()
    gam = (n + 1) * ur.EPS / (1 - (n + 1) * ur.EPS)
    back = np.linalg.norm(np.tril(A - L @ L.T)) / np.linalg.norm(np.tril(np.abs(L) @ np.abs(L).T))
    assert back <= 4.0 * gam
    Sig = er.cov_from_factor(L, ref['Kx'], ref['kqq'])
    ratio = max(np.abs(Sig[q] - ref['Sig'][q]).max() / ref['tol'][q] for q in range(len(Rq)))
    a = sla.cho_solve((L, True), y, check_finite=False)
    res = np.linalg.norm(A @ a - y) / np.linalg.norm(y)
    print('%s %s  backward error %.3g of gamma  max|dSig| / tol_q %.2e  residual %.2e (bound %.2e)  cap %.3g' % (
        name, calls, back / gam, ratio, res, _tol.solve_tol(A, a, y), cap))
    assert ratio <= 1e-2
    assert res <= _tol.solve_tol(A, a, y)
    return L


@pytest.mark.parametrize('key', SET_KEYS)
@pytest.mark.parametrize('name', CASES)
def test_sweep_equals_cholesky_of_the_kept_points(name, key):
    """Every removal set of the GPU test: the swept factor is a Cholesky factor of A_kept to the textbook backward error
    |A - L L^T| <= 4 gamma_(n+1) |L| |L^T| (Frobenius norm over the lower triangle, as in test_extend_cpu: the transformations
    are orthogonal, the factor 4 covers the accumulated reflectors and the product), its diagonal is positive, the covariances
    from it agree with those from SciPy's factor within a hundredth of the derived bound tol_q, the solve meets the project's
    residual contract, and the queries pass the meaningfulness cap on the REDUCED reference.  For the set `one` the reference
    is assembled anew from the kept points' tables; the other sets take the principal submatrix of the full system's matrix,
    which that case shows to be the same to rounding."""
    _check(name, rr.sets_of(len(_fix(name)[0]['R']))[key], fresh=key == 'one')


def test_slices_of_one_point_agree_with_the_default():
    """chunk = 1 (three sweeps of 3N columns) against the default (one sweep) on the set `three`: both are factors of A_kept
    within the bounds above, and they agree to rounding."""
    calls = rr.sets_of(len(_fix('n5_p4')[0]['R']))['three']
    La = _check('n5_p4', calls)
    Lb = _check('n5_p4', calls, chunk=1)
    assert np.abs(La - Lb).max() <= 1e-10 * np.abs(La).max()


def test_truncation_and_a_zero_row():
    """Removing the last point cuts the factor off unchanged; a reflector whose V part is exactly zero is the identity."""
    t, _, _, L = _fix('n5_p4')
    n3, M = t['R'].shape[1], len(t['R'])
    assert np.array_equal(rr.remove(L, n3, [M - 1]), L[:-n3, :-n3])
    Lk, Vk = np.array([[2.0, 0.0], [1.0, 3.0]]), np.array([[0.0, 0.0], [4.0, 0.0]])
    U, T, sgn = rr._panel(Lk, Vk)
    assert T[0, 0] == 0.0 and not U[0].any() and Lk[0, 0] == 2.0 and Lk[1, 0] == 1.0
    assert abs(Lk[1, 1] * sgn[1] - 5.0) < 1e-15 and sgn[0] == 1.0 and sgn[1] == -1.0 and not Vk.any()


def test_synthetic_boundary_case_meets_the_cap():
    """The n = 1800 case of the GPU test with the set `synth`: a removed block straddles column 512, the sweep crosses columns
    1024 and 1536, the last block is ragged (n' = 1746 = 27 x 64 + 18), and the queries pass the cap on the reduced
    reference."""
    s = er.SYNTH
    n3 = 3 * s['N']
    idx = rr.SYNTH_SET[0]
    assert idx[0] * n3 < 512 < (idx[1] + 1) * n3 and idx[1] == idx[0] + 1
    n1 = (s['M'] - len(idx)) * n3
    assert idx[0] * n3 // 64 * 64 < 1024 and n1 > 1536 and n1 % 64 == 18
    _check('synth', rr.SYNTH_SET, fresh=True)


def test_binding():
    import ctypes as C

    from sgdml_amd import _lib
    from sgdml_amd.predict import GDMLPredict

    hdr = open(os.path.join(ROOT, 'include', 'gdml_hip.h')).read()
    assert 'int gdml_factor_remove(gdml_ctx* ctx, const int64_t* idx, int64_t b, int* info);' in hdr
    lib = _lib.load()
    assert 'gdml_factor_remove' in _lib.SIGNATURES and hasattr(lib, 'gdml_factor_remove')
    assert lib.gdml_abi_version() == 4
    info = C.c_int(0)
    assert lib.gdml_factor_remove(None, None, 0, C.byref(info)) == -1
    assert callable(_lib.Context.factor_remove)
    assert callable(GDMLPredict.remove_training_points) and callable(GDMLPredict.export_model)

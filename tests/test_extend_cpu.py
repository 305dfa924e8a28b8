"""Appending training points to a Cholesky factor without a GPU: the bordering of tests/_extend_ref.py (what csrc/extend.hip
does) against SciPy's Cholesky of the full system -- the factor, the posterior covariances, the solve -- the meaningfulness
cap of the synthetic boundary case, and the binding."""
import os
import sys

import numpy as np
import pytest
import scipy.linalg as sla

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _extend_ref as er  # noqa: E402
import _tol  # noqa: E402
import _uncertainty_ref as ur  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
CASES = ['n5_p4', 'n10_p2_pbc', 'n4_p6_pbc', 'cfg0_n9_p6']  # (the two largest fixtures of the GPU test cost minutes on a CPU)


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name + '.npz')))


@pytest.mark.parametrize('name', CASES)
def test_bordering_equals_cholesky_of_the_full_system(name):
    """Every split of the GPU test: the bordered factor is a Cholesky factor of A' to the textbook backward error
    |A' - L' L'^T| <= 4 gamma_(n+1) |L'| |L'^T| (Higham, Accuracy and Stability, thm 10.3, taken in the Frobenius norm over the
    lower triangle; gamma_k = k eps / (1 - k eps); the factor 4 covers the extra triangular solve and product of the
    bordering), the covariances from it agree with those
    from SciPy's factor within a hundredth of the derived bound tol_q, and the solve meets the project's residual contract."""
    g = _load(name)
    t = er.tables(g)
    Rq = ur.queries(g)
    ref = er.full_reference(t, Rq, with_loo=False)
    A, y, n3 = ref['A'], ref['y'], ref['n3']
    n = len(A)
    Lref = sla.cholesky(A, lower=True, check_finite=False)
    gam = (n + 1) * ur.EPS / (1 - (n + 1) * ur.EPS)
    for q in range(len(Rq)):  # a condition on the reference values, not a measurement
        assert ref['tol'][q] <= 0.1 * np.diag(ref['Sig'][q]).min(), q
    for key, steps in er.splits_of(len(t['R'])).items():
        rows = [s * n3 for s in steps]
        L = er.extend(A, n - sum(rows), rows)
        assert L.shape == (n, n) and np.array_equal(L, np.tril(L))
        back = np.linalg.norm(np.tril(A - L @ L.T))  # (the factorisations read the lower triangle of A only)
        assert back <= 4.0 * gam * np.linalg.norm(np.tril(np.abs(L) @ np.abs(L).T)), key
        Sig = er.cov_from_factor(L, ref['Kx'], ref['kqq'])
        ratio = max(np.abs(Sig[q] - ref['Sig'][q]).max() / ref['tol'][q] for q in range(len(Rq)))
        a = sla.cho_solve((L, True), y, check_finite=False)
        res = np.linalg.norm(A @ a - y) / np.linalg.norm(y)
        print('%s %s  max|dSig| / tol_q %.2e   residual %.2e   |dL| / max|L| %.2e' % (
            name, key, ratio, res, np.abs(L - Lref).max() / np.abs(Lref).max()))
        assert ratio <= 1e-2, key
        assert res <= _tol.solve_tol(A, a, y), key


def test_synthetic_boundary_case_meets_the_cap():
    """The n = 1800 case of the GPU test: its queries pass the meaningfulness cap with the reference values alone, and its
    base / new split lies where the docstring of _extend_ref.SYNTH says."""
    s = er.SYNTH
    g = er.synth_fixture()
    t = er.tables(g)
    Rq = ur.queries(g)
    ref = er.full_reference(t, Rq, with_loo=False)
    n3 = 3 * s['N']
    n0, n1 = (s['M'] - s['b']) * n3, s['M'] * n3
    assert 1500 <= n1 <= 3000
    assert n0 // 512 < (n1 - 1) // 512 and s['b'] * n3 > 128  # a panel boundary inside the new columns, more than one row tile
    for q in range(len(Rq)):
        assert ref['tol'][q] <= 0.1 * np.diag(ref['Sig'][q]).min(), q
    L = er.extend(ref['A'], n0, [s['b'] * n3])
    Sig = er.cov_from_factor(L, ref['Kx'], ref['kqq'])
    assert max(np.abs(Sig[q] - ref['Sig'][q]).max() / ref['tol'][q] for q in range(len(Rq))) <= 1e-2


def test_binding():
    import ctypes as C

    from sgdml_amd import _lib
    from sgdml_amd.predict import GDMLPredict

    hdr = open(os.path.join(ROOT, 'include', 'gdml_hip.h')).read()
    assert 'int gdml_factor_extend(gdml_ctx* ctx, const double* R_desc_new, const double* R_d_desc_new, int64_t b, int* info);' in hdr
    lib = _lib.load()
    assert 'gdml_factor_extend' in _lib.SIGNATURES and hasattr(lib, 'gdml_factor_extend')
    assert lib.gdml_abi_version() == 4
    info = C.c_int(0)
    assert lib.gdml_factor_extend(None, None, None, 0, C.byref(info)) == -1
    assert callable(_lib.Context.factor_extend)
    assert callable(GDMLPredict.add_training_points) and callable(GDMLPredict.export_model)

"""Leave-one-out errors from the Cholesky factor without a GPU: the identity route of tests/_loo_ref.py (Cholesky -> L^-1 ->
block Gram -> block solve, what csrc/loo.hip does) against brute force (one Cholesky solve per fold on the matrix with the
point removed), log det A, the invariants, the end-to-end meaning with the oracle's predictor, and the binding."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _loo_ref as lr  # noqa: E402
import _uncertainty_ref as ur  # noqa: E402
from oracle import gdml_oracle as orc  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
SMALL = ['n6_p1', 'n5_p4', 'n9_p1', 'n4_p6_pbc', 'n10_p2_pbc']  # at their stored lam, every fold
BIG = ('cfg0_n9_p6', 1e-4, list(range(0, 200, 25)))  # lam = 1e-4 instead of the stored 1e-10 (there the bound exceeds r)


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name + '.npz')))


def _check_identity_vs_brute(name, lam, folds):
    A, y, n3, _ = lr.system(_load(name), lam)
    M = len(A) // n3
    folds = list(range(M)) if folds is None else folds
    r, C, _ = lr.loo_identity(A, y, n3)
    rb, _ = lr.loo_brute(A, y, n3, folds)
    b = lr.Bounds(A, y, n3)
    for k, j in enumerate(folds):
        t1 = b.terms(j)[0]
        d = np.abs(rb[k] - r[j]).max()
        print('%s fold %d  |identity - brute| %.2e  = %.3g of the first term of tol_j' % (name, j, d, d / t1))
        assert d <= t1, j


@pytest.mark.parametrize('name', SMALL)
def test_identity_equals_brute_force(name):
    _check_identity_vs_brute(name, None, None)


def test_identity_equals_brute_force_cfg0():
    _check_identity_vs_brute(*BIG)


@pytest.mark.parametrize('name', SMALL)
def test_logdet_cov_and_linearity(name):
    A, y, n3, _ = lr.system(_load(name))
    r, C, logdet = lr.loo_identity(A, y, n3)
    sign, ref = np.linalg.slogdet(A)
    assert sign == 1.0 and abs(logdet - ref) <= lr.Bounds(A, y, n3).logdet_tol()
    for j in range(len(C)):
        assert np.abs(C[j] - C[j].T).max() <= 1e-12 * np.abs(C[j]).max()
        assert np.linalg.eigvalsh(0.5 * (C[j] + C[j].T)).min() > 0.0
    b = lr.Bounds(A, y, n3)
    r3, C3, _ = lr.loo_identity(A, -3.0 * y, n3)  # two solves of the same system: within the Cholesky term of the bound
    for j in range(len(C)):
        assert np.abs(r3[j] + 3.0 * r[j]).max() <= 3.0 * b.terms(j)[0], j
    assert np.array_equal(C3, C)


def test_end_to_end_meaning():
    """F_j - std r_j is the force the oracle's predictor gives at x_j for a model trained on the other M - 1 points with the
    same sig, lam and permutations.  (A prediction is linear in the labels, so the fold's own std cancels.)"""
    g = _load('n6_p1')
    A, y, n3, std = lr.system(g)
    R_train, x, gd, tp, lat = ur.fixture_tables(g)
    M, sig, lam = len(x), float(g['sig']), float(g['lam'])
    F = np.asarray(g['F_train'], dtype=np.float64).reshape(M, n3)
    r, _, _ = lr.loo_identity(A, y, n3)
    b = lr.Bounds(A, y, n3)
    for j in range(M):
        keep = np.r_[0:j, j + 1:M]
        K = orc._full_K(x[keep], gd[keep], tp, sig, False)
        alphas, used_lu = orc.analytic_solve(K, F[keep].ravel(), lam)
        assert not used_lu
        JA = orc.d_desc_dot_vec(gd[keep], alphas.reshape(M - 1, n3))
        _, Fj = orc.predict_from_desc(x[j:j + 1], gd[j:j + 1], x[keep], JA, tp, sig)
        floor = 50 * np.finfo(float).eps * np.abs(JA).max() * 5.0 / (3 * sig**2) * np.sqrt((M - 1) * len(tp)) * max(1.0, np.abs(gd).max())
        d = np.abs(F[j] - std * r[j] - Fj[0]).max()
        print('fold %d  |F_j - std r_j - F_pred| %.2e  bound %.2e' % (j, d, std * lr.loo_tol(A, y, n3, j, b) + floor))
        assert d <= std * lr.loo_tol(A, y, n3, j, b) + floor, j


def test_binding():
    import ctypes as C

    from sgdml_amd import _lib
    from sgdml_amd.predict import GDMLPredict
    from sgdml_amd.sweep import sigma_sweep

    lib = _lib.load()
    assert 'gdml_loo' in _lib.SIGNATURES and hasattr(lib, 'gdml_loo')
    assert lib.gdml_abi_version() == 4
    ld, info = C.c_double(0.0), C.c_int(0)
    assert lib.gdml_loo(None, None, 0, 0, None, None, C.byref(ld), C.byref(info)) == -1
    assert callable(_lib.Context.loo) and callable(GDMLPredict.loo_errors)
    with pytest.raises(ValueError):
        sigma_sweep(None, None, 1, 1, 1, select='nonsense')
    from sgdml_amd.train import GDMLTrain

    t = GDMLTrain()
    try:
        assert t.loo is False  # off by default
    finally:
        del t

"""Posterior force covariance without a GPU: the NumPy restatement (tests/_uncertainty_ref.py) against the oracle's kernel
matrix on the combined set (training points and queries, an independent second route: the oracle treats the queries as ordinary
points), the invariants of the covariance, and the binding of the new entry points."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _uncertainty_ref as ur  # noqa: E402
from oracle import gdml_oracle as orc  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
CASES = ['n5_p4', 'n9_p1', 'n10_p2_pbc']


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name + '.npz')))


def _setup(name):
    g = _load(name)
    R_train, x, gd, tp, lat = ur.fixture_tables(g)
    return g, R_train, x, gd, tp, lat, float(g['sig']), float(g['lam'])


@pytest.mark.parametrize('name', CASES)
def test_cross_rows_match_oracle_on_the_combined_set(name):
    g, R_train, x, gd, tp, lat, sig, _ = _setup(name)
    Rq = ur.queries(g)
    Kx, kqq = ur.cross_rows(Rq, x, gd, tp, sig, lat)
    xa, ga = orc.desc_from_R(np.concatenate([R_train, Rq]), lat)
    K_all = orc._full_K(xa, ga, tp, sig, False)
    M, n3 = R_train.shape
    tol = 1e-13 * np.abs(K_all).max()
    for q in range(len(Rq)):
        rows = slice((M + q) * n3, (M + q + 1) * n3)
        assert np.abs(Kx[q] - K_all[rows, :M * n3]).max() <= tol, q
        assert np.abs(kqq[q] - K_all[rows, rows]).max() <= tol, q


@pytest.mark.parametrize('name', CASES)
def test_posterior_cov_invariants(name):
    g, R_train, x, gd, tp, lat, sig, lam = _setup(name)
    Rq = ur.queries(g)
    A = ur.system_matrix(x, gd, tp, sig, lam)
    Kx, kqq = ur.cross_rows(Rq, x, gd, tp, sig, lat)
    Sig = ur.posterior_cov(Kx, kqq, A)
    nA = np.linalg.norm(A, 2)
    for q in range(len(Rq)):
        tol = ur.cov_tol(Kx[q], kqq[q], A, nA)
        assert np.abs(Sig[q] - Sig[q].T).max() <= tol
        assert np.linalg.eigvalsh(0.5 * (Sig[q] + Sig[q].T)).min() >= -tol * Sig.shape[1]
        assert np.all(np.diag(Sig[q]) <= np.diag(-kqq[q]) + tol)
    # a training geometry: Sig = lam I - lam^2 [A^-1]_ii exactly, so 0 <= diag <= lam
    tol = ur.cov_tol(Kx[-1], kqq[-1], A, nA)
    d = np.diag(Sig[-1])
    assert np.all(d >= -tol) and np.all(d <= lam + tol)


@pytest.mark.parametrize('name', ['n5_p4', 'n9_p1'])
def test_posterior_cov_translation_and_permutation(name):
    g, R_train, x, gd, tp, lat, sig, lam = _setup(name)
    Rq = ur.queries(g)[:2]
    N = Rq.shape[1] // 3
    A = ur.system_matrix(x, gd, tp, sig, lam)
    nA = np.linalg.norm(A, 2)
    Kx, kqq = ur.cross_rows(Rq, x, gd, tp, sig)
    Sig = ur.posterior_cov(Kx, kqq, A)
    tols = [ur.cov_tol(Kx[q], kqq[q], A, nA) for q in range(len(Rq))]
    # rigid translation (the descriptor depends on differences only; they round differently, hence the tolerance)
    Rs = (Rq.reshape(len(Rq), N, 3) + np.array([0.7, -1.3, 0.4])).reshape(len(Rq), -1)
    Sig_s = ur.posterior_cov(*ur.cross_rows(Rs, x, gd, tp, sig), A)
    for q in range(len(Rq)):
        assert np.abs(Sig_s[q] - Sig[q]).max() <= 2 * tols[q]
    # a permutation of the model applied to the query's atoms permutes rows and columns of Sig
    perm = np.asarray(g['perms'])[-1]
    Rp = Rq.reshape(len(Rq), N, 3)[:, perm].reshape(len(Rq), -1)
    Sig_p = ur.posterior_cov(*ur.cross_rows(Rp, x, gd, tp, sig), A)
    idx = (3 * perm[:, None] + np.arange(3)).ravel()
    for q in range(len(Rq)):
        assert np.abs(Sig_p[q] - Sig[q][np.ix_(idx, idx)]).max() <= 2 * tols[q]


def test_binding():
    import ctypes as C

    from sgdml_amd import _lib
    from sgdml_amd.predict import GDMLPredict

    names = ['gdml_uncert_prepare', 'gdml_uncert_release', 'gdml_uncert_cross', 'gdml_predict_cov', 'gdml_predict_cov_dev']
    lib = _lib.load()
    for nm in names:
        assert nm in _lib.SIGNATURES
        assert hasattr(lib, nm)
    assert lib.gdml_abi_version() == 4
    info = C.c_int(0)
    assert lib.gdml_uncert_prepare(None, 10.0, 1e-10, C.byref(info)) == -1
    assert lib.gdml_uncert_release(None) == -1
    assert lib.gdml_uncert_cross(None, None, 0, None, None, None, None) == -1
    assert lib.gdml_predict_cov(None, None, 0, None, None, 0, None) == -1
    assert lib.gdml_predict_cov_dev(None, None, 0, None, None, 1, None) == -1
    for nm in ['prepare_uncertainty', 'predict_uncertainty', 'release_uncertainty']:
        assert callable(getattr(GDMLPredict, nm))
    for nm in ['uncert_prepare', 'uncert_release', 'uncert_cross', 'predict_cov', 'predict_cov_dev']:
        assert callable(getattr(_lib.Context, nm))

"""The low-latency covariance path (csrc/uncert_few.hip) without a GPU: its bindings, and what its inverted 64 x 64 diagonal
blocks cost in accuracy -- the NumPy restatement of the blocked solve (tests/_uncert_few_ref.py: the kernels' block sizes and
order) against scipy's triangular solve, within the bound the GPU test uses (_uncertainty_ref.cov_tol).  All fixtures but
n10_p2_pbc (1e-4) have lam = 1e-10, so a conditioning problem of the inverses would show here."""
import inspect
import os
import sys

import numpy as np
import pytest
import scipy.linalg as sla

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _uncert_few_ref as fr  # noqa: E402
import _uncertainty_ref as ur  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
CASES = ['n5_p4', 'n10_p2_pbc', 'n4_p6_pbc', 'cfg0_n9_p6', 'cfg1_n21_m100', 'cfg3_n42_p27_m60']


@pytest.mark.parametrize('name', CASES)
def test_blocked_solve_with_inverted_diagonal_blocks(name):
    g = dict(np.load(os.path.join(GOLDEN, name + '.npz')))
    _, x, gd, tp, lat = ur.fixture_tables(g)
    Rq = ur.queries(g)[[0, 3, 6]]  # two test geometries and the training geometry
    A = ur.system_matrix(x, gd, tp, float(g['sig']), float(g['lam']))
    Kx, kqq = ur.cross_rows(Rq, x, gd, tp, float(g['sig']), lat)
    Sig = ur.posterior_cov(Kx, kqq, A)
    nA = float(sla.eigvalsh(A, subset_by_index=[len(A) - 1, len(A) - 1])[0])
    L = sla.cholesky(A, lower=True, check_finite=False)
    few = fr.posterior_cov_few(Kx, kqq, L)
    for q in range(len(Rq)):
        tol = ur.cov_tol(Kx[q], kqq[q], A, nA)
        ratio = np.abs(few[q] - Sig[q]).max() / tol
        print('%s q=%d  max|dSig| / tol_q = %.3g' % (name, q, ratio))
        assert ratio <= 1.0, (q, ratio)


def test_inverted_blocks_are_inverses():
    rng = np.random.default_rng(3)
    n = 150  # a ragged last block
    Mx = rng.standard_normal((n, n))
    L = np.linalg.cholesky(Mx @ Mx.T + n * np.eye(n))
    inv = fr.invert_diag_blocks(L)
    assert inv.shape == (3, 64, 64)
    for b in range(3):
        w = min(64, n - 64 * b)
        D = L[64 * b:64 * b + w, 64 * b:64 * b + w]
        assert np.abs(inv[b][:w, :w] @ D - np.eye(w)).max() <= 1e-13
        assert np.array_equal(inv[b], np.tril(inv[b]))
        assert np.array_equal(inv[b][w:, w:], np.eye(64 - w))
    X = rng.standard_normal((5, n))
    Z = fr.few_solve(L, X)
    assert np.abs(Z @ L.T - X).max() <= 1e-12 * np.abs(X).max()


def test_binding():
    import ctypes as C

    from sgdml_amd import _lib
    from sgdml_amd.predict import GDMLPredict

    hdr = open(os.path.join(ROOT, 'include', 'gdml_hip.h')).read()
    assert ('int gdml_predict_cov_few(gdml_ctx* ctx, const double* R, int64_t B, const double* lat, const double* lat_inv, '
            'int full,') in hdr
    assert 'int gdml_predict_cov_few_dev(gdml_ctx* ctx, const double* R_dev, int64_t B,' in hdr
    assert '#define GDML_COV_FEW_ROWS %d' % fr.LIMIT in hdr and fr.LIMIT >= 128
    lib = _lib.load()
    for sym in ('gdml_predict_cov_few', 'gdml_predict_cov_few_dev'):
        assert sym in _lib.SIGNATURES and hasattr(lib, sym)
        assert _lib.SIGNATURES[sym] == _lib.SIGNATURES['gdml_predict_cov']
        assert getattr(lib, sym)(None, None, 0, None, None, 0, None) == -1  # NULL context
    assert lib.gdml_abi_version() == 4
    assert callable(_lib.Context.predict_cov_few) and callable(_lib.Context.predict_cov_few_dev)
    sig = inspect.signature(GDMLPredict.predict_uncertainty)
    assert sig.parameters['low_latency'].default is False and sig.parameters['full_cov'].default is False
    assert 'low_latency' in GDMLPredict.predict_uncertainty.__doc__

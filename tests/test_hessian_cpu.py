"""Analytic Hessians, CPU side: the NumPy restatement (tests/_hessian_ref.py) against finite differences of the oracle's
forces and its invariants, and the binding that exposes gdml_predict_hessian."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _hessian_ref as hr  # noqa: E402
from oracle import gdml_oracle as orc  # noqa: E402
from sgdml_amd import _lib  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
FD_CASES = ['n5_p4', 'n5_p2_ecstr', 'n9_p1', 'n10_p2_pbc']


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name + '.npz')))


@pytest.mark.parametrize('which', ['test', 'train'])
@pytest.mark.parametrize('name', FD_CASES)
def test_restatement_matches_finite_differences(name, which):
    g = _load(name)
    model, _, _ = hr.model_from_fixture(g)
    R = (g['R_test'][0] if which == 'test' else g['R_train'][1]).ravel()
    _, _, H = hr.hessian_of_model(model, R[None])
    H_fd = hr.fd_hessian(lambda X: orc.predict(model, X)[1], R, h=1e-4)
    scale = np.abs(H).max()
    assert scale > 0
    assert np.abs(H[0] - H_fd).max() <= 1e-8 * scale


@pytest.mark.parametrize('name', FD_CASES)
def test_restatement_invariants_and_forces(name):
    g = _load(name)
    model, _, _ = hr.model_from_fixture(g)
    N = g['perms'].shape[1]
    R = np.concatenate([g['R_test'][:2].reshape(2, -1), g['R_train'][:1].reshape(1, -1)])
    E, F, H = hr.hessian_of_model(model, R)
    Eo, Fo = orc.predict(model, R)
    assert np.abs(F - Fo).max() <= 1e-12 * np.abs(Fo).max()
    assert np.abs(E - Eo).max() <= 1e-10 * np.abs(Eo).max()  # the oracle sums the energy-constraint term in another order
    for h in H:
        scale = np.abs(h).max()
        assert np.abs(h - h.T).max() <= 1e-13 * scale
        # translation invariance: sum over atoms b of H[i, 3b + c] vanishes for every row i and axis c
        assert np.abs(h.reshape(3 * N, N, 3).sum(axis=1)).max() <= 1e-13 * scale


def test_binding_exposes_hessian():
    for name in ('gdml_predict_hessian', 'gdml_predict_hessian_dev'):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name), name
    assert _lib.load().gdml_abi_version() == 4
    from sgdml_amd.predict import GDMLPredict

    assert callable(getattr(GDMLPredict, 'predict_hessian', None))
    assert callable(getattr(_lib.Context, 'predict_hessian', None))
    assert callable(getattr(_lib.Context, 'predict_hessian_dev', None))


def test_hessian_entry_rejects_a_null_context():
    lib = _lib.load()
    assert lib.gdml_predict_hessian(None, None, 0, None, None, None, None, None) == -1  # GDML_ERR_INVALID
    assert lib.gdml_predict_hessian_dev(None, None, 0, None, None, None, None, None) == -1

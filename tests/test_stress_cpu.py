"""Strain derivative (virial / stress), CPU side: the NumPy restatement (tests/_stress_ref.py) against strain finite differences of
the oracle's energy, its invariants, and the binding that exposes gdml_predict_virial."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _hessian_ref as hr  # noqa: E402
import _stress_ref as sr  # noqa: E402
from oracle import gdml_oracle as orc  # noqa: E402
from sgdml_amd import _lib  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
FD_CASES = ['n10_p2_pbc', 'n9_p1', 'cfg0_n9_p6']
# n4_p6_pbc is ill-conditioned (|alpha| ~ 1e9 cancels down to O(1) outputs): the rounding of rotated or shifted coordinates
# (one ulp of the descriptors) alone moves W by 1.3e-10 resp. 1.2e-10 of max|W|; it gets the bound the GPU parity tests give it
# (tests/test_hessian_gpu.py records the same effect).  Every other fixture keeps 1e-10 (rotation) and 1e-12 (lattice shift).
ROT_TOL = {'n4_p6_pbc': 1e-8}
SHIFT_TOL = {'n4_p6_pbc': 1e-8}


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name + '.npz')))


def _oracle_energy(model):
    def energy(R, lattice):
        m = dict(model)
        m.pop('lattice', None)
        if lattice is not None:
            m['lattice'] = lattice
        return orc.predict(m, R)[0]

    return energy


@pytest.mark.parametrize('name', FD_CASES)
def test_restatement_matches_strain_finite_differences(name):
    """4-point central differences (h = 1e-4) of the oracle's energy, cell and atoms strained together: 1e-8 of max|W|, the
    margin of the Hessian's finite-difference test for the same stencil (measured: at most 7e-11)."""
    g = _load(name)
    model, _, _ = hr.model_from_fixture(g)
    lattice = model.get('lattice')
    for R in g['R_test'][:3].reshape(3, -1):
        W = sr.virial_of_model(model, R[None])[2][0]
        W_fd = sr.fd_virial(_oracle_energy(model), R, lattice, h=1e-4)
        scale = np.abs(W).max()
        assert scale > 0
        err = np.abs(W - W_fd).max() / scale
        print(name, 'strain FD error / max|W| = %.2e' % err)
        assert err <= 1e-8


@pytest.mark.parametrize('name', ['n9_p1', 'n5_p2_ecstr', 'cfg0_n9_p6'])
def test_restatement_is_minus_sum_f_r_without_a_lattice(name):
    g = _load(name)
    model, _, _ = hr.model_from_fixture(g)
    assert 'lattice' not in model
    R = g['R_test'][:3].reshape(3, -1)
    E, F, W = sr.virial_of_model(model, R)
    Eo, Fo = orc.predict(model, R)
    assert np.abs(F - Fo).max() <= 1e-12 * np.abs(Fo).max()
    assert np.abs(E - Eo).max() <= 1e-10 * np.abs(Eo).max()  # the oracle sums the energy-constraint term in another order
    W_fr = -np.einsum('bia,bic->bac', F.reshape(3, -1, 3), R.reshape(3, -1, 3))
    # sum_k F_x[k] g_k (x) (r_i - r_j) regrouped by atoms: rounding of 3 N (N - 1) / 2 summands of size <= max|f| max|r|
    scale = np.abs(F).max() * np.abs(R).max() * R.shape[1]
    assert np.abs(W - W_fr).max() <= 1e-13 * scale


@pytest.mark.parametrize('name', FD_CASES + ['n5_p2_ecstr', 'n4_p6_pbc'])
def test_restatement_invariants(name):
    g = _load(name)
    model, _, _ = hr.model_from_fixture(g)
    lattice = model.get('lattice')
    R = g['R_test'][:3].reshape(3, -1)
    E, F, W = sr.virial_of_model(model, R)
    scale = np.abs(W).max()
    # symmetric (angular-momentum balance: every term is F_x[k] d_k (x) d_k / |d_k|^3)
    assert np.abs(W - W.transpose(0, 2, 1)).max() <= 1e-13 * scale
    # a rotation of positions and lattice rotates W
    rng = np.random.default_rng(5)
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    Rq = (R.reshape(3, -1, 3) @ Q.T).reshape(3, -1)
    Eq, Fq, Wq = sr.virial_of_model(model, Rq, None if lattice is None else Q @ lattice)
    assert np.abs(Wq - Q @ W @ Q.T).max() <= ROT_TOL.get(name, 1e-10) * scale
    assert np.abs(Eq - E).max() <= 1e-10 * np.abs(E).max()
    if lattice is not None:
        # shifting one atom by a lattice vector changes the minimum-image integers only
        Rs = R.reshape(3, -1, 3).copy()
        Rs[:, 1, :] += lattice[:, 0] - 2.0 * lattice[:, 2]
        _, _, Ws = sr.virial_of_model(model, Rs.reshape(3, -1))
        assert np.abs(Ws - W).max() <= SHIFT_TOL.get(name, 1e-12) * scale


def test_binding_exposes_virial():
    for name in ('gdml_predict_virial', 'gdml_predict_virial_dev'):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name), name
    assert _lib.load().gdml_abi_version() == 4
    from sgdml_amd.predict import GDMLPredict

    for name in ('predict_virial', 'predict_stress'):
        assert callable(getattr(GDMLPredict, name, None))
    assert callable(getattr(_lib.Context, 'predict_virial', None))
    assert callable(getattr(_lib.Context, 'predict_virial_dev', None))


def test_virial_entry_rejects_a_null_context():
    lib = _lib.load()
    assert lib.gdml_predict_virial(None, None, 0, None, None, None, None, None) == -1  # GDML_ERR_INVALID
    assert lib.gdml_predict_virial_dev(None, None, 0, None, None, None, None, None) == -1


def test_lattice_argument_is_validated_without_a_gpu():
    from sgdml_amd.predict import check_lattice

    lat = np.diag([3.0, 4.0, 5.0])
    got, inv = check_lattice(lat)
    assert np.array_equal(got, lat) and np.allclose(inv @ lat, np.eye(3))
    for bad in (np.eye(2), np.ones(9), np.zeros((3, 3)), np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]]),
                np.full((3, 3), np.nan)):
        with pytest.raises(ValueError):
            check_lattice(bad)

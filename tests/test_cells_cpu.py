"""CPU-side checks of prediction with one lattice per geometry (gdml_predict_virial_cells, csrc/predict.hip and csrc/desc.hip;
predict(..., lattices=)): the library surface and the argument errors that need no device."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from sgdml_amd import _lib  # noqa: E402
from sgdml_amd.predict import GDMLPredict  # noqa: E402

NEW = ('gdml_predict_virial_cells', 'gdml_predict_virial_cells_dev', 'gdml_cell_relax_run')


def test_library_exports_the_entries_and_the_abi_version_stays():
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and getattr(lib, name) is not None
    assert lib.gdml_abi_version() == 4
    header = open(os.path.join(ROOT, 'include', 'gdml_hip.h')).read()
    for name in NEW:
        assert 'int %s(' % name in header


def test_null_context_is_invalid_before_anything_else():
    lib = _lib.load()
    R, lats, W = np.zeros((1, 9)), np.eye(3)[None].copy(), np.zeros((1, 3, 3))
    for fn in (lib.gdml_predict_virial_cells, lib.gdml_predict_virial_cells_dev):
        assert fn(None, _lib._ptr(R), 1, _lib._ptr(lats), _lib._ptr(lats), None, None, _lib._ptr(W)) == _lib.ERR_INVALID
        assert fn(None, None, 1, None, None, None, None, None) == _lib.ERR_INVALID


def test_python_rejects_bad_lattices_before_any_call():
    check = GDMLPredict._lats_and_invs
    lat = np.array([[5.0, 0.3, 0.0], [0.0, 4.0, 0.2], [0.1, 0.0, 6.0]])
    lats, invs = check(np.stack([lat, 1.1 * lat]), 2)
    assert lats.shape == invs.shape == (2, 3, 3)
    for b in range(2):
        assert np.abs(invs[b] @ lats[b] - np.eye(3)).max() <= 1e-14
    with pytest.raises(ValueError, match='either'):
        check(np.stack([lat, lat]), 2, lattice=lat)  # mutually exclusive
    for bad in (lat, np.stack([lat] * 3), np.zeros((2, 3, 4)), np.zeros((2, 9))):
        with pytest.raises(ValueError, match='lattices must be'):
            check(bad, 2)
    singular = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]])
    with pytest.raises(ValueError, match=r'lattices\[1\]'):
        check(np.stack([lat, singular]), 2)
    with pytest.raises(ValueError, match=r'lattices\[0\]'):
        check(np.stack([np.full((3, 3), np.nan), lat]), 2)

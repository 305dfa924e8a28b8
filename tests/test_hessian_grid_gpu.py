"""Analytic Hessians on the GPU (csrc/predict_hess.hip) over a grid of synthetic models: every projection variant at both sides
of every switch point of the dispatch, and every ragged batch slice, row chunk, row group and row split of the host's plan
(tests/_hessian_ref.py:hess_plan; tests/test_hessian_cpu.py asserts what the grid reaches), against a long-double reference
(hessian_ld).  Measured error / bound per case: tools/hessian_grid_parity.py, profiles/hessian_grid_parity.json."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _hessian_ref as hr  # noqa: E402
from oracle import gdml_oracle as orc  # noqa: E402
from sgdml_amd.predict import GDMLPredict  # noqa: E402

pytestmark = pytest.mark.gpu

_preds = {}


def _predictor(case):
    """One resident predictor at a time: consecutive tests on one model share it."""
    key = tuple(sorted(case.items()))
    if key not in _preds:
        _preds.clear()
        _preds[key] = GDMLPredict(hr.grid_model(**case)[0])
    return _preds[key]


def _check(case, B, generic=0, chunk_rows=0):
    m = hr.grid_measure(_predictor(case), case, B, generic, chunk_rows)
    print(case, B, generic, chunk_rows, m)
    assert m['h'] <= 1.0  # max|H - H_ld| <= 1e-10 max|H_ld| per geometry
    assert m['f'] <= 1.0  # 1e-10 max|F_ld|
    assert m['e'] <= 1.0  # 1e-10 max(1, |E_ld|)
    assert m['symmetric']  # the epilogue writes one value to both triangles
    assert m['sum_rule'] <= 1.0  # translation invariance, 1e-12 max|H|
    assert m['duplicates_equal'] and m['repeat_equal']  # fixed summation orders: bit-reproducible
    assert m['f_predict'] <= 1.0 and m['e_predict'] <= 1.0  # E and F are those of predict()


@pytest.mark.parametrize('N', hr.SIZE_N)
def test_hessian_grid_sizes(N):
    """Two queries, an unseen geometry and training geometry 0 (the n = 0 branch of gam; with P = 2 its atoms 0 and 1 are
    exchanged, so that the zero distance falls on a non-identity table row)."""
    assert np.finfo(np.longdouble).eps < 1e-18
    _check(hr.size_case(N), 2)


@pytest.mark.parametrize('generic', [0, 1])  # varies fastest: both runs of a case share the resident model
@pytest.mark.parametrize('MP,B,chunk_rows', hr.ROW_CASES)
@pytest.mark.parametrize('N', hr.ROW_N)
def test_hessian_grid_rows_and_batches(N, MP, B, chunk_rows, generic):
    """Row chunks, row groups, row splits and batch slices at N = 12 (wavefront variant) and N = 33 (block variant), and both
    with F_x kept in memory (predict.hess_generic = 1)."""
    assert np.finfo(np.longdouble).eps < 1e-18
    _check(hr.row_case(N, MP), B, generic, chunk_rows)


def test_hessian_grid_unsupported_size_leaves_the_context_usable():
    N = hr.N_UNSUPPORTED
    assert hr.hess_plan(N, 3, 2) is None and hr.hess_plan(N - 1, 3, 2) is not None
    model, _, R_query = hr.synth_model(N, 3, seed=N)
    pred = GDMLPredict(model)
    with pytest.raises(NotImplementedError):  # GDML_ERR_UNSUPPORTED: d does not fit the LDS row of the projection
        pred.predict_hessian(R_query[:2])
    E, F = pred.predict(R_query[:2])
    Eo, Fo = orc.predict(model, R_query[:2])
    assert np.abs(F - Fo).max() <= 1e-10 * np.abs(Fo).max()
    assert np.abs(E - Eo).max() <= 1e-10 * max(1.0, np.abs(Eo).max())

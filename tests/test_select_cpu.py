"""CPU side of the greedy selection of training points (csrc/select.hip): the exported symbol, and the properties of the
NumPy/SciPy reference (tests/_select_ref.py) that the GPU tests rest on -- its formulations agree, the cap of the bounds holds
for every case and pool of tests/test_select_gpu.py, the duplicate case shows what the joint rule is for, and the picked gains
never increase (what `prescreen` relies on)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _select_ref as sr  # noqa: E402
from sgdml_amd import _lib  # noqa: E402

SMALL = ['n10_p2_pbc', 'n4_p6_pbc', 'n5_p4']


def test_library_exports_the_entry_point():
    lib = _lib.load()
    assert 'gdml_select_points' in _lib.SIGNATURES and hasattr(lib, 'gdml_select_points')
    assert lib.gdml_abi_version() == 4  # additive change
    assert callable(getattr(_lib.Context, 'select_points'))
    from sgdml_amd.predict import GDMLPredict
    assert callable(getattr(GDMLPredict, 'select_training_points'))


@pytest.mark.parametrize('name', SMALL)
def test_the_formulations_of_the_reference_agree(name):
    """log det differences through the shared leading factor, the block-pivoted Cholesky of the pool's joint covariance and the
    literal difference of two full factorisations: the same picks, gains equal to round-off (1 % of the bound the GPU values
    are held to, whose assembly term alone is 1e-12 max|A| sum|A^-1|)."""
    c = sr.case(name)
    ref = c['ref']
    idx, gain, gain0 = sr.schur_sweep(c['A_U'], c['nT'], c['n3'], c['B'], c['b'], c['lam'])
    assert np.array_equal(idx, ref['idx'])
    assert (np.abs(gain - ref['gain']) <= 0.01 * ref['tol']).all()
    assert (np.abs(gain0 - ref['gain0']) <= 0.01 * ref['tol0']).all()
    for t in range(c['b']):
        for q in (ref['idx'][t], max(q_ for q_ in ref['steps'][t] if q_ != ref['idx'][t])):
            lit = sr.full_logdet_gain(c['A_U'], c['nT'], c['n3'], ref['idx'][:t], q, c['lam'])
            assert abs(lit - ref['steps'][t][q][0]) <= 0.01 * ref['steps'][t][q][1], (t, q)


@pytest.mark.parametrize('name', list(sr.CASES))
def test_the_cap_holds_and_gains_never_increase(name):
    """A condition on the reference alone: at every step the best gain leads the second (exact duplicates of the best aside)
    by ten times the sum of their bounds; and the picked gains are non-increasing (submodularity)."""
    c = sr.case(name)
    ref = c['ref']
    assert len(ref['idx']) == c['b'] and len(set(ref['idx'])) == c['b']
    for t, ratio in enumerate(ref['cap']):
        print('%s  step %d  pick %d  gain %.6g  tol %.3g  gap / (tol + tol) = %s' % (name, t, ref['idx'][t], ref['gain'][t],
                                                                                    ref['tol'][t], ratio))
        assert ratio is not None and ratio >= 10.0, (t, ratio)  # no step may be skipped
    assert (np.diff(ref['gain']) <= 0.0).all()
    for t in range(1, c['b']):  # ... and so is every candidate's gain from step to step, up to its bounds
        for q, (g, tol) in ref['steps'][t].items():
            g_prev, tol_prev = ref['steps'][t - 1][q]
            assert g <= g_prev + tol + tol_prev, (t, q)
    # the duplicate of pool[0] and pool[0] are the same matrix rows: the same gain
    assert abs(ref['gain0'][c['dup']] - ref['gain0'][0]) <= ref['tol0'][0]


def test_the_duplicate_case():
    """n10_p2_pbc at its stored lam, pool R_test[:7] + [R_test[0], R_train[0]], b = 3: ranking by initial gain takes index 7,
    the copy of index 0; the joint rule picks [0, 5, 1]."""
    c = sr.case(sr.duplicate_case())
    ref = c['ref']
    assert sr.CASES['n10_p2_pbc'] == {'lam': None, 'n_test': 7, 'b': 3} and c['lam'] == 1e-4 and c['dup'] == 7
    top = np.argsort(-ref['gain0'], kind='stable')[:3]
    assert set(top) == {0, 7, 5}
    assert list(ref['idx']) == [0, 5, 1]
    assert ref['cap'][0] is not None  # the tie of step 0 is between the two copies only
    # once index 0 is in, its copy only averages the label noise: log det(Sig (Sig + lam I)^-1 + I) <= 3N log 2, less than half
    # of what it was worth alone and below every later pick
    assert ref['steps'][1][7][0] <= c['n3'] * np.log(2.0) and ref['steps'][1][7][0] < 0.5 * ref['gain0'][7]
    assert ref['steps'][2][7][0] < ref['gain'][2]

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


# ---- the grid of tests/test_hessian_grid_gpu.py: its long-double reference against the float64 restatement, and what it reaches

GRID_MODELS = ([('size', N, 0) for N in hr.SIZE_N] + [('rows', N, MP) for N in hr.ROW_N for MP in sorted({c[0] for c in hr.ROW_CASES})]
               + [('p6', 12, 30)])


def _grid_case(axis, N, MP):
    if axis == 'size':
        return hr.size_case(N), 2
    if axis == 'p6':  # the six-permutation group of synth_model, which no grid case uses
        return dict(N=N, M=MP // 6, P=6, with_aE=True, lattice=True, seed=6), 5
    return hr.row_case(N, MP), max(min(B, 5) for mp, B, _ in hr.ROW_CASES if mp == MP)


@pytest.mark.parametrize('axis,N,MP', GRID_MODELS, ids=['%s-n%d-mp%d' % c for c in GRID_MODELS])
def test_restatement_matches_long_double_reference(axis, N, MP):
    """hessian() against hessian_ld() on the distinct geometries of every synthetic model of the grid: 1e-13 of max|H|, max|F|
    and max(1, |E|) (float64 rounding of a sum of M P <= 1024 terms; the two share no code from the geometries on)."""
    assert np.finfo(np.longdouble).eps < 1e-18, 'this host has no extended precision: the reference would be hessian() itself'
    case, n_geoms = _grid_case(axis, N, MP)
    model, R5, _ = hr.grid_model(**case)
    if case['lattice']:
        margin, n_wrap = hr.wrap_margin(np.concatenate([R5, hr.synth_model(**case)[1]]), model['lattice'][0, 0])
        assert margin >= 1e-3 and n_wrap >= (case['M'] + 5) * (N - 1)
    E_ld, F_ld, H_ld = hr.grid_reference(case, n_geoms)
    E, F, H = hr.hessian_of_model(model, R5[:n_geoms])
    for q in range(n_geoms):
        assert np.abs(H[q] - H_ld[q]).max() <= 1e-13 * np.abs(H_ld[q]).max(), q
        assert np.abs(F[q] - F_ld[q]).max() <= 1e-13 * np.abs(F_ld[q]).max(), q
        assert abs(E[q] - E_ld[q]) <= 1e-13 * max(1.0, abs(E_ld[q])), q


def test_long_double_reference_sees_the_zero_distance_row():
    """Query 1 of a grid model is training geometry 0 with atoms 0 and 1 exchanged: its descriptor equals table row (0, p = 1)."""
    case = hr.size_case(12)
    model, R5, _ = hr.grid_model(**case)
    x, _ = orc.desc_from_R(R5[1:2], (model['lattice'], np.linalg.inv(model['lattice'])))
    tp = orc.tril_perms_from_lin(model['tril_perms_lin'], x.shape[1])
    Xp, _ = orc.perm_tables(np.asarray(model['R_desc']).T, model['R_d_desc_alpha'], tp)
    assert np.array_equal(x[0], Xp[1]) and not np.array_equal(x[0], Xp[0])


def _grid_plans():
    return [hr.hess_plan(*a) for a in hr.grid_plan_inputs()]


def test_plan_restates_the_documented_cases():
    """The figures the host code is known to give (N = 33): they pin the restatement, not the grid."""
    p = hr.hess_plan(33, 600, 1)
    assert (p['variant'], p['RG'], p['JS'], p['rps'], p['chunks']) == (('block', 4), 8, 9, [67], [600])
    p = hr.hess_plan(33, 600, 1, chunk_rows=200)
    assert (p['JS'], p['chunks'], p['rps']) == (3, [200, 200, 200], [67, 67, 67])
    p = hr.hess_plan(33, 265, 1, chunk_rows=256)
    assert (p['JS'], p['chunks'], p['rps'], p['empty_splits']) == (4, [256, 9], [64, 3], [0, 1])
    assert hr.hess_plan(12, 130, 3, chunk_rows=40)['chunks'] == [40, 40, 40, 10]
    assert hr.hess_plan(12, 600, 129)['slices'] == [64, 64, 1]
    assert hr.hess_plan(hr.N_UNSUPPORTED, 3, 2) is None and hr.hess_plan(hr.N_UNSUPPORTED - 1, 3, 2) is not None
    # the switch points of the dispatch
    want = {11: ('wave', 1), 12: ('wave', 2), 16: ('wave', 2), 17: ('wave', 4), 23: ('wave', 4), 24: ('wave', 8),
            32: ('wave', 8), 33: ('block', 4), 45: ('block', 4), 46: ('block', 8), 64: ('block', 8), 65: ('block', 16),
            91: ('block', 16), 92: ('block', 32), 128: ('block', 32), 129: ('block', 48), 157: ('block', 48),
            158: ('block', 0), 197: ('block', 0)}
    for N, v in want.items():
        assert hr.hess_plan(N, 3, 2)['variant'] == v, N
    assert [hr.hess_plan(N, 3, 2)['v_lds'] for N in (128, 139, 140, 157)] == [1, 1, 0, 0]


def test_grid_reaches_every_variant_and_panel_edge():
    """What keeps the grid honest when the host code is retuned: every kernel variant and every edge of the four cuts."""
    plans = _grid_plans()
    assert all(p is not None for p in plans)
    has = lambda f: any(f(p) for p in plans)  # noqa: E731
    wave = [p for p in plans if p['variant'][0] == 'wave']
    block = [p for p in plans if p['variant'][0] == 'block' and p['variant'][1] > 0]
    generic = [p for p in plans if p['variant'] == ('block', 0)]
    assert {p['variant'][1] for p in wave} == {1, 2, 4, 8}
    assert {p['variant'][1] for p in block} == {4, 8, 16, 32, 48}
    assert all(p['v_lds'] == 1 for p in block if p['variant'][1] < 48)
    assert {p['v_lds'] for p in block if p['variant'][1] == 48} == {0, 1}
    assert any(p['v_lds'] == 0 and not p['forced'] for p in generic)
    assert any(p['v_lds'] == 1 and p['forced'] for p in generic)
    assert {p['nb'] for p in plans} == set(range(1, 11))
    assert has(lambda p: p['n3'] % 16 == 0) and has(lambda p: p['n3'] % 16 != 0)
    assert has(lambda p: p['n3'] % 64 == 0) and {p['n3'] for p in plans} >= {66, 129, 192}
    assert has(lambda p: p['slices'] == [64, 1]) and has(lambda p: p['slices'] == [64, 64, 1])
    for family in (wave, block, generic):
        assert len({p['RG'] for p in family}) >= 2
        assert any(p['last_group_rows'][-1] < p['RG'] for p in family)
        assert any(p['JS'] == 1 for p in family)
        assert any(p['JS'] > 1 and len(p['chunks']) == 1 for p in family)
        assert any(p['JS'] > 1 and len(p['chunks']) >= 3 and p['chunks'][-1] < p['chunks'][0] for p in family)
        assert any(e > 0 for p in family for e in p['empty_splits'][1:])
        assert any(r == 0 for p in family for r in p['rps_mod16']) and any(r != 0 for p in family for r in p['rps_mod16'])
        assert any(len(p['slices']) > 1 and len(p['chunks']) > 1 for p in family)  # chunks restart in the second slice
    assert {i for p in wave for i in p['idle_waves']} == {0, 1, 2, 3}

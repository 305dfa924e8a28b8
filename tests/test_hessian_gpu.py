"""Analytic Hessians on the GPU (csrc/predict_hess.hip): against the NumPy restatement (tests/_hessian_ref.py), against finite
differences of the GPU predictor's own forces, invariants, determinism, replicas, host slicing and error paths."""
import ctypes as C
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
from sgdml_amd.predict import GDMLPredict  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
CASES = ['n6_p1', 'n5_p4', 'n5_p2_ecstr', 'n9_p1', 'n10_p2_pbc', 'cfg0_n9_p6', 'cfg1_n21_m100', 'cfg3_n42_p27_m60', 'n100_m3',
         'n150_p2_m3', 'n4_p6_pbc']
# n4_p6_pbc is ill-conditioned: reordering its training points in the restatement alone moves H by 8e-11 of max|H|
TOL = {'n4_p6_pbc': 1e-8}


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name + '.npz')))


def _geoms(g):
    """Seven geometries: six test geometries (or as many as there are) and one training geometry."""
    Rt = g['R_test'].reshape(len(g['R_test']), -1)
    return np.concatenate([Rt[:6], g['R_train'][:1].reshape(1, -1)])


def _close(H, H_ref, tol):
    scale = np.abs(H_ref).max()
    return np.abs(H - H_ref).max() <= tol * scale


@pytest.mark.parametrize('name', CASES)
def test_hessian_matches_restatement(name):
    g = _load(name)
    model, _, _ = hr.model_from_fixture(g)
    tol = TOL.get(name, 1e-10)
    R7 = _geoms(g)
    E_ref, F_ref, H_ref = hr.hessian_of_model(model, R7)
    pred = GDMLPredict(model)
    # batches of 1, 7 and 256 (tiled copies; one training geometry among them) reach every slice / split branch
    E1, F1, H1 = pred.predict_hessian(R7[0])
    assert H1.shape == (1, R7.shape[1], R7.shape[1])
    assert _close(H1[0], H_ref[0], tol)
    E, F, H = pred.predict_hessian(R7)
    for q in range(len(R7)):
        assert _close(H[q], H_ref[q], tol), q
    idx = np.arange(256) % len(R7)
    Eb, Fb, Hb = pred.predict_hessian(R7[idx])
    for q in range(256):
        assert _close(Hb[q], H_ref[idx[q]], tol), q
    # E and F of the Hessian call are those of predict()
    Ep, Fp = pred.predict(R7)
    # ill-conditioned fits (n4_p6_pbc) cancel large summands down to O(1) forces: two correct summation orders differ by
    # ~eps times the summands (the floor of tests/test_oracle_golden.py)
    _, gq = orc.desc_from_R(R7, (model['lattice'], np.linalg.inv(model['lattice'])) if 'lattice' in model else None)
    f_floor = (50 * np.finfo(float).eps * model['std'] * np.abs(model['R_d_desc_alpha']).max() * 5.0 / (3 * model['sig']**2)
               * np.sqrt(model['R_desc'].shape[1] * len(model['perms'])) * max(1.0, np.abs(gq).max()))
    assert np.abs(F - Fp).max() <= 1e-12 * np.abs(Fp).max() + f_floor
    # energy constraints: summands of size std |alphas_E| cancel down to O(1) energies (5e4 -> 4 on n5_p2_ecstr), so two
    # correct summation orders differ by ~eps std max|alphas_E| sqrt(M P)
    floor = 0.0
    if 'alphas_E' in model:
        floor = 5 * np.finfo(float).eps * model['std'] * np.abs(model['alphas_E']).max() * np.sqrt(
            model['R_desc'].shape[1] * len(model['perms']))
    assert np.abs(E - Ep).max() <= 1e-12 * np.abs(Ep).max() + floor + f_floor * model['sig']
    # invariants: symmetric, translation invariant (sum over atoms b of H[i, 3b + c] = 0)
    N = R7.shape[1] // 3
    for h in H:
        scale = np.abs(h).max()
        assert np.abs(h - h.T).max() <= 1e-12 * scale
        assert np.abs(h.reshape(3 * N, N, 3).sum(axis=1)).max() <= 1e-12 * scale


@pytest.mark.parametrize('name', ['n5_p2_ecstr', 'n10_p2_pbc', 'cfg3_n42_p27_m60'])
def test_hessian_generic_and_chunked_paths(name):
    """F_x kept in memory (the path of N > 157) and table rows in many small chunks (partial H added chunk after chunk)."""
    g = _load(name)
    model, _, _ = hr.model_from_fixture(g)
    R7 = _geoms(g)
    _, _, H_ref = hr.hessian_of_model(model, R7)
    pred = GDMLPredict(model)
    for opts in ({'predict.hess_generic': 1}, {'predict.hess_chunk_rows': 16}, {'predict.hess_generic': 1, 'predict.hess_chunk_rows': 32}):
        for k, v in opts.items():
            pred._ctx.set_option(k, v)
        _, _, H = pred.predict_hessian(R7)
        for q in range(len(R7)):
            assert _close(H[q], H_ref[q], 1e-10), (opts, q)
        for k in opts:
            pred._ctx.set_option(k, 0)


def test_hessian_matches_gpu_finite_differences():
    """4-point central differences (h = 1e-4) of the GPU predictor's own forces, independent of the restatement."""
    g = _load('cfg1_n21_m100')
    model, _, _ = hr.model_from_fixture(g)
    pred = GDMLPredict(model)
    R = g['R_test'][0].ravel()
    _, _, H = pred.predict_hessian(R)
    H_fd = hr.fd_hessian(lambda X: pred.predict(X)[1], R, h=1e-4)
    assert _close(H[0], H_fd, 1e-8)


def test_hessian_deterministic_and_dev_entry():
    g = _load('cfg1_n21_m100')
    model, _, _ = hr.model_from_fixture(g)
    pred = GDMLPredict(model)
    ctx = pred._ctx
    R = np.ascontiguousarray(np.resize(_geoms(g), (70, 63)))
    B, n3 = R.shape
    a = ctx.predict_hessian(R)
    b = ctx.predict_hessian(R)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    lib = ctx._lib
    ptrs = [C.c_void_p() for _ in range(4)]
    sizes = [B * n3 * 8, B * 8, B * n3 * 8, B * n3 * n3 * 8]
    for p, s in zip(ptrs, sizes):
        ctx._check(lib.gdml_dev_alloc(ctx._h, s, C.byref(p)))
    try:
        ctx._check(lib.gdml_memcpy_h2d(ctx._h, ptrs[0], R.ctypes.data_as(C.c_void_p), R.nbytes))
        ctx.predict_hessian_dev(ptrs[0], B, ptrs[1], ptrs[2], ptrs[3])
        out = [np.empty(B), np.empty((B, n3)), np.empty((B, n3, n3))]
        for p, o in zip(ptrs[1:], out):
            ctx._check(lib.gdml_memcpy_d2h(ctx._h, o.ctypes.data_as(C.c_void_p), p, o.nbytes))
        for x, y in zip(a, out):
            assert np.array_equal(x, y)
        ctx.predict_hessian_dev(ptrs[0], B, None, None, ptrs[3])  # E and F may be NULL
        H2 = np.empty((B, n3, n3))
        ctx._check(lib.gdml_memcpy_d2h(ctx._h, H2.ctypes.data_as(C.c_void_p), ptrs[3], H2.nbytes))
        assert np.array_equal(H2, a[2])
    finally:
        for p in ptrs:
            lib.gdml_dev_free(ctx._h, p)


def test_hessian_replicas_and_host_slicing():
    g = _load('n10_p2_pbc')
    model, _, _ = hr.model_from_fixture(g)
    R = np.resize(_geoms(g), (40, 30))
    one = GDMLPredict(model)
    E, F, H = one.predict_hessian(R)
    two = GDMLPredict(model, devices=[0, 0])
    E2, F2, H2 = two.predict_hessian(R)
    assert _close(H2, H, 1e-13) and _close(F2, F, 1e-13) and _close(E2, E, 1e-13)
    one._ctx.max_query_batch = 3 * 30 * 3  # three geometries per library call
    E3, F3, H3 = one.predict_hessian(R)
    assert _close(H3, H, 1e-13) and _close(F3, F, 1e-13) and _close(E3, E, 1e-13)


def test_hessian_error_paths():
    g = _load('n10_p2_pbc')
    model, _, _ = hr.model_from_fixture(g)
    R = g['R_test'][0].reshape(1, -1)
    ctx = _lib.Context(0)
    try:
        with pytest.raises(_lib.GDMLHipError):  # no model resident
            ctx.model_n_atoms = 10
            ctx.predict_hessian(R)
    finally:
        ctx.close()
    pred = GDMLPredict(model)
    lat = np.asarray(model['lattice'], dtype=np.float64)
    lib = pred._ctx._lib
    H = np.empty((1, 30, 30))
    rc = lib.gdml_predict_hessian(pred._ctx._h, R.ctypes.data_as(C.c_void_p), 1, lat.ctypes.data_as(C.c_void_p), None,
                                  None, None, H.ctypes.data_as(C.c_void_p))
    assert rc == -1  # GDML_ERR_INVALID: a lattice without its inverse
    with pytest.raises(ValueError):  # the binding maps GDML_ERR_INVALID to ValueError, as for predict()
        pred._ctx.predict_hessian(R, (lat, None))
    with pytest.raises(ValueError):
        pred.predict_hessian(None)
    rc = lib.gdml_predict_hessian(pred._ctx._h, None, 1, None, None, None, None, H.ctypes.data_as(C.c_void_p))
    assert rc == -1
    rc = lib.gdml_predict_hessian(pred._ctx._h, R.ctypes.data_as(C.c_void_p), -1, None, None, None, None,
                                  H.ctypes.data_as(C.c_void_p))
    assert rc == -1

"""Strain derivative (virial) and stress on the GPU (gdml_predict_virial, csrc/predict.hip): against the NumPy restatement
(tests/_stress_ref.py) on every route, E and F against predict() bit for bit, strain finite differences of the GPU predictor's own
energies under a per-call lattice, invariants, determinism, replicas and error paths."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _hessian_ref as hr  # noqa: E402
import _stress_ref as sr  # noqa: E402
from sgdml_amd import _lib  # noqa: E402
from sgdml_amd.predict import GDMLPredict  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
CASES = ['n6_p1', 'n5_p4', 'n5_p2_ecstr', 'n9_p1', 'n10_p2_pbc', 'cfg0_n9_p6', 'cfg1_n21_m100', 'cfg3_n42_p27_m60', 'n100_m3',
         'n150_p2_m3', 'n4_p6_pbc']
# n4_p6_pbc is ill-conditioned: reordering its training points in a restatement alone moves the outputs by 8e-11 of their maximum
# (tests/test_hessian_gpu.py)
TOL = {'n4_p6_pbc': 1e-8}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(model, seven geometries, their restated (E, F, W)) of a fixture, computed once per session and only read."""
    g = dict(np.load(os.path.join(GOLDEN, name + '.npz')))
    model, _, _ = hr.model_from_fixture(g)
    Rt = g['R_test'].reshape(len(g['R_test']), -1)
    R7 = np.concatenate([Rt[:6], g['R_train'][:1].reshape(1, -1)])  # six test geometries (or as many as there are), one training
    ref = sr.virial_of_model(model, R7)
    for a in (R7,) + ref:
        a.setflags(write=False)
    return model, R7, ref


def _err(W, W_ref):
    return np.abs(W - W_ref).max() / np.abs(W_ref).max()


def _check(pred, R, W_ref, tol, what):
    """predict_virial(R): W against the restatement; E and F bit-identical to predict(R) on the same route and options."""
    E, F, W = pred.predict_virial(R)
    assert W.shape == (len(R), 3, 3)
    err = max(_err(W[q], W_ref[q]) for q in range(len(R)))
    print(what, 'max |W - W_ref| / max|W_ref| = %.2e' % err)
    assert err <= tol, what
    Ep, Fp = pred.predict(R)
    assert np.array_equal(E, Ep) and np.array_equal(F, Fp), what
    assert np.array_equal(W, W.transpose(0, 2, 1)), what  # six components are summed, the other triangle is a copy
    return E, F, W


@pytest.mark.parametrize('name', CASES)
def test_virial_matches_restatement(name):
    model, R7, (E_ref, F_ref, W_ref) = _case(name)
    tol = TOL.get(name, 1e-10)
    pred = GDMLPredict(model)
    ctx = pred._ctx
    # B = 1 and 7: the single launch where the shape is served (D <= 256, at most 384 coordinates), else the wave / big /
    # in-place routes
    _check(pred, R7[:1], W_ref[:1], tol, name + ' B=1')
    _check(pred, R7, W_ref, tol, name + ' B=7')
    if R7.shape[1] <= 3 * 23:  # D <= 256: the single launch serves the fixture -- every row split of it
        for rows in (2, 5, 16, 64):
            ctx.set_option('predict.fused_rows', rows)
            _check(pred, R7, W_ref, tol, name + ' B=7 fused_rows=%d' % rows)
            _check(pred, R7[3:4], W_ref[3:4], tol, name + ' B=1 fused_rows=%d' % rows)
        ctx.set_option('predict.fused_rows', 16)
    ctx.set_option('predict.fused', 0)  # three launches: the wave route (big / in-place for the large molecules)
    _check(pred, R7, W_ref, tol, name + ' B=7 fused=0')
    _check(pred, R7[:1], W_ref[:1], tol, name + ' B=1 fused=0')
    ctx.set_option('predict.fused', 1)
    idx = np.arange(256) % len(R7)  # tiled copies: the MFMA route (D <= 256), else wave / big / in-place
    _check(pred, R7[idx], W_ref[idx], tol, name + ' B=256')
    ctx.set_option('predict.mfma', 0)  # its VALU predecessor
    _check(pred, R7[idx], W_ref[idx], tol, name + ' B=256 bulk')
    ctx.set_option('predict.mfma', 1)
    if name == 'cfg3_n42_p27_m60':
        ctx.set_option('predict.mfma_wide', 2)  # the wide GEMM pipeline
        _check(pred, R7[idx], W_ref[idx], tol, name + ' B=256 wide')
        ctx.set_option('predict.mfma_wide', 1)


def test_stress_is_virial_over_volume_and_voigt_order():
    model, R7, _ = _case('n10_p2_pbc')
    pred = GDMLPredict(model)
    E, F, W = pred.predict_virial(R7)
    vol = abs(np.linalg.det(model['lattice']))
    Es, Fs, S = pred.predict_stress(R7)
    # (the volume is a 3 x 3 determinant: two correct evaluations differ by a few rounding errors)
    eps = np.finfo(float).eps
    assert np.array_equal(Es, E) and np.array_equal(Fs, F) and np.abs(S - W / vol).max() <= 8 * eps * np.abs(S).max()
    _, _, V = pred.predict_stress(R7, voigt=True)
    assert V.shape == (7, 6)
    for c, (a, b) in enumerate([(0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1)]):  # ASE: xx, yy, zz, yz, xz, xy
        assert np.array_equal(V[:, c], S[:, a, b])
    # a per-call lattice supplies the volume as well
    lat2 = 1.5 * np.asarray(model['lattice'])
    _, _, W2 = pred.predict_virial(R7, lattice=lat2)
    _, _, S2 = pred.predict_stress(R7, lattice=lat2)
    assert np.abs(S2 - W2 / abs(np.linalg.det(lat2))).max() <= 8 * eps * np.abs(S2).max()
    assert not np.array_equal(W2, W)  # (the other cell moved minimum images: the argument is not ignored)
    # a model without a lattice: W is defined, the stress is not -- unless the call brings a lattice
    model_np, R_np, _ = _case('n9_p1')
    pred_np = GDMLPredict(model_np)
    with pytest.raises(ValueError):
        pred_np.predict_stress(R_np)
    box = 100.0 * np.eye(3)
    _, _, S_np = pred_np.predict_stress(R_np, lattice=box)
    assert S_np.shape == (7, 3, 3)


def test_virial_matches_gpu_strain_finite_differences():
    """4-point central differences (h = 1e-4) of the GPU predictor's own energies with the strained cell passed per call:
    independent of the restatement, and the test of predict(R, lattice=...)."""
    model, R7, _ = _case('n10_p2_pbc')
    pred = GDMLPredict(model)
    R = R7[0]
    _, _, W = pred.predict_virial(R)
    W_fd = sr.fd_virial(lambda X, lat: pred.predict(X, lattice=lat)[0], R, model['lattice'], h=1e-4)
    err = _err(W[0], W_fd)
    print('GPU strain FD error / max|W| = %.2e' % err)
    assert err <= 1e-8


def test_virial_is_minus_sum_f_r_without_a_lattice():
    model, R7, _ = _case('cfg1_n21_m100')
    pred = GDMLPredict(model)
    for R in (R7, R7[np.arange(256) % 7]):  # wave and MFMA route
        E, F, W = pred.predict_virial(R)
        W_fr = -np.einsum('bia,bic->bac', F.reshape(len(R), -1, 3), R.reshape(len(R), -1, 3))
        err = max(_err(W[q], W_fr[q]) for q in range(len(R)))
        print('|W + sum f r| / max|W| = %.2e' % err)
        assert err <= 1e-12


def test_virial_deterministic_and_dev_entry():
    model, R7, _ = _case('cfg1_n21_m100')
    pred = GDMLPredict(model)
    ctx = pred._ctx
    R = np.ascontiguousarray(np.resize(R7, (70, 63)))
    B, n3 = R.shape
    a = ctx.predict_virial(R)
    b = ctx.predict_virial(R)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    f1 = ctx.predict_virial(R[:5])  # the single launch
    f2 = ctx.predict_virial(R[:5])
    for x, y in zip(f1, f2):
        assert np.array_equal(x, y)
    lib = ctx._lib
    ptrs = [C.c_void_p() for _ in range(4)]
    sizes = [B * n3 * 8, B * 8, B * n3 * 8, B * 9 * 8]
    for p, s in zip(ptrs, sizes):
        ctx._check(lib.gdml_dev_alloc(ctx._h, s, C.byref(p)))
    try:
        ctx._check(lib.gdml_memcpy_h2d(ctx._h, ptrs[0], R.ctypes.data_as(C.c_void_p), R.nbytes))
        ctx.predict_virial_dev(ptrs[0], B, ptrs[1], ptrs[2], ptrs[3])
        out = [np.empty(B), np.empty((B, n3)), np.empty((B, 3, 3))]
        for p, o in zip(ptrs[1:], out):
            ctx._check(lib.gdml_memcpy_d2h(ctx._h, o.ctypes.data_as(C.c_void_p), p, o.nbytes))
        for x, y in zip(a, out):
            assert np.array_equal(x, y)
        ctx.predict_virial_dev(ptrs[0], B, None, None, ptrs[3])  # E and F may be NULL
        W2 = np.empty((B, 3, 3))
        ctx._check(lib.gdml_memcpy_d2h(ctx._h, W2.ctypes.data_as(C.c_void_p), ptrs[3], W2.nbytes))
        assert np.array_equal(W2, a[2])
    finally:
        for p in ptrs:
            lib.gdml_dev_free(ctx._h, p)
    # the host entry without E and F, on the multi-launch route and on the single launch
    for Rh, ref in ((R, a), (R[:5], f1)):
        W3 = np.empty((len(Rh), 3, 3))
        ctx._check(lib.gdml_predict_virial(ctx._h, Rh.ctypes.data_as(C.c_void_p), len(Rh), None, None, None, None,
                                           W3.ctypes.data_as(C.c_void_p)))
        assert np.array_equal(W3, ref[2])


def test_virial_at_the_end_of_the_staged_host_path():
    """Host batches up to 1 MiB of R, E and F are staged through one pinned block, and W rides along up to the same batch size
    (N = 10: 61 doubles per geometry without W, 70 with -- B = 2000 fits only without; the block grows once)."""
    model, R7, (_, _, W_ref) = _case('n10_p2_pbc')
    pred = GDMLPredict(model)
    for B in (70, 2000, 2200, 70):  # staged; staged only if W rides along; beyond the staged path; staged, after the growth
        idx = np.arange(B) % 7
        _check(pred, R7[idx], W_ref[idx], 1e-10, 'n10_p2_pbc B=%d' % B)


def test_virial_alone_equals_in_batch():
    model, R7, _ = _case('n10_p2_pbc')
    pred = GDMLPredict(model)
    E7, F7, W7 = pred.predict_virial(R7)  # the single launch: a query's workgroups and row shares do not depend on B
    for q in (0, 4, 6):
        E1, F1, W1 = pred.predict_virial(R7[q])
        assert np.array_equal(W1[0], W7[q]) and np.array_equal(F1[0], F7[q]) and np.array_equal(E1[0], E7[q])
    # three launches: the row splits are sized by B, so the partial sums are grouped differently (rounding only)
    pred._ctx.set_option('predict.fused', 0)
    E7, F7, W7 = pred.predict_virial(R7)
    for q in (0, 4, 6):
        _, _, W1 = pred.predict_virial(R7[q])
        assert _err(W1[0], W7[q]) <= 1e-13


def test_predict_with_the_models_own_lattice_per_call():
    model, R7, _ = _case('n10_p2_pbc')
    pred = GDMLPredict(model)
    lat = np.array(model['lattice'])
    for R in (R7, R7[np.arange(256) % 7]):
        E, F = pred.predict(R)
        E2, F2 = pred.predict(R, lattice=lat)
        assert np.array_equal(E, E2) and np.array_equal(F, F2)
        (F3,) = pred.predict(R, return_E=False, lattice=lat)
        assert np.array_equal(F, F3)
    a = pred.predict_virial(R7)
    b = pred.predict_virial(R7, lattice=lat)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    h = pred.predict_hessian(R7[:2])
    h2 = pred.predict_hessian(R7[:2], lattice=lat)
    for x, y in zip(h, h2):
        assert np.array_equal(x, y)
    # another cell gives other forces (the argument is not ignored): 0.8 x the cell moves the minimum images
    E4, F4 = pred.predict(R7, lattice=0.8 * lat)
    assert not np.array_equal(F4, pred.predict(R7)[1])


def test_virial_replicas_and_host_slicing():
    model, R7, _ = _case('n10_p2_pbc')
    R = np.resize(R7, (140, 30))
    one = GDMLPredict(model)
    E, F, W = one.predict_virial(R)
    two = GDMLPredict(model, devices=[0, 0])
    E2, F2, W2 = two.predict_virial(R)  # two shards of 70
    assert W2.shape == W.shape
    # the shards' row splits are sized by their own batch: rounding of regrouped partial sums only
    assert _err(W2, W) <= 1e-13 and _err(F2, F) <= 1e-13 and _err(E2, E) <= 1e-13
    Ep, Fp = two.predict(R)
    assert np.array_equal(E2, Ep) and np.array_equal(F2, Fp)
    one._ctx.max_query_batch = 32  # slices of 32 geometries per library call
    E3, F3, W3 = one.predict_virial(R)
    assert _err(W3, W) <= 1e-13 and _err(F3, F) <= 1e-13 and _err(E3, E) <= 1e-13


def test_virial_error_paths():
    model, R7, _ = _case('n10_p2_pbc')
    R = np.ascontiguousarray(R7[:1])
    pred = GDMLPredict(model)
    lat = np.ascontiguousarray(model['lattice'], dtype=np.float64)
    lat_inv = np.linalg.inv(lat)
    lib = pred._ctx._lib
    W = np.empty((1, 3, 3))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.gdml_predict_virial(pred._ctx._h, None, 1, None, None, None, None, vp(W)) == -1  # R = NULL
    assert lib.gdml_predict_virial(pred._ctx._h, vp(R), 1, vp(lat), None, None, None, vp(W)) == -1  # a lattice without inverse
    assert lib.gdml_predict_virial(pred._ctx._h, vp(R), 1, None, vp(lat_inv), None, None, vp(W)) == -1
    assert lib.gdml_predict_virial(pred._ctx._h, vp(R), 1, None, None, None, None, None) == -1  # W = NULL
    assert lib.gdml_predict_virial(pred._ctx._h, vp(R), -1, None, None, None, None, vp(W)) == -1
    assert lib.gdml_predict_virial_dev(pred._ctx._h, None, 1, None, None, None, None, vp(W)) == -1
    with pytest.raises(ValueError):  # the binding maps GDML_ERR_INVALID to ValueError, as for predict()
        pred._ctx.predict_virial(R, (lat, None))
    with pytest.raises(ValueError):
        pred._ctx.predict_virial(None)
    with pytest.raises(ValueError):
        pred.predict_virial(None)
    singular = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]])
    for bad in (np.eye(2), np.ones((3, 4)), lat.ravel(), singular, np.zeros((3, 3))):
        for call in (pred.predict_virial, pred.predict_stress, pred.predict, pred.predict_hessian):
            with pytest.raises(ValueError):
                call(R, lattice=bad)
    with pytest.raises(ValueError):
        pred.predict(None, lattice=lat)  # the training-set mode has cached descriptors, no lattice to apply
    ctx = _lib.Context(0)
    try:
        with pytest.raises(_lib.GDMLHipError):  # no model resident
            ctx.model_n_atoms = 10
            ctx.predict_virial(R)
    finally:
        ctx.close()
    # the predictor still works after every rejected call
    _, _, W_ok = pred.predict_virial(R)
    assert np.isfinite(W_ok).all()

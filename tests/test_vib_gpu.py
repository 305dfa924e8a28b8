"""Harmonic vibrational analysis on the GPU (csrc/vib.hip; the eigensolver: csrc/sym_eig.hip): the batched eigensolver against LAPACK, vibrations() against the
NumPy restatement (tests/_vib_ref.py) applied to the device's own Hessians, the physics of the two toy models, invariances,
bit-identity and error paths.

Bounds.  Eigenvalues and residuals |A v - w v| carry the agreed 40 n eps |A|_F (tests/_vib_ref.bound).  Orthogonality
|V V^T - I|_max is a property of unit vectors and does not scale with A: its bound is the same figure relative to 1, 40 n eps --
never the looser of the two for the matrices here (|A|_F > 1) except the one scaled by 2^-30, where a bound that shrank with
|A|_F could not be met by any solver."""
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
import _neb_ref as nr  # noqa: E402
import _relax_ref as rr  # noqa: E402
import _vib_ref as vr  # noqa: E402
from _vib_ref import eig_inputs, eig_special, geoms as _geoms  # noqa: E402
from sgdml_amd import _lib  # noqa: E402
from sgdml_amd._lib import VibParams  # noqa: E402,F401  (the binding of gdml_vib_run: this file tests nothing without it)
from sgdml_amd.predict import GDMLPredict  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
EIG_SIZES = [1, 2, 3, 8, 63, 64, 100, 101, 140, 141, 142, 150]  # odd and even, both sides of each storage boundary (100 | 101, 141 | 142)
FIXTURES = ['n6_p1', 'n5_p4', 'n9_p1', 'n10_p2_pbc', 'cfg1_n21_m100', 'cfg3_n42_p27_m60', 'n100_m3']
SMALL = ('n6_p1', 'n5_p4', 'n9_p1', 'n10_p2_pbc')
OVERLAP_MIN = 0.9  # tests/test_vib_cpu.py checks the restated overlap (0.996) against the same threshold


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name + '.npz')))


@functools.lru_cache(maxsize=None)
def _ctx():
    return _lib.Context(0)


def eig_check(A, w, V, what=''):
    """Asserts order, sign convention and the three bounds for a batch; returns the largest error / bound ratios."""
    n = A.shape[1]
    worst = np.zeros(3)
    for m in range(len(A)):
        b = vr.bound(n, A[m])
        dw, res, orth = vr.eig_errors(A[m], w[m], V[m])
        print('%s n = %d matrix %d: eigenvalues %.2e residual %.2e (bound %.2e), orthogonality %.2e (bound %.2e)' % (
            what, n, m, dw, res, b, orth, 40.0 * n * vr.EPS))
        assert (np.diff(w[m]) >= 0.0).all()
        assert dw <= b and res <= b and orth <= 40.0 * n * vr.EPS, (what, n, m)
        if b > 0.0:
            worst = np.maximum(worst, [dw / b, res / b, orth / (40.0 * n * vr.EPS)])
    assert vr.sign_convention_holds(V)
    return worst


# ---- 1. the eigensolver

@pytest.mark.parametrize('n', EIG_SIZES)
def test_sym_eig_against_lapack(n):
    ctx = _ctx()
    A = eig_inputs(n)
    w, V, sweeps = ctx.sym_eig(A)
    eig_check(A, w, V, 'random')
    assert (sweeps >= (1 if n > 1 else 0)).all() and (sweeps <= 30).all()
    S = eig_special(n)
    ws, Vs, sw = ctx.sym_eig(S)
    eig_check(S, ws, Vs, 'special')
    assert sw[0] == 0 and sw[1] == 0  # diagonal and zero: no sweep
    assert np.array_equal(ws[0], np.sort(np.diag(S[0]))) and not ws[1].any()
    assert np.array_equal(np.abs(Vs[1]), np.eye(n))
    # V = NULL: the same eigenvalues; the same call again; a matrix alone against itself inside the batch
    w0, V0, sw0 = ctx.sym_eig(A, vectors=False)
    assert V0 is None and np.array_equal(w0, w) and np.array_equal(sw0, sweeps)
    w1, V1, sw1 = ctx.sym_eig(A)
    assert np.array_equal(w1, w) and np.array_equal(V1, V) and np.array_equal(sw1, sweeps)
    wa, Va, swa = ctx.sym_eig(A[1:2])
    assert np.array_equal(wa[0], w[1]) and np.array_equal(Va[0], V[1]) and swa[0] == sweeps[1]


def test_sym_eig_grid_stride():
    """More matrices than workgroups: every workgroup takes several and starts each from a fresh identity."""
    ctx = _ctx()
    A = eig_inputs(3, M=1100)
    w, V, sweeps = ctx.sym_eig(A)
    w_ref = np.linalg.eigvalsh(A)
    nrm = np.sqrt((A ** 2).sum(axis=(1, 2)))
    assert (np.abs(w - w_ref).max(axis=1) <= 40 * 3 * vr.EPS * nrm).all()
    res = np.sqrt(((np.einsum('mij,mkj->mki', A, V) - V * w[:, :, None]) ** 2).sum(-1)).max(axis=1)
    assert (res <= 40 * 3 * vr.EPS * nrm).all()
    assert np.abs(np.einsum('mij,mkj->mik', V, V) - np.eye(3)).max() <= 40 * 3 * vr.EPS
    assert vr.sign_convention_holds(V)
    for m in (0, 517, 1099):
        wa, Va, _ = ctx.sym_eig(A[m:m + 1])
        assert np.array_equal(wa[0], w[m]) and np.array_equal(Va[0], V[m])


@pytest.mark.parametrize('n', [8, 101, 150])
def test_sym_eig_dev_entry_equals_host_entry(n):
    ctx = _ctx()
    lib = ctx._lib
    A = eig_inputs(n)
    M = len(A)
    w, V, sweeps = ctx.sym_eig(A)
    ptrs = [C.c_void_p() for _ in range(4)]
    sizes = [A.nbytes, M * n * 8, A.nbytes, M * 8]
    for p, s in zip(ptrs, sizes):
        ctx._check(lib.gdml_dev_alloc(ctx._h, s, C.byref(p)))
    try:
        ctx._check(lib.gdml_memcpy_h2d(ctx._h, ptrs[0], A.ctypes.data_as(C.c_void_p), A.nbytes))
        ctx.sym_eig_dev(ptrs[0], M, n, ptrs[1], ptrs[2], ptrs[3])
        out = [np.empty((M, n)), np.empty((M, n, n)), np.empty(M, dtype=np.int64)]
        for p, o in zip(ptrs[1:], out):
            ctx._check(lib.gdml_memcpy_d2h(ctx._h, o.ctypes.data_as(C.c_void_p), p, o.nbytes))
        assert np.array_equal(out[0], w) and np.array_equal(out[1], V) and np.array_equal(out[2], sweeps)
        # in place (V over A), without sweeps
        ctx.sym_eig_dev(ptrs[0], M, n, ptrs[1], ptrs[0], None)
        ctx._check(lib.gdml_memcpy_d2h(ctx._h, out[1].ctypes.data_as(C.c_void_p), ptrs[0], out[1].nbytes))
        assert np.array_equal(out[1], V)
    finally:
        for p in ptrs:
            lib.gdml_dev_free(ctx._h, p)


def test_sym_eig_reports_a_matrix_that_does_not_converge():
    A = eig_inputs(5)
    A[1, 2, 3] = A[1, 3, 2] = np.nan
    with pytest.raises(ValueError, match='matrix 1 '):
        _ctx().sym_eig(A)


# ---- 2. vibrations() against the restatement on the device's own Hessians

def vib_check(pred, model, R, masses, project=None, lat=None):
    """One batch, per geometry: w2, n_rigid and n_imag against the restatement, exact zeros, rigid and vibrational rows against
    Q, residual and orthogonality of the modes against D_s, E and F against predict_hessian.  Returns the largest error / bound
    ratio of w2."""
    out = pred.vibrations(R, masses, project=project, modes=True)
    E, F, H = pred.predict_hessian(R)
    assert np.array_equal(out['E'], E) and np.array_equal(out['F'], F)
    n = R.shape[1]
    pj = vr.PROJECT[project] if project is not None else (1 if lat is not None else 2)
    worst, cache = 0.0, {}
    for b in range(len(R)):
        key = R[b].tobytes()
        if key not in cache:
            cache[key] = vr.vibrations(H[b] / model['std'], R[b], masses, h_scale=model['std'], project=pj)
        ref = cache[key]
        k = ref['n_rigid']
        nrm = np.linalg.norm(ref['D_s'])
        bnd, rel = 40.0 * n * vr.EPS * nrm, 40.0 * n * vr.EPS
        assert out['n_rigid'][b] == k and out['n_imag'][b] == ref['n_neg'], (b, out['n_rigid'][b], out['n_imag'][b])
        dw = np.abs(out['w2'][b, :n - k] - ref['w2'][:n - k]).max() if k < n else 0.0
        assert dw <= bnd, (b, dw, bnd)
        assert not out['w2'][b, n - k:].any()
        md, Q = out['modes'][b], ref['Q']
        lam = np.concatenate([out['w2'][b, :n - k], np.full(k, ref['Lambda'])])
        res = np.sqrt(((ref['D_s'] @ md.T - md.T * lam[None, :]) ** 2).sum(axis=0)).max()
        orth = np.abs(md @ md.T - np.eye(n)).max()
        assert res <= bnd and orth <= rel, (b, res, bnd, orth)
        if k:
            Pm = md[n - k:] - (md[n - k:] @ Q.T) @ Q  # P applied to the rigid rows
            assert np.sqrt((Pm ** 2).sum(axis=1)).max() <= rel
            if k < n:
                assert np.sqrt(((md[:n - k] @ Q.T) ** 2).sum(axis=1)).max() <= rel
        if b < 7:
            print('geometry %d: n_rigid %d n_imag %d sweeps %d  w2 error %.2e residual %.2e (bound %.2e) orthogonality %.2e (%.2e)' % (
                b, k, ref['n_neg'], out['sweeps'][b], dw, res, bnd, orth, rel))
        worst = max(worst, dw / bnd)
    assert np.array_equal(out['freq'], np.sign(out['w2']) * np.sqrt(np.abs(out['w2'])))
    return worst


@pytest.mark.parametrize('name', FIXTURES)
def test_vibrations_match_restatement(name):
    g = _load(name)
    model, _, lat = hr.model_from_fixture(g)
    pred = GDMLPredict(model)
    N = len(model['z'])
    m = vr.fixture_masses(N)
    R7 = _geoms(g)
    if name == 'n100_m3':
        vib_check(pred, model, R7[:2], m, lat=lat)
        return
    vib_check(pred, model, R7[:1], m, lat=lat)
    vib_check(pred, model, R7, m, lat=lat)
    if name in SMALL:
        vib_check(pred, model, R7[np.arange(70) % 7], m, lat=lat)
    if lat is not None:
        assert (pred.vibrations(R7, m)['n_rigid'] == 3).all()  # 'trans' by default
        with pytest.raises(ValueError):
            pred.vibrations(R7, m, project='rigid')


@pytest.mark.parametrize('project', ['none', 'trans'])
def test_vibrations_other_projections(project):
    g = _load('n9_p1')
    model, _, _ = hr.model_from_fixture(g)
    pred = GDMLPredict(model)
    vib_check(pred, model, _geoms(g), vr.fixture_masses(9), project=project)


# ---- 3. physics on the toys, on the device

def test_relaxed_toy_is_a_minimum():
    model, starts, _, fmax = rr.toy()
    pred = GDMLPredict(model)
    out = pred.relax(starts, fmax, max_steps=200, **rr.TOY_PARAMS['free'])
    assert out['converged'].all()
    v = pred.vibrations(out['R_end'], np.ones(6))
    assert (v['n_rigid'] == 6).all() and (v['n_imag'] == 0).all() and (v['w2'][:, :12] > 0.0).all()
    assert not v['w2'][:, 12:].any()


def test_climbing_image_is_a_first_order_saddle():
    model, A, Bm, fmax = nr.toy()
    pred = GDMLPredict(model)
    path, _ = nr.toy_bands('p4')
    out = pred.neb(path, fmax, k_spring=nr.TOY_K, climb=True, max_steps=nr.TOY_MAX_STEPS)
    assert out['converged'].all()
    ic = int(out['i_climb'][0])
    R3 = np.stack([out['R_end'][0, ic], A, Bm])
    v = pred.vibrations(R3, np.ones(5), modes=True)
    assert v['n_imag'].tolist() == [1, 0, 0] and (v['n_rigid'] == 6).all()
    assert v['w2'][0, 0] < 0.0 < v['w2'][0, 1] and abs(v['w2'][0, 0] - nr.TOY_SADDLE_MODES[0]) < 2e-3
    t = vr.band_tangent(out['R_end'][0], out['E_end'][0], ic)
    overlap = abs(v['modes'][0, 0] @ t)
    print('imaginary mode %.4f, overlap with the band tangent %.4f' % (v['w2'][0, 0], overlap))
    assert overlap > OVERLAP_MIN


# ---- 4. invariances

def test_mass_and_unit_scaling_are_exact():
    g = _load('cfg1_n21_m100')
    model, _, _ = hr.model_from_fixture(g)
    pred = GDMLPredict(model)
    R, m = _geoms(g), vr.fixture_masses(21)
    a = pred.vibrations(R, m, modes=True)
    b = pred.vibrations(R, 4.0 * m, modes=True)
    assert np.array_equal(b['w2'], a['w2'] / 4.0) and np.array_equal(b['modes'], a['modes'])
    c = pred.vibrations(R, m, f_unit=2.0)
    assert np.array_equal(c['w2'], 2.0 * a['w2']) and np.array_equal(c['n_imag'], a['n_imag'])


def test_rigid_motion_of_the_geometry_leaves_the_spectrum():
    g = _load('n9_p1')
    model, _, _ = hr.model_from_fixture(g)
    pred = GDMLPredict(model)
    R, m = _geoms(g), vr.fixture_masses(9)
    rs = np.random.RandomState(4)
    U, _ = np.linalg.qr(rs.standard_normal((3, 3)))
    R2 = (R.reshape(7, 9, 3) @ U.T + rs.standard_normal(3)[None, None, :]).reshape(7, 27)
    a, b = pred.vibrations(R, m), pred.vibrations(R2, m)
    _, _, H = pred.predict_hessian(R)
    for q in range(7):
        D_s = vr.shifted(H[q], R[q], m)[0]
        tol = 40.0 * 27 * vr.EPS * np.linalg.norm(D_s) + 1e-10 * np.abs(vr.mass_weight(H[q], m)).max()
        assert np.abs(a['w2'][q, :21] - b['w2'][q, :21]).max() <= tol
    assert np.array_equal(a['n_rigid'], b['n_rigid']) and np.array_equal(a['n_imag'], b['n_imag'])


def test_collinear_geometry_on_the_device():
    g = _load('n5_p4')
    model, _, _ = hr.model_from_fixture(g)
    pred = GDMLPredict(model)
    for bent, k in ((False, 5), (True, 6)):
        R, m = vr.collinear(bent)
        v = pred.vibrations(R, m)
        assert v['n_rigid'].tolist() == [k] and not v['w2'][0, 15 - k:].any()


# ---- 5. bits

def test_bit_identity():
    g = _load('cfg1_n21_m100')
    model, _, _ = hr.model_from_fixture(g)
    pred = GDMLPredict(model)
    R, m = _geoms(g), vr.fixture_masses(21)
    keys = ('w2', 'n_rigid', 'n_imag', 'E', 'F', 'sweeps')
    a = pred.vibrations(R, m, modes=True)
    b = pred.vibrations(R, m, modes=True)
    assert all(np.array_equal(a[k], b[k]) for k in keys + ('modes',))
    c = pred.vibrations(R, m)
    assert 'modes' not in c and all(np.array_equal(a[k], c[k]) for k in keys)
    try:
        for chunk in (1, 3, 0):
            pred._ctx.set_option('predict.vib_chunk', chunk)
            d = pred.vibrations(R, m, modes=True)
            assert all(np.array_equal(a[k], d[k]) for k in keys + ('modes',)), chunk
    finally:
        pred._ctx.set_option('predict.vib_chunk', 0)
    one = pred.vibrations(R[3], m, modes=True)
    assert all(np.array_equal(one[k][0], a[k][3]) for k in keys + ('modes',))
    two = GDMLPredict(model, devices=[0, 0])
    R14 = np.concatenate([R, R[::-1]])
    e, f = pred.vibrations(R14, m, modes=True), two.vibrations(R14, m, modes=True)
    assert all(np.array_equal(e[k], f[k]) for k in keys + ('modes',))


# ---- 6. error paths on the device

def test_error_paths_on_the_device():
    ctx = _lib.Context(0)
    try:
        lib = ctx._lib
        R, m = np.arange(6.0).reshape(1, 6), np.ones(2)
        w2, nr_, nn_ = np.zeros((1, 6)), np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
        prm = _lib.VibParams(1, 2, 1.0, None, None, 2)
        rc = lib.gdml_vib_run(ctx._h, C.byref(prm), _lib._ptr(R), _lib._ptr(m), _lib._ptr(w2), None, _lib._ptr(nr_), _lib._ptr(nn_),
                              None, None, None)
        assert rc == _lib.ERR_STATE and 'model' in lib.gdml_last_error(ctx._h).decode()
        R198, m198, w198 = np.zeros((1, 594)), np.ones(198), np.zeros((1, 594))
        prm = _lib.VibParams(1, 198, 1.0, None, None, 2)
        rc = lib.gdml_vib_run(ctx._h, C.byref(prm), _lib._ptr(R198), _lib._ptr(m198), _lib._ptr(w198), None, _lib._ptr(nr_),
                              _lib._ptr(nn_), None, None, None)
        assert rc == _lib.ERR_UNSUPPORTED
    finally:
        ctx.close()
    g = _load('n6_p1')
    model, _, _ = hr.model_from_fixture(g)
    pred = GDMLPredict(model)
    with pytest.raises(ValueError):  # N different from the model's
        pred._ctx._check(pred._ctx._lib.gdml_vib_run(
            pred._ctx._h, C.byref(_lib.VibParams(1, 2, 1.0, None, None, 2)), _lib._ptr(np.arange(6.0)), _lib._ptr(np.ones(2)),
            _lib._ptr(np.zeros(6)), None, _lib._ptr(np.zeros(1, dtype=np.int64)), _lib._ptr(np.zeros(1, dtype=np.int64)), None,
            None, None))
    empty = pred.vibrations(np.zeros((0, 18)), np.ones(6))
    assert empty['w2'].shape == (0, 18) and empty['n_imag'].shape == (0,)

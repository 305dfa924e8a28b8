"""Posterior force covariances on the GPU (csrc/uncert.hip) against the NumPy restatement (tests/_uncertainty_ref.py): the
cross-kernel at the assembly contract, its consistency with the predictor, the covariance within the derived bound
(_uncertainty_ref.cov_tol), determinism, the device entry, invariants, calibration, chunking and the error paths."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest
import scipy.linalg as sla

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _uncertainty_ref as ur  # noqa: E402
from oracle import gdml_oracle as orc  # noqa: E402
from sgdml_amd import _lib  # noqa: E402
from sgdml_amd.predict import GDMLPredict  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
# Fixtures and queries are fixed by the meaningfulness cap below: with the reference values alone the largest
# tol_q / min diag Sig_ref over these six fixtures and seven queries is 0.069 (cfg0_n9_p6 query 0, cfg3_n42_p27_m60 query 6).
# Do not add fixtures or queries without checking them the same way.
CASES = ['n5_p4', 'n10_p2_pbc', 'n4_p6_pbc', 'cfg0_n9_p6', 'cfg1_n21_m100', 'cfg3_n42_p27_m60']
RECORD = os.environ.get('GDML_UNCERTAINTY_RECORD', os.path.join(ROOT, 'profiles', 'uncertainty_parity.json'))
_observed = {}


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name + '.npz')))


@functools.lru_cache(maxsize=None)
def _ref(name):
    """Reference values of a fixture, computed once per session."""
    g = _load(name)
    R_train, x, gd, tp, lat = ur.fixture_tables(g)
    Rq = ur.queries(g)
    sig, lam = float(g['sig']), float(g['lam'])
    A = ur.system_matrix(x, gd, tp, sig, lam)
    Kx, kqq = ur.cross_rows(Rq, x, gd, tp, sig, lat)
    Sig = ur.posterior_cov(Kx, kqq, A)
    nA = float(sla.eigvalsh(A, subset_by_index=[len(A) - 1, len(A) - 1])[0])  # ||A||_2 of a symmetric positive definite matrix
    tol = np.array([ur.cov_tol(Kx[q], kqq[q], A, nA) for q in range(len(Rq))])
    return {'g': g, 'R_train': R_train, 'gd': gd, 'lat': lat, 'Rq': Rq, 'lam': lam, 'Kx': Kx, 'kqq': kqq, 'Sig': Sig, 'tol': tol,
            'model': ur.model_from_fixture(g)}


@functools.lru_cache(maxsize=None)
def _pred(name):
    """A predictor with the factor of the fixture resident (uncalibrated: covariances in units of std^2)."""
    r = _ref(name)
    pred = GDMLPredict(r['model'])
    pred.prepare_uncertainty(r['R_train'])
    return pred


def _batches(Rq):
    """Batches of 1, 7 and 256 (tiled copies): (geometries, index of each into Rq)."""
    yield Rq[:1], np.arange(1)
    yield Rq, np.arange(len(Rq))
    idx = np.arange(256) % len(Rq)
    yield Rq[idx], idx


@pytest.mark.parametrize('name', CASES)
def test_cross_kernel_parity(name):
    """gdml_uncert_cross at the project's assembly contract: max|dKx_q| <= 1e-12 max|Kx_q|, the same for k_qq."""
    r, pred = _ref(name), _pred(name)
    n3 = r['Rq'].shape[1]
    for R, idx in _batches(r['Rq']):
        Kx, kqq = pred._ctx.uncert_cross(R, r['lat'])
        Kx = Kx.reshape(len(R), n3, -1)
        for b, q in enumerate(idx):
            e_x = np.abs(Kx[b] - r['Kx'][q]).max() / np.abs(r['Kx'][q]).max()
            e_q = np.abs(kqq[b] - r['kqq'][q]).max() / np.abs(r['kqq'][q]).max()
            if len(R) <= 7:
                print('%s B=%d q=%d  dKx %.2e  dkqq %.2e' % (name, len(R), q, e_x, e_q))
            assert e_x <= ur.TAU, (len(R), b)
            assert e_q <= ur.TAU, (len(R), b)


@pytest.mark.parametrize('name', CASES)
def test_cross_kernel_reproduces_the_predictor(name):
    """Kx_q alphas_F is the predictor's force (in units of std): no oracle involved, the tolerance of test_hip_parity.test_predict."""
    r, pred = _ref(name), _pred(name)
    m = r['model']
    Kx, _ = pred._ctx.uncert_cross(r['Rq'], r['lat'])
    F = pred.predict(r['Rq'])[1]
    fl = ur.cancel_floor(m, r['gd'])
    got = (Kx @ m['alphas_F']).reshape(F.shape) * m['std']
    print('%s  |Kx alpha std - F| %.2e  bound %.2e' % (name, np.abs(got - F).max(), 1e-10 * np.abs(F).max() + fl))
    assert np.abs(got - F).max() <= 1e-10 * np.abs(F).max() + fl


@pytest.mark.parametrize('name', CASES)
def test_covariance_parity(name):
    """|Sig_gpu - Sig_ref| <= tol_q elementwise (derivation: _uncertainty_ref.cov_tol), with tol_q capped at a tenth of the
    smallest reference variance so that the comparison means something; the observed ratios go to the record file."""
    r, pred = _ref(name), _pred(name)
    std2 = r['model']['std'] ** 2
    for q in range(len(r['Rq'])):  # a condition on the reference values, not a measurement
        assert r['tol'][q] <= 0.1 * np.diag(r['Sig'][q]).min(), q
    worst = 0.0
    for R, idx in _batches(r['Rq']):
        E, F, cov = pred.predict_uncertainty(R, full_cov=True)
        assert cov.shape == (len(R), R.shape[1], R.shape[1])
        for b, q in enumerate(idx):
            ratio = np.abs(cov[b] / std2 - r['Sig'][q]).max() / r['tol'][q]
            if len(R) <= 7:
                print('%s B=%d q=%d  max|dSig| / tol_q = %.3g  (tol_q / min diag = %.3g)' % (
                    name, len(R), q, ratio, r['tol'][q] / np.diag(r['Sig'][q]).min()))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (len(R), b, ratio)
        Ep, Fp = pred.predict(R)
        assert np.array_equal(E, Ep) and np.array_equal(F, Fp)
    _observed[name] = float('%.3g' % worst)
    if len(_observed) == len(CASES):
        with open(RECORD, 'w') as f:
            json.dump({'what': 'max |Sig_gpu - Sig_ref| / tol_q per fixture (tests/test_uncertainty_gpu.py; seven queries, '
                               'batches of 1, 7 and 256)', 'ratio': {k: _observed[k] for k in CASES}}, f, indent=1)
            f.write('\n')


@pytest.mark.parametrize('name', ['n10_p2_pbc', 'cfg1_n21_m100', 'cfg3_n42_p27_m60'])
def test_modes_determinism_and_device_entry(name):
    r, pred = _ref(name), _pred(name)
    ctx, lat = pred._ctx, r['lat']
    R = np.ascontiguousarray(np.resize(r['Rq'], (70, r['Rq'].shape[1])))
    B, n3 = R.shape
    full = ctx.predict_cov(R, lat, full=True)
    var = ctx.predict_cov(R, lat, full=False)
    assert var.shape == (B, n3)
    assert np.array_equal(var, np.einsum('bii->bi', full))  # bit for bit
    assert np.array_equal(full, ctx.predict_cov(R, lat, full=True))
    assert np.array_equal(var, ctx.predict_cov(R, lat, full=False))
    _, _, v2 = pred.predict_uncertainty(R)
    assert np.array_equal(v2, var * (pred.std * pred.std * 1.0))
    lib = ctx._lib
    ptrs = [C.c_void_p() for _ in range(3)]
    for p, s in zip(ptrs, [R.nbytes, full.nbytes, var.nbytes]):
        ctx._check(lib.gdml_dev_alloc(ctx._h, s, C.byref(p)))
    try:
        ctx._check(lib.gdml_memcpy_h2d(ctx._h, ptrs[0], R.ctypes.data_as(C.c_void_p), R.nbytes))
        ctx.predict_cov_dev(ptrs[0], B, ptrs[1], lat, full=True)
        ctx.predict_cov_dev(ptrs[0], B, ptrs[2], lat, full=False)
        out = [np.empty_like(full), np.empty_like(var)]
        for p, o in zip(ptrs[1:], out):
            ctx._check(lib.gdml_memcpy_d2h(ctx._h, o.ctypes.data_as(C.c_void_p), p, o.nbytes))
        assert np.array_equal(out[0], full) and np.array_equal(out[1], var)
    finally:
        for p in ptrs:
            lib.gdml_dev_free(ctx._h, p)


@pytest.mark.parametrize('name', CASES)
def test_invariants_of_gpu_output(name):
    r, pred = _ref(name), _pred(name)
    cov = pred._ctx.predict_cov(r['Rq'], r['lat'], full=True)
    for q in range(len(cov)):
        assert np.abs(cov[q] - cov[q].T).max() <= 1e-13 * np.abs(cov[q]).max()
        assert np.all(np.diag(cov[q]) <= np.diag(-r['kqq'][q]) + r['tol'][q])  # never above the prior
    d = np.diag(cov[-1])  # the training geometry: Sig = lam I - lam^2 [A^-1]_ii
    assert np.all(d >= -r['tol'][-1]) and np.all(d <= r['lam'] + r['tol'][-1])


@pytest.mark.parametrize('name', ['n5_p4', 'cfg1_n21_m100'])
def test_calibration(name):
    r = _ref(name)
    m, g = r['model'], r['g']
    pred = GDMLPredict(m)
    pred.prepare_uncertainty(r['R_train'], F_train=g['F_train'])
    y = np.asarray(g['F_train'], dtype=np.float64).ravel() / m['std']
    s2 = -np.dot(y, m['alphas_F']) / y.size
    assert s2 > 0 and abs(pred.uncertainty_scale - s2) <= 1e-12 * s2
    _, _, cov = pred.predict_uncertainty(r['Rq'], full_cov=True)
    raw = pred._ctx.predict_cov(r['Rq'], r['lat'], full=True)
    assert np.array_equal(cov, raw * (m['std'] * m['std'] * pred.uncertainty_scale))
    pred.release_uncertainty()


@pytest.mark.parametrize('name', ['n10_p2_pbc', 'cfg0_n9_p6'])
def test_batch_chunking(name):
    r, pred = _ref(name), _pred(name)
    R = np.resize(r['Rq'], (23, r['Rq'].shape[1]))
    full = pred._ctx.predict_cov(R, r['lat'], full=True)
    Kx, kqq = pred._ctx.uncert_cross(R, r['lat'])
    pred._ctx.set_option('predict.cov_chunk', 5)
    try:
        full5 = pred._ctx.predict_cov(R, r['lat'], full=True)
        Kx5, kqq5 = pred._ctx.uncert_cross(R, r['lat'])
    finally:
        pred._ctx.set_option('predict.cov_chunk', 64)
    assert np.abs(full5 - full).max() <= 1e-13 * np.abs(full).max()
    assert np.array_equal(Kx5, Kx) and np.array_equal(kqq5, kqq)


@pytest.mark.parametrize('name', ['n5_p4', 'n10_p2_pbc', 'cfg3_n42_p27_m60'])
def test_cross_kernel_global_workspace_path(name):
    """The form for molecules whose per-permutation vectors do not fit LDS (N > 374), forced on small ones."""
    r, pred = _ref(name), _pred(name)
    Kx, kqq = pred._ctx.uncert_cross(r['Rq'], r['lat'])
    pred._ctx.set_option('predict.cov_global', 1)
    try:
        Kg, kg = pred._ctx.uncert_cross(r['Rq'], r['lat'])
    finally:
        pred._ctx.set_option('predict.cov_global', 0)
    n3 = r['Rq'].shape[1]
    for q in range(len(r['Rq'])):
        assert np.abs(Kg.reshape(len(kg), n3, -1)[q] - r['Kx'][q]).max() <= ur.TAU * np.abs(r['Kx'][q]).max()
        assert np.abs(kg[q] - r['kqq'][q]).max() <= ur.TAU * np.abs(r['kqq'][q]).max()


def test_error_paths():
    r = _ref('n10_p2_pbc')
    m, R, lat = r['model'], r['Rq'], r['lat']
    pred = GDMLPredict(m)
    with pytest.raises(_lib.GDMLHipError):  # nothing prepared
        pred.predict_uncertainty(R)
    pred.prepare_uncertainty(r['R_train'])
    pred.predict_uncertainty(R)
    pred.release_uncertainty()
    with pytest.raises(_lib.GDMLHipError):
        pred.predict_uncertainty(R)
    pred.prepare_uncertainty(r['R_train'])
    pred._ctx.assemble_K(m['sig'])  # overwrites the factor
    with pytest.raises(_lib.GDMLHipError):
        pred.predict_uncertainty(R)
    with pytest.raises(ValueError):  # geometries in another order
        pred.prepare_uncertainty(r['R_train'][::-1])
    with pytest.raises(ValueError):
        pred.prepare_uncertainty(r['R_train'][:-1])
    pred.prepare_uncertainty(r['R_train'])
    lib, ctx = pred._ctx._lib, pred._ctx
    out = np.empty((len(R), R.shape[1]))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.gdml_predict_cov(ctx._h, vp(R), len(R), vp(np.ascontiguousarray(lat[0])), None, 0, vp(out)) == -1
    assert lib.gdml_predict_cov(ctx._h, None, len(R), None, None, 0, vp(out)) == -1
    assert lib.gdml_predict_cov(ctx._h, vp(R), -1, None, None, 0, vp(out)) == -1
    assert lib.gdml_uncert_cross(ctx._h, vp(R), len(R), vp(np.ascontiguousarray(lat[0])), None, None, None) == -1
    # energy constraints: refused by the host API, and by the library for a factor that carries the energy rows
    ge = _load('n5_p2_ecstr')
    me = ur.model_from_fixture(ge)
    pe = GDMLPredict(me)
    Re = np.asarray(ge['R_train'], dtype=np.float64).reshape(len(ge['R_train']), -1)
    with pytest.raises(NotImplementedError):
        pe.prepare_uncertainty(Re)
    c = pe._ctx
    c.train_upload(ge['R_desc'], ge['R_d_desc'], pe._tril_perms)
    c.uncert_prepare(me['sig'], me['lam'])
    c.assemble_K(me['sig'], True, for_cholesky=me['lam'])
    c.chol_factor(me['lam'])
    with pytest.raises(NotImplementedError):  # GDML_ERR_UNSUPPORTED
        c.predict_cov(Re[:1])

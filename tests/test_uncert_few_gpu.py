"""Low-latency posterior force covariances of a handful of geometries (csrc/uncert_few.hip, gdml_predict_cov_few) against the
NumPy restatement of the covariance (tests/_uncertainty_ref.py): parity within the derived bound (_uncertainty_ref.cov_tol),
the six invariants the header states, the fall-back to gdml_predict_cov beyond the limit, the error paths and the host API."""
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
from test_uncertainty_gpu import _ref as _shared_ref  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
# The fixtures and queries of tests/test_uncertainty_gpu.py (tol_q <= 0.069 min diag Sig_ref there).  Branches of the solve:
# n4_p6_pbc (n = 108, 12 rows) less than one step, fewer rows than one MFMA tile; n5_p4 (150, 15); n10_p2_pbc (360, 30) lattice,
# two steps; cfg0_n9_p6 (5400, 27) ragged last step; cfg1_n21_m100 (6300, 63) one row short of four tiles; cfg3_n42_p27_m60
# (7560, 126) more than 64 rows, 252 rows at B = 2.
CASES = ['n5_p4', 'n10_p2_pbc', 'n4_p6_pbc', 'cfg0_n9_p6', 'cfg1_n21_m100', 'cfg3_n42_p27_m60']
LIMIT = 256  # GDML_COV_FEW_ROWS
RECORD = os.environ.get('GDML_UNCERT_FEW_RECORD', os.path.join(ROOT, 'profiles', 'uncert_few_parity.json'))
_observed = {}


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name + '.npz')))


def _reference(x, gd, tp, lat, sig, lam, Rq):
    A = ur.system_matrix(x, gd, tp, sig, lam)
    Kx, kqq = ur.cross_rows(Rq, x, gd, tp, sig, lat)
    Sig = ur.posterior_cov(Kx, kqq, A)
    nA = float(sla.eigvalsh(A, subset_by_index=[len(A) - 1, len(A) - 1])[0])
    tol = np.array([ur.cov_tol(Kx[q], kqq[q], A, nA) for q in range(len(Rq))])
    return Sig, tol


def _ref(name):
    """Reference values of a fixture: those of tests/test_uncertainty_gpu.py (same fixtures, same queries), computed once per
    session whichever of the two files asks first."""
    return _shared_ref(name)


@functools.lru_cache(maxsize=None)
def _pred(name):
    r = _ref(name)
    pred = GDMLPredict(r['model'])
    pred.prepare_uncertainty(r['R_train'])
    return pred


def _few_launches(ctx):
    return ctx.phase_ms('uncert_few')[1]


@pytest.mark.parametrize('name', CASES)
def test_parity(name):
    """|Sig_few / std^2 - Sig_ref| <= tol_q elementwise, every query alone and the first two together; tol_q is capped at a
    tenth of the smallest reference variance (a condition on the reference values)."""
    r, pred = _ref(name), _pred(name)
    std2 = r['model']['std'] ** 2
    n3 = r['Rq'].shape[1]
    for q in range(len(r['Rq'])):
        assert r['tol'][q] <= 0.1 * np.diag(r['Sig'][q]).min(), q
    batches = [(r['Rq'][q:q + 1], [q]) for q in range(len(r['Rq']))] + [(r['Rq'][:2], [0, 1])]
    worst = 0.0
    for R, idx in batches:
        assert len(R) * n3 <= LIMIT
        E, F, cov = pred.predict_uncertainty(R, full_cov=True, low_latency=True)
        assert _few_launches(pred._ctx) > 0
        assert cov.shape == (len(R), n3, n3)
        for b, q in enumerate(idx):
            ratio = np.abs(cov[b] / std2 - r['Sig'][q]).max() / r['tol'][q]
            print('%s B=%d q=%d  max|dSig| / tol_q = %.3g' % (name, len(R), q, ratio))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (len(R), b, ratio)
    _observed[name] = float('%.3g' % worst)
    if len(_observed) == len(CASES):
        with open(RECORD, 'w') as f:
            json.dump({'what': 'max |Sig_few - Sig_ref| / tol_q per fixture (tests/test_uncert_few_gpu.py; seven queries alone and '
                               'the first two together)', 'ratio': {k: _observed[k] for k in CASES}}, f, indent=1)
            f.write('\n')


@pytest.mark.parametrize('name', ['n10_p2_pbc', 'cfg1_n21_m100', 'cfg3_n42_p27_m60'])
def test_invariants_1_to_4(name):
    r, pred = _ref(name), _pred(name)
    ctx, lat = pred._ctx, r['lat']
    n3 = r['Rq'].shape[1]
    Bmax = LIMIT // n3  # the largest batch that still fits the limit
    assert Bmax >= 2
    R = np.ascontiguousarray(np.resize(r['Rq'], (Bmax, n3)))
    full = ctx.predict_cov_few(R, lat, full=True)
    assert _few_launches(ctx) > 0
    var = ctx.predict_cov_few(R, lat, full=False)
    assert var.shape == (Bmax, n3)
    assert np.array_equal(full, ctx.predict_cov_few(R, lat, full=True))  # 1
    assert np.array_equal(var, ctx.predict_cov_few(R, lat, full=False))
    assert np.array_equal(var, np.einsum('bii->bi', full))  # 3
    lib = ctx._lib
    ptrs = [C.c_void_p() for _ in range(3)]
    for p, s in zip(ptrs, [R.nbytes, full.nbytes, var.nbytes]):
        ctx._check(lib.gdml_dev_alloc(ctx._h, s, C.byref(p)))
    try:  # 2
        ctx._check(lib.gdml_memcpy_h2d(ctx._h, ptrs[0], R.ctypes.data_as(C.c_void_p), R.nbytes))
        ctx.predict_cov_few_dev(ptrs[0], Bmax, ptrs[1], lat, full=True)
        ctx.predict_cov_few_dev(ptrs[0], Bmax, ptrs[2], lat, full=False)
        out = [np.empty_like(full), np.empty_like(var)]
        for p, o in zip(ptrs[1:], out):
            ctx._check(lib.gdml_memcpy_d2h(ctx._h, o.ctypes.data_as(C.c_void_p), p, o.nbytes))
        assert np.array_equal(out[0], full) and np.array_equal(out[1], var)
    finally:
        for p in ptrs:
            lib.gdml_dev_free(ctx._h, p)
    # 4: a's rows whoever shares the call and wherever a stands; (a, b, b ...) up to the largest batch as well
    a, b = r['Rq'][0], r['Rq'][1]
    for fl in (True, False):
        alone = ctx.predict_cov_few(a[None], lat, full=fl)[0]
        assert np.array_equal(ctx.predict_cov_few(np.stack([a, b]), lat, full=fl)[0], alone)
        assert np.array_equal(ctx.predict_cov_few(np.stack([b, a]), lat, full=fl)[1], alone)
        aa = ctx.predict_cov_few(np.stack([a, a]), lat, full=fl)
        assert np.array_equal(aa[0], alone) and np.array_equal(aa[1], alone)
        big = ctx.predict_cov_few(np.stack([b] * (Bmax - 1) + [a]), lat, full=fl)
        assert np.array_equal(big[-1], alone)
    assert np.array_equal(full[0], ctx.predict_cov_few(a[None], lat, full=True)[0])


@pytest.mark.parametrize('name', ['n10_p2_pbc', 'cfg3_n42_p27_m60'])
def test_fallback(name):
    r, pred = _ref(name), _pred(name)
    ctx, lat = pred._ctx, r['lat']
    n3 = r['Rq'].shape[1]
    R = np.ascontiguousarray(np.resize(r['Rq'], (LIMIT // n3 + 1, n3)))  # one geometry beyond the limit
    for fl in (True, False):
        assert np.array_equal(ctx.predict_cov_few(R, lat, full=fl), ctx.predict_cov(R, lat, full=fl))
    one = r['Rq'][:1]
    old = ctx.predict_cov(one, lat, full=True)

    def route(R):
        """(result, launches of the few-row solve, launches of the batched solve) of one call"""
        ctx.profile(True)
        try:
            res = ctx.predict_cov_few(R, lat, full=True)
            return res, ctx.kernel_stat('few_solve')[1], ctx.kernel_stat('uncert_solve')[1]
        finally:
            ctx.profile(False)

    ctx.set_option('predict.cov_few_rows', 0)
    try:
        res, nf, nb = route(one)
        assert np.array_equal(res, old) and (nf, nb) == (0, 1)
        ctx.set_option('predict.cov_few_rows', n3)  # a lowered limit: one geometry fits, two do not
        few1, nf, nb = route(one)
        assert (nf, nb) == (1, 0)
        res, nf, nb = route(r['Rq'][:2])
        assert np.array_equal(res, ctx.predict_cov(r['Rq'][:2], lat, full=True)) and (nf, nb) == (0, 1)
        ctx.set_option('predict.cov_few_rows', 1e6)  # clamped to the kernel's limit
        res, nf, nb = route(R)
        assert np.array_equal(res, ctx.predict_cov(R, lat, full=True)) and (nf, nb) == (0, 1)
    finally:
        ctx.set_option('predict.cov_few_rows', LIMIT)
    # the default takes the new route at B = 1: its phase ran, with launches, and the batched solve did not
    few, nf, nb = route(one)
    assert (nf, nb) == (1, 0)
    assert _few_launches(ctx) > 0
    assert np.array_equal(few, few1)


def test_invariant_5_other_entries_keep_their_bits():
    r, pred = _ref('cfg0_n9_p6'), _pred('cfg0_n9_p6')
    ctx, lat = pred._ctx, r['lat']
    y = np.asarray(r['g']['F_train'], dtype=np.float64).ravel() / r['model']['std'] if 'F_train' in r['g'] else \
        np.cos(np.arange(ctx.K_shape()[0]) * 0.37)

    def others():
        al = ctx.chol_solve(y)
        resid, c, logdet = ctx.loo(al, cov='diag')
        return [ctx.predict_cov(r['Rq'], lat, full=True), ctx.predict_cov(r['Rq'][:1], lat, full=False), al, resid, c, np.array(logdet)]

    before = others()
    ctx.predict_cov_few(r['Rq'][:2], lat, full=True)
    ctx.predict_cov_few(r['Rq'][2:3], lat, full=False)
    assert _few_launches(ctx) > 0
    for u, v in zip(before, others()):
        assert np.array_equal(u, v)


def test_invariant_6_edited_factor():
    """After add_training_points of one test geometry and after remove_training_points([0, 5]) the path is within cov_tol of
    the reference recomputed on the edited training set."""
    r = _ref('n10_p2_pbc')
    g, m, lat = r['g'], r['model'], r['lat']
    tp = ur.fixture_tables(g)[3]
    pred = GDMLPredict(m)
    pred.prepare_uncertainty(r['R_train'], F_train=g['F_train'])
    Rt = np.asarray(g['R_test'], dtype=np.float64).reshape(len(g['R_test']), -1)
    Ft = np.asarray(g['F_test'], dtype=np.float64).reshape(len(Rt), -1)
    Rq = r['Rq'][1:4]
    pred.add_training_points(Rt[:1], Ft[:1])
    R_now = np.concatenate([r['R_train'], Rt[:1]])
    for step in range(2):
        x, gd = orc.desc_from_R(R_now, lat)
        Sig, tol = _reference(x, gd, tp, lat, float(g['sig']), float(g['lam']), Rq)
        for q in range(len(Rq)):
            cov = pred._ctx.predict_cov_few(Rq[q:q + 1], lat, full=True)[0]
            assert _few_launches(pred._ctx) > 0
            ratio = np.abs(cov - Sig[q]).max() / tol[q]
            print('step %d q=%d  max|dSig| / tol_q = %.3g' % (step, q, ratio))
            assert ratio <= 1.0, (step, q, ratio)
        if step == 0:
            pred.remove_training_points([0, 5])
            R_now = np.delete(R_now, [0, 5], axis=0)
    pred.release_uncertainty()


def test_error_paths():
    r = _ref('n10_p2_pbc')
    m, R, lat = r['model'], r['Rq'][:2], r['lat']
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    out = np.empty((len(R), R.shape[1]))
    lat0, lat1 = np.ascontiguousarray(lat[0]), np.ascontiguousarray(lat[1])
    pred = GDMLPredict(m)
    lib, ctx = pred._ctx._lib, pred._ctx
    for fn in (lib.gdml_predict_cov_few, lib.gdml_predict_cov_few_dev):
        assert fn(None, vp(R), len(R), None, None, 0, vp(out)) == -1
    with pytest.raises(_lib.GDMLHipError):  # nothing prepared
        pred.predict_uncertainty(R, low_latency=True)
    pred.prepare_uncertainty(r['R_train'])
    pred.predict_uncertainty(R, low_latency=True)
    pred.release_uncertainty()
    assert lib.gdml_predict_cov_few(ctx._h, vp(R), len(R), vp(lat0), vp(lat1), 0, vp(out)) == -4  # GDML_ERR_STATE
    with pytest.raises(_lib.GDMLHipError):
        pred.predict_uncertainty(R, low_latency=True)
    pred.prepare_uncertainty(r['R_train'])
    pred._ctx.assemble_K(m['sig'])  # overwrites the factor
    assert lib.gdml_predict_cov_few(ctx._h, vp(R), len(R), vp(lat0), vp(lat1), 0, vp(out)) == -4
    with pytest.raises(_lib.GDMLHipError):
        pred.predict_uncertainty(R, low_latency=True)
    pred.prepare_uncertainty(r['R_train'])
    for fn in (lib.gdml_predict_cov_few, lib.gdml_predict_cov_few_dev):  # (the checks come before any pointer is used)
        assert fn(ctx._h, vp(R), len(R), vp(lat0), None, 0, vp(out)) == -1
        assert fn(ctx._h, vp(R), len(R), None, vp(lat1), 0, vp(out)) == -1
        assert fn(ctx._h, None, len(R), vp(lat0), vp(lat1), 0, vp(out)) == -1
        assert fn(ctx._h, vp(R), -1, vp(lat0), vp(lat1), 0, vp(out)) == -1
        assert fn(ctx._h, vp(R), len(R), vp(lat0), vp(lat1), 0, None) == -1
        assert fn(ctx._h, vp(R), 0, vp(lat0), vp(lat1), 0, vp(out)) == 0  # B = 0: nothing to do
    pred.release_uncertainty()
    # energy constraints: the library refuses a factor that carries the energy rows
    ge = _load('n5_p2_ecstr')
    me = ur.model_from_fixture(ge)
    pe = GDMLPredict(me)
    Re = np.asarray(ge['R_train'], dtype=np.float64).reshape(len(ge['R_train']), -1)
    c = pe._ctx
    c.train_upload(ge['R_desc'], ge['R_d_desc'], pe._tril_perms)
    c.uncert_prepare(me['sig'], me['lam'])
    c.assemble_K(me['sig'], True, for_cholesky=me['lam'])
    c.chol_factor(me['lam'])
    oe = np.empty((1, Re.shape[1]))
    assert c._lib.gdml_predict_cov_few(c._h, vp(Re), 1, None, None, 0, vp(oe)) == -6  # GDML_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        c.predict_cov_few(Re[:1])


@pytest.mark.parametrize('name', ['n5_p4', 'cfg1_n21_m100'])
def test_python_entry(name):
    r = _ref(name)
    m, g = r['model'], r['g']
    pred = GDMLPredict(m)
    pred.prepare_uncertainty(r['R_train'], F_train=g['F_train'])  # calibrated: uncertainty_scale != 1
    assert pred.uncertainty_scale != 1.0
    R = r['Rq'][:2]
    for fl in (False, True):
        E, F, cov = pred.predict_uncertainty(R, full_cov=fl, low_latency=True)
        assert _few_launches(pred._ctx) > 0
        Ep, Fp = pred.predict(R)
        assert np.array_equal(E, Ep) and np.array_equal(F, Fp)
        raw = pred._ctx.predict_cov_few(R, r['lat'], full=fl)
        assert np.array_equal(cov, raw * (m['std'] * m['std'] * pred.uncertainty_scale))
        assert cov.shape == ((2, R.shape[1], R.shape[1]) if fl else (2, R.shape[1]))
    E1, F1, v1 = pred.predict_uncertainty(R[0], low_latency=True)  # a single (3N,) geometry
    assert v1.shape == (1, R.shape[1])
    Ed, Fd, vd = pred.predict_uncertainty(R)  # the default keeps its route and bits
    assert np.array_equal(vd, pred._ctx.predict_cov(R, r['lat']) * (m['std'] * m['std'] * pred.uncertainty_scale))
    pred.release_uncertainty()

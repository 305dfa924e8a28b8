"""Adding training points to a resident factor on the GPU (csrc/extend.hip, GDMLPredict.add_training_points) against the
reference values of the FULL system (tests/_extend_ref.py): covariances, solve, leave-one-out errors and log det A within the
bounds the project derives for them, parity with a model prepared from scratch, the integration constant, the exported model
and the replicas, determinism, chunking, a case across panel and tile boundaries, and the failure paths.

The base model holds the first M - b training points of a fixture (its coefficients from a GPU solve of the base system),
the last b are added: b = 1, b = 3, and successive calls of 2, 1 and 4 points (1 and 1 for the fixtures of 9 - 10 points)."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _extend_ref as er  # noqa: E402
import _uncertainty_ref as ur  # noqa: E402
from sgdml_amd import _lib  # noqa: E402
from sgdml_amd.predict import GDMLPredict  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
# The fixtures and queries of tests/test_uncertainty_gpu.py: they pass the meaningfulness cap of the covariance bound with the
# reference values alone (asserted below).  Do not add fixtures or queries without checking them the same way.
CASES = ['n5_p4', 'n10_p2_pbc', 'n4_p6_pbc', 'cfg0_n9_p6', 'cfg1_n21_m100', 'cfg3_n42_p27_m60']
SPLIT_KEYS = ['b1', 'b3', 'seq']
RECORD = os.environ.get('GDML_EXTEND_RECORD', os.path.join(ROOT, 'profiles', 'extend_parity.json'))
_observed = {}


def _load(name):
    return er.synth_fixture() if name == 'synth' else dict(np.load(os.path.join(GOLDEN, name + '.npz')))


@functools.lru_cache(maxsize=None)
def _fix(name):
    """Tables and full-system reference values of a fixture, computed once per session."""
    g = _load(name)
    t = er.tables(g)
    Rq = ur.queries(g)
    return {'g': g, 't': t, 'Rq': Rq, 'ref': er.full_reference(t, Rq)}


@functools.lru_cache(maxsize=None)
def _solved(name, M):
    """Coefficients of the first M points from a from-scratch factorisation and solve on the GPU."""
    t = _fix(name)['t']
    ctx = _lib.Context(0)
    try:
        ctx.train_upload(t['x'][:M], t['gd'][:M], t['tp'])
        ctx.uncert_prepare(t['sig'], t['lam'])
        return ctx.chol_solve(t['F'][:M].ravel() / t['std'])
    finally:
        ctx.close()


def _base(name, Mb, devices=None):
    t = _fix(name)['t']
    pred = GDMLPredict(er.model_dict(t, Mb, _solved(name, Mb)), devices=devices)
    pred.prepare_uncertainty(t['R'][:Mb], F_train=t['F'][:Mb])
    return pred


def _grow(name, steps, devices=None, chunk=None, E=None):
    """A predictor of the base model after one add_training_points call per entry of `steps`."""
    t = _fix(name)['t']
    M = len(t['R'])
    at = M - sum(steps)
    pred = _base(name, at, devices)
    if chunk is not None:
        pred._ctx.set_option('chol.extend_chunk', chunk)
    for k, s in enumerate(steps):
        out = pred.add_training_points(t['R'][at:at + s], t['F'][at:at + s],
                                       E=t['E'][:at + s] if (E is not None and k == len(steps) - 1) else None)
        at += s
        assert out['n_train'] == at == pred.n_train and out['c_updated'] == (E is not None and k == len(steps) - 1)
        assert pred._ctx.K_shape() == (at * t['R'].shape[1], at * t['R'].shape[1], 0)
    return pred


@functools.lru_cache(maxsize=None)
def _grown(name, key):
    return _grow(name, er.splits_of(len(_fix(name)['t']['R']))[key])


def _check_enlarged_model(name, pred):
    """Assertions 1 - 3 of the module docstring's list on a predictor that holds all M points; returns the observed ratios."""
    fx = _fix(name)
    t, ref, Rq = fx['t'], fx['ref'], fx['Rq']
    std, n3 = t['std'], ref['n3']
    for q in range(len(Rq)):  # a condition on the reference values, not a measurement
        assert ref['tol'][q] <= 0.1 * np.diag(ref['Sig'][q]).min(), q
    # 1. covariances in normalised units against the full system, batches of 1 and 7; the public call scales them
    w_cov = 0.0
    for R, idx in ((Rq[:1], [0]), (Rq, range(len(Rq)))):
        raw = pred._ctx.predict_cov(R, t['lat'], full=True)
        var = pred._ctx.predict_cov(R, t['lat'], full=False)
        assert np.array_equal(var, np.einsum('bii->bi', raw))  # bit for bit
        E, F, cov = pred.predict_uncertainty(R, full_cov=True)
        assert np.array_equal(cov, raw * (std * std * pred.uncertainty_scale))
        _, _, v = pred.predict_uncertainty(R)
        assert np.array_equal(v, np.einsum('bii->bi', cov))
        Ep, Fp = pred.predict(R)
        assert np.array_equal(E, Ep) and np.array_equal(F, Fp)
        for b_, q in enumerate(idx):
            ratio = np.abs(raw[b_] - ref['Sig'][q]).max() / ref['tol'][q]
            print('%s B=%d q=%d  max|dSig| / tol_q = %.3g' % (name, len(R), q, ratio))
            w_cov = max(w_cov, ratio)
            assert ratio <= 1.0, (len(R), q, ratio)
    # 2. the solve: residual of the enlarged system (alphas are never compared elementwise)
    A, y = ref['A'], ref['y']
    alphas = pred._alphas_F
    assert alphas.shape == y.shape
    res = np.linalg.norm(A @ (-alphas) - y) / np.linalg.norm(y)
    tol = er.solve_tol(ref['nA'], alphas, y)
    print('%s  residual %.3g  (bound %.3g)' % (name, res, tol))
    assert res <= tol
    # 3. leave-one-out errors, log det A and the calibration on the extended factor
    out = pred.loo_errors(F_train=t['F'])
    resid = out['F_resid'] / std
    w_loo = max(np.abs(resid[j] - ref['r'][j]).max() / ref['loo_tol'][j] for j in range(len(resid)))
    w_ld = abs(out['log_det_A'] - ref['logdet']) / ref['logdet_tol']
    print('%s  worst: r %.3g  log det A %.3g of their bounds;  scale %.12g (ref %.12g)' % (
        name, w_loo, w_ld, pred.uncertainty_scale, ref['scale']))
    assert w_loo <= 1.0 and w_ld <= 1.0
    assert abs(pred.uncertainty_scale - ref['scale']) <= 1e-9 * abs(ref['scale'])
    assert n3 * pred.n_train == len(y)
    return {'cov': float('%.3g' % w_cov), 'residual': float('%.3g' % (res / tol)), 'loo': float('%.3g' % w_loo),
            'logdet': float('%.3g' % w_ld)}


def _record():
    want = {(n, k) for n in CASES for k in SPLIT_KEYS} | {(n, 'retrain') for n in CASES}
    if set(_observed) >= want:
        ratio = {}
        for n in CASES:
            ratio[n] = {c: max(_observed[(n, k)][c] for k in SPLIT_KEYS) for c in ('cov', 'residual', 'loo', 'logdet')}
            ratio[n]['retrain'] = _observed[(n, 'retrain')]
        with open(RECORD, 'w') as f:
            json.dump({'what': 'worst observed value over its bound per fixture after add_training_points '
                               '(tests/test_extend_gpu.py; splits b = 1, b = 3 and successive calls): max |Sig_gpu - Sig_ref| / tol_q, '
                               'solve residual / its bound, max |r_gpu - r_ref| / tol_j, |d log det A| / logdet_tol, and the relative '
                               'difference of force MAE / RMSE to a model prepared from scratch over (1e-7 relative + round-off floor)',
                       'ratio': ratio}, f, indent=1)
            f.write('\n')


@pytest.mark.parametrize('key', SPLIT_KEYS)
@pytest.mark.parametrize('name', CASES)
def test_enlarged_model_against_the_full_system(name, key):
    _observed[(name, key)] = _check_enlarged_model(name, _grown(name, key))
    _record()


@pytest.mark.parametrize('name', CASES)
def test_against_a_model_prepared_from_scratch(name):
    """Force MAE and RMSE on the fixture's test set agree with those of a second predictor whose factor and coefficients
    come from prepare_uncertainty + chol_solve on the full set, to 1e-7 relative (the tolerance of validation errors)
    above the predictor's own round-off: F_test of the small golden fixtures IS the prediction of the fixture's model, so
    both errors are round-off there (1.2e-14 at max|F| = 1 on n5_p4) and a relative comparison of them alone compares
    noise.  Each predictor's forces carry up to _uncertainty_ref.cancel_floor of summation round-off, and a mean or
    root-mean-square of |F - F_test| moves by at most the largest change of F, hence the absolute term 2 floor."""
    fx = _fix(name)
    t, g = fx['t'], fx['g']
    M = len(t['R'])
    pred = _grown(name, 'seq')
    m_scratch = er.model_dict(t, M, _solved(name, M))
    scratch = GDMLPredict(m_scratch)
    Rt = np.asarray(g['R_test'], dtype=np.float64).reshape(len(g['R_test']), -1)
    Ft = np.asarray(g['F_test'], dtype=np.float64).reshape(len(Rt), -1)
    floor = 2.0 * ur.cancel_floor(m_scratch, t['gd'])
    a, b = pred.test_errors(Rt, Ft)['force'], scratch.test_errors(Rt, Ft)['force']
    ratio = max(abs(a[k] - b[k]) / (1e-7 * b[k] + floor) for k in range(2))
    dF = np.abs(pred.predict(Rt)[1] - scratch.predict(Rt)[1]).max()
    print('%s  force MAE %.10g / %.10g  RMSE %.10g / %.10g  floor %.3g  ratio %.3g  max|dF| %.3g' % (
        name, a[0], b[0], a[1], b[1], floor, ratio, dF))
    assert ratio <= 1.0
    _observed[(name, 'retrain')] = float('%.3g' % ratio)
    _record()


@pytest.mark.parametrize('name', ['n5_p4', 'cfg1_n21_m100'])
def test_integration_constant(name):
    fx = _fix(name)
    t = fx['t']
    steps = er.splits_of(len(t['R']))['seq']
    kept = _grown(name, 'seq')
    assert kept.c == t['c']  # no energies given: unchanged
    pred = _grow(name, steps, E=t['E'])
    m0 = pred.export_model()
    m0['c'] = 0.0
    E_pred = GDMLPredict(m0).predict(t['R'])[0]
    want = np.mean(t['E'] - E_pred)
    print('%s  c %.12g  mean(E - E_pred) %.12g' % (name, pred.c, want))
    assert abs(pred.c - want) <= 1e-9 * np.abs(t['E']).max()
    assert pred.export_model()['c'] == pred.c


@pytest.mark.parametrize('name', ['n10_p2_pbc', 'cfg0_n9_p6'])
def test_export_round_trip_and_replicas(name):
    fx = _fix(name)
    t, Rq = fx['t'], fx['Rq']
    steps = er.splits_of(len(t['R']))['seq']
    live = _grown(name, 'seq')
    m = live.export_model()
    M = len(t['R'])
    assert m['R_desc'].shape == (t['x'].shape[1], M) and m['alphas_F'].shape == (M * t['R'].shape[1],)
    assert np.array_equal(m['idxs_train'], np.r_[np.arange(M - sum(steps)), -np.ones(sum(steps), dtype=int)])
    assert np.isnan(m['f_err']['mae']) and np.isnan(m['f_err']['rmse']) and m['std'] == t['std'] and m['lam'] == t['lam']
    fresh = GDMLPredict(m)
    for a, b in zip(live.predict(Rq), fresh.predict(Rq)):
        assert np.array_equal(a, b)
    # two contexts on GPU 0: both replicas must hold the enlarged model (a batch large enough to be split over them)
    big = np.ascontiguousarray(np.resize(Rq, (160, Rq.shape[1])))
    live2 = _grow(name, steps, devices=[0, 0])
    assert len(live2._replicas) == 1 and not live2._replicas_stale
    fresh2 = GDMLPredict(m, devices=[0, 0])
    E2, F2 = live2.predict(big)
    for a, b in zip((E2, F2), fresh2.predict(big)):
        assert np.array_equal(a, b)
    E1, F1 = live.predict(big)  # (a shard may take another kernel than the whole batch: equal to rounding)
    assert np.abs(F1 - F2).max() <= 1e-12 * np.abs(F1).max() and np.abs(E1 - E2).max() <= 1e-12 * np.abs(E1).max()
    assert np.array_equal(live2._alphas_F, live._alphas_F)


@pytest.mark.parametrize('name', ['n10_p2_pbc', 'cfg3_n42_p27_m60'])
def test_determinism(name):
    fx = _fix(name)
    steps = er.splits_of(len(fx['t']['R']))['seq']
    a, b = _grown(name, 'seq'), _grow(name, steps)
    ca = a._ctx.predict_cov(fx['Rq'], fx['t']['lat'], full=True)
    cb = b._ctx.predict_cov(fx['Rq'], fx['t']['lat'], full=True)
    assert np.array_equal(ca, cb) and np.array_equal(a._alphas_F, b._alphas_F)


@pytest.mark.parametrize('name', ['n10_p2_pbc', 'cfg1_n21_m100'])
def test_chunked_extension(name):
    """Five points in one call at chol.extend_chunk = 2: three chunks, the later ones solved against the earlier ones' rows."""
    pred = _grow(name, [5], chunk=2)
    _check_enlarged_model(name, pred)


def test_across_panel_and_tile_boundaries():
    """P = 1, n = 1800: the 288 new rows and columns run across column 1536 (a 512-column panel boundary of the triangular
    solve) and fill more than two 128-row tiles (tests/_extend_ref.SYNTH; the cap is asserted on the CPU as well)."""
    s = er.SYNTH
    n3 = 3 * s['N']
    assert (s['M'] - s['b']) * n3 // 512 < (s['M'] * n3 - 1) // 512 and s['b'] * n3 > 256
    pred = _grow('synth', [s['b']])
    print(_check_enlarged_model('synth', pred))


class _FailingLib(object):
    """The library with gdml_factor_extend answering GDML_ERR_NOT_PD without touching the device."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, k):
        return getattr(self._lib, k)

    def gdml_factor_extend(self, h, x, g, b, info):
        return _lib.ERR_NOT_PD


def test_failures_leave_the_model_as_it_was():
    fx = _fix('n10_p2_pbc')
    t, Rq = fx['t'], fx['Rq']
    M = len(t['R'])
    Mb = M - 3
    # prepared without labels
    pred = GDMLPredict(er.model_dict(t, Mb, _solved('n10_p2_pbc', Mb)))
    pred.prepare_uncertainty(t['R'][:Mb])
    before = pred.predict_uncertainty(Rq, full_cov=True)
    shape = pred._ctx.K_shape()
    with pytest.raises(ValueError):
        pred.add_training_points(t['R'][Mb:], t['F'][Mb:])
    assert pred._ctx.K_shape() == shape and pred.n_train == Mb
    for a, b in zip(before, pred.predict_uncertainty(Rq, full_cov=True)):
        assert np.array_equal(a, b)
    # a matrix that is not positive definite (mocked return of the binding: none is built on the device)
    pred = _base('n10_p2_pbc', Mb)
    before = pred.predict_uncertainty(Rq, full_cov=True)
    alphas, scale = pred._alphas_F.copy(), pred.uncertainty_scale
    real = pred._ctx._lib
    pred._ctx._lib = _FailingLib(real)
    try:
        with pytest.raises(np.linalg.LinAlgError):
            pred.add_training_points(t['R'][Mb:], t['F'][Mb:])
    finally:
        pred._ctx._lib = real
    assert pred._ctx.K_shape() == shape and pred.n_train == Mb and pred._ctx.n_train == Mb
    assert np.array_equal(pred._alphas_F, alphas) and pred.uncertainty_scale == scale
    for a, b in zip(before, pred.predict_uncertainty(Rq, full_cov=True)):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError):  # labels that do not match the geometries
        pred.add_training_points(t['R'][Mb:], t['F'][Mb:-1])
    with pytest.raises(ValueError):
        pred.add_training_points(t['R'][Mb:], t['F'][Mb:], E=t['E'][:Mb])
    assert pred._ctx.K_shape() == shape
    # ... and the same predictor still grows
    pred.add_training_points(t['R'][Mb:], t['F'][Mb:])
    _check_enlarged_model('n10_p2_pbc', pred)


def test_error_codes():
    fx = _fix('n10_p2_pbc')
    t = fx['t']
    lib = _lib.load()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    x, gd = np.ascontiguousarray(t['x'][-1:]), np.ascontiguousarray(t['gd'][-1:])
    info = C.c_int(7)
    ctx = _lib.Context(0)
    assert lib.gdml_factor_extend(ctx._h, vp(x), vp(gd), 1, C.byref(info)) == _lib.ERR_STATE  # no training set
    ctx.train_upload(t['x'][:-1], t['gd'][:-1], t['tp'])
    assert lib.gdml_factor_extend(ctx._h, vp(x), vp(gd), 1, C.byref(info)) == _lib.ERR_STATE  # no prepared factor
    ctx.uncert_prepare(t['sig'], t['lam'])
    shape = ctx.K_shape()
    assert lib.gdml_factor_extend(ctx._h, None, None, 0, C.byref(info)) == _lib.GDML_OK and info.value == 0  # b = 0: a no-op
    assert ctx.factor_extend(x[:0], gd[:0]) == 0 and ctx.K_shape() == shape and ctx.n_train == len(t['x']) - 1
    assert lib.gdml_factor_extend(ctx._h, vp(x), vp(gd), -1, C.byref(info)) == _lib.ERR_INVALID
    assert lib.gdml_factor_extend(ctx._h, None, vp(gd), 1, C.byref(info)) == _lib.ERR_INVALID
    assert ctx.K_shape() == shape
    ctx.assemble_K(t['sig'])  # overwrites the factor
    assert lib.gdml_factor_extend(ctx._h, vp(x), vp(gd), 1, C.byref(info)) == _lib.ERR_STATE
    ctx.close()
    # energy constraints: refused by the host API, and by the library for a factor that carries the energy rows
    ge = dict(np.load(os.path.join(GOLDEN, 'n5_p2_ecstr.npz')))
    me = ur.model_from_fixture(ge)
    pe = GDMLPredict(me)
    Re = np.asarray(ge['R_train'], dtype=np.float64).reshape(len(ge['R_train']), -1)
    with pytest.raises(NotImplementedError):
        pe.add_training_points(Re[:1], Re[:1])
    c = pe._ctx
    c.train_upload(ge['R_desc'], ge['R_d_desc'], pe._tril_perms)
    c.assemble_K(me['sig'], True, for_cholesky=me['lam'])
    c.chol_factor(me['lam'])
    with pytest.raises(NotImplementedError):  # GDML_ERR_UNSUPPORTED
        c.factor_extend(ge['R_desc'][:1], ge['R_d_desc'][:1])

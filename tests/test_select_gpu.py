"""Greedy selection of training points by joint information gain on the GPU (csrc/select.hip,
GDMLPredict.select_training_points) against the NumPy/SciPy reference of tests/_select_ref.py, against the log det A of
loo_errors after add_training_points, against a slow loop of public calls, the bit-level contracts, min_gain / prescreen
and the failure paths.

Pools: the fixture's first 6 - 8 test geometries, a duplicate of pool[0] and R_train[0]; 3 or 4 picks (_select_ref.CASES, which
also records the lam every fixture runs at: the cap of the bounds holds there, tests/test_select_cpu.py asserts it).  The
observed value / bound ratios go to profiles/select_parity.json."""
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
import _select_ref as sr  # noqa: E402
import _uncertainty_ref as ur  # noqa: E402
from sgdml_amd import _lib  # noqa: E402
from sgdml_amd.predict import GDMLPredict  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
CASES = list(sr.CASES)
RECORD = os.environ.get('GDML_SELECT_RECORD', os.path.join(ROOT, 'profiles', 'select_parity.json'))
_observed = {}


@functools.lru_cache(maxsize=None)
def _alphas(name):
    """Coefficients of the case's training set at the case's lam, from a factorisation and solve on the GPU."""
    t = sr.case(name)['t']
    ctx = _lib.Context(0)
    try:
        ctx.train_upload(t['x'], t['gd'], t['tp'])
        ctx.uncert_prepare(t['sig'], t['lam'])
        return ctx.chol_solve(t['F'].ravel() / t['std'])
    finally:
        ctx.close()


def _fresh(name, labelled=True):
    t = sr.case(name)['t']
    pred = GDMLPredict(er.model_dict(t, len(t['R']), _alphas(name)))
    pred.prepare_uncertainty(t['R'], F_train=t['F'] if labelled else None)
    return pred


@functools.lru_cache(maxsize=None)
def _pred(name):
    """A prepared predictor that the tests only read (selection changes nothing)."""
    return _fresh(name)


@functools.lru_cache(maxsize=None)
def _selected(name):
    c = sr.case(name)
    return _pred(name).select_training_points(c['pool'], c['b'])


def _record():
    if set(_observed) >= {(n, k) for n in CASES for k in ('ref', 'logdet')}:
        ratio = {n: dict(_observed[(n, 'ref')], total_gain=_observed[(n, 'logdet')]) for n in CASES}
        with open(RECORD, 'w') as f:
            json.dump({'what': 'worst observed value over its bound per case of tests/test_select_gpu.py: |gain_gpu - gain_ref| / tol_t(q) '
                               'over the picks, the same over the initial gains of the whole pool, and |total_gain - (log det A after '
                               'add_training_points - log det A before - 3N k log lam)| over the sum of the two log det bounds',
                       'lam': {n: sr.case(n)['lam'] for n in CASES}, 'ratio': ratio}, f, indent=1)
            f.write('\n')


@pytest.mark.parametrize('name', CASES)
def test_against_the_reference(name):
    c = sr.case(name)
    ref = c['ref']
    out = _selected(name)
    print('%s  idx %s (ref %s)' % (name, out['idx'], ref['idx']))
    assert out['idx'].dtype == np.int64 and np.array_equal(out['idx'], ref['idx'])
    assert out['gain'].shape == (c['b'],) and out['gain_initial'].shape == (c['B'],) and out['prescreen_exact'] is None
    r_gain = np.abs(out['gain'] - ref['gain']) / ref['tol']
    r_g0 = np.abs(out['gain_initial'] - ref['gain0']) / ref['tol0']
    for t in range(c['b']):
        print('  step %d  gain %.12g  ref %.12g  tol %.3g  ratio %.3g' % (t, out['gain'][t], ref['gain'][t], ref['tol'][t], r_gain[t]))
    print('  initial gains: worst ratio %.3g (tol up to %.3g)' % (r_g0.max(), ref['tol0'].max()))
    assert r_gain.max() <= 1.0 and r_g0.max() <= 1.0
    assert out['total_gain'] == float(np.sum(out['gain'])) and out['phase_ms']['select'] > 0.0
    _observed[(name, 'ref')] = {'gain': float('%.3g' % r_gain.max()), 'gain_initial': float('%.3g' % r_g0.max())}
    _record()


@pytest.mark.parametrize('name', CASES)
def test_total_gain_is_the_growth_of_log_det_A(name):
    """Against loo_errors and add_training_points: total_gain = log det A' - log det A - 3N k log lam, within the sum of the two
    log det bounds (the labels of the added points are arbitrary: log det A does not depend on them)."""
    c = sr.case(name)
    t, ref = c['t'], c['ref']
    out = _selected(name)
    pred = _fresh(name)
    before = pred.loo_errors(F_train=t['F'])['log_det_A']
    k = len(out['idx'])
    pred.add_training_points(c['pool'][out['idx']], np.resize(t['F'][0], (k, c['n3'])))
    after = pred.loo_errors()['log_det_A']
    want = after - before - c['n3'] * k * np.log(c['lam'])
    tol = ref['tol_T'] + ref['tol_final']
    ratio = abs(out['total_gain'] - want) / tol
    print('%s  total_gain %.12g  log det growth %.12g  tol %.3g  ratio %.3g' % (name, out['total_gain'], want, tol, ratio))
    assert ratio <= 1.0
    _observed[(name, 'logdet')] = float('%.3g' % ratio)
    _record()


@pytest.mark.parametrize('name', CASES)
def test_against_a_slow_loop_of_public_calls(name):
    """argmax_q log det(raw_cov_q / lam + I) from predict_cov(full=True), add that geometry, repeat: the same picks."""
    c = sr.case(name)
    t = c['t']
    pred = _fresh(name)
    picks = []
    for _ in range(c['b']):
        raw = pred._ctx.predict_cov(c['pool'], t['lat'], full=True)
        gain = np.array([np.linalg.slogdet(raw[q] / c['lam'] + np.eye(c['n3']))[1] for q in range(c['B'])])
        gain[picks] = -np.inf
        q = int(np.argmax(gain))  # the first of equal maxima
        picks.append(q)
        pred.add_training_points(c['pool'][q:q + 1], t['F'][:1])
    print('%s  slow loop %s  select %s' % (name, picks, _selected(name)['idx']))
    assert np.array_equal(picks, _selected(name)['idx'])


@pytest.mark.parametrize('name', ['n10_p2_pbc', 'cfg0_n9_p6', 'synth132'])
def test_bit_level_contracts(name):
    c = sr.case(name)
    t, pool, B, b = c['t'], c['pool'], c['B'], c['b']
    pred = _pred(name)
    ctx = pred._ctx
    cov0 = ctx.predict_cov(pool, t['lat'], full=True)
    loo0 = ctx.loo(_alphas(name), 'diag')
    first = _selected(name)
    again = pred.select_training_points(pool, b)
    for key in ('idx', 'gain', 'gain_initial'):
        assert np.array_equal(first[key], again[key]), key
    try:
        for chunk in (1, 3, B):
            ctx.set_option('chol.select_chunk', chunk)
            o = pred.select_training_points(pool, b)
            assert np.array_equal(o['idx'], first['idx']), chunk
            assert np.array_equal(o['gain_initial'], first['gain_initial']), chunk
            s = pred.select_training_points(pool, 0)  # the streaming mode
            assert len(s['idx']) == 0 and len(s['gain']) == 0 and s['total_gain'] == 0.0
            assert np.array_equal(s['gain_initial'], first['gain_initial']), chunk
    finally:
        ctx.set_option('chol.select_chunk', 64)
    assert first['gain_initial'][c['dup']] == first['gain_initial'][0]
    if c['ref']['idx'][0] == 0:  # (the cases where the duplicated geometry is the best: the tie goes to the lower index)
        assert first['idx'][0] == 0
    # a pool in another order: every candidate keeps its initial gain bit for bit
    order = np.arange(B)[::-1]
    assert np.array_equal(pred.select_training_points(pool[order], 0)['gain_initial'], first['gain_initial'][order])
    # the factor and the training set were only read
    assert np.array_equal(ctx.predict_cov(pool, t['lat'], full=True), cov0)
    loo1 = ctx.loo(_alphas(name), 'diag')
    assert np.array_equal(loo1[0], loo0[0]) and np.array_equal(loo1[1], loo0[1]) and loo1[2] == loo0[2]


def test_the_duplicate_is_not_picked_twice():
    """The issue's observation: ranking by initial gain takes the copy of pool[0] second, the joint rule does not."""
    c = sr.case('n10_p2_pbc')
    out = _selected('n10_p2_pbc')
    top = np.argsort(-out['gain_initial'], kind='stable')[:c['b']]
    assert c['dup'] in top and c['dup'] not in out['idx'] and list(out['idx']) == [0, 5, 1]


@pytest.mark.parametrize('name', ['n10_p2_pbc', 'n4_p6_pbc'])
def test_min_gain_and_prescreen(name):
    c = sr.case(name)
    ref, pool, b, B = c['ref'], c['pool'], c['b'], c['B']
    pred = _pred(name)
    full = _selected(name)
    for stop in range(1, b):  # the midpoint of two consecutive reference gains stops at that step
        o = pred.select_training_points(pool, b, min_gain=0.5 * (ref['gain'][stop - 1] + ref['gain'][stop]))
        assert np.array_equal(o['idx'], ref['idx'][:stop]) and np.array_equal(o['gain'], full['gain'][:stop])
    assert len(pred.select_training_points(pool, b, min_gain=2.0 * ref['gain'][0])['idx']) == 0
    # prescreen: the K best by initial gain.  K_keep keeps every reference pick; K_exact >= K_keep also leaves the largest
    # dropped initial gain below the last pick's gain (K = B drops nothing)
    rank = np.empty(B, dtype=int)
    rank[np.argsort(-ref['gain0'], kind='stable')] = np.arange(B)
    desc = np.sort(ref['gain0'])[::-1]
    K_keep = max(int(rank[ref['idx']].max()) + 1, b)
    K_exact = next(K for K in range(K_keep, B + 1) if K == B or desc[K] < ref['gain'][-1])
    o = pred.select_training_points(pool, b, prescreen=K_exact)
    print('%s  K_keep %d  K_exact %d of %d' % (name, K_keep, K_exact, B))
    assert np.array_equal(o['idx'], ref['idx']) and np.array_equal(o['gain'], full['gain']) and o['prescreen_exact'] is True
    assert np.array_equal(o['gain_initial'], full['gain_initial'])
    if name == 'n10_p2_pbc':  # picks [0, 5, 1], top three by initial gain {0, 7, 5}: the branch below runs at least here
        assert K_keep > b
    if K_keep > b:  # a K that drops a pick
        o = pred.select_training_points(pool, b, prescreen=K_keep - 1)
        assert o['prescreen_exact'] is False and not np.array_equal(o['idx'], ref['idx'])
    # the joint call reports that the pool does not fit: the prescreen runs by itself with the largest K that fits
    ctx = pred._ctx
    try:
        def fits_at(budget):  # None: the whole pool fits
            ctx.set_option('chol.select_mem_budget', budget)
            try:
                ctx.select_points(pool, c['t']['lat'], b)
            except MemoryError as e:
                assert 'largest pool that fits: ' in str(e)
                return int(str(e).rsplit(': ', 1)[1])
            return None

        lo, hi = 1024.0, 64.0 * 2 ** 20  # nothing fits / everything fits: bisect to the smallest budget that holds the pool
        assert fits_at(lo) == 0 and fits_at(hi) is None
        while hi - lo > 1024.0:
            mid = 0.5 * (lo + hi)
            lo, hi = (lo, mid) if fits_at(mid) is None else (mid, hi)
        budget = lo
        fits = fits_at(budget)
        print('%s  budget %.0f bytes: largest pool that fits %s' % (name, budget, fits))
        assert fits is not None and b <= fits < B
        o = pred.select_training_points(pool, b)
        assert o['prescreen_exact'] is not None and len(o['idx']) == b
        assert np.array_equal(o['gain_initial'], full['gain_initial'])
        if o['prescreen_exact']:
            assert np.array_equal(o['idx'], ref['idx'])
        ctx.set_option('chol.select_mem_budget', 1024.0)  # nothing fits
        with pytest.raises(MemoryError):
            pred.select_training_points(pool, b)
        one = pred.select_training_points(pool, 1)  # a single pick retains nothing: no budget can refuse it
        assert one['prescreen_exact'] is None and np.array_equal(one['idx'], ref['idx'][:1])
        assert np.array_equal(one['gain'], full['gain'][:1]) and np.array_equal(one['gain_initial'], full['gain_initial'])
    finally:
        ctx.set_option('chol.select_mem_budget', 0)
    assert np.array_equal(pred.select_training_points(pool, b)['idx'], ref['idx'])


def test_failure_paths():
    c = sr.case('n10_p2_pbc')
    t, pool, B = c['t'], c['pool'], c['B']
    lib = _lib.load()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    idx, gain, gain0 = np.zeros(B, dtype=np.int64), np.zeros(B), np.zeros(B)
    k, info = C.c_int64(0), C.c_int(7)
    lat, lat_inv = np.ascontiguousarray(t['lat'][0], dtype=np.float64), np.ascontiguousarray(t['lat'][1], dtype=np.float64)

    def call(ctx, R=pool, B_=B, la=lat, li=lat_inv, b=2, idx_=idx, gain_=gain, gain0_=gain0, k_=k):
        return lib.gdml_select_points(ctx._h, None if R is None else vp(R), B_, None if la is None else vp(la),
                                      None if li is None else vp(li), b, -np.inf, None if idx_ is None else vp(idx_),
                                      None if gain_ is None else vp(gain_), None if gain0_ is None else vp(gain0_),
                                      None if k_ is None else C.byref(k_), C.byref(info))

    ctx = _lib.Context(0)
    assert call(ctx) == _lib.ERR_STATE  # no training set
    ctx.train_upload(t['x'], t['gd'], t['tp'])
    assert call(ctx) == _lib.ERR_STATE  # no prepared factor
    ctx.uncert_prepare(t['sig'], t['lam'])
    cov0 = ctx.predict_cov(pool, t['lat'], full=True)
    assert call(ctx, b=B + 1) == _lib.ERR_INVALID
    assert call(ctx, b=-1) == _lib.ERR_INVALID
    assert call(ctx, B_=-1) == _lib.ERR_INVALID
    assert call(ctx, R=None) == _lib.ERR_INVALID
    assert call(ctx, li=None) == _lib.ERR_INVALID  # a lattice without its inverse
    assert call(ctx, idx_=None) == _lib.ERR_INVALID
    assert call(ctx, gain0_=None) == _lib.ERR_INVALID
    assert call(ctx, k_=None) == _lib.ERR_INVALID
    assert call(ctx, B_=0, b=0) == _lib.GDML_OK and k.value == 0
    assert call(ctx) == _lib.GDML_OK and k.value == 2 and info.value == 0  # ... and the context works unchanged
    assert np.array_equal(idx[:2], c['ref']['idx'][:2])
    assert np.array_equal(ctx.predict_cov(pool, t['lat'], full=True), cov0)
    ctx.assemble_K(t['sig'])  # overwrites the factor
    assert call(ctx) == _lib.ERR_STATE
    ctx.close()
    # the public call: before prepare_uncertainty, bad arguments; the predictor works unchanged afterwards
    pred = GDMLPredict(er.model_dict(t, len(t['R']), _alphas('n10_p2_pbc')))
    with pytest.raises(ValueError):
        pred.select_training_points(pool, 2)
    pred.prepare_uncertainty(t['R'])  # without labels: enough for a selection
    for bad in (dict(n_select=B + 1), dict(n_select=-1), dict(n_select=1.5), dict(n_select=2, prescreen=1)):
        with pytest.raises(ValueError):
            pred.select_training_points(pool, **bad)
    with pytest.raises(ValueError):
        pred.select_training_points(pool[:, :-1], 1)
    assert np.array_equal(pred.select_training_points(pool, c['b'])['idx'], c['ref']['idx'])
    pred.release_uncertainty()  # GDML_ERR_STATE of a predictor that had a factor: ValueError as well
    with pytest.raises(ValueError):
        pred.select_training_points(pool, 2)
    pred.prepare_uncertainty(t['R'])
    assert np.array_equal(pred.select_training_points(pool, c['b'])['idx'], c['ref']['idx'])
    # energy constraints: refused by the host API, and by the library for a factor that carries the energy rows
    ge = dict(np.load(os.path.join(GOLDEN, 'n5_p2_ecstr.npz')))
    me = ur.model_from_fixture(ge)
    pe = GDMLPredict(me)
    Re = np.asarray(ge['R_train'], dtype=np.float64).reshape(len(ge['R_train']), -1)
    with pytest.raises(NotImplementedError):
        pe.select_training_points(Re[:2], 1)
    ce = pe._ctx
    ce.train_upload(ge['R_desc'], ge['R_d_desc'], pe._tril_perms)
    ce.assemble_K(me['sig'], True, for_cholesky=me['lam'])
    ce.chol_factor(me['lam'])
    with pytest.raises(NotImplementedError):  # GDML_ERR_UNSUPPORTED
        ce.select_points(Re[:2], None, 1)

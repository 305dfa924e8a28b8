"""Eigenvector following on the GPU (gdml_ef_run, csrc/ef.hip; GDMLPredict.stationary_point): step-by-step parity with the NumPy
restatement (tests/_ef_ref.py) on the fixtures, the toy runs to convergence, a band refined end to end, bit-identity and error
paths.

Bounds.  A compared quantity may deviate from the restatement by ten times the restatement's own deviation under force and
Hessian noise of 1e-10 max and energy noise of 1e-10 max|E'| -- the predictor's agreed accuracy -- measured per case
(_ef_ref.parity_reference, _ef_ref.toy_reference); trust radius, flags and the followed index must match exactly, which
tests/test_ef_cpu.py makes a fair demand: no decision of these runs lies within 1e-6 of its threshold."""
import ctypes as C
import functools
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _ef_ref as er  # noqa: E402
import _neb_ref as nr  # noqa: E402
import _relax_ref as rr  # noqa: E402
import _vib_ref as vr  # noqa: E402
from sgdml_amd import _lib  # noqa: E402
from sgdml_amd._lib import EfParams  # noqa: E402,F401  (the binding of gdml_ef_run: this file tests nothing without it)
from sgdml_amd.predict import GDMLPredict  # noqa: E402

pytestmark = pytest.mark.gpu

BARRIER_SPREAD = (0.0476037, 0.0476058)  # as tests/test_neb_cpu.py records it
OUT_KEYS = ('R_end', 'E_end', 'F_end', 'fmax_end', 'n_steps', 'converged', 'w_end', 'n_rigid', 'n_neg', 'mode_end', 'E_hist',
            'fmax_hist', 'w_follow_hist', 'k_follow_hist')
STATE_KEYS = ('trust', 'E_prev', 'dE_pred', 'flags', 't')


@functools.lru_cache(maxsize=None)
def _pred(name):
    return GDMLPredict(er.parity_start(name)[0])


@functools.lru_cache(maxsize=None)
def _toy_pred(which):
    return GDMLPredict(nr.toy()[0] if which == 'band' else rr.toy()[0])


def _same(a, b, keys=OUT_KEYS, rows=None):
    """Bit for bit, the outputs `keys` and the state (geometry `rows` of a against all of b when given)."""
    def pick(x, axis):
        return x if rows is None or x is None else np.take(x, rows, axis=axis)

    for k in keys:
        axis = 1 if k.endswith('_hist') or k == 'R' else 0
        if not np.array_equal(pick(a[k], axis), b[k]):
            return k
    for k in STATE_KEYS:
        x, y = pick(a['state'][k], 0), b['state'][k]
        if (x is None) != (y is None) or (x is not None and not np.array_equal(x, y)):
            return 'state.' + k
    return None


# ---- 1. parity with the restatement

@pytest.mark.parametrize('B', er.PARITY_BATCHES)
@pytest.mark.parametrize('order,with_follow', er.PARITY_MODES)
@pytest.mark.parametrize('name', er.PARITY_FIXTURES)
def test_parity_with_the_restatement(name, order, with_follow, B):
    m = er.parity_measure(_pred(name), name, order, with_follow, B, chain=er.parity_chain(name, B))
    print('%s order %d follow %d B %d: %s' % (name, order, with_follow, B, ', '.join(
        '%s %.1e / %.1e = %.2g' % (k, m[k]['error'], m[k]['sensitivity'], m[k]['ratio']) for k in er.PARITY_KEYS)))
    assert m['none_converged']
    assert m['k_follow_equal'] and m['trust_equal'] and m['flags_equal'], m
    assert m.get('chain_equal', True)
    for k in er.PARITY_KEYS:
        assert m[k]['ratio'] <= er.BOUND_FACTOR, (k, m[k])


# ---- 2. the toy runs to convergence

@pytest.mark.parametrize('key', sorted(er.TOY_RUNS))
def test_toy_run_to_convergence(key):
    model, R0, follow, order, fmax = er.toy_case(key)
    ref, dev = er.toy_reference(key)
    pred = _toy_pred(er.TOY_RUNS[key][0])
    out = pred.stationary_point(R0, fmax, order=order, follow=follow, max_steps=er.TOY_MAX_STEPS)
    err = np.abs(out['R_end'] - ref['R_end']).max()
    print('%s: steps %s (restated %s), f_atom %s, R_end %.1e against %.1e, n_neg %s' % (
        key, out['n_steps'].tolist(), ref['n_steps'].tolist(), ' '.join('%.1e' % f for f in out['fmax_end']), err, dev['R_end'],
        out['n_neg'].tolist()))
    assert out['converged'].all() and np.array_equal(out['n_steps'], ref['n_steps'])
    assert err <= er.BOUND_FACTOR * dev['R_end']
    assert (out['n_neg'] == order).all() and (out['n_rigid'] == 6).all()
    assert np.array_equal(out['k_follow_hist'], ref['k_follow_hist'])
    assert np.abs(out['w_end'] - ref['w_end']).max() <= er.BOUND_FACTOR * dev['w_end']
    # the same code on the same Hessian
    v = pred.vibrations(out['R_end'], np.ones(R0.shape[1] // 3), modes=True)
    assert np.array_equal(out['w_end'], v['w2']) and np.array_equal(out['n_neg'], v['n_imag'])
    if order == 1:
        assert np.array_equal(out['mode_end'], v['modes'][np.arange(len(R0)), out['k_follow_hist'][-1]])
    else:
        assert not out['mode_end'].any()
    E, F, _ = pred.predict_hessian(out['R_end'])
    assert np.array_equal(out['E_end'], E) and np.array_equal(out['F_end'], F)


def test_band_refined_end_to_end():
    """neb(climb=True) stops at the band's fmax; from its climbing image, following the band tangent, the search reaches 1e-6
    of that, at the same barrier."""
    model, A, Bm, fmax = nr.toy()
    pred = _toy_pred('band')
    path, _ = nr.toy_bands('p4')
    band = pred.neb(path, fmax, k_spring=nr.TOY_K, climb=True, max_steps=nr.TOY_MAX_STEPS)
    assert band['converged'].all()
    ic = int(band['i_climb'][0])
    t = vr.band_tangent(band['R_end'][0], band['E_end'][0], ic)
    out = pred.stationary_point(band['R_end'][0, ic], 1e-6 * fmax, order=1, follow=t, max_steps=20)
    bar = out['E_end'][0] - band['E_end'][0, [0, -1]]
    print('band fmax %.2e -> f_atom %.2e in %d steps; barrier %.8f / %.8f (band %.8f), w %.5f / %.5f' % (
        fmax, out['fmax_end'][0], out['n_steps'][0], bar[0], bar[1], band['barrier'][0, 0], out['w_end'][0, 0], out['w_end'][0, 1]))
    assert out['converged'].all() and out['fmax_end'][0] < 1e-6 * fmax and out['n_steps'][0] <= 6
    assert out['n_neg'][0] == 1 and out['n_rigid'][0] == 6
    assert BARRIER_SPREAD[0] <= bar[0] <= BARRIER_SPREAD[1] and BARRIER_SPREAD[0] <= bar[1] <= BARRIER_SPREAD[1]
    assert abs(out['w_end'][0, 0] - nr.TOY_SADDLE_MODES[0]) < 1e-3 and abs(out['w_end'][0, 1] - nr.TOY_SADDLE_MODES[1]) < 1e-3


# ---- 3. bits

def _batch():
    """Three searches of the band toy that freeze at different evaluations: the tracking start (its followed index changes at
    evaluation 2, its trust radius at 1 and 2), the start on the line and the jittered midpoint, all following the line."""
    _, st = er.toy_starts()
    R0 = np.stack([st['track'], st['line'], st['mid']])
    follow = np.repeat(np.array(st['dir'])[None], 3, axis=0)
    fmax = er.toy_fmax(nr.toy()[0], R0)
    return R0, follow, fmax


def test_repeat_and_continuation():
    pred = _toy_pred('band')
    R0, follow, fmax = _batch()
    kw = dict(order=1, record_every=1)
    whole = pred.stationary_point(R0, fmax, follow=follow, max_steps=4, **kw)
    again = pred.stationary_point(R0, fmax, follow=follow, max_steps=4, **kw)
    assert _same(whole, again, OUT_KEYS + ('R',)) is None
    k = whole['k_follow_hist'][:, 0]
    assert k[1] != k[2], k  # the cut below lies across a change of the followed index ...
    first = pred.stationary_point(R0, fmax, follow=follow, max_steps=2, **kw)
    assert first['state']['trust'][0] != whole['state']['trust'][0]  # ... and of the trust radius
    rest = pred.stationary_point(first['R_end'], fmax, state=first['state'], max_steps=2, **kw)
    assert _same(whole, rest, ('R_end', 'E_end', 'F_end', 'fmax_end', 'w_end', 'n_neg', 'mode_end')) is None
    for key in ('E_hist', 'fmax_hist', 'w_follow_hist', 'k_follow_hist', 'R'):
        assert np.array_equal(np.concatenate([first[key][:2], rest[key]]), whole[key]), key


def test_chunks_frames_and_slices_do_not_matter():
    pred = _toy_pred('band')
    R0, follow, fmax = _batch()
    ref = pred.stationary_point(R0, fmax, follow=follow, max_steps=er.TOY_MAX_STEPS)
    assert ref['converged'].all() and len(set(ref['n_steps'].tolist())) == 3
    ctx = pred._ctx
    try:
        for opt, vals in (('predict.relax_chunk_steps', (1, 5, 32)), ('predict.vib_chunk', (1, 2, 0))):
            for v in vals:
                ctx.set_option(opt, v)
                out = pred.stationary_point(R0, fmax, follow=follow, max_steps=er.TOY_MAX_STEPS)
                assert _same(ref, out) is None, (opt, v, _same(ref, out))
            ctx.set_option(opt, 32 if 'relax' in opt else 0)
        ctx.set_option('predict.md_chunk_frames', 3)
        frames = {}
        for every in (1, 2, 3):
            out = pred.stationary_point(R0, fmax, follow=follow, max_steps=er.TOY_MAX_STEPS, record_every=every)
            assert _same(ref, out) is None, every
            frames[every] = out['R']
        n_made = int(ref['n_steps'].max()) + 1
        assert frames[1].shape == (n_made, 3, 15)
        assert np.array_equal(frames[2], frames[1][::2]) and np.array_equal(frames[3], frames[1][::3])
        assert np.array_equal(frames[1][0], R0) and np.array_equal(frames[1][-1], ref['R_end'])
    finally:
        ctx.set_option('predict.relax_chunk_steps', 32)
        ctx.set_option('predict.vib_chunk', 0)
        ctx.set_option('predict.md_chunk_frames', 0)


def test_alone_frozen_and_neighbouring_calls():
    pred = _toy_pred('band')
    R0, follow, fmax = _batch()
    ones = np.ones(5)
    vib_before = pred.vibrations(R0, ones, modes=True)
    relax_before = pred.relax(R0, nr.toy()[3], max_steps=20)
    ref = pred.stationary_point(R0, fmax, follow=follow, max_steps=er.TOY_MAX_STEPS)
    # a geometry alone against itself in the batch, where predict_hessian has that property
    H3 = pred.predict_hessian(R0)[2]
    for b in range(3):
        if np.array_equal(pred.predict_hessian(R0[b])[2][0], H3[b]):
            one = pred.stationary_point(R0[b], fmax, follow=follow[b], max_steps=er.TOY_MAX_STEPS)
            n = int(one['n_steps'][0]) + 1
            assert _same(ref, one, ('R_end', 'E_end', 'F_end', 'fmax_end', 'n_steps', 'converged', 'w_end', 'n_neg', 'mode_end'),
                         rows=[b]) is None
            assert np.array_equal(ref['E_hist'][:n, b], one['E_hist'][:, 0])
    # a geometry frozen at evaluation m keeps the outputs of a run cut at m while the others run on
    m = int(ref['n_steps'].min())
    b = int(np.argmin(ref['n_steps']))
    cut = pred.stationary_point(R0, fmax, follow=follow, max_steps=m)
    assert cut['converged'][b] and not cut['converged'].all()
    for key in ('R_end', 'E_end', 'F_end', 'fmax_end', 'n_steps', 'w_end', 'n_neg', 'mode_end'):
        assert np.array_equal(ref[key][b], cut[key][b]), key
    for key in STATE_KEYS:
        assert np.array_equal(ref['state'][key][b], cut['state'][key][b]), key
    assert np.array_equal(ref['E_hist'][:m + 1, b], cut['E_hist'][:, b])
    assert (ref['E_hist'][m:, b] == ref['E_hist'][m, b]).all() and (ref['k_follow_hist'][m:, b] == ref['k_follow_hist'][m, b]).all()
    # the end point's energy and forces are predict_hessian's
    E, F, _ = pred.predict_hessian(ref['R_end'])
    assert np.array_equal(ref['E_end'], E) and np.array_equal(ref['F_end'], F)
    # vibrations and relax give the same arrays before and after
    vib_after = pred.vibrations(R0, ones, modes=True)
    relax_after = pred.relax(R0, nr.toy()[3], max_steps=20)
    assert all(np.array_equal(vib_before[k], vib_after[k]) for k in vib_before)
    assert all(np.array_equal(relax_before[k], relax_after[k]) for k in ('R_end', 'E_end', 'F_end', 'E_hist', 'fmax_hist'))


# ---- 4. error paths on the device

def _c_call(ctx, R, N, order=1, project=2):
    B, n3 = R.shape[0], R.shape[1]
    prm = _lib.EfParams(B, N, order, 1.0, None, None, 1e-3, 1e-4, 0.3, project)
    a = [R, np.full(B, 0.1), np.zeros(B), np.zeros(B), np.zeros(B, dtype=np.int64)]
    o = [np.zeros((3, B))] * 3 + [None, np.zeros(B), np.zeros((B, n3)), np.zeros((B, n3)), np.zeros(B, dtype=np.int64),
                                  np.zeros(B, dtype=np.int64), np.zeros((B, n3)), np.zeros((B, 2), dtype=np.int64), None]
    p = _lib._ptr
    rc = ctx._lib.gdml_ef_run(ctx._h, C.byref(prm), *[p(x) for x in a], None, 2, 0, None, *[p(x) for x in o])
    return rc, ctx._lib.gdml_last_error(ctx._h).decode()


def test_error_paths_on_the_device():
    ctx = _lib.Context(0)
    try:
        rc, msg = _c_call(ctx, np.arange(6.0).reshape(1, 6), 2)
        assert rc == _lib.ERR_STATE and 'model' in msg
        rc, msg = _c_call(ctx, np.zeros((1, 594)), 198)
        assert rc == _lib.ERR_UNSUPPORTED
    finally:
        ctx.close()
    pred = _pred('n6_p1')
    _, R0, _ = er.parity_start('n6_p1')
    rc, msg = _c_call(pred._ctx, np.arange(6.0).reshape(1, 6), 2)  # N different from the model's
    assert rc == _lib.ERR_INVALID and 'the model has 6 atoms' in msg, msg
    Rb = R0.copy()
    Rb[2, 7] = np.nan
    rc, msg = _c_call(pred._ctx, Rb, 6)  # refused before any launch
    assert rc == _lib.ERR_INVALID and 'coordinate 7 of geometry 2' in msg, msg
    with pytest.raises(ValueError):
        pred.stationary_point(Rb, 1e-3)
    with pytest.raises(ValueError):
        pred.stationary_point(R0, 1e-3, order=0, follow=np.ones_like(R0))
    empty = pred.stationary_point(np.zeros((0, 18)), 1e-3)
    assert empty['R_end'].shape == (0, 18) and empty['w_end'].shape == (0, 18) and empty['E_hist'].shape[1] == 0
    # max_steps = 0: one evaluation, nothing moves
    one = pred.stationary_point(R0, 1e-12, max_steps=0)
    assert np.array_equal(one['R_end'], R0) and (one['n_steps'] == 0).all() and not one['converged'].any()
    assert np.array_equal(one['state']['flags'], np.zeros(3, dtype=np.int64))


# ---- budgets on the edges of a chunk

@functools.lru_cache(maxsize=None)
def _whole_batch_run():
    R0, follow, fmax = _batch()
    return _toy_pred('band').stationary_point(R0, fmax, follow=follow, max_steps=er.TOY_MAX_STEPS, record_every=1)


def test_budgets_on_chunk_edges_are_the_whole_runs_first_rows():
    """Chunks of 4 evaluations; budgets of 1, 4, 5, 8 and 9 evaluations (one evaluation, the last row of a chunk, the first
    row of the next) with no frames, every evaluation a frame and every third: the four histories and the frames are, bit for
    bit, the first rows of the run to convergence at default options."""
    whole = _whole_batch_run()
    pred = _toy_pred('band')
    R0, follow, fmax = _batch()
    try:
        pred._ctx.set_option('predict.relax_chunk_steps', 4)
        for max_steps, every in itertools.product((0, 3, 4, 7, 8), (0, 1, 3)):
            o = pred.stationary_point(R0, fmax, follow=follow, max_steps=max_steps, record_every=every)
            n = min(max_steps + 1, whole['E_hist'].shape[0])
            for k in ('E_hist', 'fmax_hist', 'w_follow_hist', 'k_follow_hist'):
                assert o[k].shape[0] == n and np.array_equal(o[k], whole[k][:n]), (k, max_steps, every)
            assert ('R' in o) == (every > 0)
            if every:
                assert np.array_equal(o['R'], whole['R'][:n][::every]), (max_steps, every)
    finally:
        pred._ctx.set_option('predict.relax_chunk_steps', 32)

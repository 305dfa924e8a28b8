"""Geometry relaxation on the GPU (gdml_relax_run, csrc/relax.hip; GDMLPredict.relax): step by step against the NumPy
restatement (tests/_relax_ref.py), to convergence on a bound toy model, end state against predict(), determinism, continuation, chunking
and record_every bit for bit, replicas that finish at different steps, edges and error paths."""
import functools
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _md_ref as mr  # noqa: E402
import _relax_ref as rr  # noqa: E402
from sgdml_amd import _lib  # noqa: E402
from sgdml_amd.predict import GDMLPredict  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = ['n6_p1', 'n5_p4', 'n5_p2_ecstr', 'n10_p2_pbc', 'cfg1_n21_m100']  # D <= 256: the shapes of the single-launch route
LARGE = ['cfg3_n42_p27_m60', 'n100_m3']  # D > 256; n100_m3: 300 coordinates for 256 threads
N_EVAL = {'cfg3_n42_p27_m60': 5}  # (its restated forces take a third of a second per call)
ROUTED = [(n, r) for n in SMALL for r in ('step', 'general')] + [(n, 'general') for n in LARGE]
STATE_KEYS = ('V', 'dt', 'alpha', 'n_pos', 'n_taken')
EXACT_STATE = ('dt', 'alpha', 'n_pos', 'n_taken')


def _predictor(model, route='step'):
    """route 'step': the single-launch evaluation where the shape is served (the default); 'general': two pieces."""
    pred = GDMLPredict(model)
    if route == 'general':
        pred._ctx.set_option('predict.relax_fused', 0)
    return pred


@functools.lru_cache(maxsize=None)
def _toy_predictor(route):
    return _predictor(rr.toy()[0], route)


def _same(a, b):
    keys = ['R_end', 'E_end', 'F_end', 'fmax_end', 'n_steps', 'converged', 'E_hist', 'fmax_hist']
    return all(np.array_equal(a[k], b[k]) for k in keys) and all(np.array_equal(a['state'][k], b['state'][k]) for k in STATE_KEYS)


def _sub(state, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in state.items()}


# ---- 1. against the restatement, step by step

@pytest.mark.parametrize('name,route', ROUTED)
def test_steps_match_restatement(name, route):
    """30 evaluations (5 for the largest fixture) from a start in mid-run, nothing converges; B = 1 and 7.  R of every
    evaluation and the end velocities within ten times the restatement's own sensitivity to force errors of 1e-10 max|F| (the
    margin because a systematic error adds up over the steps where the noise does not); E and f_atom of every evaluation
    within that plus the predictor's agreed 1e-10; dt, alpha, n_pos, n_taken exactly (tests/test_relax_cpu.py: no decision
    lies within 1e-6 of its threshold)."""
    n = N_EVAL.get(name, 30)
    model, R0, st, ref, dev = rr.parity_reference(name, n)
    pred = _predictor(model, route)
    for B in (1, 7):
        out = pred.relax(R0[:B], max_steps=n - 1, state=_sub(st, slice(0, B)), record_every=1, **rr.parity_params(name))
        assert out['R'].shape == (n, B, R0.shape[1]) and out['E_hist'].shape == (n, B)
        assert not out['converged'].any() and (out['n_steps'] == n - 1).all()
        err = {'R': np.abs(out['R'] - ref['R'][:, :B]).max(), 'V_end': np.abs(out['state']['V'] - ref['state']['V'][:B]).max(),
               'E_hist': np.abs(out['E_hist'] - ref['E_hist'][:, :B]).max(),
               'fmax_hist': np.abs(out['fmax_hist'] - ref['fmax_hist'][:, :B]).max()}
        for k, e in err.items():
            print('%s %s B=%d %s: sensitivity %.2e, error %.2e' % (name, route, B, k, dev[k], e))
        assert err['R'] <= 10.0 * dev['R'] and err['V_end'] <= 10.0 * dev['V_end']
        for k in ('E_hist', 'fmax_hist'):
            assert err[k] <= 10.0 * dev[k] + 1e-10 * np.abs(ref[k]).max(), k
        for k in EXACT_STATE:
            assert np.array_equal(out['state'][k], ref['state'][k][:B]), k
        assert np.array_equal(out['R_end'], out['R'][-1]) and np.array_equal(out['R'][0], R0[:B])


# ---- 2. to convergence on the toy model

@pytest.mark.parametrize('key', sorted(rr.TOY_PARAMS))
@pytest.mark.parametrize('route', ['step', 'general'])
def test_toy_model_converges_like_the_restatement(route, key):
    """Seven starts of the bound toy model, each stopping at its own step.  The six lowest Hessian eigenvalues at R_end are
    allowed 6e-2 of the seventh: ten times rr.TOY_NULL_RATIO = 6e-3, what tests/test_relax_cpu.py measures (5.3e-3) and
    asserts on the restatement."""
    model, starts, d0, fmax = rr.toy()
    ref, dev = rr.toy_reference(key)
    pred = _toy_predictor(route)
    out = pred.relax(starts, fmax, max_steps=200, **rr.TOY_PARAMS[key])
    print('%s %s: steps %s (restated %s)' % (route, key, out['n_steps'], ref['n_steps']))
    assert np.array_equal(out['n_steps'], ref['n_steps']) and np.array_equal(out['converged'], ref['converged'])
    assert out['converged'].all()
    err = np.abs(out['R_end'] - ref['R_end']).max()
    print('%s %s: R_end error %.2e, sensitivity %.2e' % (route, key, err, dev['R_end']))
    assert err <= 10.0 * dev['R_end']
    for k in EXACT_STATE:
        assert np.array_equal(out['state'][k], ref['state'][k]), k
    assert (out['fmax_end'] < fmax).all()
    assert out['E_hist'].shape == (ref['n_steps'].max() + 1, 7) and (out['E_hist'][-1] < out['E_hist'][0]).all()
    assert np.array_equal(out['E_hist'][-1], out['E_end']) and np.array_equal(out['fmax_hist'][-1], out['fmax_end'])
    assert np.abs(rr.pair_distances(out['R_end']) - d0).max() <= 0.05 * np.abs(rr.pair_distances(starts) - d0).max()
    _, _, H = pred.predict_hessian(out['R_end'])
    for b in range(7):
        w = np.linalg.eigvalsh(0.5 * (H[b] + H[b].T))
        assert w[6] > 0.0 and np.abs(w[:6]).max() <= 10.0 * rr.TOY_NULL_RATIO * w[6], (b, w[:7])


# ---- 3. end state against the predictor

def _end_vs_predict(pred, out, exact):
    E, F = pred.predict(out['R_end'])
    if exact:
        assert np.array_equal(out['E_end'], E) and np.array_equal(out['F_end'], F)
    else:
        eF = np.abs(out['F_end'] - F).max() / np.abs(F).max()
        eE = np.abs(out['E_end'] - E).max() / np.abs(E).max()
        assert eF <= 1e-10 and eE <= 1e-10, (eF, eE)


@pytest.mark.parametrize('name', LARGE)
def test_end_state_is_the_predictors_bits(name):
    """D > 256: predict() of host geometries runs the kernels gdml_predict_dev runs, so E_end and F_end are the bits of
    predict(R_end)."""
    model, R0, st, _, _ = rr.parity_reference(name, N_EVAL.get(name, 30))
    pred = GDMLPredict(model)
    for B in (1, 7):
        out = pred.relax(R0[:B], max_steps=4, state=_sub(st, slice(0, B)), **rr.parity_params(name))
        _end_vs_predict(pred, out, exact=True)


def test_end_state_is_the_predictors_bits_mfma_route():
    model, R7 = mr.case('n9_p1')
    R0 = np.ascontiguousarray(R7[np.arange(256) % len(R7)])  # 256 tiled starts: the MFMA route
    pred = GDMLPredict(model)
    prm = rr.parity_params('n9_p1')
    out = pred.relax(R0, max_steps=4, state=rr.parity_state('n9_p1', 256, R0.shape[1]), **prm)
    _end_vs_predict(pred, out, exact=True)
    # replicas stop on their own here too: a threshold between the f_atom of the starts freezes some at evaluation 0
    f0 = pred.relax(R0, max_steps=0, **prm)['fmax_end']
    out = pred.relax(R0, **dict(prm, fmax=float(np.median(f0[:7])), max_steps=3))
    assert (out['n_steps'][f0 < np.median(f0[:7])] == 0).all() and (out['n_steps'] == 0).any() and (out['n_steps'] > 0).any()
    _end_vs_predict(pred, out, exact=True)


def test_end_state_is_the_predictors_bits_two_entries_per_lane():
    """D = 66 (N = 12, synthetic model): the instance of the single-launch evaluation with two descriptor entries per lane,
    which no fixture reaches.  B = 1 and 7 (252 coordinates: predict() takes its single launch too), six evaluations from
    rest: E_end and F_end are the bits of predict(R_end)."""
    model, R7 = mr.synth_n12()
    pred = GDMLPredict(model)
    for B in (1, 7):
        out = pred.relax(R7[:B], fmax=1e-12, max_steps=5, **mr.SYNTH_RELAX)
        assert out['E_hist'].shape == (6, B) and (out['n_steps'] == 5).all()
        _end_vs_predict(pred, out, exact=True)


@pytest.mark.parametrize('route', ['step', 'general'])
@pytest.mark.parametrize('name', SMALL)
def test_end_state_matches_the_predictor_small_shapes(name, route):
    """D <= 256, B <= 8.  The single-launch evaluation restates the single-launch predictor's row loop, row split and
    reduction order, so where predict() takes its single launch too (at most 384 coordinates) the end state is its bits;
    beyond that, and on the general route, whose device path uses other kernels than predict() of a small host batch, 1e-10
    of the maximum."""
    model, R0, st, _, _ = rr.parity_reference(name, 30)
    pred = _predictor(model, route)
    for B in (1, 7):
        out = pred.relax(R0[:B], max_steps=4, state=_sub(st, slice(0, B)), **rr.parity_params(name))
        _end_vs_predict(pred, out, exact=(route == 'step' and B * R0.shape[1] <= 384))


# ---- 4. bit-identical

@pytest.mark.parametrize('route', ['step', 'general'])
def test_deterministic_continuation_chunks_and_record_every(route):
    model, starts, _, fmax = rr.toy()
    ref, _ = rr.toy_reference('clip')
    pred = _toy_predictor(route)
    prm, n = rr.TOY_PARAMS['clip'], 20
    assert any(any(t <= n for t in ev) for ev in ref['neg_at']) and ref['n_steps'].min() > 2 * n  # a cut behind an event
    full = pred.relax(starts, fmax, max_steps=2 * n, record_every=1, **prm)
    assert _same(full, pred.relax(starts, fmax, max_steps=2 * n, record_every=1, **prm))  # identical calls, identical bits
    a = pred.relax(starts, fmax, max_steps=n, **prm)
    b = pred.relax(a['R_end'], fmax, max_steps=n, state=a['state'], **prm)
    assert (b['state']['n_taken'] == 2 * n).all() and (b['n_steps'] == n).all() and (full['n_steps'] == 2 * n).all()
    for k in ('R_end', 'E_end', 'F_end', 'fmax_end'):
        assert np.array_equal(b[k], full[k]), k
    for k in STATE_KEYS:
        assert np.array_equal(b['state'][k], full['state'][k]), k
    for k in ('E_hist', 'fmax_hist'):  # evaluation 0 of the continuation repeats the last one of the first call
        assert np.array_equal(np.concatenate([a[k], b[k][1:]]), full[k]), k
    whole = pred.relax(starts, fmax, max_steps=200, record_every=1, **prm)  # to convergence: replicas stop on the way
    try:
        for steps in (1, 5):
            pred._ctx.set_option('predict.relax_chunk_steps', steps)
            o = pred.relax(starts, fmax, max_steps=200, record_every=1, **prm)
            assert _same(whole, o) and np.array_equal(whole['R'], o['R']), steps
        pred._ctx.set_option('predict.relax_chunk_steps', 32)
        pred._ctx.set_option('predict.md_chunk_frames', 3)  # the frame bound cuts the chunks instead
        o = pred.relax(starts, fmax, max_steps=200, record_every=1, **prm)
        assert _same(whole, o) and np.array_equal(whole['R'], o['R'])
    finally:
        pred._ctx.set_option('predict.relax_chunk_steps', 32)
        pred._ctx.set_option('predict.md_chunk_frames', 0)
    n_made = whole['n_steps'].max() + 1
    assert whole['R'].shape[0] == n_made and np.array_equal(whole['R'][-1], whole['R_end'])
    for b_ in range(7):  # a frozen replica repeats its end positions
        assert np.array_equal(whole['R'][whole['n_steps'][b_]:, b_], np.broadcast_to(whole['R_end'][b_], (n_made - whole['n_steps'][b_], 18)))
    o0 = pred.relax(starts, fmax, max_steps=200, **prm)
    assert 'R' not in o0 and _same(whole, o0)
    o3 = pred.relax(starts, fmax, max_steps=200, record_every=3, **prm)
    assert _same(whole, o3) and np.array_equal(o3['R'], whole['R'][::3])


# ---- 5. replicas finishing at different steps

@pytest.mark.parametrize('route', ['step', 'general'])
def test_replica_alone_and_in_batch(route):
    """Single-launch route: the row shares of a workgroup belong to one replica, alone is in-batch bit for bit.  General
    route: bit for bit where predict() gives a geometry the same bits alone and in a batch, else to the allowance."""
    model, starts, _, fmax = rr.toy()
    ref, dev = rr.toy_reference('clip')
    pred = _toy_predictor(route)
    prm = rr.TOY_PARAMS['clip']
    batch = pred.relax(starts, fmax, max_steps=200, **prm)
    E7, F7 = pred.predict(starts)
    for q in (0, 4):
        alone = pred.relax(starts[q], fmax, max_steps=200, **prm)
        E1, F1 = pred.predict(starts[q])
        assert alone['n_steps'][0] == batch['n_steps'][q] and alone['converged'][0]
        if route == 'step' or (np.array_equal(F1[0], F7[q]) and np.array_equal(E1[0], E7[q])):
            n = batch['n_steps'][q] + 1
            assert np.array_equal(alone['R_end'][0], batch['R_end'][q]) and np.array_equal(alone['F_end'][0], batch['F_end'][q])
            assert np.array_equal(alone['E_hist'][:, 0], batch['E_hist'][:n, q])
            assert all(np.array_equal(alone['state'][k][0], batch['state'][k][q]) for k in STATE_KEYS)
        else:
            assert np.abs(alone['R_end'][0] - batch['R_end'][q]).max() <= 10.0 * dev['R_end']


@pytest.mark.parametrize('route', ['step', 'general'])
def test_converged_start_stays_put_while_neighbours_run(route):
    model, starts, _, fmax = rr.toy()
    pred = _toy_predictor(route)
    prm = rr.TOY_PARAMS['free']
    first = pred.relax(starts, fmax, max_steps=200, **prm)
    R0 = np.array(starts)
    R0[2] = first['R_end'][2]
    out = pred.relax(R0, fmax, max_steps=200, **prm)
    assert out['n_steps'][2] == 0 and out['converged'][2] and np.array_equal(out['R_end'][2], R0[2])
    assert not out['state']['V'][2].any() and out['state']['n_taken'][2] == 0 and out['state']['dt'][2] == prm['dt_start']
    others = [0, 1, 3, 4, 5, 6]
    assert np.array_equal(out['n_steps'][others], first['n_steps'][others])
    if route == 'step':  # a replica's bits do not depend on its neighbours
        assert np.array_equal(out['R_end'][others], first['R_end'][others])
    assert (out['E_hist'][:, 2] == out['E_end'][2]).all()  # repeats its only value


def test_route_boundary_eight_and_nine_replicas():
    """B = 8 takes the single-launch route, B = 9 the general one: the same steps, positions to the allowance."""
    model, starts, _, fmax = rr.toy()
    ref, dev = rr.toy_reference('clip')
    pred = _toy_predictor('step')
    R9 = np.ascontiguousarray(starts[np.arange(9) % 7])
    o8 = pred.relax(R9[:8], fmax, max_steps=200, **rr.TOY_PARAMS['clip'])
    o9 = pred.relax(R9, fmax, max_steps=200, **rr.TOY_PARAMS['clip'])
    assert np.array_equal(o8['n_steps'], ref['n_steps'][np.arange(8) % 7]) and np.array_equal(o9['n_steps'][:8], o8['n_steps'])
    err = np.abs(o9['R_end'][:8] - o8['R_end']).max()
    print('B = 8 vs B = 9: %.2e (sensitivity %.2e)' % (err, dev['R_end']))
    assert err <= 10.0 * dev['R_end']
    # more than eight replicas: the general route, whatever the option says
    assert _same(o9, _toy_predictor('general').relax(R9, fmax, max_steps=200, **rr.TOY_PARAMS['clip']))


# ---- 6. edges

@pytest.mark.parametrize('route', ['step', 'general'])
def test_budget_edges(route):
    model, starts, _, fmax = rr.toy()
    pred = _toy_predictor(route)
    prm = rr.TOY_PARAMS['clip']
    E, F = pred.predict(starts)
    o = pred.relax(starts, fmax, max_steps=0, record_every=1, **prm)  # one evaluation, no step
    assert (o['n_steps'] == 0).all() and not o['converged'].any() and np.array_equal(o['R_end'], starts)
    assert o['E_hist'].shape == (1, 7) and o['R'].shape == (1, 7, 18) and (o['state']['n_taken'] == 0).all()
    if route == 'step':  # 126 coordinates: predict() takes its single launch too
        assert np.array_equal(o['E_end'], E) and np.array_equal(o['F_end'], F)
    else:
        assert np.abs(o['F_end'] - F).max() <= 1e-10 * np.abs(F).max() and np.abs(o['E_end'] - E).max() <= 1e-10 * np.abs(E).max()
    g = np.sqrt((o['F_end'].reshape(7, 6, 3) ** 2).sum(-1)).max(axis=1)
    assert np.abs(o['fmax_end'] - g).max() <= 4 * np.finfo(float).eps * g.max()
    o = pred.relax(starts, fmax, max_steps=10, **prm)  # a budget that ends before convergence
    assert (o['n_steps'] == 10).all() and not o['converged'].any() and (o['state']['n_taken'] == 10).all()
    assert o['E_hist'].shape == (11, 7)
    o2 = pred.relax(starts, fmax, max_steps=10, f_unit=2.0, **prm)  # the unit factor scales the gradient
    assert not np.array_equal(o2['R_end'], o['R_end']) and np.abs(o2['fmax_hist'][0] - 2.0 * o['fmax_hist'][0]).max() <= 1e-12


def test_lattice_shift_leaves_energies_and_forces():
    """Atoms moved by whole lattice vectors: the minimum image undoes the shift, positions are never wrapped.  To the
    predictor's tolerance of 1e-10 (the shifted coordinates carry a rounding error of eps |lattice vector|)."""
    name = 'n10_p2_pbc'
    model, R0, st, _, _ = rr.parity_reference(name, 30)
    lat = np.asarray(model['lattice'], dtype=np.float64)  # cell vectors in the columns
    shift = np.zeros((10, 3))
    shift[2] = lat[:, 0]
    shift[5] = -lat[:, 1] + lat[:, 2]
    shift[7] = 2 * lat[:, 2]
    pred = GDMLPredict(model)
    kw = dict(max_steps=20, state=_sub(st, slice(0, 2)), **rr.parity_params(name))
    a = pred.relax(R0[:2], **kw)
    b = pred.relax(R0[:2] + shift.ravel()[None], **kw)
    assert np.abs(b['R_end'] - a['R_end'] - shift.ravel()[None]).max() <= 1e-10  # not wrapped
    eF = np.abs(a['F_end'] - b['F_end']).max() / np.abs(a['F_end']).max()
    eE = np.abs(a['E_hist'] - b['E_hist']).max() / np.abs(a['E_hist']).max()
    print('lattice shift: forces %.2e, energies %.2e' % (eF, eE))
    assert eF <= 1e-10 and eE <= 1e-10
    assert _same(a, pred.relax(R0[:2], lattice=lat, **kw))  # the model's own cell per call: the same bits
    assert not np.array_equal(pred.relax(R0[:2], lattice=0.8 * lat, **kw)['F_end'], a['F_end'])  # the argument is not ignored


@pytest.mark.parametrize('route', ['step', 'general'])
def test_error_paths_launch_nothing_and_leave_the_predictor_working(route):
    model, starts, _, fmax = rr.toy()
    pred = _toy_predictor(route)
    R0 = np.array(starts[:3])
    E_ok, F_ok = pred.predict(R0)
    ok = dict(R0=R0, fmax=fmax, max_steps=5)

    def bad(exc=ValueError, **kw):
        with pytest.raises(exc):
            pred.relax(**dict(ok, **kw))
        E, F = pred.predict(R0)
        assert np.array_equal(E, E_ok) and np.array_equal(F, F_ok)

    bad(fmax=0.0)
    bad(fmax=-1.0)
    bad(fmax=float('nan'))
    bad(max_steps=-1)
    bad(dt_start=0.0)
    bad(dt_start=0.5, dt_max=0.4)
    bad(max_step=0.0)
    bad(f_inc=0.9)
    bad(f_dec=1.0)
    bad(f_dec=0.0)
    bad(alpha_start=0.0)
    bad(alpha_start=1.5)
    bad(f_alpha=0.0)
    bad(f_alpha=1.5)
    bad(n_min=-1)
    bad(record_every=-1)
    bad(R0=R0[:, :15])
    bad(state=dict(rr.fresh_state(3, 18), dt=np.array([0.1, -0.1, 0.1])))
    for lattice in (np.eye(2), np.zeros((3, 3))):
        bad(lattice=lattice)
    R_nan = R0.copy()
    R_nan[1, 4] = np.nan
    with pytest.raises(FloatingPointError, match='geometry 1 .* evaluation 0'):
        pred.relax(**dict(ok, R0=R_nan))
    E, F = pred.predict(R0)
    assert np.array_equal(E, E_ok) and np.array_equal(F, F_ok)
    ctx = pred._ctx  # the C boundary: exactly one of lattice / inverse
    with pytest.raises(ValueError):
        ctx.relax_run(R0, fmax, 5, rr.fresh_state(3, 18), 1.0, lat_and_inv=(np.eye(3), None))
    out = pred.relax(**ok)  # and the optimiser itself still works
    assert (out['n_steps'] == 5).all() and np.isfinite(out['E_end']).all()


def test_wrong_atom_count_and_missing_model():
    model, starts, _, fmax = rr.toy()
    ctx = _toy_predictor('step')._ctx
    saved, ctx.model_n_atoms = ctx.model_n_atoms, 5
    try:
        with pytest.raises(ValueError, match='atoms'):
            ctx.relax_run(starts[:1, :15], fmax, 5, rr.fresh_state(1, 15), 1.0)
    finally:
        ctx.model_n_atoms = saved
    empty = _lib.Context(0)
    try:
        empty.model_n_atoms = 6
        with pytest.raises(_lib.GDMLHipError):  # no model resident
            empty.relax_run(starts, fmax, 5, rr.fresh_state(7, 18), 1.0)
    finally:
        empty.close()


# ---- budgets on the edges of a chunk

@functools.lru_cache(maxsize=None)
def _whole_toy_run(route):
    model, starts, _, fmax = rr.toy()
    return _toy_predictor(route).relax(starts, fmax, max_steps=200, record_every=1, **rr.TOY_PARAMS['clip'])


@pytest.mark.parametrize('route', ['step', 'general'])
def test_budgets_on_chunk_edges_are_the_whole_runs_first_rows(route):
    """Chunks of 4 evaluations; budgets of 1, 4, 5, 8 and 9 evaluations (one evaluation, the last row of a chunk, the first
    row of the next) with no frames, every evaluation a frame and every third: every history and the frames are, bit for bit,
    the first rows of the run to convergence at default options."""
    model, starts, _, fmax = rr.toy()
    whole = _whole_toy_run(route)
    pred = _toy_predictor(route)
    try:
        pred._ctx.set_option('predict.relax_chunk_steps', 4)
        for max_steps, every in itertools.product((0, 3, 4, 7, 8), (0, 1, 3)):
            o = pred.relax(starts, fmax, max_steps=max_steps, record_every=every, **rr.TOY_PARAMS['clip'])
            n = min(max_steps + 1, whole['E_hist'].shape[0])
            for k in ('E_hist', 'fmax_hist'):
                assert o[k].shape[0] == n and np.array_equal(o[k], whole[k][:n]), (k, max_steps, every)
            assert ('R' in o) == (every > 0)
            if every:
                assert np.array_equal(o['R'], whole['R'][:n][::every]), (max_steps, every)
    finally:
        pred._ctx.set_option('predict.relax_chunk_steps', 32)

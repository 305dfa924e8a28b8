"""Nudged elastic band on the GPU (gdml_neb_run, csrc/neb.hip; GDMLPredict.neb): step by step against the NumPy restatement
(tests/_neb_ref.py), to convergence on a toy with a barrier, end state against predict(), determinism, continuation, chunking
and record_every bit for bit, bands that freeze at different evaluations, relax() untouched, edges and error paths."""
import functools
import itertools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _neb_ref as nr  # noqa: E402
import _relax_ref as rr  # noqa: E402
from sgdml_amd.predict import GDMLPredict  # noqa: E402

pytestmark = pytest.mark.gpu

STATE_KEYS = ('V', 'dt', 'alpha', 'n_pos', 'n_taken')
EXACT_STATE = ('dt', 'alpha', 'n_pos', 'n_taken')
OUT_KEYS = ('R_end', 'E_end', 'F_end', 'fmax_end', 'n_steps', 'converged', 'i_climb', 'barrier', 's', 'f_tangent', 'Emax_hist',
            'fmax_hist')
BAND_KEYS = ('R_end', 'E_end', 'F_end', 'fmax_end', 'n_steps', 'converged', 'i_climb', 'barrier', 's', 'f_tangent')


@functools.lru_cache(maxsize=None)
def _toy_predictor():
    return GDMLPredict(nr.toy()[0])


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in OUT_KEYS) and all(np.array_equal(a['state'][k], b['state'][k]) for k in STATE_KEYS)


def _toy_run(key, **kw):
    path, climb = nr.toy_bands(key)
    args = dict(k_spring=nr.TOY_K, climb=climb, max_steps=nr.TOY_MAX_STEPS)
    args.update(kw)
    return path, _toy_predictor().neb(path, nr.toy()[3], **args)


# ---- 1. against the restatement, step by step

@pytest.mark.parametrize('climb', [False, True])
@pytest.mark.parametrize('name,P,B', nr.PARITY_CASES)
def test_steps_match_restatement(name, P, B, climb):
    """30 evaluations (5 for the largest fixture) from a start in mid-run, nothing converges.  R of every evaluation and the end
    velocities within ten times the restatement's own sensitivity to force errors of 1e-10 max|F| and energy errors of 1e-10
    max|E'|; the history within that plus the predictor's agreed 1e-10; dt, alpha, n_pos, n_taken and i_climb exactly
    (tests/test_neb_cpu.py: no decision lies within 1e-6 of its threshold)."""
    model, path, st, ref, dev = nr.parity_reference(name, P, B, climb)
    n = nr.PARITY_N_EVAL.get(name, 30)
    pred = GDMLPredict(model)
    out = pred.neb(path, k_spring=nr.PARITY_K, climb=climb, max_steps=n - 1, state=st, record_every=1, **rr.parity_params(name))
    assert out['R'].shape == (n, B, P, path.shape[2]) and out['Emax_hist'].shape == (n, B)
    assert not out['converged'].any() and (out['n_steps'] == n - 1).all()
    err = {'R': np.abs(out['R'] - ref['R']).max(), 'V_end': np.abs(out['state']['V'] - ref['state']['V']).max(),
           'Emax_hist': np.abs(out['Emax_hist'] - ref['Emax_hist']).max(),
           'fmax_hist': np.abs(out['fmax_hist'] - ref['fmax_hist']).max()}
    for k, e in err.items():
        print('%s P=%d B=%d climb=%d %s: sensitivity %.2e, error %.2e' % (name, P, B, climb, k, dev[k], e))
    assert err['R'] <= 10.0 * dev['R'] and err['V_end'] <= 10.0 * dev['V_end']
    for k in ('Emax_hist', 'fmax_hist'):
        assert err[k] <= 10.0 * dev[k] + 1e-10 * np.abs(ref[k]).max(), k
    for k in EXACT_STATE:
        assert np.array_equal(out['state'][k], ref['state'][k]), k
    assert np.array_equal(out['i_climb'], ref['i_climb'])
    assert np.array_equal(out['R_end'], out['R'][-1]) and np.array_equal(out['R'][0], path)
    assert np.array_equal(out['R_end'][:, [0, -1]], path[:, [0, -1]]) and not out['state']['V'][:, [0, -1]].any()
    assert np.abs(out['f_tangent'] - ref['f_tangent']).max() <= 10.0 * dev['f_tangent'] + 1e-10 * np.abs(ref['F_end']).max()
    assert np.abs(out['s'] - ref['s']).max() <= 10.0 * dev['s']


# ---- 2. to convergence on the toy

@pytest.mark.parametrize('key', sorted(nr.TOY_RUNS))
def test_toy_bands_converge_like_the_restatement(key):
    """Bands of a key freeze at different evaluations.  The barrier may differ from the restatement's by the deviation of R_end
    mapped through the forces at the highest image (dE = sum |F_k| dR) plus the predictor's agreed 1e-10 of max|E| (the end
    points do not move: their energies carry only that).  The six null modes of the Hessian at the climbing image are allowed
    ten times nr.TOY_NULL_RATIO, what tests/test_neb_cpu.py measures and asserts on the restatement."""
    model, _, _, fmax = nr.toy()
    _, ref, dev = nr.toy_reference(key)
    path, out = _toy_run(key)
    B = len(path)
    print('%s: steps %s (restated %s), barrier %s' % (key, out['n_steps'], ref['n_steps'], out['barrier'][:, 0]))
    assert np.array_equal(out['n_steps'], ref['n_steps']) and np.array_equal(out['converged'], ref['converged'])
    assert out['converged'].all() and (out['fmax_end'] < fmax).all()
    err = np.abs(out['R_end'] - ref['R_end']).max()
    print('%s: R_end error %.2e, sensitivity %.2e' % (key, err, dev['R_end']))
    assert err <= 10.0 * dev['R_end']
    for k in EXACT_STATE:
        assert np.array_equal(out['state'][k], ref['state'][k]), k
    assert np.array_equal(out['i_climb'], ref['i_climb'])
    F_top = np.abs(ref['F_end'][np.arange(B), ref['i_climb']]).sum(axis=1)
    bound = 10.0 * dev['R_end'] * F_top[:, None] + 1e-10 * np.abs(ref['E_end']).max()
    print('%s: barrier error %.2e, bound %.2e' % (key, np.abs(out['barrier'] - ref['barrier']).max(), bound.min()))
    assert (np.abs(out['barrier'] - ref['barrier']) <= bound).all()
    assert np.array_equal(out['barrier'][:, 0], out['E_end'][np.arange(B), out['i_climb']] - out['E_end'][:, 0])
    assert out['Emax_hist'].shape == (ref['n_steps'].max() + 1, B)
    assert np.array_equal(out['Emax_hist'][-1], out['E_end'][np.arange(B), out['i_climb']])
    assert np.array_equal(out['fmax_hist'][-1], out['fmax_end'])
    for b in range(B):  # E along the band rises to i_climb and falls after it
        E, ic = out['E_end'][b], out['i_climb'][b]
        assert (np.diff(E[:ic + 1]) > 0).all() and (np.diff(E[ic:]) < 0).all()
    seg = np.sqrt(((out['R_end'][:, 1:] - out['R_end'][:, :-1]) ** 2).sum(-1))
    assert (out['s'][:, 0] == 0).all() and np.abs(out['s'][:, 1:] - np.cumsum(seg, axis=1)).max() <= 1e-13
    assert (out['f_tangent'][:, [0, -1]] == 0).all()
    assert np.abs(out['f_tangent'] - ref['f_tangent']).max() <= 10.0 * dev['f_tangent'] + 1e-10 * np.abs(ref['F_end']).max()
    if nr.TOY_RUNS[key][1]:
        _, _, H = _toy_predictor().predict_hessian(out['R_end'][np.arange(B), out['i_climb']])
        for b in range(B):
            w = np.linalg.eigvalsh(0.5 * (H[b] + H[b].T))
            order = np.argsort(np.abs(w))
            null, rest = w[order[:6]], np.sort(w[order[6:]])
            assert rest[0] < 0.0 and rest[1] > 0.0 and np.abs(null).max() <= 10.0 * nr.TOY_NULL_RATIO * rest[1], (b, w)


# ---- 3. end state against the predictor

def _end_vs_predict(pred, out, exact):
    B, P, n3 = out['R_end'].shape
    E, F = pred.predict(out['R_end'].reshape(B * P, n3))
    E, F = E.reshape(B, P), F.reshape(B, P, n3)
    if exact:
        assert np.array_equal(out['E_end'], E) and np.array_equal(out['F_end'], F)
    else:
        eF = np.abs(out['F_end'] - F).max() / np.abs(F).max()
        eE = np.abs(out['E_end'] - E).max() / np.abs(E).max()
        assert eF <= 1e-10 and eE <= 1e-10, (eF, eE)


@pytest.mark.parametrize('name,P,B', [c for c in nr.PARITY_CASES if c[0] in ('cfg3_n42_p27_m60', 'n100_m3')])
def test_end_state_is_the_predictors_bits(name, P, B):
    """D > 256: predict() of host geometries runs the kernels gdml_predict_dev runs, so E_end and F_end are the bits of
    predict() of the B P geometries of R_end."""
    model, path, st = nr.parity_band(name, P, B)
    pred = GDMLPredict(model)
    out = pred.neb(path, k_spring=nr.PARITY_K, climb=True, max_steps=4, state=st, **rr.parity_params(name))
    _end_vs_predict(pred, out, exact=True)


def test_end_state_is_the_predictors_bits_mfma_route():
    model, path, st = nr.parity_band('n9_p1', 4, 64)  # 256 geometries: the MFMA route
    pred = GDMLPredict(model)
    out = pred.neb(path, k_spring=nr.PARITY_K, climb=True, max_steps=4, state=st, **rr.parity_params('n9_p1'))
    _end_vs_predict(pred, out, exact=True)


@pytest.mark.parametrize('name,P,B', [('n6_p1', 7, 3), ('n5_p4', 3, 3), ('n10_p2_pbc', 7, 3), ('cfg1_n21_m100', 4, 3)])
def test_end_state_matches_the_predictor_small_shapes(name, P, B):
    """D <= 256, few geometries: predict() of a small host batch may take other kernels than the device path: 1e-10."""
    model, path, st = nr.parity_band(name, P, B)
    pred = GDMLPredict(model)
    out = pred.neb(path, k_spring=nr.PARITY_K, climb=True, max_steps=4, state=st, **rr.parity_params(name))
    _end_vs_predict(pred, out, exact=False)


# ---- 4. bit-identical

def test_deterministic_continuation_chunks_and_record_every():
    pred = _toy_predictor()
    fmax = nr.toy()[3]
    _, ref, _ = nr.toy_reference('p8')
    n = 10  # the cut lies behind a negative-power event and a change of the climbing image
    assert any(t <= n for t in ref['neg_at'][0]) and len(set(ref['climb_at'][0][:n + 1])) >= 2 and ref['n_steps'][0] > 2 * n
    path, full = _toy_run('p8', max_steps=2 * n, record_every=1)
    assert _same(full, _toy_run('p8', max_steps=2 * n, record_every=1)[1])  # identical calls, identical bits
    _, a = _toy_run('p8', max_steps=n)
    b = pred.neb(a['R_end'], fmax, k_spring=nr.TOY_K, climb=True, max_steps=n, state=a['state'])
    assert (b['state']['n_taken'] == 2 * n).all() and (b['n_steps'] == n).all() and (full['n_steps'] == 2 * n).all()
    for k in BAND_KEYS:
        if k != 'n_steps':
            assert np.array_equal(b[k], full[k]), k
    for k in STATE_KEYS:
        assert np.array_equal(b['state'][k], full['state'][k]), k
    for k in ('Emax_hist', 'fmax_hist'):  # evaluation 0 of the continuation repeats the last one of the first call
        assert np.array_equal(np.concatenate([a[k], b[k][1:]]), full[k]), k
    # the two-phase use is such a continuation: without climbing first, then climbing
    _, plain = _toy_run('p8', climb=False, max_steps=30)
    two = pred.neb(plain['R_end'], fmax, k_spring=nr.TOY_K, climb=True, state=plain['state'], max_steps=nr.TOY_MAX_STEPS)
    assert two['converged'].all() and abs(two['barrier'][0, 0] - nr.TOY_BARRIER) <= 2e-6

    path, whole = _toy_run('p8_x3', record_every=1)  # to convergence: bands freeze on the way
    try:
        for steps in (1, 5):
            pred._ctx.set_option('predict.relax_chunk_steps', steps)
            o = _toy_run('p8_x3', record_every=1)[1]
            assert _same(whole, o) and np.array_equal(whole['R'], o['R']), steps
        pred._ctx.set_option('predict.relax_chunk_steps', 32)
        pred._ctx.set_option('predict.md_chunk_frames', 3)  # the frame bound cuts the chunks instead
        o = _toy_run('p8_x3', record_every=1)[1]
        assert _same(whole, o) and np.array_equal(whole['R'], o['R'])
    finally:
        pred._ctx.set_option('predict.relax_chunk_steps', 32)
        pred._ctx.set_option('predict.md_chunk_frames', 0)
    n_made = whole['n_steps'].max() + 1
    assert whole['R'].shape == (n_made,) + path.shape and np.array_equal(whole['R'][-1], whole['R_end'])
    assert np.array_equal(whole['R'][0], path)
    for b_ in range(len(path)):  # a frozen band repeats its end positions
        assert (whole['R'][whole['n_steps'][b_]:, b_] == whole['R_end'][b_][None]).all()
    o0 = _toy_run('p8_x3')[1]
    assert 'R' not in o0 and _same(whole, o0)
    o3 = _toy_run('p8_x3', record_every=3)[1]
    assert _same(whole, o3) and np.array_equal(o3['R'], whole['R'][::3])


def test_frozen_band_keeps_its_bits_while_others_run_on():
    """A run cut at the evaluation at which the first band converges gives that band the outputs it has in the full run, in
    which the other bands go on for tens of evaluations."""
    path, whole = _toy_run('p8_x3')
    first = int(np.argmin(whole['n_steps']))
    m = int(whole['n_steps'][first])
    assert (np.delete(whole['n_steps'], first) > m + 3).all()
    _, cut = _toy_run('p8_x3', max_steps=m)
    assert cut['converged'][first] and not np.delete(cut['converged'], first).any()
    for k in BAND_KEYS:
        assert np.array_equal(cut[k][first], whole[k][first]), k
    for k in STATE_KEYS:
        assert np.array_equal(cut['state'][k][first], whole['state'][k][first]), k
    assert np.array_equal(whole['R_end'][:, [0, -1]], path[:, [0, -1]]) and not whole['state']['V'][:, [0, -1]].any()
    assert (whole['Emax_hist'][m:, first] == whole['Emax_hist'][m, first]).all()  # repeats its last value


def test_band_alone_and_in_batch():
    """Bit for bit where predict() gives the band's images the same bits alone and in the batch, else to the allowance."""
    pred = _toy_predictor()
    _, ref, dev = nr.toy_reference('p4_x3')
    path, batch = _toy_run('p4_x3')
    B, P, n3 = path.shape
    E3, F3 = pred.predict(path.reshape(B * P, n3))
    for q in (0, 2):
        alone = pred.neb(path[q], nr.toy()[3], k_spring=nr.TOY_K, climb=True, max_steps=nr.TOY_MAX_STEPS)
        E1, F1 = pred.predict(path[q])
        assert alone['n_steps'][0] == batch['n_steps'][q] and alone['converged'][0]
        if np.array_equal(F1, F3.reshape(B, P, n3)[q]) and np.array_equal(E1, E3.reshape(B, P)[q]):
            for k in BAND_KEYS:
                assert np.array_equal(alone[k][0], batch[k][q]), k
            assert all(np.array_equal(alone['state'][k][0], batch['state'][k][q]) for k in STATE_KEYS)
        else:
            assert np.abs(alone['R_end'][0] - batch['R_end'][q]).max() <= 10.0 * dev['R_end']


# ---- 5. relax() keeps its bits

def test_relax_is_untouched_by_a_band_run_on_the_same_context():
    """relax() on both of its routes gives the same arrays before and after a neb() call on the same context."""
    pred = _toy_predictor()
    _, A, Bm, fmax = nr.toy()
    starts = np.stack([A, Bm, A])[:, None, :].repeat(3, axis=1).reshape(9, -1)
    starts = starts + 0.05 * np.random.RandomState(4).standard_normal(starts.shape)

    def both_routes():
        outs = []
        for fused, R0 in ((1, starts[:3]), (0, starts)):
            pred._ctx.set_option('predict.relax_fused', fused)
            outs.append(pred.relax(R0, fmax, max_steps=60, record_every=7))
        pred._ctx.set_option('predict.relax_fused', 1)
        return outs

    keys = ('R_end', 'E_end', 'F_end', 'fmax_end', 'n_steps', 'converged', 'E_hist', 'fmax_hist', 'R')
    before = both_routes()
    _toy_run('p4_x3', max_steps=40)
    after = both_routes()
    for o, p in zip(before, after):
        assert all(np.array_equal(o[k], p[k]) for k in keys)
        assert all(np.array_equal(o['state'][k], p['state'][k]) for k in STATE_KEYS)
        assert (o['n_steps'] > 0).all()


# ---- 6. edges and error paths

def test_budget_edges():
    pred = _toy_predictor()
    fmax = nr.toy()[3]
    path, o = _toy_run('p4_x3', max_steps=0, record_every=1)  # one evaluation, no step
    B, P, n3 = path.shape
    assert (o['n_steps'] == 0).all() and not o['converged'].any() and np.array_equal(o['R_end'], path)
    assert o['Emax_hist'].shape == (1, B) and o['R'].shape == (1, B, P, n3) and (o['state']['n_taken'] == 0).all()
    assert not o['state']['V'].any()
    _end_vs_predict(pred, o, exact=False)
    ref_F, ref_t = zip(*[nr.band_force(path[b], o['E_end'][b], o['F_end'][b], nr.TOY_K, True) for b in range(B)])
    f_atom = np.sqrt((np.array(ref_F).reshape(B, P * 5, 3) ** 2).sum(-1)).max(axis=1)
    assert np.abs(o['fmax_end'] - f_atom).max() <= 1e-13 and np.abs(o['f_tangent'] - np.array(ref_t)).max() <= 1e-13
    _, o = _toy_run('p4_x3', max_steps=10)  # a budget that ends before convergence
    assert (o['n_steps'] == 10).all() and not o['converged'].any() and (o['state']['n_taken'] == 10).all()
    assert o['Emax_hist'].shape == (11, B)
    _, o2 = _toy_run('p4_x3', max_steps=10, f_unit=2.0)  # the unit factor scales the gradient, not the springs
    assert not np.array_equal(o2['R_end'], o['R_end'])
    _, o3 = _toy_run('p4_x3', max_steps=10, k_spring=2.0 * nr.TOY_K)
    assert not np.array_equal(o3['R_end'], o['R_end'])
    # a band that is converged at evaluation 0 stays put while the others run
    _, done = _toy_run('p4_x3')
    start = np.array(path)
    start[1] = done['R_end'][1]
    again = pred.neb(start, fmax, k_spring=nr.TOY_K, climb=True, max_steps=nr.TOY_MAX_STEPS)
    assert again['n_steps'][1] == 0 and again['converged'][1] and np.array_equal(again['R_end'][1], start[1])
    assert not again['state']['V'][1].any() and again['state']['n_taken'][1] == 0
    assert np.array_equal(again['n_steps'][[0, 2]], done['n_steps'][[0, 2]]) and again['converged'].all()
    empty = pred.neb(np.zeros((0, 4, n3)), fmax, k_spring=nr.TOY_K)  # no band: relax() accepts no geometry too
    assert empty['R_end'].shape == (0, 4, n3) and empty['barrier'].shape == (0, 2) and empty['n_steps'].shape == (0,)
    one = pred.neb(path[0], fmax, k_spring=nr.TOY_K, climb=True, max_steps=3)  # (P, 3N): one band
    assert one['R_end'].shape == (1, P, n3)


def test_error_paths_launch_nothing_and_leave_the_predictor_working():
    pred = _toy_predictor()
    fmax = nr.toy()[3]
    path, _ = nr.toy_bands('p4_x3')
    B, P, n3 = path.shape
    flat = path.reshape(B * P, n3)
    E_ok, F_ok = pred.predict(flat)
    ok = dict(R_path=path, fmax=fmax, k_spring=nr.TOY_K, max_steps=5)

    def bad(exc=ValueError, **kw):
        with pytest.raises(exc):
            pred.neb(**dict(ok, **kw))
        E, F = pred.predict(flat)
        assert np.array_equal(E, E_ok) and np.array_equal(F, F_ok)

    bad(fmax=0.0)
    bad(fmax=float('nan'))
    bad(k_spring=0.0)
    bad(k_spring=float('inf'))
    bad(max_steps=-1)
    bad(dt_start=0.0)
    bad(dt_start=0.5, dt_max=0.4)
    bad(max_step=0.0)
    bad(f_inc=0.9)
    bad(f_dec=1.0)
    bad(alpha_start=1.5)
    bad(f_alpha=0.0)
    bad(n_min=-1)
    bad(record_every=-1)
    bad(R_path=path[:, :2])
    bad(R_path=path[:, :, :12])
    bad(state=dict(nr.fresh_state(B, P, n3), dt=np.array([0.1, -0.1, 0.1])))
    for lattice in (np.eye(2), np.zeros((3, 3))):
        bad(lattice=lattice)
    R_nan = path.copy()
    R_nan[1, 2, 4] = np.nan
    with pytest.raises(FloatingPointError, match='band 1 .* evaluation 0'):
        pred.neb(**dict(ok, R_path=R_nan))
    R_nan = path.copy()
    R_nan[2, 0, 0] = np.nan  # an end point
    with pytest.raises(FloatingPointError, match='band 2 .* evaluation 0'):
        pred.neb(**dict(ok, R_path=R_nan))
    E, F = pred.predict(flat)
    assert np.array_equal(E, E_ok) and np.array_equal(F, F_ok)
    out = pred.neb(**ok)  # and the band itself still works
    assert (out['n_steps'] == 5).all() and np.isfinite(out['E_end']).all()


# ---- budgets on the edges of a chunk

@functools.lru_cache(maxsize=None)
def _whole_toy_run():
    return _toy_run('p8_x3', record_every=1)[1]


def test_budgets_on_chunk_edges_are_the_whole_runs_first_rows():
    """Chunks of 4 evaluations; budgets of 1, 4, 5, 8 and 9 evaluations (one evaluation, the last row of a chunk, the first
    row of the next) with no frames, every evaluation a frame and every third: every history and the frames are, bit for bit,
    the first rows of the run to convergence at default options."""
    whole = _whole_toy_run()
    pred = _toy_predictor()
    try:
        pred._ctx.set_option('predict.relax_chunk_steps', 4)
        for max_steps, every in itertools.product((0, 3, 4, 7, 8), (0, 1, 3)):
            o = _toy_run('p8_x3', max_steps=max_steps, record_every=every)[1]
            n = min(max_steps + 1, whole['Emax_hist'].shape[0])
            for k in ('Emax_hist', 'fmax_hist'):
                assert o[k].shape[0] == n and np.array_equal(o[k], whole[k][:n]), (k, max_steps, every)
            assert ('R' in o) == (every > 0)
            if every:
                assert np.array_equal(o['R'], whole['R'][:n][::every]), (max_steps, every)
    finally:
        pred._ctx.set_option('predict.relax_chunk_steps', 32)

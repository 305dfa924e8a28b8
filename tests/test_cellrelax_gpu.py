"""Variable-cell relaxation on the GPU (gdml_cell_relax_run, csrc/cellrelax.hip; GDMLPredict.relax_cell): with the cell masked
out it is relax() bit for bit; step by step against the NumPy restatement (tests/_cellrelax_ref.py); the periodic toy to
convergence; end state against the per-geometry-lattice predictor; determinism, continuation, chunking and record_every bit for
bit; geometries that finish at different steps; frames; edges and error paths."""
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

import _cellrelax_ref as cr  # noqa: E402
import _relax_ref as rr  # noqa: E402
from sgdml_amd import _lib  # noqa: E402
from sgdml_amd.predict import GDMLPredict, check_lattice  # noqa: E402

pytestmark = pytest.mark.gpu

STATE_KEYS = ('S', 'C', 'L0', 'V', 'dt', 'alpha', 'n_pos', 'n_taken')
OUT_KEYS = ('R_end', 'lattice_end', 'E_end', 'F_end', 'stress_end', 'vol_end', 'fmax_end', 'n_steps', 'converged', 'E_hist',
            'vol_hist', 'fmax_hist')


@functools.lru_cache(maxsize=None)
def _toy_predictor():
    return GDMLPredict(cr.toy()[0])


def _same(a, b, keys=OUT_KEYS):
    return all(np.array_equal(a[k], b[k]) for k in keys) and all(np.array_equal(a['state'][k], b['state'][k]) for k in STATE_KEYS)


def _toy_kw(pressure=cr.TOY_PRESSURE, **kw):
    model, starts, L_starts, d0, fmax = cr.toy()
    return dict(dict(R0=starts, fmax=fmax, lattices=L_starts, pressure=pressure, max_steps=400, **cr.TOY_FIRE), **kw)


# ---- 1. the cell masked out: relax() on the general route, bit for bit

def _masked_equals_relax(pred, R0, lattice, fire_state, **prm):
    B, n3 = R0.shape
    ctx = pred._ctx
    ctx.set_option('predict.relax_fused', 0)
    try:
        ref = pred.relax(R0, state=fire_state, lattice=lattice, **prm)
    finally:
        ctx.set_option('predict.relax_fused', 1)
    N = n3 // 3
    lat = check_lattice(lattice)[0]
    st = None
    if fire_state is not None:
        st = dict(fire_state, S=R0, C=np.broadcast_to(float(N) * np.eye(3), (B, 3, 3)), L0=np.broadcast_to(lat, (B, 3, 3)),
                  V=np.concatenate([fire_state['V'], np.zeros((B, 9))], axis=1))
    out = pred.relax_cell(R0, lattice=lattice, mask=np.zeros((3, 3)), pressure=0.0, state=st, **prm)
    for k in ('R_end', 'E_end', 'F_end', 'E_hist', 'fmax_hist', 'n_steps', 'converged', 'fmax_end'):
        assert np.array_equal(out[k], ref[k]), k
    for k in ('dt', 'alpha', 'n_pos', 'n_taken'):
        assert np.array_equal(out['state'][k], ref['state'][k]), k
    assert np.array_equal(out['state']['V'][:, :n3], ref['state']['V']) and not out['state']['V'][:, n3:].any()
    assert np.array_equal(out['state']['S'], ref['R_end'])  # Fd = I: s are the positions
    assert np.array_equal(out['lattice_end'], np.broadcast_to(lat, (B, 3, 3)))
    assert np.array_equal(out['state']['C'], np.broadcast_to(float(N) * np.eye(3), (B, 3, 3)))
    return out


def test_masked_cell_is_relax_bit_for_bit_on_the_toy():
    model, starts, L_starts, d0, fmax = cr.toy()
    for key in sorted(rr.TOY_PARAMS):  # clipped steps and free steps; to convergence in the fixed cell or 60 steps
        out = _masked_equals_relax(_toy_predictor(), np.array(starts), model['lattice'], None, fmax=fmax, max_steps=60,
                                   **rr.TOY_PARAMS[key])
        assert out['E_hist'].shape[0] >= 2
    _masked_equals_relax(_toy_predictor(), np.array(starts[3:4]), L_starts[3], None, fmax=fmax, max_steps=25, **rr.TOY_PARAMS['free'])


def test_masked_cell_is_relax_bit_for_bit_on_the_fixture():
    name = 'n10_p2_pbc'
    model, R0, st, _, _ = rr.parity_reference(name, 30)
    pred = GDMLPredict(model)
    for B in (1, 7):
        sub = {k: np.ascontiguousarray(v[:B]) for k, v in st.items()}
        _masked_equals_relax(pred, np.ascontiguousarray(R0[:B]), model['lattice'], sub, max_steps=29, **rr.parity_params(name))


# ---- 2. against the restatement, step by step

@pytest.mark.parametrize('name', cr.PARITY_FIXTURES)
def test_steps_match_restatement(name):
    """30 evaluations from a start in mid-run with Fd != I, mask = 1 and pressure 0.01; nothing converges; B = 1 and 7.  The
    Cartesian frame and the lattice of every evaluation (which is also the check of every recorded frame: R_rec = Fd s and
    lat_rec = Fd L0 of the restated state) and the end velocities within ten times the restatement's own sensitivity to noise
    of 1e-10 on E, F and W; E, Vol and f_atom of every evaluation within that plus the predictor's agreed 1e-10; dt, alpha,
    n_pos, n_taken exactly.  The scheme and the factor are tests/test_relax_gpu.py's; tools/cellrelax_parity.py records the
    same measurement in profiles/cellrelax_parity.json."""
    pred = GDMLPredict(cr.parity_case(name)[0])
    for B in cr.PARITY_BATCHES:
        m = cr.parity_measure(pred, name, B)
        for k in cr.PARITY_KEYS:
            print('%s B=%d %s: sensitivity %.2e, error %.2e, allowed %.2e' % (name, B, k, m[k]['sensitivity'], m[k]['error'],
                                                                              m[k]['allowed']))
        assert m['none_converged'] and m['frames_are_the_end']
        for k in cr.PARITY_KEYS:
            assert m[k]['error'] <= m[k]['allowed'], (k, m[k])
        assert m['state_equal']


# ---- 3. the toy to convergence

@pytest.mark.parametrize('pressure', [0.0, cr.TOY_PRESSURE])
def test_toy_converges_like_the_restatement(pressure):
    model, starts, L_starts, d0, fmax = cr.toy()
    ref, dev = cr.toy_reference(pressure)
    pred = _toy_predictor()
    out = pred.relax_cell(**_toy_kw(pressure))
    print('p = %g: steps %s (restated %s)' % (pressure, out['n_steps'], ref['n_steps']))
    assert np.array_equal(out['n_steps'], ref['n_steps']) and np.array_equal(out['converged'], ref['converged'])
    assert out['converged'].all() and (out['fmax_end'] < fmax).all()
    for k in cr.EXACT_STATE:
        assert np.array_equal(out['state'][k], ref['state'][k]), k
    e_metric = np.abs(cr.metric(out['lattice_end']) - cr.metric(ref['lattice_end'])).max()
    e_pairs = np.abs(cr.pair_distances(out['R_end'], out['lattice_end']) - cr.pair_distances(ref['R_end'], ref['lattice_end'])).max()
    print('p = %g: metric error %.2e (sensitivity %.2e), pair distances %.2e (%.2e)' %
          (pressure, e_metric, dev['metric_end'], e_pairs, dev['pairs_end']))
    assert e_metric <= cr.BOUND_FACTOR * dev['metric_end'] and e_pairs <= cr.BOUND_FACTOR * dev['pairs_end']
    assert np.array_equal(out['E_hist'][-1], out['E_end']) and np.array_equal(out['vol_hist'][-1], out['vol_end'])
    assert out['E_hist'].shape == (ref['n_steps'].max() + 1, 7)
    # the stress of the end state balances the external pressure: W / Vol + p = 0 to the convergence threshold
    resid = out['stress_end'] + pressure * np.eye(3)[None]
    assert np.abs(resid * out['vol_end'][:, None, None]).max() / 6.0 < 4.0 * fmax
    if pressure == 0.0:
        assert np.abs(cr.pair_distances(out['R_end'], out['lattice_end']) - d0).max() <= \
            0.05 * np.abs(cr.pair_distances(starts, L_starts) - d0).max()


# ---- 4. end state against the predictor

def _dev_cells(ctx, R, lats, invs):
    B, n3 = R.shape
    lib, h = ctx._lib, ctx._h
    ptrs = [C.c_void_p() for _ in range(6)]
    sizes = [B * n3 * 8, B * 72, B * 72, B * 8, B * n3 * 8, B * 72]
    for p, s in zip(ptrs, sizes):
        ctx._check(lib.gdml_dev_alloc(h, s, C.byref(p)))
    try:
        for p, a in zip(ptrs[:3], (R, lats, invs)):
            a = np.ascontiguousarray(a, dtype=np.float64)
            ctx._check(lib.gdml_memcpy_h2d(h, p, a.ctypes.data_as(C.c_void_p), a.nbytes))
        ctx.predict_cells_dev(ptrs[0], B, ptrs[1], ptrs[2], ptrs[3], ptrs[4], ptrs[5])
        out = [np.empty(B), np.empty((B, n3)), np.empty((B, 3, 3))]
        for p, o in zip(ptrs[3:], out):
            ctx._check(lib.gdml_memcpy_d2h(h, o.ctypes.data_as(C.c_void_p), p, o.nbytes))
        return out
    finally:
        for p in ptrs:
            lib.gdml_dev_free(h, p)


def _end_is_the_predictors(pred, out):
    lats = out['lattice_end']
    invs = np.array([cr.inv3(L) for L in lats])
    E, F, W = _dev_cells(pred._ctx, out['R_end'], lats, invs)
    assert np.array_equal(out['E_end'], E * pred.std + pred.c) and np.array_equal(out['F_end'], F * pred.std)
    assert np.array_equal(out['stress_end'], W * pred.std / out['vol_end'][:, None, None])
    assert np.abs(out['vol_end'] - np.abs(np.linalg.det(lats))).max() <= 1e-13 * out['vol_end'].max()


def test_end_state_is_the_predictors_bits():
    """E_end, F_end and W_end are the bits of gdml_predict_virial_cells_dev(R_end, lat_end) at the same B: after a budget that
    ends before convergence, and after a run in which the geometries froze at different evaluations."""
    pred = _toy_predictor()
    for B in (1, 7):
        kw = _toy_kw(max_steps=12)
        kw.update(R0=kw['R0'][:B], lattices=kw['lattices'][:B])
        _end_is_the_predictors(pred, pred.relax_cell(**kw))
    out = pred.relax_cell(**_toy_kw())
    assert len(set(out['n_steps'].tolist())) > 1
    _end_is_the_predictors(pred, out)


# ---- 5. bit-identical

def test_deterministic_continuation_chunks_and_record_every():
    model, starts, L_starts, d0, fmax = cr.toy()
    pred = _toy_predictor()
    n = 20
    ref, _ = cr.toy_reference(cr.TOY_PRESSURE)
    assert ref['n_steps'].min() > 2 * n
    full = pred.relax_cell(**_toy_kw(max_steps=2 * n, record_every=1))
    assert _same(full, pred.relax_cell(**_toy_kw(max_steps=2 * n, record_every=1)))  # identical calls, identical bits
    a = pred.relax_cell(**_toy_kw(max_steps=n))
    b = pred.relax_cell(**_toy_kw(max_steps=n, state=a['state']))
    assert (b['state']['n_taken'] == 2 * n).all() and (b['n_steps'] == n).all() and (full['n_steps'] == 2 * n).all()
    for k in ('R_end', 'lattice_end', 'E_end', 'F_end', 'stress_end', 'vol_end', 'fmax_end'):
        assert np.array_equal(b[k], full[k]), k
    for k in STATE_KEYS:
        assert np.array_equal(b['state'][k], full['state'][k]), k
    for k in ('E_hist', 'vol_hist', 'fmax_hist'):  # evaluation 0 of the continuation repeats the last one of the first call
        assert np.array_equal(np.concatenate([a[k], b[k][1:]]), full[k]), k
    whole = pred.relax_cell(**_toy_kw(record_every=1))  # to convergence: geometries stop on the way
    frames = lambda o: np.array_equal(whole['R'], o['R']) and np.array_equal(whole['lattice'], o['lattice'])  # noqa: E731
    ctx = pred._ctx
    try:
        for steps in (1, 5):
            ctx.set_option('predict.relax_chunk_steps', steps)
            o = pred.relax_cell(**_toy_kw(record_every=1))
            assert _same(whole, o) and frames(o), steps
        ctx.set_option('predict.relax_chunk_steps', 32)
        ctx.set_option('predict.md_chunk_frames', 3)  # the frame bound cuts the chunks instead
        o = pred.relax_cell(**_toy_kw(record_every=1))
        assert _same(whole, o) and frames(o)
    finally:
        ctx.set_option('predict.relax_chunk_steps', 32)
        ctx.set_option('predict.md_chunk_frames', 0)
    n_made = whole['n_steps'].max() + 1
    assert whole['R'].shape == (n_made, 7, 18) and whole['lattice'].shape == (n_made, 7, 3, 3)
    assert np.array_equal(whole['R'][-1], whole['R_end']) and np.array_equal(whole['lattice'][-1], whole['lattice_end'])
    assert np.array_equal(whole['R'][0], starts) and np.array_equal(whole['lattice'][0], L_starts)
    for q in range(7):  # a frozen geometry repeats its end positions, lattice and volume
        t = whole['n_steps'][q]
        assert (whole['R'][t:, q] == whole['R_end'][q]).all() and (whole['lattice'][t:, q] == whole['lattice_end'][q]).all()
        assert (whole['vol_hist'][t:, q] == whole['vol_end'][q]).all()
    o0 = pred.relax_cell(**_toy_kw())
    assert 'R' not in o0 and 'lattice' not in o0 and _same(whole, o0)
    o3 = pred.relax_cell(**_toy_kw(record_every=3))
    assert _same(whole, o3) and np.array_equal(o3['R'], whole['R'][::3]) and np.array_equal(o3['lattice'], whole['lattice'][::3])


def test_geometry_alone_and_in_batch():
    """Bit for bit where the per-geometry-lattice predictor gives a geometry the same bits alone and in a batch of 7 (its row
    splits are sized by B), else the same steps and the end state to the allowance."""
    model, starts, L_starts, d0, fmax = cr.toy()
    ref, dev = cr.toy_reference(cr.TOY_PRESSURE)
    pred = _toy_predictor()
    batch = pred.relax_cell(**_toy_kw())
    invs = np.array([cr.inv3(L) for L in L_starts])
    E7, F7, W7 = pred._ctx.predict_cells(starts, L_starts, invs)
    for q in (0, 4):
        alone = pred.relax_cell(**_toy_kw(R0=starts[q], lattices=L_starts[q:q + 1]))
        E1, F1, W1 = pred._ctx.predict_cells(starts[q:q + 1], L_starts[q:q + 1], invs[q:q + 1])
        assert alone['n_steps'][0] == batch['n_steps'][q] and alone['converged'][0]
        if np.array_equal(F1[0], F7[q]) and np.array_equal(E1[0], E7[q]) and np.array_equal(W1[0], W7[q]):
            m = batch['n_steps'][q] + 1
            for k in ('R_end', 'lattice_end', 'F_end', 'stress_end', 'vol_end'):
                assert np.array_equal(alone[k][0], batch[k][q]), k
            assert np.array_equal(alone['E_hist'][:, 0], batch['E_hist'][:m, q])
            assert all(np.array_equal(alone['state'][k][0], batch['state'][k][q]) for k in STATE_KEYS)
        else:
            assert np.abs(alone['R_end'][0] - batch['R_end'][q]).max() <= cr.BOUND_FACTOR * dev['R_end']
            assert np.abs(alone['lattice_end'][0] - batch['lattice_end'][q]).max() <= cr.BOUND_FACTOR * dev['lattice_end']


def test_converged_start_stays_put_while_neighbours_run():
    model, starts, L_starts, d0, fmax = cr.toy()
    pred = _toy_predictor()
    first = pred.relax_cell(**_toy_kw())
    R0, L0 = np.array(starts), np.array(L_starts)
    R0[2], L0[2] = first['R_end'][2], first['lattice_end'][2]
    out = pred.relax_cell(**_toy_kw(R0=R0, lattices=L0))
    assert out['n_steps'][2] == 0 and out['converged'][2]
    assert np.array_equal(out['R_end'][2], R0[2]) and np.array_equal(out['lattice_end'][2], L0[2])
    assert not out['state']['V'][2].any() and out['state']['n_taken'][2] == 0 and out['state']['dt'][2] == cr.TOY_FIRE['dt_start']
    assert np.array_equal(out['state']['C'][2], 6.0 * np.eye(3))
    others = [0, 1, 3, 4, 5, 6]
    assert np.array_equal(out['n_steps'][others], first['n_steps'][others])
    assert (out['E_hist'][:, 2] == out['E_end'][2]).all() and (out['vol_hist'][:, 2] == out['vol_end'][2]).all()


# ---- 6. mask, edges and error paths

def test_slab_mask_relaxes_in_plane_only():
    pred = _toy_predictor()
    slab = np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 0.0]])
    out = pred.relax_cell(**_toy_kw(mask=slab, max_steps=30))
    Fd = out['state']['C'] / 6.0
    assert np.array_equal(Fd[:, 2, :], np.broadcast_to([0.0, 0.0, 1.0], (7, 3))) and np.array_equal(Fd[:, :2, 2], np.zeros((7, 2)))
    assert (np.abs(Fd[:, :2, :2] - np.eye(2)).max(axis=(1, 2)) > 1e-4).all()
    assert not out['state']['V'][:, 18:].reshape(7, 3, 3)[:, 2, :].any()


def test_budget_edges():
    model, starts, L_starts, d0, fmax = cr.toy()
    pred = _toy_predictor()
    o = pred.relax_cell(**_toy_kw(max_steps=0, record_every=1))  # one evaluation, no step
    assert (o['n_steps'] == 0).all() and not o['converged'].any()
    assert np.array_equal(o['R_end'], starts) and np.array_equal(o['lattice_end'], L_starts)
    assert o['E_hist'].shape == (1, 7) and o['R'].shape == (1, 7, 18) and o['lattice'].shape == (1, 7, 3, 3)
    assert (o['state']['n_taken'] == 0).all() and np.array_equal(o['state']['S'], starts)
    _end_is_the_predictors(pred, o)
    assert np.abs(o['vol_end'] - np.abs(np.linalg.det(L_starts))).max() <= 1e-13 * o['vol_end'].max()
    # f_atom of the start: the largest row norm of the restated generalised force
    G = cr.gen_force(lambda R, L: (o['E_end'], o['F_end'], o['stress_end'] * o['vol_end'][:, None, None]),
                     cr.join(starts, np.broadcast_to(6.0 * np.eye(3), (7, 3, 3))), L_starts, 6.0, cr.TOY_PRESSURE)[1]
    g = np.sqrt((G.reshape(7, 9, 3) ** 2).sum(-1)).max(axis=1)
    assert np.abs(o['fmax_end'] - g).max() <= 1e-12 * g.max()
    o = pred.relax_cell(**_toy_kw(max_steps=10))  # a budget that ends before convergence
    assert (o['n_steps'] == 10).all() and not o['converged'].any() and (o['state']['n_taken'] == 10).all()
    assert o['E_hist'].shape == o['vol_hist'].shape == (11, 7)
    o2 = pred.relax_cell(**_toy_kw(max_steps=10, f_unit=2.0, pressure=2.0 * cr.TOY_PRESSURE))  # the unit factor scales G
    assert not np.array_equal(o2['R_end'], o['R_end']) and np.abs(o2['fmax_hist'][0] - 2.0 * o['fmax_hist'][0]).max() <= 1e-12
    one = pred.relax_cell(starts, fmax, lattice=L_starts[0], max_steps=3)  # one lattice, broadcast to all starts
    assert np.array_equal(one['state']['L0'], np.broadcast_to(L_starts[0], (7, 3, 3)))
    dflt = pred.relax_cell(starts, fmax, max_steps=3)  # the model's lattice by default
    assert np.array_equal(dflt['state']['L0'], np.broadcast_to(model['lattice'], (7, 3, 3)))


def test_error_paths_launch_nothing_and_leave_the_predictor_working():
    model, starts, L_starts, d0, fmax = cr.toy()
    pred = _toy_predictor()
    R0, L0 = np.array(starts[:3]), np.array(L_starts[:3])
    invs = np.array([cr.inv3(L) for L in L0])
    ok_bits = pred._ctx.predict_cells(R0, L0, invs)
    ok = dict(R0=R0, fmax=fmax, lattices=L0, max_steps=5)

    def bad(exc=ValueError, **kw):
        with pytest.raises(exc):
            pred.relax_cell(**dict(ok, **kw))
        for x, y in zip(ok_bits, pred._ctx.predict_cells(R0, L0, invs)):
            assert np.array_equal(x, y)

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
    bad(cell_factor=0.0)
    bad(cell_factor=-1.0)
    bad(cell_factor=float('inf'))
    bad(pressure=float('nan'))
    bad(mask=np.ones((2, 2)))
    bad(mask=0.5 * np.ones((3, 3)))
    bad(mask=np.array([[1.0, 0.0, 1.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0]]))
    bad(lattices=L0[:2])
    bad(lattices=L0, lattice=L0[0])
    bad(lattices=np.zeros((3, 3, 3)))
    for lattice in (np.eye(2), np.zeros((3, 3))):
        bad(lattices=None, lattice=lattice)
    st = pred.relax_cell(**ok)['state']
    bad(state=dict(st, dt=np.array([0.1, -0.1, 0.1])))
    bad(state=dict(st, C=np.zeros((3, 3, 3))))
    bad(state={k: v for k, v in st.items() if k != 'L0'})
    nolat = GDMLPredict({k: v for k, v in model.items() if k != 'lattice'})
    with pytest.raises(ValueError, match='needs a lattice'):
        nolat.relax_cell(R0, fmax, max_steps=2)
    R_nan = R0.copy()
    R_nan[1, 4] = np.nan
    with pytest.raises(FloatingPointError, match='geometry 1 .* evaluation 0'):
        pred.relax_cell(**dict(ok, R0=R_nan))
    for x, y in zip(ok_bits, pred._ctx.predict_cells(R0, L0, invs)):
        assert np.array_equal(x, y)
    out = pred.relax_cell(**ok)  # and the optimiser itself still works
    assert (out['n_steps'] == 5).all() and np.isfinite(out['E_end']).all()


def test_wrong_atom_count_and_missing_model():
    model, starts, L_starts, d0, fmax = cr.toy()
    ctx = _toy_predictor()._ctx
    st = cr.fresh_state(starts[:1, :15], L_starts[:1], 5.0)
    saved, ctx.model_n_atoms = ctx.model_n_atoms, 5
    try:
        with pytest.raises(ValueError, match='atoms'):
            ctx.cell_relax_run(st['S'], st['C'], st['L0'], fmax, 5, st, 1.0, cell_factor=5.0)
    finally:
        ctx.model_n_atoms = saved
    empty = _lib.Context(0)
    try:
        empty.model_n_atoms = 6
        st = cr.fresh_state(starts, L_starts, 6.0)
        with pytest.raises(_lib.GDMLHipError):  # no model resident
            empty.cell_relax_run(st['S'], st['C'], st['L0'], fmax, 5, st, 1.0, cell_factor=6.0)
    finally:
        empty.close()


# ---- budgets on the edges of a chunk

@functools.lru_cache(maxsize=None)
def _whole_toy_run():
    return _toy_predictor().relax_cell(**_toy_kw(record_every=1))


def test_budgets_on_chunk_edges_are_the_whole_runs_first_rows():
    """Chunks of 4 evaluations; budgets of 1, 4, 5, 8 and 9 evaluations (one evaluation, the last row of a chunk, the first
    row of the next) with no frames, every evaluation a frame and every third: every history and both frame arrays are, bit
    for bit, the first rows of the run to convergence at default options."""
    whole = _whole_toy_run()
    pred = _toy_predictor()
    try:
        pred._ctx.set_option('predict.relax_chunk_steps', 4)
        for max_steps, every in itertools.product((0, 3, 4, 7, 8), (0, 1, 3)):
            o = pred.relax_cell(**_toy_kw(max_steps=max_steps, record_every=every))
            n = min(max_steps + 1, whole['E_hist'].shape[0])
            for k in ('E_hist', 'vol_hist', 'fmax_hist'):
                assert o[k].shape[0] == n and np.array_equal(o[k], whole[k][:n]), (k, max_steps, every)
            for k in ('R', 'lattice'):
                assert (k in o) == (every > 0)
                if every:
                    assert np.array_equal(o[k], whole[k][:n][::every]), (k, max_steps, every)
    finally:
        pred._ctx.set_option('predict.relax_chunk_steps', 32)

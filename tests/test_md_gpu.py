"""Molecular dynamics on the GPU (gdml_md_run, csrc/md.hip; GDMLPredict.run_md): against the NumPy restatement
(tests/_md_ref.py), recorded frames against predict(), determinism, restart, record_every and chunking bit for bit, replicas,
the noise stream, conservation laws and error paths.  Masses 1 throughout."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _md_ref as mr  # noqa: E402
from sgdml_amd import _lib  # noqa: E402
from sgdml_amd.predict import GDMLPredict  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = ['n6_p1', 'n5_p4', 'n5_p2_ecstr', 'n10_p2_pbc', 'cfg1_n21_m100']  # D <= 256: the shapes of the single-launch predictor
LARGE = ['cfg3_n42_p27_m60', 'n100_m3']  # D > 256
STEPS = {'cfg3_n42_p27_m60': 5}  # (its restated forces take a third of a second per call)
LANGEVIN = dict(thermostat='langevin', gamma=0.5, kT=0.05, seed=77)
THERMO = {'nve': {}, 'langevin': LANGEVIN}
FIELDS = ('R', 'V', 'E_pot', 'E_kin')
ALL = ('R', 'V', 'F', 'E')


def _start(name, B=7):
    model, R7 = mr.case(name)
    R0 = np.ascontiguousarray(R7[np.arange(B) % len(R7)])
    return model, R0, mr.start_velocities(B, R0.shape[1], mr.V_SCALE[name]), np.ones(R0.shape[1] // 3)


@functools.lru_cache(maxsize=None)
def _reference(name, thermo):
    """Restated trajectory of seven replicas and its sensitivity to the predictor's agreed error: the largest deviation, per
    field, of a second restated run whose forces carry independent noise of 1e-10 max|F| (the project's prediction tolerance,
    tests/test_stress_gpu.py).  Computed once per session, only read."""
    model, R0, V0, masses = _start(name)
    n = STEPS.get(name, 30)
    clean = mr.run(mr.force_fn(model), R0, V0, masses, mr.DT[name], n, **THERMO[thermo])
    noisy = mr.run(mr.force_fn(model, rel_noise=1e-10, seed=1), R0, V0, masses, mr.DT[name], n, **THERMO[thermo])
    dev = {k: np.abs(clean[k] - noisy[k]).max() for k in FIELDS}
    for a in clean.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return clean, dev, n


def _predictor(model, route):
    """route 'step': the single-launch step where the shape is served (the default); 'general': three pieces per step."""
    pred = GDMLPredict(model)
    if route == 'general':
        pred._ctx.set_option('predict.md_fused', 0)
    return pred


# (fixture, route): every small shape on both routes, the large ones on the only route they have
ROUTED = [(n, r) for n in SMALL for r in ('step', 'general')] + [(n, 'general') for n in LARGE]


def _same(a, b, keys=None):
    keys = keys or [k for k in a if isinstance(a[k], np.ndarray)]
    return all(np.array_equal(a[k], b[k]) for k in keys) and a['step_end'] == b['step_end']


# ---- 1. against the restatement

@pytest.mark.parametrize('thermo', ['nve', 'langevin'])
@pytest.mark.parametrize('name,route', ROUTED)
def test_trajectory_matches_restatement(name, route, thermo):
    """R, V, E_pot, E_kin of every frame, B = 1 and B = 7.  Tolerance: ten times the restatement's own sensitivity to force
    errors of 1e-10 max|F| (the margin because a systematic error adds up over the steps where the noise does not)."""
    clean, dev, n = _reference(name, thermo)
    model, R0, V0, masses = _start(name)
    pred = _predictor(model, route)
    for B in (1, 7):  # replica 0 alone draws the noise of replica 0 in the batch
        out = pred.run_md(R0[:B], V0[:B], masses, mr.DT[name], n, record=ALL, **THERMO[thermo])
        assert out['step_end'] == n
        for k in FIELDS:
            err = np.abs(out[k] - clean[k][:, :B]).max()
            print('%s %s %s B=%d %s: sensitivity %.2e, error %.2e' % (name, route, thermo, B, k, dev[k], err))
        for k in FIELDS:
            assert np.abs(out[k] - clean[k][:, :B]).max() <= 10.0 * dev[k], (name, thermo, B, k)
        assert np.array_equal(out['R_end'], out['R'][-1]) and np.array_equal(out['V_end'], out['V'][-1])


# ---- 2. frames against the predictor

def _frames_vs_predict(pred, out, exact):
    for k in range(len(out['R'])):
        E, F = pred.predict(out['R'][k])
        if exact:
            assert np.array_equal(out['E_pot'][k], E) and np.array_equal(out['F'][k], F), k
        else:
            eF = np.abs(out['F'][k] - F).max() / np.abs(F).max()
            eE = np.abs(out['E_pot'][k] - E).max() / np.abs(E).max()
            assert eF <= 1e-10 and eE <= 1e-10, (k, eF, eE)


@pytest.mark.parametrize('name', LARGE)
def test_frames_are_the_predictors_bits(name):
    """D > 256: predict() of host geometries runs the kernels gdml_predict_dev runs, so E_pot and F of a frame are the bits of
    predict(R_frame)."""
    model, R0, V0, masses = _start(name)
    pred = GDMLPredict(model)
    for B in (1, 7):
        for th in THERMO.values():
            out = pred.run_md(R0[:B], V0[:B], masses, mr.DT[name], 6, record_every=2, record=ALL, **th)
            assert out['R'].shape == (3, B, R0.shape[1])
            _frames_vs_predict(pred, out, exact=True)


def test_frames_are_the_predictors_bits_mfma_route():
    model, R0, V0, masses = _start('n9_p1', B=256)  # 256 tiled starts: the MFMA route
    pred = GDMLPredict(model)
    out = pred.run_md(R0, V0, masses, mr.DT['n9_p1'], 6, record_every=3, record=ALL, **LANGEVIN)
    _frames_vs_predict(pred, out, exact=True)
    assert not np.array_equal(out['R'][-1][0], out['R'][-1][7])  # same start, other noise
    again = pred.run_md(R0, V0, masses, mr.DT['n9_p1'], 6, record_every=3, record=ALL, **LANGEVIN)
    assert _same(out, again)


@pytest.mark.parametrize('route', ['step', 'general'])
@pytest.mark.parametrize('name', SMALL)
def test_frames_match_the_predictor_small_shapes(name, route):
    """D <= 256, B <= 8.  Single-launch step: it restates the single-launch predictor's row loop, row split and reduction
    order, so where predict() takes its single launch too (at most 384 coordinates) the frames are its bits; beyond that
    (seven replicas of 21 atoms), and on the general route, whose device path uses other kernels than predict() of a small
    host batch, 1e-10 of the maximum."""
    model, R0, V0, masses = _start(name)
    pred = _predictor(model, route)
    for B in (1, 7):
        for th in THERMO.values():
            out = pred.run_md(R0[:B], V0[:B], masses, mr.DT[name], 6, record_every=2, record=ALL, **th)
            _frames_vs_predict(pred, out, exact=(route == 'step' and B * R0.shape[1] <= 384))


def test_frames_are_the_predictors_bits_two_entries_per_lane():
    """D = 66 (N = 12, synthetic model): the instance of the single-launch step with two descriptor entries per lane, which no
    fixture reaches.  B = 1 and 7 (252 coordinates: predict() takes its single launch too), six steps, every frame: E_pot and
    F are the bits of predict(R_frame)."""
    model, R7 = mr.synth_n12()
    V0 = mr.start_velocities(7, R7.shape[1], mr.SYNTH_V_SCALE)
    pred = GDMLPredict(model)
    for B in (1, 7):
        for th in THERMO.values():
            out = pred.run_md(R7[:B], V0[:B], np.ones(12), mr.SYNTH_DT, 6, record=ALL, **th)
            assert out['R'].shape == (6, B, 36)
            _frames_vs_predict(pred, out, exact=True)


# ---- 3. determinism and restart

@pytest.mark.parametrize('thermo', ['nve', 'langevin'])
@pytest.mark.parametrize('name,route', [('n5_p4', 'step'), ('n10_p2_pbc', 'step'), ('cfg1_n21_m100', 'step'),
                                        ('n5_p4', 'general'), ('n100_m3', 'general')])
def test_deterministic_restart_record_every_and_chunks(name, route, thermo):
    model, R0, V0, masses = _start(name, B=3)
    pred = _predictor(model, route)
    th, dt, n = THERMO[thermo], mr.DT[name], 6
    full = pred.run_md(R0, V0, masses, dt, 2 * n, record=ALL, **th)
    assert _same(full, pred.run_md(R0, V0, masses, dt, 2 * n, record=ALL, **th))  # identical calls, identical bits
    a = pred.run_md(R0, V0, masses, dt, n, record=ALL, **th)
    b = pred.run_md(a['R_end'], a['V_end'], masses, dt, n, record=ALL, step0=a['step_end'], **th)
    assert b['step_end'] == 2 * n
    for k in ('R', 'V', 'F', 'E_pot', 'E_kin'):
        assert np.array_equal(np.concatenate([a[k], b[k]]), full[k]), k
    assert np.array_equal(b['R_end'], full['R_end']) and np.array_equal(b['V_end'], full['V_end'])
    for every in (3, 2 * n):
        o = pred.run_md(R0, V0, masses, dt, 2 * n, record_every=every, record=ALL, **th)
        assert np.array_equal(o['R_end'], full['R_end']) and np.array_equal(o['V_end'], full['V_end'])
        for k in ('R', 'V', 'F', 'E_pot', 'E_kin'):
            assert np.array_equal(o[k], full[k][every - 1::every]), (every, k)
    o = pred.run_md(R0, V0, masses, dt, 2 * n + 1, record_every=5, record=('R',), **th)  # steps behind the last frame
    assert o['R'].shape[0] == 2 and 'V' not in o and 'F' not in o and np.array_equal(o['R'], full['R'][4::5])
    for frames in (1, 5):  # a chunk bound forced small: 12 or 3 synchronisations instead of one
        pred._ctx.set_option('predict.md_chunk_frames', frames)
        assert _same(full, pred.run_md(R0, V0, masses, dt, 2 * n, record=ALL, **th))
    pred._ctx.set_option('predict.md_chunk_frames', 0)
    short = pred.run_md(R0, V0, masses, dt, 3, record_every=5, record=ALL, **th)  # fewer steps than a frame takes
    assert short['R'].shape[0] == 0 and np.array_equal(short['R_end'], full['R'][2]) and short['step_end'] == 3
    none = pred.run_md(R0, V0, masses, dt, 0, record=ALL, **th)  # no step: the start comes back
    assert np.array_equal(none['R_end'], R0) and np.array_equal(none['V_end'], V0) and none['R'].shape[0] == 0


# ---- 4. replicas

@pytest.mark.parametrize('name', LARGE + ['n5_p4', 'cfg1_n21_m100'])
def test_replica_alone_and_in_batch(name):
    """D > 256: the general route, bit for bit where predict() itself gives a geometry the same bits alone and in a batch.
    The small shapes take the single-launch step, whose row shares belong to one replica, like the single-launch predictor's."""
    model, R0, V0, masses = _start(name)
    pred = GDMLPredict(model)
    dt, n = mr.DT[name], STEPS.get(name, 30)
    batch = pred.run_md(R0, V0, masses, dt, n, record=ALL)
    E7, F7 = pred.predict(R0)
    for q in (0, 4):
        alone = pred.run_md(R0[q], V0[q], masses, dt, n, record=ALL)
        E1, F1 = pred.predict(R0[q])
        if np.array_equal(F1[0], F7[q]) and np.array_equal(E1[0], E7[q]):  # predict() has the property for this shape
            for k in ('R', 'V', 'F', 'E_pot', 'E_kin'):
                assert np.array_equal(alone[k][:, 0], batch[k][:, q]), (q, k)
        else:  # its row splits are sized by B: regrouped partial sums, the tolerance of the restatement test
            _, dev, _ = _reference(name, 'nve')
            for k in FIELDS:
                err = np.abs(alone[k][:, 0] - batch[k][:, q]).max()
                print('%s replica %d alone vs in batch, %s: %.2e (sensitivity %.2e)' % (name, q, k, err, dev[k]))
                assert err <= 10.0 * dev[k], (q, k)


def test_replicas_draw_their_own_noise():
    """Replicas with one start differ under the thermostat, and replica b consumes gdml_md_noise(...)[b]: with c1 = exp(-gamma
    dt) = 0 exactly and V0 = 0 one step gives R1 = R0 + dt/2 (dt/2 a0) + dt/2 sqrt(kT) xi."""
    model, R7 = mr.case('n100_m3')
    B, n3 = 4, R7.shape[1]
    R0 = np.ascontiguousarray(np.repeat(R7[:1], B, axis=0))
    V0, masses = np.zeros((B, n3)), np.ones(n3 // 3)
    pred = GDMLPredict(model)
    dt, kT, seed, step0 = 0.002, 0.25, 2**63 + 11, 2**32 + 5
    out = pred.run_md(R0, V0, masses, dt, 1, thermostat='langevin', gamma=1e6, kT=kT, seed=seed, step0=step0, record=('R',))
    assert out['step_end'] == step0 + 1
    for b in range(1, B):
        assert not np.array_equal(out['R'][0, b], out['R'][0, 0])
    _, F0 = pred.predict(R0)
    xi = (out['R'][0] - R0 - 0.25 * dt * dt * F0) / (0.5 * dt * np.sqrt(kT))
    want = pred._ctx.md_noise(seed, step0, B, n3)
    err = np.abs(xi - want).max()
    print('noise recovered from one step vs gdml_md_noise: %.2e' % err)
    # recovering xi divides a difference of positions (|R| ~ 10, 1e-15 rounding) by dt / 2 sqrt(kT) = 5e-4: 1e-11 or so
    assert err <= 1e-9
    assert np.array_equal(pred._ctx.md_noise(seed, step0, 2, n3), want[:2])  # not a function of B


# ---- 5. the noise stream

@pytest.mark.parametrize('n3', [15, 63, 300])
def test_noise_matches_restatement(n3):
    """Absolute error 1e-14: HIP documents at most 2 ulp for double log / sin / cos, on values |xi| < 7; a wrong integer
    stream misses by O(1).  n3 not a multiple of 4: the tail block."""
    ctx = _lib.Context(0)
    try:
        for seed in (0, 2**63 + 11):
            for step in (0, 1, 2**32 + 5):
                got = ctx.md_noise(seed, step, 3, n3)
                err = np.abs(got - mr.normals(seed, step, 3, n3)).max()
                print('seed %d step %d n3 %d: %.2e' % (seed, step, n3, err))
                assert err <= 1e-14
    finally:
        ctx.close()


# ---- 6. physics

@pytest.mark.parametrize('name,route', [('n6_p1', 'step'), ('n6_p1', 'general'), ('n100_m3', 'general')])
def test_energy_drift_is_second_order(name, route):
    """The dt, dt / 2 drift ratio of tests/test_md_cpu.py on the GPU, on both routes."""
    model, R0, V0, masses = _start(name, B=1)
    pred = _predictor(model, route)
    dt, n = mr.DT[name], 40
    e0 = pred.predict(R0)[0] + 0.5 * (V0 * V0).sum(axis=1)
    d = []
    for h, steps in ((dt, n), (dt / 2, 2 * n)):
        out = pred.run_md(R0, V0, masses, h, steps)
        d.append(np.abs(out['E_pot'] + out['E_kin'] - e0[None]).max())
    print('%s %s: drift %.3e at dt, %.3e at dt/2, ratio %.3f' % (name, route, d[0], d[1], d[0] / d[1]))
    assert 3.0 <= d[0] / d[1] <= 5.0


@pytest.mark.parametrize('name', ['n5_p2_ecstr', 'n100_m3'])
def test_langevin_without_friction_is_verlet(name):
    model, R0, V0, masses = _start(name)
    _, dev, n = _reference(name, 'nve')
    pred = GDMLPredict(model)
    nve = pred.run_md(R0, V0, masses, mr.DT[name], n, record=ALL)
    lan = pred.run_md(R0, V0, masses, mr.DT[name], n, record=ALL, thermostat='langevin', gamma=0.0, kT=0.05, seed=3)
    for k in FIELDS:
        err = np.abs(nve[k] - lan[k]).max()
        print('%s gamma = 0 vs NVE, %s: %.2e (sensitivity %.2e)' % (name, k, err, dev[k]))
        assert err <= 10.0 * dev[k], k


def test_lattice_shift_leaves_forces_and_energies():
    """Atoms moved by whole lattice vectors: the minimum image undoes the shift, positions are never wrapped.  To rounding:
    the shifted coordinates carry an absolute rounding error of eps |lattice vector|, which the pair distances (>= 0.47)
    see as a relative 1e-15 or so per step -- far inside the project's prediction tolerance of 1e-10, which is asserted."""
    model, R0, V0, masses = _start('n10_p2_pbc', B=2)
    lat = np.asarray(model['lattice'], dtype=np.float64)  # cell vectors in the columns
    shift = np.zeros((10, 3))
    shift[2] = lat[:, 0]
    shift[5] = -lat[:, 1] + lat[:, 2]
    shift[7] = 2 * lat[:, 2]
    pred = GDMLPredict(model)
    dt = mr.DT['n10_p2_pbc']
    a = pred.run_md(R0, V0, masses, dt, 20, record=ALL)
    b = pred.run_md(R0 + shift.ravel()[None], V0, masses, dt, 20, record=ALL)
    assert np.abs(b['R'] - a['R'] - shift.ravel()[None, None]).max() <= 1e-10  # not wrapped
    eF = np.abs(a['F'] - b['F']).max() / np.abs(a['F']).max()
    eE = np.abs(a['E_pot'] - b['E_pot']).max() / np.abs(a['E_pot']).max()
    print('lattice shift: forces %.2e, energies %.2e' % (eF, eE))
    assert eF <= 1e-10 and eE <= 1e-10
    c = pred.run_md(R0, V0, masses, dt, 20, record=ALL, lattice=lat)  # the model's own cell per call: the same bits
    assert _same(a, c)
    d = pred.run_md(R0, V0, masses, dt, 20, record=ALL, lattice=0.8 * lat)  # another cell: the argument is not ignored
    assert not np.array_equal(d['F'], a['F'])


@pytest.mark.parametrize('name', ['n6_p1', 'cfg3_n42_p27_m60'])
def test_total_momentum_is_conserved(name):
    """No lattice, NVE, masses 1: the momentum changes by dt times the force sums, which vanish to rounding.  A force is a sum
    of N - 1 pair terms, so |sum_i F_i| <= N eps sum_i |F_i| <= N^2 eps max|F| per step; the velocity updates add eps max|V|
    per atom and step.  Bound: 4 n N eps (dt N max|F| + max|V|)."""
    model, R0, V0, masses = _start(name)
    pred = GDMLPredict(model)
    n, dt, N = 20, mr.DT[name], len(masses)
    out = pred.run_md(R0, V0, masses, dt, n, record=ALL)
    P0 = V0.reshape(7, N, 3).sum(axis=1)
    P = out['V'].reshape(n, 7, N, 3).sum(axis=2)
    bound = 4 * n * N * np.finfo(float).eps * (dt * N * np.abs(out['F']).max() + np.abs(out['V']).max())
    print('%s: momentum change %.2e, bound %.2e' % (name, np.abs(P - P0[None]).max(), bound))
    assert np.abs(P - P0[None]).max() <= bound


def test_the_two_routes_agree_and_share_the_kinetic_energy_tree():
    """One start on both routes: the trajectories differ by the rounding of two force kernels (inside the tolerance of the
    restatement test), and E_kin is the same function of the recorded V on both (one tree)."""
    name = 'cfg1_n21_m100'
    model, R0, V0, masses = _start(name)
    _, dev, n = _reference(name, 'langevin')
    a = _predictor(model, 'step').run_md(R0, V0, masses, mr.DT[name], n, record=ALL, **LANGEVIN)
    b = _predictor(model, 'general').run_md(R0, V0, masses, mr.DT[name], n, record=ALL, **LANGEVIN)
    for k in FIELDS:
        err = np.abs(a[k] - b[k]).max()
        print('step vs general route, %s: %.2e (sensitivity %.2e)' % (k, err, dev[k]))
        assert err <= 10.0 * dev[k], k
    eps = np.finfo(float).eps
    for o in (a, b):  # 63 terms: per-thread products, then a tree of depth 8 -- a few eps of the sum
        assert np.abs(o['E_kin'] - 0.5 * (o['V'] * o['V']).sum(axis=2)).max() <= 16 * eps * o['E_kin'].max()
    # more than eight replicas: the general route, whatever the option says
    model9, R9, V9, m9 = _start('n6_p1', B=9)
    p1, p0 = _predictor(model9, 'step'), _predictor(model9, 'general')
    assert _same(p1.run_md(R9, V9, m9, 0.02, 5, record=ALL), p0.run_md(R9, V9, m9, 0.02, 5, record=ALL))


# ---- 7. error paths

def test_error_paths_launch_nothing_and_leave_the_predictor_working():
    model, R0, V0, masses = _start('n6_p1', B=2)
    pred = GDMLPredict(model)
    E_ok, F_ok = pred.predict(R0)
    ok = dict(R0=R0, V0=V0, masses=masses, dt=0.02, n_steps=4)

    def bad(exc=ValueError, **kw):
        with pytest.raises(exc):
            pred.run_md(**dict(ok, **kw))
        E, F = pred.predict(R0)
        assert np.array_equal(E, E_ok) and np.array_equal(F, F_ok)

    bad(n_steps=-1)
    bad(record_every=0)
    bad(masses=np.array([1.0, 1.0, 0.0, 1.0, 1.0, 1.0]))
    bad(masses=np.array([1.0, 1.0, -1.0, 1.0, 1.0, 1.0]))
    bad(dt=0.0)
    bad(dt=-0.02)
    bad(dt=float('nan'))
    bad(gamma=-0.1, thermostat='langevin')
    bad(kT=-0.1, thermostat='langevin')
    bad(thermostat='nose-hoover')
    bad(thermostat=1)
    bad(step0=-1)
    R_nan = R0.copy()
    R_nan[1, 4] = np.nan
    bad(R0=R_nan)
    V_inf = V0.copy()
    V_inf[0, 0] = np.inf
    bad(V0=V_inf)
    bad(R0=R0[:, :15])  # wrong shapes
    bad(V0=V0[:1])
    bad(masses=np.ones(5))
    bad(record=('R', 'W'))
    bad(record='Q')
    for lattice in (np.eye(2), np.zeros((3, 3))):
        bad(lattice=lattice)
    # the C boundary: exactly one of lattice / inverse, a thermostat other than 0 or 1, the wrong N
    ctx = pred._ctx
    with pytest.raises(ValueError):
        ctx.md_run(R0, V0, masses, 0.02, 4, lat_and_inv=(np.eye(3), None))
    with pytest.raises(ValueError):
        ctx.md_run(R0, V0, masses, 0.02, 4, thermostat=2)
    prm = _lib.MDParams(1, 5, 0.02, _lib._ptr(masses), 1.0, None, None, 0, 0.0, 0.0, 0, 0)
    Rc, Vc = R0[:1, :15].copy(), V0[:1, :15].copy()
    assert ctx._lib.gdml_md_run(ctx._h, C.byref(prm), _lib._ptr(Rc), _lib._ptr(Vc), 4, 1, None, None, None, None, None, None) == -1
    assert 'atoms' in ctx._lib.gdml_last_error(ctx._h).decode()
    empty = _lib.Context(0)
    try:
        empty.model_n_atoms = 6
        with pytest.raises(_lib.GDMLHipError):  # no model resident
            empty.md_run(R0, V0, masses, 0.02, 4)
    finally:
        empty.close()
    out = pred.run_md(**ok)  # and the integrator itself still works
    assert out['R'].shape == (4, 2, 18) and np.isfinite(out['E_pot']).all()

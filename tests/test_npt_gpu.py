"""Constant-pressure dynamics on the GPU (gdml_npt_run, csrc/npt.hip; GDMLPredict.run_npt): with an infinitely heavy piston it
is run_md()'s general route bit for bit; step by step against the NumPy restatement (tests/_npt_ref.py); frames against the
per-geometry-lattice predictor; determinism, continuation, record_every and chunking bit for bit; the ensemble identities of
the Langevin piston and the second order of NPH on the periodic toy; edges and error paths."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _cellrelax_ref as cr  # noqa: E402
import _md_ref as mr  # noqa: E402
import _npt_ref as nr  # noqa: E402
from sgdml_amd import _lib  # noqa: E402
from sgdml_amd.predict import GDMLPredict  # noqa: E402

pytestmark = pytest.mark.gpu

LANGEVIN = dict(thermostat='langevin', gamma=0.5, kT=0.05, seed=77)
MODES = {'nph': {}, 'npt': dict(thermostat='langevin', gamma=0.3, gamma_baro=0.4, kT=0.002, seed=5)}
FRAMES = ('R', 'V', 'F', 'lattice', 'E_pot', 'E_kin', 'vol', 'pressure', 'p_eps', 'enthalpy')
ENDS = ('R_end', 'V_end', 'lattice_end', 'vol_end')
ALL = ('R', 'V', 'F', 'lattice', 'E')


@functools.lru_cache(maxsize=None)
def _toy_predictor():
    return GDMLPredict(cr.toy()[0])


def _toy_kw(mode='nph', n_steps=12, **kw):
    model, starts, L_starts, d0, fmax = cr.toy()
    base = dict(R0=starts, V0=mr.start_velocities(7, 18, 0.05), masses=np.linspace(1.0, 2.0, 6), dt=0.05, n_steps=n_steps,
                pressure=cr.TOY_PRESSURE, piston_mass=20.0, lattices=L_starts, record=ALL, **MODES[mode])
    return dict(base, **kw)


def _same(a, b, keys=FRAMES + ENDS):
    return (all(np.array_equal(a[k], b[k]) for k in keys) and all(np.array_equal(a['state'][k], b['state'][k]) for k in a['state'])
            and a['step_end'] == b['step_end'])


# ---- 1. the anchor: an infinitely heavy piston is run_md()'s general route, bit for bit

def _anchor(pred, R0, V0, masses, lattice, dt, n, thermo):
    ctx = pred._ctx
    ctx.set_option('predict.md_fused', 0)
    try:
        ref = pred.run_md(R0, V0, masses, dt, n, lattice=lattice, record=('R', 'V', 'F', 'E'), step0=3, **thermo)
    finally:
        ctx.set_option('predict.md_fused', 1)
    out = pred.run_npt(R0, V0, masses, dt, n, 0.37, np.inf, lattice=lattice, record=ALL, step0=3, gamma_baro=0.4, **thermo)
    for k in ('R', 'V', 'F', 'E_pot', 'E_kin', 'R_end', 'V_end'):
        assert np.array_equal(out[k], ref[k]), k
    B = len(R0)
    assert out['step_end'] == ref['step_end'] == n + 3
    assert np.array_equal(out['lattice'], np.broadcast_to(np.asarray(lattice, dtype=np.float64), (n, B, 3, 3)))
    assert np.array_equal(out['lattice_end'], out['lattice'][-1]) and not out['state']['eps'].any()
    assert (out['vol'] == out['vol'][0, 0]).all() and (out['vol_end'] == out['vol'][0, 0]).all()
    assert np.isfinite(out['p_eps']).all() and np.abs(out['p_eps']).max() > 0.0  # the piston is kicked and goes nowhere


@pytest.mark.parametrize('thermo', [{}, LANGEVIN], ids=['nve', 'langevin'])
def test_infinite_piston_mass_is_run_md_bit_for_bit_on_the_toy(thermo):
    model, starts, L_starts, d0, fmax = cr.toy()
    V0 = mr.start_velocities(7, 18, 0.05)
    masses = np.linspace(1.0, 2.0, 6)
    for B in (7, 1):
        _anchor(_toy_predictor(), np.array(starts[:B]), V0[:B], masses, L_starts[2], 0.05, 12, thermo)


@pytest.mark.parametrize('thermo', [{}, LANGEVIN], ids=['nve', 'langevin'])
def test_infinite_piston_mass_is_run_md_bit_for_bit_on_the_fixture(thermo):
    name = 'n10_p2_pbc'
    model, R7 = mr.case(name)
    pred = GDMLPredict(model)
    R0 = np.ascontiguousarray(R7[np.arange(7) % len(R7)])
    V0 = mr.start_velocities(7, R0.shape[1], mr.V_SCALE[name])
    masses = 1.0 + 0.5 * (np.arange(10) % 3)
    for B in (1, 7):
        _anchor(pred, R0[:B], V0[:B], masses, model['lattice'], mr.DT[name], 12, thermo)


# ---- 2. against the restatement, step by step

@pytest.mark.parametrize('mode', ['nph', 'npt'])
@pytest.mark.parametrize('name', nr.PARITY_FIXTURES)
def test_steps_match_restatement(name, mode):
    """30 steps at pressure 0.01 from distinct eps0 of order 1e-2 and nonzero p_eps0, masses 1 + 0.5 (i mod 3); B = 1 and 7.  In
    the restatement every replica's volume changes by 0.1 % to 2 % over the run (asserted: the cell moves).  R, V and lattice
    of every frame, E_kin, p_eps and the end eps within ten times the restatement's own sensitivity to noise of 1e-10 on E, F
    and W; E_pot, vol, pressure and enthalpy within that plus the predictor's agreed 1e-10 of the largest value.  The piston's
    noise index 3N opens a new Philox block for n4_p6_pbc (12) and sits inside one for n10_p2_pbc (30).
    tools/npt_parity.py records the same measurement in profiles/npt_parity.json."""
    model, kw, ref, dev = nr.parity_reference(name, mode)
    dvol = nr.volume_change(kw, ref)
    print('%s %s: restated volume change %.3f %% .. %.3f %%' % (name, mode, 100 * dvol.min(), 100 * dvol.max()))
    assert dvol.min() >= 1e-3 and dvol.max() <= 2e-2
    pred = GDMLPredict(model)
    keys = nr.PARITY_KEYS + ('enthalpy',)
    for B in nr.PARITY_BATCHES:
        m = nr.parity_measure(pred, name, mode, B)
        for k in keys:
            print('%s %s B=%d %s: sensitivity %.2e, error %.2e, allowed %.2e' % (name, mode, B, k, m[k]['sensitivity'],
                                                                                 m[k]['error'], m[k]['allowed']))
        assert m['frames_are_the_end']
        for k in keys:
            assert m[k]['error'] <= m[k]['allowed'], (k, m[k])


# ---- 3. frames are the predictor's

@pytest.mark.parametrize('mode', ['nph', 'npt'])
def test_frames_are_the_predictors_bits(mode):
    pred = _toy_predictor()
    for B in (1, 7):
        kw = _toy_kw(mode, n_steps=6, record_every=2, f_unit=1.5)
        kw.update(R0=kw['R0'][:B], V0=kw['V0'][:B], lattices=kw['lattices'][:B])
        out = pred.run_npt(**kw)
        assert out['R'].shape == (3, B, 18) and out['lattice'].shape == (3, B, 3, 3)
        for k in range(3):
            E, F, W = pred.predict_virial(out['R'][k], lattices=out['lattice'][k])
            assert np.array_equal(out['E_pot'][k], E) and np.array_equal(out['F'][k], F), k
            trW = W[:, 0, 0] + W[:, 1, 1] + W[:, 2, 2]
            P = (2.0 * out['E_kin'][k] - 1.5 * trW) / (3.0 * out['vol'][k])
            assert np.abs(out['pressure'][k] - P).max() <= 1e-12 * np.abs(P).max()
            det = np.abs(np.linalg.det(out['lattice'][k]))
            assert np.abs(out['vol'][k] - det).max() <= 1e-13 * det.max()
            H = out['E_kin'][k] + 1.5 * E + kw['pressure'] * out['vol'][k] + out['p_eps'][k] ** 2 / 40.0
            assert np.abs(out['enthalpy'][k] - H).max() <= 1e-13 * np.abs(H).max()
        assert (np.abs(out['lattice'][-1] - out['lattice'][0]).max(axis=(1, 2)) > 0.0).all()  # the cell moves


# ---- 4. bit-identical repetitions

@pytest.mark.parametrize('mode', ['nph', 'npt'])
def test_deterministic_continuation_chunks_and_record_every(mode):
    model, starts, L_starts, d0, fmax = cr.toy()
    pred = _toy_predictor()
    n = 9
    full = pred.run_npt(**_toy_kw(mode, n_steps=2 * n, step0=4))
    assert _same(full, pred.run_npt(**_toy_kw(mode, n_steps=2 * n, step0=4)))  # identical calls, identical bits
    a = pred.run_npt(**_toy_kw(mode, n_steps=n, step0=4))
    assert a['step_end'] == 4 + n
    b = pred.run_npt(**_toy_kw(mode, n_steps=n, R0=a['R_end'], V0=a['V_end'], state=a['state'], step0=a['step_end'],
                               lattices=None))
    for k in FRAMES:
        assert np.array_equal(np.concatenate([a[k], b[k]]), full[k]), k
    for k in ('R_end', 'V_end', 'lattice_end', 'vol_end'):
        assert np.array_equal(b[k], full[k]), k
    assert all(np.array_equal(b['state'][k], full['state'][k]) for k in ('eps', 'p_eps', 'L0')) and b['step_end'] == full['step_end']
    for every in (3, 2 * n):
        o = pred.run_npt(**_toy_kw(mode, n_steps=2 * n, step0=4, record_every=every))
        for k in FRAMES:
            assert np.array_equal(o[k], full[k][every - 1::every]), (k, every)
        assert all(np.array_equal(o[k], full[k]) for k in ENDS) and np.array_equal(o['state']['p_eps'], full['state']['p_eps'])
    ctx = pred._ctx
    try:
        for frames in (1, 5):
            ctx.set_option('predict.md_chunk_frames', frames)
            assert _same(full, pred.run_npt(**_toy_kw(mode, n_steps=2 * n, step0=4))), frames
    finally:
        ctx.set_option('predict.md_chunk_frames', 0)
    few = pred.run_npt(**_toy_kw(mode, n_steps=2, step0=4, record_every=3))  # no frame, two steps
    assert few['R'].shape == (0, 7, 18) and few['vol'].shape == (0, 7) and few['lattice'].shape == (0, 7, 3, 3)
    assert np.array_equal(few['R_end'], full['R'][1]) and np.array_equal(few['state']['p_eps'], full['p_eps'][1])
    none = pred.run_npt(**_toy_kw(mode, n_steps=0, step0=4))  # the start comes back
    kw = _toy_kw(mode)
    assert np.array_equal(none['R_end'], kw['R0']) and np.array_equal(none['V_end'], kw['V0']) and none['step_end'] == 4
    assert np.array_equal(none['lattice_end'], L_starts) and not none['state']['eps'].any() and not none['state']['p_eps'].any()
    assert none['E_pot'].shape == (0, 7)
    only = pred.run_npt(**_toy_kw(mode, n_steps=2 * n, step0=4, record=()))
    assert not any(k in only for k in ('R', 'V', 'F', 'lattice')) and _same(full, only, FRAMES[4:] + ENDS)


# ---- 5. the ensemble on the device

def test_langevin_piston_samples_the_ensemble_on_the_device():
    """The toy model, 256 replicas (the starts tiled), 5000 steps, the first 1000 dropped, scalars of every 5th step: <G_eps> =
    0, <2K>/3N = kT and <p_eps^2>/Wp = kT within 4 standard errors of the scatter of the replica means.  Measured on an MI355X:
    0.6, 3.0 and 2.1 standard errors (-0.12, -0.0073 and -0.015 kT), Vol within 0.941 - 1.143 of the toy cell's volume."""
    model, starts, L_starts, d0, fmax = cr.toy()
    e = nr.ENSEMBLE
    idx = np.arange(256) % 7
    out = _toy_predictor().run_npt(starts[idx], mr.start_velocities(256, 18, np.sqrt(e['kT'])), np.ones(6), e['dt'], 5000,
                                   cr.TOY_PRESSURE, e['piston_mass'], record_every=5, thermostat='langevin', gamma=e['gamma'],
                                   gamma_baro=e['gamma_baro'], kT=e['kT'], seed=e['seed'], lattices=L_starts[idx], record=())
    ratio = out['vol'] / abs(nr.det3(cr.TOY_LATTICE))  # (the volume the CPU test's condition is stated against)
    print('Vol/V0 in [%.3f, %.3f]' % (ratio.min(), ratio.max()))
    assert ratio.min() >= 0.9 and ratio.max() <= 1.25
    sl = slice(200, None)
    G = nr.g_from_frames(out['E_kin'], out['pressure'], out['vol'], cr.TOY_PRESSURE, 1.0 + 3.0 / 18)
    ids = nr.identities(out['E_kin'][sl], out['p_eps'][sl], G[sl], 18, e['kT'], e['piston_mass'])
    for k, (off, se) in ids.items():
        print('%s: off by %.3g = %.2f standard errors (%.4f kT)' % (k, off, abs(off) / se, off / e['kT']))
    for k, (off, se) in ids.items():
        assert abs(off) <= 4.0 * se, k


# ---- 6. NPH on the device

def test_nph_is_second_order_on_the_device():
    model, starts, L_starts, d0, fmax = cr.toy()
    pred = _toy_predictor()
    V0 = mr.start_velocities(7, 18, 0.02)
    E0 = pred.predict_virial(starts, lattices=L_starts)[0]
    H0 = (0.5 * V0 * V0).sum(axis=1) + E0 + cr.TOY_PRESSURE * np.abs(np.array([nr.det3(L) for L in L_starts]))
    dH = []
    for dt in (0.1, 0.05):
        o = pred.run_npt(starts, V0, np.ones(6), dt, int(round(20.0 / dt)), cr.TOY_PRESSURE, 20.0, lattices=L_starts, record=())
        dH.append(np.abs(o['enthalpy'] - H0[None]).max())
        print('dt = %.2f: max|dH| = %.3e' % (dt, dH[-1]))
    print('ratio %.3f' % (dH[0] / dH[1]))
    assert 3.5 <= dH[0] / dH[1] <= 4.5


# ---- 7. error paths before any launch

def test_error_paths_launch_nothing_and_leave_the_predictor_working():
    model, starts, L_starts, d0, fmax = cr.toy()
    pred = _toy_predictor()
    R0, L0 = np.array(starts[:3]), np.array(L_starts[:3])
    ok = dict(R0=R0, V0=np.zeros((3, 18)), masses=np.ones(6), dt=0.05, n_steps=4, pressure=0.0, piston_mass=20.0, lattices=L0)
    ok_bits = pred.predict_virial(R0, lattices=L0)

    def bad(exc=ValueError, **kw):
        with pytest.raises(exc):
            pred.run_npt(**dict(ok, **kw))
        for x, y in zip(ok_bits, pred.predict_virial(R0, lattices=L0)):
            assert np.array_equal(x, y)

    bad(lattices=L0, lattice=L0[0])
    bad(lattices=L0[:2])
    bad(lattices=np.zeros((3, 3, 3)))
    bad(lattices=None, lattice=np.eye(2))
    bad(lattices=None, lattice=np.zeros((3, 3)))
    bad(R0=R0[:, :15])
    bad(V0=np.zeros((2, 18)))
    bad(masses=np.ones(5))
    bad(masses=np.array([1.0, 1.0, 0.0, 1.0, 1.0, 1.0]), exc=(ValueError, _lib.GDMLHipError))
    bad(piston_mass=0.0)
    bad(piston_mass=-1.0)
    bad(piston_mass=float('nan'))
    bad(pressure=float('inf'))
    bad(pressure=float('nan'))
    bad(dt=float('nan'))
    bad(dt=0.0, exc=(ValueError, _lib.GDMLHipError))
    bad(gamma_baro=-1.0, exc=(ValueError, _lib.GDMLHipError))
    bad(gamma_baro=float('nan'))
    bad(thermostat='nose')
    bad(record=('R', 'W'))
    bad(seed=-1)
    bad(state=dict(eps=np.zeros(3), p_eps=np.zeros(3)))
    bad(state=dict(eps=np.zeros(2), p_eps=np.zeros(3), L0=L0))
    bad(state=dict(eps=np.array([0.0, np.nan, 0.0]), p_eps=np.zeros(3), L0=L0))
    bad(state=dict(eps=np.zeros(3), p_eps=np.zeros(3), L0=np.zeros((3, 3, 3))))
    R_nan = R0.copy()
    R_nan[1, 4] = np.nan
    bad(R0=R_nan)
    nolat = GDMLPredict({k: v for k, v in model.items() if k != 'lattice'})
    with pytest.raises(ValueError, match='needs a lattice'):
        nolat.run_npt(R0, ok['V0'], ok['masses'], 0.05, 2, 0.0, 20.0)
    dflt = pred.run_npt(**dict(ok, lattices=None))  # the model's lattice by default
    assert np.array_equal(dflt['state']['L0'], np.broadcast_to(model['lattice'], (3, 3, 3)))
    out = pred.run_npt(**ok)  # and the integrator itself still works
    assert out['step_end'] == 4 and np.isfinite(out['enthalpy']).all()
    assert GDMLPredict.piston_mass(6, 0.002, 10.0) == 21 * 0.002 * 100.0


def test_blow_up_names_replica_and_step():
    model, starts, L_starts, d0, fmax = cr.toy()
    pred = _toy_predictor()
    V0 = np.zeros((3, 18))
    V0[1, 0] = 1e200  # overflows the kinetic energy of replica 1 at the first step
    with pytest.raises(FloatingPointError, match='replica 1 .* step 7'):
        pred.run_npt(starts[:3], V0, np.ones(6), 0.05, 5, 0.0, 20.0, lattices=L_starts[:3], step0=7)


def test_c_entry_null_context_empty_batch_and_missing_model():
    model, starts, L_starts, d0, fmax = cr.toy()
    ctx = _toy_predictor()._ctx
    lib = ctx._lib
    mass = np.ones(6)
    prm = _lib.NPTParams(1, 6, 0.05, _lib._ptr(mass), 1.0, 0, 0.0, 0.0, 0.0, 0, 0, 0.0, 20.0)
    R, V, eps, p_eps = np.array(starts[:1]), np.zeros((1, 18)), np.zeros(1), np.zeros(1)
    L0, Li = np.array(L_starts[:1]), np.array([cr.inv3(L_starts[0])])
    args = [_lib._ptr(a) for a in (R, V, eps, p_eps, L0, Li)]
    assert lib.gdml_npt_run(None, C.byref(prm), *args, 4, 1, *([None] * 10)) == -1
    assert 'ctx is NULL' in lib.gdml_last_error(None).decode()
    prm5 = _lib.NPTParams(1, 5, 0.05, _lib._ptr(mass), 1.0, 0, 0.0, 0.0, 0.0, 0, 0, 0.0, 20.0)
    assert lib.gdml_npt_run(ctx._h, C.byref(prm5), *args, 4, 1, *([None] * 10)) == -1  # N differs from the model's
    assert lib.gdml_npt_run(ctx._h, C.byref(prm), *args, 4, 1, *([None] * 10)) == 0  # no frame array is required
    assert not np.array_equal(R, starts[:1]) and eps[0] != 0.0
    empty = ctx.npt_run(np.zeros((0, 18)), np.zeros((0, 18)), np.zeros(0), np.zeros(0), np.zeros((0, 3, 3)), np.zeros((0, 3, 3)),
                        mass, 0.05, 4, 0.0, 20.0, record=('R', 'lat'))
    assert empty['R'].shape == (4, 0, 18) and empty['vol'].shape == (4, 0) and empty['R_end'].shape == (0, 18)
    bare = _lib.Context(0)
    try:
        bare.model_n_atoms = 6
        with pytest.raises(_lib.GDMLHipError):  # no model resident
            bare.npt_run(R, V, eps, p_eps, L0, Li, mass, 0.05, 4, 0.0, 20.0)
    finally:
        bare.close()

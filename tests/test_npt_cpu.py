"""CPU-side checks of the on-device constant-pressure dynamics (gdml_npt_run, csrc/npt.hip): the restated integrator
(tests/_npt_ref.py) as a yardstick on the closed-form springs of the periodic toy -- second order, time reversible, the three
ensemble identities of the Langevin piston -- its reduction to the restated run_md with an infinitely heavy piston, the
piston's place in the noise stream, and the library surface (exports, argument errors that need no device)."""
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

P_EXT = cr.TOY_PRESSURE


@functools.lru_cache(maxsize=None)
def _springs():
    model, starts, L_starts, d0, fmax = cr.toy()
    return cr.springs_virial_fn(d0), starts, L_starts, np.ones(6)


def _toy_volume():
    """V0 of the volume conditions: the volume of the toy's own cell TOY_LATTICE, which the seven starts strain by -4.6 % to
    +1 %.  Measured on the restatement: 0.950 - 1.163 in NPH (dt-converged) and 0.941 - 1.143 under the Langevin piston.
    Against each start's OWN volume the NPH runs span 0.955 - 1.202, the ensemble runs 0.939 - 1.180: the NPH bound of 1.2 is a
    statement about the toy's cell, not about the replica's reference lattice."""
    return abs(nr.det3(cr.TOY_LATTICE))


def test_batched_springs_are_the_toys_springs():
    model, starts, L_starts, d0, fmax = cr.toy()
    a = cr.springs_virial_fn(d0)(starts, L_starts)
    b = nr.springs_batch_fn(d0)(starts, L_starts)
    for x, y in zip(a, b):
        assert np.abs(x - y).max() <= 1e-14 * max(1.0, np.abs(x).max())


def test_restated_nph_is_second_order():
    """NPH, Wp = 20, 20 time units at dt = 0.2, 0.1, 0.05: max|H - H(0)| falls by 4 per halving (3.5 - 4.5), no pair crosses the
    minimum-image boundary and the volume stays within [0.9, 1.2] V0."""
    fn, starts, L_starts, masses = _springs()
    V0 = mr.start_velocities(7, 18, 0.02)
    H0 = nr.enthalpy_start(fn, starts, V0, masses, L_starts, P_EXT, 20.0)
    vol0 = _toy_volume()
    dH = []
    for dt in (0.2, 0.1, 0.05):
        o = nr.run(fn, starts, V0, masses, L_starts, dt, int(round(20.0 / dt)), P_EXT, 20.0)
        dH.append(np.abs(o['enthalpy'] - H0[None]).max())
        margin = cr.image_integers(o['R_end'], o['lattice_end'])[1]
        ratio = o['vol'] / vol0
        print('dt = %.2f: max|dH| = %.2e, image margin %.3f, Vol/V0 in [%.3f, %.3f]' % (dt, dH[-1], margin, ratio.min(),
                                                                                       ratio.max()))
        assert margin > 0.0
        assert ratio.min() >= 0.9 and ratio.max() <= 1.2
    print('ratios %.3f %.3f' % (dH[0] / dH[1], dH[1] / dH[2]))
    assert 3.5 <= dH[0] / dH[1] <= 4.5 and 3.5 <= dH[1] / dH[2] <= 4.5


def test_restated_nph_is_time_reversible():
    """100 steps, v and p_eps flipped, 100 more steps: back at the start within 1e-12."""
    fn, starts, L_starts, masses = _springs()
    V0 = mr.start_velocities(7, 18, 0.1)
    a = nr.run(fn, starts, V0, masses, L_starts, 0.05, 100, P_EXT, 20.0)
    b = nr.run(fn, a['R_end'], -a['V_end'], masses, L_starts, 0.05, 100, P_EXT, 20.0, eps0=a['state']['eps'],
               p_eps0=-a['state']['p_eps'])
    err = (np.abs(b['R_end'] - starts).max(), np.abs(-b['V_end'] - V0).max(), np.abs(b['state']['eps']).max(),
           np.abs(b['state']['p_eps']).max())
    print('back at the start within R %.1e, V %.1e, eps %.1e, p_eps %.1e' % err)
    assert np.abs(a['state']['eps']).max() > 1e-4  # the cell moved
    assert max(err) <= 1e-12


def test_restated_langevin_piston_samples_the_ensemble():
    """64 replicas, 6000 steps, the first 1000 dropped: <G_eps> = 0, <2K>/3N = kT and <p_eps^2>/Wp = kT within 4 standard errors
    of the scatter of the replica means; G_eps written with kappa = 1 on the same data is more than 4 standard errors off."""
    model, starts, L_starts, d0, fmax = cr.toy()
    e = nr.ENSEMBLE
    idx = np.arange(64) % 7
    R0, L0 = starts[idx], L_starts[idx]
    V0 = mr.start_velocities(64, 18, np.sqrt(e['kT']))
    o = nr.run(nr.springs_batch_fn(d0), R0, V0, np.ones(6), L0, e['dt'], 6000, P_EXT, e['piston_mass'], thermostat='langevin',
               gamma=e['gamma'], gamma_baro=e['gamma_baro'], kT=e['kT'], seed=e['seed'])
    ratio = o['vol'] / _toy_volume()
    print('Vol/V0 in [%.3f, %.3f]' % (ratio.min(), ratio.max()))
    assert ratio.min() >= 0.9 and ratio.max() <= 1.25
    sl = slice(1000, None)
    ids = nr.identities(o['E_kin'][sl], o['p_eps'][sl], o['G_eps'][sl], 18, e['kT'], e['piston_mass'])
    for k, (off, se) in ids.items():
        print('%s: off by %.3g = %.2f standard errors (%.4f kT)' % (k, off, abs(off) / se, off / e['kT']))
    # the recorded fields alone give the same G_eps
    G = nr.g_from_frames(o['E_kin'], o['pressure'], o['vol'], P_EXT, 1.0 + 3.0 / 18)
    assert np.abs(G - o['G_eps']).max() <= 1e-12
    G1 = nr.g_from_frames(o['E_kin'], o['pressure'], o['vol'], P_EXT, 1.0)
    off1, se1 = nr.identities(o['E_kin'][sl], o['p_eps'][sl], G1[sl], 18, e['kT'], e['piston_mass'])['G_eps']
    print('G_eps with kappa = 1: off by %.2f standard errors' % (abs(off1) / se1))
    for k, (off, se) in ids.items():
        assert abs(off) <= 4.0 * se, k
    assert abs(off1) > 4.0 * se1


@pytest.mark.parametrize('thermostat', [None, 'langevin'])
def test_infinite_piston_mass_is_the_restated_md(thermostat):
    fn, starts, L_starts, masses = _springs()
    masses = np.linspace(1.0, 2.0, 6)
    V0 = mr.start_velocities(7, 18, 0.05)
    kw = dict(thermostat=thermostat, gamma=0.3, kT=0.004, seed=9, step0=3)
    md = mr.run(lambda R: fn(R, L_starts)[:2], starts, V0, masses, 0.05, 12, **kw)
    o = nr.run(fn, starts, V0, masses, L_starts, 0.05, 12, 0.37, np.inf, gamma_baro=0.4, p_eps0=np.full(7, 0.5), **kw)
    for k in ('R', 'V', 'E_pot', 'E_kin', 'R_end', 'V_end'):
        assert np.array_equal(o[k], md[k]), k
    assert np.array_equal(o['lattice'], np.broadcast_to(L_starts, (12, 7, 3, 3))) and not o['state']['eps'].any()
    assert np.isfinite(o['p_eps']).all() and np.isfinite(o['enthalpy']).all()


def test_piston_noise_is_coordinate_3n_of_the_stream():
    """One Langevin step: p_eps(1) = b1 (p_eps(0) + dt/2 G(0)) + b2 sqrt(Wp kT) xi + dt/2 G(1) gives xi back."""
    fn, starts, L_starts, masses = _springs()
    V0 = mr.start_velocities(7, 18, 0.05)
    dt, Wp, kT, gb, seed, step0 = 0.1, 20.0, 0.002, 0.7, 123, 41
    o = nr.run(fn, starts, V0, masses, L_starts, dt, 1, P_EXT, Wp, thermostat='langevin', gamma=0.2, gamma_baro=gb, kT=kT,
               seed=seed, step0=step0, p_eps0=np.full(7, 0.01))
    E, F, W = fn(starts, L_starts)
    K = (0.5 * V0 * V0).sum(axis=1)
    G0 = nr.g_eps(1.0 + 3.0 / 18, K, W, np.abs(np.linalg.det(L_starts)), P_EXT)
    b1 = np.exp(-gb * dt)
    xi = (o['p_eps'][0] - 0.5 * dt * o['G_eps'][0] - b1 * (0.01 + 0.5 * dt * G0)) / (np.sqrt(1.0 - b1 * b1) * np.sqrt(Wp * kT))
    want = mr.normals(seed, step0, 7, 19)
    assert np.abs(xi - want[:, 18]).max() <= 1e-9
    assert np.array_equal(want[:, :18], mr.normals(seed, step0, 7, 18))  # the particles' noise is run_md's


# ---- the library surface

def test_library_exports_the_npt_entry():
    """Fails without the feature.  The change is additive: gdml_abi_version() stays."""
    lib = _lib.load()
    assert hasattr(lib, 'gdml_npt_run') and 'gdml_npt_run' in _lib.SIGNATURES
    assert lib.gdml_abi_version() == 4
    assert C.sizeof(_lib.NPTParams) == 104  # 8-byte members, two ints padded to 8


def _params(**kw):
    mass = kw.pop('mass', np.ones(3))
    d = dict(B=1, N=3, dt=0.01, f_scale=1.0, thermostat=0, gamma=0.0, gamma_baro=0.0, kT=0.0, seed=0, step0=0, pressure=0.0,
             piston_mass=10.0)
    d.update(kw)
    p = _lib.NPTParams(d['B'], d['N'], d['dt'], _lib._ptr(mass), d['f_scale'], d['thermostat'], d['gamma'], d['gamma_baro'],
                       d['kT'], d['seed'], d['step0'], d['pressure'], d['piston_mass'])
    p._keep = mass
    return p


def test_argument_errors_need_no_device():
    """Every argument check of gdml_npt_run comes before the first use of the context: with ctx = NULL each bad argument
    returns GDML_ERR_INVALID with its own message, and good arguments get as far as the missing context."""
    lib = _lib.load()
    a = dict(R=np.zeros((1, 9)), V=np.zeros((1, 9)), eps=np.zeros(1), p_eps=np.zeros(1), L0=np.eye(3)[None].copy(),
             L0_inv=np.eye(3)[None].copy())

    def call(p, n_steps=4, record_every=1, **nulls):
        q = {k: (None if k in nulls else _lib._ptr(v)) for k, v in a.items()}
        rc = lib.gdml_npt_run(None, None if p is None else C.byref(p), q['R'], q['V'], q['eps'], q['p_eps'], q['L0'], q['L0_inv'],
                              n_steps, record_every, *([None] * 10))
        return rc, lib.gdml_last_error(None).decode()

    assert call(_params()) == (-1, 'gdml_npt_run: ctx is NULL')
    assert call(_params(piston_mass=np.inf, thermostat=1, gamma=0.1, gamma_baro=0.1, kT=1.0)) == (-1, 'gdml_npt_run: ctx is NULL')
    assert call(_params(B=0)) == (-1, 'gdml_npt_run: ctx is NULL')
    bad = [
        (dict(n_steps=-1), {}, 'n_steps'), (dict(record_every=0), {}, 'record_every'),
        ({}, dict(mass=np.array([1.0, 0.0, 1.0])), 'mass'), ({}, dict(mass=np.array([1.0, np.nan, 1.0])), 'mass'),
        ({}, dict(dt=0.0), 'dt'), ({}, dict(dt=np.nan), 'dt'), ({}, dict(gamma=-1.0), 'gamma'), ({}, dict(kT=-1.0), 'kT'),
        ({}, dict(thermostat=2), 'thermostat'), ({}, dict(step0=-1), 'step0'), ({}, dict(B=-1), 'B out of range'),
        ({}, dict(N=0), 'N out of range'), ({}, dict(f_scale=np.inf), 'f_scale'),
        ({}, dict(gamma_baro=-0.5), 'gamma_baro'), ({}, dict(gamma_baro=np.nan), 'gamma_baro'),
        ({}, dict(piston_mass=0.0), 'piston_mass'), ({}, dict(piston_mass=-3.0), 'piston_mass'),
        ({}, dict(piston_mass=np.nan), 'piston_mass'), ({}, dict(pressure=np.inf), 'pressure'),
        ({}, dict(pressure=np.nan), 'pressure'),
        (dict(R=1), {}, 'R or V'), (dict(V=1), {}, 'R or V'), (dict(eps=1), {}, 'eps'), (dict(p_eps=1), {}, 'p_eps'),
        (dict(L0=1), {}, 'L0'), (dict(L0_inv=1), {}, 'L0'),
    ]
    for kw_call, kw_par, token in bad:
        rc, msg = call(_params(**kw_par), **kw_call)
        assert rc == -1 and token in msg and 'ctx is NULL' not in msg, (kw_call, kw_par, msg)
    rc, msg = call(None)
    assert rc == -1 and 'params is NULL' in msg

"""CPU-side checks of the on-device path-integral MD (gdml_pimd_run, gdml_pimd_modes, csrc/pimd.hip): the library surface
(exports, struct layout, argument errors that need no device), the normal-mode matrix of the library against its defining
properties and the restatement's, and the restated integrator (tests/_pimd_ref.py) as a yardstick: exact free flow, restart,
the quantum harmonic oscillator's kinetic energy, second-order drift."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _md_ref as mr  # noqa: E402
import _pimd_ref as pr  # noqa: E402
from sgdml_amd import _lib  # noqa: E402


def test_library_exports_the_pimd_entries():
    """Fails without the feature.  The change is additive, so gdml_abi_version() stays 4."""
    lib = _lib.load()
    for name in ('gdml_pimd_run', 'gdml_pimd_modes'):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert lib.gdml_abi_version() == 4
    assert C.sizeof(_lib.PIMDParams) == 112  # 8-byte members; N and beads share one, thermostat is padded to 8
    assert C.sizeof(_lib.MDParams) == 96


@pytest.mark.parametrize('P', [1, 2, 3, 4, 7, 16, 128])
def test_modes_of_the_library(P):
    """Fails without the feature.  C is orthonormal, diagonalises the ring's spring matrix with the stated frequencies, and
    is the restatement's matrix to 4 ulp of the largest entry (libm's cos against NumPy's, the angle reduced exactly)."""
    kT, hbar = 0.7, 0.3
    Cm, omega = _lib.Context.pimd_modes(P, kT, hbar)
    assert Cm.shape == (P, P) and omega.shape == (P,)
    assert np.abs(Cm.T @ Cm - np.eye(P)).max() <= 1e-14
    wP = P * kT / hbar
    S = 2.0 * np.eye(P) - np.roll(np.eye(P), 1, axis=0) - np.roll(np.eye(P), -1, axis=0)  # cyclic second difference
    lam = Cm.T @ S @ Cm * wP**2
    scale = max((omega**2).max(), wP**2)
    assert np.abs(lam - np.diag(omega**2)).max() <= 1e-12 * scale
    C_ref, w_ref = pr.modes(P, kT, hbar)
    assert np.abs(Cm - C_ref).max() <= 4 * np.finfo(float).eps * np.abs(C_ref).max()
    assert np.abs(omega - w_ref).max() <= 4 * np.finfo(float).eps * max(np.abs(w_ref).max(), 1e-300)
    assert omega[0] == 0.0


def test_modes_argument_errors():
    for bad in (dict(beads=0), dict(beads=129), dict(hbar=0.0), dict(hbar=-1.0), dict(hbar=np.inf), dict(kT=-1.0)):
        with pytest.raises(ValueError):
            _lib.Context.pimd_modes(**dict(dict(beads=4, kT=1.0, hbar=1.0), **bad))


def _params(**kw):
    mass = kw.pop('mass', np.ones(3))
    lat = kw.pop('lat', None)
    lat_inv = kw.pop('lat_inv', None)
    d = dict(B=1, N=3, beads=2, dt=0.01, f_scale=1.0, thermostat=0, gamma_centroid=0.0, pile_lambda=1.0, kT=1.0, hbar=1.0, seed=0,
             step0=0)
    d.update(kw)
    p = _lib.PIMDParams(d['B'], d['N'], d['beads'], d['dt'], _lib._ptr(mass), d['f_scale'], _lib._ptr(lat), _lib._ptr(lat_inv),
                        d['thermostat'], d['gamma_centroid'], d['pile_lambda'], d['kT'], d['hbar'], d['seed'], d['step0'])
    p._keep = (mass, lat, lat_inv)
    return p


def test_argument_errors_need_no_device():
    """Every argument check of gdml_pimd_run comes before the first use of the context: with ctx = NULL each bad argument
    returns GDML_ERR_INVALID with its own message, and good arguments get as far as the missing context."""
    lib = _lib.load()
    R, V = np.zeros((1, 2, 9)), np.zeros((1, 2, 9))
    eye = np.eye(3)

    def call(p, n_steps=4, record_every=1):
        rc = lib.gdml_pimd_run(None, C.byref(p), _lib._ptr(R), _lib._ptr(V), n_steps, record_every, None, None, None, None, None,
                               None, None)
        return rc, lib.gdml_last_error(None).decode()

    assert call(_params()) == (-1, 'gdml_pimd_run: ctx is NULL')
    assert call(_params(lat=eye, lat_inv=eye, thermostat=1, gamma_centroid=0.5)) == (-1, 'gdml_pimd_run: ctx is NULL')
    assert call(_params(beads=1, kT=0.0)) == (-1, 'gdml_pimd_run: ctx is NULL')  # kT = 0 is classical MD's, allowed for one bead
    assert call(_params(beads=128)) == (-1, 'gdml_pimd_run: ctx is NULL')
    bad = [
        # what gdml_md_run rejects
        (dict(n_steps=-1), {}, 'n_steps'), (dict(record_every=0), {}, 'record_every'),
        ({}, dict(mass=np.array([1.0, 0.0, 1.0])), 'mass'), ({}, dict(mass=np.array([1.0, 1.0, -2.0])), 'mass'),
        ({}, dict(mass=np.array([1.0, np.nan, 1.0])), 'mass'),
        ({}, dict(dt=0.0), 'dt'), ({}, dict(dt=-0.1), 'dt'), ({}, dict(dt=np.nan), 'dt'), ({}, dict(gamma_centroid=-1.0), 'gamma'),
        ({}, dict(kT=-1.0), 'kT'), ({}, dict(lat=eye), 'lattice'), ({}, dict(lat_inv=eye), 'lattice'),
        ({}, dict(thermostat=2), 'thermostat'), ({}, dict(thermostat=-1), 'thermostat'), ({}, dict(step0=-1), 'step0'),
        ({}, dict(B=-1), 'B out of range'), ({}, dict(f_scale=np.inf), 'f_scale'), ({}, dict(N=0), 'N out of range'),
        # the ring's own
        ({}, dict(beads=0), 'beads'), ({}, dict(beads=129), 'beads'), ({}, dict(beads=-3), 'beads'),
        ({}, dict(hbar=0.0), 'hbar'), ({}, dict(hbar=-1.0), 'hbar'), ({}, dict(hbar=np.inf), 'hbar'), ({}, dict(hbar=np.nan), 'hbar'),
        ({}, dict(kT=0.0), 'kT'), ({}, dict(pile_lambda=0.0), 'pile_lambda'), ({}, dict(pile_lambda=-1.0), 'pile_lambda'),
        ({}, dict(B=2**24, beads=128), 'B * beads'),
    ]
    for kw_call, kw_par, token in bad:
        rc, msg = call(_params(**kw_par), **kw_call)
        assert rc == -1 and token in msg and 'ctx is NULL' not in msg, (kw_call, kw_par, msg)
    p = _params()
    assert lib.gdml_pimd_run(None, C.byref(p), None, _lib._ptr(V), 4, 1, None, None, None, None, None, None, None) == -1
    assert 'R or V' in lib.gdml_last_error(None).decode()
    assert lib.gdml_pimd_run(None, None, _lib._ptr(R), _lib._ptr(V), 4, 1, None, None, None, None, None, None, None) == -1


def _zero_force(R):
    return np.zeros(len(R)), np.zeros_like(R)


@pytest.mark.parametrize('P', [3, 4])
def test_free_ring_follows_the_closed_form(P):
    """Zero force: n steps of the restated NVE ring are the normal-mode solution at t = n dt, to 1e-12 (omega_max dt = 1, so
    every step is a real rotation)."""
    rs = np.random.RandomState(P)
    B, n3, dt, kT, n = 2, 6, 0.05, 0.3, 25
    hbar = 2 * P * kT * dt
    masses = np.array([1.0, 1.7])
    R0, V0 = rs.standard_normal((B, P, n3)), rs.standard_normal((B, P, n3))
    out = pr.run(_zero_force, R0, V0, masses, dt, n, P, kT, hbar)
    Cm, omega = pr.modes(P, kT, hbar)
    assert abs(omega.max() * dt - (1.0 if P % 2 == 0 else np.sin((P // 2) * np.pi / P))) <= 1e-15
    q0, v0 = np.einsum('jk,bjc->bkc', Cm, R0), np.einsum('jk,bjc->bkc', Cm, V0)
    q, v = pr.flow(q0, v0, omega, n * dt)
    R, V = np.einsum('jk,bkc->bjc', Cm, q), np.einsum('jk,bkc->bjc', Cm, v)
    eR, eV = np.abs(out['R_end'] - R).max(), np.abs(out['V_end'] - V).max()
    print('P = %d: free flow after %d steps, R %.2e, V %.2e' % (P, n, eR, eV))
    assert eR <= 1e-12 * np.abs(R).max() and eV <= 1e-12 * np.abs(V).max()
    # the ring's energy is conserved by the exact flow
    H = out['E_kin'] + out['E_spring']
    assert np.abs(H - H[0]).max() <= 1e-12 * np.abs(H).max()


def test_restated_pile_restarts_bit_for_bit():
    model, R0, V0 = pr.start('n6_p1', 2, 3)
    masses = np.linspace(1.0, 2.0, R0.shape[2] // 3)
    fn = mr.force_fn(model)
    kw = dict(beads=3, kT=0.05, hbar=2 * 3 * 0.05 * 0.02, thermostat='pile', gamma_centroid=0.5, seed=3)
    full = pr.run(fn, R0, V0, masses, 0.02, 12, **kw)
    a = pr.run(fn, R0, V0, masses, 0.02, 6, **kw)
    b = pr.run(fn, a['R_end'], a['V_end'], masses, 0.02, 6, step0=a['step_end'], **kw)
    assert b['step_end'] == 12
    assert np.array_equal(b['R_end'], full['R_end']) and np.array_equal(b['V_end'], full['V_end'])
    for k in ('R', 'V', 'E') + pr.RING:
        assert np.array_equal(b[k], full[k][6:]), k
    nve = pr.run(fn, R0, V0, masses, 0.02, 12, beads=3, kT=0.05, hbar=kw['hbar'])
    assert not np.array_equal(full['R'], nve['R'])


def test_restated_collapsed_ring_stays_collapsed():
    """All beads at one point with one velocity, no thermostat: the internal modes are formed from r_j - r_0, so they are
    exactly zero and every bead follows the classical trajectory with the others, bit for bit."""
    model, R7 = mr.case('n6_p1')
    P, n3 = 3, R7.shape[1]
    R0 = np.repeat(R7[:2, None, :], P, axis=1)
    V0 = np.repeat(mr.start_velocities(2, n3, 0.2)[:, None, :], P, axis=1)
    out = pr.run(mr.force_fn(model), R0, V0, np.linspace(1.0, 2.0, n3 // 3), 0.02, 10, P, 0.05, 2 * P * 0.05 * 0.02)
    for k in ('R', 'V'):
        assert np.array_equal(out[k], np.repeat(out[k][:, :, :1], P, axis=2)), k
    assert np.all(out['E_spring'] == 0.0) and not np.array_equal(out['R'][-1], R0)


W_HO = 3.0


def _oscillator(R):
    return 0.5 * W_HO**2 * (R * R).sum(axis=1), -W_HO**2 * R


def _oscillator_run(P, dt):
    """512 one-dimensional rings, kT = hbar = m = 1, centroid friction 1; per-ring time averages after 1000 discarded steps."""
    B = 512
    R0 = np.zeros((B, P, 1))
    V0 = np.sqrt(P * 1.0) * np.random.RandomState(2).standard_normal((B, P, 1))
    out = pr.run(_oscillator, R0, V0, np.ones(1), dt, 6000, P, 1.0, 1.0, thermostat='pile', gamma_centroid=1.0, seed=11,
                 record=(), dof_masses=True)
    return {k: out[k][1000:].mean(axis=0) for k in ('K_cv', 'K_prim', 'E_pot')}


def _exact_kinetic(P):
    _, omega = pr.modes(P, 1.0, 1.0)
    return 0.5 * (W_HO**2 / (W_HO**2 + omega**2)).sum()


@pytest.mark.parametrize('P', [4, 8])
def test_harmonic_oscillator_estimators(P):
    """Quantum harmonic oscillator, omega = 3, kT = hbar = m = 1: the exact P-bead kinetic energy is (kT/2) sum_k omega^2 /
    (omega^2 + omega_k^2).  The ring averages of K_cv and of the bead-mean potential (equal to it by the virial theorem) at
    dt = 0.02, and of K_prim at dt = 0.01, within five standard errors (spread of the 512 per-ring averages / sqrt 512)."""
    exact = _exact_kinetic(P)
    assert abs(exact - {4: 0.7812, 8: 0.8158}[P]) <= 5e-5
    for dt, names in ((0.02, ('K_cv', 'E_pot')), (0.01, ('K_prim',))):
        avg = _oscillator_run(P, dt)
        for k in names:
            mean, se = avg[k].mean(), avg[k].std(ddof=1) / np.sqrt(len(avg[k]))
            print('P = %d dt = %.2f %s: %.4f +- %.4f (exact %.4f, %.1f standard errors)' % (P, dt, k, mean, se, exact,
                                                                                         abs(mean - exact) / se))
            assert abs(mean - exact) <= 5.0 * se, (P, dt, k)


@pytest.mark.parametrize('name,P', [('n6_p1', 3), ('n6_p1', 4), ('n100_m3', 4)])
def test_restated_ring_drift_is_second_order(name, P):
    """Halving dt over the same physical time (the same hbar) divides the drift of H_P by 4: 3.5 - 4.5 for the restatement (the
    GPU tests allow 3 - 5)."""
    model, R0, V0 = pr.start(name, 1, P)
    masses = np.ones(R0.shape[2] // 3)
    fn = mr.force_fn(model)
    dt, kT, n = mr.DT[name], 0.05, 40
    hbar = 2 * P * kT * dt
    E0, F0 = fn(R0.reshape(P, -1))
    q0 = pr.ring_quantities(R0, V0, E0[None], F0[None], np.repeat(masses, 3)[None, None, :], P, kT, P * kT / hbar, 1.0)
    H0 = P * q0[0] + q0[1] + q0[2]
    d = []
    for h, steps in ((dt, n), (dt / 2, 2 * n)):
        out = pr.run(fn, R0, V0, masses, h, steps, P, kT, hbar, record=())
        d.append(np.abs(pr.hamiltonian(out, P) - H0[None]).max())
    print('%s P = %d: drift %.3e at dt, %.3e at dt/2, ratio %.3f' % (name, P, d[0], d[1], d[0] / d[1]))
    assert 3.5 <= d[0] / d[1] <= 4.5

"""CPU-side checks of the on-device molecular dynamics (gdml_md_run, csrc/md.hip): the restated noise stream against the
generator's published vectors and the moments of a normal, the restated integrator as a yardstick (second order), and the
library surface (exports, argument errors that need no device)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _md_ref as mr  # noqa: E402
from sgdml_amd import _lib  # noqa: E402


def _hex(words):
    return ' '.join('%08x' % int(w) for w in words)


def test_philox_known_answer_vectors():
    """Philox4x32-10 known-answer vectors of the generator's authors (Random123 kat_vectors)."""
    f = 0xFFFFFFFF
    assert _hex(mr.philox4x32_10((0, 0), (0, 0, 0, 0))) == '6627e8d5 e169c58d bc57ac4c 9b00dbd8'
    assert _hex(mr.philox4x32_10((f, f), (f, f, f, f))) == '408f276d 41c83b0e a20bc7c6 6d5451fd'
    assert _hex(mr.philox4x32_10((0xA4093822, 0x299F31D0), (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344))) == \
        'd16cfe09 94fdcceb 5001e420 24126ea1'


def test_noise_depends_on_seed_step_replica_coordinate_only():
    a = mr.normals(12345, 7, 5, 63)
    assert np.array_equal(mr.normals(12345, 7, 3, 63), a[:3])  # not on B
    assert np.array_equal(mr.normals(12345, 7, 5, 30), a[:, :30])  # not on the number of coordinates (tail block included)
    assert not np.array_equal(mr.normals(12345, 8, 5, 63), a)
    assert not np.array_equal(mr.normals(12346, 7, 5, 63), a)
    assert not np.array_equal(mr.normals(12345 + 2**32, 7, 5, 63), a)  # the high half of the seed is part of the key
    assert not np.array_equal(mr.normals(12345, 7 + 2**32, 5, 63), a)  # and the high half of the step of the counter
    assert len(np.unique(a)) == a.size


def test_restated_normals_have_the_moments_of_a_normal():
    """10^6 draws.  For n independent standard normals the sample mean has standard error 1 / sqrt n, the mean of x^2
    sqrt(2 / n) (var x^2 = 3 - 1), the mean of x^4 sqrt(96 / n) (var x^4 = E x^8 - 9 = 105 - 9) and the mean of x_i x_{i+1}
    1 / sqrt(n - 1) (var of a product of independent normals = 1).  Each statistic within five standard errors."""
    x = mr.normals(2024, 3, 1000, 1000).ravel()
    n = x.size
    assert n == 10**6
    stats = {
        'mean': (x.mean(), 0.0, 1.0 / np.sqrt(n)),
        'variance': ((x * x).mean(), 1.0, np.sqrt(2.0 / n)),
        'fourth moment': ((x**4).mean(), 3.0, np.sqrt(96.0 / n)),
        'lag-1 correlation': ((x[:-1] * x[1:]).mean(), 0.0, 1.0 / np.sqrt(n - 1)),
    }
    for what, (got, want, se) in stats.items():
        print('%s: %.5f (expected %.1f, standard error %.1e)' % (what, got, want, se))
        assert abs(got - want) <= 5.0 * se, what
    assert np.abs(x).max() < 7.0  # u >= 2^-33: |xi| <= sqrt(2 * 33 ln 2) = 6.8


@pytest.mark.parametrize('name', ['n6_p1', 'n100_m3'])
def test_restated_verlet_is_second_order(name):
    """The yardstick itself: halving dt over the same physical time divides the energy drift of the restated velocity Verlet
    by 4 (3.5 - 4.5 for the restatement alone; the GPU tests allow 3 - 5), with steps of at most 1 % of the shortest pair
    distance.  The GPU tests reuse these dt."""
    model, R7 = mr.case(name)
    n3 = R7.shape[1]
    masses = np.ones(n3 // 3)
    R0, V0 = R7[:1], mr.start_velocities(1, n3, mr.V_SCALE[name])
    fn = mr.force_fn(model)
    dt, n = mr.DT[name], 40
    d1, s1 = mr.drift(fn, R0, V0, masses, dt, n)
    d2, s2 = mr.drift(fn, R0, V0, masses, dt / 2, 2 * n)
    dmin = mr.min_pair_distance(model, R0)
    print('%s: drift %.3e at dt, %.3e at dt/2, ratio %.3f; largest step %.4f, shortest distance %.4f' % (name, d1, d2, d1 / d2, s1,
                                                                                                   dmin))
    assert 3.5 <= d1 / d2 <= 4.5
    assert max(s1, s2) <= 0.01 * dmin


def test_restated_langevin_reduces_to_verlet_and_restarts():
    model, R7 = mr.case('n6_p1')
    n3 = R7.shape[1]
    masses = np.linspace(1.0, 2.0, n3 // 3)
    R0, V0 = R7[:3], mr.start_velocities(3, n3, 0.3)
    fn = mr.force_fn(model)
    nve = mr.run(fn, R0, V0, masses, 0.02, 12)
    lan0 = mr.run(fn, R0, V0, masses, 0.02, 12, thermostat='langevin', gamma=0.0, kT=0.7, seed=3)
    assert np.abs(lan0['R'] - nve['R']).max() <= 1e-13  # c1 = 1, c2 = 0: the two half drifts are one drift, to rounding
    full = mr.run(fn, R0, V0, masses, 0.02, 12, thermostat='langevin', gamma=0.5, kT=0.7, seed=3)
    a = mr.run(fn, R0, V0, masses, 0.02, 6, thermostat='langevin', gamma=0.5, kT=0.7, seed=3)
    b = mr.run(fn, a['R_end'], a['V_end'], masses, 0.02, 6, thermostat='langevin', gamma=0.5, kT=0.7, seed=3, step0=a['step_end'])
    assert np.array_equal(b['R_end'], full['R_end']) and np.array_equal(b['R'], full['R'][6:])
    assert not np.array_equal(full['R'], nve['R'])


def test_library_exports_the_md_entries():
    """Fails without the feature: the two entry points are exported and bound.  The change is additive (no existing signature
    moved), so gdml_abi_version() stays at the value every other ABI test of the suite pins."""
    lib = _lib.load()
    for name in ('gdml_md_run', 'gdml_md_noise'):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert lib.gdml_abi_version() == 4
    assert C.sizeof(_lib.MDParams) == 96  # the C struct's layout: 8-byte members, two ints padded to 8


def _params(**kw):
    mass = kw.pop('mass', np.ones(3))
    lat = kw.pop('lat', None)
    lat_inv = kw.pop('lat_inv', None)
    d = dict(B=1, N=3, dt=0.01, f_scale=1.0, thermostat=0, gamma=0.0, kT=0.0, seed=0, step0=0)
    d.update(kw)
    p = _lib.MDParams(d['B'], d['N'], d['dt'], _lib._ptr(mass), d['f_scale'], _lib._ptr(lat), _lib._ptr(lat_inv), d['thermostat'],
                      d['gamma'], d['kT'], d['seed'], d['step0'])
    p._keep = (mass, lat, lat_inv)
    return p


def test_argument_errors_need_no_device():
    """Every argument check of gdml_md_run comes before the first use of the context: with ctx = NULL each bad argument
    returns GDML_ERR_INVALID with its own message, and good arguments get as far as the missing context."""
    lib = _lib.load()
    R, V = np.zeros((1, 9)), np.zeros((1, 9))
    eye = np.eye(3)

    def call(p, n_steps=4, record_every=1):
        rc = lib.gdml_md_run(None, C.byref(p), _lib._ptr(R), _lib._ptr(V), n_steps, record_every, None, None, None, None, None,
                             None)
        return rc, lib.gdml_last_error(None).decode()

    assert call(_params()) == (-1, 'gdml_md_run: ctx is NULL')
    assert call(_params(lat=eye, lat_inv=eye)) == (-1, 'gdml_md_run: ctx is NULL')
    bad = [
        (dict(n_steps=-1), {}, 'n_steps'), (dict(record_every=0), {}, 'record_every'),
        ({}, dict(mass=np.array([1.0, 0.0, 1.0])), 'mass'), ({}, dict(mass=np.array([1.0, 1.0, -2.0])), 'mass'),
        ({}, dict(mass=np.array([1.0, np.nan, 1.0])), 'mass'),
        ({}, dict(dt=0.0), 'dt'), ({}, dict(dt=-0.1), 'dt'), ({}, dict(dt=np.nan), 'dt'), ({}, dict(gamma=-1.0), 'gamma'),
        ({}, dict(kT=-1.0), 'kT'), ({}, dict(lat=eye), 'lattice'), ({}, dict(lat_inv=eye), 'lattice'),
        ({}, dict(thermostat=2), 'thermostat'), ({}, dict(thermostat=-1), 'thermostat'), ({}, dict(step0=-1), 'step0'),
        ({}, dict(B=-1), 'B out of range'),
    ]
    for kw_call, kw_par, token in bad:
        rc, msg = call(_params(**kw_par), **kw_call)
        assert rc == -1 and token in msg and 'ctx is NULL' not in msg, (kw_call, kw_par, msg)
    xi = np.zeros((1, 9))
    assert lib.gdml_md_noise(0, -1, 1, 9, _lib._ptr(xi), None) == -1
    assert lib.gdml_md_noise(0, 0, 1, 0, _lib._ptr(xi), None) == -1
    assert lib.gdml_md_noise(0, 0, 1, 9, None, None) == -1
    assert lib.gdml_md_noise(0, 0, 1, 9, _lib._ptr(xi), None) == -1 and 'ctx is NULL' in lib.gdml_last_error(None).decode()

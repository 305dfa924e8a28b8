"""CPU-side checks of the on-device geometry relaxation (gdml_relax_run, csrc/relax.hip; GDMLPredict.relax): the NumPy
restatement (tests/_relax_ref.py) meets the conditions the GPU tests rely on, and the library surface (export, struct layout,
argument errors that need no device)."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _hessian_ref as hr  # noqa: E402
import _md_ref as mr  # noqa: E402
import _relax_ref as rr  # noqa: E402
from sgdml_amd import _lib  # noqa: E402
from sgdml_amd.predict import GDMLPredict  # noqa: E402

FIXTURES = ['n6_p1', 'n5_p4', 'n5_p2_ecstr', 'n10_p2_pbc', 'cfg1_n21_m100', 'cfg3_n42_p27_m60', 'n100_m3', 'n9_p1']
N_EVAL = {'cfg3_n42_p27_m60': 5}
MARGIN = 1e-6  # the predictor's agreed error is 1e-10: four decades keep a branch or the convergence step from flipping


# ---- the restatement on the toy model

@pytest.mark.parametrize('key', sorted(rr.TOY_PARAMS))
def test_toy_model_meets_the_conditions_of_the_gpu_tests(key):
    model, starts, d0, fmax = rr.toy()
    out, dev = rr.toy_reference(key)
    print('%s: steps %s, negative-power events %s, clipped steps %s' % (key, out['n_steps'], out['neg_events'], out['clipped']))
    print('%s: power margin %.2e, threshold margin %.2e, sensitivity of R_end %.2e' % (key, out['power_margin'].min(),
                                                                                       out['fmax_margin'].min(), dev['R_end']))
    assert out['converged'].all() and (out['n_steps'] <= 200).all() and (out['n_steps'] > 0).all()
    assert (out['neg_events'] >= 1).all()
    if key == 'clip':
        assert out['clipped'].sum() >= 1
    else:
        assert out['clipped'].sum() == 0
    assert out['power_margin'].min() >= MARGIN and out['fmax_margin'].min() >= MARGIN
    assert (out['fmax_end'] < fmax).all() and np.isfinite(dev['R_end'])
    # a minimum of the springs: the pair distances came home
    err0, err1 = np.abs(rr.pair_distances(starts) - d0).max(), np.abs(rr.pair_distances(out['R_end']) - d0).max()
    print('%s: pair distances off equilibrium by %.4f at the start, %.4f at the end' % (key, err0, err1))
    assert err1 <= 0.05 * err0
    # and of the model: six soft modes (translations exactly, rotations to the residual force), the seventh positive
    _, _, H = hr.hessian_of_model(model, out['R_end'])
    ratio = 0.0
    for b in range(len(starts)):
        w = np.linalg.eigvalsh(H[b])
        assert w[6] > 0.0
        ratio = max(ratio, np.abs(w[:6]).max() / w[6])
    print('%s: six lowest |eigenvalues| over the seventh: %.2e' % (key, ratio))
    assert ratio <= rr.TOY_NULL_RATIO


@pytest.mark.parametrize('key', sorted(rr.TOY_PARAMS))
def test_energy_falls_between_negative_power_events(key):
    """p > 0 at evaluation t says the last step went downhill to first order; the restated run on the toy model confirms it
    for the energy itself at every evaluation that is no negative-power event."""
    out, _ = rr.toy_reference(key)
    for b in range(out['E_hist'].shape[1]):
        E = out['E_hist'][:out['n_steps'][b] + 1, b]
        up = [t for t in range(1, len(E)) if E[t] > E[t - 1]]
        assert set(up) <= set(out['neg_at'][b]), (b, up, out['neg_at'][b])
        assert E[-1] < E[0]


@pytest.mark.parametrize('name', FIXTURES)
def test_margins_of_the_parity_runs(name):
    """Every (fixture, parameter set) the GPU tests compare step by step: no decision within 1e-6 of its threshold, nothing
    converges, and the run exercises both signs of the power and the growth of dt."""
    n = N_EVAL.get(name, 30)
    _, R0, st, out, dev = rr.parity_reference(name, n)
    print('%s: negative-power events %s, clipped %s, power margin %.2e, threshold margin %.2e' % (
        name, out['neg_events'], out['clipped'], out['power_margin'].min(), out['fmax_margin'].min()))
    print('%s: sensitivities %s' % (name, {k: '%.1e' % v for k, v in dev.items()}))
    assert out['power_margin'].min() >= MARGIN and out['fmax_margin'].min() >= MARGIN
    assert not out['converged'].any() and (out['n_steps'] == n - 1).all()
    assert out['neg_events'].sum() >= 1 and (out['neg_events'] == 0).any()
    assert all(np.isfinite(v) for v in dev.values())
    if n == 30:
        assert (out['state']['dt'] > st['dt']).any()  # n_pos passed n_min


def test_restated_continuation_equals_the_uncut_run():
    model, starts, _, fmax = rr.toy()
    fn = mr.force_fn(model)
    full = rr.run(fn, starts, fmax, max_steps=40, **rr.TOY_PARAMS['clip'])
    a = rr.run(fn, starts, fmax, max_steps=20, **rr.TOY_PARAMS['clip'])
    b = rr.run(fn, a['R_end'], fmax, max_steps=20, state=a['state'], **rr.TOY_PARAMS['clip'])
    assert any(any(t <= 20 for t in ev) for ev in full['neg_at'])  # the cut lies behind a negative-power event
    assert np.array_equal(b['R_end'], full['R_end'])
    for k in ('V', 'dt', 'alpha', 'n_pos', 'n_taken'):
        assert np.array_equal(b['state'][k], full['state'][k]), k
    assert (b['state']['n_taken'] == 40).all() and (b['n_steps'] == 20).all()


# ---- the library surface

def test_library_exports_the_relax_entry():
    lib = _lib.load()
    assert hasattr(lib, 'gdml_relax_run') and 'gdml_relax_run' in _lib.SIGNATURES
    assert lib.gdml_abi_version() == 4
    assert C.sizeof(_lib.RelaxParams) == 104  # 8-byte members, one int padded to 8


def _params(**kw):
    lat, lat_inv = kw.pop('lat', None), kw.pop('lat_inv', None)
    d = dict(B=1, N=3, f_scale=1.0, fmax=0.01, dt_max=1.0, max_step=0.2, f_inc=1.1, f_dec=0.5, alpha_start=0.1, f_alpha=0.99,
             n_min=5)
    d.update(kw)
    p = _lib.RelaxParams(d['B'], d['N'], d['f_scale'], _lib._ptr(lat), _lib._ptr(lat_inv), d['fmax'], d['dt_max'], d['max_step'],
                         d['f_inc'], d['f_dec'], d['alpha_start'], d['f_alpha'], d['n_min'])
    p._keep = (lat, lat_inv)
    return p


def test_argument_errors_need_no_device():
    """Every argument check of gdml_relax_run comes before the first use of the context: with ctx = NULL each bad argument
    returns GDML_ERR_INVALID with its own message, and good arguments get as far as the missing context."""
    lib = _lib.load()
    eye = np.eye(3)

    def call(p, max_steps=4, record_every=0, dt=0.1, with_frames=False, drop=None):
        R, V = np.zeros((1, 9)), np.zeros((1, 9))
        a = dict(dt=np.array([dt]), alpha=np.array([0.1]), n_pos=np.zeros(1, dtype=np.int64), n_taken=np.zeros(1, dtype=np.int64),
                 R_rec=np.zeros((max(max_steps, 0) + 1, 1, 9)) if with_frames else None, E_hist=np.zeros((max(max_steps, 0) + 1, 1)),
                 f_hist=np.zeros((max(max_steps, 0) + 1, 1)), E_end=np.zeros(1), F_end=np.zeros((1, 9)),
                 status=np.zeros((1, 2), dtype=np.int64), bad=np.zeros(1, dtype=np.int64))
        if drop:
            a[drop] = None
        rc = lib.gdml_relax_run(None, C.byref(p), _lib._ptr(R), _lib._ptr(V), _lib._ptr(a['dt']), _lib._ptr(a['alpha']),
                                _lib._ptr(a['n_pos']), _lib._ptr(a['n_taken']), max_steps, record_every, _lib._ptr(a['R_rec']),
                                _lib._ptr(a['E_hist']), _lib._ptr(a['f_hist']), _lib._ptr(a['E_end']), _lib._ptr(a['F_end']),
                                _lib._ptr(a['status']), _lib._ptr(a['bad']))
        return rc, lib.gdml_last_error(None).decode()

    assert call(_params()) == (-1, 'gdml_relax_run: ctx is NULL')
    assert call(_params(lat=eye, lat_inv=eye)) == (-1, 'gdml_relax_run: ctx is NULL')
    assert call(_params(f_inc=1.0, f_alpha=1.0, alpha_start=1.0, n_min=0, dt_max=0.1), max_steps=0) == \
        (-1, 'gdml_relax_run: ctx is NULL')  # the closed ends of the ranges
    assert call(_params(), record_every=1, with_frames=True) == (-1, 'gdml_relax_run: ctx is NULL')
    bad = [
        ({}, dict(fmax=0.0), 'fmax'), ({}, dict(fmax=-1.0), 'fmax'), ({}, dict(fmax=np.nan), 'fmax'), ({}, dict(fmax=np.inf), 'fmax'),
        (dict(max_steps=-1), {}, 'max_steps'), (dict(dt=0.0), {}, 'dt of replica'), (dict(dt=-0.1), {}, 'dt of replica'),
        (dict(dt=np.nan), {}, 'dt of replica'), (dict(dt=0.5), dict(dt_max=0.4), 'dt_max'), ({}, dict(max_step=0.0), 'max_step'),
        ({}, dict(max_step=-0.2), 'max_step'), ({}, dict(f_inc=0.99), 'f_inc'), ({}, dict(f_dec=0.0), 'f_dec'),
        ({}, dict(f_dec=1.0), 'f_dec'), ({}, dict(f_dec=np.nan), 'f_dec'), ({}, dict(alpha_start=0.0), 'alpha_start'),
        ({}, dict(alpha_start=1.1), 'alpha_start'), ({}, dict(f_alpha=0.0), 'f_alpha'), ({}, dict(f_alpha=1.01), 'f_alpha'),
        ({}, dict(n_min=-1), 'n_min'), ({}, dict(lat=eye), 'lattice'), ({}, dict(lat_inv=eye), 'lattice'),
        ({}, dict(B=-1), 'B out of range'), ({}, dict(N=0), 'N out of range'), (dict(record_every=-1), {}, 'record_every'),
        (dict(record_every=0, with_frames=True), {}, 'record_every'), (dict(drop='alpha'), {}, 'state array'),
        (dict(drop='status'), {}, 'output array'),
    ]
    for kw_call, kw_par, token in bad:
        rc, msg = call(_params(**kw_par), **kw_call)
        assert rc == -1 and token in msg and 'ctx is NULL' not in msg, (kw_call, kw_par, msg)
    rc = lib.gdml_relax_run(None, None, None, None, None, None, None, None, 1, 0, None, None, None, None, None, None, None)
    assert rc == -1 and 'params is NULL' in lib.gdml_last_error(None).decode()


class _NoLaunch(object):
    """Stands in for the device context: reaching it means an argument check let a bad call through."""
    model_n_atoms = 6

    def relax_run(self, *a, **kw):
        raise AssertionError('a bad argument reached the device call')


def test_python_argument_checks_come_before_the_device():
    stub = types.SimpleNamespace(n_atoms=6, std=1.0, c=0.0, _ctx=_NoLaunch(), _lat_and_inv=lambda lattice: None)
    R0 = np.zeros((2, 18))
    ok = dict(R0=R0, fmax=0.01)

    def bad(**kw):
        with pytest.raises(ValueError):
            GDMLPredict.relax(stub, **dict(ok, **kw))

    bad(R0=R0[:, :15])
    bad(R0=np.zeros((2, 3, 18)))
    bad(fmax=float('nan'))
    bad(dt_start=float('inf'))
    bad(max_step=float('nan'))
    bad(f_unit=float('nan'))
    bad(max_steps=2.5)
    bad(record_every=0.5)
    bad(state=dict(V=np.zeros((2, 18))))  # incomplete
    st = rr.fresh_state(2, 18)
    bad(state=dict(st, V=np.zeros((1, 18))))
    bad(state=dict(st, dt=np.array([0.1, np.nan])))
    with pytest.raises(AssertionError):  # and a good call gets as far as the device
        GDMLPredict.relax(stub, **ok)
    # the binding's own shape checks
    ctx = types.SimpleNamespace(model_n_atoms=6)
    for key, val in (('dt', np.full(3, 0.1)), ('n_taken', np.zeros(1, dtype=np.int64)), ('V', np.zeros((3, 18)))):
        with pytest.raises(ValueError):
            _lib.Context.relax_run(ctx, R0, 0.01, 10, dict(st, **{key: val}), 1.0)

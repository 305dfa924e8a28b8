"""CPU-side checks of the on-device nudged elastic band (gdml_neb_run, csrc/neb.hip; GDMLPredict.neb): the NumPy restatement
(tests/_neb_ref.py) meets the conditions the GPU tests rely on, and the library surface (export, struct layout, argument
errors) needs no device."""
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
import _neb_ref as nr  # noqa: E402
from sgdml_amd import _lib  # noqa: E402
from sgdml_amd.predict import GDMLPredict  # noqa: E402

MARGIN = 1e-6  # no decision of a run the GPU tests compare lies closer to its threshold (relative)


def _margins(out):
    return out['gap_margin'].min(), out['power_margin'].min(), out['fmax_margin'].min()


# ---- the toy with a barrier

@pytest.mark.parametrize('key', sorted(nr.TOY_RUNS))
def test_toy_runs_converge_with_margins(key):
    """Every toy run of the GPU tests converges on the restatement, every energy comparison of every evaluation has a gap of
    at least 1e-6 max|E'|, the FIRE decisions have relax's margins, and the bands of a key freeze at different evaluations."""
    P, climb, seeds = nr.TOY_RUNS[key]
    path, out, dev = nr.toy_reference(key)
    gap, pm, fm = _margins(out)
    print('%s: steps %s, barrier %s, i_climb %s, gap %.2e, power %.2e, threshold %.2e' % (
        key, out['n_steps'], out['barrier'][:, 0], out['i_climb'], gap, pm, fm))
    print('%s: sensitivities %s' % (key, {k: '%.1e' % v for k, v in dev.items()}))
    assert out['converged'].all() and (out['n_steps'] < nr.TOY_MAX_STEPS).all()
    assert gap >= MARGIN and pm >= MARGIN and fm >= MARGIN
    assert len(set(out['n_steps'].tolist())) == len(seeds)
    assert all(np.isfinite(v) for v in dev.values())
    assert all(len(ev) >= 1 for ev in out['neg_at'])
    # the same saddle whatever P: one barrier (the two end points are mirror images: the same energy)
    assert np.abs(out['barrier'] - nr.TOY_BARRIER).max() <= 2e-6, out['barrier']
    for b in range(len(seeds)):  # E along the band rises to i_climb and falls after it
        E, ic = out['E_end'][b], out['i_climb'][b]
        assert (np.diff(E[:ic + 1]) > 0).all() and (np.diff(E[ic:]) < 0).all()
        assert np.array_equal(out['R_end'][b, [0, -1]], path[b, [0, -1]]) and not out['state']['V'][b, [0, -1]].any()
    assert np.abs(out['s'][:, -1] - np.sqrt(((out['R_end'][:, 1:] - out['R_end'][:, :-1]) ** 2).sum(-1)).sum(-1)).max() < 1e-12


@pytest.mark.parametrize('key', [k for k in sorted(nr.TOY_RUNS) if nr.TOY_RUNS[k][1]])
def test_climbing_image_is_a_first_order_saddle(key):
    """The climbing image's Hessian on the restatement: exactly one negative eigenvalue beyond the null-mode band (six modes
    within TOY_NULL_RATIO of the first positive one)."""
    model = nr.toy()[0]
    _, out, _ = nr.toy_reference(key)
    Rc = out['R_end'][np.arange(len(out['i_climb'])), out['i_climb']]
    _, _, H = hr.hessian_of_model(model, Rc)
    ratio = 0.0
    for b in range(len(Rc)):
        w = np.linalg.eigvalsh(H[b])
        order = np.argsort(np.abs(w))
        null, rest = w[order[:6]], np.sort(w[order[6:]])
        print('%s band %d: negative %.4f, null band %.2e, first positive %.4f' % (key, b, rest[0], np.abs(null).max(), rest[1]))
        assert rest[0] < 0.0 and rest[1] > 0.0
        assert abs(rest[0] - nr.TOY_SADDLE_MODES[0]) < 2e-3 and abs(rest[1] - nr.TOY_SADDLE_MODES[1]) < 2e-3
        ratio = max(ratio, np.abs(null).max() / rest[1])
    assert ratio <= nr.TOY_NULL_RATIO


# ---- step-by-step parity runs

@pytest.mark.parametrize('climb', [False, True])
@pytest.mark.parametrize('name,P,B', nr.PARITY_CASES)
def test_margins_of_the_parity_runs(name, P, B, climb):
    _, path, st, out, dev = nr.parity_reference(name, P, B, climb)
    n = nr.PARITY_N_EVAL.get(name, 30)
    gap, pm, fm = _margins(out)
    print('%s P=%d B=%d climb=%d: gap %.2e, power %.2e, threshold %.2e; %s' % (
        name, P, B, climb, gap, pm, fm, {k: '%.1e' % v for k, v in dev.items()}))
    assert gap >= MARGIN and pm >= MARGIN and fm >= MARGIN
    assert not out['converged'].any() and (out['n_steps'] == n - 1).all()
    assert all(np.isfinite(v) for v in dev.values())
    assert out['R'].shape == (n, B, P, path.shape[2])


def test_parity_runs_cover_both_power_signs_and_a_moving_climbing_image():
    negs = [len(ev) for c in nr.PARITY_CASES for ev in nr.parity_reference(*c, True)[3]['neg_at']]
    assert min(negs) == 0 and max(negs) >= 1
    moved = [len(set(ic)) for c in nr.PARITY_CASES for ic in nr.parity_reference(*c, True)[3]['climb_at']]
    assert max(moved) >= 2


# ---- continuation

def test_restated_continuation_equals_the_uncut_run():
    """n steps plus a continuation against 2 n steps on the P = 8 toy band, across a change of i_climb and a negative-power
    event; and the two-phase use: a band relaxed without climbing, continued with climb."""
    model, _, _, fmax = nr.toy()
    path, ref, _ = nr.toy_reference('p8')
    fn = nr.force_fn(model)
    kw = dict(k_spring=nr.TOY_K, climb=True)
    full = nr.run(fn, path, fmax, max_steps=20, **kw)
    a = nr.run(fn, path, fmax, max_steps=10, **kw)
    b = nr.run(fn, a['R_end'], fmax, max_steps=10, state=a['state'], **kw)
    assert any(t <= 10 for t in full['neg_at'][0]) and len(set(full['climb_at'][0][:11])) >= 2
    assert np.array_equal(b['R_end'], full['R_end'])
    for k in ('V', 'dt', 'alpha', 'n_pos', 'n_taken'):
        assert np.array_equal(b['state'][k], full['state'][k]), k
    assert (b['state']['n_taken'] == 20).all() and (b['n_steps'] == 10).all()
    plain = nr.run(fn, path, fmax, max_steps=30, k_spring=nr.TOY_K, climb=False)
    two = nr.run(fn, plain['R_end'], fmax, max_steps=nr.TOY_MAX_STEPS, state=plain['state'], **kw)
    assert two['converged'][0] and abs(two['barrier'][0, 0] - nr.TOY_BARRIER) <= 2e-6


# ---- the library surface

def test_library_exports_the_neb_entry():
    lib = _lib.load()
    assert hasattr(lib, 'gdml_neb_run') and 'gdml_neb_run' in _lib.SIGNATURES
    assert lib.gdml_abi_version() == 4
    assert C.sizeof(_lib.NebParams) == 120 and C.sizeof(_lib.RelaxParams) == 104
    assert _lib.NebParams.k_spring.offset == 104 and _lib.NebParams.climb.offset == 112 and _lib.NebParams.P.offset == 12


def _params(**kw):
    lat, lat_inv = kw.pop('lat', None), kw.pop('lat_inv', None)
    d = dict(B=1, N=3, P=4, f_scale=1.0, fmax=0.01, dt_max=1.0, max_step=0.2, f_inc=1.1, f_dec=0.5, alpha_start=0.1,
             f_alpha=0.99, n_min=5, k_spring=0.5, climb=1)
    d.update(kw)
    p = _lib.NebParams(d['B'], d['N'], d['P'], d['f_scale'], _lib._ptr(lat), _lib._ptr(lat_inv), d['fmax'], d['dt_max'],
                       d['max_step'], d['f_inc'], d['f_dec'], d['alpha_start'], d['f_alpha'], d['n_min'], d['k_spring'], d['climb'])
    p._keep = (lat, lat_inv)
    return p


def test_argument_errors_need_no_device():
    """Every argument check of gdml_neb_run comes before the first use of the context: with ctx = NULL each bad argument returns
    GDML_ERR_INVALID with its own message, and good arguments get as far as the missing context."""
    lib = _lib.load()
    eye = np.eye(3)

    def call(p, max_steps=4, record_every=0, dt=0.1, with_frames=False, drop=None):
        P = max(int(p.P), 1)
        R, V = np.zeros((1, P, 9)), np.zeros((1, P, 9))
        n = max(max_steps, 0) + 1
        a = dict(dt=np.array([dt]), alpha=np.array([0.1]), n_pos=np.zeros(1, dtype=np.int64), n_taken=np.zeros(1, dtype=np.int64),
                 R_rec=np.zeros((n, 1, P, 9)) if with_frames else None, E_hist=np.zeros((n, 1)), f_hist=np.zeros((n, 1)),
                 E_end=np.zeros((1, P)), F_end=np.zeros((1, P, 9)), i_climb=np.zeros(1, dtype=np.int64), s=np.zeros((1, P)),
                 f_tan=np.zeros((1, P)), status=np.zeros((1, 2), dtype=np.int64), bad=np.zeros(1, dtype=np.int64))
        if drop:
            a[drop] = None
        rc = lib.gdml_neb_run(None, C.byref(p), _lib._ptr(R), _lib._ptr(V), _lib._ptr(a['dt']), _lib._ptr(a['alpha']),
                              _lib._ptr(a['n_pos']), _lib._ptr(a['n_taken']), max_steps, record_every, _lib._ptr(a['R_rec']),
                              _lib._ptr(a['E_hist']), _lib._ptr(a['f_hist']), _lib._ptr(a['E_end']), _lib._ptr(a['F_end']),
                              _lib._ptr(a['i_climb']), _lib._ptr(a['s']), _lib._ptr(a['f_tan']), _lib._ptr(a['status']),
                              _lib._ptr(a['bad']))
        return rc, lib.gdml_last_error(None).decode()

    assert call(_params()) == (-1, 'gdml_neb_run: ctx is NULL')
    assert call(_params(lat=eye, lat_inv=eye, climb=0)) == (-1, 'gdml_neb_run: ctx is NULL')
    assert call(_params(P=3, f_inc=1.0, f_alpha=1.0, alpha_start=1.0, n_min=0, dt_max=0.1), max_steps=0) == \
        (-1, 'gdml_neb_run: ctx is NULL')  # the closed ends of the ranges
    assert call(_params(P=128), record_every=1, with_frames=True) == (-1, 'gdml_neb_run: ctx is NULL')
    bad = [
        ({}, dict(fmax=0.0), 'fmax'), ({}, dict(fmax=np.nan), 'fmax'), ({}, dict(fmax=np.inf), 'fmax'),
        (dict(max_steps=-1), {}, 'max_steps'), (dict(dt=0.0), {}, 'dt of replica'), (dict(dt=np.nan), {}, 'dt of replica'),
        (dict(dt=0.5), dict(dt_max=0.4), 'dt_max'), ({}, dict(max_step=0.0), 'max_step'), ({}, dict(f_inc=0.99), 'f_inc'),
        ({}, dict(f_dec=0.0), 'f_dec'), ({}, dict(f_dec=1.0), 'f_dec'), ({}, dict(alpha_start=0.0), 'alpha_start'),
        ({}, dict(alpha_start=1.1), 'alpha_start'), ({}, dict(f_alpha=0.0), 'f_alpha'), ({}, dict(f_alpha=1.01), 'f_alpha'),
        ({}, dict(n_min=-1), 'n_min'), ({}, dict(lat=eye), 'lattice'), ({}, dict(lat_inv=eye), 'lattice'),
        ({}, dict(B=-1), 'B out of range'), ({}, dict(N=0), 'N out of range'), (dict(record_every=-1), {}, 'record_every'),
        (dict(record_every=0, with_frames=True), {}, 'record_every'), (dict(drop='alpha'), {}, 'state array'),
        (dict(drop='status'), {}, 'output array'), (dict(drop='s'), {}, 'output array'), (dict(drop='i_climb'), {}, 'output array'),
        (dict(drop='f_tan'), {}, 'output array'), ({}, dict(P=2), 'P outside'), ({}, dict(P=129), 'P outside'),
        ({}, dict(P=0), 'P outside'), ({}, dict(k_spring=0.0), 'k_spring'), ({}, dict(k_spring=-0.5), 'k_spring'),
        ({}, dict(k_spring=np.nan), 'k_spring'), ({}, dict(k_spring=np.inf), 'k_spring'),
    ]
    for kw_call, kw_par, token in bad:
        rc, msg = call(_params(**kw_par), **kw_call)
        assert rc == -1 and msg.startswith('gdml_neb_run: ') and token in msg and 'ctx is NULL' not in msg, (kw_call, kw_par, msg)
    # B P >= 2^31 (no array of that size is touched before the check)
    p = _params(B=2 ** 25, P=64)
    z = np.zeros(1)
    zi = np.zeros(1, dtype=np.int64)
    rc = lib.gdml_neb_run(None, C.byref(p), _lib._ptr(z), _lib._ptr(z), _lib._ptr(z), _lib._ptr(z), _lib._ptr(zi), _lib._ptr(zi),
                          4, 0, None, _lib._ptr(z), _lib._ptr(z), _lib._ptr(z), _lib._ptr(z), _lib._ptr(zi), _lib._ptr(z),
                          _lib._ptr(z), _lib._ptr(zi), None)
    assert rc == -1 and 'B P out of range' in lib.gdml_last_error(None).decode()
    rc = lib.gdml_neb_run(None, None, None, None, None, None, None, None, 1, 0, None, None, None, None, None, None, None, None,
                          None, None)
    assert rc == -1 and 'params is NULL' in lib.gdml_last_error(None).decode()


class _NoLaunch(object):
    """Stands in for the device context: reaching it means an argument check let a bad call through."""
    model_n_atoms = 5

    def neb_run(self, *a, **kw):
        raise AssertionError('a bad argument reached the device call')


def test_python_argument_checks_come_before_the_device():
    stub = types.SimpleNamespace(n_atoms=5, std=1.0, c=0.0, _ctx=_NoLaunch(), _lat_and_inv=lambda lattice: None)
    Rp = np.zeros((2, 4, 15))
    ok = dict(R_path=Rp, fmax=0.01, k_spring=0.5)

    def bad(**kw):
        with pytest.raises(ValueError):
            GDMLPredict.neb(stub, **dict(ok, **kw))

    bad(R_path=Rp[:, :, :12])
    bad(R_path=np.zeros(15))
    bad(R_path=np.zeros((2, 2, 4, 15)))
    bad(R_path=Rp[:, :2])  # two images: no interior
    bad(R_path=np.zeros((1, 129, 15)))
    bad(fmax=float('nan'))
    bad(k_spring=float('nan'))
    bad(k_spring=0.0)
    bad(k_spring=-1.0)
    bad(dt_start=float('inf'))
    bad(max_step=float('nan'))
    bad(f_unit=float('nan'))
    bad(max_steps=2.5)
    bad(record_every=0.5)
    bad(state=dict(V=np.zeros((2, 4, 15))))  # incomplete
    st = nr.fresh_state(2, 4, 15)
    bad(state=dict(st, V=np.zeros((2, 3, 15))))
    bad(state=dict(st, dt=np.array([0.1, np.nan])))
    with pytest.raises(AssertionError):  # and a good call gets as far as the device
        GDMLPredict.neb(stub, **ok)
    with pytest.raises(AssertionError):  # a single band as (P, 3N)
        GDMLPredict.neb(stub, **dict(ok, R_path=Rp[0]))
    # the binding's own shape checks
    ctx = types.SimpleNamespace(model_n_atoms=5)
    for key, val in (('dt', np.full(3, 0.1)), ('n_taken', np.zeros(1, dtype=np.int64)), ('V', np.zeros((3, 4, 15)))):
        with pytest.raises(ValueError):
            _lib.Context.neb_run(ctx, Rp, 0.01, 0.5, 10, dict(st, **{key: val}), 1.0)
    with pytest.raises(ValueError):
        _lib.Context.neb_run(ctx, Rp[0], 0.01, 0.5, 10, st, 1.0)


def test_interpolate_path():
    A, Bm = np.arange(15.0), np.arange(15.0)[::-1] * 0.3
    path = GDMLPredict.interpolate_path(A, Bm, 5)
    assert path.shape == (1, 5, 15) and np.array_equal(path[0, 0], A) and np.array_equal(path[0, -1], Bm)
    assert np.allclose(path[0, 2], 0.5 * (A + Bm)) and np.allclose(np.diff(path[0], axis=0), (Bm - A) / 4.0)
    two = GDMLPredict.interpolate_path(np.stack([A, Bm]), np.stack([Bm, A]), 3)
    assert two.shape == (2, 3, 15) and np.array_equal(two, nr.interpolate(np.stack([A, Bm]), np.stack([Bm, A]), 3))
    assert GDMLPredict.interpolate_path(A.reshape(1, 5, 3), Bm.reshape(1, 5, 3), 4).shape == (1, 4, 15)
    for bad in (dict(n_images=1), dict(n_images=2.5), dict(R_b=Bm[:12])):
        with pytest.raises(ValueError):
            GDMLPredict.interpolate_path(**dict(dict(R_a=A, R_b=Bm, n_images=4), **bad))

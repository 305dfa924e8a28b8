"""CPU-side checks of the eigenvector-following search (gdml_ef_run, csrc/ef.hip; GDMLPredict.stationary_point): the NumPy
restatement (tests/_ef_ref.py) on the toy models of the band and relaxation tests, the margins of every decision of every run the
GPU test compares, and the argument errors of the C entry and of stationary_point() that need no device."""
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _ef_ref as er  # noqa: E402
import _hessian_ref as hr  # noqa: E402
import _md_ref as mr  # noqa: E402
import _neb_ref as nr  # noqa: E402
import _relax_ref as rr  # noqa: E402
import _vib_ref as vr  # noqa: E402
from sgdml_amd import _lib  # noqa: E402
from sgdml_amd._lib import EfParams  # noqa: E402,F401  (the binding of gdml_ef_run: this file tests nothing without it)
from sgdml_amd.predict import GDMLPredict  # noqa: E402

# the spread of the barrier over the band toy's runs at the band's fmax, as tests/test_neb_cpu.py records it
BARRIER_SPREAD = (0.0476037, 0.0476058)


def _print_margins(what, out):
    m = out['margins']
    print('%s: smallest margins rho %.2e, clip %.2e, fmax %.2e, floor %.2e, overlap %.2e' % (
        what, m['rho'].min(), m['clip'].min(), m['fmax'].min(), m['floor'].min(), m['overlap'].min()))


def _reach(f_atom, w_soft, n_atoms):
    """How far a geometry whose largest atomic force is f_atom can lie from its stationary point, to first order: the gradient
    norm is at most sqrt(N) f_atom, the displacement that over the softest curvature |w_soft|; a pair distance changes by at
    most twice the displacement, the energy by at most |g|^2 / (2 |w_soft|).  Returns (energy, pair distance) bounds; the
    tests allow twice as much for the higher orders."""
    g = np.sqrt(n_atoms) * f_atom
    return 2.0 * g * g / (2.0 * abs(w_soft)), 2.0 * 2.0 * g / abs(w_soft)


def _same_point(out, ref_R, ref_E, ref_f, model):
    """Energy and pair distances of the searches' end points against reference geometries whose largest atomic force is ref_f."""
    n_atoms = out['R_end'].shape[1] // 3
    w_soft = np.abs(out['w_end'][:, :3 * n_atoms - 6]).min()
    dE, dd = _reach(max(ref_f, out['fmax_end'].max()), w_soft, n_atoms)
    dE += 1e-10 * np.abs(ref_E - model['c']).max()  # the agreed accuracy of an energy
    got_E, got_d = np.abs(out['E_end'] - ref_E).max(), np.abs(rr.pair_distances(out['R_end']) - rr.pair_distances(ref_R)).max()
    print('   against the reference point: energy %.2e (bound %.2e), pair distances %.2e (bound %.2e)' % (got_E, dE, got_d, dd))
    assert got_E <= dE and got_d <= dd


def _barrier(model, E_saddle):
    _, A, Bm, _ = nr.toy()
    E_ends, _, _ = hr.hessian_of_model(model, np.stack([A, Bm]))
    return E_saddle - E_ends


# ---- the search on the toys

def test_saddle_from_the_jittered_midpoint():
    """Converges to 1e-9 of the starting force in five steps (quadratically at the end), to the band toy's barrier, with one
    negative eigenvalue and six null modes."""
    model, R0, _, _, fmax = er.toy_case('saddle_mid')
    out, dev = er.toy_reference('saddle_mid')
    bar = _barrier(model, out['E_end'][0])
    print('saddle from the midpoint: %d steps, f_atom %.2e (fmax %.2e), barrier %.8f / %.8f, w %.5f / %.5f, f_atom history %s' % (
        out['n_steps'][0], out['fmax_end'][0], fmax, bar[0], bar[1], out['w_end'][0, 0], out['w_end'][0, 1],
        ' '.join('%.1e' % f for f in out['fmax_hist'][:, 0])))
    assert out['converged'].all() and out['n_steps'][0] == 5
    assert BARRIER_SPREAD[0] <= bar[0] <= BARRIER_SPREAD[1] and BARRIER_SPREAD[0] <= bar[1] <= BARRIER_SPREAD[1]
    assert abs(bar[0] - nr.TOY_BARRIER) < 1e-6
    assert out['n_neg'][0] == 1 and out['n_rigid'][0] == 6 and not out['w_end'][0, 9:].any()
    assert abs(out['w_end'][0, 0] - nr.TOY_SADDLE_MODES[0]) < 1e-3 and abs(out['w_end'][0, 1] - nr.TOY_SADDLE_MODES[1]) < 1e-3
    # quadratic at the end: the last two force ratios shrink faster than the ones before
    f = out['fmax_hist'][:, 0]
    assert f[-1] / f[-2] < 1e-3 and f[-2] / f[-3] < 1e-1
    # unprojected, the six rigid modes are null modes at a saddle converged this far (they were not at the band's fmax)
    _, _, H = hr.hessian_of_model(model, out['R_end'])
    raw = np.linalg.eigvalsh(H[0])
    null = np.sort(np.abs(raw))[:6]
    print('raw null band %.2e of the first positive eigenvalue' % (null.max() / out['w_end'][0, 1]))
    assert null.max() <= 1e-6 * out['w_end'][0, 1]
    assert np.array_equal(out['mode_end'][0], vr.jacobi(vr.shifted(H[0], out['R_end'][0], np.ones(5))[0])[1][0])


def test_saddle_from_the_line_with_a_follow_vector():
    """From 0.3 along the line between the minima, following the line direction: the same saddle.  The Hessian there has two
    negative eigenvalues at the first two evaluations; the mode along the line is the lowest one throughout, so the followed
    index never leaves 0 on this start -- test_followed_index_changes uses a start where it does."""
    model = er.toy_case('saddle_line')[0]
    out, _ = er.toy_reference('saddle_line')
    mid, _ = er.toy_reference('saddle_mid')
    print('saddle from the line: %d steps, f_atom %.2e, followed index %s, w_follow %s' % (
        out['n_steps'][0], out['fmax_end'][0], out['k_follow_hist'][:, 0].tolist(), out['w_follow_hist'][:, 0].round(4).tolist()))
    assert out['converged'].all() and out['n_steps'][0] == 6 and out['n_neg'][0] == 1
    _same_point(out, mid['R_end'], mid['E_end'], mid['fmax_end'][0], model)
    _, _, H = hr.hessian_of_model(model, out['R'][:2, 0])
    for n in range(2):
        w = er.spectrum(H[n], out['R'][n, 0], 1.0, 2)[0]
        assert (w[:9] < 0.0).sum() == 2, (n, w[:3])
    assert not out['k_follow_hist'].any()


def test_followed_index_changes():
    """A start nearer the minimum, off the line: the mode along the line direction is the second lowest at the first two
    evaluations and the lowest afterwards; the search tracks it to the same saddle, and the trust radius changes on the way."""
    out, _ = er.toy_reference('saddle_track')
    mid, _ = er.toy_reference('saddle_mid')
    k = out['k_follow_hist'][:, 0]
    print('tracking start: %d steps, followed index %s, trust %s' % (out['n_steps'][0], k.tolist(), out['trust_hist'][:, 0].tolist()))
    assert out['converged'].all() and out['n_neg'][0] == 1
    assert k[0] == 1 and k[-1] == 0
    assert len(set(out['trust_hist'][:, 0].tolist())) > 1
    _same_point(out, mid['R_end'], mid['E_end'], mid['fmax_end'][0], er.toy_case('saddle_track')[0])
    # without the follow vector the search maximises the lowest mode from the start: another path
    model, R0, _, _, fmax = er.toy_case('saddle_track')
    plain = er.run(er.hessian_fn(model), R0, fmax, order=1, max_steps=er.TOY_MAX_STEPS)
    assert not np.array_equal(plain['R'][1], out['R'][1])


def test_minimum_from_the_line():
    """order = 0 from the same start: the energy drops to the minimum's and the lowest eigenvalue turns positive."""
    model, A, _, _ = nr.toy()
    out, _ = er.toy_reference('min_line')
    E_A, _, _ = hr.hessian_of_model(model, A[None])
    print('minimum from the line: %d steps, f_atom %.2e, E %.10f (FIRE minimum %.10f), lowest w %s' % (
        out['n_steps'][0], out['fmax_end'][0], out['E_end'][0], E_A[0], out['w_follow_hist'][:, 0].round(4).tolist()))
    assert out['converged'].all() and out['n_steps'][0] == 7 and out['n_neg'][0] == 0
    assert out['w_follow_hist'][0, 0] < 0.0 < out['w_follow_hist'][-1, 0] and (out['w_end'][0, :9] > 0.0).all()
    dE = np.diff(out['E_hist'][:, 0])  # drops at every step, down to the accuracy of an energy
    assert (dE < 1e-10 * np.abs(out['E_hist']).max()).all() and (dE[:-2] < 0.0).all()
    # FIRE stopped at 1e-6 of its starting force: the energies agree to second order in its residual, the distances to first
    _, F_A = mr.force_fn(model)(A[None])
    _same_point(out, A[None], E_A, np.sqrt((F_A.reshape(-1, 3) ** 2).sum(-1)).max(), model)
    assert not out['mode_end'].any()


def test_minima_of_the_relaxation_toy():
    """The seven starts of the relaxation toy: the energies and pair distances of FIRE's minima (positions need not agree: the
    projection removes the rotation FIRE picks up), in 5 to 7 steps instead of FIRE's 68 to 125 evaluations."""
    out, _ = er.toy_reference('min_relax')
    fire, _ = rr.toy_reference('free')
    print('relaxation toy: steps %s (FIRE %s), f_atom %s' % (out['n_steps'].tolist(), fire['n_steps'].tolist(),
                                                              ' '.join('%.1e' % f for f in out['fmax_end'])))
    assert out['converged'].all() and (out['n_neg'] == 0).all() and (out['n_rigid'] == 6).all()
    assert (out['n_steps'] <= 8).all() and (fire['n_steps'] >= 8 * out['n_steps']).all()
    _same_point(out, fire['R_end'], fire['E_end'], fire['fmax_end'].max(), rr.toy()[0])
    assert (out['w_end'][:, :12] > 0.0).all() and not out['w_end'][:, 12:].any()


def test_continuation_of_the_restatement():
    """n steps and a continuation against the uncut run, across the change of the followed index and a trust change."""
    model, R0, follow, order, fmax = er.toy_case('saddle_track')
    whole, _ = er.toy_reference('saddle_track')
    first = er.run(er.hessian_fn(model), R0, fmax, order=order, follow=follow, max_steps=2)
    assert first['n_steps'][0] == 2 and not first['converged'].any()
    rest = er.run(er.hessian_fn(model), first['R_end'], fmax, order=order, state=first['state'], max_steps=er.TOY_MAX_STEPS)
    assert np.array_equal(rest['R_end'], whole['R_end']) and rest['n_steps'][0] == whole['n_steps'][0] - 2
    assert np.array_equal(np.concatenate([first['E_hist'][:2], rest['E_hist']]), whole['E_hist'])
    assert np.array_equal(np.concatenate([first['k_follow_hist'][:2], rest['k_follow_hist']]), whole['k_follow_hist'])


# ---- the margins of every decision the GPU test compares

@pytest.mark.parametrize('key', sorted(er.TOY_RUNS))
def test_margins_of_the_toy_runs(key):
    out, dev = er.toy_reference(key)
    _print_margins(key, out)
    print('%s: deviation under noise %s' % (key, ', '.join('%s %.1e' % kv for kv in sorted(dev.items()))))
    assert er.smallest_margin(out) > er.MARGIN_MIN
    assert all(np.isfinite(v) for v in dev.values())


@pytest.mark.parametrize('name', er.PARITY_FIXTURES)
def test_margins_of_the_parity_runs(name):
    """No decision of a parity run within MARGIN_MIN of its threshold (a start that had one would be replaced in
    _ef_ref.PARITY_STARTS, not the margin); the noisy twin takes the same decisions, so the bounds are finite."""
    for order, with_follow in er.PARITY_MODES:
        _, _, _, out, dev = er.parity_reference(name, order, with_follow)
        _print_margins('%s order %d follow %d' % (name, order, with_follow), out)
        print('   trust %s, followed index %s' % (out['trust_hist'].T.tolist(), out['k_follow_hist'].T.tolist()))
        print('   deviation under noise %s' % ', '.join('%s %.1e' % kv for kv in sorted(dev.items())))
        assert er.smallest_margin(out) > er.MARGIN_MIN
        assert all(np.isfinite(v) for v in dev.values())
        assert not out['converged'].any() and (out['n_steps'] == er.PARITY_N_EVAL - 1).all()


def test_lapack_stands_in_for_the_jacobi_iteration_on_the_largest_fixture():
    """_ef_ref.eigensolve takes LAPACK beyond JACOBI_MAX_N: on n100_m3 the two solvers agree far below the noise that defines
    the bounds."""
    model, R0, _ = er.parity_start('n100_m3')
    _, _, H = hr.hessian_of_model(model, R0[:1])
    D_s = vr.shifted(H[0], R0[0], np.ones(100), project=2)[0]
    assert D_s.shape[0] > er.JACOBI_MAX_N
    w_j, V_j, sweeps = vr.jacobi(D_s)
    w_l, V_l, _ = er.eigensolve(D_s)
    gap = np.diff(w_l[:294]).min()
    print('n100_m3: |D_s|_F %.1f, smallest gap %.2e, eigenvalues differ by %.1e, eigenvectors by %.1e (%d sweeps)' % (
        np.linalg.norm(D_s), gap, np.abs(w_j - w_l).max(), np.abs(V_j[:294] - V_l[:294]).max(), sweeps))
    assert np.abs(w_j - w_l).max() <= vr.bound(300, D_s)
    assert np.abs(V_j[:294] - V_l[:294]).max() <= 100.0 * vr.bound(300, D_s) / gap
    assert np.abs(V_j[:294] - V_l[:294]).max() < 1e-9


# ---- the library surface

def test_struct_layout_and_exports():
    lib = _lib.load()
    assert C.sizeof(_lib.EfParams) == 72
    P = _lib.EfParams
    assert [(P.B.offset, P.N.offset, P.order.offset, P.f_scale.offset, P.lat.offset, P.lat_inv.offset, P.fmax.offset,
             P.trust_min.offset, P.trust_max.offset, P.project.offset)] == [(0, 8, 12, 16, 24, 32, 40, 48, 56, 64)]
    assert hasattr(lib, 'gdml_ef_run') and lib.gdml_abi_version() == 4
    # the pinned sizes of the structs that were there before
    assert [C.sizeof(s) for s in (_lib.RelaxParams, _lib.VibParams)] == [104, 48]


def _ef_call(lib, R, null=(), t=None, trust=None, flags=None, E_prev=None, dE_pred=None, max_steps=3, record_every=0, **kw):
    par = dict(B=R.shape[0] if R is not None else 1, N=2, order=1, f_scale=1.0, lat=None, lat_inv=None, fmax=1e-3, trust_min=1e-4,
               trust_max=0.3, project=2)
    par.update(kw)
    keep = [par['lat'], par['lat_inv']]
    prm = _lib.EfParams(par['B'], par['N'], par['order'], par['f_scale'], _lib._ptr(keep[0]), _lib._ptr(keep[1]), par['fmax'],
                        par['trust_min'], par['trust_max'], par['project'])
    B, n3 = max(par['B'], 1), 3 * max(par['N'], 1)
    a = dict(R=R, trust=np.full(B, 0.1) if trust is None else trust, E_prev=np.zeros(B) if E_prev is None else E_prev,
             dE_pred=np.zeros(B) if dE_pred is None else dE_pred, flags=np.zeros(B, dtype=np.int64) if flags is None else flags,
             t=t, R_rec=None, E_hist=np.zeros((max(max_steps, 0) + 1, B)), fmax_hist=np.zeros((max(max_steps, 0) + 1, B)),
             w_follow_hist=np.zeros((max(max_steps, 0) + 1, B)), k_follow_hist=None, E_end=np.zeros(B), F_end=np.zeros((B, n3)),
             w_end=np.zeros((B, n3)), n_rigid=np.zeros(B, dtype=np.int64), n_neg=np.zeros(B, dtype=np.int64),
             mode_end=np.zeros((B, n3)), status=np.zeros((B, 2), dtype=np.int64), first_bad_step=None)
    for k in null:
        a[k] = None
    p = _lib._ptr
    rc = lib.gdml_ef_run(None, C.byref(prm), p(a['R']), p(a['trust']), p(a['E_prev']), p(a['dE_pred']), p(a['flags']), p(a['t']),
                         max_steps, record_every, p(a['R_rec']), p(a['E_hist']), p(a['fmax_hist']), p(a['w_follow_hist']),
                         p(a['k_follow_hist']), p(a['E_end']), p(a['F_end']), p(a['w_end']), p(a['n_rigid']), p(a['n_neg']),
                         p(a['mode_end']), p(a['status']), p(a['first_bad_step']))
    return rc, lib.gdml_last_error(None).decode()


def test_ef_argument_checks_without_a_context():
    lib = _lib.load()
    R, eye = np.arange(12.0).reshape(2, 6), np.eye(3)
    ok = (-1, 'gdml_ef_run: ctx is NULL')  # every argument is fine: only the context is missing
    assert _ef_call(lib, R) == ok
    assert _ef_call(lib, R, order=0) == ok
    assert _ef_call(lib, R, t=np.ones((2, 6))) == ok
    assert _ef_call(lib, R, project=1, lat=eye, lat_inv=eye) == ok
    assert _ef_call(lib, R, project=0, B=0) == ok
    assert _ef_call(lib, R, max_steps=0) == ok
    assert _ef_call(lib, R, trust=np.array([1e-4, 0.3]), flags=np.array([3, 1]), E_prev=np.ones(2), dE_pred=-np.ones(2)) == ok
    bad = [
        (dict(fmax=0.0), 'fmax'), (dict(fmax=-1.0), 'fmax'), (dict(fmax=np.nan), 'fmax'), (dict(fmax=np.inf), 'fmax'),
        (dict(max_steps=-1), 'max_steps'), (dict(order=2), 'order'), (dict(order=-1), 'order'),
        (dict(trust_min=0.0), 'trust_min'), (dict(trust_min=-1.0), 'trust_min'), (dict(trust_min=np.nan), 'trust_min'),
        (dict(trust_max=1e-5), 'trust_max'), (dict(trust_max=np.inf), 'trust_max'), (dict(trust_max=np.nan), 'trust_max'),
        (dict(trust=np.array([0.1, 0.31])), 'trust of geometry 1'), (dict(trust=np.array([1e-5, 0.1])), 'trust of geometry 0'),
        (dict(trust=np.array([0.1, np.nan])), 'trust of geometry 1'),
        (dict(project=2, lat=eye, lat_inv=eye), 'project = 2 with a lattice'), (dict(project=3), 'project'), (dict(project=-1), 'project'),
        (dict(lat=eye), 'lattice'), (dict(lat_inv=eye), 'lattice'),
        (dict(order=0, t=np.ones((2, 6))), 'follow vector with order = 0'),
        (dict(f_scale=0.0), 'f_scale'), (dict(f_scale=-1.0), 'f_scale'), (dict(f_scale=np.nan), 'f_scale'),
        (dict(B=-1), 'B out of range'), (dict(N=0), 'N out of range'), (dict(record_every=-1), 'record_every'),
        (dict(flags=np.array([0, 4])), 'flags of geometry 1'), (dict(flags=np.array([-1, 0])), 'flags of geometry 0'),
        (dict(flags=np.array([1, 0]), E_prev=np.array([np.nan, 0.0])), 'E_prev or dE_pred of geometry 0'),
        (dict(flags=np.array([0, 3]), dE_pred=np.array([0.0, np.inf])), 'E_prev or dE_pred of geometry 1'),
    ]
    for kw, token in bad:
        rc, msg = _ef_call(lib, R, **kw)
        assert rc == -1 and token in msg and msg.startswith('gdml_ef_run') and 'ctx is NULL' not in msg, (kw, msg)
    for val in (np.nan, np.inf):
        Rb, tb = R.copy(), np.ones((2, 6))
        Rb[1, 4], tb[0, 2] = val, val
        rc, msg = _ef_call(lib, Rb)
        assert rc == -1 and 'coordinate 4 of geometry 1' in msg, msg
        rc, msg = _ef_call(lib, R, t=tb)
        assert rc == -1 and 'follow vector entry 2 of geometry 0' in msg, msg
    for name in ('R', 'trust', 'E_prev', 'dE_pred', 'flags', 'E_hist', 'fmax_hist', 'w_follow_hist', 'E_end', 'F_end', 'w_end',
                 'n_rigid', 'n_neg', 'mode_end', 'status'):
        rc, msg = _ef_call(lib, R, null=(name,))
        assert rc == -1 and 'NULL' in msg and 'ctx is NULL' not in msg, (name, msg)
    rc = lib.gdml_ef_run(None, None, *([None] * 6), 0, 0, *([None] * 13))
    assert rc == -1 and 'params is NULL' in lib.gdml_last_error(None).decode()
    # beyond the Hessian's limit: unsupported, and said before the context is looked at
    rc, msg = _ef_call(lib, np.zeros((1, 3 * 198)), N=198)
    assert rc == _lib.ERR_UNSUPPORTED and '197' in msg, msg
    assert _ef_call(lib, np.zeros((1, 3 * 197)), N=197) == ok


class _NoLaunch(object):
    """Stands in for the device context: reaching it means an argument check let a bad call through."""
    model_n_atoms = 6

    def ef_run(self, *a, **kw):
        raise AssertionError('a bad argument reached the device call')


def test_python_argument_checks_come_before_the_device():
    ctx = _NoLaunch()
    lat = (np.eye(3) * 9.0, np.eye(3) / 9.0)

    def stub(lat_and_inv=None):
        return types.SimpleNamespace(n_atoms=6, std=1.0, c=0.0, _ctx=ctx, _lat_and_inv=lambda lattice: lat_and_inv,
                                     _VIB_PROJECT=GDMLPredict._VIB_PROJECT)

    R = np.zeros((2, 18))
    state = er.fresh_state(2)

    def bad(s=None, **kw):
        a = dict(R0=R, fmax=1e-3)
        a.update(kw)
        with pytest.raises(ValueError):
            GDMLPredict.stationary_point(s or stub(), **a)

    bad(R0=R[:, :15])
    bad(R0=np.zeros((2, 3, 18)))
    for val in (np.nan, np.inf):
        Rb, tb = R.copy(), np.ones((2, 18))
        Rb[1, 3], tb[0, 1] = val, val
        bad(R0=Rb)
        bad(follow=tb)
        for name in ('fmax', 'trust_start', 'trust_max', 'trust_min', 'f_unit'):
            bad(**{name: val})
    bad(fmax=0.0)
    bad(fmax=-1.0)
    bad(f_unit=0.0)
    bad(order=2)
    bad(order='saddle')
    bad(max_steps=-1)
    bad(max_steps=2.5)
    bad(record_every=-1)
    bad(trust_min=0.0)
    bad(trust_start=0.5)
    bad(trust_start=1e-5)
    bad(trust_max=0.05)
    bad(project='rotations')
    bad(project=2)
    bad(stub(lat), project='rigid')
    bad(order=0, follow=np.ones((2, 18)))
    bad(follow=np.ones((2, 15)))
    bad(follow=np.ones((3, 18)))
    bad(follow=np.concatenate([np.ones((1, 18)), np.zeros((1, 18))]))
    bad(state={k: v for k, v in state.items() if k != 'flags'})
    bad(state=state, follow=np.ones((2, 18)))
    bad(state=dict(state, t=np.ones((2, 18))), order=0)
    bad(state=dict(state, t=np.ones((2, 15))))
    bad(state=dict(state, trust=np.full(3, 0.1)))
    bad(state=dict(state, trust=np.array([0.1, 0.5])))
    bad(state=dict(state, E_prev=np.array([0.0, np.nan])))
    # what passes the checks reaches the device call
    for s, kw in ((stub(), {}), (stub(lat), {}), (stub(lat), dict(project='trans')), (stub(lat), dict(project='none')),
                  (stub(), dict(project='rigid', order=0)), (stub(), dict(follow=np.ones((2, 18)))), (stub(), dict(state=state)),
                  (stub(), dict(state=dict(state, t=np.ones((2, 18)))))):
        with pytest.raises(AssertionError):
            GDMLPredict.stationary_point(s, R, 1e-3, **kw)
    # the binding's own shape checks
    ns = types.SimpleNamespace(model_n_atoms=6)
    with pytest.raises(ValueError):
        _lib.Context.ef_run(ns, R, 1e-3, 3, dict(state, trust=np.full(3, 0.1)))
    with pytest.raises(ValueError):
        _lib.Context.ef_run(ns, R, 1e-3, 3, dict(state, t=np.ones((2, 15))))

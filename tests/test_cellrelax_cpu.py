"""CPU-side checks of the on-device variable-cell relaxation (gdml_cell_relax_run, csrc/cellrelax.hip;
GDMLPredict.relax_cell): the NumPy restatement (tests/_cellrelax_ref.py) is the gradient of the enthalpy and meets the conditions
the GPU tests rely on, and the library surface (struct layout, argument errors that need no device)."""
import ctypes as C
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

MARGIN = 1e-6  # as tests/test_relax_cpu.py: four decades above the predictor's agreed error


# ---- the restated generalised force is minus the gradient of the enthalpy

@pytest.mark.parametrize('name', ['n4_p6_pbc', 'n10_p2_pbc'])
def test_generalised_force_is_minus_the_gradient_of_the_enthalpy(name):
    """mask = 1, pressure 0.01, the sheared Fd of the parity tests, f_unit = 1.3: G against 4-point central differences in every
    one of the 3N + 9 coordinates of H = f_unit E + pressure Vol.  No minimum-image integer changes inside the stencil (asserted
    from the rounded L^-1 (r_i - r_j)), so H is smooth there.  The bound is the difference formula's rounding error, (3 / 2)
    delta |H| / h with delta the relative noise of one restated energy: 1e-13 (a few hundred roundings) for n10_p2_pbc with
    h = 1e-4; 1e-10 for the ill-conditioned n4_p6_pbc (tests/test_stress_gpu.py: reordering its training points alone moves
    the outputs by 8e-11), hence h = 1e-3 there.  The truncation error h^4 H^(5) / 30 is below both."""
    model, st, cf = cr.parity_case(name)
    vf = cr.model_virial_fn(model)
    u0 = cr.join(st['S'][:1], st['C'][:1])
    L0 = st['L0'][:1]
    p, f_unit = cr.PARITY_PRESSURE, 1.3
    h, delta = {'n4_p6_pbc': (1e-3, 1e-10), 'n10_p2_pbc': (1e-4, 1e-13)}[name]
    _, G, _, r0, lat0 = cr.gen_force(vf, u0, L0, cf, p, None, f_unit)
    ints0, margin = cr.image_integers(r0, lat0)
    n = u0.shape[1]
    G_fd = np.zeros(n)
    for k in range(n):
        e = []
        for s in (2.0, 1.0, -1.0, -2.0):
            u = u0.copy()
            u[0, k] += s * h
            r, lat = cr.cartesian(u, L0, cf)[:2]
            ints, m = cr.image_integers(r, lat)
            assert np.array_equal(ints, ints0), (k, s)
            margin = min(margin, m)
            e.append(cr.enthalpy(vf, u, L0, cf, p, f_unit)[0])
        G_fd[k] = -(-e[0] + 8.0 * e[1] - 8.0 * e[2] + e[3]) / (12.0 * h)
    err = np.abs(G[0] - G_fd).max()
    bound = 1.5 * delta * abs(cr.enthalpy(vf, u0, L0, cf, p, f_unit)[0]) / h
    print('%s: |G + grad H| = %.2e (cell rows %.2e), bound %.2e, max|G| = %.2e, image margin %.4f' %
          (name, err, np.abs(G[0, -9:] - G_fd[-9:]).max(), bound, np.abs(G[0]).max(), margin))
    assert margin > 0.0 and err <= bound and bound <= 1e-5 * np.abs(G[0]).max()  # (the bound resolves G to five digits)


def test_mask_zeroes_components_and_adjugate_inverse():
    model, st, cf = cr.parity_case('n10_p2_pbc')
    vf = cr.model_virial_fn(model)
    u0, L0 = cr.join(st['S'][:2], st['C'][:2]), st['L0'][:2]
    G1 = cr.gen_force(vf, u0, L0, cf, 0.01)[1]
    G0 = cr.gen_force(vf, u0, L0, cf, 0.01, np.zeros((3, 3)))[1]
    assert not G0[:, -9:].any() and np.array_equal(G0[:, :-9], G1[:, :-9]) and G1[:, -9:].all()
    M = np.array([[5.6, 0.4, 0.0], [0.0, 5.2, 0.3], [0.2, 0.0, 6.4]])
    assert np.abs(cr.inv3(M) @ M - np.eye(3)).max() <= 4 * np.finfo(float).eps
    assert abs(cr.adj_det(M)[1] - np.linalg.det(M)) <= 1e-13 * abs(np.linalg.det(M))


# ---- the periodic toy

def _hessian(vf, u, L0, pressure, h=1e-5):
    """Hessian of H in u by central differences of the restated G (one geometry)."""
    n = u.shape[1]
    H = np.zeros((n, n))
    for k in range(n):
        e = np.zeros((1, n))
        e[0, k] = h
        H[k] = -(cr.gen_force(vf, u + e, L0, 6.0, pressure)[1][0] - cr.gen_force(vf, u - e, L0, 6.0, pressure)[1][0]) / (2 * h)
    return 0.5 * (H + H.T)


def test_toy_is_periodic_along_all_three_cell_vectors():
    model, starts, L_starts, d0, fmax = cr.toy()
    ints, margin = cr.image_integers(starts, L_starts)
    wraps = [int((np.abs(ints[..., a]) > 0).sum()) for a in range(3)]
    print('wrapped pairs along the cell vectors %s of %d, image margin %.3f' % (wraps, 7 * 15, margin))
    assert min(wraps) >= 7 and margin >= 0.05  # at least one wrapped pair per start and axis, none near a jump
    strain = np.array([np.linalg.solve(cr.TOY_LATTICE.T, L.T).T - np.eye(3) for L in L_starts])
    assert 0.01 <= np.abs(strain).max() <= 0.045 and (np.abs(strain[:, 0, 1]) > 0).all()


def test_toy_hessian_has_exactly_six_null_modes_at_the_relaxed_state():
    """The Hessian of H in u at the restated end state: six near-null modes (three translations of s exactly, three rotations of
    Fd to the residual force), the seventh eigenvalue positive and separated by _relax_ref.TOY_NULL_RATIO.
    This holds for the relaxed state under the tension TOY_PRESSURE only.  At pressure 0 the relaxed springs carry no load, the
    Hessian is J^T (d2E/dx2) J with J the (15, 27) Jacobian of the D = 15 descriptor entries, so its rank is at most 15 and
    3N + 9 - 15 = 12 modes are null whatever the placement of six atoms (measured: twelve eigenvalues below 1e-3, the
    thirteenth 9e-2); six null modes would need D >= 3N + 3, i.e. N >= 8.  Under tension every spring is stretched and the
    second derivatives of the pair distances stiffen the six floppy modes (measured at -0.004: six lowest |w| <= 6e-5, the
    seventh 2.3e-2)."""
    model, starts, L_starts, d0, fmax = cr.toy()
    vf = cr.model_virial_fn(model)
    out, _ = cr.toy_reference(cr.TOY_PRESSURE)
    ratio = 0.0
    for b in (0, 3, 6):
        w = np.linalg.eigvalsh(_hessian(vf, out['u_end'][b:b + 1], out['state']['L0'][b:b + 1], cr.TOY_PRESSURE))
        print('start %d under tension: lowest eigenvalues %s' % (b, np.array2string(w[:8], precision=2)))
        assert w[6] > 0.0
        ratio = max(ratio, np.abs(w[:6]).max() / w[6])
    print('six lowest |eigenvalues| over the seventh: %.2e' % ratio)
    assert ratio <= rr.TOY_NULL_RATIO
    out0, _ = cr.toy_reference(0.0)
    w = np.linalg.eigvalsh(_hessian(vf, out0['u_end'][:1], out0['state']['L0'][:1], 0.0))
    print('pressure 0: lowest eigenvalues %s' % np.array2string(w[:14], precision=2))
    assert np.abs(w[:12]).max() <= 0.05 * w[12]  # the rank bound: twelve, not six


@pytest.mark.parametrize('pressure', [0.0, cr.TOY_PRESSURE])
def test_toy_meets_the_conditions_of_the_gpu_tests(pressure):
    model, starts, L_starts, d0, fmax = cr.toy()
    out, dev = cr.toy_reference(pressure)
    print('p = %g: steps %s, negative-power events %s, clipped %s' % (pressure, out['n_steps'], out['neg_events'], out['clipped']))
    print('p = %g: power margin %.2e, threshold margin %.2e, sensitivity of R_end %.2e, of the metric %.2e' %
          (pressure, out['power_margin'].min(), out['fmax_margin'].min(), dev['R_end'], dev['metric_end']))
    assert out['converged'].all() and (out['n_steps'] <= 400).all() and (out['n_steps'] > 0).all()
    assert out['power_margin'].min() >= MARGIN and out['fmax_margin'].min() >= MARGIN
    assert (out['fmax_end'] < fmax).all() and all(np.isfinite(v) for v in dev.values())
    ints0, _ = cr.image_integers(starts, L_starts)
    ints1, margin = cr.image_integers(out['R_end'], out['lattice_end'])
    assert np.array_equal(ints0, ints1) and margin >= 0.05
    # the generalised force of the end state, entry by entry: max |T Fd^-T| / cell_factor < fmax
    vf = cr.model_virial_fn(model)
    G = cr.gen_force(vf, out['u_end'], out['state']['L0'], 6.0, pressure)[1]
    assert np.abs(G[:, -9:]).max() < fmax
    err0 = np.abs(cr.pair_distances(starts, L_starts) - d0).max()
    err1 = np.abs(cr.pair_distances(out['R_end'], out['lattice_end']) - d0).max()
    print('p = %g: pair distances off rest by %.4f at the start, %.4f at the end; volumes %s' %
          (pressure, err0, err1, np.array2string(out['vol_end'], precision=2)))
    if pressure == 0.0:
        # the model's own error: the exact springs relaxed the same way end within fmax of rest, the model (force error
        # 1e-2 of the start's forces) within a few 1e-3; 5 % of the start's deviation, as tests/test_relax_cpu.py asks
        assert err1 <= 0.05 * err0
    else:
        assert (out['vol_end'] > np.abs(np.linalg.det(cr.TOY_LATTICE))).all()  # tension: the cell has grown


# ---- the library surface

def _params(**kw):
    d = dict(B=1, N=3, f_scale=1.0, fmax=0.01, dt_max=1.0, max_step=0.2, f_inc=1.1, f_dec=0.5, alpha_start=0.1, f_alpha=0.99,
             n_min=5, pressure=0.0, cell_factor=3.0)
    mask = kw.pop('mask', None)
    d.update(kw)
    p = _lib.CellRelaxParams(d['B'], d['N'], d['f_scale'], d['fmax'], d['dt_max'], d['max_step'], d['f_inc'], d['f_dec'],
                             d['alpha_start'], d['f_alpha'], d['n_min'], d['pressure'], d['cell_factor'], _lib._ptr(mask))
    p._keep = mask
    return p


def test_struct_layout():
    assert C.sizeof(_lib.CellRelaxParams) == 112


def test_argument_errors_need_no_context():
    """Every argument check of gdml_cell_relax_run comes before the first use of the context: with ctx = NULL each bad argument
    is reported as itself, and a good call as 'ctx is NULL'."""
    lib = _lib.load()

    def call(p, max_steps=4, record_every=0, dt=0.1, frames=False, drop=None, L0=None, Cc=None):
        n = max(max_steps, 0) + 1
        a = dict(S=np.zeros((1, 9)), Cc=3.0 * np.eye(3)[None] if Cc is None else Cc, L0=5.0 * np.eye(3)[None] if L0 is None else L0,
                 V=np.zeros((1, 18)), dt=np.array([dt]), alpha=np.array([0.1]), n_pos=np.zeros(1, dtype=np.int64),
                 n_taken=np.zeros(1, dtype=np.int64), R_rec=np.zeros((n, 1, 9)) if frames else None,
                 lat_rec=np.zeros((n, 1, 9)) if frames else None, E_hist=np.zeros((n, 1)), vol_hist=np.zeros((n, 1)),
                 fmax_hist=np.zeros((n, 1)), R_end=np.zeros((1, 9)), lat_end=np.zeros((1, 9)), E_end=np.zeros(1),
                 F_end=np.zeros((1, 9)), W_end=np.zeros((1, 9)), vol_end=np.zeros(1), status=np.zeros((1, 2), dtype=np.int64),
                 bad=np.zeros(1, dtype=np.int64))
        a = {k: (None if v is None else np.ascontiguousarray(v)) for k, v in a.items()}
        if drop:
            a[drop] = None
        q = _lib._ptr
        rc = lib.gdml_cell_relax_run(None, C.byref(p), q(a['S']), q(a['Cc']), q(a['L0']), q(a['V']), q(a['dt']), q(a['alpha']),
                                     q(a['n_pos']), q(a['n_taken']), max_steps, record_every, q(a['R_rec']), q(a['lat_rec']),
                                     q(a['E_hist']), q(a['vol_hist']), q(a['fmax_hist']), q(a['R_end']), q(a['lat_end']),
                                     q(a['E_end']), q(a['F_end']), q(a['W_end']), q(a['vol_end']), q(a['status']), q(a['bad']))
        return rc, lib.gdml_last_error(None).decode()

    ok = (-1, 'gdml_cell_relax_run: ctx is NULL')
    slab = np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 0.0], [0.0, 0.0, 0.0]])
    assert call(_params()) == ok
    assert call(_params(mask=slab, pressure=-2.5)) == ok
    assert call(_params(), record_every=1, frames=True) == ok
    singular = np.array([[[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]]])
    nan = np.full((1, 3, 3), np.nan)
    bad_mask = np.ones((3, 3))
    bad_mask[0, 1] = 0.0  # not symmetric
    cases = [
        (dict(), dict(fmax=0.0), 'fmax'), (dict(), dict(fmax=float('nan')), 'fmax'), (dict(max_steps=-1), dict(), 'max_steps'),
        (dict(dt=0.0), dict(), 'dt of replica'), (dict(dt=2.0), dict(), 'dt_max'), (dict(), dict(max_step=0.0), 'max_step'),
        (dict(), dict(f_inc=0.9), 'f_inc'), (dict(), dict(f_dec=1.0), 'f_dec'), (dict(), dict(alpha_start=0.0), 'alpha_start'),
        (dict(), dict(f_alpha=1.5), 'f_alpha'), (dict(), dict(n_min=-1), 'n_min'), (dict(record_every=-1), dict(), 'record_every'),
        (dict(record_every=0, frames=True), dict(), 'record_every'), (dict(), dict(N=0), 'N out of range'),
        (dict(), dict(B=-1), 'B out of range'), (dict(), dict(f_scale=float('inf')), 'f_scale'),
        (dict(drop='S'), dict(), 'state array'), (dict(drop='V'), dict(), 'state array'),
        (dict(drop='E_hist'), dict(), 'output array'), (dict(drop='status'), dict(), 'output array'),
        # what a cell relaxation adds
        (dict(drop='L0'), dict(), 'needs a lattice per geometry'), (dict(drop='Cc'), dict(), 'Cc is NULL'),
        (dict(drop='vol_hist'), dict(), 'output array'), (dict(drop='lat_end'), dict(), 'output array'),
        (dict(drop='W_end'), dict(), 'output array'),
        (dict(L0=singular), dict(), 'L0 of geometry 0'), (dict(L0=nan), dict(), 'L0 of geometry 0'),
        (dict(Cc=singular), dict(), 'C of geometry 0'), (dict(Cc=nan), dict(), 'C of geometry 0'),
        (dict(Cc=np.zeros((1, 3, 3))), dict(), 'C of geometry 0'),
        (dict(), dict(mask=0.5 * np.ones((3, 3))), 'mask'), (dict(), dict(mask=bad_mask), 'mask'),
        (dict(), dict(mask=np.full((3, 3), np.nan)), 'mask'),
        (dict(), dict(cell_factor=0.0), 'cell_factor'), (dict(), dict(cell_factor=-3.0), 'cell_factor'),
        (dict(), dict(cell_factor=float('inf')), 'cell_factor'), (dict(), dict(pressure=float('nan')), 'pressure'),
        (dict(), dict(pressure=float('inf')), 'pressure'),
    ]
    for kw_call, kw_par, token in cases:
        rc, msg = call(_params(**kw_par), **kw_call)
        assert rc == -1 and token in msg and 'ctx is NULL' not in msg, (kw_call, kw_par, msg)
    rc = lib.gdml_cell_relax_run(None, None, *([None] * 8), 1, 0, *([None] * 13))
    assert rc == -1 and 'params is NULL' in lib.gdml_last_error(None).decode()

"""CPU-side checks of the harmonic vibrational analysis (gdml_vib_run, csrc/vib.hip; gdml_sym_eig, csrc/sym_eig.hip; GDMLPredict.vibrations): the
NumPy restatement (tests/_vib_ref.py) against LAPACK and on the toy models of the relaxation and band tests, the margins of the
rank rule, the two host helpers, and the argument errors of the C entries and of vibrations() that need no device."""
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
import _relax_ref as rr  # noqa: E402
import _vib_ref as vr  # noqa: E402
from sgdml_amd import _lib  # noqa: E402
from sgdml_amd._lib import VibParams  # noqa: E402,F401  (the binding of gdml_vib_run: this file tests nothing without it)
from sgdml_amd.predict import GDMLPredict  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
FIXTURES = ['n6_p1', 'n5_p4', 'n9_p1', 'n10_p2_pbc', 'cfg1_n21_m100', 'cfg3_n42_p27_m60', 'n100_m3']
# the imaginary mode of the band toy's climbing image against the band tangent there, as measured on the restatement
# (test_band_toy_saddle prints it): 0.98 or more on every run
OVERLAP_MIN = 0.9


def fixture_geoms(name):
    g = dict(np.load(os.path.join(GOLDEN, name + '.npz')))
    Rt = g['R_test'].reshape(len(g['R_test']), -1)
    return g, np.concatenate([Rt[:6], g['R_train'][:1].reshape(1, -1)])


# ---- the eigensolver's restatement

@pytest.mark.parametrize('n', [1, 2, 3, 7, 64])
def test_jacobi_restatement_against_lapack(n):
    rs = np.random.RandomState(100 + n)
    for trial in range(3):
        A = rs.standard_normal((n, n))
        A = A + A.T
        w, V, sweeps = vr.jacobi(A)
        dw, res, orth = vr.eig_errors(A, w, V)
        b = vr.bound(n, A)
        print('n = %d: sweeps %d, eigenvalues %.2e, residual %.2e, orthogonality %.2e, bound %.2e (|A|_F = %.2e)' % (
            n, sweeps, dw, res, orth, b, np.linalg.norm(A)))
        assert sweeps <= vr.MAX_SWEEPS and (np.diff(w) >= 0.0).all() and vr.sign_convention_holds(V)
        assert dw <= b and res <= b
        assert orth <= 40.0 * n * vr.EPS  # unit vectors: the bound relative to 1
    # a diagonal matrix takes no sweep; the zero matrix neither
    assert vr.jacobi(np.diag(np.arange(1.0, n + 1.0)))[2] == 0
    assert vr.jacobi(np.zeros((n, n)))[2] == 0


def test_conventions_of_order_and_sign():
    w, V = vr.order_and_sign(np.array([2.0, -1.0, 2.0]), np.array([[0.6, 0.0, -0.8], [0.0, -1.0, 0.0], [-0.8, 0.0, -0.6]]))
    assert np.array_equal(w, [-1.0, 2.0, 2.0])
    # column 1 first; the tie 2.0 keeps columns 0, 2 in order; largest component positive, the first one on ties
    assert np.array_equal(V, [[0.0, 1.0, 0.0], [-0.6, 0.0, 0.8], [0.8, 0.0, 0.6]])
    w, V = vr.order_and_sign(np.array([1.0]), np.array([[-1.0]]))
    assert np.array_equal(V, [[1.0]])
    _, V = vr.order_and_sign(np.array([0.0, 1.0]), np.array([[-0.5, 0.5], [0.5, 0.5]]) * np.sqrt(2.0))
    assert V[0, 0] > 0.0 and V[0, 1] < 0.0  # a tie of magnitudes: the lower index decides


# ---- physics on the toys

def _toy_minima():
    model, starts, _, _ = rr.toy()
    out, _ = rr.toy_reference('free')
    return model, out['R_end']


def test_relaxation_toy_minimum():
    """Six rigid modes and only positive vibrations at every restated minimum; unprojected, the six lowest eigenvalues stay
    within the ratio the relaxation test asserts."""
    model, R = _toy_minima()
    _, _, H = hr.hessian_of_model(model, R)
    m = np.ones(6)
    for b in range(len(R)):
        v = vr.vibrations(H[b], R[b], m)
        vib = v['w2'][:18 - v['n_rigid']]
        assert v['n_rigid'] == 6 and v['n_neg'] == 0 and (vib > 0.0).all(), (b, vib)
        assert not v['w2'][12:].any()
        raw = np.linalg.eigvalsh(vr.mass_weight(H[b], m))
        ratio = np.abs(raw[:6]).max() / raw[6]
        print('minimum %d: softest vibration %.4f (raw seventh %.4f), raw null band %.2e of it, tau %.1e' % (
            b, vib[0], raw[6], ratio, v['tau']))
        assert ratio <= rr.TOY_NULL_RATIO
        assert abs(vib[0] - raw[6]) <= 10 * rr.TOY_NULL_RATIO * raw[6]


@pytest.mark.parametrize('key', ['p4', 'p8'])
def test_band_toy_saddle(key):
    """Exactly one imaginary mode at the restated climbing image, far beyond tau, along the band; none at the two minima."""
    model, A, Bm, _ = nr.toy()
    _, out, _ = nr.toy_reference(key)
    m = np.ones(5)
    for b in range(len(out['i_climb'])):
        ic = int(out['i_climb'][b])
        Rc = out['R_end'][b, ic]
        _, _, H = hr.hessian_of_model(model, Rc[None])
        v = vr.vibrations(H[0], Rc, m)
        vib = v['w2'][:15 - v['n_rigid']]
        assert v['n_rigid'] == 6 and v['n_neg'] == 1 and (vib < 0.0).sum() == 1
        assert -vib[0] > 100.0 * v['tau']
        raw = np.linalg.eigvalsh(vr.mass_weight(H[0], m))
        order = np.argsort(np.abs(raw))
        null, rest = raw[order[:6]], np.sort(raw[order[6:]])
        assert np.abs(null).max() / rest[1] <= nr.TOY_NULL_RATIO
        t = vr.band_tangent(out['R_end'][b], out['E_end'][b], ic)
        overlap = abs(v['modes'][0] @ t)
        print('%s band %d: imaginary w2 %.4f (tau %.1e), first real %.4f, overlap with the tangent %.4f' % (
            key, b, vib[0], v['tau'], vib[1], overlap))
        assert overlap > OVERLAP_MIN
    ends = np.stack([A, Bm])
    _, _, H = hr.hessian_of_model(model, ends)
    for e in range(2):
        v = vr.vibrations(H[e], ends[e], m)
        assert v['n_rigid'] == 6 and v['n_neg'] == 0 and (v['w2'][:9] > 0.0).all()


# ---- the rank rule

def test_collinear_geometry_has_five_rigid_modes():
    rs = np.random.RandomState(5)
    H = rs.standard_normal((15, 15))
    for bent, k in ((False, 5), (True, 6)):
        R, m = vr.collinear(bent)
        v = vr.vibrations(H + H.T, R, m)
        assert v['n_rigid'] == k and not v['w2'][15 - k:].any()
        assert (np.abs(v['w2'][:15 - k]) < v['Lambda']).all()
        # the rigid rows are eigenvectors at Lambda: D_s Q^T = Lambda Q^T
        assert np.abs(v['D_s'] @ v['Q'].T - v['Lambda'] * v['Q'].T).max() <= 40 * 15 * vr.EPS * np.linalg.norm(v['D_s'])
    R1, m1 = np.array([0.3, -1.0, 2.0]), np.array([12.0])
    assert vr.vibrations(np.diag([1.0, 2.0, 3.0]), R1, m1)['n_rigid'] == 3
    assert vr.vibrations(H + H.T, vr.collinear()[0], vr.collinear()[1], project=1)['n_rigid'] == 3
    assert vr.vibrations(H + H.T, vr.collinear()[0], vr.collinear()[1], project=0)['n_rigid'] == 0


def test_rank_rule_margins():
    """No decision of the rank rule sits within 1e3 of its threshold 1e-10: every remainder ratio of every geometry the tests
    use lies below 1e-13 or above 1e-7."""
    geoms = [('collinear',) + vr.collinear(), ('bent',) + vr.collinear(True), ('atom', np.array([0.3, -1.0, 2.0]), np.array([12.0]))]
    for b, R in enumerate(_toy_minima()[1]):
        geoms.append(('relax toy %d' % b, R, np.ones(6)))
    _, A, Bm, _ = nr.toy()
    out = nr.toy_reference('p4')[1]
    geoms += [('band A', A, np.ones(5)), ('band B', Bm, np.ones(5)),
              ('band saddle', out['R_end'][0, int(out['i_climb'][0])], np.ones(5))]
    for name in FIXTURES:
        if name == 'n10_p2_pbc':
            continue  # periodic: translations only, which are orthogonal by construction (checked below)
        _, R7 = fixture_geoms(name)
        for q, R in enumerate(R7):
            geoms.append(('%s %d' % (name, q), R, vr.fixture_masses(len(R) // 3)))
    lo, hi = 0.0, np.inf
    for name, R, m in geoms:
        _, ratios = vr.rigid_basis(R, m, 2)
        small = ratios[~(ratios > 1e-7)]
        small = small[~np.isnan(small)]
        if small.size:
            lo = max(lo, small.max())
        if (ratios > 1e-7).any():
            hi = min(hi, ratios[ratios > 1e-7].min())
        assert ((ratios < 1e-13) | (ratios > 1e-7) | np.isnan(ratios)).all(), (name, ratios)
    print('rank rule: largest dropped ratio %.1e, smallest kept ratio %.1e (threshold %.0e)' % (lo, hi, vr.RANK_TOL))
    _, R7 = fixture_geoms('n10_p2_pbc')
    _, ratios = vr.rigid_basis(R7[0], vr.fixture_masses(10), 1)
    assert (ratios > 1e-7).all()


# ---- the host helpers

def test_harmonic_thermo_against_level_sums():
    rs = np.random.RandomState(2)
    w2 = rs.uniform(0.2, 4.0, (3, 6)) ** 2
    hbar = 0.7
    e = hbar * np.sqrt(w2)
    n = np.arange(2000)[:, None, None]
    for kT in (0.3, 1.0, 5.0):
        lv = e[None] * (n + 0.5)  # levels of every oscillator
        wts = np.exp(-(lv - lv[0]) / kT)
        Z = wts.sum(axis=0)
        F_ref = (lv[0] - kT * np.log(Z)).sum(axis=-1)
        U_ref = ((lv * wts).sum(axis=0) / Z).sum(axis=-1)
        t = GDMLPredict.harmonic_thermo(w2, kT, hbar)
        assert np.allclose(t['zpe'], 0.5 * e.sum(-1), rtol=1e-14)
        assert np.allclose(t['F_vib'], F_ref, rtol=1e-12) and np.allclose(t['U_vib'], U_ref, rtol=1e-12)
        assert np.allclose(t['S_vib'], (U_ref - F_ref) / kT, rtol=1e-10)
    # classical limit kT >> hbar w: U -> kT per mode, F -> kT sum ln(hbar w / kT)
    t = GDMLPredict.harmonic_thermo(w2, 1e4, hbar)
    assert np.allclose(t['U_vib'], 6 * 1e4, rtol=1e-6)
    assert np.allclose(t['F_vib'], 1e4 * np.log(e / 1e4).sum(-1), rtol=1e-6)
    # kT -> 0: the zero-point energy alone
    for kT in (0.0, 1e-6):
        t = GDMLPredict.harmonic_thermo(w2, kT, hbar)
        assert np.allclose(t['F_vib'], t['zpe'], rtol=1e-14) and np.allclose(t['U_vib'], t['zpe'], rtol=1e-14)
        assert np.abs(t['S_vib']).max() <= 1e-12
    for bad in (dict(w2_vib=[1.0, -1e-9], kT=1.0, hbar=1.0), dict(w2_vib=[1.0, np.nan], kT=1.0, hbar=1.0),
                dict(w2_vib=[1.0], kT=-1.0, hbar=1.0), dict(w2_vib=[1.0], kT=1.0, hbar=0.0)):
        with pytest.raises(ValueError):
            GDMLPredict.harmonic_thermo(**bad)


def test_htst_prefactor_against_the_product():
    w_min = np.array([0.5, 1.1, 2.0, 3.3, 0.9])
    w_sad = np.array([0.7, 1.0, 2.5, 3.0])
    w2_sad = np.concatenate([[-0.4], w_sad ** 2])
    nu = GDMLPredict.htst_prefactor(w_min ** 2, w2_sad)
    assert np.isclose(nu, np.prod(w_min) / np.prod(w_sad) / (2 * np.pi), rtol=1e-14)
    # 600 modes of magnitude 1e3: the plain products overflow, the logarithms do not
    big = np.full(600, 1e6)
    assert np.isclose(GDMLPredict.htst_prefactor(big, np.concatenate([[-1.0], big[1:]])), 1e3 / (2 * np.pi), rtol=1e-10)
    for a, b in ((w_min ** 2, w_sad ** 2), (w_min ** 2, np.concatenate([[-0.4, -0.1], w_sad[:3] ** 2])),
                 (w_min ** 2, w2_sad[:4]), (np.concatenate([[-1.0], w_min[1:] ** 2]), w2_sad),
                 (w_min ** 2, np.concatenate([[-0.4, 0.0], w_sad[:3] ** 2]))):
        with pytest.raises(ValueError):
            GDMLPredict.htst_prefactor(a, b)


# ---- the library surface

def test_struct_layout_and_exports():
    lib = _lib.load()
    assert C.sizeof(_lib.VibParams) == 48
    assert [(_lib.VibParams.B.offset, _lib.VibParams.N.offset, _lib.VibParams.h_scale.offset, _lib.VibParams.lat.offset,
             _lib.VibParams.lat_inv.offset, _lib.VibParams.project.offset)] == [(0, 8, 16, 24, 32, 40)]
    for name in ('gdml_sym_eig', 'gdml_sym_eig_dev', 'gdml_vib_run'):
        assert hasattr(lib, name)


def test_sym_eig_argument_checks_without_a_context():
    lib = _lib.load()
    A, w = np.eye(3)[None].copy(), np.zeros((1, 3))

    def call(fn, A_=A, M=1, n=3, w_=w):
        rc = fn(None, _lib._ptr(A_), M, n, _lib._ptr(w_), None, None)
        return rc, lib.gdml_last_error(None).decode()

    for fn, name in ((lib.gdml_sym_eig, 'gdml_sym_eig'), (lib.gdml_sym_eig_dev, 'gdml_sym_eig_dev')):
        assert call(fn) == (-1, name + ': ctx is NULL')  # every argument is fine: only the context is missing
        assert call(fn, M=0) == (-1, name + ': ctx is NULL')
        assert call(fn, n=591) == (-1, name + ': ctx is NULL')
        for kw, token in ((dict(M=-1), 'M < 0'), (dict(n=0), 'n = 0'), (dict(n=-3), 'n = -3'), (dict(n=592), 'n = 592'),
                          (dict(A_=None), 'NULL'), (dict(w_=None), 'NULL'), (dict(M=2 ** 62 // 9), '2^62'),
                          (dict(M=2 ** 62), '2^62')):
            rc, msg = call(fn, **kw)
            assert rc == -1 and token in msg and msg.startswith(name) and 'ctx is NULL' not in msg, (kw, msg)
        assert call(fn, M=2 ** 62 // 9 - 1)[1] == name + ': ctx is NULL'  # M n n = 2^62 - 9: allowed as far as this check goes


def _vib_call(lib, R, masses, out=True, **kw):
    par = dict(B=R.shape[0] if R is not None else 1, N=2, h_scale=1.0, lat=None, lat_inv=None, project=2)
    par.update(kw)
    keep = [par['lat'], par['lat_inv']]
    prm = _lib.VibParams(par['B'], par['N'], par['h_scale'], _lib._ptr(keep[0]), _lib._ptr(keep[1]), par['project'])
    B, n3 = max(par['B'], 1), 3 * max(par['N'], 1)
    w2, nr_, nn_ = np.zeros((B, n3)), np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    rc = lib.gdml_vib_run(None, C.byref(prm), _lib._ptr(R), _lib._ptr(masses), _lib._ptr(w2) if out else None, None,
                          _lib._ptr(nr_), _lib._ptr(nn_), None, None, None)
    return rc, lib.gdml_last_error(None).decode()


def test_vib_argument_checks_without_a_context():
    lib = _lib.load()
    R, m, eye = np.arange(12.0).reshape(2, 6), np.array([1.0, 12.0]), np.eye(3)
    assert _vib_call(lib, R, m) == (-1, 'gdml_vib_run: ctx is NULL')
    assert _vib_call(lib, R, m, project=1, lat=eye, lat_inv=eye) == (-1, 'gdml_vib_run: ctx is NULL')
    assert _vib_call(lib, R, m, project=0, B=0) == (-1, 'gdml_vib_run: ctx is NULL')
    bad = [
        (dict(project=2, lat=eye, lat_inv=eye), 'project = 2 with a lattice'), (dict(project=3), 'project'), (dict(project=-1), 'project'),
        (dict(lat=eye), 'lattice'), (dict(lat_inv=eye), 'lattice'),
        (dict(h_scale=0.0), 'h_scale'), (dict(h_scale=-1.0), 'h_scale'), (dict(h_scale=np.nan), 'h_scale'), (dict(h_scale=np.inf), 'h_scale'),
        (dict(B=-1), 'B out of range'), (dict(N=0), 'N out of range'),
    ]
    for kw, token in bad:
        rc, msg = _vib_call(lib, R, m, **kw)
        assert rc == -1 and token in msg and 'ctx is NULL' not in msg, (kw, msg)
    for mm in (np.array([1.0, 0.0]), np.array([-1.0, 1.0]), np.array([1.0, np.nan]), np.array([np.inf, 1.0])):
        rc, msg = _vib_call(lib, R, mm)
        assert rc == -1 and 'mass of atom' in msg, msg
    for val in (np.nan, np.inf):
        Rb = R.copy()
        Rb[1, 4] = val
        rc, msg = _vib_call(lib, Rb, m)
        assert rc == -1 and 'coordinate 4 of geometry 1' in msg, msg
    for kw in (dict(R=None), dict(masses=None), dict(out=False)):
        a = dict(R=R, masses=m)
        a.update(kw)
        rc, msg = _vib_call(lib, **a)
        assert rc == -1 and 'NULL' in msg and 'ctx is NULL' not in msg, (kw, msg)
    rc = lib.gdml_vib_run(None, None, None, None, None, None, None, None, None, None, None)
    assert rc == -1 and 'params is NULL' in lib.gdml_last_error(None).decode()
    # beyond the Hessian's limit: unsupported, and said before the context is looked at
    R198, m198 = np.zeros((1, 3 * 198)), np.ones(198)
    rc, msg = _vib_call(lib, R198, m198, N=198)
    assert rc == _lib.ERR_UNSUPPORTED and '197' in msg, msg
    assert _vib_call(lib, np.zeros((1, 3 * 197)), np.ones(197), N=197) == (-1, 'gdml_vib_run: ctx is NULL')


class _NoLaunch(object):
    """Stands in for the device context: reaching it means an argument check let a bad call through."""
    model_n_atoms = 6

    def vib_run(self, *a, **kw):
        raise AssertionError('a bad argument reached the device call')


def test_python_argument_checks_come_before_the_device():
    ctx = _NoLaunch()
    lat = (np.eye(3) * 9.0, np.eye(3) / 9.0)

    def stub(lat_and_inv=None):
        return types.SimpleNamespace(n_atoms=6, std=1.0, c=0.0, _ctx=ctx, _lat_and_inv=lambda lattice: lat_and_inv,
                                     _VIB_PROJECT=GDMLPredict._VIB_PROJECT, _min_shard_hessian=4,
                                     _sharded=lambda n, fn, min_shard=None: [fn(ctx, 0, n)])

    R, m = np.zeros((2, 18)), np.ones(6)

    def bad(s=None, **kw):
        a = dict(R=R, masses=m)
        a.update(kw)
        with pytest.raises(ValueError):
            GDMLPredict.vibrations(s or stub(), **a)

    bad(R=None)
    bad(R=R[:, :15])
    bad(R=np.zeros((2, 3, 18)))
    bad(masses=np.ones(5))
    bad(masses=np.ones((6, 1)))
    for val in (np.nan, np.inf):
        Rb, mb = R.copy(), m.copy()
        Rb[1, 3], mb[2] = val, val
        bad(R=Rb)
        bad(masses=mb)
        bad(f_unit=val)
    bad(masses=np.array([1.0, 1.0, 0.0, 1.0, 1.0, 1.0]))
    bad(masses=-m)
    bad(f_unit=0.0)
    bad(f_unit=-1.0)
    bad(project='rotations')
    bad(project=2)
    bad(stub(lat), project='rigid')
    # what passes the checks reaches the device call: the default projection follows the lattice
    for s, proj in ((stub(), None), (stub(lat), None), (stub(lat), 'trans'), (stub(lat), 'none'), (stub(), 'rigid')):
        with pytest.raises(AssertionError):
            GDMLPredict.vibrations(s, R, m, project=proj)
    # the binding's own shape check
    with pytest.raises(ValueError):
        _lib.Context.vib_run(types.SimpleNamespace(model_n_atoms=6, _masses=lambda mm: _lib.Context._masses(
            types.SimpleNamespace(model_n_atoms=6), mm)), R, np.ones(5))

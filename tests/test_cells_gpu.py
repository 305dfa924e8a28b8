"""Prediction with one lattice per geometry on the GPU (gdml_predict_virial_cells, csrc/predict.hip; desc_cells_kernel,
csrc/desc.hip; predict / predict_virial / predict_stress(..., lattices=)): bit for bit against the one-lattice entries on every
route behind the descriptors, against the NumPy restatement (tests/_stress_ref.py) with distinct lattices, host entry against
device entry, determinism, and the Python surface."""
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
import _stress_ref as sr  # noqa: E402
from sgdml_amd import _lib  # noqa: E402
from sgdml_amd.predict import GDMLPredict, check_lattice  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = ['n4_p6_pbc', 'n10_p2_pbc']
TOL = {'n4_p6_pbc': 1e-8}  # tests/test_stress_gpu.py: the fixture is ill-conditioned; 1e-10 otherwise


@functools.lru_cache(maxsize=None)
def _predictor(name):
    return GDMLPredict(mr.case(name)[0])


@functools.lru_cache(maxsize=None)
def _strained(name):
    """Seven geometries of the fixture, each strained together with its cell by its own symmetric strain of up to 3 % per
    component (the minimum-image integers stay as they are): (R (7,3N), lattices (7,3,3), inverses)."""
    model, R7 = mr.case(name)
    lat = np.asarray(model['lattice'], dtype=np.float64)
    eps = 0.03 * (2.0 * np.random.RandomState(11).random_sample((7, 3, 3)) - 1.0)
    S = np.eye(3)[None] + 0.5 * (eps + eps.transpose(0, 2, 1))
    R = np.einsum('bac,bic->bia', S, R7.reshape(7, -1, 3)).reshape(7, -1)
    lats = np.einsum('bac,cd->bad', S, lat)
    invs = np.array([check_lattice(L)[1] for L in lats])
    for a in (R, lats, invs):
        a.setflags(write=False)
    return R, lats, invs


class _Dev(object):
    """Device copies of host arrays for the _dev entries; freed on exit."""

    def __init__(self, ctx):
        self.ctx, self.ptrs = ctx, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for p in self.ptrs:
            self.ctx._lib.gdml_dev_free(self.ctx._h, p)

    def alloc(self, nbytes):
        p = C.c_void_p()
        self.ctx._check(self.ctx._lib.gdml_dev_alloc(self.ctx._h, max(int(nbytes), 8), C.byref(p)))
        self.ptrs.append(p)
        return p

    def put(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        p = self.alloc(a.nbytes)
        self.ctx._check(self.ctx._lib.gdml_memcpy_h2d(self.ctx._h, p, a.ctypes.data_as(C.c_void_p), a.nbytes))
        return p

    def get(self, p, shape):
        o = np.empty(shape)
        self.ctx._check(self.ctx._lib.gdml_memcpy_d2h(self.ctx._h, o.ctypes.data_as(C.c_void_p), p, o.nbytes))
        return o


def _dev_one(ctx, R, lat_and_inv, virial=True):
    """gdml_predict_virial_dev (or gdml_predict_dev) with ONE lattice for the batch."""
    B, n3 = R.shape
    with _Dev(ctx) as d:
        pR, pE, pF, pW = d.put(R), d.alloc(B * 8), d.alloc(B * n3 * 8), d.alloc(B * 72)
        lat, inv = _lib._lat_pair(lat_and_inv)
        if virial:
            ctx.predict_virial_dev(pR, B, pE, pF, pW, lat_and_inv)
        else:
            ctx._check(ctx._lib.gdml_predict_dev(ctx._h, pR, B, _lib._ptr(lat), _lib._ptr(inv), pE, pF))
        return d.get(pE, B), d.get(pF, (B, n3)), d.get(pW, (B, 3, 3)) if virial else None


def _dev_cells(ctx, R, lats, invs, virial=True):
    B, n3 = R.shape
    with _Dev(ctx) as d:
        pR, pL, pI, pE, pF, pW = d.put(R), d.put(lats), d.put(invs), d.alloc(B * 8), d.alloc(B * n3 * 8), d.alloc(B * 72)
        ctx.predict_cells_dev(pR, B, pL, pI, pE, pF, pW if virial else None)
        return d.get(pE, B), d.get(pF, (B, n3)), d.get(pW, (B, 3, 3)) if virial else None


def _same(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


def _check_equal_lattices(ctx, R, lat_and_inv, what):
    B = len(R)
    lats = np.broadcast_to(lat_and_inv[0], (B, 3, 3))
    invs = np.broadcast_to(lat_and_inv[1], (B, 3, 3))
    one = _dev_one(ctx, R, lat_and_inv)
    cells = _dev_cells(ctx, R, lats, invs)
    assert _same(one, cells), what
    assert _same(_dev_one(ctx, R, lat_and_inv, virial=False), _dev_cells(ctx, R, lats, invs, virial=False)), what  # W = NULL
    assert np.array_equal(one[0], _dev_one(ctx, R, lat_and_inv, virial=False)[0]), what
    return cells


@pytest.mark.parametrize('name', CASES)
def test_equal_lattices_give_the_bits_of_the_one_lattice_entries(name):
    """B = 1 and 7 (the WAVE route) and B = 256 on MFMA, on BULK (predict.mfma = 0) and, for the 10-atom fixture, on WIDE
    (predict.mfma_wide = 2): E, F and W of gdml_predict_virial_cells_dev are those of gdml_predict_virial_dev, and with
    W = NULL E and F are those of gdml_predict_dev."""
    model, R7 = mr.case(name)
    pred = _predictor(name)
    ctx = pred._ctx
    lai = pred.lat_and_inv
    _check_equal_lattices(ctx, R7[:1], lai, name + ' B=1')
    _check_equal_lattices(ctx, R7, lai, name + ' B=7')
    R256 = np.ascontiguousarray(R7[np.arange(256) % len(R7)])
    _check_equal_lattices(ctx, R256, lai, name + ' B=256 mfma')
    try:
        ctx.set_option('predict.mfma', 0)
        _check_equal_lattices(ctx, R256, lai, name + ' B=256 bulk')
        ctx.set_option('predict.mfma', 1)
        if name == 'n10_p2_pbc':
            ctx.set_option('predict.mfma_wide', 2)
            _check_equal_lattices(ctx, R256, lai, name + ' B=256 wide')
    finally:
        ctx.set_option('predict.mfma', 1)
        ctx.set_option('predict.mfma_wide', 1)


@pytest.mark.parametrize('name', CASES)
def test_distinct_lattices_row_by_row(name):
    """Each geometry's cell strained differently by up to 3 %: row b equals, bit for bit, row b of the one-lattice call on the
    whole batch with lattice b, and agrees with the restatement with that lattice within the fixture's tolerance of
    tests/test_stress_gpu.py."""
    model, _ = mr.case(name)
    R, lats, invs = _strained(name)
    ctx = _predictor(name)._ctx
    E, F, W = _dev_cells(ctx, R, lats, invs)
    assert not np.array_equal(W[0], W[1])
    tol = TOL.get(name, 1e-10)
    tp = sr.orc.tril_perms_from_lin(model['tril_perms_lin'], model['R_desc'].shape[0])
    worst = 0.0
    for b in range(7):
        Eb, Fb, Wb = _dev_one(ctx, R, (lats[b], invs[b]))
        assert np.array_equal(E[b], Eb[b]) and np.array_equal(F[b], Fb[b]) and np.array_equal(W[b], Wb[b]), b
        Er, Fr, Wr = sr.virial(R[b:b + 1], np.asarray(model['R_desc']).T, model['R_d_desc_alpha'], tp, model['sig'],
                               model.get('alphas_E'), (lats[b], np.linalg.inv(lats[b])))
        err = max(np.abs(W[b] - Wr[0]).max() / np.abs(Wr).max(), np.abs(F[b] - Fr[0]).max() / np.abs(Fr).max(),
                  abs(E[b] - Er[0]) / abs(Er[0]))
        worst = max(worst, err)
        assert err <= tol, (b, err)
    print('%s: distinct lattices against the restatement: %.2e' % (name, worst))


@pytest.mark.parametrize('name', CASES)
def test_host_entry_equals_device_entry_and_repeats(name):
    R, lats, invs = _strained(name)
    ctx = _predictor(name)._ctx
    for B in (1, 7, 70):  # one to eight host geometries take the general route too
        idx = np.arange(B) % 7
        Rb, Lb, Ib = (np.ascontiguousarray(a[idx]) for a in (R, lats, invs))
        dev = _dev_cells(ctx, Rb, Lb, Ib)
        host = ctx.predict_cells(Rb, Lb, Ib)
        assert _same(dev, host), B
        assert _same(host, ctx.predict_cells(Rb, Lb, Ib)) and _same(dev, _dev_cells(ctx, Rb, Lb, Ib)), B
        E, F, W = ctx.predict_cells(Rb, Lb, Ib, virial=False)  # W_out = NULL: a plain prediction
        assert W is None and np.array_equal(E, host[0]) and np.array_equal(F, host[1])
        E, F, W = ctx.predict_cells(Rb, Lb, Ib, return_E=False)
        assert E is None and np.array_equal(F, host[1]) and np.array_equal(W, host[2])
        assert np.array_equal(host[2], host[2].transpose(0, 2, 1))


def test_python_surface_scales_and_divides_by_each_volume():
    name = 'n10_p2_pbc'
    model, R7 = mr.case(name)
    R, lats, invs = _strained(name)
    pred = _predictor(name)
    E0, F0, W0 = pred._ctx.predict_cells(R, lats, invs)
    E, F, W = pred.predict_virial(R, lattices=lats)
    assert np.array_equal(E, E0 * pred.std + pred.c) and np.array_equal(F, F0 * pred.std) and np.array_equal(W, W0 * pred.std)
    Ep, Fp = pred.predict(R, lattices=lats)
    assert np.array_equal(Ep, E) and np.array_equal(Fp, F)
    (Fq,) = pred.predict(R, return_E=False, lattices=lats)
    assert np.array_equal(Fq, F)
    Es, Fs, S = pred.predict_stress(R, lattices=lats)
    vol = np.abs(np.linalg.det(lats))
    assert vol.max() / vol.min() > 1.02  # the volumes differ: one common divisor would show
    assert np.array_equal(Es, E) and np.array_equal(Fs, F)
    assert np.abs(S - W / vol[:, None, None]).max() <= 8 * np.finfo(float).eps * np.abs(S).max()
    _, _, V = pred.predict_stress(R, lattices=lats, voigt=True)
    assert np.array_equal(V, S.reshape(7, 9)[:, [0, 4, 8, 5, 2, 1]])
    # all lattices the model's own: the one-lattice call on the general route (70 geometries: no single launch)
    R70 = np.ascontiguousarray(R7[np.arange(70) % 7])
    a = pred.predict_virial(R70)
    b = pred.predict_virial(R70, lattices=np.broadcast_to(model['lattice'], (70, 3, 3)))
    assert _same(a, b)


def test_error_paths():
    name = 'n10_p2_pbc'
    R, lats, invs = _strained(name)
    pred = _predictor(name)
    ctx, lib = pred._ctx, pred._ctx._lib
    vp = _lib._ptr
    Rc, Lc, Ic, W, F = (np.ascontiguousarray(a) for a in (R, lats, invs, np.empty((7, 3, 3)), np.empty((7, 30))))
    for fn in (lib.gdml_predict_virial_cells, lib.gdml_predict_virial_cells_dev):  # rejected before any pointer is used
        assert fn(ctx._h, None, 7, vp(Lc), vp(Ic), None, None, vp(W)) == -1
        assert fn(ctx._h, vp(Rc), 7, None, vp(Ic), None, None, vp(W)) == -1
        assert fn(ctx._h, vp(Rc), 7, vp(Lc), None, None, None, vp(W)) == -1
    assert lib.gdml_predict_virial_cells(ctx._h, vp(Rc), -1, vp(Lc), vp(Ic), None, vp(F), None) == -1
    assert lib.gdml_predict_virial_cells(ctx._h, vp(Rc), 7, vp(Lc), vp(Ic), None, None, None) == -1  # neither F nor W
    lat = np.asarray(mr.case(name)[0]['lattice'])
    singular = np.array([[1.0, 2.0, 3.0], [2.0, 4.0, 6.0], [0.0, 0.0, 1.0]])
    bad_member = np.array(lats)
    bad_member[3] = singular
    for call in (pred.predict, pred.predict_virial, pred.predict_stress):
        with pytest.raises(ValueError):
            call(R, lattice=lat, lattices=lats)
        for bad in (lats[:6], lat, np.zeros((7, 3, 4)), bad_member):
            with pytest.raises(ValueError):
                call(R, lattices=bad)
        with pytest.raises(ValueError):
            call(R, lattice=np.eye(2))  # lattice= keeps its errors
    with pytest.raises(ValueError):
        pred.predict(None, lattices=lats)
    empty = _lib.Context(0)
    try:
        empty.model_n_atoms = 10
        with pytest.raises(_lib.GDMLHipError):  # no model resident
            empty.predict_cells(Rc, Lc, Ic)
    finally:
        empty.close()
    E, F, W2 = pred.predict_virial(R, lattices=lats)  # the predictor still works
    assert np.isfinite(W2).all()

"""Gradient of the model evidence in sig and lam without a GPU: K' of tests/_evidence_ref.py against a central difference of
the oracle's kernel matrix, the helper's derivatives against central differences of its own evidence, the stepping rule of
GDMLPredict.optimize_hyperparameters on the NumPy evidence, and the binding."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _evidence_ref as er  # noqa: E402
import _uncertainty_ref as ur  # noqa: E402
from oracle import gdml_oracle as orc  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
FIXTURES = ['n5_p4', 'n9_p1', 'n4_p6_pbc', 'n10_p2_pbc']


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name + '.npz')))


@pytest.mark.parametrize('name', FIXTURES)
def test_dK_dsig_is_the_derivative_of_the_oracle_kernel(name):
    """Central difference of oracle._full_K at relative step h = 1e-5: truncation h^2 sig^2 |K'''| / 6 ~ 1e-10 |K'| and
    round-off eps |K| / (h sig) ~ 1e-11 |K'| (observed: at most 2e-10 of max|K'|); asserted at 1e-8.  K' is symmetric to
    rounding."""
    g = _load(name)
    x, gd, tp, _, _, _ = er.tables(g)
    sig = float(g['sig'])
    Kp = er.dK_dsig(x, gd, tp, sig)
    h = 1e-5 * sig
    fd = (orc._full_K(x, gd, tp, sig + h, False) - orc._full_K(x, gd, tp, sig - h, False)) / (2.0 * h)
    scale = np.abs(Kp).max()
    print('%s  max|K\' - fd| / max|K\'| = %.2e   asymmetry %.2e' % (name, np.abs(Kp - fd).max() / scale, np.abs(Kp - Kp.T).max() / scale))
    assert np.abs(Kp - fd).max() <= 1e-8 * scale
    assert np.abs(Kp - Kp.T).max() <= 1e-14 * scale


@pytest.mark.parametrize('name', FIXTURES)
def test_derivatives_are_those_of_the_evidence(name):
    """d_sig and d_lam of the helper against central differences of the helper's own profiled evidence at relative step 1e-3,
    to 1e-4 relative (truncation ~ step^2; loosest value observed 1e-5)."""
    g = _load(name)
    x, gd, tp, y, _, _ = er.tables(g)
    sig, lam = float(g['sig']), float(g['lam'])
    b = er.bounds_of(g)
    assert abs(b.lml - er.evidence_at(x, gd, tp, y, sig, lam)) <= 0.5 * (b.n * b.s2_tol / b.s2 + b.tol[4])  # two solves of one system
    h = 1e-3
    fd_sig = (er.evidence_at(x, gd, tp, y, sig * (1 + h), lam) - er.evidence_at(x, gd, tp, y, sig * (1 - h), lam)) / (2 * h * sig)
    fd_lam = (er.evidence_at(x, gd, tp, y, sig, lam * (1 + h)) - er.evidence_at(x, gd, tp, y, sig, lam * (1 - h))) / (2 * h * lam)
    print('%s  d_sig %.6e (fd %.6e)  d_lam %.6e (fd %.6e)' % (name, b.d_sig, fd_sig, b.d_lam, fd_lam))
    assert abs(b.d_sig - fd_sig) <= 1e-4 * abs(fd_sig)
    assert abs(b.d_lam - fd_lam) <= 1e-4 * abs(fd_lam)


def test_stepping_rule_finds_the_maximum_in_log_sig():
    """`ascend` on the NumPy evidence of n5_p4 in log sig, started a factor 2 off: the returned point is no lower than the
    start and no lower than its neighbours at +-1 % in sig."""
    from sgdml_amd.predict import ascend

    g = _load('n5_p4')
    x, gd, tp, y, _, _ = er.tables(g)
    lam = float(g['lam'])

    def fun(v):
        sig = float(np.exp(v[0]))
        b = er.Bounds(ur.system_matrix(x, gd, tp, sig, lam), er.dK_dsig(x, gd, tp, sig), y)
        return b.lml, np.array([sig * b.d_sig])

    start = np.log([2.0 * float(g['sig'])])
    xb, trace = ascend(fun, start, max_iter=30, gtol=1e-4)
    vals = [t[1] for t in trace]
    assert all(b >= a for a, b in zip(vals, vals[1:])) and np.array_equal(trace[-1][0], xb)
    sig = float(np.exp(xb[0]))
    f = er.evidence_at(x, gd, tp, y, sig, lam)
    print('sig %.6g -> %.6g in %d steps, lml %.6f -> %.6f' % (np.exp(start[0]), sig, len(trace) - 1, vals[0], f))
    assert f >= vals[0]
    assert f >= er.evidence_at(x, gd, tp, y, 1.01 * sig, lam) and f >= er.evidence_at(x, gd, tp, y, 0.99 * sig, lam)


def test_stepping_rule_failed_steps_and_bounds():
    """A point that cannot be evaluated halves the step; a bound holds the iterate; the values never decrease."""
    from sgdml_amd.predict import ascend

    def fun(v):  # concave, maximum at (1, -2); not evaluable beyond v[0] > 1.5
        if v[0] > 1.5:
            raise np.linalg.LinAlgError('not positive definite')
        return -(v[0] - 1.0) ** 2 - 3.0 * (v[1] + 2.0) ** 2, np.array([-2.0 * (v[0] - 1.0), -6.0 * (v[1] + 2.0)])

    xb, trace = ascend(fun, [-4.0, 3.0], max_iter=50, gtol=1e-8, max_step=10.0)
    assert np.allclose(xb, [1.0, -2.0], atol=1e-6)
    xb, trace = ascend(fun, [-4.0, 3.0], max_iter=50, gtol=1e-8, bounds=([-5.0, -1.0], [0.5, 5.0]))
    assert np.allclose(xb, [0.5, -1.0], atol=1e-6)
    vals = [t[1] for t in trace]
    assert all(b >= a for a, b in zip(vals, vals[1:]))


def test_binding_exports_and_declares_the_entry():
    from sgdml_amd import _lib

    hdr = open(os.path.join(ROOT, 'include', 'gdml_hip.h')).read()
    m = re.search(r'int gdml_evidence_grad\(([^;]*)\);', hdr)
    assert m is not None
    n_args = len(re.sub(r'/\*.*?\*/', '', m.group(1)).split(','))
    res, args = _lib.SIGNATURES['gdml_evidence_grad']
    assert len(args) == n_args == 5
    assert 'evidence.hip' in open(os.path.join(ROOT, 'sgdml_amd', 'csrc', 'Makefile')).read()
    if os.path.exists(_lib.LIB_PATH):
        import ctypes as C

        assert hasattr(C.CDLL(_lib.LIB_PATH), 'gdml_evidence_grad')
        assert _lib.load().gdml_abi_version() == 4

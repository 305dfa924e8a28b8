"""The contract of the nine entries that work on the resident Cholesky factor (csrc/resident.hip,
resident_factor_check): the code each of them returns in every state in which it must refuse.  Raw library calls; every refusal
comes from a host-side check, nothing is launched in a bad state."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _uncertainty_ref as ur  # noqa: E402
from sgdml_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
OK, STATE, UNSUPPORTED = _lib.GDML_OK, _lib.ERR_STATE, _lib.ERR_UNSUPPORTED  # 0, -4, -6
ANY_FACTOR = ('gdml_loo', 'gdml_evidence_grad')  # accept a factor of gdml_chol_factor; the other seven want gdml_uncert_prepare's
PREPARED = ('gdml_predict_cov', 'gdml_predict_cov_dev', 'gdml_predict_cov_few', 'gdml_predict_cov_few_dev', 'gdml_select_points',
            'gdml_factor_extend', 'gdml_factor_remove')


def _tables(name):
    g = dict(np.load(os.path.join(GOLDEN, name + '.npz')))
    R, x, gd, tp, _ = ur.fixture_tables(g)
    return R, x, gd, tp, float(g['sig']), float(g['lam'])


def _codes(ctx, R, x, gd, M):
    """Return code of every entry, called with valid arguments for a resident training set of M points (queries R[:2], one
    point to append, point 0 to remove).  The _dev entries get host pointers: a refusal comes before any pointer is used."""
    lib, h = ctx._lib, ctx._h
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    n3 = R.shape[1]
    q = np.ascontiguousarray(R[:2])
    alphas, resid, terms, out = np.full(M * n3, 0.5), np.empty(M * n3), np.empty(5), np.empty((2, n3))
    idx, gain, gain0, one = np.zeros(1, dtype=np.int64), np.zeros(1), np.zeros(2), np.zeros(1, dtype=np.int64)
    x1, g1 = np.ascontiguousarray(x[:1]), np.ascontiguousarray(gd[:1])
    logdet, info, k = C.c_double(0.0), C.c_int(0), C.c_int64(0)
    codes = {
        'gdml_loo': lib.gdml_loo(h, vp(alphas), alphas.size, 0, vp(resid), None, C.byref(logdet), C.byref(info)),
        'gdml_evidence_grad': lib.gdml_evidence_grad(h, vp(alphas), alphas.size, vp(terms), C.byref(info)),
        'gdml_select_points': lib.gdml_select_points(h, vp(q), 2, None, None, 1, -np.inf, vp(idx), vp(gain), vp(gain0), C.byref(k),
                                                     C.byref(info)),
        'gdml_factor_extend': lib.gdml_factor_extend(h, vp(x1), vp(g1), 1, C.byref(info)),
        'gdml_factor_remove': lib.gdml_factor_remove(h, vp(one), 1, C.byref(info)),
    }
    for name in PREPARED[:4]:
        codes[name] = getattr(lib, name)(h, vp(q), 2, None, None, 0, vp(out))
    assert set(codes) == set(ANY_FACTOR + PREPARED)
    return codes


def _expect(any_factor, prepared):
    return {**{k: any_factor for k in ANY_FACTOR}, **{k: prepared for k in PREPARED}}


def test_refusals_by_state():
    R, x, gd, tp, sig, lam = _tables('n6_p1')
    M = len(x)
    ctx = _lib.Context(0)
    try:
        assert _codes(ctx, R, x, gd, M) == _expect(STATE, STATE), 'no training set'
        ctx.train_upload(x, gd, tp)
        assert _codes(ctx, R, x, gd, M) == _expect(STATE, STATE), 'training set, no matrix'
        ctx.assemble_K(sig, False, for_cholesky=lam)
        assert _codes(ctx, R, x, gd, M) == _expect(STATE, STATE), 'assembled, not factored'
        ctx.chol_factor(lam)
        assert _codes(ctx, R, x, gd, M) == _expect(OK, STATE), 'factored by gdml_chol_factor, not prepared'
        ctx.uncert_prepare(sig, lam)
        ctx.uncert_release()
        assert _codes(ctx, R, x, gd, M) == _expect(STATE, STATE), 'prepared, then released'
        ctx.uncert_prepare(sig, lam)
        ctx.train_upload(x[:M - 1], gd[:M - 1], tp)  # the factor in the buffer is that of M points
        assert _codes(ctx, R, x, gd, M - 1) == _expect(STATE, STATE), 'prepared, then another training set'
        with pytest.raises(_lib.GDMLHipError, match='does not belong to the resident training set'):
            ctx.loo(np.zeros((M - 1) * R.shape[1]))
        ctx.uncert_prepare(sig, lam)  # ... and the context recovers
        assert ctx.predict_cov(R[:2]).shape == (2, R.shape[1])
    finally:
        ctx.close()


def test_refusal_of_energy_constraint_rows():
    R, x, gd, tp, sig, lam = _tables('n5_p2_ecstr')
    ctx = _lib.Context(0)
    try:
        ctx.train_upload(x, gd, tp)
        ctx.assemble_K(sig, True, for_cholesky=lam)
        ctx.chol_factor(lam)
        assert _codes(ctx, R, x, gd, len(x)) == _expect(UNSUPPORTED, UNSUPPORTED)
    finally:
        ctx.close()

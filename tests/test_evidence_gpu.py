"""Gradient of the model evidence in sig and lam on the GPU (csrc/evidence.hip) against the NumPy restatement
(tests/_evidence_ref.py): parity of the five sums and the two derivatives within the derived bounds, determinism and the
invariants, the meaning through the public API (central differences of loo_errors' evidence), the optimiser and the error
paths."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _evidence_ref as er  # noqa: E402
import _extend_ref as xr  # noqa: E402
import _uncertainty_ref as ur  # noqa: E402
from sgdml_amd import _lib  # noqa: E402
from sgdml_amd.predict import GDMLPredict  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
# (fixture, lam; None = the stored one).  Every case passes the meaningfulness cap below with the reference values alone
# (largest bound / |value|: 2.7e-3, n4_p6_pbc, a^T K' a).  cfg0 / cfg1 / cfg3_n42_p27 at their stored lam = 1e-10 do not (the
# trace bound is 0.15 of the value for cfg3_n42_p27, 7.5 times the value for cfg1): do not add cases without checking them.
SMALL = [('n6_p1', None), ('n5_p4', None), ('n9_p1', None), ('n4_p6_pbc', None), ('n10_p2_pbc', None)]
RAISED = [('cfg3_n42_p27', 1e-4),   # 3N = 126: the LDS form at its largest, P = 27
          ('n100_m3', 1e-4),        # 3N = 300 > 128: the tile is walked in global memory
          ('cfg0_n9_p6', 1e-4),     # n = 5400: eleven panels, four chunks of 64 points
          ('cfg1_n21_m100', 1e-4)]  # n = 6300, 3N = 63: the benchmark's shape
CASES = SMALL + RAISED
CAP = 1e-2
RECORD = os.environ.get('GDML_EVIDENCE_RECORD', os.path.join(ROOT, 'profiles', 'evidence_parity.json'))
_observed = {}


def _load(name):
    return dict(np.load(os.path.join(GOLDEN, name + '.npz')))


@functools.lru_cache(maxsize=None)
def _ref(name, lam):
    """Reference values and bounds of a case, computed once per session."""
    g = _load(name)
    b = er.bounds_of(g, lam)
    model = ur.model_from_fixture(g)
    if lam is not None:
        model['lam'] = float(lam)
    M = g['R_train'].shape[0]
    return {'g': g, 'b': b, 'model': model, 'R_train': np.asarray(g['R_train'], dtype=np.float64).reshape(M, -1),
            'F_train': np.asarray(g['F_train'], dtype=np.float64).reshape(M, -1), 'y': er.tables(g)[3]}


@functools.lru_cache(maxsize=None)
def _pred(name, lam):
    """A predictor with the factor of the case resident, and the coefficients of y for that factor."""
    r = _ref(name, lam)
    pred = GDMLPredict(r['model'])
    pred.prepare_uncertainty(r['R_train'])
    return pred, pred._ctx.chol_solve(r['y'])


def _ratios(b, terms, out=None):
    q = {k: abs(terms[i] - b.terms[i]) / b.tol[i] for i, k in enumerate(er.TERMS)}
    if out is not None:
        q['d_sig'] = abs(out['d_sig'] - b.d_sig) / b.d_sig_tol
        q['d_lam'] = abs(out['d_lam'] - b.d_lam) / b.d_lam_tol
    return q


@pytest.mark.parametrize('name,lam', CASES)
def test_parity(name, lam):
    """Each of the five sums within its bound of the reference value, d_sig and d_lam of the public method within the
    propagated bounds (derivations: _evidence_ref.Bounds), every bound of the five sums capped at a hundredth of its value so
    that the comparison means something (the derivatives can pass through zero and carry no cap of their own); the observed
    error / bound ratios go to the record file."""
    r = _ref(name, lam)
    b = r['b']
    for i, k in enumerate(er.TERMS):  # a condition on the reference values, not a measurement
        assert b.tol[i] <= CAP * abs(b.terms[i]), k
    pred, alphas = _pred(name, lam)
    terms = pred._ctx.evidence_grad(alphas)
    out = pred.evidence_gradient(F_train=r['F_train'])
    assert np.array_equal(out['terms'], terms) and out['log_det_A'] == terms[4]
    assert out['d_log_sig'] == pred.sig * out['d_sig'] and out['d_log_lam'] == pred._lam * out['d_lam']
    s2 = float(-np.dot(r['y'], alphas) / r['y'].size)
    assert out['signal_variance'] == s2
    assert abs(out['log_marginal_likelihood'] - b.lml) <= 0.5 * (b.n * b.s2_tol / b.s2 + b.tol[4])
    q = _ratios(b, terms, out)
    for k in q:
        print('%s  %-10s |gpu - ref| / bound = %.3g' % (name, k, q[k]))
    assert all(v <= 1.0 for v in q.values()), q
    _observed[name] = {k: float('%.3g' % v) for k, v in q.items()}
    if len(_observed) == len(CASES):
        with open(RECORD, 'w') as f:
            json.dump({'what': 'largest |gpu - ref| / bound of tr A^-1, <A^-1, K\'>, a^T K\' a, a^T a, log det A, d_sig and d_lam per '
                               'case (tests/test_evidence_gpu.py; cfg0, cfg1, cfg3 and n100_m3 at lam = 1e-4)',
                       'ratio': {k: _observed[k] for k, _ in CASES}}, f, indent=1)
            f.write('\n')


def test_global_vector_path():
    """Option chol.evidence_global: tile and per-pair vectors in global memory (the path of descriptors beyond LDS), P = 2."""
    name, lam = 'n10_p2_pbc', None
    r = _ref(name, lam)
    pred, alphas = _pred(name, lam)
    try:
        pred._ctx.set_option('chol.evidence_global', 1)
        terms = pred._ctx.evidence_grad(alphas)
        assert np.array_equal(terms, pred._ctx.evidence_grad(alphas))
    finally:
        pred._ctx.set_option('chol.evidence_global', 0)
    q = _ratios(r['b'], terms)
    print(q)
    assert all(v <= 1.0 for v in q.values()), q


def test_determinism_chunks_and_logdet():
    name, lam = 'cfg0_n9_p6', 1e-4  # n = 5400 spans eleven 512-column panels: c0 takes many values
    r = _ref(name, lam)
    pred, alphas = _pred(name, lam)
    ctx = pred._ctx
    full = ctx.evidence_grad(alphas)
    assert np.array_equal(full, ctx.evidence_grad(alphas))  # bit for bit
    assert full[4] == ctx.loo(alphas)[2]  # the same gather and host sum
    try:
        for chunk in (1, 3):
            ctx.set_option('chol.evidence_chunk', chunk)
            got = ctx.evidence_grad(alphas)
            q = _ratios(r['b'], got)
            print('chunk %d' % chunk, q)
            assert all(v <= 1.0 for v in q.values()), (chunk, q)
            assert got[4] == full[4] and got[3] == full[3]
    finally:
        ctx.set_option('chol.evidence_chunk', 64)


def test_factor_is_only_read():
    name, lam = 'n10_p2_pbc', None
    r = _ref(name, lam)
    pred, alphas = _pred(name, lam)
    ctx = pred._ctx
    Rq = ur.queries(r['g'])
    lat = (np.asarray(r['g']['lattice']), np.linalg.inv(r['g']['lattice']))
    before = (ctx.predict_cov(Rq, lat, full=True), ctx.loo(alphas, 'full'), ctx.chol_solve(r['y']))
    held = ctx.mem_info()[0]
    ctx.evidence_grad(alphas)
    assert ctx.mem_info()[0] <= held  # the second matrix is gone (the work slots are the ones loo carved)
    after = (ctx.predict_cov(Rq, lat, full=True), ctx.loo(alphas, 'full'), ctx.chol_solve(r['y']))
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[2], after[2])
    assert np.array_equal(before[1][0], after[1][0]) and np.array_equal(before[1][1], after[1][1]) and before[1][2] == after[1][2]


def _sub_bounds(t, keep):
    x, gd = t['x'][keep], t['gd'][keep]
    y = (t['F'][keep] / t['std']).ravel()
    return er.Bounds(ur.system_matrix(x, gd, t['tp'], t['sig'], t['lam']), er.dK_dsig(x, gd, t['tp'], t['sig']), y), y


def test_on_extended_and_reduced_factors():
    """The call works at once on the factor left by add_training_points / remove_training_points and agrees with a freshly
    prepared predictor of the same points: both within the bounds of the reference values of that system."""
    name = 'n10_p2_pbc'
    g = _load(name)
    t = xr.tables(g)
    M, n3 = t['R'].shape
    # grown: the first M - 2 points, then the last two
    keep0 = np.arange(M - 2)
    b0, y0 = _sub_bounds(t, keep0)
    pred = GDMLPredict(xr.model_dict(t, M - 2, -b0.a))
    pred.prepare_uncertainty(t['R'][:M - 2], t['F'][:M - 2])
    pred.add_training_points(t['R'][M - 2:], t['F'][M - 2:])
    r = _ref(name, None)
    grown = pred.evidence_gradient()
    fresh = _pred(name, None)[0].evidence_gradient(F_train=r['F_train'])
    for out in (grown, fresh):
        q = _ratios(r['b'], out['terms'], out)
        print('grown / fresh', q)
        assert all(v <= 1.0 for v in q.values()), q
    # reduced: two points out of the middle
    keep = np.array([j for j in range(M) if j not in (2, 7)])
    bk, yk = _sub_bounds(t, keep)
    pred.remove_training_points([2, 7])
    reduced = pred.evidence_gradient()
    pf = GDMLPredict(pred.export_model())
    pf.prepare_uncertainty(t['R'][keep], t['F'][keep])
    fresh = pf.evidence_gradient()
    for out in (reduced, fresh):
        q = _ratios(bk, out['terms'], out)
        print('reduced / fresh', q)
        assert all(v <= 1.0 for v in q.values()), q


def test_meaning_through_the_public_api():
    """d_log_sig and d_log_lam against central differences of loo_errors(...)['log_marginal_likelihood'] from predictors
    prepared at sig (1 +- 1e-3) and lam (1 +- 1e-3), at the signal variance of the centre (the partial derivatives at fixed s^2
    are what the entry returns).  Tolerance: ten times the NumPy helper's own gap between its analytic value and the same
    central difference of its own evidence (the truncation error, common to both; the factor 10 covers GPU rounding)."""
    name, h = 'n10_p2_pbc', 1e-3
    r = _ref(name, None)
    g, b = r['g'], r['b']
    x, gd, tp, y, _, _ = er.tables(g)
    sig, lam = float(g['sig']), float(g['lam'])
    pred, _ = _pred(name, None)
    out = pred.evidence_gradient(F_train=r['F_train'])
    s2 = out['signal_variance']

    def lml_gpu(sg, lm):
        m = dict(r['model'])
        m['sig'], m['lam'] = sg, lm
        p = GDMLPredict(m)
        p.prepare_uncertainty(r['R_train'])
        p.uncertainty_scale = s2
        return p.loo_errors(F_train=r['F_train'])['log_marginal_likelihood']

    rec = {}
    for key, pts, ana in (('d_log_sig', ((sig * (1 + h), lam), (sig * (1 - h), lam)), sig * b.d_sig),
                          ('d_log_lam', ((sig, lam * (1 + h)), (sig, lam * (1 - h))), lam * b.d_lam)):
        fd_ref = (er.evidence_at(x, gd, tp, y, *pts[0], s2=b.s2) - er.evidence_at(x, gd, tp, y, *pts[1], s2=b.s2)) / (2 * h)
        gap = abs(ana - fd_ref)
        fd_gpu = (lml_gpu(*pts[0]) - lml_gpu(*pts[1])) / (2 * h)
        print('%s  gpu %.9e  fd(gpu lml) %.9e  helper %.9e  helper gap %.3e  gpu gap %.3e' % (
            key, out[key], fd_gpu, ana, gap, abs(out[key] - fd_gpu)))
        rec[key] = {'helper_gap': float('%.3g' % gap), 'gpu_gap': float('%.3g' % abs(out[key] - fd_gpu))}
        assert abs(out[key] - fd_gpu) <= 10.0 * gap, key
    path = os.path.join(os.path.dirname(RECORD), 'evidence_fd.json')
    with open(path, 'w') as f:
        json.dump({'what': 'n10_p2_pbc, relative step 1e-3: |analytic - central difference| of the NumPy helper (the tolerance is '
                           'ten times that) and |evidence_gradient - central difference of loo_errors| on the GPU', 'gap': rec}, f, indent=1)
        f.write('\n')


@pytest.mark.parametrize('name,params', [('n5_p4', ('sig',)), ('n10_p2_pbc', ('sig', 'lam'))])
def test_optimiser(name, params):
    """From sig off by a factor 2: the returned point, evaluated by the NumPy helper, is no lower than the start and than its
    +-1 % neighbours in each optimised parameter; export_model() carries it and predicts what the predictor predicts."""
    r = _ref(name, None)
    g = r['g']
    x, gd, tp, y, _, _ = er.tables(g)
    m = dict(r['model'])
    m['sig'] = 2.0 * float(g['sig'])
    start = {'sig': m['sig'], 'lam': float(m['lam'])}
    pred = GDMLPredict(m)
    E = np.asarray(g['E_train'], dtype=np.float64).ravel()
    trace = pred.optimize_hyperparameters(r['R_train'], r['F_train'], E_train=E, params=params, max_iter=40, gtol=1e-5)
    best = {'sig': pred.sig, 'lam': pred._lam}
    print(name, 'start', start, 'best', best, len(trace) - 1, 'steps')
    assert trace[0]['sig'] == start['sig'] and trace[-1]['sig'] == best['sig'] and trace[-1]['lam'] == best['lam']
    assert all(k == 'sig' or k in params or best[k] == start[k] for k in best)
    lml = lambda hp: er.evidence_at(x, gd, tp, y, hp['sig'], hp['lam'])
    f = lml(best)
    assert f >= lml(start)
    for k in params:
        for s in (0.99, 1.01):
            assert f >= lml(dict(best, **{k: s * best[k]})), (k, s)
    ex = pred.export_model()
    assert ex['sig'] == pred.sig and ex['lam'] == pred._lam and np.array_equal(ex['alphas_F'], pred._alphas_F)
    alphas = pred._ctx.chol_solve(y)  # the best point's factor is resident
    assert np.array_equal(alphas, pred._alphas_F)
    Rq = ur.queries(g)
    E1, F1 = pred.predict(Rq)
    E2, F2 = GDMLPredict(ex).predict(Rq)
    assert np.array_equal(E1, E2) and np.array_equal(F1, F2)
    # a forced failure leaves everything as it was
    state = (pred.sig, pred._lam, pred._alphas_F.copy(), pred.c)
    cov = pred.predict_uncertainty(Rq)[2]
    with pytest.raises(ValueError):
        pred.optimize_hyperparameters(r['R_train'], r['F_train'][:, :-1], params=params)
    assert (pred.sig, pred._lam, pred.c) == (state[0], state[1], state[3]) and np.array_equal(pred._alphas_F, state[2])
    assert np.array_equal(pred.predict_uncertainty(Rq)[2], cov)


def test_optimiser_restores_after_a_failure_mid_way():
    """An exception out of the ascent (forced in the second trial point) restores sig, lam, the coefficients, the prediction
    tables and a factor that gives the bits it gave before."""
    name = 'n10_p2_pbc'
    r = _ref(name, None)
    pred = GDMLPredict(r['model'])
    pred.prepare_uncertainty(r['R_train'], r['F_train'])
    Rq = ur.queries(r['g'])
    before = pred.predict_uncertainty(Rq)
    state = (pred.sig, pred._lam, pred._alphas_F.copy(), pred.uncertainty_scale, pred.c)
    ctx, calls = pred._ctx, [0]
    orig = ctx.evidence_grad

    def failing(alphas):
        calls[0] += 1
        if calls[0] == 2:
            raise RuntimeError('forced')
        return orig(alphas)

    ctx.evidence_grad = failing
    try:
        with pytest.raises(RuntimeError):
            pred.optimize_hyperparameters(r['R_train'], r['F_train'])
    finally:
        del ctx.evidence_grad
    assert calls[0] == 2
    assert (pred.sig, pred._lam, pred.uncertainty_scale, pred.c) == (state[0], state[1], state[3], state[4])
    assert np.array_equal(pred._alphas_F, state[2])
    after = pred.predict_uncertainty(Rq)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert np.isfinite(pred.evidence_gradient()['d_sig'])  # the labels of prepare_uncertainty are still there


def test_error_paths():
    g = _load('n10_p2_pbc')
    _, x, gd, tp, _ = ur.fixture_tables(g)
    n = x.shape[0] * 3 * g['R_train'].shape[1]
    sig, lam = float(g['sig']), float(g['lam'])
    alphas = np.asarray(g['alphas'], dtype=np.float64)
    c = _lib.Context()
    try:
        with pytest.raises(_lib.GDMLHipError):  # no training set
            c.evidence_grad(alphas)
        c.train_upload(x, gd, tp)
        with pytest.raises(_lib.GDMLHipError):  # no matrix at all
            c.evidence_grad(alphas)
        c.assemble_K(sig, False, for_cholesky=lam)
        with pytest.raises(_lib.GDMLHipError):  # a matrix, not factored
            c.evidence_grad(alphas)
        c.chol_factor(lam)
        terms = c.evidence_grad(alphas)  # a factor from the training path (no gdml_uncert_prepare) is accepted
        assert np.all(np.isfinite(terms))
        with pytest.raises(ValueError):  # wrong n
            c.evidence_grad(alphas[:-1])
        lib, vp = c._lib, (lambda a: a.ctypes.data_as(C.c_void_p))
        out, info = np.empty(5), C.c_int(0)
        assert lib.gdml_evidence_grad(c._h, None, n, vp(out), C.byref(info)) == -1
        assert lib.gdml_evidence_grad(c._h, vp(alphas), n, None, C.byref(info)) == -1
        assert lib.gdml_evidence_grad(c._h, vp(alphas), n, vp(out), None) == 0  # info is optional
        assert np.array_equal(out, terms)
        # the second matrix does not fit: forced through the option that bounds the memory the call may count on
        held = c.mem_info()[0]
        try:
            c.set_option('chol.evidence_mem_budget', 1024.0)
            with pytest.raises(MemoryError) as ei:
                c.evidence_grad(alphas)
            ld = (n + 15) // 16 * 16
            assert str(n * ld * 8) in str(ei.value) and '1024' in str(ei.value)
        finally:
            c.set_option('chol.evidence_mem_budget', 0)
        assert c.mem_info()[0] == held
        assert np.array_equal(c.evidence_grad(alphas), terms)
        c.assemble_K(sig)  # overwrites the factor
        with pytest.raises(_lib.GDMLHipError):
            c.evidence_grad(alphas)
    finally:
        c.close()
    # a multi-rank (virtual) communicator: the factor of such a context is distributed
    c = _lib.Context()
    try:
        c.comm_init(None, 0, 2)
        c.train_upload(x, gd, tp)
        with pytest.raises(NotImplementedError):
            c.evidence_grad(alphas)
    finally:
        c.close()
    # energy constraints: refused by the host API, and by the library for a factor that carries the energy rows
    ge = _load('n5_p2_ecstr')
    me = ur.model_from_fixture(ge)
    pe = GDMLPredict(me)
    with pytest.raises(NotImplementedError):
        pe.evidence_gradient()
    with pytest.raises(NotImplementedError):
        pe.optimize_hyperparameters(ge['R_train'], ge['F_train'])
    ce = pe._ctx
    ce.train_upload(ge['R_desc'], ge['R_d_desc'], pe._tril_perms)
    ce.assemble_K(me['sig'], True, for_cholesky=me['lam'])
    ce.chol_factor(me['lam'])
    with pytest.raises(NotImplementedError):  # GDML_ERR_UNSUPPORTED
        ce.evidence_grad(np.zeros(ge['R_desc'].shape[0] * 15))
    # no labels anywhere
    p0 = GDMLPredict(ur.model_from_fixture(g))
    p0.prepare_uncertainty(np.asarray(g['R_train'], dtype=np.float64).reshape(x.shape[0], -1))
    with pytest.raises(ValueError):
        p0.evidence_gradient()

"""Parity record of the vibrational analysis (profiles/vib_parity.json): the measured errors of gdml_sym_eig against LAPACK per
matrix order and of GDMLPredict.vibrations against the NumPy restatement per fixture, beside their bounds (the cases and checks
of tests/test_vib_gpu.py, whose helpers this runs), and the bit comparison of gdml_sym_eig_absv between two builds of the
library.

    python tools/vib_parity.py --absv-dump FILE.npz [--lib libgdml_hip.so]     one gdml_sym_eig_absv call at N = 21, 100, 150 on
                                                             that build of the library, results into FILE.npz
    python tools/vib_parity.py [--absv A.npz B.npz] [--out profiles/vib_parity.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

ABSV_SIZES = (21, 100, 150)


def absv_inputs(N, M=4):
    """Distance matrices of M random geometries of N atoms."""
    r = np.random.RandomState(N).standard_normal((M, N, 3)) * N ** (1.0 / 3.0)
    return np.sqrt(((r[:, :, None, :] - r[:, None, :, :]) ** 2).sum(-1))


def absv_dump(path, lib_path):
    """Plain ctypes on the four symbols involved: a parent build's library lacks the newer entries the binding asks for."""
    import ctypes as C

    lib = C.CDLL(lib_path)
    h = C.c_void_p()
    assert lib.gdml_ctx_create(0, C.byref(h)) == 0
    out = {}
    for N in ABSV_SIZES:
        adj = np.ascontiguousarray(absv_inputs(N))
        v = np.empty_like(adj)
        rc = lib.gdml_sym_eig_absv(h, adj.ctypes.data_as(C.c_void_p), C.c_int64(len(adj)), C.c_int(N), v.ctypes.data_as(C.c_void_p))
        assert rc == 0, rc
        out['n%d' % N] = v
    lib.gdml_ctx_destroy(h)
    np.savez(path, **out)


def measure():
    import _hessian_ref as hr
    import _vib_ref as vr
    import test_vib_gpu as tv
    from sgdml_amd.predict import GDMLPredict

    ctx = tv._ctx()
    eig = []
    for n in tv.EIG_SIZES:
        A = np.concatenate([tv.eig_inputs(n), tv.eig_special(n)])
        w, V, sweeps = ctx.sym_eig(A)
        errs = np.array([vr.eig_errors(A[m], w[m], V[m]) for m in range(len(A))])
        bnd = np.array([vr.bound(n, A[m]) for m in range(len(A))])
        ok = bnd > 0.0
        eig.append(dict(n=n, matrices=len(A), sweeps_max=int(sweeps.max()),
                        eigenvalue_error_over_bound=float((errs[ok, 0] / bnd[ok]).max()),
                        residual_over_bound=float((errs[ok, 1] / bnd[ok]).max()),
                        orthogonality=float(errs[:, 2].max()), orthogonality_bound=40.0 * n * vr.EPS))
    fixtures = []
    for name in tv.FIXTURES:
        g = tv._load(name)
        model, _, lat = hr.model_from_fixture(g)
        pred = GDMLPredict(model)
        R = tv._geoms(g)[:2 if name == 'n100_m3' else 7]
        m = vr.fixture_masses(len(model['z']))
        worst = tv.vib_check(pred, model, R, m, lat=lat)
        out = pred.vibrations(R, m)
        fixtures.append(dict(fixture=name, n=int(R.shape[1]), geometries=len(R), w2_error_over_bound=float(worst),
                             n_rigid=int(out['n_rigid'][0]), sweeps_max=int(out['sweeps'].max())))
    return dict(bound='40 n eps |A|_F (eigenvalues, residuals); 40 n eps (orthogonality)', sym_eig=eig, vibrations=fixtures)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--absv-dump')
    ap.add_argument('--lib', default=os.path.join(ROOT, 'sgdml_amd', 'libgdml_hip.so'))
    ap.add_argument('--absv', nargs=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vib_parity.json'))
    a = ap.parse_args()
    if a.absv_dump:
        absv_dump(a.absv_dump, a.lib)
        sys.exit(0)
    res = measure()
    if a.absv:
        x, y = np.load(a.absv[0]), np.load(a.absv[1])
        res['sym_eig_absv_parent_vs_this'] = {k: dict(array_equal=bool(np.array_equal(x[k], y[k])),
                                                      max_abs_difference=float(np.abs(x[k] - y[k]).max())) for k in sorted(x.files)}
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))

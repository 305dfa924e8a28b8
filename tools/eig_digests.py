"""SHA-256 digests of what the Jacobi eigensolver's entries and everything built on them return: the record that one kernel
template, one launcher and one plan (csrc/sym_eig.hip, csrc/sym_eig_plan.h) and the split of csrc/vib.hip by subject (vib.hip,
ef.hip) changed no output bit (tests/golden/eig_parent_digests.json, tests/test_eig_bits_gpu.py).  Only the package's public
bindings, so the same file runs against an older library (GDML_HIP_LIB selects it).

    python tools/eig_digests.py [--out tests/golden/eig_parent_digests.json]

Inputs are those of the existing tests (tests/_vib_ref.py: eig_inputs, eig_special, geoms; tools/vib_parity.py: absv_inputs;
tests/_ef_ref.py: parity_start and the PARITY_* settings; tests/golden/perm_c3.npz as tests/test_hip_r6.py matches it).
  eig      gdml_sym_eig on eig_inputs(n) and eig_special(n), n in EIG_N (odd and even, every storage route, both sides of
           100 | 101 and 141 | 142): w, V, sweeps, and w, sweeps of the call without vectors; M = 1100 at n = 3 (the grid stride)
  eigdev   gdml_sym_eig_dev, n in 8, 101, 150: w, V, sweeps out of place, then V in place over A without sweeps
  absv     gdml_sym_eig_absv on absv_inputs(N), N in ABSV_N; M = 1100 at N = 3
  perm     gdml_perm_match without eigenvectors on the three cases of perm_c3.npz: the cost matrix, and the kept pairs and their
           assignments sorted by pair (the device appends them in no particular order)
  vib      vibrations() with modes on seven geometries of VIB_FIXTURES, every allowed projection x predict.vib_chunk 0, 1, 3;
           n100_m3 (n3 = 300: the device-memory route) with two geometries, the default projection, predict.vib_chunk 0 and 1
  ef       stationary_point() on the first three parity starts of every PARITY_FIXTURES x PARITY_MODES x predict.vib_chunk 0, 1
           with record_every = 1: every array returned (end state, end outputs, histories, frames).  PARITY_N_EVAL evaluations;
           two on n100_m3, where one takes most of a second (the first takes the step without a predecessor, the second is
           the last of the run)"""
import argparse
import ctypes as C
import functools
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import _ef_ref as er  # noqa: E402
import _hessian_ref as hr  # noqa: E402
import _vib_ref as vr  # noqa: E402
import vib_parity  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
EIG_N = (1, 2, 3, 8, 63, 64, 100, 101, 141, 142, 150)
EIGDEV_N = (8, 101, 150)
ABSV_N = (2, 3, 21, 100, 101, 141, 142, 150)
STRIDE_M = 1100
VIB_FIXTURES = ('n6_p1', 'n5_p4', 'n10_p2_pbc', 'cfg1_n21_m100')
VIB_CHUNKS = (0, 1, 3)
EF_CHUNKS = (0, 1)


def case_ids():
    ids = ['eig-n%d' % n for n in EIG_N] + ['eig-n3-M%d' % STRIDE_M]
    ids += ['eigdev-n%d' % n for n in EIGDEV_N]
    ids += ['absv-N%d' % n for n in ABSV_N] + ['absv-N3-M%d' % STRIDE_M, 'perm']
    ids += ['vib-%s' % f for f in VIB_FIXTURES + ('n100_m3',)]
    ids += ['ef-%s-order%d-follow%d-chunk%d' % (f, o, int(t), c) for f in er.PARITY_FIXTURES for o, t in er.PARITY_MODES for c in EF_CHUNKS]
    return ids


def _sha(a):
    a = np.asarray(a)
    return hashlib.sha256(np.ascontiguousarray(a, dtype='<i8' if a.dtype.kind in 'iub' else '<f8').tobytes()).hexdigest()


def _flat(d, pre=''):
    """{path: digest} of every array in a nested dict; a missing one (None) is recorded as such."""
    out = {}
    for k in sorted(d):
        v = d[k]
        if isinstance(v, dict):
            out.update(_flat(v, pre + k + '.'))
        else:
            out[pre + k] = 'none' if v is None else _sha(v)
    return out


def _eig(ctx, n, M=None):
    d = {}
    for tag, A in (('random', vr.eig_inputs(n, M) if M else vr.eig_inputs(n)),) + ((('special', vr.eig_special(n)),) if not M else ()):
        w, V, sw = ctx.sym_eig(A)
        w0, _, sw0 = ctx.sym_eig(A, vectors=False)
        d.update({tag + '|w': _sha(w), tag + '|V': _sha(V), tag + '|sweeps': _sha(sw), tag + '|w_only': _sha(w0),
                  tag + '|sweeps_only': _sha(sw0)})
    return d


def _eigdev(ctx, n):
    lib = ctx._lib
    A = vr.eig_inputs(n)
    M = len(A)
    ptrs = [C.c_void_p() for _ in range(4)]
    for p, s in zip(ptrs, [A.nbytes, M * n * 8, A.nbytes, M * 8]):
        ctx._check(lib.gdml_dev_alloc(ctx._h, s, C.byref(p)))
    try:
        ctx._check(lib.gdml_memcpy_h2d(ctx._h, ptrs[0], A.ctypes.data_as(C.c_void_p), A.nbytes))
        ctx.sym_eig_dev(ptrs[0], M, n, ptrs[1], ptrs[2], ptrs[3])
        out = [np.empty((M, n)), np.empty((M, n, n)), np.empty(M, dtype=np.int64)]
        for p, o in zip(ptrs[1:], out):
            ctx._check(lib.gdml_memcpy_d2h(ctx._h, o.ctypes.data_as(C.c_void_p), p, o.nbytes))
        d = dict(w=_sha(out[0]), V=_sha(out[1]), sweeps=_sha(out[2]))
        ctx.sym_eig_dev(ptrs[0], M, n, ptrs[1], ptrs[0], None)  # in place (V over A), without sweeps
        ctx._check(lib.gdml_memcpy_d2h(ctx._h, out[0].ctypes.data_as(C.c_void_p), ptrs[1], out[0].nbytes))
        ctx._check(lib.gdml_memcpy_d2h(ctx._h, out[1].ctypes.data_as(C.c_void_p), ptrs[0], out[1].nbytes))
        d.update(w_inplace=_sha(out[0]), V_inplace=_sha(out[1]))
        return d
    finally:
        for p in ptrs:
            lib.gdml_dev_free(ctx._h, p)


def _perm(ctx):
    from sgdml_amd.utils import perm

    g = np.load(os.path.join(GOLDEN, 'perm_c3.npz'))
    lat = g['lat']
    d = {}
    for name, R, z, li in (('c3', g['R'], g['z'], None), ('c3_small', g['R2'], g['z2'], None),
                           ('c3_small_lattice', g['R2'], g['z2'], (lat, np.linalg.inv(lat)))):
        adj = perm._dist_matrices(np.asarray(R, dtype=float), li)
        _, species = np.unique(np.asarray(z), return_inverse=True)
        cost, ij, pm = ctx.perm_match(None, adj, species)
        order = np.lexsort((ij[:, 1], ij[:, 0]))
        d.update({name + '|cost': _sha(cost), name + '|ij': _sha(ij[order]), name + '|perms': _sha(pm[order])})
    return d


@functools.lru_cache(maxsize=None)
def _predictor(name):
    from sgdml_amd.predict import GDMLPredict

    g = dict(np.load(os.path.join(GOLDEN, name + '.npz')))
    model, _, lat = hr.model_from_fixture(g)
    return GDMLPredict(model), vr.geoms(g), len(model['z']), lat


def _vib(name):
    pred, R7, N, lat = _predictor(name)
    m = vr.fixture_masses(N)
    big = name == 'n100_m3'
    R = R7[:2] if big else R7
    projections = (None,) if big else (('none', 'trans') if lat is not None else ('none', 'trans', 'rigid'))
    d = {}
    try:
        for chunk in (0, 1) if big else VIB_CHUNKS:
            pred._ctx.set_option('predict.vib_chunk', chunk)
            for pj in projections:
                d.update(_flat(pred.vibrations(R, m, project=pj, modes=True), 'chunk%d|%s|' % (chunk, pj or 'default')))
    finally:
        pred._ctx.set_option('predict.vib_chunk', 0)
    return d


def _ef(name, order, with_follow, chunk):
    pred = _predictor(name)[0]
    _, R0, follow = er.parity_start(name)
    n_eval = 2 if name == 'n100_m3' else er.PARITY_N_EVAL
    try:
        pred._ctx.set_option('predict.vib_chunk', chunk)
        out = pred.stationary_point(R0[:3], er.PARITY_FMAX, order=order, follow=follow[:3] if with_follow else None,
                                    max_steps=n_eval - 1, record_every=1, **er.PARITY_TRUST)
    finally:
        pred._ctx.set_option('predict.vib_chunk', 0)
    return _flat(out)


def digests(case_id, ctx=None):
    """{output name: sha256} of one case.  ctx: the context of the eigensolver cases (the fixtures bring their predictors')."""
    from sgdml_amd import _lib

    tok = case_id.split('-')
    if tok[0] == 'vib':
        return _vib(tok[1])
    if tok[0] == 'ef':
        return _ef(tok[1], int(tok[2][5:]), bool(int(tok[3][6:])), int(tok[4][5:]))
    own = ctx is None
    if own:
        ctx = _lib.Context(0)
    try:
        M = int(tok[2][1:]) if len(tok) > 2 else None
        if tok[0] == 'eig':
            return _eig(ctx, int(tok[1][1:]), M)
        if tok[0] == 'eigdev':
            return _eigdev(ctx, int(tok[1][1:]))
        if tok[0] == 'absv':
            N = int(tok[1][1:])
            return dict(absv=_sha(ctx.sym_eig_absv(vib_parity.absv_inputs(N, M) if M else vib_parity.absv_inputs(N))))
        assert case_id == 'perm', case_id
        return _perm(ctx)
    finally:
        if own:
            ctx.close()


if __name__ == '__main__':
    import time

    from sgdml_amd import _lib

    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(GOLDEN, 'eig_parent_digests.json'))
    a = ap.parse_args()
    out = {}
    c = _lib.Context(0)
    for cid in case_ids():
        t0 = time.time()
        out[cid] = digests(cid, c)
        print(cid, len(out[cid]), '%.2f s' % (time.time() - t0), flush=True)
    c.close()
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')

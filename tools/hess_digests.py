"""SHA-256 digests of what predict_hessian, predict and predict_virial return on seeded synthetic models: the record that a
refactor of csrc/predict_hess.hip or of the predict epilogues changed no output bit (tests/golden/hess_parent_digests.json,
tests/test_hess_bits_gpu.py).  Only the Python API and the options a test may set, so the same file runs against an older
checkout (GDML_HIP_LIB selects the library).

    python tools/hess_digests.py [--out tests/golden/hess_parent_digests.json]

Hessian cases (models of tests/_hessian_ref.py: row_case / size_case, geometries as in its grid): chunked rows at N = 12 (wave
variant) and N = 33 (block variant, one and two batch slices), each also with predict.hess_generic = 1; N = 139 | 140 (v in
LDS | in memory at KT = 48) and N = 158 (KT = 0).  Prediction cases (synth_model, one with a lattice and one with alphas_E):
N = 3 and 12 at M P = 16, 128, 144 rows and B = 1 and 3 queries -- 1, 8 and 9 row splits, i.e. below, on and just past a batch
of eight of the epilogue's sums -- with predict.fused = 0, so that the batched route and its epilogue serve them; N = 129
(D = 8256 > 8192: the epilogue that reads F_x in place) with a one-geometry model."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _hessian_ref as hr  # noqa: E402

HESS_ROWS = [(12, 130, 3, 40), (33, 265, 1, 128), (33, 600, 65, 100)]  # N, M P, B, predict.hess_chunk_rows
HESS_SIZES = [139, 140, 158]  # B = 2
PRED_N, PRED_MP, PRED_B = (3, 12), (16, 128, 144), (1, 3)
PRED_WIDE = (129, 1, 2)  # N, M (the smallest the model builder takes), B


def case_ids():
    ids = ['hess-rows-n%d-mp%d-b%d-c%d-g%d' % (c + (g,)) for c in HESS_ROWS for g in (0, 1)]
    ids += ['hess-size-n%d' % N for N in HESS_SIZES]
    ids += ['pred-n%d-mp%d-%s' % (N, MP, kind) for N in PRED_N for MP in PRED_MP for kind in ('lattice', 'aE')]
    return ids + ['pred-wide-n%d' % PRED_WIDE[0]]


def _sha(a):
    a = np.ascontiguousarray(a, dtype='<f8')
    return hashlib.sha256(a.tobytes()).hexdigest()


def _with_options(pred, opts, fn):
    try:
        for k, v in opts.items():
            pred._ctx.set_option(k, v)
        return fn()
    finally:
        for k in opts:
            pred._ctx.set_option(k, 1 if k == 'predict.fused' else 0)


def _predict_digests(pred, R):
    def run():
        E, F = pred.predict(R)
        Ev, Fv, W = pred.predict_virial(R)
        return dict(E=_sha(E), F=_sha(F), E_virial=_sha(Ev), F_virial=_sha(Fv), W=_sha(W))

    return _with_options(pred, {'predict.fused': 0}, run)


def digests(case_id):
    """{output name: sha256} of one case; a prediction case holds one entry per batch size."""
    from sgdml_amd.predict import GDMLPredict

    tok = case_id.split('-')
    num = lambda t: int(t.lstrip('nmpbcg'))  # noqa: E731
    if tok[0] == 'hess':
        if tok[1] == 'rows':
            N, MP, B, chunk, generic = (num(t) for t in tok[2:])
            case = hr.row_case(N, MP)
        else:
            N, B, chunk, generic = num(tok[2]), 2, 0, 0
            case = hr.size_case(N)
        model, R5, _ = hr.grid_model(**case)
        R = np.ascontiguousarray(R5[hr.batch_index(B)])
        pred = GDMLPredict(model)
        E, F, H = _with_options(pred, {'predict.hess_generic': generic, 'predict.hess_chunk_rows': chunk},
                                lambda: pred.predict_hessian(R))
        return dict(E=_sha(E), F=_sha(F), H=_sha(H))
    if tok[1] == 'wide':
        N, M, B = PRED_WIDE
        model, _, Rq = hr.synth_model(N, M, lattice=True, seed=N)
        return _predict_digests(GDMLPredict(model), Rq[:B])
    N, MP, kind = num(tok[1]), num(tok[2]), tok[3]
    model, _, Rq = hr.synth_model(N, MP, with_aE=kind == 'aE', lattice=kind == 'lattice', seed=1000 * N + MP)
    pred = GDMLPredict(model)
    return {'B%d_%s' % (B, k): v for B in PRED_B for k, v in _predict_digests(pred, Rq[:B]).items()}


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'hess_parent_digests.json'))
    a = ap.parse_args()
    out = {}
    for cid in case_ids():
        out[cid] = digests(cid)
        print(cid, json.dumps(out[cid]), flush=True)
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')

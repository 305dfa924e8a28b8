"""SHA-256 digests of what the Nystroem build, the three forms of the preconditioner application and gdml_pcg return: the
record that splitting csrc/cg.hip by stage (gram_tn.hip, chol_solve.hip, nystroem.hip, precon_apply.hip, cg.hip) around
csrc/precon_plan.h changed no output bit (tests/golden/nys_parent_digests.json, tests/test_nys_bits_gpu.py).  Only
sgdml_amd._lib and the options a test may set, so the same file runs against an older library (GDML_HIP_LIB selects it).

    python tools/nys_digests.py [--out tests/golden/nys_parent_digests.json]

Matrices and loader are those of the edge tests (tests/_nys_ref.py: case_matrix, load_nystroem, which sets the pitch padding and
the work block to NaN).  Hashed is the meaningful region only: rows [0, n) x columns [0, m) of the factor, the lower triangle
of L, the float overlay and its pad for the in-place fp32 form, the scores, the applications, the info word -- never pitch
padding or the scratch upper triangle.
  gram    (270, 257); (16392, 129) with nys.syrk_split 1 and 0: X1 and L of the first stage
  solve   (594, m), m = 63, 513, 576, nys.trsm_left 1 and 0: X1, L, X2, scores
  gemv64  (2100, 131), (594, 525), (13, 1), pcg.gemv_plain 0 and 1: X2, scores, P v
  f32     (594, m), m = 129 ... 132, 525: pcg.f32_inplace 0 / 1 x pcg.f32_gram_rows 2048 / 256 x every entry of F32_APPLY
  qr      (594, 513) with nys.force_qr
  mf      the really assembled system of _nys_ref.mf_system
  pcg     fixture pcg_n9_m400, set up as test_pcg_solves_system does: pcg.depth 0 and 2, with and without the preconditioner,
          a warm start, a stop from the callback at iteration 3: iterate, iteration count, final residual, residual history"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _nys_ref as nr  # noqa: E402

GRAM = [(270, 257, 1), (16392, 129, 1), (16392, 129, 0)]  # n, m, nys.syrk_split
SOLVE_M = (63, 513, 576)
GEMV64 = [(2100, 131), (594, 525), (13, 1)]
F32_M = (129, 130, 131, 132, 525)
F32_GRAM_ROWS = (2048, 256)
QR = (594, 513)
PCG_FIXTURE = 'pcg_n9_m400'


def case_ids():
    ids = ['gram-n%d-m%d-split%d' % c for c in GRAM]
    ids += ['solve-n%d-m%d-left%d' % (nr.SOLVE_N, m, lf) for m in SOLVE_M for lf in (1, 0)]
    ids += ['gemv64-n%d-m%d-plain%d' % (n, m, p) for n, m in GEMV64 for p in (0, 1)]
    ids += ['f32-n%d-m%d' % (nr.F32_N, m) for m in F32_M]
    return ids + ['qr-n%d-m%d' % QR, 'mf', 'pcg']


def _sha(a, dtype='<f8'):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=dtype).tobytes()).hexdigest()


def _word(i):
    return _sha([int(i)], '<i8')


def _key(opts):
    return ','.join('%s=%g' % kv for kv in sorted(opts.items())) or 'default'


def _factor(ctx, n, m, lam=nr.LAM):
    """Load the case and factor it; returns (info, the (n + m) x m buffer read back)."""
    K, idx = nr.case_matrix(n, m, 'a', 0)
    nr.load_nystroem(ctx, n, idx, K)
    _, _, info = ctx.nystroem_factor(lam, idx, want_factor=False, want_lev=False)
    return info, ctx.K_to_host()


def _stages(ctx, n, m, opts, second):
    """Form 1 without scores leaves X1 and L in the buffer; the scores then bring the second solve."""
    with nr.options(ctx, dict(opts, **{'pcg.precon_form': 1})):
        info, H = _factor(ctx, n, m)
        d = dict(info=_word(info), X1=_sha(H[:n]), L=_sha(np.tril(H[n:n + m])))
        if second:
            d['lev'] = _sha(ctx.nystroem_lev_scores())
            d['X2'] = _sha(ctx.K_to_host()[:n])
    return d


def _form0(ctx, n, m, opts):
    v = nr.vec(n, 0)
    with nr.options(ctx, dict(opts, **{'pcg.precon_form': 0})):
        info, H = _factor(ctx, n, m)
        return dict(info=_word(info), X2=_sha(H[:n]), L=_sha(np.tril(H[n:n + m])), Pv=_sha(ctx.precon_apply(nr.LAM, v)),
                    lev=_sha(ctx.nystroem_lev_scores()))


def _f32(ctx, n, m):
    v = nr.vec(n, 0)
    d = {}
    for rows in F32_GRAM_ROWS:
        for inplace in (0, 1):
            pre = 'rows%d|inplace%d|' % (rows, inplace)
            with nr.options(ctx, {'pcg.precon_form': 3, 'pcg.f32_inplace': inplace, 'pcg.f32_gram_rows': rows}):
                info, H = _factor(ctx, n, m)
                d[pre + 'info'] = _word(info)
                d[pre + 'L'] = _sha(np.tril(H[n:n + m]))
                d[pre + 'min_pivot'] = _sha([ctx.get_option('pcg.f32_last_min_pivot')])
                if inplace:
                    X32, pad = nr._f32_overlay(ctx, n, m)
                    d[pre + 'X32'], d[pre + 'pad'] = _sha(X32, '<f4'), _sha(pad, '<f4')
                else:
                    d[pre + 'X2'] = _sha(H[:n])
                d[pre + 'lev'] = _sha(ctx.nystroem_lev_scores())
                for ap in nr.F32_APPLY:
                    with nr.options(ctx, ap):
                        d[pre + 'Pv|' + _key(ap)] = _sha(ctx.precon_apply(nr.LAM, v))
    return d


def _mf(ctx):
    xd, gd, tp, K_nm, idx, _ = nr.mf_system(0)
    v = nr.vec(len(K_nm), 0)
    with nr.options(ctx, {'pcg.precon_form': 1}):
        ctx.train_upload(xd, gd, tp)
        ctx.assemble_K(nr.MF['sig'], False, idx=idx, alloc_extra_rows=len(idx))
        _, _, info = ctx.nystroem_factor(nr.MF['lam'], idx, want_factor=False, want_lev=False)
        return dict(info=_word(info), Pv=_sha(ctx.precon_apply(nr.MF['lam'], v)))


def _pcg(ctx):
    from oracle import gdml_oracle as orc

    g = dict(np.load(os.path.join(ROOT, 'tests', 'golden', PCG_FIXTURE + '.npz'), allow_pickle=True))
    M, N = g['R_train'].shape[:2]
    sig, lam, y, idx = float(g['sig']), float(g['lam']), g['y'], g['inducing_pts_idxs']
    tp = orc.tril_perms_from_atom_perms(g['perms'])
    xd, gd = ctx.desc_from_R(g['R_train'].reshape(M, -1), N)
    ctx.train_upload(xd, gd, tp)
    ctx.assemble_K(sig, False, idx=idx, alloc_extra_rows=len(idx))
    _, _, info = ctx.nystroem_factor(lam, idx)
    ctx.predict_upload_model(xd, np.zeros_like(xd), tp, sig, None)
    d = dict(info=_word(info))

    def run(tag, **kw):
        hist = []
        stop_at = kw.pop('stop_at', None)
        x, inf, iters, resid = ctx.pcg(lam, False, y, callback=lambda it, r, fetch_x: hist.append(r) or it == stop_at, **kw)
        d.update({tag + '|x': _sha(x), tag + '|iters': _word(iters), tag + '|info': _word(inf), tag + '|resid': _sha([resid]),
                  tag + '|hist': _sha(hist)})
        return x

    try:
        for depth in (0, 2):
            ctx.set_option('pcg.depth', depth)
            run('depth%d|precon' % depth, rtol=1e-4, maxiter=5000)
            run('depth%d|plain' % depth, rtol=1e-4, maxiter=40, use_precon=False)  # (cond ~ 1e10: 40 iterations of it)
            x10 = run('depth%d|ten' % depth, rtol=1e-12, maxiter=10)
            run('depth%d|warm' % depth, rtol=1e-4, maxiter=5000, x0=x10)
            run('depth%d|stop3' % depth, rtol=1e-12, maxiter=50, stop_at=3)
    finally:
        ctx.set_option('pcg.depth', 2)
    return d


def digests(case_id, ctx=None):
    """{output name: sha256} of one case."""
    from sgdml_amd import _lib

    own = ctx is None
    if own:
        ctx = _lib.Context(0)
    try:
        tok = case_id.split('-')
        num = [int(t.lstrip('nmsplitefa')) for t in tok[1:]]
        if tok[0] == 'gram':
            return _stages(ctx, num[0], num[1], {'nys.syrk_split': num[2]}, second=False)
        if tok[0] == 'solve':
            return _stages(ctx, num[0], num[1], {'nys.trsm_left': num[2]}, second=True)
        if tok[0] == 'gemv64':
            return _form0(ctx, num[0], num[1], {'pcg.gemv_plain': num[2]})
        if tok[0] == 'f32':
            return _f32(ctx, num[0], num[1])
        if tok[0] == 'qr':
            return _form0(ctx, num[0], num[1], {'nys.force_qr': 1})
        return _mf(ctx) if case_id == 'mf' else _pcg(ctx)
    finally:
        for k, v in nr.options.DEFAULTS.items():
            ctx.set_option(k, v)
        if own:
            ctx.close()


if __name__ == '__main__':
    from sgdml_amd import _lib

    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'nys_parent_digests.json'))
    a = ap.parse_args()
    out = {}
    c = _lib.Context(0)
    for cid in case_ids():
        out[cid] = digests(cid, c)
        print(cid, len(out[cid]), flush=True)
    c.close()
    with open(a.out, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write('\n')

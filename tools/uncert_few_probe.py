"""Low-latency covariance probe: gdml_predict_cov_few_dev against gdml_predict_cov_dev, one process, one prepared factor per
shape, the two entries alternating.

    python tools/uncert_few_probe.py [--shapes A,B] [--min-s 0.5] [--out FILE.json]

Shapes A (N = 21, P = 1, M = 1000) and B (N = 42, P = 27, M = 500) of tools/uncertainty_probe.py, n = 63 000 both; batches
B = 1, 2, 4 on A and 1, 2 on B (marginal variances, the default output).  Every point is warmed up, repeated at least three
times and for at least --min-s seconds and closed by a device synchronise.  The old path is timed in three separate blocks
(each block: every batch size, old then new), so that its own spread is on file; the new path's three values are kept as well.
Phase times come from further calls with the library's per-kernel event timers on: once with the solve timed as a whole
("few_solve"), once with its two per-step kernels timed one by one (the events then slow the solve down: those two figures say
where the time goes, not how long the solve takes).  Work is algorithmic: n^2 3N B flops for the solve, n^2 / 2 * 8 bytes for the
factor read once; floor = max(bytes / 8 TB/s, flops / 78.6 TFLOP/s).  The per-geometry cost of the old path at B = 64 comes
from the same run."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench import perm_group, synth_geometries  # noqa: E402
from oracle import gdml_oracle as orc  # noqa: E402
from sgdml_amd import _lib  # noqa: E402
from uncertainty_probe import PEAK_FP64, PEAK_HBM, SHAPES, _timed  # noqa: E402

BATCHES = {'A': [1, 2, 4], 'B': [1, 2]}


def run_shape(key, min_s, sig=20.0, lam=1e-10, seed=0):
    N, kind, M = SHAPES[key]
    n3 = 3 * N
    n = n3 * M
    R, _, _ = synth_geometries(N, M + 8, seed=seed)
    R = R.reshape(M + 8, -1)
    perms = perm_group(N, kind)
    tp = orc.tril_perms_from_atom_perms(perms)
    ctx = _lib.Context(0)
    xd, gd = ctx.desc_from_R(R[:M], N)
    ctx.train_upload(xd, gd, tp)
    ctx.uncert_prepare(sig, lam)
    ctx.sync()
    head = {'shape': key, 'N': N, 'P': len(perms), 'M': M, 'n': n}
    lib, h = ctx._lib, ctx._h
    bufs = {}
    for B in BATCHES[key] + [64]:
        Rq = np.ascontiguousarray(np.resize(R[M:], (B, n3)))
        pR, pV = C.c_void_p(), C.c_void_p()
        ctx._check(lib.gdml_dev_alloc(h, Rq.nbytes, C.byref(pR)))
        ctx._check(lib.gdml_dev_alloc(h, B * n3 * 8, C.byref(pV)))
        ctx._check(lib.gdml_memcpy_h2d(h, pR, Rq.ctypes.data_as(C.c_void_p), Rq.nbytes))
        bufs[B] = (pR, pV)
    out = []
    try:
        old = {B: [] for B in BATCHES[key]}
        new = {B: [] for B in BATCHES[key]}
        for _ in range(3):
            for B in BATCHES[key]:
                pR, pV = bufs[B]
                old[B].append(_timed(lambda: ctx.predict_cov_dev(pR, B, pV), ctx.sync, min_s)[0])
                new[B].append(_timed(lambda: ctx.predict_cov_few_dev(pR, B, pV), ctx.sync, min_s)[0])
        pR, pV = bufs[64]
        ms64 = _timed(lambda: ctx.predict_cov_dev(pR, 64, pV), ctx.sync, min_s)[0]
        for B in BATCHES[key]:
            pR, pV = bufs[B]
            ctx.profile(True)
            ctx.predict_cov_few_dev(pR, B, pV)
            ctx.sync()
            ph = {k: ctx.kernel_stat('few_' + k)[0] for k in ('cross', 'inv', 'solve', 'gram')}
            launches = ctx.phase_ms('uncert_few')[1]
            ctx.profile(False)
            ctx.set_option('predict.cov_few_split_timers', 1)
            ctx.profile(True)
            ctx.predict_cov_few_dev(pR, B, pV)
            ctx.sync()
            sp = {k: ctx.kernel_stat('few_' + k)[:2] for k in ('diag', 'upd')}
            ctx.profile(False)
            ctx.set_option('predict.cov_few_split_timers', 0)
            ctx.profile(True)
            ctx.predict_cov_dev(pR, B, pV)
            ctx.sync()
            po = {k: ctx.kernel_stat('uncert_' + k)[0] for k in ('cross', 'solve', 'gram')}
            ctx.profile(False)
            fl, by = float(n) * n * n3 * B, 0.5 * n * n * 8
            floor_b, floor_f = by / PEAK_HBM * 1e3, fl / PEAK_FP64 * 1e3
            ms_old, ms_new = float(np.median(old[B])), float(np.median(new[B]))
            rec = dict(head, B=B, rows=n3 * B, ms_old_blocks=old[B], ms_new_blocks=new[B], ms_old=ms_old, ms_new=ms_new,
                       old_spread_ms=max(old[B]) - min(old[B]), speedup=ms_old / ms_new, launches_new=launches,
                       ms_few_cross=ph['cross'], ms_few_inv=ph['inv'], ms_few_solve=ph['solve'], ms_few_gram=ph['gram'],
                       ms_few_diag_sum=sp['diag'][0], few_diag_launches=sp['diag'][1], ms_few_upd_sum=sp['upd'][0],
                       few_upd_launches=sp['upd'][1], ms_old_cross=po['cross'], ms_old_solve=po['solve'], ms_old_gram=po['gram'],
                       solve_factor_gbs=by / ph['solve'] * 1e-6, solve_tflops=fl / ph['solve'] * 1e-9,
                       floor_ms=max(floor_b, floor_f), floor_bound='hbm' if floor_b >= floor_f else 'mfma',
                       solve_frac_of_floor=max(floor_b, floor_f) / ph['solve'], ms_old_B64=ms64, ms_old_B64_per_geometry=ms64 / 64,
                       new_over_old_B64_per_geometry=ms_new / B / (ms64 / 64))
            print(json.dumps(rec), flush=True)
            out.append(rec)
    finally:
        for pR, pV in bufs.values():
            lib.gdml_dev_free(h, pR)
            lib.gdml_dev_free(h, pV)
    ctx.uncert_release()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='A,B')
    ap.add_argument('--min-s', type=float, default=0.5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    _lib.preflight()
    recs = []
    for key in a.shapes.split(','):
        recs += run_shape(key, a.min_s)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump({'peak_fp64_tflops': PEAK_FP64 * 1e-12, 'peak_hbm_tbs': PEAK_HBM * 1e-12, 'points': recs}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()

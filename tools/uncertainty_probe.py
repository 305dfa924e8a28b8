"""Posterior covariance probe: seconds of gdml_uncert_prepare and milliseconds per phase of gdml_predict_cov_dev (cross-kernel,
forward solve, Gram step) on seeded synthetic training sets.

    python tools/uncertainty_probe.py [--shapes A,B] [--batches 1,16,64] [--min-s 0.5] [--out FILE.json]

prepare (assembly of A = -K + lam I and its Cholesky factorisation) is timed by the host clock around the call, after one
warm-up call, median of three.  Every predict_cov point (marginal variances, the default output) is warmed up, repeated at
least three times and for at least --min-s seconds, and closed by a
device synchronise; the phase times come from one further call with the library's per-kernel event timers on (the phases
run back to back on one stream, so they add up to the call).  Work is algorithmic: the solve n^2 3N B flops against the
fp64 MFMA peak and, for its memory floor, the n^2 / 2 * 8 bytes of the factor read once; the Gram step in this mode is
row square-norms, so it is rated by the bytes of Z it reads, the cross-kernel by the bytes it writes."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import perm_group, synth_geometries  # noqa: E402
from oracle import gdml_oracle as orc  # noqa: E402
from sgdml_amd import _lib  # noqa: E402

SHAPES = {'A': (21, None, 1000), 'B': (42, 'c3x3', 500)}  # N, permutation group, M (A: bench configs[1], n = 63 000)
PEAK_FP64 = 78.6e12
PEAK_HBM = 8.0e12


def _timed(fn, sync, min_s):
    fn()
    sync()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        sync()
        dt = time.perf_counter() - t0
        if dt >= min_s and n >= 3:
            return dt / n * 1e3, n


def run_shape(key, batches, min_s, sig=20.0, lam=1e-10, seed=0):
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
    prep = []
    for _ in range(4):
        ctx.sync()
        t0 = time.perf_counter()
        ctx.uncert_prepare(sig, lam)
        ctx.sync()
        prep.append(time.perf_counter() - t0)
    head = {'shape': key, 'N': N, 'P': len(perms), 'M': M, 'n': n, 'prepare_s_first': prep[0], 'prepare_s': float(np.median(prep[1:])),
            'assemble_ms': ctx.phase_ms('assemble')[0], 'factor_ms': ctx.phase_ms('factor')[0]}
    print(json.dumps(head), flush=True)
    lib, h = ctx._lib, ctx._h
    out = []
    for B in batches:
        Rq = np.ascontiguousarray(np.resize(R[M:], (B, n3)))
        pR, pV = C.c_void_p(), C.c_void_p()
        ctx._check(lib.gdml_dev_alloc(h, Rq.nbytes, C.byref(pR)))
        ctx._check(lib.gdml_dev_alloc(h, B * n3 * 8, C.byref(pV)))
        try:
            ctx._check(lib.gdml_memcpy_h2d(h, pR, Rq.ctypes.data_as(C.c_void_p), Rq.nbytes))
            ms, reps = _timed(lambda: ctx.predict_cov_dev(pR, B, pV), ctx.sync, min_s)
            ctx.profile(True)
            ctx.predict_cov_dev(pR, B, pV)
            ctx.sync()
            ph = {k: ctx.kernel_stat('uncert_' + k)[0] for k in ('cross', 'solve', 'gram')}
            inner = {k: ctx.kernel_stat(k)[0] for k in ('gemm_nt_sub', 'panel_trsm')}
            ctx.profile(False)
        finally:
            lib.gdml_dev_free(h, pR)
            lib.gdml_dev_free(h, pV)
        fl_solve = float(n) * n * n3 * B
        rec = dict(head, B=B, ms_call=ms, reps=reps, ms_cross=ph['cross'], ms_solve=ph['solve'], ms_gram=ph['gram'],
                   ms_solve_gemm=inner['gemm_nt_sub'], ms_solve_panel_trsm=inner['panel_trsm'],
                   solve_tflops=fl_solve / ph['solve'] * 1e-9, solve_frac_peak=fl_solve / (ph['solve'] * 1e-3) / PEAK_FP64,
                   solve_factor_gbs=0.5 * n * n * 8 / ph['solve'] * 1e-6, solve_floor_ms=0.5 * n * n * 8 / PEAK_HBM * 1e3,
                   gram_gbs=B * n3 * float(n) * 8.0 / ph['gram'] * 1e-6,
                   cross_gbs=B * M * n3 * n3 * 8.0 / ph['cross'] * 1e-6)
        print(json.dumps(rec), flush=True)
        out.append(rec)
    ctx.uncert_release()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='A,B')
    ap.add_argument('--batches', default='1,16,64')
    ap.add_argument('--min-s', type=float, default=0.5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    _lib.preflight()
    recs = []
    for key in a.shapes.split(','):
        recs += run_shape(key, [int(b) for b in a.batches.split(',')], a.min_s)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump({'peak_fp64_tflops': PEAK_FP64 * 1e-12, 'peak_hbm_tbs': PEAK_HBM * 1e-12, 'points': recs}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()

"""Leave-one-out probe: milliseconds of one gdml_loo call and of its phases (seed, solve, Gram, block solve) on seeded
synthetic training sets, against the factorisation time measured in the same run.

    python tools/loo_probe.py [--shapes A,B] [--cov none,diag] [--min-s 0.5] [--out FILE.json]

The factor comes from gdml_uncert_prepare (one warm-up, then the call whose "factor" phase time is kept).  Every gdml_loo
point is warmed up, repeated at least three times and for at least --min-s seconds by the host clock (the call ends with a
synchronising copy of its results); the phase times come from one further call with the library's per-kernel event timers
on (the phases run back to back on one stream).  The solve is rated by its algorithmic work n^3 / 3 flops against the fp64
MFMA peak; the flops it actually issues (whole 128-row tiles, c0 on the 512-column panel grid) are reported beside it.
brute_force_s is M x (assembly + factorisation) from the measured phase times -- stated, not run."""
import argparse
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


def run_shape(key, covs, min_s, sig=20.0, lam=1e-10, seed=0):
    N, kind, M = SHAPES[key]
    n3 = 3 * N
    n = n3 * M
    R, _, _ = synth_geometries(N, M, seed=seed)
    perms = perm_group(N, kind)
    tp = orc.tril_perms_from_atom_perms(perms)
    ctx = _lib.Context(0)
    xd, gd = ctx.desc_from_R(R.reshape(M, -1), N)
    ctx.train_upload(xd, gd, tp)
    for _ in range(2):
        ctx.uncert_prepare(sig, lam)
        ctx.sync()
    assemble_ms, factor_ms = ctx.phase_ms('assemble')[0], ctx.phase_ms('factor')[0]
    alphas = ctx.chol_solve(np.random.RandomState(seed).normal(size=n))
    head = {'shape': key, 'N': N, 'P': len(perms), 'M': M, 'n': n, 'assemble_ms': assemble_ms, 'factor_ms': factor_ms,
            'brute_force_s': M * (assemble_ms + factor_ms) * 1e-3}
    print(json.dumps(head), flush=True)
    out = []
    for cov in covs:
        ctx.loo(alphas, cov)
        reps, t0 = 0, time.perf_counter()
        while True:
            ctx.loo(alphas, cov)
            reps += 1
            dt = time.perf_counter() - t0
            if dt >= min_s and reps >= 3:
                break
        ms = dt / reps * 1e3
        phase_ms = ctx.phase_ms('loo')[0]
        ctx.profile(True)
        ctx.loo(alphas, cov)
        ctx.sync()
        ph = {k: ctx.kernel_stat('loo_' + k) for k in ('seed', 'solve', 'gram', 'block')}
        inner = {k: ctx.kernel_stat(k)[0] for k in ('gemm_nt_sub', 'panel_trsm')}
        ctx.profile(False)
        fl = float(n) ** 3 / 3.0
        rec = dict(head, cov=cov or 'none', ms_call=ms, reps=reps, ms_phase=phase_ms, ms_seed=ph['seed'][0], ms_solve=ph['solve'][0],
                   ms_gram=ph['gram'][0], ms_block=ph['block'][0], ms_solve_gemm=inner['gemm_nt_sub'],
                   ms_solve_panel_trsm=inner['panel_trsm'], solve_tflops=fl / ph['solve'][0] * 1e-9,
                   solve_frac_peak=fl / (ph['solve'][0] * 1e-3) / PEAK_FP64, solve_issued_over_algorithmic=ph['solve'][2] / fl,
                   call_over_factor=ms / factor_ms, brute_force_over_call=head['brute_force_s'] / (ms * 1e-3))
        print(json.dumps(rec), flush=True)
        out.append(rec)
    ctx.uncert_release()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='A,B')
    ap.add_argument('--cov', default='none,diag')
    ap.add_argument('--min-s', type=float, default=0.5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    _lib.preflight()
    recs = []
    for key in a.shapes.split(','):
        recs += run_shape(key, [None if c == 'none' else c for c in a.cov.split(',')], a.min_s)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump({'peak_fp64_tflops': PEAK_FP64 * 1e-12, 'points': recs}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()

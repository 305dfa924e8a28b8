"""Evidence-gradient probe: milliseconds of one gdml_evidence_grad call and of its phases (seed, solve, rows of A^-1,
contraction) on seeded synthetic training sets, against the factorisation time measured in the same run.

    python tools/evidence_grad_probe.py [--shapes A,B] [--min-s 0.5] [--out profiles/evidence_grad_probe.json]

The factor comes from gdml_uncert_prepare (one warm-up, then the call whose "factor" phase time is kept).  The call is warmed
up, repeated at least three times and for at least --min-s seconds by the host clock (it ends with a synchronising copy of
its results and frees its second matrix); the phase times come from one further call with the library's per-kernel event
timers on (the phases run back to back on one stream).  Every phase is reported beside the factorisation time of the same
run; the solve and the inverse are rated by their algorithmic work n^3 / 3 flops against the fp64 MFMA peak, the contraction
by the n^2 / 2 doubles it has to read against the HBM rate.  A shape whose second matrix does not fit is reported as such."""
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
PEAK_HBM = 8.0e12
KERNELS = ('seed', 'solve', 'inv', 'contract')


def run_shape(key, min_s, sig=20.0, lam=1e-10, seed=0):
    N, kind, M = SHAPES[key]
    n = 3 * N * M
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
    rec = {'shape': key, 'N': N, 'P': len(perms), 'M': M, 'n': n, 'assemble_ms': assemble_ms, 'factor_ms': factor_ms}
    try:
        ctx.evidence_grad(alphas)
    except MemoryError as e:
        rec['error'] = str(e)
        print(json.dumps(rec), flush=True)
        ctx.close()
        return rec
    reps, t0 = 0, time.perf_counter()
    while True:
        terms = ctx.evidence_grad(alphas)
        reps += 1
        dt = time.perf_counter() - t0
        if dt >= min_s and reps >= 3:
            break
    ms = dt / reps * 1e3
    phase_ms = ctx.phase_ms('evidence')[0]
    ctx.profile(True)
    ctx.evidence_grad(alphas)
    ctx.sync()
    ph = {k: ctx.kernel_stat('evidence_' + k)[0] for k in KERNELS}
    ctx.profile(False)
    fl = float(n) ** 3 / 3.0
    rec.update(ms_call=ms, reps=reps, ms_phase=phase_ms, terms=[float(t) for t in terms],
               call_over_factor=ms / factor_ms,
               solve_frac_peak=fl / (ph['solve'] * 1e-3) / PEAK_FP64, inv_frac_peak=fl / (ph['inv'] * 1e-3) / PEAK_FP64,
               contract_frac_hbm=4.0 * float(n) ** 2 / (ph['contract'] * 1e-3) / PEAK_HBM)
    for k in KERNELS:
        rec['ms_' + k] = ph[k]
        rec[k + '_over_factor'] = ph[k] / factor_ms
    print(json.dumps(rec), flush=True)
    ctx.uncert_release()
    ctx.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='A,B')
    ap.add_argument('--min-s', type=float, default=0.5)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'evidence_grad_probe.json'))
    a = ap.parse_args()
    _lib.preflight()
    recs = [run_shape(key, a.min_s) for key in a.shapes.split(',')]
    if a.out:
        with open(a.out, 'w') as f:
            json.dump({'peak_fp64_tflops': PEAK_FP64 * 1e-12, 'peak_hbm_tb_s': PEAK_HBM * 1e-12, 'points': recs}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()

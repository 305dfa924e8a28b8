"""Factor-reduction probe: milliseconds of GDMLPredict.remove_training_points (whole call, host steps, device phases) on seeded
synthetic training sets, against the alternative in the same process: prepare_uncertainty from scratch on the kept points
plus one chol_solve.

    python tools/remove_probe.py [--shapes A,B] [--points 1,16] [--positions quarter,middle,last] [--reps 2] [--out FILE.json]

Shapes are those of tools/uncertainty_probe.py: A (N = 21, P = 1, M = 1000) and B (N = 42, P = 27, M = 500), n = 63 000 both.
b consecutive points leave, starting at M // 4 (`quarter`), at M // 2 (`middle`) or ending with the last point (`last`: a pure
truncation, no sweep runs -- what is left is the compaction copy).  Every repetition builds a fresh predictor of the full
model, prepares its factor, removes the points (timed by the host clock; the call ends with the coefficients on the host,
so the device is idle when it returns), and then runs the alternative on the same predictor; the first repetition is a
warm-up, the median of the others is reported.  One further repetition runs with the library's per-kernel event timers on
and gives the split of the device time (remove_compact / _panel / _apply; they run back to back on one stream).
The compaction is rated by the bytes it moves (the kept lower triangle read and written)."""
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
from sgdml_amd.predict import GDMLPredict  # noqa: E402

SHAPES = {'A': (21, None, 1000), 'B': (42, 'c3x3', 500), 'T': (9, 'c2x2', 40)}  # N, permutation group, M before the removal
PEAK_HBM = 8.0e12


def _model(xd, gd, tp, perms, alphas, sig, lam, std):
    M = len(xd)
    return {'type': 'm', 'z': np.ones(perms.shape[1], dtype=np.int64), 'R_desc': np.ascontiguousarray(xd.T),
            'R_d_desc_alpha': orc.d_desc_dot_vec(gd, alphas.reshape(M, -1)), 'sig': sig, 'lam': lam, 'std': std, 'c': 0.0,
            'perms': perms, 'alphas_F': alphas, 'use_E_cstr': False, 'tril_perms_lin': orc.tril_perms_lin_from_tril_perms(tp)}


def base_model(key, sig=20.0, lam=1e-10, seed=0):
    N, kind, M = SHAPES[key]
    R, _, F = synth_geometries(N, M, seed=seed)
    R, F = R.reshape(M, -1), np.asarray(F, dtype=np.float64).reshape(M, -1)
    std = float(np.std(F))
    perms = perm_group(N, kind)
    tp = orc.tril_perms_from_atom_perms(perms)
    ctx = _lib.Context(0)
    xd, gd = ctx.desc_from_R(R, N)
    ctx.train_upload(xd, gd, tp)
    ctx.uncert_prepare(sig, lam)
    alphas = ctx.chol_solve(F.ravel() / std)
    ctx.uncert_release()
    ctx.close()
    return R, F, std, _model(xd, gd, tp, perms, alphas, sig, lam, std)


def run_point(key, base, b, where, reps):
    N, kind, M = SHAPES[key]
    R, F, std, model = base
    n3 = 3 * N
    first = {'quarter': M // 4, 'middle': M // 2, 'last': M - b}[where]
    idx = np.arange(first, first + b)
    keep = np.setdiff1d(np.arange(M), idx)
    n0, n1 = n3 * M, n3 * (M - b)
    calls, scratch, parts, last = [], [], [], None
    for rep in range(reps + 2):
        profiled = rep == reps + 1
        pred = GDMLPredict(model)
        pred.prepare_uncertainty(R, F_train=F)
        pred._ctx.sync()
        if profiled:
            pred._ctx.profile(True)
        t0 = time.perf_counter()
        out = pred.remove_training_points(idx)
        t1 = time.perf_counter()
        if profiled:
            pred._ctx.profile(False)
            last = out
        else:
            ts = time.perf_counter()
            pred.prepare_uncertainty(R[keep], F_train=F[keep])
            t_prep = time.perf_counter()
            pred._ctx.chol_solve(F[keep].ravel() / std)
            te = time.perf_counter()
            if rep > 0:
                calls.append(1e3 * (t1 - t0))
                scratch.append((1e3 * (te - ts), 1e3 * (t_prep - ts), 1e3 * (te - t_prep)))
                parts.append(out)
        pred.release_uncertainty()
        del pred
    call_ms = float(np.median(calls))
    sc = np.median(np.array(scratch), axis=0)
    k = last.get('kernel_ms', {})
    rec = {'shape': key, 'N': N, 'P': len(model['perms']), 'M': M, 'b': b, 'position': where, 'first': int(first), 'n': n0, 'n_kept': n1,
           'reps': reps, 'ms_call': call_ms, 'ms_call_all': calls,
           'ms_host': {h: float(np.median([p['host_ms'][h] for p in parts])) for h in ('remove', 'solve', 'model')},
           'ms_phase_remove': float(np.median([p['phase_ms']['remove'] for p in parts])),
           'ms_phase_solve': float(np.median([p['phase_ms']['solve'] for p in parts])),
           'ms_kernels_profiled': k, 'ms_call_profiled': None if last is None else sum(last['host_ms'].values()),
           'ms_scratch': float(sc[0]), 'ms_scratch_prepare': float(sc[1]), 'ms_scratch_solve': float(sc[2]),
           'speedup': float(sc[0] / call_ms),
           'compact_gbs': (float(n1) * (n1 + 1) * 8.0 / k['remove_compact'] * 1e-6) if k.get('remove_compact') else None,
           'two_pass_floor_ms': 2.0 * 0.5 * n1 * n1 * 8 / PEAK_HBM * 1e3}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='A,B')
    ap.add_argument('--points', default='1,16')
    ap.add_argument('--positions', default='quarter,middle,last')
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    _lib.preflight()
    recs = []
    for key in a.shapes.split(','):
        base = base_model(key)
        for b in a.points.split(','):
            for where in a.positions.split(','):
                recs.append(run_point(key, base, int(b), where, a.reps))
                if a.out:  # (kept up to date: a long run that is cut short leaves what it measured)
                    with open(a.out, 'w') as f:
                        json.dump({'peak_hbm_tbs': PEAK_HBM * 1e-12, 'points': recs}, f, indent=1)
                        f.write('\n')


if __name__ == '__main__':
    main()

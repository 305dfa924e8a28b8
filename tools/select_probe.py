"""Selection probe: milliseconds of GDMLPredict.select_training_points (whole call, device phase, per-kernel split) on a seeded
synthetic training set, against the slow loop that the calls of the parent commit allow: per pick, gdml_predict_cov on the
whole pool (full covariances), the gains log det(Sig_q / lam + I) on the host, gdml_factor_extend of the best candidate.

    python tools/select_probe.py [--shape A] [--pools 64,256] [--picks 16] [--reps 2] [--out profiles/select_probe.json]

Shape A is BASELINE.json configs[1]: N = 21, P = 1, M = 1000, n = 63 000 (T: a small shape for trying the probe).  The pool
is a second seeded set of geometries of the same molecule.  The selection only reads the factor, so all pools are timed on
one prepared predictor (first call = warm-up, median of the others); then the slow loop runs once per pool on the same
context and its 16 added points are removed again (a truncation of the factor).  One further selection per pool runs with
the library's per-kernel event timers on.  select_column is rated against its memory floor: the 8 m_pool ld bytes of W it
reads once per step, over 8 TB/s."""
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

SHAPES = {'A': (21, None, 1000), 'T': (9, 'c2x2', 40)}  # N, permutation group, M
PEAK_HBM = 8.0e12
KERNELS = ('select_cross', 'select_solve', 'select_gram', 'select_score', 'select_column', 'select_update')


def slow_loop(ctx, pool, xd, gd, b, lam, n3):
    """The picks of the greedy rule from calls that exist without gdml_select_points; the factor grows by b points."""
    picks = []
    for _ in range(b):
        raw = ctx.predict_cov(pool, None, full=True)
        gain = np.linalg.slogdet(raw / lam + np.eye(n3))[1]
        gain[picks] = -np.inf
        q = int(np.argmax(gain))
        picks.append(q)
        ctx.factor_extend(xd[q:q + 1], gd[q:q + 1])
    return picks


def run(key, pools, b, reps, sig=20.0, lam=1e-6, seed=0):
    N, kind, M = SHAPES[key]
    n3 = 3 * N
    R, _, F = synth_geometries(N, M, seed=seed)
    R, F = R.reshape(M, -1), np.asarray(F, dtype=np.float64).reshape(M, -1)
    Rp = synth_geometries(N, max(pools), seed=seed + 1)[0].reshape(max(pools), -1)
    std = float(np.std(F))
    perms = perm_group(N, kind)
    tp = orc.tril_perms_from_atom_perms(perms)
    ctx = _lib.Context(0)
    xd, gd = ctx.desc_from_R(R, N)
    ctx.close()
    model = {'type': 'm', 'z': np.ones(N, dtype=np.int64), 'R_desc': np.ascontiguousarray(xd.T),
             'R_d_desc_alpha': np.zeros((M, xd.shape[1])), 'sig': sig, 'lam': lam, 'std': std, 'c': 0.0, 'perms': perms,
             'alphas_F': np.zeros(M * n3), 'use_E_cstr': False, 'tril_perms_lin': orc.tril_perms_lin_from_tril_perms(tp)}
    pred = GDMLPredict(model)
    t0 = time.perf_counter()
    pred.prepare_uncertainty(R)
    pred._ctx.sync()
    ms_prepare = 1e3 * (time.perf_counter() - t0)
    ctx = pred._ctx
    xp, gp = ctx.desc_from_R(Rp, N)
    recs = []
    for B in pools:
        pool = np.ascontiguousarray(Rp[:B])
        calls, phases, out = [], [], None
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            out = pred.select_training_points(pool, b)
            t1 = time.perf_counter()
            if rep > 0:
                calls.append(1e3 * (t1 - t0))
                phases.append(out['phase_ms']['select'])
        ctx.profile(True)
        w0 = ctx.kernel_stat('select_column')
        prof = pred.select_training_points(pool, b)
        w1 = ctx.kernel_stat('select_column')
        ctx.profile(False)
        t0 = time.perf_counter()
        picks = slow_loop(ctx, pool, xp, gp, b, lam, n3)
        ms_slow = 1e3 * (time.perf_counter() - t0)
        ctx.factor_remove(np.arange(M, M + b))  # back to the M points of the model
        k = prof.get('kernel_ms', {})
        col_ms, col_bytes = w1[0] - w0[0], w1[2] - w0[2]
        rec = {'shape': key, 'N': N, 'P': len(perms), 'M': M, 'n': M * n3, 'lam': lam, 'pool': B, 'picks': b, 'reps': reps,
               'ms_prepare': ms_prepare, 'ms_call': float(np.median(calls)), 'ms_call_all': calls,
               'ms_phase_select': float(np.median(phases)), 'ms_kernels': k,
               'ms_slow_loop': ms_slow, 'speedup': ms_slow / float(np.median(calls)),
               'same_picks': bool(np.array_equal(picks, out['idx'])),
               'column_steps': int(w1[1] - w0[1]), 'column_ms_per_step': col_ms / max(1, w1[1] - w0[1]),
               'column_floor_ms_per_step': col_bytes / max(1, w1[1] - w0[1]) / PEAK_HBM * 1e3,
               'column_fraction_of_hbm_peak': (col_bytes / PEAK_HBM * 1e3 / col_ms) if col_ms > 0 else None}
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    pred.release_uncertainty()
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='A')
    ap.add_argument('--pools', default='64,256')
    ap.add_argument('--picks', type=int, default=16)
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                                                  'select_probe.json'))
    a = ap.parse_args()
    _lib.preflight()
    recs = run(a.shape, [int(v) for v in a.pools.split(',')], a.picks, a.reps)
    with open(a.out, 'w') as f:
        json.dump({'peak_hbm_tbs': PEAK_HBM * 1e-12, 'points': recs}, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()

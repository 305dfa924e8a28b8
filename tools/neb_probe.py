"""Nudged-elastic-band probe: microseconds per evaluation of GDMLPredict.neb (B bands of P images; positions, velocities,
forces and the optimiser's state resident on the device) on the configs[1] shape of the benchmark (N = 21, M = 1000, one
permutation), against two yardsticks measured in the same process: GDMLPredict.relax of the same B P geometries, uncoupled, on
the general route -- the same prediction per evaluation, one launch fewer -- and the host loop neb() replaces, a NumPy band
(tests/_neb_ref.py's step, vectorised over the bands) around GDMLPredict.predict.

    python tools/neb_probe.py [--shapes 1x8,1x32,8x16,32x32] [--rounds 5] [--min-s 0.3] [--out profiles/neb_probe.json]

fmax is set so that nothing converges and the step cap so small that the images stay where they are: every call makes
max_steps + 1 evaluations of all B P geometries.  Every shape alternates its variants for --rounds rounds; a round repeats one
call for at least --min-s seconds after one warm-up call.  Reported per variant: the median of the rounds and their spread
(max - min) / median.  No rate is asserted anywhere: the file records what was measured."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from md_probe import timed_steps  # noqa: E402
from relax_probe import FIRE, stats  # noqa: E402
from stress_probe import N, M, SIG, build_predictor  # noqa: E402  (the same model; its 1000-unit cell wraps nothing)

K_SPRING = 0.5


def host_neb(pred, R, n_steps, fmax, dt_start, max_step, k=K_SPRING, n_min=5, f_inc=1.1, f_dec=0.5, alpha_start=0.1,
             f_alpha=0.99):
    """The loop a user writes today: one predict() of all B P images per evaluation, improved tangents, springs, the climbing
    image and FIRE per band in NumPy."""
    B, P, n3 = R.shape
    R = R.copy()
    V = np.zeros((B, P - 2, n3))
    dt, alpha, n_pos = np.full(B, dt_start), np.full(B, alpha_start), np.zeros(B, dtype=np.int64)
    dt_max = 10.0 * dt_start
    rows = np.arange(B)
    for t in range(n_steps + 1):
        E, F = pred.predict(R.reshape(B * P, n3))
        E, g = E.reshape(B, P), F.reshape(B, P, n3)[:, 1:-1]
        tp, tm = R[:, 2:] - R[:, 1:-1], R[:, 1:-1] - R[:, :-2]
        ep, e0, em = E[:, 2:], E[:, 1:-1], E[:, :-2]
        dp, dm = np.abs(ep - e0), np.abs(em - e0)
        d_max, d_min = np.maximum(dp, dm), np.minimum(dp, dm)
        a = np.where((ep > e0) & (e0 > em), 1.0, np.where((ep < e0) & (e0 < em), 0.0, np.where(ep > em, d_max, d_min)))
        b = np.where((ep > e0) & (e0 > em), 0.0, np.where((ep < e0) & (e0 < em), 1.0, np.where(ep > em, d_min, d_max)))
        tau = a[..., None] * tp + b[..., None] * tm
        len_t = np.sqrt((tau * tau).sum(-1))
        dot = (g * tau).sum(-1) / len_t
        c = (k * (np.sqrt((tp * tp).sum(-1)) - np.sqrt((tm * tm).sum(-1))) - dot) / len_t
        ic = np.argmax(e0, axis=1)
        c[rows, ic] = -2.0 * dot[rows, ic] / len_t[rows, ic]
        Fb = g + c[..., None] * tau
        f_atom = np.sqrt((Fb.reshape(B, -1, 3) ** 2).sum(-1)).max(axis=1)
        if (f_atom < fmax).all() or t == n_steps:
            break
        if t > 0:
            p = (Fb * V).sum(axis=(1, 2))
            up = p > 0.0
            ratio = alpha * np.sqrt((V * V).sum(axis=(1, 2))) / np.sqrt((Fb * Fb).sum(axis=(1, 2)))
            V = np.where(up[:, None, None], (1.0 - alpha)[:, None, None] * V + ratio[:, None, None] * Fb, 0.0)
            grow = up & (n_pos > n_min)
            dt = np.where(grow, np.minimum(dt * f_inc, dt_max), np.where(up, dt, dt * f_dec))
            alpha = np.where(grow, alpha * f_alpha, np.where(up, alpha, alpha_start))
            n_pos = np.where(up, n_pos + 1, 0)
        V = V + dt[:, None, None] * Fb
        d = dt[:, None, None] * V
        nrm = np.sqrt((d * d).sum(axis=(1, 2)))
        d = np.where((nrm > max_step)[:, None, None], d * (max_step / np.maximum(nrm, 1e-300))[:, None, None], d)
        R[:, 1:-1] += d
    return R, E


def run_points(pred, Rq, shapes, rounds, min_s):
    ctx = pred._ctx
    out = []
    for B, P in shapes:
        n3 = 3 * N
        path = np.ascontiguousarray(np.resize(Rq, (B, P, n3)))
        path += 1e-3 * np.random.RandomState(2).standard_normal(path.shape)  # no two images alike
        flat = path.reshape(B * P, n3)
        n_dev = 2000 if B * P <= 32 else (500 if B * P <= 128 else 100)
        n_host = 200 if B * P <= 128 else 20
        variants = {'neb': (lambda: pred.neb(path, k_spring=K_SPRING, climb=True, max_steps=n_dev - 1, **FIRE), n_dev),
                    'relax_general_route': (lambda: pred.relax(flat, max_steps=n_dev - 1, **FIRE), n_dev),
                    'host_neb': (lambda: host_neb(pred, path, n_host - 1, **FIRE), n_host)}
        rates = {k: [] for k in variants}
        ctx.set_option('predict.relax_fused', 0)
        for _ in range(rounds):
            for k, (fn, n) in variants.items():
                rates[k].append(timed_steps(fn, n, min_s))
        ctx.set_option('predict.relax_fused', 1)
        rec = {'N': N, 'M': M, 'B': B, 'P': P, 'geometries': B * P, 'evaluations_per_call': {k: n for k, (_, n) in variants.items()}}
        rec.update({k: stats(v) for k, v in rates.items()})
        rec['neb_over_relax'] = rec['neb']['us_per_evaluation'] / rec['relax_general_route']['us_per_evaluation']
        rec['host_neb_over_neb'] = rec['host_neb']['us_per_evaluation'] / rec['neb']['us_per_evaluation']
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='1x8,1x32,8x16,32x32')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--min-s', type=float, default=0.3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit('--rounds: the median of at least five rounds')
    pred, Rq = build_predictor()
    shapes = [tuple(int(v) for v in s.split('x')) for s in a.shapes.split(',')]
    result = {'shape': {'N': N, 'M': M, 'perms': 1, 'sig': SIG, 'fire': FIRE, 'k_spring': K_SPRING, 'climb': True},
              'yardsticks': {'relax_general_route': 'GDMLPredict.relax of the same B P geometries, uncoupled, predict.relax_fused = 0',
                             'host_neb': 'NumPy band around GDMLPredict.predict (one call per evaluation), same process'},
              'points': run_points(pred, Rq, shapes, a.rounds, a.min_s)}
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()

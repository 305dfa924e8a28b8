"""Variable-cell relaxation probe: microseconds per evaluation of GDMLPredict.relax_cell (reference positions, cell, velocities
and the optimiser's state resident on the device) on the configs[1] shape of the benchmark (N = 21, M = 1000, one permutation,
the 1000-unit cell of tools/stress_probe.py), against two yardsticks measured in the same process:
  (a) GDMLPredict.relax on the general route (predict.relax_fused = 0) at the same B -- the same launches per evaluation with
      the plain epilogue and desc_kernel instead of the virial epilogue and desc_cells_kernel, and a smaller update kernel; the
      expectation is the stress / predict ratio of the README (1.06-1.12) plus the one small launch before evaluation 0;
  (b) the host loop relax_cell replaces, the only way before it: a NumPy FIRE over (s, C) that calls predict_stress once per
      geometry per evaluation (one lattice per call).

    python tools/cellrelax_probe.py [--batches 1,8,64,1024] [--rounds 5] [--min-s 0.3] [--out profiles/cellrelax_probe.json]

fmax is set so that nothing converges and the step cap so small that geometries and cells stay where they are: every call
makes max_steps + 1 evaluations of all B geometries.  Every point alternates its variants for --rounds rounds; a round repeats
one call for at least --min-s seconds after one warm-up call.  Reported per variant: the median of the rounds and their spread
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
from stress_probe import N, M, SIG, build_predictor  # noqa: E402


def host_fire_cell(pred, R0, lat, n_steps, fmax, dt_start, max_step, pressure=0.0, n_min=5, f_inc=1.1, f_dec=0.5, alpha_start=0.1,
                   f_alpha=0.99):
    """The loop a user writes today: u = (s, N Fd) per geometry, one predict_stress() per geometry per evaluation (a call takes
    one lattice), FIRE for all B geometries in NumPy."""
    B = R0.shape[0]
    cf = float(N)
    s = R0.reshape(B, N, 3).copy()
    Cc = np.broadcast_to(cf * np.eye(3), (B, 3, 3)).copy()
    V = np.zeros((B, 3 * N + 9))
    dt, alpha, n_pos = np.full(B, dt_start), np.full(B, alpha_start), np.zeros(B, dtype=np.int64)
    dt_max = 10.0 * dt_start
    E = np.zeros(B)
    for t in range(n_steps + 1):
        Fd = Cc / cf
        G = np.empty((B, 3 * N + 9))
        for b in range(B):
            L = Fd[b] @ lat
            e, f, S = pred.predict_stress((s[b] @ Fd[b].T).ravel(), lattice=L)
            vol = abs(np.linalg.det(L))
            E[b] = e[0]
            G[b, :3 * N] = (f.reshape(N, 3) @ Fd[b]).ravel()
            G[b, 3 * N:] = (-(S[0] * vol + pressure * vol * np.eye(3)) @ np.linalg.inv(Fd[b]).T / cf).ravel()
        f_atom = np.sqrt((G.reshape(B, -1, 3) ** 2).sum(-1)).max(axis=1)
        if (f_atom < fmax).all() or t == n_steps:
            break
        if t > 0:
            p = (G * V).sum(axis=1)
            up = p > 0.0
            mix = (1.0 - alpha)[:, None] * V + (alpha * np.sqrt((V * V).sum(axis=1)) / np.sqrt((G * G).sum(axis=1)))[:, None] * G
            V = np.where(up[:, None], mix, 0.0)
            grow = up & (n_pos > n_min)
            dt = np.where(grow, np.minimum(dt * f_inc, dt_max), np.where(up, dt, dt * f_dec))
            alpha = np.where(grow, alpha * f_alpha, np.where(up, alpha, alpha_start))
            n_pos = np.where(up, n_pos + 1, 0)
        V = V + dt[:, None] * G
        d = dt[:, None] * V
        nrm = np.sqrt((d * d).sum(axis=1))
        d = np.where((nrm > max_step)[:, None], d * (max_step / np.maximum(nrm, 1e-300))[:, None], d)
        s = s + d[:, :3 * N].reshape(B, N, 3)
        Cc = Cc + d[:, 3 * N:].reshape(B, 3, 3)
    return s, Cc, E


def run_points(pred, Rq, batches, rounds, min_s):
    ctx = pred._ctx
    lat = np.asarray(pred.lat_and_inv[0], dtype=np.float64)
    out = []
    for B in batches:
        R0 = np.ascontiguousarray(np.resize(Rq, (B, 3 * N)))
        n_dev = 1000 if B <= 8 else (500 if B <= 64 else 100)
        n_host = 100 if B == 1 else (20 if B <= 8 else (5 if B <= 64 else 2))
        variants = {'relax_cell': (lambda: pred.relax_cell(R0, max_steps=n_dev - 1, **FIRE), n_dev),
                    'relax_general_route': (lambda: pred.relax(R0, max_steps=n_dev - 1, **FIRE), n_dev),
                    'host_fire_cell': (lambda: host_fire_cell(pred, R0, lat, n_host - 1, **FIRE), n_host)}
        rates = {k: [] for k in variants}
        ctx.set_option('predict.relax_fused', 0)
        try:
            for _ in range(rounds):
                for k, (fn, n) in variants.items():
                    rates[k].append(timed_steps(fn, n, min_s))
        finally:
            ctx.set_option('predict.relax_fused', 1)
        rec = {'N': N, 'M': M, 'B': B, 'evaluations_per_call': {k: n for k, (_, n) in variants.items()}}
        rec.update({k: stats(v) for k, v in rates.items()})
        rec['relax_cell_over_relax_general_route'] = (rec['relax_cell']['us_per_evaluation'] /
                                                      rec['relax_general_route']['us_per_evaluation'])
        rec['host_fire_cell_over_relax_cell'] = rec['host_fire_cell']['us_per_evaluation'] / rec['relax_cell']['us_per_evaluation']
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,8,64,1024')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--min-s', type=float, default=0.3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit('--rounds: the median of at least five rounds')
    pred, Rq = build_predictor()
    result = {'shape': {'N': N, 'M': M, 'P': 1, 'sig': SIG, 'fire': FIRE, 'lattice': 'cubic, 1000 (nothing wraps)',
                        'mask': 'all ones', 'pressure': 0.0, 'cell_factor': N},
              'yardsticks': {'relax_general_route': 'GDMLPredict.relax with predict.relax_fused = 0, same B, same process',
                             'host_fire_cell': 'NumPy FIRE over (s, C) around GDMLPredict.predict_stress, one call per geometry '
                                               'per evaluation, same process'},
              'points': run_points(pred, Rq, [int(b) for b in a.batches.split(',')], a.rounds, a.min_s)}
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()

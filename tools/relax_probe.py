"""Relaxation probe: microseconds per evaluation of GDMLPredict.relax (positions, velocities, forces and the optimiser's
state resident on the device) on the configs[1] shape of the benchmark (N = 21, M = 1000, one permutation), against two
yardsticks measured in the same process, neither of them code the relaxation added: GDMLPredict.run_md (NVE) on the same route
and shape -- the same predictor per step with a shorter epilogue -- and the host loop relax() replaces, a NumPy FIRE around
GDMLPredict.predict.

    python tools/relax_probe.py [--batches 1,8,64,1024] [--rounds 5] [--min-s 0.3] [--out profiles/relax_probe.json]

Per batch size: relax on the route the library picks (one launch per evaluation up to eight geometries, two pieces beyond) and,
where the single launch serves the shape, on the general route as well (options predict.relax_fused / predict.md_fused = 0).
fmax is set so that nothing converges and the step cap so small that the geometries stay where they are: every call makes
max_steps + 1 evaluations of all B geometries.  Every point alternates its variants for --rounds rounds; a round repeats one
call for at least --min-s seconds after one warm-up call.  Reported per variant: the median of the rounds and their spread
(max - min) / median -- the run-to-run noise any comparison in this file has to be read against.  No rate is asserted
anywhere: the file records what was measured."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from md_probe import DT, timed_steps  # noqa: E402
from stress_probe import N, M, SIG, build_predictor  # noqa: E402  (the same model; its 1000-unit cell wraps nothing)

FIRE = dict(fmax=1e-30, dt_start=1e-3, max_step=1e-6)


def host_fire(pred, R, n_steps, fmax, dt_start, max_step, n_min=5, f_inc=1.1, f_dec=0.5, alpha_start=0.1, f_alpha=0.99):
    """The loop a user writes today: one predict() per evaluation, FIRE for all B geometries in NumPy."""
    B = R.shape[0]
    V = np.zeros_like(R)
    dt, alpha, n_pos = np.full(B, dt_start), np.full(B, alpha_start), np.zeros(B, dtype=np.int64)
    dt_max = 10.0 * dt_start
    for t in range(n_steps + 1):
        E, F = pred.predict(R)
        f_atom = np.sqrt((F.reshape(B, -1, 3) ** 2).sum(-1)).max(axis=1)
        if (f_atom < fmax).all() or t == n_steps:
            break
        if t > 0:
            p = (F * V).sum(axis=1)
            up = p > 0.0
            mix = (1.0 - alpha)[:, None] * V + (alpha * np.sqrt((V * V).sum(axis=1)) / np.sqrt((F * F).sum(axis=1)))[:, None] * F
            V = np.where(up[:, None], mix, 0.0)
            grow = up & (n_pos > n_min)
            dt = np.where(grow, np.minimum(dt * f_inc, dt_max), np.where(up, dt, dt * f_dec))
            alpha = np.where(grow, alpha * f_alpha, np.where(up, alpha, alpha_start))
            n_pos = np.where(up, n_pos + 1, 0)
        V = V + dt[:, None] * F
        d = dt[:, None] * V
        nrm = np.sqrt((d * d).sum(axis=1))
        d = np.where((nrm > max_step)[:, None], d * (max_step / np.maximum(nrm, 1e-300))[:, None], d)
        R = R + d
    return R, E


def stats(v):
    med = float(np.median(v))
    return {'us_per_evaluation': 1e6 / med, 'rounds_evaluations_per_s': [float(x) for x in v],
            'spread': float((max(v) - min(v)) / med)}


def run_points(pred, Rq, batches, rounds, min_s):
    ctx = pred._ctx
    masses = np.ones(N)
    out = []
    for B in batches:
        R0 = np.ascontiguousarray(np.resize(Rq, (B, 3 * N)))
        V0 = np.zeros_like(R0)
        n_dev = 2000 if B <= 8 else (500 if B <= 64 else 100)
        n_host = 200 if B <= 64 else 20
        fused = B <= 8
        # relax makes max_steps + 1 evaluations, run_md n_steps + 1 (the forces of the start)
        variants = {'relax': (lambda: pred.relax(R0, max_steps=n_dev - 1, **FIRE), n_dev),
                    'run_md_nve': (lambda: pred.run_md(R0, V0, masses, DT, n_dev - 1, record_every=n_dev - 1, record=('R',)), n_dev)}
        if fused:
            variants['relax_general_route'] = variants['relax']
            variants['run_md_nve_general_route'] = variants['run_md_nve']
        variants['host_fire'] = (lambda: host_fire(pred, R0, n_host - 1, **FIRE), n_host)
        rates = {k: [] for k in variants}
        for _ in range(rounds):
            for k, (fn, n) in variants.items():
                for opt in ('predict.relax_fused', 'predict.md_fused'):
                    ctx.set_option(opt, 0 if k.endswith('general_route') else 1)
                rates[k].append(timed_steps(fn, n, min_s))
        for opt in ('predict.relax_fused', 'predict.md_fused'):
            ctx.set_option(opt, 1)
        rec = {'N': N, 'M': M, 'B': B, 'route': 'single launch per evaluation' if fused else 'general',
               'evaluations_per_call': {k: n for k, (_, n) in variants.items()}}
        rec.update({k: stats(v) for k, v in rates.items()})
        rec['relax_over_run_md'] = rec['relax']['us_per_evaluation'] / rec['run_md_nve']['us_per_evaluation']
        if fused:
            rec['relax_over_run_md_general_route'] = (rec['relax_general_route']['us_per_evaluation'] /
                                                      rec['run_md_nve_general_route']['us_per_evaluation'])
        rec['host_fire_over_relax'] = rec['host_fire']['us_per_evaluation'] / rec['relax']['us_per_evaluation']
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def chunk_sweep(pred, Rq, rounds, min_s, lengths=(4, 8, 16, 32, 64, 128, 4096)):
    """One geometry on the single-launch route, chunk lengths (option predict.relax_chunk_steps) alternating per round: what a
    synchronisation costs per evaluation -- the figure the default chunk length is chosen from."""
    R0 = np.ascontiguousarray(np.resize(Rq, (1, 3 * N)))
    n = 2048
    rates = {c: [] for c in lengths}
    for _ in range(rounds):
        for c in lengths:
            pred._ctx.set_option('predict.relax_chunk_steps', c)
            rates[c].append(timed_steps(lambda: pred.relax(R0, max_steps=n - 1, **FIRE), n, min_s))
    pred._ctx.set_option('predict.relax_chunk_steps', 32)
    out = [dict(chunk_steps=c, **stats(v)) for c, v in rates.items()]
    print(json.dumps(out), flush=True)
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
    result = {'shape': {'N': N, 'M': M, 'P': 1, 'sig': SIG, 'fire': FIRE, 'md_dt': DT},
              'yardsticks': {'run_md_nve': 'GDMLPredict.run_md, velocity Verlet, same route and shape, one recorded frame',
                             'host_fire': 'NumPy FIRE around GDMLPredict.predict (one call per evaluation), same process'},
              'points': run_points(pred, Rq, [int(b) for b in a.batches.split(',')], a.rounds, a.min_s),
              'chunk_sweep_B1': chunk_sweep(pred, Rq, a.rounds, a.min_s)}
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()

"""MD probe: steps per second of GDMLPredict.run_md (positions, velocities and forces resident on the device) against the
host loop it replaces -- a NumPy velocity Verlet around GDMLPredict.predict -- in the same process, on the configs[1] shape of
the benchmark (N = 21, M = 1000, one permutation).

    python tools/md_probe.py [--batches 1,8,64,1024] [--rounds 5] [--min-s 0.3] [--out profiles/md_probe.json]

Per batch size: run_md without and with the Langevin thermostat, on the route the library picks (one launch per step up to
eight replicas, three pieces per step beyond) and, where the single launch serves the shape, on the general route as well
(option predict.md_fused = 0); then the host loop.  Every point alternates its variants for --rounds rounds; a round repeats one
call (a trajectory of a fixed number of steps, one recorded frame) for at least --min-s seconds after one unrecorded warm-up
call.  Reported per variant: the median of the rounds in steps per second and their spread (max - min) / median -- the run-to-run
noise any comparison in this file has to be read against.  No rate is asserted anywhere: the file records what was measured."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from stress_probe import N, M, SIG, build_predictor  # noqa: E402  (the same model; its 1000-unit cell wraps nothing)

DT = 1e-5
LANGEVIN = dict(thermostat='langevin', gamma=0.5, kT=0.01, seed=1)


def host_verlet(pred, R, V, masses3, dt, n_steps):
    """The loop a user writes today: one predict() per step, the integrator in NumPy."""
    _, F = pred.predict(R)
    for _ in range(n_steps):
        V = V + 0.5 * dt * F / masses3
        R = R + dt * V
        E, F = pred.predict(R)
        V = V + 0.5 * dt * F / masses3
    return R, V, E


def timed_steps(fn, n_steps, min_s):
    """steps per second of fn(), which advances n_steps."""
    fn()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= min_s:
            return n * n_steps / dt


def stats(v):
    med = float(np.median(v))
    return {'median_steps_per_s': med, 'us_per_step': 1e6 / med, 'rounds_steps_per_s': [float(x) for x in v],
            'spread': float((max(v) - min(v)) / med)}


def run_points(batches, rounds, min_s):
    pred, Rq = build_predictor()
    ctx = pred._ctx
    masses = np.ones(N)
    out = []
    for B in batches:
        R0 = np.ascontiguousarray(np.resize(Rq, (B, 3 * N)))
        V0 = 0.01 * np.random.RandomState(1).standard_normal(R0.shape)
        n_dev = 2000 if B <= 8 else (500 if B <= 64 else 100)
        n_host = 200 if B <= 64 else 20
        fused = B <= 8

        def dev(th, n=n_dev):
            return lambda: pred.run_md(R0, V0, masses, DT, n, record_every=n, record=('R',), **th)

        variants = {'run_md_nve': (dev({}), n_dev), 'run_md_langevin': (dev(LANGEVIN), n_dev)}
        if fused:
            variants['run_md_nve_general_route'] = (dev({}), n_dev)
            variants['run_md_langevin_general_route'] = (dev(LANGEVIN), n_dev)
        variants['host_loop_nve'] = (lambda: host_verlet(pred, R0, V0, masses.repeat(3)[None], DT, n_host), n_host)
        rates = {k: [] for k in variants}
        for _ in range(rounds):
            for k, (fn, n) in variants.items():
                ctx.set_option('predict.md_fused', 0 if k.endswith('general_route') else 1)
                rates[k].append(timed_steps(fn, n, min_s))
        ctx.set_option('predict.md_fused', 1)
        rec = {'N': N, 'M': M, 'B': B, 'route': 'single launch per step' if fused else 'general',
               'steps_per_call': {k: n for k, (_, n) in variants.items()}}
        rec.update({k: stats(v) for k, v in rates.items()})
        rec['run_md_nve_over_host_loop'] = rec['run_md_nve']['median_steps_per_s'] / rec['host_loop_nve']['median_steps_per_s']
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
    result = {'shape': {'N': N, 'M': M, 'P': 1, 'sig': SIG, 'dt': DT, 'masses': 1.0, 'langevin': LANGEVIN},
              'host_loop': 'NumPy velocity Verlet around GDMLPredict.predict (one call per step), same process',
              'points': run_points([int(b) for b in a.batches.split(',')], a.rounds, a.min_s)}
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()

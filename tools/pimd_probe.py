"""PIMD probe: steps per second of GDMLPredict.run_pimd (B rings of P beads resident on the device) on the configs[1] shape of
the benchmark (N = 21, M = 1000, one permutation), beside two yardsticks that this path does not touch:
  run_md with B * P independent replicas on the general route (option predict.md_fused = 0) -- the same prediction batch and
    the same number of launches per step, without the coupling between beads;
  a NumPy ring step (the same normal-mode flow) around GDMLPredict.predict, one call per step, in the same process.

    python tools/pimd_probe.py [--points 1x8,1x32,8x32] [--rounds 5] [--min-s 0.3] [--out profiles/pimd_probe.json]

Per point: run_pimd without and with the PILE thermostat at the default tile width of the first kernel and with the narrow
tile (option predict.pimd_tile = 32), then the yardsticks.  The protocol is tools/md_probe.py's: every point alternates its
variants for --rounds rounds; a round repeats one call (a trajectory of a fixed number of steps, one recorded frame) for at
least --min-s seconds after one unrecorded warm-up call.  Reported per variant: the median of the rounds in steps per second
and their spread (max - min) / median.  No rate is asserted anywhere: the file records what was measured."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from md_probe import DT, stats, timed_steps  # noqa: E402
from stress_probe import N, M, SIG, build_predictor  # noqa: E402  (the same model; its 1000-unit cell wraps nothing)
from sgdml_amd import _lib  # noqa: E402

KT = 0.01
PILE = dict(thermostat='pile', gamma_centroid=0.5, seed=1)
LANGEVIN = dict(thermostat='langevin', gamma=0.5, kT=KT, seed=1)


def host_ring(pred, R, V, masses3, dt, n_steps, Cm, omega):
    """The loop a user writes today: one predict() of all beads per step, the ring's free flow in NumPy.  R, V (B,P,3N)."""
    B, P, n3 = R.shape
    w = omega[None, :, None]
    cs, wsn = np.cos(w * dt), w * np.sin(w * dt)
    sn = np.where(w > 0.0, np.sin(w * dt) / np.where(w > 0.0, w, 1.0), dt)
    _, F = pred.predict(R.reshape(B * P, n3))
    for _ in range(n_steps):
        V = V + 0.5 * dt * F.reshape(B, P, n3) / masses3
        q, v = np.einsum('jk,bjc->bkc', Cm, R), np.einsum('jk,bjc->bkc', Cm, V)
        q, v = cs * q + sn * v, -wsn * q + cs * v
        R, V = np.einsum('jk,bkc->bjc', Cm, q), np.einsum('jk,bkc->bjc', Cm, v)
        E, F = pred.predict(R.reshape(B * P, n3))
        V = V + 0.5 * dt * F.reshape(B, P, n3) / masses3
    return R, V, E


def run_points(points, rounds, min_s):
    pred, Rq = build_predictor()
    ctx = pred._ctx
    masses = np.ones(N)
    out = []
    for B, P in points:
        hbar = 2 * P * KT * DT  # omega_max dt = 1
        rs = np.random.RandomState(1)
        R0 = np.resize(Rq, (B, 1, 3 * N)) + 1e-3 * rs.standard_normal((B, P, 3 * N))
        V0 = 0.01 * rs.standard_normal(R0.shape)
        Rm, Vm = R0.reshape(B * P, -1), V0.reshape(B * P, -1)
        Cm, omega = _lib.Context.pimd_modes(P, KT, hbar)
        n_dev = 1000 if B * P <= 64 else 200
        n_host = 100 if B * P <= 64 else 20

        def ring(th):
            return lambda: pred.run_pimd(R0, V0, masses, DT, n_dev, P, KT, hbar, record_every=n_dev, record=('Rc',), **th)

        def replicas(th):
            return lambda: pred.run_md(Rm, Vm, masses, DT, n_dev, record_every=n_dev, record=('R',), **th)

        variants = {
            'run_pimd_nve': (ring({}), n_dev), 'run_pimd_pile': (ring(PILE), n_dev),
            'run_pimd_nve_tile32': (ring({}), n_dev), 'run_pimd_pile_tile32': (ring(PILE), n_dev),
            'run_md_replicas_nve': (replicas({}), n_dev), 'run_md_replicas_langevin': (replicas(LANGEVIN), n_dev),
            'host_ring_nve': (lambda: host_ring(pred, R0, V0, masses.repeat(3)[None, None], DT, n_host, Cm, omega), n_host),
        }
        rates = {k: [] for k in variants}
        ctx.set_option('predict.md_fused', 0)  # B * P replicas on the general route, whatever their number
        for _ in range(rounds):
            for k, (fn, n) in variants.items():
                ctx.set_option('predict.pimd_tile', 32 if k.endswith('tile32') else 0)
                rates[k].append(timed_steps(fn, n, min_s))
        ctx.set_option('predict.pimd_tile', 0)
        ctx.set_option('predict.md_fused', 1)
        rec = {'N': N, 'M': M, 'B': B, 'P': P, 'default_tile': 64 if P <= 64 else 32,
               'steps_per_call': {k: n for k, (_, n) in variants.items()}}
        rec.update({k: stats(v) for k, v in rates.items()})
        med = {k: rec[k]['median_steps_per_s'] for k in variants}
        rec['ring_step_over_replica_step_nve'] = med['run_md_replicas_nve'] / med['run_pimd_nve']  # time ratio
        rec['ring_step_over_replica_step_thermostat'] = med['run_md_replicas_langevin'] / med['run_pimd_pile']
        rec['run_pimd_nve_over_host_ring'] = med['run_pimd_nve'] / med['host_ring_nve']
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--points', default='1x8,1x32,8x32')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--min-s', type=float, default=0.3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit('--rounds: the median of at least five rounds')
    points = [tuple(int(x) for x in p.split('x')) for p in a.points.split(',')]
    result = {'shape': {'N': N, 'M': M, 'P_perms': 1, 'sig': SIG, 'dt': DT, 'kT': KT, 'hbar': '2 beads kT dt', 'masses': 1.0,
                        'pile': PILE, 'langevin': LANGEVIN},
              'yardsticks': {'run_md_replicas': 'run_md with B * beads independent replicas, general route (predict.md_fused = 0)',
                             'host_ring': 'NumPy ring step around GDMLPredict.predict (one call per step), same process'},
              'ratios': 'ring_step_over_replica_step_*: time of a ring step / time of a step of B * beads replicas',
              'points': run_points(points, a.rounds, a.min_s)}
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()

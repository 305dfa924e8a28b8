"""NPT probe: microseconds per step of GDMLPredict.run_npt (positions, velocities, forces, virial, cell and piston resident on
the device) on the configs[1] shape of the benchmark (N = 21, M = 1000, one permutation, the cubic 1000-unit cell of
tools/stress_probe.py), against two yardsticks measured in the same process:
  (a) GDMLPredict.run_md on the general route (predict.md_fused = 0) at the same B and with the same thermostat -- the same
      launches per step with the plain epilogue and desc_kernel instead of the virial epilogue and desc_cells_kernel; the
      expectation is the relax_cell / relax ratio of profiles/cellrelax_probe.json (1.13-1.23);
  (b) the host loop run_npt replaces, the only way before it: the same NPH step in NumPy around predict_stress, one call per
      replica per step (a call takes one lattice).

    python tools/npt_probe.py [--batches 1,8,64,1024] [--rounds 5] [--min-s 0.3] [--out profiles/npt_probe.json]

Every point alternates its variants for --rounds rounds; a round repeats one call (a trajectory of a fixed number of steps,
one recorded frame) for at least --min-s seconds after one warm-up call.  Reported per variant: the median of the rounds and
their spread (max - min) / median.  No rate is asserted anywhere: the file records what was measured."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from md_probe import DT, LANGEVIN, timed_steps  # noqa: E402
from stress_probe import N, M, SIG, build_predictor  # noqa: E402

PISTON_MASS = 1e9  # the cell of this shape holds vacuum: a piston so heavy that it stays where it is
NPT = dict(LANGEVIN, gamma_baro=0.5)


def host_nph(pred, R, V, masses3, lat, dt, n_steps, pressure, Wp):
    """The loop a user writes today: the NPH step of run_npt in NumPy, one predict_stress() per replica per step."""
    B, n3 = R.shape
    kappa = 1.0 + 3.0 / n3
    vol0 = abs(np.linalg.det(lat))
    eps, p_eps = np.zeros(B), np.zeros(B)

    def evaluate(R, eps):
        F, trW, E = np.empty_like(R), np.empty(B), np.empty(B)
        for b in range(B):
            lam = np.exp(eps[b])
            e, f, S = pred.predict_stress(R[b], lattice=lam * lat)
            E[b], F[b], trW[b] = e[0], f[0], np.trace(S[0]) * lam ** 3 * vol0
        return E, F, trW

    E, F, trW = evaluate(R, eps)
    K = (0.5 * masses3 * V * V).sum(axis=1)
    for _ in range(n_steps):
        p_eps = p_eps + 0.5 * dt * (kappa * 2.0 * K - trW - 3.0 * pressure * np.exp(3.0 * eps) * vol0)
        alpha = p_eps / Wp
        s = np.exp(-kappa * alpha * dt / 4.0)[:, None]
        V = s * (s * V + 0.5 * dt * F / masses3)
        q = np.exp(alpha * dt / 2.0)[:, None]
        R = q * (q * R + dt * V)
        eps = eps + alpha * dt
        E, F, trW = evaluate(R, eps)
        V = s * (s * V + 0.5 * dt * F / masses3)
        K = (0.5 * masses3 * V * V).sum(axis=1)
        p_eps = p_eps + 0.5 * dt * (kappa * 2.0 * K - trW - 3.0 * pressure * np.exp(3.0 * eps) * vol0)
    return R, V, E


def stats(v):
    med = float(np.median(v))
    return {'median_steps_per_s': med, 'us_per_step': 1e6 / med, 'rounds_steps_per_s': [float(x) for x in v],
            'spread': float((max(v) - min(v)) / med)}


def run_points(pred, Rq, batches, rounds, min_s):
    ctx = pred._ctx
    lat = np.asarray(pred.lat_and_inv[0], dtype=np.float64)
    masses = np.ones(N)
    out = []
    for B in batches:
        R0 = np.ascontiguousarray(np.resize(Rq, (B, 3 * N)))
        V0 = 0.01 * np.random.RandomState(1).standard_normal(R0.shape)
        n_dev = 1000 if B <= 8 else (500 if B <= 64 else 100)
        n_host = 100 if B == 1 else (20 if B <= 8 else (5 if B <= 64 else 2))

        def npt(th, n=n_dev):
            return lambda: pred.run_npt(R0, V0, masses, DT, n, 0.0, PISTON_MASS, record_every=n, record=('R',), **th)

        def md(th, n=n_dev):
            return lambda: pred.run_md(R0, V0, masses, DT, n, record_every=n, record=('R',), **th)

        variants = {'run_npt_nph': (npt({}), n_dev), 'run_npt_npt': (npt(NPT), n_dev),
                    'run_md_nve_general_route': (md({}), n_dev), 'run_md_langevin_general_route': (md(LANGEVIN), n_dev),
                    'host_loop_nph': (lambda: host_nph(pred, R0, V0, masses.repeat(3)[None], lat, DT, n_host, 0.0, PISTON_MASS),
                                      n_host)}
        rates = {k: [] for k in variants}
        ctx.set_option('predict.md_fused', 0)
        try:
            for _ in range(rounds):
                for k, (fn, n) in variants.items():
                    rates[k].append(timed_steps(fn, n, min_s))
        finally:
            ctx.set_option('predict.md_fused', 1)
        rec = {'N': N, 'M': M, 'B': B, 'steps_per_call': {k: n for k, (_, n) in variants.items()}}
        rec.update({k: stats(v) for k, v in rates.items()})
        rec['nph_over_run_md_nve_general_route'] = rec['run_npt_nph']['us_per_step'] / rec['run_md_nve_general_route']['us_per_step']
        rec['npt_over_run_md_langevin_general_route'] = (rec['run_npt_npt']['us_per_step'] /
                                                         rec['run_md_langevin_general_route']['us_per_step'])
        rec['host_loop_nph_over_run_npt_nph'] = rec['host_loop_nph']['us_per_step'] / rec['run_npt_nph']['us_per_step']
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
    result = {'shape': {'N': N, 'M': M, 'P': 1, 'sig': SIG, 'dt': DT, 'masses': 1.0, 'lattice': 'cubic, 1000 (nothing wraps)',
                        'pressure': 0.0, 'piston_mass': PISTON_MASS, 'npt': NPT},
              'yardsticks': {'run_md_general_route': 'GDMLPredict.run_md with predict.md_fused = 0, same B, same thermostat, '
                                                     'same process',
                             'host_loop_nph': 'the NPH step in NumPy around GDMLPredict.predict_stress, one call per replica '
                                              'per step, same process'},
              'points': run_points(pred, Rq, [int(b) for b in a.batches.split(',')], a.rounds, a.min_s)}
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()

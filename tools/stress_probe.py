"""Stress probe: host-to-host milliseconds of GDMLPredict.predict_stress against GDMLPredict.predict in the same process, on
the configs[1] shape of the benchmark (N = 21, M = 1000, one permutation) with a cubic cell large enough that nothing wraps.

    python tools/stress_probe.py [--batches 1,64,1000,16384] [--rounds 5] [--min-s 0.3] [--parent-lib LIB.so] [--out FILE.json]

Every point alternates the two calls for --rounds rounds; a round repeats one call for at least --min-s seconds and records the
mean time per call.  Reported per point: the median of the rounds and their spread (max - min) / median -- the run-to-run
noise any comparison in this file has to be read against.

--parent-lib: a libgdml_hip.so built from the parent commit.  predict() at B = 1 and B = 16384 is then timed in fresh child
processes that alternate between that library and this tree's (parent, this, parent, this, ...), three of each."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, M, SIG = 21, 1000, 20.0


def build_predictor(first_touch=True):
    from bench import synth_geometries
    from oracle import gdml_oracle as orc
    from sgdml_amd import _lib
    from sgdml_amd.predict import GDMLPredict

    lib = C.CDLL(_lib.LIB_PATH)  # a parent library has no virial entries: time what it has
    for name in ('gdml_predict_virial', 'gdml_predict_virial_dev'):
        if not hasattr(lib, name):
            _lib.SIGNATURES.pop(name, None)
    R, _, _ = synth_geometries(N, M + 64, seed=0)
    R = R.reshape(M + 64, -1)
    rng = np.random.RandomState(0)
    xd, _ = orc.desc_from_R(R[:M])
    tp = orc.tril_perms_from_atom_perms(np.arange(N)[None])
    model = {'type': 'm', 'z': np.ones(N, dtype=np.int64), 'R_desc': np.ascontiguousarray(xd.T),
             'R_d_desc_alpha': rng.normal(size=xd.shape), 'sig': SIG, 'std': 1.0, 'c': 0.0, 'perms': np.arange(N)[None],
             'tril_perms_lin': orc.tril_perms_lin_from_tril_perms(tp), 'lattice': 1000.0 * np.eye(3)}
    if first_touch:
        _lib.preflight()
    return GDMLPredict(model), R[M:]


def timed(fn, min_s):
    fn()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= min_s:
            return dt / n * 1e3


def stats(ms):
    med = float(np.median(ms))
    return {'median_ms': med, 'rounds_ms': [float(v) for v in ms], 'spread': float((max(ms) - min(ms)) / med)}


def run_points(batches, rounds, min_s, with_stress=True):
    pred, Rq = build_predictor(first_touch=with_stress)  # (the children follow the parent process's first touch)
    out = []
    for B in batches:
        R = np.ascontiguousarray(np.resize(Rq, (B, 3 * N)))
        t_p, t_s = [], []
        for _ in range(rounds):
            t_p.append(timed(lambda: pred.predict(R), min_s))
            if with_stress:
                t_s.append(timed(lambda: pred.predict_stress(R), min_s))
        rec = {'N': N, 'M': M, 'B': B, 'predict': stats(t_p)}
        if with_stress:
            rec['predict_stress'] = stats(t_s)
            rec['stress_over_predict'] = rec['predict_stress']['median_ms'] / rec['predict']['median_ms']
        print(json.dumps(rec), flush=True)
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,64,1000,16384')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--min-s', type=float, default=0.3)
    ap.add_argument('--parent-lib', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--child', action='store_true', help='internal: predict() only, one JSON line')
    a = ap.parse_args()
    batches = [int(b) for b in a.batches.split(',')]
    if a.child:
        print('CHILD ' + json.dumps(run_points(batches, a.rounds, a.min_s, with_stress=False)), flush=True)
        return
    result = {'shape': {'N': N, 'M': M, 'P': 1, 'sig': SIG, 'lattice': 'cubic, 1000 (nothing wraps)'},
              'points': run_points(batches, a.rounds, a.min_s)}
    if a.parent_lib:
        runs = []
        for k in range(6):  # fresh processes, alternating
            which = 'parent' if k % 2 == 0 else 'this'
            env = dict(os.environ)
            if which == 'parent':
                env['GDML_HIP_LIB'] = os.path.abspath(a.parent_lib)
            else:
                env.pop('GDML_HIP_LIB', None)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--batches', '1,16384', '--rounds',
                                str(a.rounds), '--min-s', str(a.min_s)], env=env, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:  # nothing more is started on the device after a failed run
                raise RuntimeError('child run (%s library) failed with %d: %s' % (which, p.returncode, p.stderr[-400:]))
            line = [l for l in p.stdout.splitlines() if l.startswith('CHILD ')][-1]
            for rec in json.loads(line[6:]):
                runs.append({'library': which, 'run': k // 2, 'B': rec['B'], 'median_ms': rec['predict']['median_ms'],
                             'spread': rec['predict']['spread']})
                print(json.dumps(runs[-1]), flush=True)
        summary = {}
        for B in (1, 16384):
            for which in ('parent', 'this'):
                v = [r['median_ms'] for r in runs if r['B'] == B and r['library'] == which]
                summary['B%d_%s' % (B, which)] = {'runs_ms': v, 'median_ms': float(np.median(v)),
                                                  'spread': float((max(v) - min(v)) / np.median(v))}
            summary['B%d_this_over_parent' % B] = summary['B%d_this' % B]['median_ms'] / summary['B%d_parent' % B]['median_ms']
        result['predict_vs_parent'] = {'runs': runs, 'summary': summary}
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(result, f, indent=1)


if __name__ == '__main__':
    main()

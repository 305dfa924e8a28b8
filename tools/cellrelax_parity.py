"""Parity record of the variable-cell relaxation over the cases of tests/test_cellrelax_gpu.py (profiles/cellrelax_parity.json):
per periodic fixture and batch the measured error of every compared quantity (Cartesian frames, lattice frames, end velocities,
E, Vol and f_atom histories) against the NumPy restatement (tests/_cellrelax_ref.py), the restatement's own deviation under the
predictor's agreed error (noise of 1e-10 on E, F and W) and their ratio (the test allows 1), beside the exact comparisons.

    python tools/cellrelax_parity.py [--out profiles/cellrelax_parity.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def measure():
    import _cellrelax_ref as cr
    from sgdml_amd.predict import GDMLPredict

    cases = []
    for name in cr.PARITY_FIXTURES:
        pred = GDMLPredict(cr.parity_case(name)[0])
        for B in cr.PARITY_BATCHES:
            m = cr.parity_measure(pred, name, B)
            cases.append(dict(fixture=name, B=B, evaluations=cr.PARITY_N_EVAL, pressure=cr.PARITY_PRESSURE, measured=m))
            print(name, B, ' '.join('%s %.2g' % (k, m[k]['ratio']) for k in cr.PARITY_KEYS), flush=True)
    worst = {k: max(c['measured'][k]['ratio'] for c in cases) for k in cr.PARITY_KEYS}
    flags = {k: all(c['measured'][k] for c in cases) for k in ('state_equal', 'none_converged', 'frames_are_the_end')}
    return dict(bound='error <= %g x sensitivity (+ 1e-10 of the largest value for the histories)' % cr.BOUND_FACTOR,
                sensitivity='deviation of a second restated run under independent noise of 1e-10 relative on E, F and W',
                worst_error_over_allowed=worst, all_cases=flags, cases=cases)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cellrelax_parity.json'))
    a = ap.parse_args()
    res = measure()
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(dict(worst_error_over_allowed=res['worst_error_over_allowed'], all_cases=res['all_cases']), indent=1))

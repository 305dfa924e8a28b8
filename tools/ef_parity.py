"""Parity record of the eigenvector-following search over the cases of tests/test_ef_gpu.py (profiles/ef_parity.json): per fixture,
order, follow vector and batch the measured error of every compared quantity against the NumPy restatement, the restatement's
own deviation under the predictor's agreed error (noise of 1e-10) and their ratio (the test allows 10), beside the exact
comparisons (trust radius, flags, followed index, the chain of one-step calls).

    python tools/ef_parity.py [--out profiles/ef_parity.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def measure():
    import _ef_ref as er
    from sgdml_amd.predict import GDMLPredict

    cases = []
    for name in er.PARITY_FIXTURES:
        pred = GDMLPredict(er.parity_start(name)[0])
        for order, with_follow in er.PARITY_MODES:
            for B in er.PARITY_BATCHES:
                m = er.parity_measure(pred, name, order, with_follow, B, chain=er.parity_chain(name, B))
                cases.append(dict(fixture=name, order=order, follow=with_follow, B=B, evaluations=er.PARITY_N_EVAL, measured=m))
                print(name, order, with_follow, B, ' '.join('%s %.2g' % (k, m[k]['ratio']) for k in er.PARITY_KEYS), flush=True)
    worst = {k: max(c['measured'][k]['ratio'] for c in cases) for k in er.PARITY_KEYS}
    flags = {k: all(c['measured'].get(k, True) for c in cases)
             for k in ('k_follow_equal', 'trust_equal', 'flags_equal', 'chain_equal', 'none_converged')}
    return dict(bound='error <= %g x sensitivity' % er.BOUND_FACTOR,
                sensitivity='deviation of a second restated run under force and Hessian noise of 1e-10 max, energy noise of 1e-10 max|E\'|',
                worst_error_over_sensitivity=worst, all_cases=flags, cases=cases)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ef_parity.json'))
    a = ap.parse_args()
    res = measure()
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(dict(worst_error_over_sensitivity=res['worst_error_over_sensitivity'], all_cases=res['all_cases']), indent=1))

"""Parity record of the analytic Hessians over the grid of tests/test_hessian_grid_gpu.py (profiles/hessian_grid_parity.json): per
case the host's plan (tests/_hessian_ref.py:hess_plan) and the measured error over bound of H, F and E against the long-double
reference, beside the other figures the test asserts on.

    python tools/hessian_grid_parity.py [--out profiles/hessian_grid_parity.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def measure():
    import _hessian_ref as hr
    from sgdml_amd.predict import GDMLPredict

    assert np.finfo(np.longdouble).eps < 1e-18, 'no extended precision on this host'
    runs = [(hr.size_case(N), 2, 0, 0) for N in hr.SIZE_N]
    runs += [(hr.row_case(N, MP), B, generic, chunk) for N in hr.ROW_N for MP, B, chunk in hr.ROW_CASES for generic in (0, 1)]
    cases, pred, resident = [], None, None
    for case, B, generic, chunk in runs:
        if case != resident:
            pred, resident = GDMLPredict(hr.grid_model(**case)[0]), case
        m = hr.grid_measure(pred, case, B, generic, chunk)
        plan = hr.hess_plan(case['N'], case['M'] * case['P'], B, generic, chunk)
        cases.append(dict(case=case, B=B, hess_generic=generic, hess_chunk_rows=chunk, plan=plan, measured=m))
        print(case['N'], case['M'] * case['P'], B, generic, chunk, plan['variant'], 'h %.3g f %.3g e %.3g' % (m['h'], m['f'], m['e']),
              flush=True)
    worst = {k: max(c['measured'][k] for c in cases) for k in ('h', 'f', 'e', 'sum_rule', 'f_predict', 'e_predict')}
    flags = {k: all(c['measured'][k] for c in cases) for k in ('symmetric', 'duplicates_equal', 'repeat_equal')}
    return dict(bounds=dict(h='1e-10 max|H_ld| per geometry', f='1e-10 max|F_ld|', e='1e-10 max(1, |E_ld|)',
                            sum_rule='1e-12 max|H|', f_predict='1e-12 max|F| + floor', e_predict='1e-12 max|E| + floors'),
                reference='hessian_ld (np.longdouble, eps = %.3g)' % np.finfo(np.longdouble).eps,
                worst_error_over_bound=worst, all_cases=flags, cases=cases)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hessian_grid_parity.json'))
    a = ap.parse_args()
    res = measure()
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
    print(json.dumps(dict(worst_error_over_bound=res['worst_error_over_bound'], all_cases=res['all_cases']), indent=1))

"""Parity record of the Nystroem build and application over the grid of tests/test_nys_edges_gpu.py
(profiles/nys_edges_parity.json): per case, option and check the measured ratio -- error / bound for the stage checks S1-S4,
error / allowance for the measured checks M1-M5 -- beside the allowance itself and the float64 restatement's own error
(tests/_nys_ref.py), and the largest ratio per check.

    python tools/nys_edges_parity.py [--out profiles/nys_edges_parity.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def _plain(x):
    """JSON-ready copy: three significant digits for floats, no arrays."""
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    if isinstance(x, (bool, np.bool_)):
        return bool(x)
    if isinstance(x, (int, np.integer)):
        return int(x)
    if isinstance(x, (float, np.floating)):
        return float('%.3g' % x)
    return x


def measure():
    import _nys_ref as nr
    from sgdml_amd import _lib

    assert np.finfo(np.longdouble).eps < 1e-18, 'no extended precision on this host'
    ctx = _lib.Context(0)
    cases, worst, failed = {}, {}, {}
    try:
        for group, key, run in nr.gpu_cases():
            t0 = time.time()
            res = run(ctx)
            q = nr.ratios(res)
            for k, v in q.items():
                chk = k.split('[')[0].split('.')[-1]
                worst[chk] = max(worst.get(chk, 0.0), v)
            bad = nr.failures(res)
            if bad:
                failed[key] = bad
            cases[key] = dict(group=group, seconds=round(time.time() - t0, 2), result=_plain(res))
            print('%s (%.1f s): ' % (key, time.time() - t0) + ', '.join('%s %.3g' % kv for kv in sorted(q.items())), flush=True)
    finally:
        ctx.close()
    return dict(what='error / bound of the stage checks S1-S4 and error / allowance of the measured checks M1-M5 of '
                     'tests/test_nys_edges_gpu.py, per case and option (the tests assert every ratio <= 1); X_allowance = 10 x '
                     'X_restatement, the largest error of the float64 restatement over three seeds; X_error = the device\'s',
                reference='np.longdouble, eps = %.3g' % np.finfo(np.longdouble).eps,
                worst_ratio=_plain(dict(sorted(worst.items()))), failed=failed, cases=cases)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nys_edges_parity.json'))
    a = ap.parse_args()
    res = measure()
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
    print(json.dumps(dict(worst_ratio=res['worst_ratio'], failed=res['failed']), indent=1))

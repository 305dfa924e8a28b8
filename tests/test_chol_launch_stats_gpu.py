"""Launch statistics of the factorisation (gdml_kernel_stat) against a record: tests/golden/chol_launch_stats.json holds, per
case, the launches and the algorithmic flops that the per-kernel timers report for gemm_nt_sub_diag, gemm_nt_sub,
gemm_nt_sub_deep and panel_trsm.  It was written by this module's --record mode on the commit BEFORE the host side of
csrc/chol.hip was rewritten around launch descriptions (PlanLowerLaunch, tile_sched.h), so a change of the launch code that
moves, drops or recounts a launch fails here.

Cases: the four of tests/test_chol_deep_gpu.py, each with chol.deep = 0 and with its W; the three option sets of
tests/test_tile_balance_gpu.py, each with gemm.balance = 0 and 1; every one with and without the carried right-hand-side
row; matrix family 'a' of tests/_chol_ref.py.  Asserted: info = 0, a finite factor, equal launch counts, flops equal to
1e-12 relative (sums of exactly representable per-launch counts: only the order of adding them may differ).  That the
factors of two schedules are bitwise equal is asserted by those two modules and not repeated.

    python tests/test_chol_launch_stats_gpu.py --record [path]     # rewrites the record from the library in the tree
"""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _chol_ref as cr  # noqa: E402
import test_chol_deep_gpu as deep_cases  # noqa: E402
import test_tile_balance_gpu as balance_cases  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'chol_launch_stats.json')
KERNELS = ('gemm_nt_sub_diag', 'gemm_nt_sub', 'gemm_nt_sub_deep', 'panel_trsm')


def _cases():
    """id -> (n, with_rhs, options), cases of one n next to each other (one cached matrix at a time)."""
    out = {}
    for name, (n, W, deep_min) in deep_cases.CASES.items():
        for tag, extra in (('deep0', {'chol.deep': 0}), ('deepW', {'chol.deep': W, 'chol.deep_min_rows': deep_min})):
            for rhs in (False, True):
                out['%s-%s-%s' % (name, tag, 'rhs' if rhs else 'norhs')] = (n, rhs, dict(deep_cases.BASE, **extra))
    for p in balance_cases.CASES:
        n, _, opts = p.values
        for bal in (0, 1):
            for rhs in (False, True):
                out['n%d-balance%d-%s' % (n, bal, 'rhs' if rhs else 'norhs')] = (n, rhs, dict(opts, **{'gemm.balance': bal}))
    return dict(sorted(out.items(), key=lambda kv: (kv[1][0], kv[0])))


CASES = _cases()


def run_case(n, with_rhs, opts):
    """(info, factor finite, {kernel: [launches, flops]})"""
    from sgdml_amd import _lib

    A, y = cr.reference('a', n)[:2]
    c = _lib.Context()
    try:
        for k, v in opts.items():
            c.set_option(k, v)
        cr.load_spd(c, n, A, y if with_rhs else None)
        c.profile(True)
        info = c.chol_factor(0.0)
        stat = {k: [int(c.kernel_stat(k)[1]), float(c.kernel_stat(k)[2])] for k in KERNELS}
        c.profile(False)
        buf = c.K_to_host()
        finite = bool(np.isfinite(np.tril(buf[:n, :n])).all()) and (not with_rhs or bool(np.isfinite(buf[n, :n]).all()))
        return info, finite, stat
    finally:
        c.close()


@pytest.fixture(scope='module')
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize('case', list(CASES))
def test_launch_statistics_equal_the_record(case, golden):
    info, finite, stat = run_case(*CASES[case])
    want = golden[case]
    print(case, stat, want)
    assert info == 0 and finite
    for k in KERNELS:
        assert stat[k][0] == want[k][0], (k, stat[k], want[k])
        assert abs(stat[k][1] - want[k][1]) <= 1e-12 * abs(want[k][1]), (k, stat[k], want[k])


def test_the_record_names_exactly_the_cases(golden):
    assert sorted(golden) == sorted(CASES)


if __name__ == '__main__':
    if len(sys.argv) < 2 or sys.argv[1] != '--record':
        sys.exit(__doc__)
    rec = {}
    for case, args in CASES.items():
        info, finite, stat = run_case(*args)
        assert info == 0 and finite, case
        rec[case] = stat
        print(case, stat, flush=True)
    path = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    with open(path, 'w') as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write('\n')

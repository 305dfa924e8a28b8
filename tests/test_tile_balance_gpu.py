"""Balanced tile lists of the lower trailing updates (csrc/tile_sched.h, option gemm.balance) on the GPU: the factor must be
bit-identical to the one of the super-tile enumeration (gemm.balance = 0) -- every C tile gets the same arithmetic in the
same k order, only the workgroup that computes it changes.  Matrices, loading and bounds are those of tests/_chol_ref.py;
the options make the pair, the single fused and the tail arm of the schedule each occur at these small orders."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _chol_ref as cr  # noqa: E402

pytestmark = pytest.mark.gpu

STAT_KERNELS = ('gemm_nt_sub_diag', 'gemm_nt_sub', 'panel_trsm')

CASES = [
    # n = 2500 + carried row: 20 tile rows, 3 super rows, ragged last super row, fewer super tiles than XCDs
    pytest.param(2500, True, {'chol.nb': 128, 'chol.outer': 256, 'chol.outer_min_rows': 1500, 'chol.fused_min_rows': 700},
                 id='n2500-rhs'),
    # n = 4224: 33 tile rows, 5 super rows
    pytest.param(4224, False, {'chol.nb': 128, 'chol.outer': 256, 'chol.outer_min_rows': 2000, 'chol.fused_min_rows': 1000},
                 id='n4224-norhs'),
    # n = 3072: 24 tile rows, a multiple of 8
    pytest.param(3072, True, {'chol.nb': 128, 'chol.outer': 256, 'chol.outer_min_rows': 1500, 'chol.fused_min_rows': 700},
                 id='n3072-rhs'),
]


def _factor(n, A, y, opts, balance):
    from sgdml_amd import _lib

    c = _lib.Context()
    try:
        for k, v in opts.items():
            c.set_option(k, v)
        c.set_option('gemm.balance', balance)
        cr.load_spd(c, n, A, y)
        c.profile(True)
        info = c.chol_factor(0.0)
        counts = {k: c.kernel_stat(k)[1] for k in STAT_KERNELS}
        c.profile(False)
        buf = c.K_to_host()
        return info, counts, np.tril(buf[:n, :n]), (buf[n, :n].copy() if y is not None else None)
    finally:
        c.close()


@pytest.mark.parametrize('n,with_rhs,opts', CASES)
def test_balanced_factor_is_bit_identical(n, with_rhs, opts):
    A, y, _, _, _ = cr.reference('a', n)
    arms, want = cr.schedule(n, with_rhs, opts['chol.nb'], opts['chol.outer'], opts['chol.fused_min_rows'],
                             opts['chol.outer_min_rows'])
    assert {a[0] for a in arms} >= {'pair', 'single', 'tail'}, arms
    info0, counts0, L0, row0 = _factor(n, A, y if with_rhs else None, opts, 0)
    info1, counts1, L1, row1 = _factor(n, A, y if with_rhs else None, opts, 1)
    assert info0 == 0 and info1 == 0
    assert counts0 == counts1 == want, (counts0, counts1, want)
    assert np.isfinite(L1).all()
    assert np.array_equal(L0, L1), 'lower triangle differs in %d entries' % int((L0 != L1).sum())
    if with_rhs:
        assert np.array_equal(row0, row1), 'carried row differs'
    q = cr.factor_ratio(A, L1)
    print('n = %d: factor at %.3g of factor_bound' % (n, q))
    assert q <= 2.0  # the bound tests/test_chol_edges_gpu.py asserts (its docstring, (i))

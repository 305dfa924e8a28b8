"""Cholesky and triangular solves on the GPU (csrc/chol.hip) at the block and panel edges of every schedule branch, against
SciPy in fp64 on the host (tests/_chol_ref.py; its inputs and bounds are checked without a GPU by test_chol_edges_cpu.py).

Every case asserts
  (i)   |A - L L^T| <= 2 factor_bound componentwise on the lower triangle (factor_bound assumes correctly rounded operations;
        the kernels take 1/sqrt by a hardware estimate and two Newton steps, which is not proven correctly rounded: factor 2),
  (ii)  family 'a' only: max|L - L_ref| <= 1e-11 max|L_ref| (the tolerance of tests/test_hip_parity.py at this conditioning),
  (iii) |y - A x| <= solve_bound componentwise; with a carried right-hand side chol_solve(None) and chol_solve(y) agree,
  (iv)  no NaN in L or x, although the strict upper triangle and the pitch padding of the buffer are loaded as NaN,
and, where options select an arm of the schedule, that the per-kernel timers report the launches of exactly that arm
(_chol_ref.schedule restates the host logic; a threshold that quietly routes elsewhere changes the counts).
The largest ratios of the device's and of SciPy's factor to factor_bound go to profiles/chol_edges_parity.json."""
import json
import os
import re
import sys

import numpy as np
import pytest
import scipy.linalg as sla

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _chol_ref as cr  # noqa: E402

pytestmark = pytest.mark.gpu

RECORD = os.environ.get('GDML_CHOL_EDGES_RECORD', os.path.join(ROOT, 'profiles', 'chol_edges_parity.json'))
STAT_KERNELS = ('gemm_nt_sub_diag', 'gemm_nt_sub', 'panel_trsm')
_observed = {}
_expected = []


def _cases(prefix, rows):
    """pytest params with ids; the ids double as the keys of the record file."""
    out = []
    for r in rows:
        key = prefix + '-' + '-'.join(str(v) for v in r[0])
        _expected.append(key)
        out.append(pytest.param(key, *r[1], id=key))
    return out


@pytest.fixture(scope='module')
def ctx():
    from sgdml_amd import _lib

    c = _lib.Context()
    yield c
    c.close()


@pytest.fixture
def ctx_factory():
    from sgdml_amd import _lib

    made = []

    def make(opts=None):
        c = _lib.Context()
        made.append(c)
        for k, v in (opts or {}).items():
            c.set_option(k, v)
        return c

    yield make
    for c in made:
        c.close()


@pytest.fixture(scope='module', autouse=True)
def _record():
    yield
    if all(k in _observed for k in _expected):  # a full run of the module only
        with open(RECORD, 'w') as f:
            json.dump({'what': 'largest |A - L L^T|_ij / (gamma_{n+1} (|L||L^T|)_ij) over the lower triangle, per case, of the '
                               'device factor and of SciPy\'s factor of the same matrix (the tests assert device <= 2), and the '
                               'largest |y - A x|_i / solve_bound_i of the device solves (tests/test_chol_edges_gpu.py; case = '
                               'group-size-family-rhs row or options)',
                       'ratio': {k: _observed[k] for k in _expected}}, f, indent=1)
            f.write('\n')


def _sched(n, with_rhs, opts):
    return cr.schedule(n, with_rhs, opts.get('chol.nb', 512), opts.get('chol.outer', 1024),
                       opts.get('chol.fused_min_rows', 12288), opts.get('chol.outer_min_rows', 16384))


def _factor_and_check(c, key, family, n, with_rhs, opts=None):
    """Load, factor, check (i)-(iv) and the launch counts of the arms; returns (A, y, L, G)."""
    A, y, Lref, Gref, _ = cr.reference(family, n)
    cr.load_spd(c, n, A, y if with_rhs else None)
    c.profile(True)
    assert c.chol_factor(0.0) == 0
    got = {k: c.kernel_stat(k)[1] for k in STAT_KERNELS}
    c.profile(False)
    arms, want = _sched(n, with_rhs, opts or {})
    assert got == want, (got, want, arms)
    L = np.tril(c.K_to_host()[:n])
    assert np.isfinite(L).all(), 'NaN from the scratch triangle or the padding leaked into L'
    G = cr.abs_gram(L)
    q_dev, q_ref = cr.factor_ratio(A, L, G), cr.factor_ratio(A, Lref, Gref)
    q_L = np.abs(L - Lref).max() / np.abs(Lref).max()
    xs = {'y': -c.chol_solve(y)}
    if with_rhs:
        xs['row'] = -c.chol_solve(None)
    for x in xs.values():
        assert np.isfinite(x).all(), 'NaN leaked into x'
    q_x = max(cr.solve_ratio(A, G, x, y) for x in xs.values())
    q_agree = cr.agree_ratio(A, G, xs['y'], xs['row']) if with_rhs else 0.0
    print('%s: factor %.3g (SciPy %.3g) of factor_bound, max|dL| / max|L| = %.3g, solve %.3g, carried row vs y %.3g of '
          'solve_bound' % (key, q_dev, q_ref, q_L, q_x, q_agree))
    if key in _expected:
        _observed[key] = {'device': float('%.3g' % q_dev), 'scipy': float('%.3g' % q_ref), 'solve': float('%.3g' % q_x)}
    assert q_dev <= 2.0                      # (i)
    if family == 'a':
        assert q_L <= 1e-11                  # (ii)
    assert q_x <= 1.0 and q_agree <= 1.0     # (iii)
    return A, y, L, G


FAMILY_RHS = [(f, r) for f in 'ab' for r in (False, True)]


@pytest.mark.parametrize('key,n,family,with_rhs', _cases('edge', [
    ((n, f, 'rhs' if r else 'norhs'), (n, f, r)) for n in cr.BLOCK_EDGE_SIZES for f, r in FAMILY_RHS]))
def test_block_edges_default_options(ctx, key, n, family, with_rhs):
    """Default options.  n < 64: the first panel is the whole matrix and narrower than a block (lone potrf64_kernel; with the
    right-hand-side row a ragged potrf_trsm64_kernel).  64, 128, 512: whole blocks, the last step of the chain has no rows
    below (writeback_block_kernel flush + lone potrf64_kernel) unless the carried row is there (then the `below > 0` split
    of panel_factor: step chain over the block + row-local solve of one row).  65, 126, 130, 511: ragged last step.  513,
    576, 1022: one panel behind the first ('last' arm: 1, 64, 510 columns), 1024: the tail arm with one panel and a 512-wide
    last one, 1026: tail + ragged last.  Without the carried row chol_solve(y) runs the forward substitution on its own
    (63, 64, 65: one block ragged, one block full, two blocks with a 1-row second one)."""
    _factor_and_check(ctx, key, family, n, with_rhs)


@pytest.mark.parametrize('key,with_rhs', _cases('switch', [((cr.SWITCH_N, 'a', 'rhs' if r else 'norhs'), (r,)) for r in (False, True)]))
def test_rows_below_first_block_around_2048(ctx, key, with_rhs):
    """2048 rows below the first 64-block (n = 2112) and 2049 (the same with the carried row): the sizes on either side of
    the `m <= 2048` test in panel_factor_steps.  On the resident path the step chain of an aligned panel only spans the
    panel's own rows (m <= 448) and a ragged panel is the last one (m <= 512), so rank64_update_kernel serves both: the
    test pins that the result does not depend on which side the size falls."""
    _factor_and_check(ctx, key, 'a', cr.SWITCH_N, with_rhs)


@pytest.mark.parametrize('key,nb,family,with_rhs', _cases('nb_single', [
    ((nb, f, 'rhs' if r else 'norhs'), (nb, f, r)) for nb in cr.NB_SINGLE for f, r in FAMILY_RHS]))
def test_panel_widths_fused_single(ctx_factory, key, nb, family, with_rhs):
    """chol.nb = 64 ... 448 at n = 1026 (ragged against all of them), chol.fused_min_rows = 1: every panel but the last is
    factored by workgroup 0 of a fused launch (gemm_nt_sub_diag launches = panels - 2)."""
    opts = {'chol.nb': nb, 'chol.outer': nb, 'chol.fused_min_rows': 1}
    arms, want = _sched(cr.NB_SWEEP_N, with_rhs, opts)
    assert want['gemm_nt_sub_diag'] == len(arms) - 1 >= 1
    _factor_and_check(ctx_factory(opts), key, family, cr.NB_SWEEP_N, with_rhs, opts)


@pytest.mark.parametrize('key,nb,family,with_rhs', _cases('nb_pair', [
    ((nb, f, 'rhs' if r else 'norhs'), (nb, f, r)) for nb in cr.NB_PAIR + (192,) for f, r in FAMILY_RHS]))
def test_panel_widths_pairs(ctx_factory, key, nb, family, with_rhs):
    """chol.nb = 128, 256, 384 with chol.outer = 2 nb at n = 1542: panel pairs (two fused launches each, the second with the
    K = nb update of b's columns in front), then a single panel and the ragged last one.  192 is not a multiple of the
    128-row tile the diagonal-block counter counts in: the gate must route it to single panels."""
    opts = {'chol.nb': nb, 'chol.outer': 2 * nb, 'chol.outer_min_rows': 1, 'chol.fused_min_rows': 1}
    arms, _ = _sched(cr.NB_PAIR_N, with_rhs, opts)
    assert (arms[0][0] == 'pair') == (nb != 192)
    _factor_and_check(ctx_factory(opts), key, family, cr.NB_PAIR_N, with_rhs, opts)


@pytest.mark.parametrize('key,n,opts,family,with_rhs', _cases('arm', [
    ((c[0], f, 'rhs' if r else 'norhs'), (c[1], c[2], f, r)) for c in cr.ARM_EDGES for f, r in FAMILY_RHS]))
def test_arm_edges_nb512(ctx_factory, key, n, opts, family, with_rhs):
    """The thresholds between the arms at chol.nb = 512, each at its edge (the cases and what they walk: _chol_ref.ARM_EDGES;
    test_chol_edges_cpu.py checks that each case has the arms it names)."""
    _factor_and_check(ctx_factory(opts), key, family, n, with_rhs, opts)


@pytest.mark.parametrize('n,family', [(2046, 'a'), (2048, 'a'), (2070, 'a'), (2070, 'b')])
def test_backward_substitution_persistent_and_per_block(ctx_factory, n, family):
    """trsv.persist = 1 and 0 on the same factor, below (2046), at (2048) and above the persistent kernel's threshold with a
    ragged last 64-block (2070 = 32 * 64 + 22): each against scipy.linalg.solve_triangular on the device's own L, and
    against each other, within solve_bound; the launch count of the solve phase tells which kernel ran (a persistent launch
    that gives up and falls back shows as one launch too many)."""
    c = ctx_factory()
    A, y, L, G = _factor_and_check(c, 'bwd-%d-%s' % (n, family), family, n, False)
    z = sla.solve_triangular(L, y, lower=True, check_finite=False)
    x_tri = sla.solve_triangular(L, z, lower=True, trans='T', check_finite=False)
    xs = {}
    for persist in (1, 0):
        c.set_option('trsv.persist', persist)
        xs[persist] = -c.chol_solve(y)
        assert c.phase_ms('solve')[1] == cr.solve_launches(n, persist)
        assert np.isfinite(xs[persist]).all()
        q = cr.solve_ratio(A, G, xs[persist], y), cr.agree_ratio(A, G, xs[persist], x_tri)
        print('n = %d persist = %d: residual %.3g, against solve_triangular %.3g of solve_bound' % ((n, persist) + q))
        assert max(q) <= 1.0
    q = cr.agree_ratio(A, G, xs[0], xs[1])
    print('n = %d: persist 0 against 1: %.3g of solve_bound' % (n, q))
    assert q <= 1.0
    if n < 2048:  # the option changes nothing below the threshold
        assert np.array_equal(xs[0], xs[1])


@pytest.mark.parametrize('name,n,opts,p', cr.NOT_PD, ids=[c[0] for c in cr.NOT_PD])
def test_not_positive_definite_reports_lapack_index(ctx_factory, name, n, opts, p):
    """The identity with a single -1 at diagonal index p: info is LAPACK's 1-based p + 1 from whichever kernel meets it
    (potrf_trsm64_kernel at c0 = 0 and 64, the lone potrf64_kernel of a ragged last block, the step chain of the tail arm on
    the second stream, diag_block_role inside a fused launch: single panel, block a and block b of a pair), and the context
    then refuses to factor the consumed matrix.  A failed pivot is an error return: diag_block_role goes on (NaN) and
    returns, the only wait of a fused launch is workgroup 0's bounded wait for tile counts that do not depend on values."""
    from sgdml_amd import _lib

    c = ctx_factory(opts)
    A = np.eye(n)
    A[p, p] = -1.0
    cr.load_spd(c, n, A)
    c.profile(True)
    with pytest.raises(np.linalg.LinAlgError) as e:
        c.chol_factor(0.0)
    m = re.search(r'(\d+)-th leading minor of the array is not positive definite', str(e.value))
    assert m and int(m.group(1)) == p + 1, str(e.value)
    got = {k: c.kernel_stat(k)[1] for k in STAT_KERNELS}
    c.profile(False)
    assert got == _sched(n, False, opts)[1]  # the whole schedule ran, in the arms the case names
    with pytest.raises(_lib.GDMLHipError, match='consumed by a failed factorisation'):
        c.chol_factor(0.0)
    with pytest.raises(_lib.GDMLHipError, match='no Cholesky factor resident'):
        c.chol_solve(np.ones(n))

"""The Nystroem build and its application on the GPU (csrc/nystroem.hip: gdml_nystroem_factor, gdml_nystroem_lev_scores on
gram_tn.hip and tall_trsm of chol_solve.hip; csrc/precon_apply.hip: gdml_precon_apply) at the edges of every kernel branch, against long-double references on the host (tests/_nys_ref.py;
its bounds, allowances and case tables are checked without a GPU by tests/test_nys_edges_cpu.py).

Every case loads ITS matrix into the resident buffer with the pitch padding and the m-row work block set to NaN, runs the
library and asserts
  stage checks S1-S4: derived componentwise bounds on what each stage makes of the inputs read back from the device
                      (ratio error / bound <= 1), S5: bit comparisons of the in-place fp32 overlay with the fp32 copy,
  measured checks M1-M5: error against the long-double reference <= 10 x the largest error of the float64 restatement
                      over three seeds (ratio error / allowance <= 1),
  that nothing read back holds a NaN, and that the info bits name the branch the case was built for.
One parametrised test per group; after the last case of a group the context is used once more with default options.
tools/nys_edges_parity.py records the ratios in profiles/nys_edges_parity.json."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _nys_ref as nr  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = nr.gpu_cases()


@pytest.fixture(scope='module')
def ctx():
    from sgdml_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


def _group(name):
    rows = [(k, run) for g, k, run in CASES if g == name]
    return [pytest.param(k, run, k == rows[-1][0], id=k) for k, run in rows]


def _check(ctx, key, run, last):
    try:
        res = run(ctx)
        q = nr.ratios(res)
        print('%s: ' % key + ', '.join('%s %.3g' % kv for kv in sorted(q.items())))
        bad = nr.failures(res)
        assert not bad, bad
    finally:
        for k, v in nr.options.DEFAULTS.items():
            ctx.set_option(k, v)
    if last:
        assert nr.still_usable(ctx)


@pytest.mark.parametrize('key,run,last', _group('gram_tiles'))
def test_gram_tiles(ctx, key, run, last):
    """syrk_tn_tile<true / false>, the guarded k tail, the triangular tile index: S1, M1."""
    _check(ctx, key, run, last)


@pytest.mark.parametrize('key,run,last', _group('gram_split'))
def test_gram_split(ctx, key, run, last):
    """syrk_tn_split_kernel + gram_sum_parts_kernel (S = 2, second range 8184 rows) and the one-pass form: S1, S2."""
    _check(ctx, key, run, last)


@pytest.mark.parametrize('key,run,last', _group('solves'))
def test_solves(ctx, key, run, last):
    """tall_trsm: the panel branch, the trsm64 loop with w = 1, 2, 13, 63, left- and right-looking updates across a
    512-column strip: S2, M4 (S1 at m = 513, 576)."""
    _check(ctx, key, run, last)


@pytest.mark.parametrize('key,run,last', _group('gemv64'))
def test_fp64_gemvs(ctx, key, run, last):
    """gemv_t_part_kernel, reduce_parts_kernel, gemv_n_precon_kernel, row_sqnorm_kernel: S3, S4; pcg.gemv_plain 0 and 1
    bit-equal."""
    _check(ctx, key, run, last)


@pytest.mark.parametrize('key,run,last', _group('f32_form'))
def test_fp32_form(ctx, key, run, last):
    """build_f32_form and the fp32 GEMVs at m % 4 = 1, 2, 3, 0 and m = 525, with 256-row Gram chunks, 64-row parts,
    pcg.f32_rw 1 / 2 / 4, plain loads, in place and with a separate copy: S5, and M2 for every variant on its own."""
    _check(ctx, key, run, last)


@pytest.mark.parametrize('key,run,last', _group('qr'))
def test_cholesky_qr_branch(ctx, key, run, last):
    """nys.force_qr: the Gram matrix over the n + m stacked rows, three solve rounds: M3."""
    _check(ctx, key, run, last)


@pytest.mark.parametrize('key,run,last', _group('conditioning'))
def test_stage_checks_do_not_depend_on_conditioning(ctx, key, run, last):
    """Six decades in K_mm and in X1^T X1 + lam I, lam = 1e-6: S1, S2, S4 only."""
    _check(ctx, key, run, last)


@pytest.mark.parametrize('key,run,last', _group('matrix_free'))
def test_matrix_free_form(ctx, key, run, last):
    """A really assembled system, nothing overwritten: gather / scatter, gemv_t_part_kernel<false> on Z with two row parts,
    gemv_n_precon_kernel<false, false>, precon_finish_kernel: M5 against nys_ld on the oracle's K_nm."""
    _check(ctx, key, run, last)

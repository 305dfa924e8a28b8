"""Plans of the Nystroem build and of the preconditioner application (csrc/precon_plan.h) without a GPU:
tests/precon_plan_driver.cpp is compiled with the host compiler (address and undefined-behaviour sanitizers where the toolchain
has them; the program has its own main) and prints every field of gram_split_plan, choose_precon_form, f32_gram_chunk and
precon_apply_plan for each request.

The reference is not the header: tests/_nys_ref.py (gram_plan, apply_plan, the chunk clamp of f32_form_f64) restates what
gram_tn, build_f32_form and precon_apply_device computed inline before the header existed.  The GPU grid
(tests/test_nys_edges_gpu.py) and tests/test_nys_edges_cpu.py rest on that restatement; this test is what ties it to the
compiled arithmetic, field by field.

Inputs: every case of the grid with the option variants the GPU grid uses (nys.syrk_split 0 / 1, pcg.f32_rows_per 64 / 1024,
pcg.f32_rw 0 ... 5, pcg.gemv_plain 0 / 1); n_loc in {0, 1, 7, 8, 63, 64, 65, 2047, 2048, 2049} x m = 1 ... 1030 for forms 0 and
3; gram_split_plan on both sides of each of its limits -- the tile target (8192 is no triangular number: T = 8128 | 8256 at
127 | 128 tile rows), n / S = 8191 | 8192 for S = 2 ... 8, S m ldc 8 at and just above 2 GiB; the three iterative shapes of
bench.py (n = 315 000, 252 000, 900 000 with m = 9072, 18018, 7200); choose_precon_form at 8 chunk m = 2^30 - 8 | 2^30.

Independent of the restatement: t starts at an even offset; part, t, u do not overlap and the workspace covers the last of
them; u holds the padded m; the row ranges of the split cover [0, n) exactly once and every range but the last is a
multiple of 16; parts, column blocks and row blocks cover n_loc and m; the launches and the work figure are those of the form."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _nys_ref as nr  # noqa: E402

SRC = os.path.join(ROOT, 'tests', 'precon_plan_driver.cpp')
N_SWEEP = (0, 1, 7, 8, 63, 64, 65, 2047, 2048, 2049)
BENCH_SHAPES = ((315000, 9072), (252000, 18018), (900000, 7200))
GIB2 = 2 << 30


def _gram_inputs():
    """(n, m, ldc, split)"""
    rows = [(n, m, nr.round16(m), s) for n, m, _, _ in nr.grid_cases() for s in (0, 1)]
    rows += [(n, m, nr.round16(m), s) for n, m in BENCH_SHAPES for s in (0, 1)]
    rows += [(10**6, m, nr.round16(m), 1) for m in (127 * 128, 127 * 128 + 1)]          # T = 8128 | 8256
    rows += [(S * 8192 - d, 129, 144, 1) for S in range(2, 9) for d in (1, 0)]          # n / S = 8191 | 8192
    rows += [(10**6, 8192, ldc, 1) for ldc in (8192, 8208, 16384, 16400)]               # S = 4 | 2 at 2 GiB, and 16 columns more
    return rows


def _apply_inputs():
    """(form, n_loc, m, ld, gemv_plain, f32_rows_per, f32_rw)"""
    rows = []
    for n, m in sorted({c[:2] for c in nr.grid_cases()}) + list(BENCH_SHAPES):
        rows += [(0, n, m, nr.round16(m), plain, 1024, 4) for plain in (0, 1)]
        rows += [(3, n, m, nr.round16(m), plain, rp, rw) for plain in (0, 1) for rp in (64, 1024) for rw in range(6)]
    for n in N_SWEEP:
        for m in range(1, 1031):
            rows.append((0, n, m, nr.round16(m), 0, 1024, 4))
            rows += [(3, n, m, nr.round16(m), 0, rp, rw) for rp, rw in ((1024, 4), (64, 4), (1024, 1), (1024, 2))]
    return rows


def _form_inputs():
    """(option, chunk, m)"""
    return [(o, chunk, m) for o in (0, 1, 2, 3) for chunk, m in ((2**27 - 1, 1), (2**27, 1), (2**17, 2**10), (2**17 - 1, 2**10), (594, 130))]


def _chunk_inputs():
    """(pcg.f32_gram_rows, n_loc)"""
    return [(o, n) for o in (0, 100, 255, 256, 257, 300, 2047, 2048) for n in N_SWEEP + (594,)]


def _requests():
    return ([('gram',) + r for r in _gram_inputs()] + [('form',) + r for r in _form_inputs()] +
            [('chunk',) + r for r in _chunk_inputs()] + [('apply',) + r for r in _apply_inputs()])


def _compiler():
    for name in ('g++', 'c++', 'clang++', '/opt/rocm/lib/llvm/bin/clang++', '/opt/rocm/llvm/bin/clang++'):
        path = shutil.which(name)
        if path:
            return path
    raise AssertionError('no host C++ compiler found')


@pytest.fixture(scope='module')
def drivers(tmp_path_factory):
    """The sanitized program (runtime linked statically where the compiler can) and the plain one."""
    d = tmp_path_factory.mktemp('precon_plan')
    base = [_compiler(), '-std=c++17', '-O1', '-g', '-Wall', SRC, '-o']
    plain = str(d / 'driver')
    subprocess.run(base + [plain], check=True)
    san_flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    for extra in (['-static-libasan', '-static-libubsan'], []):
        san = str(d / 'driver_san')
        if subprocess.run(base + [san] + san_flags + extra, capture_output=True, text=True).returncode == 0:
            return [san, plain]
    return [plain]  # toolchain without the sanitizer runtimes


@pytest.fixture(scope='module')
def plans(drivers):
    """{kind: [(input tuple, {field: value})]} as every built program computes them (the programs agree)."""
    reqs = _requests()
    text = ''.join(' '.join(str(v) for v in r) + '\n' for r in reqs)
    outs = []
    for exe in drivers:
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        print(exe, r.returncode, r.stderr[-4000:])
        if r.returncode != 0 and 'does not come first' in r.stderr:
            continue  # a preloaded library keeps the sanitizer's runtime from starting: the plain program computes the same
        assert r.returncode == 0
        outs.append(r.stdout)
    assert outs and all(o == outs[0] for o in outs)
    lines = outs[0].splitlines()
    assert len(lines) == len(reqs)
    out = {}
    for req, line in zip(reqs, lines):
        head, tail = line.split(' : ')
        assert head.split() == [str(v) for v in req], line
        tok = tail.split()
        out.setdefault(req[0], []).append((req[1:], {k: float(v) if k == 'work' else int(v) for k, v in zip(tok[0::2], tok[1::2])}))
    return out


def _ranges(n, S, rows_per):
    return [(s * rows_per, max(s * rows_per, min(n, (s + 1) * rows_per))) for s in range(S)]


def test_gram_split_plan_is_the_restatement(plans):
    seen_S = set()
    for (n, m, ldc, split), p in plans['gram']:
        want = nr.gram_plan(n, m, split, ldc)
        got = dict(tiles=p['tiles'], T=p['T'], S=p['S'], rows_per=p['rows_per'], ranges=_ranges(n, p['S'], p['rows_per']))
        assert got == {k: want[k] for k in got}, ((n, m, ldc, split), p, want)
        assert p['part_bytes'] == (p['S'] * m * ldc * 8 if p['S'] > 1 else 0)
        seen_S.add(p['S'])
        # the ranges cover [0, n) exactly once; every range but the last is a multiple of 16
        r = got['ranges']
        assert r[0][0] == 0 and r[-1][1] == n and all(a[1] == b[0] for a, b in zip(r, r[1:])), (n, m, r)
        assert all((b - a) % nr.TBK == 0 for a, b in r[:-1]), (n, m, r)
        assert split or p['S'] == 1
        assert p['part_bytes'] <= GIB2 and (p['S'] == 1 or n // p['S'] >= 8192)
    assert seen_S == set(range(1, 9))
    by = {k: p for k, p in plans['gram']}
    # both sides of each limit
    assert by[(10**6, 127 * 128, 127 * 128, 1)]['T'] == 8128 and by[(10**6, 127 * 128 + 1, nr.round16(127 * 128 + 1), 1)]['T'] == 8256
    assert by[(10**6, 127 * 128 + 1, nr.round16(127 * 128 + 1), 1)]['S'] == 1
    for S in range(2, 9):
        assert by[(S * 8192, 129, 144, 1)]['S'] == S and by[(S * 8192 - 1, 129, 144, 1)]['S'] == S - 1
    assert [by[(10**6, 8192, ldc, 1)]['S'] for ldc in (8192, 8208, 16384, 16400)] == [4, 3, 2, 1]
    assert by[(10**6, 8192, 8192, 1)]['part_bytes'] == GIB2 == by[(10**6, 8192, 16384, 1)]['part_bytes']


def test_precon_form_and_gram_chunk(plans):
    for (option, chunk, m), p in plans['form']:
        want = option if option in (0, 1, 3) else (3 if 8 * chunk * m >= 2**30 else 0)
        assert p['form'] == want, (option, chunk, m, p)
    by = {k: p['form'] for k, p in plans['form']}
    assert by[(2, 2**27 - 1, 1)] == 0 and by[(2, 2**27, 1)] == 3  # 8 chunk m = 2^30 - 8 | 2^30
    for (option, n_loc), p in plans['chunk']:
        if n_loc > 0:  # the clamp as tests/_nys_ref.py:f32_form_f64 restates it
            want = min(256 if option < 256 else option // 16 * 16, n_loc)
        else:
            want = 1
        assert p['chunk'] == want, (option, n_loc, p)


def test_apply_plan_is_the_restatement(plans):
    seen = set()
    for (form, n, m, ld, plain, rows_per, rw), p in plans['apply']:
        key = (form, n, m, ld, plain, rows_per, rw)
        want = nr.apply_plan(n, m, form, rows_per, rw)
        parts = [min(n, (k + 1) * p['rows_per']) - k * p['rows_per'] for k in range(p['nparts'])]
        got = dict(nparts=p['nparts'], parts=parts, col_blocks=p['col_blocks'])
        if form == 3:
            got['rw'] = p['rw']
            assert p['row_blocks'] * 4 * p['rw'] - n == (-n) % (4 * p['rw']) == (4 * p['rw'] - want['rem_rows']) % (4 * p['rw']), (key, p)
        else:
            assert p['rw'] == 1 and p['rows_per'] == 2048 and p['row_blocks'] == (n + 3) // 4, (key, p)
        assert got == {k: want[k] for k in got}, (key, p, want)
        assert p['form'] == form and p['nt'] == (0 if plain else 1), (key, p)
        seen.add((form, p['nt'], p['rw']))
        # independent of the restatement
        cols = 1024 if form == 3 else 512
        assert p['nparts'] >= 1 and p['nparts'] * p['rows_per'] >= n and p['rows_per'] >= 64, (key, p)
        assert p['col_blocks'] * cols >= m > (p['col_blocks'] - 1) * cols, (key, p)
        assert p['o_t'] % 2 == 0 and p['nparts'] * m <= p['o_t'] <= p['nparts'] * m + 1, (key, p)  # part ends before t, read in pairs
        assert p['o_t'] + m <= p['o_u'], (key, p)  # t holds m entries
        assert (p['o_u'] + p['n_u']) * 8 <= p['ws_bytes'], (key, p)
        if form == 3:
            assert p['n_u'] == ld >= (m + 3) // 4 * 4 and p['o_u'] % 2 == 0, (key, p)  # u is zeroed over ld entries: the pad [m, m4) reads zero
            assert p['ws_bytes'] == (p['nparts'] * m + 2 * ld + 4) * 8 and p['launches'] == 5, (key, p)
            assert p['work'] == 8.0 * n * m + 8.0 * m * m, (key, p)
        else:
            assert p['n_u'] == 0 and p['ws_bytes'] == (p['nparts'] * m + m + 2) * 8 and p['launches'] == 3, (key, p)
            assert p['work'] == 16.0 * n * m, (key, p)
    assert seen == {(0, nt, 1) for nt in (0, 1)} | {(3, nt, rw) for nt in (0, 1) for rw in (1, 2, 4)}, seen

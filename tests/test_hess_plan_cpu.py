"""Plan of the analytic Hessian (csrc/hess_plan.h) without a GPU: tests/hess_plan_driver.cpp is compiled with the host compiler
(address and undefined-behaviour sanitizers where the toolchain has them; the program has its own main) and prints the plan,
every row chunk and every batch slice of each input.

The reference is not the header: tests/_hessian_ref.py:hess_plan restates what hess_device computed inline before the plan
existed.  The GPU grid (tests/test_hessian_grid_gpu.py) and tests/test_hessian_cpu.py::test_grid_reaches_every_variant_and_panel_edge
rest on that restatement; this test is what ties it to the compiled arithmetic, field by field.

Inputs: every call of the grid; every N = 2 ... 198 (198: refused) x every row case of the grid x predict.hess_generic 0 | 1;
and tables large enough for the memory cap to cut the chunk, N = 33, 128, 197 x M P = 600, 10^5 x B = 1, 64, 1000.

Independent of the restatement: the chunk is a multiple of the row group; chunks cover the rows and slices the batch; the
splits cover every chunk; no chunk has more groups than the first, whose count is G; the projection's LDS stays within
160 KiB; the workspace is the sum of its segments, laid end to end."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _hessian_ref as hr  # noqa: E402

SRC = os.path.join(ROOT, 'tests', 'hess_plan_driver.cpp')
PLAN_FIELDS = ('supported', 'variant', 'sel', 'v_lds', 'lds', 'D', 'n3', 'nb', 'ld', 'n_tp', 'Bs', 'RG', 'nr_cap', 'G', 'JS', 'nU', 'nCS',
               'nPF', 'nPE', 'nHp', 'nFX', 'nTau', 'ws', 'oW', 'oCS', 'oPF', 'oPE', 'oHp', 'oFX', 'oTau')


def _inputs():
    rows = list(hr.grid_plan_inputs())
    rows += [(N, MP, B, generic, chunk) for N in range(2, 199) for MP, B, chunk in hr.ROW_CASES for generic in (0, 1)]
    rows += [(N, MP, B, generic, 0) for N in (33, 128, 197) for MP in (600, 10**5) for B in (1, 64, 1000) for generic in (0, 1)]
    return rows


def _compiler():
    for name in ('g++', 'c++', 'clang++', '/opt/rocm/lib/llvm/bin/clang++', '/opt/rocm/llvm/bin/clang++'):
        path = shutil.which(name)
        if path:
            return path
    raise AssertionError('no host C++ compiler found')


@pytest.fixture(scope='module')
def drivers(tmp_path_factory):
    """The sanitized program (runtime linked statically where the compiler can) and the plain one."""
    d = tmp_path_factory.mktemp('hess_plan')
    base = [_compiler(), '-std=c++17', '-O1', '-g', '-Wall', SRC, '-o']
    plain = str(d / 'driver')
    subprocess.run(base + [plain], check=True)
    san_flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    for extra in (['-static-libasan', '-static-libubsan'], []):
        san = str(d / 'driver_san')
        if subprocess.run(base + [san] + san_flags + extra, capture_output=True, text=True).returncode == 0:
            return [san, plain]
    return [plain]  # toolchain without the sanitizer runtimes


def _parse(row, line):
    """One line of the driver as {field: value}, with 'chunks' [(nr, groups, grid_x, rps, accumulate)] and 'slices' [bs]."""
    head, tail = line.split(' : ')
    assert tuple(int(v) for v in head.split()) == row
    tok = tail.split()
    if tok == ['supported', '0']:
        return None
    n = 2 * len(PLAN_FIELDS)
    assert tuple(tok[0:n:2]) == PLAN_FIELDS, line
    p = {k: (v if k == 'variant' else int(v)) for k, v in zip(tok[0:n:2], tok[1:n:2])}
    assert tok[n] == 'chunks'
    at = tok.index('slices')
    p['chunks'] = [tuple(int(v) for v in c.split(',')) for c in tok[n + 1:at]]
    p['slices'] = [int(v) for v in tok[at + 1:]]
    return p


@pytest.fixture(scope='module')
def plans(drivers):
    """[(input tuple, parsed plan or None)] as every built program computes them (the programs agree)."""
    inputs = _inputs()
    text = ''.join(' '.join(str(v) for v in row) + '\n' for row in inputs)
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
    assert len(lines) == len(inputs)
    return [(row, _parse(row, line)) for row, line in zip(inputs, lines)]


def _as_restatement(row, p):
    """The driver's plan in the shape of hr.hess_plan; what that derives from chunks and groups is derived here from the
    driver's own chunk values."""
    N, MP, B, generic, _ = row
    wave = p['variant'] == 'wave'
    nr, groups, grid_x, rps, _ = (list(c) for c in zip(*p['chunks']))
    return dict(
        N=N, D=p['D'], n3=p['n3'], MP=MP, B=B, variant=(p['variant'], p['sel']), forced=bool(generic), v_lds=p['v_lds'],
        lds_bytes=p['lds'], nb=p['nb'], ld=p['ld'], n_tp=p['n_tp'], Bs=p['Bs'], slices=p['slices'], RG=p['RG'], nr_cap=p['nr_cap'],
        G=p['G'], JS=p['JS'], ws=[p['nU'], p['nU'], p['nCS'], p['nPF'], p['nPE'], p['nHp'], p['nFX'], p['nTau']], ws_bytes=p['ws'],
        chunks=nr, rps=rps, groups=groups, last_group_rows=[n - (g - 1) * p['RG'] for n, g in zip(nr, groups)],
        idle_waves=[4 * x - g if wave else x - g for x, g in zip(grid_x, groups)],
        empty_splits=[p['JS'] - (n + r - 1) // r for n, r in zip(nr, rps)], rps_mod16=[r % hr.HK for r in rps])


def test_plan_is_the_restatement(plans):
    bad = []
    for row, p in plans:
        want = hr.hess_plan(*row)
        got = None if p is None else _as_restatement(row, p)
        if got != want:
            bad.append((row, got, want))
    for row, got, want in bad[:5]:
        print('N MP B generic chunk_rows =', row)
        for k in sorted(set(got or {}) | set(want or {})):
            if (got or {}).get(k) != (want or {}).get(k):
                print('  %s: header %s restatement %s' % (k, (got or {}).get(k), (want or {}).get(k)))
    assert not bad, '%d of %d plans differ' % (len(bad), len(plans))
    refused = {row[0] for row, p in plans if p is None}
    assert refused == {hr.N_UNSUPPORTED}


def test_plan_invariants(plans):
    seen = set()
    for row, p in plans:
        if p is None:
            continue
        N, MP, B = row[:3]
        seen.add((p['variant'], p['sel']))
        assert p['nr_cap'] % p['RG'] == 0, (row, p)
        assert sum(c[0] for c in p['chunks']) == MP and all(c[0] >= 1 for c in p['chunks']), (row, p)
        assert sum(p['slices']) == B and all(1 <= s <= p['Bs'] for s in p['slices']), (row, p)
        for i, (nr, groups, grid_x, rps, accumulate) in enumerate(p['chunks']):
            assert p['JS'] * rps >= nr, (row, p)
            assert groups <= p['chunks'][0][1], (row, p)
            assert groups * p['RG'] >= nr > (groups - 1) * p['RG'], (row, p)
            assert grid_x == ((groups + 3) // 4 if p['variant'] == 'wave' else groups), (row, p)
            assert accumulate == int(i > 0), (row, p)
        assert p['G'] == p['chunks'][0][1], (row, p)
        assert p['lds'] <= 160 * 1024, (row, p)
        lengths = [p['nU'], p['nU'], p['nCS'], p['nPF'], p['nPE'], p['nHp'], p['nFX'], p['nTau']]
        assert p['ws'] == 8 * sum(lengths), (row, p)
        offsets = [0, p['oW'], p['oCS'], p['oPF'], p['oPE'], p['oHp'], p['oFX'], p['oTau']]
        assert offsets == [sum(lengths[:i]) for i in range(8)], (row, p)
    # the memory cap alone cuts the chunk in some of the large tables
    assert any(p is not None and row[4] == 0 and len(p['chunks']) > 1 for row, p in plans)
    assert seen == {('wave', k) for k in (1, 2, 4, 8)} | {('block', k) for k in (0, 4, 8, 16, 32, 48)}, seen

"""Plan of the batched predictor (csrc/predict_plan.h) without a GPU: tests/predict_plan_driver.cpp is compiled with the host
compiler (address and undefined-behaviour sanitizers where the toolchain has them; the program has its own main) and prints
the plan of every input of a grid.

The reference is not the header: `_parent_plan` restates, statement by statement and in its order, what predict_device_w
computed inline before the plan existed -- sgdml_amd/csrc/predict.hip at commit 136c553, lines 947-1039 (routes, QB, n_qt,
JS, max_js, the cost search, rows per split, workspace, the MFMA kernel's tile count and LDS) and 960-977 (the wide route's
workspace and its four epilogues), with the launches of lines 1054-1085 and 920-935 for grids, block sizes and the epilogue.

Grid: N = 2, 3, 9, 12, 21, 23, 24, 45, 46, 91, 92, 128, 129 (D = 1 ... 253 | 276 ... 990 | 1035 ... 4095 | 4186, 8128 | 8256:
both sides of D = 256, 1024, 4096, 8192 and of every KPL step) x B = 1 ... 100000 (both sides of QB steps and of 256) x
M P = 1 ... 27000 (both sides of 16 and 64), plus N = 24, B = 256 at M P = 14153 | 14154 (M P B D = 999 994 368 | 1 000 065 024);
defaults and each option on its own; with and without the virial; 256 and 304 compute units.

Independent of the restatement: every route is met; the splits cover the rows and none is empty; the workspace holds
JS B (D + 1) doubles; the MFMA kernel's LDS stays within 160 KB; WAVE never serves D > 1024."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'predict_plan_driver.cpp')

NS = (2, 3, 9, 12, 21, 23, 24, 45, 46, 91, 92, 128, 129)
BS = (1, 2, 3, 7, 8, 9, 255, 256, 257, 1000, 4096, 100000)
MPS = (1, 15, 16, 17, 63, 64, 65, 1000, 6000, 27000)
DEFAULTS = dict(wave_only=0, mfma=1, mfma_wide=1, fill=1024)
OPTIONS = ({}, {'wave_only': 1}, {'mfma': 0}, {'mfma_wide': 0}, {'mfma_wide': 2}, {'fill': 1})
FIELDS = ('route', 'sel', 'QB', 'grid_x', 'grid_y', 'block', 'JS', 'rps', 'lds', 'ws', 'stats', 'epi_lds_row', 'epi_virial', 'epi_JS',
          'epi_lds')


def _parent_plan(N, MP, B, ncu, virial, wave_only, mfma, mfma_wide, fill):
    """predict_device_w of 136c553 (see the module docstring); integer division is C's on non-negative values."""
    MQ, MR, PQ, PR = 64, 16, 32, 32  # the tile constants of predict_plan.h
    D = N * (N - 1) // 2
    KPL = 1
    while KPL * 64 < D:
        KPL <<= 1
    big = D > 1024
    wide_opt = mfma_wide
    beyond = D > 8192
    wide = beyond or (B >= 256 and D > 256 and not wave_only and
                      (wide_opt == 2 or (wide_opt == 1 and float(MP) * float(B) * float(D) >= 1.0e9)))
    if wide:  # lines 960-977: one partial, epilogue <false> (in place, no LDS) beyond, else <true> with D * 8 bytes
        return dict(route='WIDE', sel=0, QB=0, grid_x=0, grid_y=0, block=0, JS=1, rps=MP, lds=0, ws=(B * D + B) * 8, stats=0,
                    epi_lds_row=int(not beyond), epi_virial=int(virial), epi_JS=1, epi_lds=0 if beyond else D * 8)
    bulk = (not big) and B >= 256 and D <= 256 and not wave_only
    is_mfma = bulk and bool(mfma)
    QB = 8 if KPL <= 4 else (4 if KPL == 8 else (2 if KPL == 16 else 1))
    while QB > 1 and B < QB:
        QB >>= 1
    js_cap = MP // 16 if MP // 16 > 1 else 1
    while QB > 1 and ((B + QB - 1) // QB) * js_cap < fill:
        QB >>= 1
    n_qt = (B + MQ - 1) // MQ if is_mfma else (B + PQ - 1) // PQ if bulk else (B + QB - 1) // QB
    JS = ((512 if is_mfma else 2048 if bulk else 4096) + n_qt - 1) // n_qt
    max_js = (MP // 64 if MP // 64 > 1 else 1) if bulk else (MP // 16 if MP // 16 > 1 else 1)
    if big:
        n_qt = B
        JS = (1024 + B - 1) // B
        max_js = MP // 4 if MP // 4 > 1 else 1
    if JS > max_js:
        JS = max_js
    if JS < 1:
        JS = 1
    if is_mfma:
        best, best_cost = 1, None
        js = 1
        while js <= 64 and js <= max_js:
            rows = (((MP + js - 1) // js) + MR - 1) // MR * MR
            js_eff = (MP + rows - 1) // rows
            rounds = (n_qt * js_eff + ncu - 1) // ncu
            cost = rounds * (rows // MR + 3)
            if best_cost is None or cost < best_cost:
                best_cost, best = cost, js
            js += 1
        JS = best
    rps = (MP + JS - 1) // JS
    if bulk:
        rps = (rps + PR - 1) // PR * PR
    JS = (MP + rps - 1) // rps
    out = dict(JS=JS, rps=rps, ws=(JS * B * D + JS * B) * 8, QB=0, lds=0, stats=0, epi_lds_row=1, epi_virial=int(virial), epi_JS=JS,
               epi_lds=D * 8)
    if is_mfma:
        nt = 2 * ((D + 31) // 32)
        out.update(route='MFMA', sel=nt, grid_x=n_qt, grid_y=JS, block=256, lds=4 * MR * (16 * nt + 2) * 8, stats=2 * MP * 8)
    elif bulk:
        out.update(route='BULK', sel=min((D + 31) // 32, 8), grid_x=n_qt, grid_y=JS, block=256)
    elif big:
        out.update(route='BIG', sel=8 if D <= 4096 else 16, grid_x=B, grid_y=JS, block=512)
    else:  # dispatch_qb / launch_pred: QB is a power of two within the kernel's limit already; four wavefronts per workgroup
        out.update(route='WAVE', sel=min(KPL, 32), QB=QB, grid_x=(((B + QB - 1) // QB) * JS + 3) // 4, grid_y=1, block=256)
    return out


def _inputs():
    shapes = list(itertools.product(NS, MPS, BS)) + [(24, 14153, 256), (24, 14154, 256)]
    for (N, MP, B), opts, virial, ncu in itertools.product(shapes, OPTIONS, (0, 1), (256, 304)):
        o = dict(DEFAULTS, **opts)
        yield (N, MP, B, ncu, virial, o['wave_only'], o['mfma'], o['mfma_wide'], o['fill'])


def _compiler():
    for name in ('g++', 'c++', 'clang++', '/opt/rocm/lib/llvm/bin/clang++', '/opt/rocm/llvm/bin/clang++'):
        path = shutil.which(name)
        if path:
            return path
    raise AssertionError('no host C++ compiler found')


@pytest.fixture(scope='module')
def drivers(tmp_path_factory):
    """The sanitized program (runtime linked statically where the compiler can) and the plain one."""
    d = tmp_path_factory.mktemp('predict_plan')
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
    """[(input tuple, {field: value})] as the header computes them."""
    inputs = list(_inputs())
    text = ''.join(' '.join(str(v) for v in row) + '\n' for row in inputs)
    for exe in drivers:
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        print(r.stderr[-4000:])
        if r.returncode != 0 and 'does not come first' in r.stderr:
            continue  # a preloaded library keeps the sanitizer's runtime from starting: the plain program computes the same
        break
    assert r.returncode == 0
    lines = r.stdout.splitlines()
    assert len(lines) == len(inputs)
    out = []
    for row, line in zip(inputs, lines):
        head, tail = line.split(' : ')
        assert tuple(int(v) for v in head.split()) == row
        tok = tail.split()
        got = dict(zip(tok[0::2], tok[1::2]))
        assert tuple(got) == FIELDS, line
        out.append((row, {k: (v if k == 'route' else int(v)) for k, v in got.items()}))
    return out


def test_plan_is_the_parents_arithmetic(plans):
    bad = [(row, got, _parent_plan(*row)) for row, got in plans if got != _parent_plan(*row)]
    for row, got, want in bad[:10]:
        print('N MP B ncu virial wave_only mfma mfma_wide fill =', row, '\n  header', got, '\n  parent', want)
    assert not bad, '%d of %d plans differ' % (len(bad), len(plans))


def test_plan_invariants(plans):
    routes = {}
    for row, p in plans:
        N, MP, B = row[:3]
        D = N * (N - 1) // 2
        routes[p['route']] = routes.get(p['route'], 0) + 1
        assert p['JS'] * p['rps'] >= MP, (row, p)
        assert (p['JS'] - 1) * p['rps'] < MP, (row, p)  # no empty split
        assert p['ws'] >= p['JS'] * B * (D + 1) * 8, (row, p)
        assert p['epi_JS'] == p['JS'], (row, p)
        if p['route'] == 'MFMA':
            assert p['lds'] <= 160 * 1024, (row, p)
        if p['route'] == 'WAVE':
            assert D <= 1024, (row, p)
    print(routes)
    assert set(routes) == {'WAVE', 'BIG', 'BULK', 'MFMA', 'WIDE'}, routes
    # the 1e9 work threshold: M P = 14153 stays on the wave kernel, 14154 goes to the pipeline (defaults)
    by_row = {row: p['route'] for row, p in plans}
    assert by_row[(24, 14153, 256, 256, 0, 0, 1, 1, 1024)] == 'WAVE'
    assert by_row[(24, 14154, 256, 256, 0, 0, 1, 1, 1024)] == 'WIDE'

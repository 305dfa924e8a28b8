"""Plan of the batched Jacobi eigensolver, slice length and slice workspace of the spectrum (csrc/sym_eig_plan.h) without a GPU:
tests/sym_eig_plan_driver.cpp is compiled with the host compiler (address and undefined-behaviour sanitizers where the toolchain
has them; the program has its own main) and prints every field of sym_eig_plan, spectrum_slice_len and spectrum_ws for each
request.  The reference is the NumPy restatement in tests/_vib_ref.py, compared field by field.

Inputs.  The plan: every N in 1 ... 591 (the Hessian's limit of 197 atoms) x num_cus 1, 64, 256 x both values of cap_global x
M in 1, grid - 1, grid, grid + 1 of the case (grid: what the case launches for a batch without end).  The slice length: n3 in
3, 63, 300, 303, 423, 426, 591 (both sides of the two storage boundaries n3 = 300 | 303 and 423 | 426 among them) x B in 1, 63,
64, 65, 10^6 x option in 0, 1, 3, 10^9.  The workspace: with and without R.

Independent of the restatement: lds <= 160 KiB; V in LDS only with A; V in LDS exactly for N <= 100 and A exactly for N <= 141
(by the formula, checked by hand: N = 100 needs 162 864 B, N = 101 164 512 B with both matrices and 82 904 B with A alone,
N = 141 160 824 B and N = 142 164 224 B with A alone; the limit is 163 840 B); no work matrices exactly when V is in LDS;
1 <= grid <= M.  The slice length lies in 1 ... B, is min(option, B) for a positive option and otherwise a multiple of 64
whenever it exceeds 64 and is below B.  The workspace's fields ascend, do not overlap and add up to the total."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _vib_ref as vr  # noqa: E402

SRC = os.path.join(ROOT, 'tests', 'sym_eig_plan_driver.cpp')
MAX_N = 591
NUM_CUS = (1, 64, 256)
SLICE_N3 = (3, 63, 300, 303, 423, 426, 591)
SLICE_B = (1, 63, 64, 65, 10**6)
SLICE_OPTION = (0, 1, 3, 10**9)
WS_WORK = (0, 2 * 300 * 301, 256 * 2 * 591 * 591)


def _plan_inputs():
    """(num_cus, M, N, cap_global)"""
    rows = []
    for N in range(1, MAX_N + 1):
        for cus in NUM_CUS:
            for cap in (0, 1):
                grid = vr.sym_eig_plan(cus, 2**40, N, cap)['grid']
                rows += [(cus, M, N, cap) for M in sorted({1, grid - 1, grid, grid + 1}) if M >= 1]
    return rows


def _requests():
    reqs = [('plan',) + r for r in _plan_inputs()]
    reqs += [('slice', cus, B, n3, opt) for cus in NUM_CUS for B in SLICE_B for n3 in SLICE_N3 for opt in SLICE_OPTION]
    reqs += [('ws', ln, N, work, with_R) for ln in (1, 3, 64, 4096) for N in (1, 21, 100, 197) for work in WS_WORK for with_R in (0, 1)]
    return reqs


def _compiler():
    for name in ('g++', 'c++', 'clang++', '/opt/rocm/lib/llvm/bin/clang++', '/opt/rocm/llvm/bin/clang++'):
        path = shutil.which(name)
        if path:
            return path
    raise AssertionError('no host C++ compiler found')


@pytest.fixture(scope='module')
def drivers(tmp_path_factory):
    """The sanitized program (runtime linked statically where the compiler can) and the plain one."""
    d = tmp_path_factory.mktemp('sym_eig_plan')
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
        out.setdefault(req[0], []).append((req[1:], {k: int(v) for k, v in zip(tok[0::2], tok[1::2])}))
    return out


def test_sym_eig_plan_is_the_restatement(plans):
    assert len(plans['plan']) > 2 * 3 * 3 * MAX_N
    for (cus, M, N, cap), p in plans['plan']:
        key = (cus, M, N, cap)
        assert p == vr.sym_eig_plan(cus, M, N, cap), key
        # independent of the restatement
        assert p['lds'] <= 160 * 1024, key
        assert p['a_in_lds'] or not p['v_in_lds'], key
        assert p['v_in_lds'] == (N <= 100) and p['a_in_lds'] == (N <= 141), key
        assert (p['work_doubles'] == 0) == bool(p['v_in_lds']), key
        assert 1 <= p['grid'] <= M, key
        assert p['NP'] % 2 == 1 and N <= p['NP'] <= N + 1, key
        if not p['v_in_lds']:
            assert p['work_doubles'] == p['grid'] * 2 * N * p['NP'], key
        if cap and not p['a_in_lds']:
            assert p['grid'] <= cus, key
    by = {k: p for k, p in plans['plan']}
    # the two storage boundaries, by hand
    assert by[(64, 1, 100, 1)]['lds'] == 162864
    assert by[(64, 1, 101, 1)]['lds'] == 82904 and 82904 + 101 * 101 * 8 == 164512 > 160 * 1024
    assert by[(64, 1, 141, 1)]['lds'] == 160824
    assert by[(64, 1, 142, 1)]['lds'] == 164224 - 142 * 143 * 8 and 164224 > 160 * 1024
    # cap_global is the one difference between the callers: the device-memory route, and only there
    for cus in NUM_CUS:
        for N in (100, 141, 142, 591):
            full, search = (vr.sym_eig_plan(cus, 2**40, N, c)['grid'] for c in (1, 0))
            assert by[(cus, full + 1, N, 1)]['grid'] == full and by[(cus, search + 1, N, 0)]['grid'] == search
            assert (full, search) == ((cus, 4 * cus) if N > 141 else (search, search)), (cus, N)


def test_spectrum_slice_len(plans):
    assert len(plans['slice']) == len(NUM_CUS) * len(SLICE_B) * len(SLICE_N3) * len(SLICE_OPTION)
    for (cus, B, n3, opt), p in plans['slice']:
        key = (cus, B, n3, opt)
        got = p['len']
        assert got == vr.spectrum_slice_len(cus, B, n3, opt), key
        assert 1 <= got <= B, key
        if opt > 0:
            assert got == min(opt, B), key
        elif 64 < got < B:
            assert got % 64 == 0, key


def test_spectrum_ws_both_forms(plans):
    seen = set()
    for (ln, N, work, with_R), s in plans['ws']:
        key = (ln, N, work, with_R)
        n3 = 3 * N
        # the fields' lengths, stated here once more: offsets ascending and disjoint, the total their sum
        lengths = [('work', work), ('H', ln * n3 * n3), ('R', ln * n3 if with_R else 0), ('F', ln * n3), ('w', ln * n3), ('info', 4 * ln),
                   ('E', ln), ('mass', N), ('sweeps', ln), ('n_rigid', ln), ('n_neg', ln)]
        at = 0
        for f, n in lengths:
            assert s[f] == at, (key, f)
            at += n
        assert s['total'] == at == sum(n for _, n in lengths), key
        assert s['with_R'] == with_R and (with_R or s['R'] == s['F']), key
        assert s['per_geometry'] * ln == s['total'] - work - N and s['per_geometry'] == n3 * n3 + (3 if with_R else 2) * n3 + 8, key
        ref, total = vr.spectrum_ws(ln, N, work, with_R)
        assert total == s['total'] and all(s[f] == o for f, o, _ in ref), key
        assert [f for f, _ in lengths] == list(vr.SPECTRUM_FIELDS)
        seen.add(with_R)
    assert seen == {0, 1}

"""Tile schedule of the lower trailing updates (csrc/tile_sched.h) without a GPU: tests/tile_balance_driver.cpp is compiled
with the host compiler (address and undefined-behaviour sanitizers where the toolchain has them; the program has its own
main) and runs the kernels' decode for every block index of every launch of
  - tile lists of 1 .. 40, 320 and 481 tile rows (every tiles_m % 8, fewer than 8 super rows), with and without the
    first-column-first form, in one and two launches, with and without a second problem, with and without a carried row;
  - every lower launch of the plan (chol_plan_build, chol.deep = 0) of the benchmark's factorisation (n = 63 000, 63 001
    rows) and of n = 2500, 2501 rows, at the default options and at chol.nb = 128 with the thresholds of
    tests/test_tile_balance_gpu.py, through the launcher's own host functions (plan_lower_sched, plan_lower_range);
  - the integer range of the super-tile list of a launch against the floating-point share it replaced.
Per list it asserts: every lower tile exactly once and none above the diagonal; first-column tiles in the first launch and
ahead of the rest on their XCD; exactly the diagonal block's tiles counted; per-XCD work within 8 tiles of the launch's mean
(second problem at K2 / K); fewer than 8 empty blocks; the flop counts; and that the super-tile enumeration (gemm.balance = 0)
is the old one, restated with explicit loops."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'tile_balance_driver.cpp')


def _compiler():
    for name in ('g++', 'c++', 'clang++', '/opt/rocm/lib/llvm/bin/clang++', '/opt/rocm/llvm/bin/clang++'):
        path = shutil.which(name)
        if path:
            return path
    raise AssertionError('no host C++ compiler found')


@pytest.fixture(scope='module')
def drivers(tmp_path_factory):
    """The sanitized program (runtime linked statically where the compiler can) and the plain one."""
    d = tmp_path_factory.mktemp('tile_balance')
    base = [_compiler(), '-std=c++17', '-O1', '-g', '-Wall', SRC, '-o']
    plain = str(d / 'driver')
    subprocess.run(base + [plain], check=True)
    san_flags = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined']
    for extra in (['-static-libasan', '-static-libubsan'], []):
        san = str(d / 'driver_san')
        if subprocess.run(base + [san] + san_flags + extra, capture_output=True, text=True).returncode == 0:
            return [san, plain]
    return [plain]  # toolchain without the sanitizer runtimes


def test_every_block_of_every_launch(drivers):
    for exe in drivers:
        r = subprocess.run([exe], capture_output=True, text=True)
        print(r.stdout[-4000:])
        print(r.stderr[-4000:])
        if r.returncode != 0 and 'does not come first' in r.stderr:
            continue  # a preloaded library keeps the sanitizer's runtime from starting: the plain program checks the same
        break
    assert r.returncode == 0
    assert ' 0 failures' in r.stdout
    # the benchmark's factorisation: 45 outer steps of two fused launches, 8 single fused launches, 24 tail launches
    assert 'factorisation n 63000 rows 63001: 45 pairs, 8 single fused, 24 plain lower launches' in r.stdout

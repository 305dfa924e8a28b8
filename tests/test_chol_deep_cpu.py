"""The factorisation's launch plan (chol_plan_build in sgdml_amd/csrc/tile_sched.h, run by chol_factor_device) without a GPU.
tests/chol_plan_driver.cpp prints the plan as events; this module replays them at tile granularity and asserts, over a sweep
of n (multiples of 128 and not), n_rows = n and n + 1, chol.nb = 128 / 256 / 512 and chol.deep = 2 / 3 / 4 outer panels, with
a deep regime that ends after a whole block, inside a block, when the panel pairs run out, and that is never entered:
  1. every lower tile receives every panel left of its column's panel exactly once,
  2. in ascending k order without a gap (a tile's covered depth only ever grows from where it stands),
  3. a panel is read as an operand only after its rows below were solved earlier in stream order, and a diagonal block is
     factored / its rows solved only when every update of their tiles was issued earlier, or, for the block that workgroup 0
     of a launch factors, inside that launch by exactly the tiles that count themselves,
  4. no tile appears twice in one launch, none lies above the diagonal, none outside its segment,
  5. the operations are those of the one-level schedule with each paired launch replaced one for one; with chol.deep = 0 the
     plan is the parent schedule's launch list, restated here with explicit loops."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'chol_plan_driver.cpp')
GT = 128


def _compiler():
    for name in ('g++', 'c++', 'clang++', '/opt/rocm/lib/llvm/bin/clang++', '/opt/rocm/llvm/bin/clang++'):
        path = shutil.which(name)
        if path:
            return path
    raise AssertionError('no host C++ compiler found')


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp('chol_plan') / 'driver')
    subprocess.run([_compiler(), '-std=c++17', '-O2', '-Wall', SRC, '-o', exe], check=True)
    return exe


def one_level_ops(n, n_rows, nb, outer, outer_min, fused_min):
    """The loop of chol_factor_device before the plan existed, as (kind, k0, nb, t0, nb2)."""
    NB = nb if (nb >= 64 and nb % 64 == 0 and nb <= 512) else 512
    min_rows = max(fused_min, 1)
    OB = outer if (outer == 2 * NB and NB % GT == 0) else NB

    def width_at(c0):
        left = n - (c0 + OB)
        w = OB if (OB > NB and left > 0 and left >= outer_min) else NB
        return min(n - c0, w)

    k0, w = 0, min(n, NB)
    ops = [('PANEL', 0, 0, 0, w)]
    while True:
        t0 = k0 + w
        if t0 >= n:
            break
        nb2 = width_at(t0)
        t1 = t0 + nb2
        fuse = nb2 % 64 == 0 and n - t1 >= min_rows and n_rows - t1 > 0
        if fuse and nb2 == 2 * NB:
            ops += [('PAIR1', k0, w, t0, nb2), ('TRSM', 0, 0, t0, NB), ('PAIR2', k0, w, t0, nb2), ('TRSM', 0, 0, t0 + NB, NB)]
        else:
            ops.append(('RECT', k0, w, t0, nb2))
            if fuse:
                ops += [('FUSED', k0, w, t0, nb2), ('TRSM', 0, 0, t0, nb2)]
            elif t1 < n:
                ops.append(('TAIL', k0, w, t0, nb2))
            else:
                ops.append(('PANEL', 0, 0, t0, nb2))
        k0, w = t0, nb2
    return ops


def replay(exe, n, n_rows, nb, outer, outer_min, fused_min, deep, deep_min):
    """Runs the driver, checks 1-4 and returns (ops, header, per-launch summaries)."""
    r = subprocess.run([exe] + [str(v) for v in (n, n_rows, nb, outer, outer_min, fused_min, deep, deep_min)], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split('\n')
    head = lines[0].split()
    assert head[0] == 'PLAN'
    hdr = {head[i]: int(head[i + 1]) for i in range(1, len(head), 2)}
    NB = hdr['NB']
    tm, tn = -(-n_rows // GT), -(-n // GT)
    cover = {}      # lower tile -> depth covered so far (panels [0, cover) received)
    units = []      # factored panels (c0, w) in order
    diag_done, solved = set(), set()
    ops, summaries = [], []

    def unit_final(kb, ke):
        k = kb
        for c0, w in units:
            if c0 == k and (c0, w) in solved:
                k = c0 + w
            if k >= ke:
                break
        return k == ke

    def update(ti, tj, kb, ke, launch_tiles):
        assert 0 <= tj <= ti < tm and tj < tn, ('tile above the diagonal or outside the matrix', ti, tj)
        assert (ti, tj) not in launch_tiles, ('tile twice in one launch', ti, tj)
        launch_tiles.add((ti, tj))
        assert ke <= tj * GT, ('panel not left of the tile', ti, tj, kb, ke)
        assert unit_final(kb, ke), ('operand read before it was solved', ti, tj, kb, ke)
        assert cover.get((ti, tj), 0) == kb, ('panels out of order, twice or with a gap', ti, tj, cover.get((ti, tj), 0), kb, ke)
        assert not units or tj * GT >= units[-1][0] + units[-1][1], ('update of a factored column', ti, tj)
        cover[(ti, tj)] = ke

    def col_tiles(c0, w):
        return range(c0 // GT, -(-min(c0 + w, n) // GT))

    def need(ti, tj, c0):
        assert cover.get((ti, tj), 0) == c0, ('tile used before its last update', ti, tj, cover.get((ti, tj), 0), c0)

    launch_tiles, counted = set(), set()
    for ln in lines[1:]:
        f = ln.split()
        if not f:
            continue
        if f[0] == 'OP':
            ops.append((f[1],) + tuple(int(v) for v in f[2:]))
            launch_tiles, counted = set(), set()
        elif f[0] == 'G':
            r0, c0, c1, lower, kb, ke = (int(v) for v in f[1:])
            assert r0 % GT == 0 and c0 % GT == 0
            for tj in range(c0 // GT, -(-min(c1, n) // GT)):
                for ti in range(max(r0 // GT, tj), tm):
                    update(ti, tj, kb, ke, launch_tiles)
        elif f[0] == 'U':
            seg, ti, tj, kb, ke, cnt = (int(v) for v in f[1:])
            update(ti, tj, kb, ke, launch_tiles)
            if cnt:
                counted.add((ti, tj))
        elif f[0] == 'D':
            c0, w = int(f[1]), int(f[2])
            assert c0 % GT == 0 and (not units or units[-1][0] + units[-1][1] == c0) and units[-1] in solved
            block = {(ti, tj) for tj in col_tiles(c0, w) for ti in col_tiles(c0, w) if tj <= ti}
            for ti, tj in block:
                need(ti, tj, c0)
            if ops[-1][0] == 'SEG':  # workgroup 0 waits for len(block) counts: exactly the block's tiles, all in this launch
                assert counted == block and block <= launch_tiles, (sorted(counted), sorted(block))
            units.append((c0, w))
            diag_done.add(c0)
        elif f[0] == 'T':
            c0, w = int(f[1]), int(f[2])
            assert units[-1] == (c0, w) and c0 in diag_done and (c0, w) not in solved
            for tj in col_tiles(c0, w):
                for ti in range((c0 + w) // GT, tm):
                    need(ti, tj, c0)
            solved.add((c0, w))
        elif f[0] == 'P':
            c0, w = int(f[1]), int(f[2])
            assert (not units and c0 == 0) or (units[-1][0] + units[-1][1] == c0 and units[-1] in solved)
            for tj in col_tiles(c0, w):
                for ti in range(tj, tm):
                    need(ti, tj, c0 if tj * GT >= c0 else 0)
            units.append((c0, w))
            diag_done.add(c0)
            solved.add((c0, w))
        elif f[0] == 'S':
            summaries.append({f[i]: float(f[i + 1]) for i in range(1, len(f), 2)})
    assert units[-1][0] + units[-1][1] == n and all(u in solved or u == units[-1] for u in units)
    # 1: every lower tile ends with exactly the panels left of its own column's panel
    start = {}
    for c0, w in units:
        for tj in col_tiles(c0, w):
            start.setdefault(tj, c0)
    for tj in range(tn):
        for ti in range(tj, tm):
            assert cover.get((ti, tj), 0) == start[tj], (ti, tj, cover.get((ti, tj), 0), start[tj])
    return ops, hdr, summaries


def _sizes(nb, wp):
    W, OB = wp * 2 * nb, 2 * nb
    base = nb + 2 * W + 3 * OB
    return W, OB, [base + 128, base + 64, base + 133, base + 256 + 7]


@pytest.mark.parametrize('wp', [2, 3, 4])
@pytest.mark.parametrize('nb', [128, 256, 512])
def test_plan_sweep(driver, nb, wp):
    W, OB, sizes = _sizes(nb, wp)
    for n in sizes:
        for n_rows in (n, n + 1):
            want = one_level_ops(n, n_rows, nb, OB, 1, 1)
            # deep regime ended by the threshold after two whole blocks, inside the third block, by the pairs running out
            # (threshold 1), never entered (threshold above n), and switched off
            x_block, x_inside = nb + 2 * W, nb + 2 * W + OB
            for mode, deep, deep_min, x_want in (('block', W, n - x_block + 1, x_block), ('inside', W, n - x_inside + 1, x_inside),
                                                 ('pairs', W, 1, None), ('never', W, n + 1, 0), ('off', 0, 1, 0)):
                ops, hdr, summ = replay(driver, n, n_rows, nb, OB, 1, 1, deep, deep_min)
                if x_want is not None:
                    assert hdr['deep_end'] == x_want, (mode, n, hdr)
                else:
                    assert hdr['deep_end'] > x_inside
                # 5: the same operations, each paired launch of the deep regime replaced by one composed launch
                k = {'n': 0}

                def legacy(o):
                    if o[0] != 'SEG':
                        return o
                    k['n'] += 1
                    return (('PAIR1', 'PAIR2')[(k['n'] - 1) % 2],) + o[1:]
                assert [legacy(o) for o in ops] == want, (mode, n, n_rows)
                n_seg = sum(o[0] == 'SEG' for o in ops)
                if hdr['deep_end'] == 0:
                    assert ops == want and n_seg == 0
                else:
                    assert n_seg == 2 * ((hdr['deep_end'] - nb) // OB + 1)
                    assert all(o[3] > hdr['deep_end'] for o in ops if o[0] in ('PAIR1', 'PAIR2'))
                    assert sum(s['far'] for s in summ) > 0
                    if mode == 'inside' and n_rows - (nb + 3 * W) > 2 * GT:  # the last step carries the cut block's pass
                        assert summ[-1]['far'] + summ[-2]['far'] > 0


def test_default_options_at_the_benchmark_size(driver):
    """n = 63 000 with the carried row: chol.deep = 0 is the parent's list (45 pairs, 8 fused, 24 tail launches); chol.deep =
    4096 with the default threshold keeps every check, every launch of the regime carries far tiles after the first block,
    and the XCDs of a composed launch carry the same cost within four long tiles (the contiguous runs of single tiles round to whole
    tiles once per class of tiles, far and near)."""
    n = 63000
    ops, hdr, _ = replay(driver, n, n + 1, 512, 1024, 16384, 12288, 0, 26624)
    assert ops == one_level_ops(n, n + 1, 512, 1024, 16384, 12288) and hdr['deep_end'] == 0
    assert sum(o[0] == 'PAIR1' for o in ops) == 45 and sum(o[0] == 'FUSED' for o in ops) == 8 and sum(o[0] == 'TAIL' for o in ops) == 24
    ops, hdr, summ = replay(driver, n, n + 1, 512, 1024, 16384, 12288, 4096, 26624)
    assert hdr['deep'] == 4096 and n - hdr['deep_end'] < 26624 <= n - (hdr['deep_end'] - 1024)
    seg = [o for o in ops if o[0] == 'SEG']
    assert len(seg) == len(summ) == 2 * ((hdr['deep_end'] - 512) // 1024 + 1)
    first_block = 2 * 4  # launches of the steps t0 = 512 ... 3584: nothing is pending yet
    assert all(s['far'] == 0 for s in summ[:first_block]) and all(s['far'] > 0 for s in summ[first_block:])
    for s in summ[first_block:]:
        assert s['xcd_cost_max'] - s['xcd_cost_min'] <= 4 * (4096 + 512 + 66), s


def test_table_size_at_large_n(driver):
    """The composed launches' tables are sized from the plan (no fixed block caps them): at n = 150 000 they need 4 x the
    8 MB that hold the balanced lists, the plan still runs the deep regime down to the threshold, and the longest XCD list and
    every tile index fit their fields (32 bits per count in the kernel argument, 14 bits per index: the driver exits non-zero
    on a tile outside its segment).  A matrix of 2^21 tile rows or more gets the one-level list."""
    argv = (150000, 150001, 512, 1024, 16384, 12288, 4096, 26624, 'summary')
    r = subprocess.run([driver] + [str(v) for v in argv], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    head = r.stdout.split('\n', 1)[0].split()
    hdr = {head[i]: int(head[i + 1]) for i in range(1, len(head), 2)}
    summ = [ln.split() for ln in r.stdout.split('\n') if ln.startswith('S ')]
    assert hdr['deep'] == 4096 and 150000 - hdr['deep_end'] < 26624 <= 150000 - (hdr['deep_end'] - 1024)
    assert hdr['table_bytes'] > 4 * (8 << 20) and hdr['longest_xcd_list'] < 2 ** 31
    assert hdr['table_bytes'] >= 4 * sum(int(f[2]) for f in summ) and len(summ) == 2 * ((hdr['deep_end'] - 512) // 1024 + 1)
    r = subprocess.run([driver] + [str(v) for v in (128 * 0x3ff0, 128 * 0x3ff0, 512, 1024, 16384, 12288, 4096, 26624, 'summary')],
                       capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith('PLAN NB 512 OB 1024 deep 0 deep_end 0 table_bytes 0 ')

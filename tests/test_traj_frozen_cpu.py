"""Host-only part of the run-until-frozen chunk loop (csrc/traj_host.h: traj_next_chunk, traj_take_chunk, traj_repeat_frozen)
without a GPU: tests/traj_frozen_driver.cpp is compiled with the host compiler (address and undefined-behaviour sanitizers
where the toolchain has them; the program has its own main), runs the loop against a simulated device and prints the schedule
and the arrays the caller would get.

The reference is not the header: `_parent_run` restates in NumPy what the entries did before the header existed --
sgdml_amd/csrc/traj.h at commit 41cc5f4, lines 243-263 (the chunk loop with its two histories: which evaluations a chunk
takes, their rows and frame slots, the rows copied on, the end of the run) and 271-287 (what a frozen replica repeats in the
two histories and in the frames), and sgdml_amd/csrc/vib.hip lines 856-863 for every further history (kept for the whole run on
the device, written at [t, b] by active replicas only, `src = e if e >= 0 and u > e else u` afterwards).  A second frame field
(gdml_cell_relax_run's lattices) follows lines 271-287 with its own length.  Compared: rows below n_made and their frames, which
is what the Python layer returns.

Grid: B = 1, 3 x max_steps = 0, 1, 3, 4, 7, 8, 33 x chunk_steps = 1, 4, 5, 32 x record_every = 0, 1, 2, 3 x frame bound = 1, 3,
unbounded x n_hist = 2, 3, 4 x freeze patterns: all active to the end | replica 0 frozen at evaluation 0 | replicas frozen at
the last row of the first chunk, the first row of the next and the row after | all frozen before the budget."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'traj_frozen_driver.cpp')

BS = (1, 3)
MAX_STEPS = (0, 1, 3, 4, 7, 8, 33)
CHUNK_STEPS = (1, 4, 5, 32)
RECORD_EVERY = (0, 1, 2, 3)
FRAME_BOUNDS = (1, 3, None)
N_HIST = (2, 3, 4)
FRAME_LEN = (3, 2)


def _parent_chunk(t, max_steps, chunk_steps, record, record_every, max_frames):
    """traj.h:244-251: [(t, row, frame)] of the chunk that starts at t."""
    t0, in_chunk, evs = t, 0, []
    while t <= max_steps and t - t0 < chunk_steps:
        on = record and t % record_every == 0
        if on and in_chunk == max_frames:
            break
        evs.append((t, t - t0, in_chunk if on else -1))
        if on:
            in_chunk += 1
        t += 1
    return evs


def _parent_run(B, max_steps, chunk_steps, record_every, max_frames, n_hist, e):
    """The parent's run and repeat (see the module docstring) on the driver's simulated device."""
    record = record_every > 0
    n_eval = max_steps + 1
    hist = np.full((n_hist, n_eval, B), -1, dtype=np.int64)
    rec = [np.full((max_steps // record_every + 1 if record else 0, B, n), -1, dtype=np.int64) for n in FRAME_LEN]
    end = [np.full((B, n), -1, dtype=np.int64) for n in FRAME_LEN]
    status = np.full((B, 2), -1, dtype=np.int64)
    chunk = np.full((2, chunk_steps, B), -1, dtype=np.int64)  # the device's two history buffers, never cleared
    chunks, t, done = [], 0, 0
    active = True
    while t <= max_steps and active:  # traj.h:243 (no bad flag is ever set here)
        evs = _parent_chunk(t, max_steps, chunk_steps, record, record_every, max_frames)
        chunks.append(evs)
        for te, row, frame in evs:
            for b in range(B):
                if status[b, 0] >= 0:
                    continue
                chunk[:, row, b] = [((h + 1) * 1000 + te) * 10 + b for h in range(2)]
                hist[2:, te, b] = [((h + 1) * 1000 + te) * 10 + b for h in range(2, n_hist)]  # whole-run arrays (vib.hip)
                for f, n in enumerate(FRAME_LEN):
                    end[f][b] = 500000 + (10 * te + b) * 10 + np.arange(n)
                    if frame >= 0:
                        rec[f][done + frame, b] = end[f][b]
                if te == e[b] or te == max_steps:
                    status[b] = (1 if te == e[b] else 0, te)
        t0, t = t, evs[-1][0] + 1
        done += sum(frame >= 0 for _, _, frame in evs)
        hist[:2, t0:t] = chunk[:, :t - t0]  # traj.h:256-257
        active = bool((status[:, 0] < 0).any())  # traj.h:258-262
    n_made = max(t if status[b, 1] < 0 else status[b, 1] + 1 for b in range(B))  # traj.h:273-277
    for b in range(B):  # traj.h:278-286
        eb = status[b, 1]
        if eb < 0:
            continue
        for u in range(eb + 1, n_made):
            hist[:2, u, b] = hist[:2, eb, b]
            if record and u % record_every == 0:
                for f in range(2):
                    rec[f][u // record_every, b] = end[f][b]
    for b in range(B):  # vib.hip:856-863
        eb = status[b, 1]
        for u in range(t):
            src = eb if (eb >= 0 and u > eb) else u
            hist[2:, u, b] = hist[2:, src, b]
    n_fr = (n_made + record_every - 1) // record_every if record else 0
    return dict(chunks=chunks, t=t, n_made=n_made, hist=hist[:, :n_made], rec=[r[:n_fr] for r in rec])


def _cases():
    for B, ms, cs, re, fb, nh in itertools.product(BS, MAX_STEPS, CHUNK_STEPS, RECORD_EVERY, FRAME_BOUNDS, N_HIST):
        mf = cs if fb is None else fb  # a chunk of cs evaluations never holds more than cs frames
        t1 = _parent_chunk(0, ms, cs, re > 0, re, mf)[-1][0] + 1  # the first chunk of a run is [0, t1)
        pats = [[-1] * B, [0] + [-1] * (B - 1)]
        pats += [[t1 - 1 + (b + s) % 3 for b in range(B)] for s in range(3 if B == 1 else 1)]
        if ms >= 1:
            pats.append([min(b, ms - 1) for b in range(B)])
        for e in pats:
            yield (B, ms, cs, re, mf, nh, [x if x <= ms else -1 for x in e])


def _compiler():
    for name in ('g++', 'c++', 'clang++', '/opt/rocm/lib/llvm/bin/clang++', '/opt/rocm/llvm/bin/clang++'):
        path = shutil.which(name)
        if path:
            return path
    raise AssertionError('no host C++ compiler found')


@pytest.fixture(scope='module')
def drivers(tmp_path_factory):
    """The sanitized program (runtime linked statically where the compiler can) and the plain one."""
    d = tmp_path_factory.mktemp('traj_frozen')
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
def runs(drivers):
    """[(case, what the driver printed for it, parsed)]."""
    cases = list(_cases())
    text = ''.join(' '.join(str(v) for v in c[:6] + tuple(c[6])) + '\n' for c in cases)
    for exe in drivers:
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        print(r.stderr[-4000:])
        if r.returncode != 0 and 'does not come first' in r.stderr:
            continue  # a preloaded library keeps the sanitizer's runtime from starting: the plain program computes the same
        break
    assert r.returncode == 0
    blocks = r.stdout.split('CASE\n')[1:]
    assert len(blocks) == len(cases)
    out = []
    for case, block in zip(cases, blocks):
        B, ms, cs, re, mf, nh, e = case
        got = dict(chunks=[], bounds=[], hist={}, rec={})
        for line in block.splitlines():
            tok = line.split()
            v = [int(x) for x in tok[1:]]
            if tok[0] == 'CHUNK':
                got['chunks'].append([])
                got['bounds'].append(tuple(v))
            elif tok[0] == 'EV':
                got['chunks'][-1].append(tuple(v))
            elif tok[0] == 'END':
                got['t'], got['n_made'] = v
            elif tok[0] == 'H':
                got['hist'][(v[0], v[1])] = v[2:]
            else:
                assert tok[0] == 'F', line
                got['rec'][(v[0], v[1])] = v[2:]
        out.append((case, got))
    return out


def test_schedule_invariants(runs):
    for case, got in runs:
        B, ms, cs, re, mf, nh, e = case
        evs = [ev for ch in got['chunks'] for ev in ch]
        # every evaluation up to the end of the run is scheduled exactly once and in order
        assert [t for t, _, _ in evs] == list(range(got['t'])), case
        assert got['t'] <= ms + 1, case
        # the run ends with the budget, or when every replica has frozen -- and then in the chunk of the last freeze
        frozen_at = [ms if x < 0 else x for x in e]
        last = max(frozen_at)
        assert got['chunks'][-1][0][0] <= last < got['t'], case
        assert got['n_made'] == last + 1, case
        for ch, (t0, t1, frames) in zip(got['chunks'], got['bounds']):
            assert 1 <= len(ch) <= cs and (t0, t1) == (ch[0][0], ch[-1][0] + 1), case
            assert [row for _, row, _ in ch] == list(range(len(ch))), case  # rows from 0, within the chunk buffer
            on = [(t, fr) for t, _, fr in ch if fr >= 0]
            # frames are the evaluations with t % record_every == 0, in slots 0, 1, ... within the frame bound
            assert [t for t, _ in on] == [t for t, _, _ in ch if re > 0 and t % re == 0], case
            assert [fr for _, fr in on] == list(range(len(on))) and len(on) == frames, case
            assert frames <= mf or re == 0, case


def test_loop_and_repeat_are_the_parents(runs):
    bad = []
    for case, got in runs:
        want = _parent_run(*case)
        B, nh = case[0], case[5]
        ok = got['chunks'] == want['chunks'] and got['t'] == want['t'] and got['n_made'] == want['n_made']
        ok = ok and len(got['hist']) == nh * want['n_made'] and len(got['rec']) == 2 * len(want['rec'][0])
        ok = ok and all(v == want['hist'][h, u].tolist() for (h, u), v in got['hist'].items())
        ok = ok and all(v == want['rec'][f][j].ravel().tolist() for (f, j), v in got['rec'].items())
        if not ok:
            bad.append((case, got, want))
    for case, got, want in bad[:5]:
        print('B max_steps chunk_steps record_every max_frames n_hist e =', case, '\n  header', got, '\n  parent', want)
    assert not bad, '%d of %d runs differ' % (len(bad), len(runs))


def test_nothing_unwritten_is_returned(runs):
    """Every row below n_made and every frame of them holds a stored or a repeated value (-1 marks what no store reached)."""
    for case, got in runs:
        assert all(x >= 0 for v in got['hist'].values() for x in v), case
        assert all(x >= 0 for v in got['rec'].values() for x in v), case

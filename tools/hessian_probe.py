"""Analytic Hessian probe: milliseconds per gdml_predict_hessian_dev call against the finite-difference route (one
gdml_predict_dev call over the 2 x 3N displaced geometries of every Hessian) on seeded synthetic models.

    python tools/hessian_probe.py [--shapes A,B,C] [--batches 1,16,64,256] [--min-s 0.5] [--out FILE.json]

Every point is warmed up, repeated for at least --min-s seconds of work and closed by a device synchronise.  The flop
counts are algorithmic: analytic 36 N^2 + 33 D per (Hessian, table row); finite differences 6N predictions of 10 D MP.
The finite-difference call carries at most 32768 geometries (its descriptor buffers): at large B it covers fewer
Hessians, and the comparison is per Hessian.
Kernel times for the fraction of the fp64 peak come from a separate rocprofv3 --kernel-trace --stats run of this script."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import synth_geometries  # noqa: E402
from oracle import gdml_oracle as orc  # noqa: E402
from sgdml_amd import _lib  # noqa: E402

SHAPES = {'A': (21, 1, 1000), 'B': (42, 27, 2000), 'C': (100, 1, 3000)}  # N, P, M (bench configs[1], [3], [4])
PEAK_FP64 = 78.6e12


def _timed(fn, sync, min_s):
    fn()
    sync()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        sync()
        dt = time.perf_counter() - t0
        if dt >= min_s:
            return dt / n * 1e3, n


def run_shape(key, batches, min_s, seed=0):
    N, P, M = SHAPES[key]
    D, n3 = N * (N - 1) // 2, 3 * N
    R, _, _ = synth_geometries(N, M + 8, seed=seed)
    R = R.reshape(M + 8, -1)
    rng = np.random.RandomState(seed)
    perms = np.array([np.arange(N)] + [rng.permutation(N) for _ in range(P - 1)])
    tp = orc.tril_perms_from_atom_perms(perms)
    ctx = _lib.Context(0)
    xd, _ = ctx.desc_from_R(R[:M], N)
    ctx.predict_upload_model(xd, rng.normal(size=xd.shape), tp, 20.0, None)
    lib, h = ctx._lib, ctx._h
    MP = M * P
    out = []
    for B in batches:
        Rq = np.ascontiguousarray(np.resize(R[M:], (B, n3)))
        bfd = min(B, max(1, 32768 // (2 * n3)))  # Hessians per finite-difference call (bounds its descriptor buffers)
        Rfd = np.ascontiguousarray((Rq[:bfd, None, None, :] + np.array([1e-4, -1e-4])[None, None, :, None]
                                    * np.eye(n3)[None, :, None, :]).reshape(-1, n3))  # (B, 3N, 2, 3N)
        nfd = Rfd.shape[0]
        ptr = {}
        for name, nbytes in (('R', B * n3 * 8), ('E', B * 8), ('F', B * n3 * 8), ('H', B * n3 * n3 * 8),
                             ('Rfd', nfd * n3 * 8), ('Efd', nfd * 8), ('Ffd', nfd * n3 * 8)):
            p = C.c_void_p()
            ctx._check(lib.gdml_dev_alloc(h, nbytes, C.byref(p)))
            ptr[name] = p
        try:
            ctx._check(lib.gdml_memcpy_h2d(h, ptr['R'], Rq.ctypes.data_as(C.c_void_p), Rq.nbytes))
            ctx._check(lib.gdml_memcpy_h2d(h, ptr['Rfd'], Rfd.ctypes.data_as(C.c_void_p), Rfd.nbytes))
            ms_an, reps_an = _timed(lambda: ctx.predict_hessian_dev(ptr['R'], B, ptr['E'], ptr['F'], ptr['H']), ctx.sync, min_s)
            ms_fd, reps_fd = _timed(lambda: ctx._check(lib.gdml_predict_dev(h, ptr['Rfd'], nfd, None, None, ptr['Efd'],
                                                                             ptr['Ffd'])), ctx.sync, min_s)
            ctx.profile(True)
            ctx.predict_hessian_dev(ptr['R'], B, ptr['E'], ptr['F'], ptr['H'])
            ctx.sync()
            kms, kn, kw = ctx.kernel_stat('hessian')
            ctx.profile(False)
        finally:
            for p in ptr.values():
                lib.gdml_dev_free(h, p)
        fl_an = B * MP * (36.0 * N * N + 33.0 * D)
        fl_fd = nfd * 10.0 * D * MP  # per call of bfd Hessians
        rec = {'shape': key, 'N': N, 'P': P, 'M': M, 'B': B, 'ms_analytic': ms_an, 'reps_analytic': reps_an,
               'fd_hessians_per_call': bfd, 'ms_fd': ms_fd, 'reps_fd': reps_fd,
               'speedup': (ms_fd / bfd) / (ms_an / B), 'flop_analytic': fl_an, 'flop_fd': fl_fd,
               'tflops_analytic': fl_an / ms_an * 1e-9, 'tflops_fd': fl_fd / ms_fd * 1e-9,
               'hessian_ktime_ms': kms / max(kn, 1), 'ms_per_hessian_analytic': ms_an / B,
               'ms_per_hessian_fd': ms_fd / bfd}
        print(json.dumps(rec), flush=True)
        out.append(rec)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='A,B,C')
    ap.add_argument('--batches', default='1,16,64,256')
    ap.add_argument('--min-s', type=float, default=0.5)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    _lib.preflight()
    recs = []
    for key in a.shapes.split(','):
        recs += run_shape(key, [int(b) for b in a.batches.split(',')], a.min_s)
    if a.out:
        with open(a.out, 'w') as f:
            json.dump({'peak_fp64_tflops': PEAK_FP64 * 1e-12, 'points': recs}, f, indent=1)


if __name__ == '__main__':
    main()

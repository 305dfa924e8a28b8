"""Vibrational-analysis probe: milliseconds per gdml_vib_run call (Hessians, projection and eigen-kernel on the device,
(B,3N) numbers back) against the route a user had before it -- gdml_predict_hessian, (B,3N,3N) doubles to the host, the same
projection in NumPy and numpy.linalg.eigh -- in one process, on a seeded synthetic model (N = 21, M = 1000, one permutation).

    python tools/vib_probe.py [--batches 1,64,1024] [--rounds 5] [--min-s 0.3] [--out profiles/vib_probe.json]

Every point is warmed up; a round repeats the call for at least --min-s seconds; the figure is the median of the rounds, with
the smallest and largest round beside it.  The split into Hessian, projection and eigen-kernel time comes from a further call
under gdml_profile (HIP events around the kernels).  A second table times gdml_sym_eig alone on random matrices of order 100,
101, 141 and 142 -- the last order of each LDS storage route and the first of the next."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import synth_geometries  # noqa: E402
from oracle import gdml_oracle as orc  # noqa: E402
from sgdml_amd import _lib  # noqa: E402

N, M_TRAIN = 21, 1000
EPS = np.finfo(np.float64).eps


def rounds_of(fn, rounds, min_s):
    fn()
    ms = []
    for _ in range(rounds):
        n, t0 = 0, time.perf_counter()
        while True:
            fn()
            n += 1
            dt = time.perf_counter() - t0
            if dt >= min_s:
                break
        ms.append(dt / n * 1e3)
    ms.sort()
    return dict(ms=ms[len(ms) // 2], ms_min=ms[0], ms_max=ms[-1])


def host_route(ctx, R, mass, h_scale):
    """predict_hessian + projection (tests/_vib_ref.py's, vectorised over the batch) + LAPACK eigh."""
    _, _, H = ctx.predict_hessian(R)
    B, n = H.shape[0], H.shape[1]
    sw = np.sqrt(np.repeat(mass, 3))
    D = h_scale * (0.5 * (H + H.transpose(0, 2, 1))) / (sw[None, :, None] * sw[None, None, :])
    r = R.reshape(B, -1, 3)
    cm = (mass[None, :, None] * r).sum(axis=1) / mass.sum()
    d = r - cm[:, None, :]
    cands = np.zeros((B, 6, n // 3, 3))
    for c in range(3):
        cands[:, c, :, c] = 1.0
        e = np.zeros(3)
        e[c] = 1.0
        cands[:, 3 + c] = np.cross(e[None, None, :], d)
    cands = cands.reshape(B, 6, n) * sw[None, None, :]
    Q = np.zeros((B, 6, n))
    keep = np.zeros((B, 6), dtype=bool)
    for a in range(6):
        v = cands[:, a].copy()
        orig2 = (v * v).sum(-1)
        for b in range(a):
            v -= (Q[:, b] * v).sum(-1)[:, None] * Q[:, b]
        rem2 = (v * v).sum(-1)
        keep[:, a] = (orig2 > 0.0) & (rem2 >= 1e-10 * orig2)
        Q[:, a] = np.where(keep[:, a, None], v / np.sqrt(np.where(rem2 > 0.0, rem2, 1.0))[:, None], 0.0)
    QQ = np.einsum('bai,baj->bij', Q, Q)
    P = np.eye(n)[None] - QQ
    PDP = P @ D @ P
    lam = 2.0 * np.sqrt((PDP ** 2).sum(axis=(1, 2)))
    w = np.linalg.eigvalsh(PDP + lam[:, None, None] * QQ)
    k = keep.sum(axis=1)
    for b in range(B):
        w[b, n - k[b]:] = 0.0
    return w


def run(batches, rounds, min_s, seed=0):
    n3 = 3 * N
    R, _, _ = synth_geometries(N, M_TRAIN + 8, seed=seed)
    R = R.reshape(M_TRAIN + 8, -1)
    rng = np.random.RandomState(seed)
    tp = orc.tril_perms_from_atom_perms(np.arange(N)[None])
    ctx = _lib.Context(0)
    xd, _ = ctx.desc_from_R(R[:M_TRAIN], N)
    ctx.predict_upload_model(xd, rng.normal(size=xd.shape), tp, 20.0, None)
    ctx.max_query_batch = max(ctx.max_query_batch, 1024 * n3)  # the yardstick's Hessians in one library call as well
    mass = np.array([1.0, 12.0, 16.0])[np.arange(N) % 3]
    points = []
    for B in batches:
        Rq = np.ascontiguousarray(np.resize(R[M_TRAIN:], (B, n3)) + 1e-3 * rng.standard_normal((B, n3)))
        w_dev = ctx.vib_run(Rq, mass)['w2']
        w_host = host_route(ctx, Rq, mass, 1.0)
        scale = np.abs(w_host).max()
        p = dict(B=B, N=N, M=M_TRAIN, max_w2_difference_rel=float(np.abs(w_dev - w_host).max() / scale))
        p['device'] = rounds_of(lambda: ctx.vib_run(Rq, mass), rounds, min_s)
        p['device_modes'] = rounds_of(lambda: ctx.vib_run(Rq, mass, modes=True), rounds, min_s)
        p['host'] = rounds_of(lambda: host_route(ctx, Rq, mass, 1.0), rounds, min_s)
        p['host_hessian_only'] = rounds_of(lambda: ctx.predict_hessian(Rq), rounds, min_s)
        p['speedup'] = p['host']['ms'] / p['device']['ms']
        p['speedup_modes'] = p['host']['ms'] / p['device_modes']['ms']
        ctx.profile(True)
        ctx.vib_run(Rq, mass)
        ctx.sync()
        for key, name in (('hessian', 'hessian'), ('projection', 'vib_project'), ('eigen', 'sym_eig_full')):
            ms, launches, _ = ctx.kernel_stat(name)
            p['kernel_ms_' + key] = ms
        ctx.profile(False)
        points.append(p)
        print(json.dumps(p))
    routes = []
    Mq = 64
    for n in (100, 101, 141, 142):
        A = rng.standard_normal((Mq, n, n))
        A = A + A.transpose(0, 2, 1)
        w, V, sweeps = ctx.sym_eig(A)
        q = dict(n=n, M=Mq, sweeps_max=int(sweeps.max()), route='LDS: matrix and rotations' if n <= 100 else
                 'LDS: matrix; rotations in device memory' if n <= 141 else 'device memory')
        q['device'] = rounds_of(lambda: ctx.sym_eig(A), rounds, min_s)
        q['lapack_eigh'] = rounds_of(lambda: np.linalg.eigh(A), rounds, min_s)
        routes.append(q)
        print(json.dumps(q))
    ctx.close()
    return dict(points=points, eig_routes=routes, rounds=rounds, min_s=min_s)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,64,1024')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--min-s', type=float, default=0.3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vib_probe.json'))
    a = ap.parse_args()
    res = run([int(b) for b in a.batches.split(',')], a.rounds, a.min_s)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)

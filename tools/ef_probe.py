"""Eigenvector-following probe: milliseconds per evaluation of gdml_ef_run (Hessians, projection, eigen-kernel and step on the
device, state resident) on a seeded synthetic model (N = 21, M = 1000, one permutation), next to two yardsticks in the same
process: one gdml_vib_run call with modes of the same batch (the work of an evaluation without the step kernel, plus its host
copies), and the route a user had before -- a NumPy loop of gdml_predict_hessian, the same projection, numpy.linalg.eigh and the
same step.

    python tools/ef_probe.py [--batches 1,8,64,1024] [--evals 4] [--rounds 5] [--out profiles/ef_probe.json]

Nothing converges (fmax = 1e-12).  Every point is warmed up by one call; the figure is the median of the rounds, with
spread = (max - min) / median beside it."""
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
FMAX = 1e-12
TRUST = dict(trust_min=1e-4, trust_max=0.05)
TRUST_START = 0.02


def rounds_of(fn, rounds, per):
    fn()
    ms = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) / per * 1e3)
    ms.sort()
    med = ms[len(ms) // 2]
    return dict(ms=med, ms_min=ms[0], ms_max=ms[-1], spread=(ms[-1] - ms[0]) / med)


def fresh(B):
    return dict(trust=np.full(B, TRUST_START), E_prev=np.zeros(B), dE_pred=np.zeros(B), flags=np.zeros(B, dtype=np.int64), t=None)


def host_loop(ctx, R0, n_eval, order=1):
    """n_eval evaluations of the search around gdml_predict_hessian: projection (rigid, unit masses, vectorised over the
    batch), LAPACK eigh, the step of the header.  Returns the end positions."""
    R = R0.copy()
    B, n = R.shape
    trust, E_prev, dE_pred = np.full(B, TRUST_START), np.zeros(B), np.zeros(B)
    have, clipped = np.zeros(B, dtype=bool), np.zeros(B, dtype=bool)
    for it in range(n_eval):
        E, F, H = ctx.predict_hessian(R)
        g = -F
        D = 0.5 * (H + H.transpose(0, 2, 1))
        r = R.reshape(B, -1, 3)
        d = r - r.mean(axis=1, keepdims=True)
        cands = np.zeros((B, 6, n // 3, 3))
        for c in range(3):
            cands[:, c, :, c] = 1.0
            e = np.zeros(3)
            e[c] = 1.0
            cands[:, 3 + c] = np.cross(e[None, None, :], d)
        cands = cands.reshape(B, 6, n)
        Q = np.zeros((B, 6, n))
        for a in range(6):
            v = cands[:, a].copy()
            for b in range(a):
                v -= (Q[:, b] * v).sum(-1)[:, None] * Q[:, b]
            Q[:, a] = v / np.sqrt((v * v).sum(-1))[:, None]
        QQ = np.einsum('bai,baj->bij', Q, Q)
        P = np.eye(n)[None] - QQ
        PDP = P @ D @ P
        lam = 2.0 * np.sqrt((PDP ** 2).sum(axis=(1, 2)))
        w, U = np.linalg.eigh(PDP + lam[:, None, None] * QQ)
        if it == n_eval - 1:
            break
        nv = n - 6
        w, U = w[:, :nv], U[:, :, :nv]
        ok = have & (np.abs(dE_pred) > 1e-8 * np.maximum(np.abs(E), np.abs(E_prev)))
        rho = np.where(ok, (E - E_prev) / np.where(ok, dE_pred, 1.0), 1.0)
        shrink = ok & ((rho < 0.25) | (rho > 1.75))
        grow = ok & (rho > 0.75) & (rho < 1.25) & clipped
        trust = np.where(shrink, np.maximum(trust / 2, TRUST['trust_min']), np.where(grow, np.minimum(2 * trust, TRUST['trust_max']), trust))
        gt = np.einsum('bji,bj->bi', U, g)
        dd = np.abs(w) + np.sqrt(w * w + 4.0 * gt * gt)
        s = -2.0 * gt / dd
        if order == 1:
            s[:, 0] = -s[:, 0]
        nrm = np.sqrt((s * s).sum(-1))
        clipped = nrm > trust
        s = np.where(clipped[:, None], s * (trust / nrm)[:, None], s)
        dE_pred = (gt * s + 0.5 * w * s * s).sum(-1)
        E_prev, have = E, np.ones(B, dtype=bool)
        R = R + np.einsum('bji,bi->bj', U, s)
    return R


def run(batches, n_eval, rounds, seed=0):
    n3 = 3 * N
    R, _, _ = synth_geometries(N, M_TRAIN + 8, seed=seed)
    R = R.reshape(M_TRAIN + 8, -1)
    rng = np.random.RandomState(seed)
    tp = orc.tril_perms_from_atom_perms(np.arange(N)[None])
    ctx = _lib.Context(0)
    xd, _ = ctx.desc_from_R(R[:M_TRAIN], N)
    ctx.predict_upload_model(xd, rng.normal(size=xd.shape), tp, 20.0, None)
    ctx.max_query_batch = max(ctx.max_query_batch, 1024 * n3)  # the yardstick's Hessians in one library call as well
    mass = np.ones(N)
    points = []
    for B in batches:
        Rq = np.ascontiguousarray(np.resize(R[M_TRAIN:], (B, n3)) + 1e-3 * rng.standard_normal((B, n3)))

        def device():
            return ctx.ef_run(Rq, FMAX, n_eval - 1, fresh(B), order=1, **TRUST)

        out = device()
        assert (out['status'][:, 0] == 0).all() and (out['first_bad_step'] < 0).all()
        R_host = host_loop(ctx, Rq, n_eval)
        p = dict(B=B, N=N, M=M_TRAIN, evaluations=n_eval,
                 max_R_end_difference=float(np.abs(out['R_end'] - R_host).max()))
        p['device_per_evaluation'] = rounds_of(device, rounds, n_eval)
        p['vib_run_modes_call'] = rounds_of(lambda: ctx.vib_run(Rq, mass, modes=True), rounds, 1)
        p['vib_run_call'] = rounds_of(lambda: ctx.vib_run(Rq, mass), rounds, 1)
        p['host_per_evaluation'] = rounds_of(lambda: host_loop(ctx, Rq, n_eval), rounds, n_eval)
        p['evaluation_over_vib_modes_call'] = p['device_per_evaluation']['ms'] / p['vib_run_modes_call']['ms']
        p['speedup_over_host'] = p['host_per_evaluation']['ms'] / p['device_per_evaluation']['ms']
        ctx.profile(True)
        device()
        ctx.sync()
        for key, name in (('hessian', 'hessian'), ('eigen', 'sym_eig_full')):
            ms, launches, _ = ctx.kernel_stat(name)
            p['kernel_ms_per_evaluation_' + key] = ms / n_eval
        ctx.profile(False)
        points.append(p)
        print(json.dumps(p), flush=True)
    ctx.close()
    return dict(points=points, rounds=rounds)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', default='1,8,64,1024')
    ap.add_argument('--evals', type=int, default=4)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ef_probe.json'))
    a = ap.parse_args()
    res = run([int(b) for b in a.batches.split(',')], a.evals, a.rounds)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)

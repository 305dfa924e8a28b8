"""GPU parity at BASELINE.json's configuration shapes against fixtures produced by the reference
(tests/golden/make_golden_r2.py), all through the C ABI: configs[0] (N=9, P=6, M=200: K samples, analytic
train, predictions, validation errors), configs[3] (N=42, P=27) and configs[4] (N=60) kernels, the reference's
PCG residual history, its LU branch, and the sharded iterative solver run by two processes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import gdml_oracle as orc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')


def load(name):
    return dict(np.load(os.path.join(GOLD, name + '.npz')))


@pytest.fixture
def ctx():
    from sgdml_amd import _lib

    c = _lib.Context()
    yield c
    c.close()


def make_task(g, **extra):
    M, N = g['R_train'].shape[:2]
    task = {
        'type': 't', 'code_version': '1.0.3', 'dataset_name': np.array('synth'), 'dataset_theory': np.array('pair'),
        'z': g['z'], 'R_train': g['R_train'], 'F_train': g['F_train'], 'E_train': g['E_train'],
        'idxs_train': np.arange(M), 'md5_train': 'x', 'idxs_valid': np.arange(0), 'md5_valid': 'x',
        'sig': int(g['sig']), 'lam': float(g['lam']), 'use_E': True, 'use_E_cstr': False,
        'use_sym': g['perms'].shape[0] > 1, 'perms': g['perms'],
    }
    task.update(extra)
    return task


@pytest.mark.parametrize('name', ['cfg0_n9_p6', 'cfg3_n42_p27', 'cfg4_n60_p1', 'cfg1_n21_m100', 'cfg3_n42_p27_m60', 'n100_m3', 'n150_p2_m3'])
def test_K_samples_at_config_shapes(ctx, name):
    """Device-assembled K (full, un-negated, host copy) vs the reference's sampled rows/columns, norm and max."""
    g = load(name)
    M, N = g['R_train'].shape[:2]
    xd, gd = ctx.desc_from_R(g['R_train'].reshape(M, -1), N)
    tp = orc.tril_perms_from_atom_perms(g['perms'])
    ctx.train_upload(xd, gd, tp)
    K = ctx.assemble_K(float(g['sig']), False, to_host=True)
    assert K.shape == (3 * N * M, 3 * N * M)
    scale = float(g['K_absmax'])
    assert np.abs(K[np.ix_(g['rows'], g['cols'])] - g['K_sample']).max() <= 1e-12 * scale
    assert abs(np.linalg.norm(K) - float(g['K_fro'])) <= 1e-11 * float(g['K_fro'])
    assert np.abs(K - K.T).max() <= 1e-13 * scale  # permutations form a group -> symmetric
    # K v through the matrix-free operator (the CG mat-vec) at this shape
    rs = np.random.RandomState(1)
    v = rs.normal(size=K.shape[0])
    ctx.predict_upload_model(xd, np.zeros_like(xd), tp, float(g['sig']), None)
    Kv = ctx.kernel_matvec(float(g['lam']), False, v)
    ref = K @ v - float(g['lam']) * v
    assert np.abs(Kv - ref).max() <= 1e-11 * np.abs(ref).max()


@pytest.mark.parametrize('name', ['cfg0_n9_p6', 'cfg3_n42_p27', 'cfg4_n60_p1', 'cfg1_n21_m100', 'cfg3_n42_p27_m60', 'n100_m3', 'n150_p2_m3'])
def test_dropin_train_predict_at_config_shapes(name):
    """GDMLTrain.train (analytic) + GDMLPredict on the fixture's task: residual of the solve with the
    reference's K-free check, model constants and predictions vs the reference's model (alphas themselves are
    conditioning-limited at lam = 1e-10 and are compared through what they predict)."""
    from sgdml_amd.predict import GDMLPredict
    from sgdml_amd.train import GDMLTrain

    g = load(name)
    M, N = g['R_train'].shape[:2]
    tr = GDMLTrain()
    try:
        model = tr.train(make_task(g))
        assert model['solver_name'] == 'analytic'
        ctx = tr._context()
        # residual of OUR coefficients with the matrix-free operator: ||(-K + lam) (-alpha) - y|| / ||y||
        tp = orc.tril_perms_from_atom_perms(g['perms'])
        ctx.predict_upload_model(model['R_desc'].T.copy(), np.zeros_like(model['R_desc'].T), tp, float(g['sig']), None)
        r = ctx.kernel_matvec(float(g['lam']), False, -model['alphas_F']) + g['y']  # y - A x, A x = -(K x - lam x)
        assert np.linalg.norm(r) <= 1e-10 * np.linalg.norm(g['y'])
    finally:
        tr.__del__()
    assert abs(model['std'] - float(g['model_std'])) <= 1e-12 * float(g['model_std'])
    pred = GDMLPredict(model)
    nt = len(g['R_test'])
    E, F = pred.predict(g['R_test'].reshape(nt, -1))
    assert np.abs(F - g['F_test']).max() <= 2e-4 * np.abs(g['F_test']).max()
    assert np.abs(E - g['E_test']).max() <= 2e-4 * np.abs(g['E_test']).max()
    assert abs(model['c'] - float(g['model_c'])) <= 2e-4 * max(1.0, abs(float(g['model_c'])))
    # the reference's own coefficients through our prediction kernels: tight
    model_ref = dict(model)
    from sgdml_amd.utils.desc import Desc

    d = Desc(N)
    xd, gd = orc.desc_from_R(g['R_train'].reshape(M, -1))
    model_ref['R_d_desc_alpha'] = d.d_desc_dot_vec(gd, g['alphas'].reshape(M, -1))
    model_ref['c'] = float(g['model_c'])
    pred2 = GDMLPredict(model_ref)
    E2, F2 = pred2.predict(g['R_test'].reshape(nt, -1))
    assert np.abs(F2 - g['F_test']).max() <= 1e-9 * np.abs(g['F_test']).max()
    assert np.abs(E2 - g['E_test']).max() <= 1e-9 * np.abs(g['E_test']).max()
    if 'valid_errors' in g:  # configs[0]: the validation loop of cli.py:1564-1605 on the device
        nv = len(g['R_valid'])
        errs = pred2.test_errors(g['R_valid'].reshape(nv, -1), g['F_valid_ref'].reshape(nv, -1), g['E_valid_ref'])
        got = np.array([errs['energy'][0], errs['energy'][1], errs['force'][0], errs['force'][1]])
        np.testing.assert_allclose(got, g['valid_errors'], rtol=1e-7)


def test_pcg_history_vs_reference(ctx):
    """gdml_pcg on the inducing columns the reference drew (N=9, M=400, k=21): same residual history as scipy's
    cg inside the reference's Iterative.solve -- first steps to rounding, whole history within the drift two
    correct PCG runs show on this system (the oracle drifts by <= 7 %), iteration count within 10 %."""
    g = load('pcg_n9_m400')
    M, N = g['R_train'].shape[:2]
    sig, lam, y = float(g['sig']), float(g['lam']), g['y']
    xd, gd = ctx.desc_from_R(g['R_train'].reshape(M, -1), N)
    tp = orc.tril_perms_from_atom_perms(g['perms'])
    idx = g['inducing_pts_idxs']
    ctx.train_upload(xd, gd, tp)
    ctx.assemble_K(sig, False, idx=idx, alloc_extra_rows=len(idx))
    ctx.nystroem_factor(lam, idx)
    ctx.predict_upload_model(xd, np.zeros_like(xd), tp, sig, None)
    hist = []
    x, info, iters, resid = ctx.pcg(lam, False, y, rtol=1e-4, maxiter=5000,
                                    callback=lambda it, r, fetch_x: hist.append(r) or False)
    ref = g['resid_hist']
    assert info == 0
    n_ref = int(g['n_iters'])
    assert abs(iters - n_ref) <= max(2, n_ref // 10), (iters, n_ref)
    # callback k reports ||r_k|| after update k, like scipy's callback (the reference's history)
    ours = np.array(hist)
    np.testing.assert_allclose(ours[:8], ref[:8], rtol=1e-6)
    k = min(len(ours), len(ref))
    np.testing.assert_allclose(ours[:k], ref[:k], rtol=0.15)
    # both solutions predict alike
    from sgdml_amd.utils.desc import Desc

    d = Desc(N)
    F = []
    for coeffs in (g['alphas'], -x):
        ctx.predict_upload_model(xd, d.d_desc_dot_vec(gd, coeffs.reshape(M, -1)), tp, sig, None)
        F.append(ctx.predict(g['R_test'].reshape(len(g['R_test']), -1))[1])
    assert np.abs(F[1] - F[0]).max() <= 5e-3 * np.abs(F[0]).max()


def test_rccl_collectives_execute_with_one_rank(ctx):
    """A real RCCL communicator of size one: ncclAllReduce / ncclAllGather are CALLED (comm_stats counts them)
    by the Nystroem factor, the preconditioner, the mat-vec and PCG, and nothing changes numerically."""
    from sgdml_amd import _lib

    g = load('n6_p1')
    lam, sig = float(g['lam']), float(g['sig'])
    tp = orc.tril_perms_from_lin(g['tril_perms_lin'], g['R_desc'].shape[1])
    idx = g['col_idxs']
    res = []
    for with_comm in (False, True):
        c = _lib.Context()
        try:
            if with_comm:
                c.comm_init(c.comm_unique_id(), 0, 1)
            c.train_upload(g['R_desc'], g['R_d_desc'], tp)
            c.assemble_K(sig, False, idx=idx, alloc_extra_rows=len(idx))
            lev, _, _ = c.nystroem_factor(lam, idx)
            n0 = c.comm_stats()[0]
            c.predict_upload_model(g['R_desc'], np.zeros_like(g['R_desc']), tp, sig, None)
            Kv = c.kernel_matvec(lam, False, g['v'])
            n1 = c.comm_stats()[0]
            Pv = c.precon_apply(lam, g['v'])
            n2 = c.comm_stats()[0]
            x, info, iters, _ = c.pcg(lam, False, g['y'], rtol=1e-6, maxiter=3000)
            n3, nbytes = c.comm_stats()
            assert info == 0
            if with_comm:
                assert n0 == 3  # two all-reduces of the m x m blocks + the all-gather of the leverage scores
                assert n1 - n0 == 1 and n2 - n1 == 2  # mat-vec: all-gather; preconditioner: all-reduce + all-gather
                # per iteration: preconditioner (2) + mat-vec (1); the pipelined loop has queued up to pcg.depth = 2 iterations beyond
                # the one that met the tolerance
                assert 3 * iters <= n3 - n2 <= 3 * (iters + 2) and nbytes > 0
            else:
                assert n3 == 0
            res.append((lev, Kv, Pv, x))
        finally:
            c.close()
    for a, b in zip(*res):
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-9 * np.abs(a).max())


def test_rccl_probe_child_process_one_rank():
    """sgdml_amd._rccl_probe (the child bench.py runs on every rank before it commits to RCCL): a size-one communicator,
    the toy sharded solve completes, its collectives are counted, and the answer equals the same solve without a
    communicator."""
    import json
    import subprocess
    import sys

    from sgdml_amd import _lib

    uid = _lib.Context.comm_unique_id()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, '-m', 'sgdml_amd._rccl_probe', '0', '0', '1', uid.hex()], cwd=root, timeout=300,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-500:]
    out = json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith('{')][-1])
    assert out['ok'] and out['collectives'] >= 3 + 3 * 5
    assert _lib.device_pci_bus_id(0) and ':' in _lib.device_pci_bus_id(0)


@pytest.mark.parametrize('world', [2, 3])
def test_sharded_iterative_processes_share_one_gpu(tmp_path, world):
    """The sharded iterative solver END TO END through GDMLTrain / Iterative / nystroem.hip, precon_apply.hip, cg.hip / comm.hip: `world`
    processes (torch.distributed.run, gloo) share GPU 0, each holds a row shard of the Nystroem factor and a
    query shard of the mat-vec, the collectives are host-staged.  Must reproduce the reference's PCG run on the
    same inducing columns (iteration count, residual) and make the same number of collectives per iteration."""
    g = load('pcg_n9_m400')
    out = str(tmp_path / 'shard.npz')
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', OMP_NUM_THREADS='2')
    port = 29000 + (os.getpid() % 500) + world
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(world),
           '--master-addr', '127.0.0.1', '--master-port', str(port),
           os.path.join(ROOT, 'tests', '_sharded_worker.py'), out, 'host']
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    r = dict(np.load(out))
    n_ref = int(g['n_iters'])
    assert np.array_equal(r['inducing'], g['inducing_pts_idxs'])
    assert abs(int(r['iters']) - n_ref) <= max(2, n_ref // 10), (int(r['iters']), n_ref)
    assert float(r['resid']) <= 1e-4 * float(r['norm_y'])
    # collectives: Nystroem factor 2 (its leverage scores -- one more all-gather -- are only computed when a restart asks
    # for them), then 3 per PCG iteration (+ the integration-constant / setup mat-vecs)
    assert int(r['coll_calls']) >= 2 + 3 * int(r['iters'])
    # the model predicts like the reference's
    from sgdml_amd import _lib
    from sgdml_amd.utils.desc import Desc

    M, N = g['R_train'].shape[:2]
    c = _lib.Context()
    try:
        xd, gd = c.desc_from_R(g['R_train'].reshape(M, -1), N)
        tp = orc.tril_perms_from_atom_perms(g['perms'])
        F = []
        for coeffs in (g['alphas'], r['alphas']):
            c.predict_upload_model(xd, Desc(N).d_desc_dot_vec(gd, coeffs.reshape(M, -1)), tp, float(g['sig']), None)
            F.append(c.predict(g['R_test'].reshape(len(g['R_test']), -1))[1])
        assert np.abs(F[1] - F[0]).max() <= 5e-3 * np.abs(F[0]).max()
    finally:
        c.close()


@pytest.mark.parametrize('form', [2, 3])
def test_sharded_iterative_without_torch(tmp_path, form):
    """The same sharded solve with NO PyTorch in the processes: two plain subprocesses (no launcher), rendezvous and the
    host-staged collectives over sgdml_amd.hostchannel (GDMLTrain.init_distributed with its default group).  form = 3: the
    fp32 + Gram-correction preconditioner in its sharded form (row shards of X32, Gram matrix summed over the ranks, T0
    replicated) -- converged in no more iterations than the reference."""
    g = load('pcg_n9_m400')
    out = str(tmp_path / 'shard_chan.npz')
    port = 28000 + (os.getpid() % 900) + 3 * form
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE='2', LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port),
                   OMP_NUM_THREADS='2', GDML_OPTIONS='pcg.precon_form=%d' % form)
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, 'tests', '_sharded_worker.py'), out, 'chan'], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    for p in procs:
        so, se = p.communicate(timeout=600)
        assert p.returncode == 0, so[-2000:] + se[-3000:]
    r = dict(np.load(out))
    n_ref = int(g['n_iters'])
    assert np.array_equal(r['inducing'], g['inducing_pts_idxs'])
    if form == 3:
        assert n_ref // 4 <= int(r['iters']) <= n_ref + max(2, n_ref // 10), (int(r['iters']), n_ref)
    else:
        assert abs(int(r['iters']) - n_ref) <= max(2, n_ref // 10), (int(r['iters']), n_ref)
    assert float(r['resid']) <= 1e-4 * float(r['norm_y'])
    assert int(r['coll_calls']) >= 2 + 3 * int(r['iters'])


def _upload_as_K(ctx, A):
    """Load an arbitrary square matrix as the resident 'K' (so that -K + lam I = A for lam = 0): assemble a dummy
    two-atom problem of the right order and overwrite the buffer (pattern of test_cholesky_multi_panel)."""
    import ctypes as C

    n = A.shape[0]
    assert n % 6 == 0
    M = n // 6
    ds = orc.synth_dataset(2, M, seed=1)
    xo, go = orc.desc_from_R(ds['R'].reshape(M, -1))
    ctx.train_upload(xo, go, np.zeros((1, 1), dtype=np.int64))
    ctx.assemble_K(10.0, False)
    assert ctx.K_shape()[0] == n
    p, ld = C.c_void_p(), C.c_int64()
    ctx._check(ctx._lib.gdml_K_dev(ctx._h, C.byref(p), C.byref(ld)))
    buf = np.zeros((n, ld.value))
    buf[:, :n] = -A
    ctx._check(ctx._lib.gdml_memcpy_h2d(ctx._h, p, buf.ctypes.data_as(C.c_void_p), buf.nbytes))


@pytest.mark.parametrize('n', [66, 258, 1026])
def test_lu_solve_general_matrix_vs_lapack(ctx, n):
    """gdml_lu_solve on non-symmetric, indefinite matrices (partial pivoting really permutes): solution vs
    scipy.linalg.solve (dgesv), several panels, ragged last panel."""
    import scipy.linalg as sla

    rs = np.random.RandomState(n)
    A = rs.normal(size=(n, n))
    A[rs.randint(0, n, 5), :] *= 1e-3  # weak rows: pivoting matters
    y = rs.normal(size=n)
    _upload_as_K(ctx, A)
    x = -ctx.lu_solve(0.0, y)
    xr = sla.solve(A, y)
    assert np.linalg.norm(A @ x - y) <= 1e-12 * np.linalg.norm(A, 2) * np.linalg.norm(x)
    assert np.abs(x - xr).max() <= 1e-9 * np.abs(xr).max()
    with pytest.raises(Exception):  # the matrix was consumed
        ctx.lu_solve(0.0, y)


def test_lu_solve_singular_reports(ctx):
    n = 66
    A = np.eye(n)
    A[:, 40] = 0.0
    A[40, :] = 0.0
    _upload_as_K(ctx, A)
    with pytest.raises(np.linalg.LinAlgError, match='singular'):
        ctx.lu_solve(0.0, np.ones(n))


def test_lu_branch_matches_reference():
    """The fixture on which the reference's Cholesky failed and its LU branch ran (analytic.py:101-114): our
    Cholesky reports the failure too, Analytic.solve takes the device LU, and the model predicts like the
    reference's."""
    from sgdml_amd.predict import GDMLPredict
    from sgdml_amd.solvers.analytic import Analytic
    from sgdml_amd.train import GDMLTrain

    g = load('lu_branch')
    took = []
    orig = Analytic.solve

    def spy(self, *a, **kw):
        out = orig(self, *a, **kw)
        took.append(self.used_lu)
        return out

    Analytic.solve = spy
    tr = GDMLTrain()
    try:
        model = tr.train(make_task(g, lam=float(g['lam'])))
    finally:
        Analytic.solve = orig
        tr.__del__()
    assert took == [True]
    pred = GDMLPredict(model)
    nt = len(g['R_test'])
    E, F = pred.predict(g['R_test'].reshape(nt, -1))
    assert np.abs(F - g['F_test']).max() <= 1e-6 * np.abs(g['F_test']).max()
    assert np.abs(E - g['E_test']).max() <= 1e-6 * np.abs(g['E_test']).max()


def test_nystroem_qr_branch_matches_reference(ctx):
    """Second Nystroem factorisation through the alternative branch (reference: QR of [K_nm; sqrt(lam) I],
    iterative.py:313-324; here shifted CholeskyQR3): the factor is unique up to row signs, so L^T L (what the
    preconditioner applies) is compared with the reference's QR-branch output, and the leverage scores with its
    column norms."""
    g = load('nys_qr')
    M, N = g['R_train'].shape[:2]
    sig, lam, idx = float(g['sig']), float(g['lam']), g['col_idxs']
    xd, gd = ctx.desc_from_R(g['R_train'].reshape(M, -1), N)
    tp = orc.tril_perms_from_atom_perms(g['perms'])
    ctx.train_upload(xd, gd, tp)
    ref = g['L_inv_K_mn_qr']
    P_ref = ref.T @ ref
    out = {}
    for force in (0, 1):
        ctx.set_option('nys.force_qr', force)
        ctx.assemble_K(sig, False, idx=idx, alloc_extra_rows=len(idx))
        lev, fac, info = ctx.nystroem_factor(lam, idx, want_factor=True)
        assert (info & 1) == force  # bit 0 = alternative (QR-equivalent) branch; bits 8.. = jitter escalations
        P = fac.T @ fac
        assert np.abs(P - P_ref).max() <= 1e-9 * np.abs(P_ref).max(), force
        np.testing.assert_allclose(lev, (ref**2).sum(0), rtol=1e-8)
        v = np.random.RandomState(0).normal(size=P.shape[0])
        out[force] = ctx.precon_apply(lam, v)
        np.testing.assert_allclose(out[force], (P_ref @ v - v) / lam, rtol=1e-6, atol=1e-6 * np.abs(out[force]).max())
    ctx.set_option('nys.force_qr', 0)


def _reference_solve(ctx, R, y, N, sig, lam, perms=None):
    M = R.shape[0]
    xd, gd = ctx.desc_from_R(R.reshape(M, -1), N)
    tp = np.arange(N * (N - 1) // 2, dtype=np.int64)[None] if perms is None else orc.tril_perms_from_atom_perms(perms)
    ctx.train_upload(xd, gd, tp)
    ctx.assemble_K(sig, False, alloc_extra_rows=1, for_cholesky=lam)
    ctx.chol_set_rhs(y)
    ctx.chol_factor(lam)
    a = ctx.chol_solve(None)
    ctx.predict_upload_model(xd, np.zeros_like(xd), tp, sig, None)
    return a, (lambda v: ctx.kernel_matvec(lam, False, v))


_P6 = np.array([[0, 1, 2, 3, 4, 5, 6, 7, 8], [1, 2, 0, 3, 4, 5, 6, 7, 8], [2, 0, 1, 3, 4, 5, 6, 7, 8],
                [0, 1, 2, 4, 3, 5, 6, 7, 8], [1, 2, 0, 4, 3, 5, 6, 7, 8], [2, 0, 1, 4, 3, 5, 6, 7, 8]])


@pytest.mark.parametrize('lookahead', [0, 1])
@pytest.mark.parametrize('N,M,nb,perms', [(21, 30, 128, None), (9, 100, 256, None), (21, 70, 512, None),
                                          (9, 60, 256, _P6), (26, 20, 128, None)])
def test_distributed_cholesky_single_rank(ctx, N, M, nb, perms, lookahead):
    """gdml_dist_chol_solve with one rank (no communicator): row-cyclic assembly (register-resident kernel for
    P = 1, N <= 21; the LDS kernel's cyclic mode for permutation groups and larger molecules), broadcast-buffer panel
    solve, cyclic-lower trailing update, blocked backward substitution -- vs the single-GPU factorisation.  Both
    schedules: dist.lookahead = 0 (every step in order on the compute stream, the default) and 1 (one panel of look-ahead
    over three streams)."""
    ds = orc.synth_dataset(N, M, seed=9, jitter=0.3)
    y = ds['F'].ravel() / np.std(ds['F'])
    a_ref, Kop = _reference_solve(ctx, ds['R'], y, N, 20.0, 1e-10, perms)
    ctx.set_option('dist.nb', nb)
    ctx.set_option('dist.lookahead', lookahead)
    ctx.set_option('dist.force_panels', 1)  # (round 6: a one-rank call otherwise degenerates to the single-GPU factorisation)
    a = ctx.dist_chol_solve(20.0, 1e-10, y)
    r = Kop(-a) + y  # y - A x with A x = -(K x - lam x)
    assert np.linalg.norm(r) <= 1e-9 * np.linalg.norm(y)
    if lookahead == 0:  # the default one-rank path: the single-GPU schedule behind the same entry point
        ctx.set_option('dist.force_panels', 0)
        a1 = ctx.dist_chol_solve(20.0, 1e-10, y)
        assert np.linalg.norm(Kop(-a1) + y) <= 1e-9 * np.linalg.norm(y)
        assert np.abs(a1 - a_ref).max() <= 1e-4 * np.abs(a_ref).max()
    # alphas of two correct factorisations differ by about cond(A) * eps * |alphas|: the two paths assemble K with different
    # kernels (entries equal to ~1e-16 relative), lam = 1e-10 against |K| ~ 1e0..1e1 gives cond(A) up to ~1e10-1e11, i.e. a
    # relative difference up to ~1e-5 (observed 2e-5 on the 26-atom case): the residual above is the parity statement, this
    # bound only catches a wrong solution
    assert np.abs(a - a_ref).max() <= 1e-4 * np.abs(a_ref).max()


@pytest.mark.parametrize('lookahead', [0, 1])
@pytest.mark.parametrize('world,N,M,nb', [(2, 21, 30, 128), (3, 21, 45, 128), (2, 9, 120, 512)])
def test_distributed_cholesky_processes_share_one_gpu(tmp_path, ctx, world, N, M, nb, lookahead):
    """The block-row-cyclic Cholesky run by `world` processes (each holds only its row blocks of the matrix;
    collectives host-staged through gloo): same solution as one GPU, and every rank holds ~1/world of the matrix.
    lookahead = 1: the opt-in three-stream schedule (comm_ensure_second, block broadcasts on the critical stream, panel
    gather on the collective stream) under host-staged collectives."""
    out = str(tmp_path / 'dchol.npz')
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', OMP_NUM_THREADS='2')
    port = 29600 + (os.getpid() % 300) + 7 * world + M % 7 + 31 * lookahead
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(world),
           '--master-addr', '127.0.0.1', '--master-port', str(port),
           os.path.join(ROOT, 'tests', '_dist_chol_worker.py'), out, str(N), str(M), str(nb), 'host', str(lookahead)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    r = dict(np.load(out))
    a_ref, Kop = _reference_solve(ctx, r['R'], r['y'], N, 20.0, 1e-10)
    res = Kop(-r['alphas']) + r['y']
    assert np.linalg.norm(res) <= 1e-9 * np.linalg.norm(r['y'])
    assert np.abs(r['alphas'] - a_ref).max() <= 1e-5 * np.abs(a_ref).max()
    n = 3 * N * M
    nblk = -(-n // nb)
    assert int(r['coll_calls']) >= 2 * nblk  # per panel: diagonal block + look-ahead block broadcasts, panel gather (+ backward substitution)


def test_distributed_cholesky_rccl_one_gpu_per_rank(tmp_path, ctx):
    """The same factorisation with RCCL (ncclBroadcast of the diagonal / look-ahead blocks, ncclAllGather of the panels from
    the collective stream, all-reduces of the backward substitution) on two physical GPUs.  Skipped on a one-GPU box: until
    a multi-GPU box has run this test the RCCL branch of csrc/dist_chol.hip counts as unverified (README, DESIGN)."""
    from sgdml_amd import _lib

    if _lib.device_count() < 2:
        pytest.skip('needs two GPUs')
    N, M, nb, world = 21, 60, 128, 2
    out = str(tmp_path / 'dchol_rccl.npz')
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', OMP_NUM_THREADS='2', HSA_ENABLE_IPC_MODE_LEGACY='0')
    port = 29400 + (os.getpid() % 300)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(world),
           '--master-addr', '127.0.0.1', '--master-port', str(port),
           os.path.join(ROOT, 'tests', '_dist_chol_worker.py'), out, str(N), str(M), str(nb), 'rccl']
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    r = dict(np.load(out))
    a_ref, Kop = _reference_solve(ctx, r['R'], r['y'], N, 20.0, 1e-10)
    res = Kop(-r['alphas']) + r['y']
    assert np.linalg.norm(res) <= 1e-9 * np.linalg.norm(r['y'])
    assert np.abs(r['alphas'] - a_ref).max() <= 1e-4 * np.abs(a_ref).max()


def test_dropin_train_distributed_analytic(tmp_path):
    """GDMLTrain.train in distributed mode with the analytic solver: Analytic.solve goes through the distributed
    Cholesky (2 processes, one GPU, host-staged collectives) and the model equals the single-process one."""
    from sgdml_amd.train import GDMLTrain

    g = load('pcg_n9_m400')
    out = str(tmp_path / 'dtrain.npz')
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', OMP_NUM_THREADS='2')
    port = 29950 + (os.getpid() % 40)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
           '--master-addr', '127.0.0.1', '--master-port', str(port),
           os.path.join(ROOT, 'tests', '_sharded_worker.py'), out, 'host', 'analytic']
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    r = dict(np.load(out))
    assert str(r['solver']) == 'analytic' and int(r['coll_calls']) > 0
    tr = GDMLTrain()
    try:
        tr._force_solver = 'analytic'
        model = tr.train(make_task(g))
    finally:
        tr.__del__()
    assert np.abs(r['alphas'] - model['alphas_F']).max() <= 1e-5 * np.abs(model['alphas_F']).max()
    assert abs(float(r['c']) - model['c']) <= 1e-6 * max(1.0, abs(model['c']))


def test_sharded_iterative_energy_constraints_one_checkpoint_writer(tmp_path):
    """Energy constraints through GDMLTrain.train with the iterative solver after init_distributed (round 6: row-sharded like
    the force-only systems -- until then every rank solved redundantly under a parked communicator).  Two processes sharing
    the GPU, a clock that makes every tenth iteration a checkpoint: only the group's rank 0 calls save_progr_callback, both
    ranks end with the same coefficients, and they are the single-process solve's (same seed = same inducing columns) to
    the solver's tolerance."""
    from sgdml_amd.train import GDMLTrain

    out = str(tmp_path / 'ecstr_cg.npz')
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', OMP_NUM_THREADS='2')
    port = 29900 + (os.getpid() % 40)
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
           '--master-addr', '127.0.0.1', '--master-port', str(port),
           os.path.join(ROOT, 'tests', '_sharded_worker.py'), out, 'host', 'ecstr_cg']
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    r = dict(np.load(out))
    assert int(r['iters']) >= 20, int(r['iters'])  # long enough for checkpoints to be due
    assert int(r['coll_calls']) > int(r['iters'])  # sharded: collectives in every iteration
    written = [ln for ln in open(out + '.ckpt.rank0').read().split() if ln]
    assert len(written) >= 1 and all(int(v) % 10 == 1 for v in written), written  # solver_iters = iteration + 1
    assert not os.path.exists(out + '.ckpt.rank1')
    g = dict(load('n5_p2_ecstr'))
    g.setdefault('z', np.full(g['R_train'].shape[1], 6))
    task = make_task(g, use_E_cstr=True)
    tr = GDMLTrain()
    try:
        tr._force_solver = 'cg'
        tr._force_n_inducing_pts = 1
        np.random.seed(5)  # rank 0's seed in the worker: the same inducing columns
        model = tr.train(task)
    finally:
        tr.__del__()
    assert abs(int(model['solver_iters']) - int(r['iters'])) <= max(3, int(r['iters']) // 10)
    # lam = 1e-10 (cond ~ 1e10) at solver_tol = 1e-4: two correct iterate sequences that differ in the order of their sums end
    # percent-level apart in the coefficients (observed 0.7 %); a wrong layout would be an O(1) difference
    assert np.abs(r['alphas'] - model['alphas_F']).max() <= 5e-2 * np.abs(model['alphas_F']).max()


@pytest.mark.parametrize('mode', ['ecstr', 'ecstr_dist', 'lu'])
def test_distributed_mode_redundant_solves(tmp_path, mode):
    """After init_distributed: energy constraints (train.py:235-300) go through the distributed Cholesky, whose last row blocks
    hold the M energy rows (round 6; fixtures n5_p2_ecstr -- one row block, the second rank owns nothing -- and
    ecstr_n9_p6_m40 with dist.nb = 128: nine row blocks over two ranks, the reference's coefficients compared directly).
    What the sharded solvers do not carry is solved by every rank on its own GPU with the communicator parked
    (gdml_comm_suspend), like a single-GPU run: the LU branch of a system on which the (distributed) Cholesky fails
    (analytic.py:101-114; fixture lu_branch).  Two processes sharing the GPU: the model equals the reference's."""
    from sgdml_amd.predict import GDMLPredict

    g = load({'ecstr': 'n5_p2_ecstr', 'ecstr_dist': 'ecstr_n9_p6_m40', 'lu': 'lu_branch'}[mode])
    out = str(tmp_path / 'redundant.npz')
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', OMP_NUM_THREADS='2')
    port = 29700 + (os.getpid() % 200) + {'ecstr': 0, 'lu': 3, 'ecstr_dist': 5}[mode]
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
           '--master-addr', '127.0.0.1', '--master-port', str(port),
           os.path.join(ROOT, 'tests', '_sharded_worker.py'), out, 'host', mode]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    r = dict(np.load(out))
    assert list(r['used_lu']) == [mode == 'lu']
    assert int(r['coll_calls']) > 0  # the factorisation ran through the communicator (the LU case: its failing first attempt)
    model = {k: r[k] for k in r if k not in ('used_lu', 'coll_calls', 'alphas_F')}
    model.update(type='m', sig=int(r['sig']), c=float(r['c']), std=float(r['std']))
    nt = len(g['R_test'])
    E, F = GDMLPredict(model).predict(g['R_test'].reshape(nt, -1))
    tol = {'lu': 1e-6, 'ecstr': 2e-4, 'ecstr_dist': 1e-7}[mode]  # as in the single-GPU tests of the fixtures (lam = 1e-10 / 1e-8)
    assert np.abs(F - g['F_test']).max() <= tol * np.abs(g['F_test']).max()
    assert np.abs(E - g['E_test']).max() <= tol * max(1.0, np.abs(g['E_test']).max())
    if mode == 'ecstr_dist':  # cond(A) ~ 1e9 at lam = 1e-8: coefficients of two correct solves agree to ~1e-6
        assert np.abs(r['alphas_F'] - g['alphas_F']).max() <= 1e-5 * np.abs(g['alphas_F']).max()
        assert np.abs(r['alphas_E'] - g['alphas_E']).max() <= 1e-5 * np.abs(g['alphas_E']).max()


def _ecstr_system(ctx, g):
    """Uploads the energy-constraint fixture; returns (label vector, mat-vec of A = -K + lam I with the energy rows)."""
    M, N = g['R_train'].shape[:2]
    xd, gd = ctx.desc_from_R(g['R_train'].reshape(M, -1), N)
    tp = orc.tril_perms_from_atom_perms(g['perms'])
    ctx.train_upload(xd, gd, tp)
    ctx.predict_upload_model(xd, np.zeros_like(xd), tp, float(g['sig']), np.zeros(M))
    return g['y'], (lambda v: ctx.kernel_matvec(float(g['lam']), True, v))


@pytest.mark.parametrize('lookahead', [0, 1])
@pytest.mark.parametrize('nb', [128, 256, 512])
def test_distributed_cholesky_energy_constraints_single_rank(ctx, nb, lookahead):
    """gdml_dist_chol_solve on a system with energy constraints (n = 3N M + M, round 6): the panel schedule of the distributed
    code on one rank (dist.force_panels) -- force rows from the row-cyclic assembly, the M energy rows from
    assemble_erows_cyclic_launch, in row blocks 8 (nb = 128: 56 force rows + 40 energy rows), 4 and 2 -- against the reference's
    coefficients (fixture ecstr_n9_p6_m40: GDMLTrain.train with use_E_cstr) and by the residual through the reference-pinned
    mat-vec; then the one-rank default (the single-GPU schedule behind the same entry point)."""
    g = load('ecstr_n9_p6_m40')
    y, Aop = _ecstr_system(ctx, g)
    a_ref = np.hstack((g['alphas_F'], g['alphas_E']))
    ctx.set_option('dist.nb', nb)
    ctx.set_option('dist.lookahead', lookahead)
    for force in (1, 0):
        ctx.set_option('dist.force_panels', force)
        a = ctx.dist_chol_solve(float(g['sig']), float(g['lam']), y)
        assert a.shape == a_ref.shape
        assert np.linalg.norm(Aop(-a) + y) <= 1e-10 * np.linalg.norm(y)
        assert np.abs(a - a_ref).max() <= 1e-5 * np.abs(a_ref).max()
    with pytest.raises(Exception):  # neither 3N M nor 3N M + M values
        ctx.dist_chol_solve(float(g['sig']), float(g['lam']), y[:-1])


@pytest.mark.parametrize('world', [2, 3])
def test_sharded_nystroem_pcg_with_energy_constraints(tmp_path, ctx, world):
    """Energy constraints in the ROW-SHARDED iterative path (round 6): every rank holds the force rows of its points followed
    by their energy rows; the replicated device vectors are rank-major inside the library (VecLayout, csrc/common.h) and
    permuted where they enter and leave.  `world` processes sharing the GPU (host-staged collectives; 40 points over 3 ranks =
    14 + 14 + 12: a ragged last shard) against the same calls on one context: leverage scores, one preconditioner
    application, the mat-vec, the PCG solution, an iterate fetched inside the callback, a warm start."""
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import _ecstr_shard_worker as w

    g = load('ecstr_n9_p6_m40')
    out = str(tmp_path / 'ecstr_shard.npz')
    env = dict(os.environ, MASTER_ADDR='127.0.0.1', OMP_NUM_THREADS='2')
    port = 29500 + (os.getpid() % 90) + 3 * world
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(world),
           '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.join(ROOT, 'tests', '_ecstr_shard_worker.py'), out]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    r = dict(np.load(out))
    idx, v = w.inputs(g)
    one = w.run(ctx, g, idx, v)
    M, N = g['R_train'].shape[:2]
    per = -(-M // world)
    assert list(r['rows']) == [max(0, min(M, (k + 1) * per) - k * per) * (3 * N + 1) for k in range(world)]  # 1/world each
    assert np.abs(r['Kv'] - one['Kv']).max() <= 1e-11 * np.abs(one['Kv']).max()
    # factor rows are the same numbers up to the order of the m x m sums: lam = 1e-8, cond ~ 1e9
    assert np.abs(r['lev'] - one['lev']).max() <= 1e-5 * np.abs(one['lev']).max()
    assert np.abs(r['z'] - one['z']).max() <= 1e-5 * np.abs(one['z']).max()
    assert int(r['pinfo']) == 0 and int(one['pinfo']) == 0
    assert abs(int(r['iters']) - int(one['iters'])) <= max(3, int(one['iters']) // 10)
    y = g['y']
    Aop = lambda a: ctx.kernel_matvec(float(g['lam']), True, a)
    for x in (r['x'], one['x']):
        assert np.linalg.norm(-Aop(x) - y) <= 2e-5 * np.linalg.norm(y)   # A x = y, A v = -(K v - lam v)
    assert np.abs(r['x5'] - one['x5']).max() <= 1e-4 * np.abs(one['x5']).max()  # the iterate of iteration 5, reference order
    assert int(r['iters_w']) <= 1

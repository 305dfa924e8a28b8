"""NumPy restatement of the on-device variable-cell relaxation (gdml_cell_relax_run, csrc/cellrelax.hip) on top of the restated
virial (tests/_stress_ref.py) and the restated FIRE update (tests/_relax_ref.run), and a periodic bound toy model.

The contract (include/gdml_hip.h states the same).  Per geometry: a fixed reference lattice L0, a deformation gradient Fd and
reference positions s_i; r_i = Fd s_i, lattice L = Fd L0 (cell vectors in the columns).  Generalised coordinates: the (N + 3) x 3
array u = (s_1 .. s_N, C), C = cell_factor Fd.  Evaluation t of an active geometry:
  1. Fd = C / cell_factor;  L = Fd L0;  r = Fd s;  Vol = |det L|  (3 x 3 products summed left to right, inverses adjugate / det)
  2. E, F, W = predictor with virial for (r, L)
  3. g = f_unit F;  G_i = Fd^T g_i;  T = mask o (f_unit W + pressure Vol I);  G_cell = -T Fd^-T / cell_factor
     (mask = 1: G = -dH/du of H = f_unit E + pressure Vol, because dE = W : dFd Fd^-1 and dVol = Vol tr(dFd Fd^-1) at fixed s)
  4. _relax_ref.run's step on u with G: f_atom = max over the N + 3 rows of |G_row|, convergence, budget, the FIRE update
"""
import functools

import numpy as np

import _md_ref as mr
import _relax_ref as rr
import _stress_ref as sr
from oracle import gdml_oracle as orc


def adj_det(M):
    """Adjugate (row-major 3 x 3) and determinant in the order the header writes down."""
    (a, b, c), (d, e, f), (g, h, i) = np.asarray(M, dtype=np.float64)
    adj = np.array([[e * i - f * h, c * h - b * i, b * f - c * e],
                    [f * g - d * i, a * i - c * g, c * d - a * f],
                    [d * h - e * g, b * g - a * h, a * e - b * d]])
    return adj, a * adj[0, 0] + b * adj[1, 0] + c * adj[2, 0]


def inv3(M):
    adj, det = adj_det(M)
    return adj / det


def mul3(A, B):
    """A @ B with every entry summed from left to right."""
    return A[:, [0]] * B[0][None] + A[:, [1]] * B[1][None] + A[:, [2]] * B[2][None]


def split(u):
    """u (B,3N+9) -> s (B,N,3), C (B,3,3)."""
    u = np.asarray(u, dtype=np.float64)
    return u[:, :-9].reshape(len(u), -1, 3), u[:, -9:].reshape(len(u), 3, 3)


def join(s, C):
    B = len(s)
    return np.concatenate([np.reshape(s, (B, -1)), np.reshape(C, (B, 9))], axis=1)


def cartesian(u, L0, cell_factor):
    """Step 1 for every geometry: (r (B,3N), L (B,3,3), L^-1, Vol (B,), Fd, Fd^-1)."""
    s, C = split(u)
    B = len(s)
    Fd = C / cell_factor
    L = np.array([mul3(Fd[b], L0[b]) for b in range(B)])
    r = s[:, :, [0]] * Fd[:, None, :, 0] + s[:, :, [1]] * Fd[:, None, :, 1] + s[:, :, [2]] * Fd[:, None, :, 2]
    Li = np.array([inv3(L[b]) for b in range(B)])
    vol = np.abs(np.array([adj_det(L[b])[1] for b in range(B)]))
    Fi = np.array([inv3(Fd[b]) for b in range(B)])
    return r.reshape(B, -1), L, Li, vol, Fd, Fi


def gen_force(virial_fn, u, L0, cell_factor, pressure=0.0, mask=None, f_unit=1.0):
    """Steps 1-3: (E (B,), G (B,3N+9), Vol (B,), r, L) of coordinates u.  virial_fn(R (B,3N), lattices (B,3,3)) -> (E, F, W)
    scaled as predict_virial() scales them."""
    mask = np.ones((3, 3)) if mask is None else np.asarray(mask, dtype=np.float64)
    r, L, _, vol, Fd, Fi = cartesian(u, L0, cell_factor)
    E, F, W = virial_fn(r, L)
    B = len(r)
    g = f_unit * F.reshape(B, -1, 3)
    G_at = np.einsum('bac,bia->bic', Fd, g)  # Fd^T g_i
    T = mask[None] * (f_unit * W + (pressure * vol)[:, None, None] * np.eye(3)[None])
    G_cell = -np.einsum('bac,bdc->bad', T, Fi) / cell_factor  # T Fd^-T
    return E, join(G_at, G_cell), vol, r, L


def enthalpy(virial_fn, u, L0, cell_factor, pressure=0.0, f_unit=1.0):
    r, L, _, vol, _, _ = cartesian(u, L0, cell_factor)
    return f_unit * virial_fn(r, L)[0] + pressure * vol


def model_virial_fn(model, rel_noise=0.0, seed=0):
    """Restated (E, F, W) of a model with one lattice per geometry, scaled like predict_virial(); rel_noise: E, F and W each
    perturbed by independent normal noise of rel_noise times their largest magnitude (a fresh draw per call)."""
    rs = np.random.RandomState(seed)

    def fn(R, lats):
        out = [sr.virial_of_model(model, R[b:b + 1], lattice=lats[b]) for b in range(len(R))]
        E, F, W = (np.concatenate([o[i] for o in out]) for i in range(3))
        if rel_noise:
            E = E + rel_noise * np.abs(E).max() * rs.standard_normal(E.shape)
            F = F + rel_noise * np.abs(F).max() * rs.standard_normal(F.shape)
            W = W + rel_noise * np.abs(W).max() * rs.standard_normal(W.shape)
        return E, F, W

    return fn


def fresh_state(R0, L0, cell_factor, dt_start=0.1, alpha_start=0.1):
    R0 = np.asarray(R0, dtype=np.float64)
    B, n3 = R0.shape
    st = rr.fresh_state(B, n3 + 9, dt_start, alpha_start)
    st.update(S=R0.copy(), C=np.broadcast_to(cell_factor * np.eye(3), (B, 3, 3)).copy(), L0=np.array(L0, dtype=np.float64))
    return st


def run(virial_fn, fmax, state, pressure=0.0, mask=None, cell_factor=None, max_steps=1000, f_unit=1.0, **fire):
    """The restated run from `state` ({'S', 'C', 'L0'} and the FIRE state; fresh_state() makes a fresh one).  Returns a dict like
    GDMLPredict.relax_cell's with the frames of every evaluation ('R', 'lattice', 'u') and _relax_ref.run's margins."""
    L0 = np.asarray(state['L0'], dtype=np.float64)
    u0 = join(state['S'], state['C'])
    n_at = (u0.shape[1] - 9) // 3
    cf = float(n_at) if cell_factor is None else float(cell_factor)
    vols = []

    def force(u):
        E, G, vol, _, _ = gen_force(virial_fn, u, L0, cf, pressure, mask, f_unit)
        vols.append(vol)
        return E, G

    out = rr.run(force, u0, fmax, max_steps=max_steps, state={k: state[k] for k in ('V', 'dt', 'alpha', 'n_pos', 'n_taken')},
                 f_unit=1.0, **fire)
    B = len(u0)
    frames = [cartesian(u, L0, cf) for u in out['R']]
    out['u'] = out.pop('R')
    out['R'] = np.array([f[0] for f in frames])
    out['lattice'] = np.array([f[1] for f in frames])
    # a frozen geometry repeats the volume of its last evaluation (rr.run evaluates it on, its coordinates unchanged)
    out['vol_hist'] = np.array(vols)
    r, L, _, vol, _, _ = cartesian(out['R_end'], L0, cf)
    s, C = split(out['R_end'])
    out['state'].update(S=s.reshape(B, -1), C=C, L0=L0)
    out.update(u_end=out['R_end'], R_end=r, lattice_end=L, vol_end=vol, G_end=out.pop('F_end'))
    return out


def metric(L):
    """L^T L of lattices (B,3,3): the rotation-free content of a cell."""
    return np.einsum('bka,bkc->bac', L, L)


def pair_distances(R, lats):
    """Minimum-image pair distances (B,D) of geometries in their own cells."""
    return np.array([np.linalg.norm(sr.pair_vectors(R[b:b + 1], (lats[b], np.linalg.inv(lats[b])))[0], axis=-1)
                     for b in range(len(R))])


def image_integers(R, lats):
    """The minimum-image integers rint(L^-1 (r_i - r_j)) (B,D,3) and the fractional parts' distance from a half."""
    out, margin = [], np.inf
    for b in range(len(R)):
        r = np.reshape(R[b], (-1, 3))
        i, j = orc.tril_pairs(len(r))
        c = (r[i] - r[j]) @ np.linalg.inv(lats[b]).T
        out.append(np.around(c))
        margin = min(margin, np.abs(np.abs(c - np.around(c)) - 0.5).min())
    return np.array(out), margin


# ---- the periodic bound toy model

TOY_LATTICE = np.array([[4.6, 0.3, 0.0], [0.0, 4.3, 0.2], [0.15, 0.0, 4.9]])  # cell vectors in the columns


def _springs_pbc(R, lats, d0):
    """E = sum over pairs (d - d0)^2 / 2 on the minimum-image distances, F = -grad E and W = dE/d eps for geometries R (M,3N)
    in cells lats (M,3,3)."""
    M = len(R)
    N = R.shape[1] // 3
    i, j = orc.tril_pairs(N)
    E, F, W = np.zeros(M), np.zeros((M, N, 3)), np.zeros((M, 3, 3))
    for m in range(M):
        dk = sr.pair_vectors(R[m:m + 1], (lats[m], np.linalg.inv(lats[m])))[0]
        dist = np.sqrt((dk ** 2).sum(-1))
        E[m] = 0.5 * ((dist - d0) ** 2).sum()
        pair = -((dist - d0) / dist)[:, None] * dk  # force on atom i of a pair
        np.add.at(F[m], i, pair)
        np.subtract.at(F[m], j, pair)
        W[m] = -np.einsum('ka,kc->ac', pair, dk)
    return E, F.reshape(M, -1), W


def springs_virial_fn(d0):
    return lambda R, lats: _springs_pbc(np.asarray(R), np.asarray(lats), d0)


@functools.lru_cache(maxsize=None)
def toy():
    """(model, seven starts (7,18), their lattices (7,3,3), rest distances d0 (15,), fmax): six atoms in the cell TOY_LATTICE
    (edges about 3: with six atoms spread over it, pairs wrap along all three cell vectors), harmonic springs (k = 1) on all 15
    MINIMUM-IMAGE pair distances.  M = 150 training geometries: 0.1 normal jitter on the atoms and a random strain of up to 3 %
    per component on atoms and cell together, descriptors with each geometry's own cell; sigma = 1, lambda = 1e-10, one
    permutation, c = 0, RandomState(3); trained with the oracle on the CPU (n = 2700).  Seven starts: the base strained by
    about 2 % with a shear and displaced by 0.08 normal; fmax = 1e-3 of the largest atomic force of the starts."""
    rs = np.random.RandomState(3)
    N, M, sig, lam = 6, 150, 1.0, 1e-10
    # six points of the 3 x 3 x 3 grid of fractional thirds, every third present along every axis: pair differences are 0 or
    # +-1/3 (2/3 wraps to -1/3), a sixth away from the half at which the minimum image jumps
    frac = np.array([[0, 0, 0], [1, 1, 0], [2, 0, 1], [0, 2, 1], [1, 0, 2], [2, 2, 2]], float) / 3.0
    base = frac @ TOY_LATTICE.T + 0.05 * rs.standard_normal((N, 3))
    lat_inv = np.linalg.inv(TOY_LATTICE)
    dk0 = sr.pair_vectors(base.reshape(1, -1), (TOY_LATTICE, lat_inv))[0]
    d0 = np.sqrt((dk0 ** 2).sum(-1))
    eps = 0.03 * (2.0 * rs.random_sample((M, 3, 3)) - 1.0)
    S = np.eye(3)[None] + 0.5 * (eps + eps.transpose(0, 2, 1))
    R_train = np.einsum('mab,mib->mia', S, base[None] + 0.1 * rs.standard_normal((M, N, 3))).reshape(M, -1)
    L_train = np.einsum('mab,bc->mac', S, TOY_LATTICE)
    e7 = 0.02 * (2.0 * rs.random_sample((7, 3, 3)) - 1.0)
    e7[:, 0, 1] += 0.02  # a shear
    S7 = np.eye(3)[None] + e7
    starts = np.einsum('mab,mib->mia', S7, base[None] + 0.08 * rs.standard_normal((7, N, 3))).reshape(7, -1)
    L_starts = np.einsum('mab,bc->mac', S7, TOY_LATTICE)
    _, F_train, _ = _springs_pbc(R_train, L_train, d0)
    std = np.std(F_train)
    xg = [orc.desc_from_R(R_train[m:m + 1], (L_train[m], np.linalg.inv(L_train[m]))) for m in range(M)]
    x, gd = np.concatenate([a for a, _ in xg]), np.concatenate([b for _, b in xg])
    perms = np.arange(N)[None]
    tp = orc.tril_perms_from_atom_perms(perms)
    lin = orc.tril_perms_lin_from_tril_perms(tp)
    K = orc.assemble_K(x, gd, lin, sig)
    alphas, _ = orc.analytic_solve(K, F_train.ravel() / std, lam)
    model = {'type': 'm', 'z': np.ones(N, dtype=np.int64), 'R_desc': np.ascontiguousarray(x.T),
             'R_d_desc_alpha': orc.d_desc_dot_vec(gd, alphas.reshape(M, -1)), 'sig': sig, 'std': float(std), 'c': 0.0,
             'perms': perms, 'tril_perms_lin': lin, 'lattice': TOY_LATTICE.copy()}
    _, F0, _ = model_virial_fn(model)(starts, L_starts)
    fmax = 1e-3 * np.sqrt((F0.reshape(7, N, 3) ** 2).sum(-1)).max()
    for a in (starts, L_starts, d0):
        a.setflags(write=False)
    return model, starts, L_starts, d0, float(fmax)


# parameter sets the tests run on the toy: FIRE parameters, and the pressure of the runs under load
TOY_FIRE = dict(dt_start=0.1, max_step=0.2)
TOY_PRESSURE = -0.004  # tension: the springs end stretched, which makes the minimum of H strict (tests/test_cellrelax_cpu.py)

# step-by-step parity on the periodic fixtures: fmax so small that nothing converges, mask = 1, a nonzero pressure, a sheared
# start Fd, a start in mid-run (seeded velocities, one step taken)
PARITY = dict(fmax=1e-12, max_step=0.02)
PARITY_DT = {'n4_p6_pbc': 0.1, 'n10_p2_pbc': 5.0 * mr.DT['n10_p2_pbc']}
PARITY_V = {'n4_p6_pbc': 0.2, 'n10_p2_pbc': mr.V_SCALE['n10_p2_pbc']}
PARITY_PRESSURE = 0.01
PARITY_V_CELL = 0.2
PARITY_FD = np.array([[1.01, 0.012, 0.0], [0.004, 0.99, -0.008], [0.0, 0.006, 1.015]])


def parity_params(name):
    return dict(PARITY, dt_start=PARITY_DT[name])


@functools.lru_cache(maxsize=None)
def parity_case(name):
    """(model, state of seven starts in mid-run, cell_factor) of a periodic fixture: S = the fixture's geometries pulled back by
    PARITY_FD (so that Fd s are the fixture's), C = N PARITY_FD, L0 = Fd^-1 model lattice, seeded velocities on atoms and cell,
    n_taken = 1."""
    model, R7 = mr.case(name)
    R0 = np.ascontiguousarray(R7[np.arange(7) % len(R7)])
    N = R0.shape[1] // 3
    Fi = np.linalg.inv(PARITY_FD)
    S = np.einsum('ab,mib->mia', Fi, R0.reshape(7, N, 3)).reshape(7, -1)
    L0 = np.broadcast_to(Fi @ np.asarray(model['lattice'], dtype=np.float64), (7, 3, 3)).copy()
    st = rr.fresh_state(7, 3 * N + 9, PARITY_DT[name])
    st['V'] = mr.start_velocities(7, 3 * N + 9, PARITY_V[name])
    st['V'][:, -9:] *= PARITY_V_CELL  # (a cell row moves every atom)
    st['n_taken'][:] = 1
    st.update(S=S, C=np.broadcast_to(float(N) * PARITY_FD, (7, 3, 3)).copy(), L0=L0)
    for a in st.values():
        a.setflags(write=False)
    return model, st, float(N)


@functools.lru_cache(maxsize=None)
def parity_reference(name, n_eval):
    """Restated run of parity_case(name) (n_eval evaluations) and its sensitivity to the predictor's agreed error: the deviation
    of a second restated run whose E, F and W carry independent noise of 1e-10 relative (the scheme of _relax_ref).  Computed
    once per session, only read."""
    model, st, cf = parity_case(name)
    kw = dict(pressure=PARITY_PRESSURE, cell_factor=cf, max_steps=n_eval - 1, **parity_params(name))
    fmax = kw.pop('fmax')
    clean = run(model_virial_fn(model), fmax, st, **kw)
    noisy = run(model_virial_fn(model, rel_noise=1e-10, seed=1), fmax, st, **kw)
    return model, st, cf, clean, deviation(clean, noisy)


@functools.lru_cache(maxsize=None)
def toy_reference(pressure):
    """The same for the toy model run to convergence under `pressure`."""
    model, starts, L_starts, _, fmax = toy()
    st = fresh_state(starts, L_starts, 6.0, TOY_FIRE['dt_start'])
    kw = dict(pressure=pressure, cell_factor=6.0, max_steps=400, **TOY_FIRE)
    clean = run(model_virial_fn(model), fmax, st, **kw)
    noisy = run(model_virial_fn(model, rel_noise=1e-10, seed=1), fmax, st, **kw)
    return clean, deviation(clean, noisy)


def deviation(clean, noisy):
    dev = {'V_end': np.abs(clean['state']['V'] - noisy['state']['V']).max()}
    for k in ('R', 'lattice', 'R_end', 'lattice_end', 'E_hist', 'vol_hist', 'fmax_hist'):
        dev[k] = np.abs(clean[k] - noisy[k]).max() if clean[k].shape == noisy[k].shape else np.inf
    dev['metric_end'] = np.abs(metric(clean['lattice_end']) - metric(noisy['lattice_end'])).max()
    dev['pairs_end'] = np.abs(pair_distances(clean['R_end'], clean['lattice_end']) -
                              pair_distances(noisy['R_end'], noisy['lattice_end'])).max()
    for o in (clean, noisy):
        for a in o.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return dev


# ---- what the GPU test and tools/cellrelax_parity.py measure

PARITY_FIXTURES = ('n4_p6_pbc', 'n10_p2_pbc')
PARITY_BATCHES = (1, 7)
PARITY_N_EVAL = 30
PARITY_KEYS = ('R', 'lattice', 'V_end', 'E_hist', 'vol_hist', 'fmax_hist')
BOUND_FACTOR = 10.0  # tests/test_relax_gpu.py: a systematic error adds up over the steps where the noise does not
EXACT_STATE = ('dt', 'alpha', 'n_pos', 'n_taken')


def sub_state(state, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in state.items()}


def parity_measure(pred, name, B, n_eval=PARITY_N_EVAL):
    """One parity case on the device: GDMLPredict.relax_cell from parity_case(name)'s first B starts, every evaluation
    recorded, against the restated run.  Per compared quantity the error, the restatement's sensitivity, what the test allows
    (BOUND_FACTOR x sensitivity; for E, Vol and f_atom plus the predictor's agreed 1e-10 of the largest value) and their ratio;
    beside them the exact comparisons."""
    model, st, cf, ref, dev = parity_reference(name, n_eval)
    out = pred.relax_cell(st['S'][:B], state=sub_state(st, slice(0, B)), pressure=PARITY_PRESSURE, cell_factor=cf,
                          max_steps=n_eval - 1, record_every=1, **parity_params(name))
    got = {'R': out['R'], 'lattice': out['lattice'], 'V_end': out['state']['V'], 'E_hist': out['E_hist'],
           'vol_hist': out['vol_hist'], 'fmax_hist': out['fmax_hist']}
    want = {'R': ref['R'][:, :B], 'lattice': ref['lattice'][:, :B], 'V_end': ref['state']['V'][:B], 'E_hist': ref['E_hist'][:, :B],
            'vol_hist': ref['vol_hist'][:, :B], 'fmax_hist': ref['fmax_hist'][:, :B]}
    m = {}
    for k in PARITY_KEYS:
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        allowed = BOUND_FACTOR * dev[k] + (1e-10 * np.abs(ref[k]).max() if k.endswith('_hist') else 0.0)
        err = float(np.abs(got[k] - want[k]).max())
        m[k] = dict(error=err, sensitivity=float(dev[k]), allowed=float(allowed), ratio=err / allowed)
    m['state_equal'] = all(np.array_equal(out['state'][k], ref['state'][k][:B]) for k in EXACT_STATE)
    m['none_converged'] = bool(not out['converged'].any() and (out['n_steps'] == n_eval - 1).all())
    m['frames_are_the_end'] = bool(np.array_equal(out['R'][-1], out['R_end']) and np.array_equal(out['lattice'][-1], out['lattice_end']))
    return m

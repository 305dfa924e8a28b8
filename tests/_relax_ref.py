"""NumPy restatement of the on-device geometry relaxation (gdml_relax_run, csrc/relax.hip) around a force callback, the margins
of its decisions, and a bound toy model (the committed fixtures are fits to synthetic data without a minimum: under FIRE their
molecules dissociate or collapse, so they serve for step-by-step parity only).

The step (the contract; include/gdml_hip.h and csrc/relax.hip state the same).  g = f_unit * F, F the forces of predict(); sums
and norms over a replica's 3N coordinates; state v, dt, alpha, n_pos, n_taken per replica.  Evaluation t = 0, 1, ... of an
active replica:
  1. E, F = predictor(r);  f_atom = max over atoms |g_atom|;  both into the history
  2. f_atom < fmax: converged -- r, v, dt, alpha, n_pos, n_taken, E, F freeze, never written again
  3. else t = max_steps: stops unconverged, freezes the same way
  4. else, if n_taken > 0:  p = g . v;
       p > 0:   v <- (1 - alpha) v + (alpha |v| / |g|) g;  if n_pos > n_min: dt <- min(dt f_inc, dt_max), alpha <- alpha f_alpha;
                n_pos += 1
       p <= 0:  v <- 0, alpha <- alpha_start, dt <- dt f_dec, n_pos <- 0
     v <- v + dt g;  Delta = dt v;  |Delta| > max_step: Delta <- Delta (max_step / |Delta|);  r <- r + Delta;  n_taken += 1
"""
import functools

import numpy as np

import _md_ref as mr
from oracle import gdml_oracle as orc

DEFAULTS = dict(dt_start=0.1, dt_max=None, max_step=0.2, n_min=5, f_inc=1.1, f_dec=0.5, alpha_start=0.1, f_alpha=0.99)


def fresh_state(B, n3, dt_start=0.1, alpha_start=0.1):
    return dict(V=np.zeros((B, n3)), dt=np.full(B, float(dt_start)), alpha=np.full(B, float(alpha_start)),
                n_pos=np.zeros(B, dtype=np.int64), n_taken=np.zeros(B, dtype=np.int64))


def run(force_fn, R0, fmax, max_steps=1000, dt_start=0.1, dt_max=None, max_step=0.2, n_min=5, f_inc=1.1, f_dec=0.5,
        alpha_start=0.1, f_alpha=0.99, state=None, f_unit=1.0):
    """force_fn(R (B,3N)) -> (E (B,), F (B,3N)) scaled as predict() scales them (called with all B geometries at every
    evaluation, frozen ones included, like the general route).  Returns a dict like GDMLPredict.relax's with R frames of every
    evaluation ('R', 'V': the state each evaluation started from), and per replica: 'neg_events' (negative-power events),
    'clipped' (clipped steps), 'neg_at' (their evaluation indices), 'power_margin' (smallest |g.v| / (|g| |v|) over the
    branch decisions; inf without one) and 'fmax_margin' (smallest |f_atom - fmax| / fmax over the evaluations)."""
    R = np.array(R0, dtype=np.float64).reshape(-1, np.shape(R0)[-1])
    B, n3 = R.shape
    if dt_max is None:
        dt_max = 10.0 * dt_start
    st = fresh_state(B, n3, dt_start, alpha_start) if state is None else {k: np.array(v) for k, v in state.items()}
    V, dt, alpha, n_pos, n_taken = st['V'], st['dt'], st['alpha'], st['n_pos'], st['n_taken']
    active = np.ones(B, dtype=bool)
    conv = np.zeros(B, dtype=bool)
    n_steps = np.full(B, -1, dtype=np.int64)
    E_end, F_end, f_end = np.zeros(B), np.zeros((B, n3)), np.zeros(B)
    hist = {k: [] for k in ('E', 'f', 'R', 'V')}
    neg, clipped = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    neg_at = [[] for _ in range(B)]
    pm, fm = np.full(B, np.inf), np.full(B, np.inf)
    for t in range(max_steps + 1):
        if not active.any():
            break
        E, F = force_fn(R)
        hist['R'].append(R.copy())
        hist['V'].append(V.copy())
        for b in np.nonzero(active)[0]:
            g = f_unit * F[b]
            f_atom = np.sqrt((g.reshape(-1, 3) ** 2).sum(axis=1)).max()
            E_end[b], F_end[b], f_end[b] = E[b], F[b], f_atom
            fm[b] = min(fm[b], abs(f_atom - fmax) / fmax)
            if f_atom < fmax or t == max_steps:
                active[b], conv[b], n_steps[b] = False, f_atom < fmax, t
                continue
            v = V[b]
            if n_taken[b] > 0:
                p = np.sum(g * v)
                g_nrm, v_nrm = np.sqrt(np.sum(g * g)), np.sqrt(np.sum(v * v))
                if g_nrm > 0 and v_nrm > 0:
                    pm[b] = min(pm[b], abs(p) / (g_nrm * v_nrm))
                if p > 0.0:
                    v = (1.0 - alpha[b]) * v + (alpha[b] * v_nrm / g_nrm) * g
                    if n_pos[b] > n_min:
                        dt[b] = min(dt[b] * f_inc, dt_max)
                        alpha[b] = alpha[b] * f_alpha
                    n_pos[b] += 1
                else:
                    v = np.zeros(n3)
                    alpha[b] = alpha_start
                    dt[b] = dt[b] * f_dec
                    n_pos[b] = 0
                    neg[b] += 1
                    neg_at[b].append(t)
            v = v + dt[b] * g
            d = dt[b] * v
            d_nrm = np.sqrt(np.sum(d * d))
            if d_nrm > max_step:
                d = d * (max_step / d_nrm)
                clipped[b] += 1
            V[b] = v
            R[b] = R[b] + d
            n_taken[b] += 1
        hist['E'].append(E_end.copy())
        hist['f'].append(f_end.copy())
    return dict(R_end=R, E_end=E_end, F_end=F_end, fmax_end=f_end, n_steps=n_steps, converged=conv,
                E_hist=np.array(hist['E']), fmax_hist=np.array(hist['f']), R=np.array(hist['R']), V=np.array(hist['V']),
                state=dict(V=V, dt=dt, alpha=alpha, n_pos=n_pos, n_taken=n_taken), neg_events=neg, clipped=clipped,
                neg_at=neg_at, power_margin=pm, fmax_margin=fm)


# ---- the bound toy model

def _springs(R, d0):
    """E = sum over pairs (d - d0)^2 / 2 and F = -grad E for geometries R (M,N,3)."""
    i, j = orc.tril_pairs(R.shape[1])
    diff = R[:, i, :] - R[:, j, :]
    dist = np.sqrt((diff ** 2).sum(-1))
    E = 0.5 * ((dist - d0[None]) ** 2).sum(-1)
    pair = -((dist - d0[None]) / dist)[..., None] * diff  # force on atom i of a pair
    F = np.zeros_like(R)
    for m in range(R.shape[0]):
        np.add.at(F[m], i, pair[m])
        np.subtract.at(F[m], j, pair[m])
    return E, F


@functools.lru_cache(maxsize=None)
def toy():
    """(model, seven starts (7,18), equilibrium pair distances d0 (15,), fmax): six atoms on the first six points of a 3 x 3 x 3
    grid of spacing 1.5 plus 0.2 normal jitter, harmonic springs (k = 1) on all 15 pair distances, M = 150 training geometries
    with 0.1 normal jitter, sigma = 1, lambda = 1e-10, one permutation, c = 0, RandomState(3); seven starts displaced by 0.08
    normal; fmax = 1e-3 of the largest atomic force of the starts.  Trained with the oracle on the CPU (n = 2700)."""
    rs = np.random.RandomState(3)
    N, M, sig, lam = 6, 150, 1.0, 1e-10
    grid = np.array([[a, b, c] for a in range(3) for b in range(3) for c in range(3)], float) * 1.5
    base = grid[:N] + 0.2 * rs.standard_normal((N, 3))
    i, j = orc.tril_pairs(N)
    d0 = np.sqrt(((base[i] - base[j]) ** 2).sum(-1))
    R_train = base[None] + 0.1 * rs.standard_normal((M, N, 3))
    starts = (base[None] + 0.08 * rs.standard_normal((7, N, 3))).reshape(7, -1)
    _, F_train = _springs(R_train, d0)
    std = np.std(F_train)
    x, gd = orc.desc_from_R(R_train.reshape(M, -1))
    perms = np.arange(N)[None]
    tp = orc.tril_perms_from_atom_perms(perms)
    lin = orc.tril_perms_lin_from_tril_perms(tp)
    K = orc.assemble_K(x, gd, lin, sig)
    alphas, _ = orc.analytic_solve(K, F_train.ravel() / std, lam)
    model = {'type': 'm', 'z': np.ones(N, dtype=np.int64), 'R_desc': np.ascontiguousarray(x.T),
             'R_d_desc_alpha': orc.d_desc_dot_vec(gd, alphas.reshape(M, -1)), 'sig': sig, 'std': float(std), 'c': 0.0,
             'perms': perms, 'tril_perms_lin': lin}
    _, F0 = mr.force_fn(model)(starts)
    fmax = 1e-3 * np.sqrt((F0.reshape(7, N, 3) ** 2).sum(-1)).max()
    starts.setflags(write=False)
    return model, starts, d0, float(fmax)


def pair_distances(R):
    r = np.asarray(R).reshape(len(R), -1, 3)
    i, j = orc.tril_pairs(r.shape[1])
    return np.sqrt(((r[:, i] - r[:, j]) ** 2).sum(-1))


# parameter sets the GPU tests run on the toy model: 'clip' clips steps, 'free' never does
TOY_PARAMS = {'clip': dict(dt_start=0.3, max_step=0.02), 'free': dict(dt_start=0.1, max_step=0.2)}

# largest |eigenvalue| of the six lowest modes of the Hessian at a relaxed toy geometry over the seventh, as measured on the
# restatement (tests/test_relax_cpu.py asserts it; the GPU test allows ten times as much).  The rotations are no null modes
# at a finite residual force.
TOY_NULL_RATIO = 6e-3

# step-by-step parity on the fixtures: fmax so small that nothing converges; time steps five times those of the MD tests,
# the step cap a tenth of the default so that steps are clipped once dt has grown
PARITY = dict(fmax=1e-12, max_step=0.02)


def parity_params(name):
    return dict(PARITY, dt_start=5.0 * mr.DT[name])


def parity_state(name, B, n3):
    """A start in mid-run -- seeded velocities, one step taken -- so that the first evaluation already takes the branch on
    the sign of g.v (about half the replicas start with a negative-power event)."""
    st = fresh_state(B, n3, parity_params(name)['dt_start'])
    st['V'] = mr.start_velocities(B, n3, mr.V_SCALE[name])
    st['n_taken'][:] = 1
    return st


@functools.lru_cache(maxsize=None)
def parity_reference(name, n_eval):
    """Restated run of the fixture's seven starts (n_eval evaluations) and its sensitivity to the predictor's agreed error:
    the deviation of a second restated run whose forces carry independent noise of 1e-10 max|F| (the scheme of
    test_md_gpu._reference).  Computed once per session, only read."""
    model, R7 = mr.case(name)
    R0 = np.ascontiguousarray(R7[np.arange(7) % len(R7)])
    st = parity_state(name, 7, R0.shape[1])
    kw = dict(max_steps=n_eval - 1, state=st, **parity_params(name))
    clean = run(mr.force_fn(model), R0, **kw)
    noisy = run(mr.force_fn(model, rel_noise=1e-10, seed=1), R0, **kw)
    return model, R0, st, clean, _deviation(clean, noisy)


@functools.lru_cache(maxsize=None)
def toy_reference(key):
    """The same for the toy model run to convergence with TOY_PARAMS[key]."""
    model, starts, _, fmax = toy()
    kw = dict(max_steps=200, **TOY_PARAMS[key])
    clean = run(mr.force_fn(model), starts, fmax, **kw)
    noisy = run(mr.force_fn(model, rel_noise=1e-10, seed=1), starts, fmax, **kw)
    return clean, _deviation(clean, noisy)


def _deviation(clean, noisy):
    dev = {'V_end': np.abs(clean['state']['V'] - noisy['state']['V']).max()}
    for k in ('R', 'R_end', 'E_hist', 'fmax_hist'):
        dev[k] = np.abs(clean[k] - noisy[k]).max() if clean[k].shape == noisy[k].shape else np.inf
    for o in (clean, noisy):
        for a in o.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return dev

"""NumPy restatement of the on-device nudged elastic band (gdml_neb_run, csrc/neb.hip; GDMLPredict.neb) around a force
callback, the margins of its decisions, and a toy model with a barrier.

The step (the contract; include/gdml_hip.h and csrc/neb.hip state the same).  g = f_unit * F, F the forces of predict(); E the
energies of predict() (they enter through comparisons and the ratio of two differences only, so their scale and offset do not
matter).  A band is ONE FIRE system: state v, dt, alpha, n_pos, n_taken per band.  Images 0 and P - 1 never move.  Evaluation
t = 0, 1, ... of an active band:
  1. E, F = predictor of all P images (the end points' are computed and not used for motion)
  2. for every interior image i, tau+ = r_{i+1} - r_i, tau- = r_i - r_{i-1} (plain differences):
       E_{i+1} > E_i > E_{i-1}: tau = tau+;   E_{i+1} < E_i < E_{i-1}: tau = tau-;   otherwise, with dE_max, dE_min the larger and
       the smaller of |E_{i+1} - E_i|, |E_{i-1} - E_i|: tau = tau+ dE_max + tau- dE_min if E_{i+1} > E_{i-1}, else
       tau = tau+ dE_min + tau- dE_max;   tau^ = tau / |tau|
       F_i = g_i - (g_i . tau^) tau^ + k (|tau+| - |tau-|) tau^
       climb: the interior image of highest E (ties: the lowest index; chosen anew at every evaluation) gets
       F_i = g_i - 2 (g_i . tau^) tau^ instead
  3. f_atom = max over interior images and atoms |F_{i,atom}|;  f_atom < fmax: converged;  else t = max_steps: stops unconverged;
     a frozen band is never written again
  4. else relax's update 4 (tests/_relax_ref.py) on the band vector of (P - 2) 3N coordinates with F in place of g
"""
import functools

import numpy as np

import _md_ref as mr
import _relax_ref as rr
from oracle import gdml_oracle as orc


def fresh_state(B, P, n3, dt_start=0.1, alpha_start=0.1):
    return dict(V=np.zeros((B, P, n3)), dt=np.full(B, float(dt_start)), alpha=np.full(B, float(alpha_start)),
                n_pos=np.zeros(B, dtype=np.int64), n_taken=np.zeros(B, dtype=np.int64))


def highest(E):
    """The interior image of highest energy, ties to the lowest index."""
    return 1 + int(np.argmax(E[1:-1]))


def band_force(r, E, g, k_spring, climb):
    """Step 2 for one band: r, g (P,3N), E (P,).  Returns F (P,3N; zero rows at the ends), g . tau^ (P,; 0 at the ends)."""
    P = len(r)
    F, ftan = np.zeros_like(r), np.zeros(P)
    ic = highest(E)
    for i in range(1, P - 1):
        tp, tm = r[i + 1] - r[i], r[i] - r[i - 1]
        if E[i + 1] > E[i] > E[i - 1]:
            tau = tp
        elif E[i + 1] < E[i] < E[i - 1]:
            tau = tm
        else:
            dp, dm = abs(E[i + 1] - E[i]), abs(E[i - 1] - E[i])
            d_max, d_min = max(dp, dm), min(dp, dm)
            tau = tp * d_max + tm * d_min if E[i + 1] > E[i - 1] else tp * d_min + tm * d_max
        len_t = np.sqrt(np.sum(tau * tau))
        dot = np.sum(g[i] * tau) / len_t
        ftan[i] = dot
        if climb and i == ic:
            F[i] = g[i] + (-2.0 * dot / len_t) * tau
        else:
            len_p, len_m = np.sqrt(np.sum(tp * tp)), np.sqrt(np.sum(tm * tm))
            F[i] = g[i] + ((k_spring * (len_p - len_m) - dot) / len_t) * tau
    return F, ftan


def energy_gap(E, climb):
    """Smallest gap of the energy comparisons of step 2: neighbouring images, and with climb the highest interior image against
    the second highest."""
    gap = np.abs(np.diff(E)).min()
    if climb and len(E) > 3:
        top = np.sort(E[1:-1])
        gap = min(gap, top[-1] - top[-2])
    return gap


def run(force_fn, R_path, fmax, k_spring, climb=False, max_steps=1000, dt_start=0.1, dt_max=None, max_step=0.2, n_min=5,
        f_inc=1.1, f_dec=0.5, alpha_start=0.1, f_alpha=0.99, state=None, f_unit=1.0, e_offset=0.0):
    """force_fn(R (B P,3N)) -> (E, F) scaled as predict() scales them, called with all B P images at every evaluation.
    Returns a dict like GDMLPredict.neb's with R frames of every evaluation, and per band: 'neg_at' (evaluations with a
    negative-power event), 'climb_at' (i_climb of every evaluation the band made), 'power_margin', 'fmax_margin' (as
    _relax_ref.run) and 'gap_margin' (smallest energy_gap / max|E - e_offset| over the evaluations; e_offset: the model's c)."""
    R = np.array(R_path, dtype=np.float64)
    R = R[None] if R.ndim == 2 else R
    B, P, n3 = R.shape
    nv = (P - 2) * n3
    if dt_max is None:
        dt_max = 10.0 * dt_start
    st = fresh_state(B, P, n3, dt_start, alpha_start) if state is None else {k: np.array(v) for k, v in state.items()}
    V, dt, alpha, n_pos, n_taken = st['V'], st['dt'], st['alpha'], st['n_pos'], st['n_taken']
    V[:, 0], V[:, -1] = 0.0, 0.0
    active = np.ones(B, dtype=bool)
    conv = np.zeros(B, dtype=bool)
    n_steps = np.full(B, -1, dtype=np.int64)
    E_end, F_end, f_end, Emax = np.zeros((B, P)), np.zeros((B, P, n3)), np.zeros(B), np.zeros(B)
    i_climb = np.zeros(B, dtype=np.int64)
    s, f_tan = np.zeros((B, P)), np.zeros((B, P))
    hist = {k: [] for k in ('E', 'f', 'R')}
    neg_at, climb_at = [[] for _ in range(B)], [[] for _ in range(B)]
    pm, fm, gm = np.full(B, np.inf), np.full(B, np.inf), np.full(B, np.inf)
    for t in range(max_steps + 1):
        if not active.any():
            break
        E, F = force_fn(R.reshape(B * P, n3))
        E, F = E.reshape(B, P), F.reshape(B, P, n3)
        hist['R'].append(R.copy())
        for b in np.nonzero(active)[0]:
            Fb, ftan = band_force(R[b], E[b], f_unit * F[b], k_spring, climb)
            ic = highest(E[b])
            f_atom = np.sqrt((Fb[1:-1].reshape(-1, 3) ** 2).sum(axis=1)).max()
            E_end[b], F_end[b], f_end[b], Emax[b], i_climb[b], f_tan[b] = E[b], F[b], f_atom, E[b, ic], ic, ftan
            s[b, 1:] = np.cumsum(np.sqrt(((R[b, 1:] - R[b, :-1]) ** 2).sum(axis=1)))
            climb_at[b].append(ic)
            fm[b] = min(fm[b], abs(f_atom - fmax) / fmax)
            gm[b] = min(gm[b], energy_gap(E[b], climb) / np.abs(E[b] - e_offset).max())
            if f_atom < fmax or t == max_steps:
                active[b], conv[b], n_steps[b] = False, f_atom < fmax, t
                continue
            g, v = Fb[1:-1].reshape(nv), V[b, 1:-1].reshape(nv)
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
                    v = np.zeros(nv)
                    alpha[b] = alpha_start
                    dt[b] = dt[b] * f_dec
                    n_pos[b] = 0
                    neg_at[b].append(t)
            v = v + dt[b] * g
            d = dt[b] * v
            d_nrm = np.sqrt(np.sum(d * d))
            if d_nrm > max_step:
                d = d * (max_step / d_nrm)
            V[b, 1:-1] = v.reshape(P - 2, n3)
            R[b, 1:-1] = R[b, 1:-1] + d.reshape(P - 2, n3)
            n_taken[b] += 1
        hist['E'].append(Emax.copy())
        hist['f'].append(f_end.copy())
    top = E_end[np.arange(B), i_climb]
    return dict(R_end=R, E_end=E_end, F_end=F_end, fmax_end=f_end, n_steps=n_steps, converged=conv, i_climb=i_climb,
                barrier=np.stack([top - E_end[:, 0], top - E_end[:, -1]], axis=1), s=s, f_tangent=f_tan,
                Emax_hist=np.array(hist['E']), fmax_hist=np.array(hist['f']), R=np.array(hist['R']),
                state=dict(V=V, dt=dt, alpha=alpha, n_pos=n_pos, n_taken=n_taken), neg_at=neg_at, climb_at=climb_at,
                power_margin=pm, fmax_margin=fm, gap_margin=gm)


def force_fn(model, rel_noise=0.0, seed=0):
    """_md_ref.force_fn with, for rel_noise > 0, independent normal noise of rel_noise * max|E - c| on every energy as well:
    the tangent depends on E."""
    inner = mr.force_fn(model, rel_noise=rel_noise, seed=seed)
    rs = np.random.RandomState(seed + 1000)
    c = float(model['c'])

    def fn(R):
        E, F = inner(R)
        if rel_noise:
            E = E + rel_noise * np.abs(E - c).max() * rs.standard_normal(E.shape)
        return E, F

    return fn


def _deviation(clean, noisy):
    dev = {'V_end': np.abs(clean['state']['V'] - noisy['state']['V']).max()}
    for k in ('R', 'R_end', 'Emax_hist', 'fmax_hist', 'barrier', 's', 'f_tangent'):
        dev[k] = np.abs(clean[k] - noisy[k]).max() if clean[k].shape == noisy[k].shape else np.inf
    for o in (clean, noisy):
        for a in list(o.values()) + list(o['state'].values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return dev


def interpolate(R_a, R_b, P):
    t = (np.arange(P) / (P - 1.0))[None, :, None]
    path = R_a[:, None, :] + t * (R_b - R_a)[:, None, :]
    path[:, 0], path[:, -1] = R_a, R_b
    return path


# ---- step-by-step parity on the fixtures

# spring constant and jitter of the interior images of the parity bands
PARITY_K, PARITY_JITTER = 1.0, 0.01

# (fixture, P, B): P = 3 one interior image (also the climbing one); P = 16 / 17 on n6_p1: (P - 2) 3N = 252 / 270 coordinates, just
# under / over the 256-thread stride; n100_m3: 300 coordinates per image
PARITY_CASES = [('n6_p1', 3, 1), ('n6_p1', 4, 3), ('n6_p1', 7, 1), ('n6_p1', 7, 3), ('n6_p1', 16, 1), ('n6_p1', 17, 1),
                ('n5_p4', 3, 3), ('n5_p4', 7, 1), ('n10_p2_pbc', 4, 1), ('n10_p2_pbc', 7, 3), ('cfg1_n21_m100', 4, 3),
                ('cfg1_n21_m100', 7, 1), ('cfg3_n42_p27_m60', 4, 1), ('n100_m3', 3, 1), ('n100_m3', 4, 3)]
PARITY_N_EVAL = {'cfg3_n42_p27_m60': 5}  # (its restated forces take a third of a second per call)


def parity_band(name, P, B):
    """Band b = the interpolation between the fixture's starts b and b + 1 plus seeded jitter on the interior images; a start
    state in mid-run as _relax_ref.parity_state (seeded velocities, one step taken)."""
    model, R7 = mr.case(name)
    n3 = R7.shape[1]
    idx = np.arange(B + 1) % len(R7)
    path = interpolate(R7[idx[:-1]], R7[idx[1:]], P)
    path[:, 1:-1] += PARITY_JITTER * np.random.RandomState(11).standard_normal((B, P - 2, n3))
    st = fresh_state(B, P, n3, rr.parity_params(name)['dt_start'])
    st['V'] = mr.start_velocities(B * P, n3, mr.V_SCALE[name]).reshape(B, P, n3)
    st['V'][:, 0], st['V'][:, -1] = 0.0, 0.0
    st['n_taken'][:] = 1
    return model, path, st


@functools.lru_cache(maxsize=None)
def parity_reference(name, P, B, climb):
    """Restated run of a parity band (30 evaluations, 5 for the largest fixture; nothing converges) and its sensitivity to the
    predictor's agreed error: the deviation of a second restated run with independent force noise of 1e-10 max|F| and energy
    noise of 1e-10 max|E'|.  Computed once per session, only read."""
    model, path, st = parity_band(name, P, B)
    n_eval = PARITY_N_EVAL.get(name, 30)
    kw = dict(k_spring=PARITY_K, climb=climb, max_steps=n_eval - 1, state=st, e_offset=float(model['c']), **rr.parity_params(name))
    clean = run(force_fn(model), path, **kw)
    noisy = run(force_fn(model, rel_noise=1e-10, seed=1), path, **kw)
    path.setflags(write=False)
    return model, path, st, clean, _deviation(clean, noisy)


# ---- a toy with a barrier

TOY_SEED = 1


@functools.lru_cache(maxsize=None)
def toy(seed=TOY_SEED):
    """(model, minimum A (15,), minimum B (15,), fmax).  sGDML's descriptor holds pair distances only, so every model is exactly
    mirror-symmetric: a non-planar minimum has a twin, with a saddle between them.  Five atoms: four on a square of side 1.5
    with z = +-0.35 alternating, a fifth at the centre with z = 0.1, 0.05 normal jitter; unit springs on the 10 pair distances
    (_relax_ref._springs); M = 150 training geometries on the line between the geometry and its mirror image (z -> -z), t in
    [-0.15, 1.15], with 0.1 normal jitter; sigma = 1, lambda = 1e-10, one permutation, c = 0, RandomState(TOY_SEED); trained with the
    oracle on the CPU (n = 2250).  Both minima are the FIRE restatement's (fmax_relax below); fmax = 1e-3 of the largest atomic
    force on the line between them."""
    rs = np.random.RandomState(seed)
    N, M, sig, lam = 5, 150, 1.0, 1e-10
    base = np.array([[0.0, 0.0, 0.35], [1.5, 0.0, -0.35], [1.5, 1.5, 0.35], [0.0, 1.5, -0.35], [0.75, 0.75, 0.1]])
    base = base + 0.05 * rs.standard_normal((N, 3))
    mirror = base * np.array([1.0, 1.0, -1.0])
    i, j = orc.tril_pairs(N)
    d0 = np.sqrt(((base[i] - base[j]) ** 2).sum(-1))
    t = rs.uniform(-0.15, 1.15, M)[:, None, None]
    R_train = base[None] + t * (mirror - base)[None] + 0.1 * rs.standard_normal((M, N, 3))
    _, F_train = rr._springs(R_train, d0)
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
    fn = mr.force_fn(model)
    ends = np.stack([base.ravel(), mirror.ravel()])
    _, F0 = fn(ends)
    f_relax = 1e-6 * np.sqrt((F0.reshape(2, N, 3) ** 2).sum(-1)).max()
    ends = rr.run(fn, ends, max(f_relax, 1e-9), max_steps=2000)
    assert ends['converged'].all()
    A, Bm = ends['R_end']
    _, F_line = fn(interpolate(A[None], Bm[None], 33)[0])
    fmax = 1e-3 * np.sqrt((F_line.reshape(33, N, 3) ** 2).sum(-1)).max()
    A.setflags(write=False)
    Bm.setflags(write=False)
    return model, A, Bm, float(fmax)


# As measured on the restatement (tests/test_neb_cpu.py prints and asserts them): the barrier of every toy run (0.0476037 ...
# 0.0476058 over the runs; fmax leaves the climbing image that far from the saddle); at the climbing image the one negative
# Hessian eigenvalue and the first positive one; the largest |eigenvalue| of the six null modes over the first positive one
# (3.3e-3 measured; the GPU test allows ten times the constant; the rotations are no null modes at a finite residual force).
TOY_BARRIER = 0.047605
TOY_SADDLE_MODES = (-0.262, 0.087)
TOY_NULL_RATIO = 4e-3

TOY_K = 0.5
TOY_JITTER = 0.02
TOY_MAX_STEPS = 400

# the runs to convergence: key -> (P, climb, seeds of the bands' jitter); several bands of a key freeze at different evaluations.
# Measured on the restatement (tests/test_neb_cpu.py prints them): steps to converge p3 80, p4 75, p8 125, p4_x3 75 / 81 / 86,
# p8_x3 125 / 80 / 75, p3_plain 80 / 68; smallest compared energy gap over a whole run, in units of max|E'|: P = 3 2.0e-2 (with
# and without climbing), P = 4 5.4e-4 ... 2.5e-3, P = 8 7.0e-5 ... 7.4e-4; smallest |F.v| / (|F||v|) 4.2e-3, smallest
# |f_atom - fmax| / fmax 7.1e-3.  In the P = 8 band of seed 1 the climbing image changes at evaluation 7 and the first
# negative-power event is at evaluation 8: the cut of the continuation tests (10) lies behind both.
TOY_RUNS = {'p3': (3, True, (1,)), 'p4': (4, True, (1,)), 'p8': (8, True, (1,)), 'p4_x3': (4, True, (1, 2, 3)),
            'p8_x3': (8, True, (1, 2, 5)), 'p3_plain': (3, False, (1, 2))}


def toy_bands(key):
    """The start of a toy run: per seed, the line between the two minima with TOY_JITTER normal jitter on the interior images
    (the middle image of an unjittered line with an odd P lies on the planar configuration, a stationary point by symmetry
    which need not be the saddle: the start always breaks the symmetry)."""
    _, A, Bm, _ = toy()
    P, climb, seeds = TOY_RUNS[key]
    path = np.repeat(interpolate(A[None], Bm[None], P), len(seeds), axis=0)
    for b, seed in enumerate(seeds):
        path[b, 1:-1] += TOY_JITTER * np.random.RandomState(seed).standard_normal((P - 2, path.shape[2]))
    return path, climb


@functools.lru_cache(maxsize=None)
def toy_reference(key):
    """Restated run of a toy case to convergence, and its deviation under force and energy noise of 1e-10."""
    model, _, _, fmax = toy()
    path, climb = toy_bands(key)
    kw = dict(k_spring=TOY_K, climb=climb, max_steps=TOY_MAX_STEPS)
    clean = run(force_fn(model), path, fmax, **kw)
    noisy = run(force_fn(model, rel_noise=1e-10, seed=1), path, fmax, **kw)
    path.setflags(write=False)
    return path, clean, _deviation(clean, noisy)

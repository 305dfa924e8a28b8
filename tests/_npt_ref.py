"""NumPy restatement of the on-device constant-pressure dynamics (gdml_npt_run, csrc/npt.hip; GDMLPredict.run_npt): isotropic
Martyna-Tobias-Klein equations, NPH or with a Langevin thermostat on the particles and on the piston, on top of the restated
noise (_md_ref.normals), the restated virial (_cellrelax_ref.model_virial_fn) and the periodic toy (_cellrelax_ref.toy).

The contract (include/gdml_hip.h states the same).  Per replica: masses m, N_f = 3N, kappa = 1 + 3/N_f; f = f_unit F and
Wv = f_unit W (F, W as predict_virial() returns them); K = sum m v^2 / 2; reference lattice L0, V0 = |det L0|; state
(r, v, eps, p_eps); lambda = exp(eps), L = lambda L0, L^-1 = L0^-1 / lambda, Vol = lambda^3 V0; piston mass Wp (inf allowed:
alpha is exactly 0), alpha = p_eps / Wp;  G_eps = kappa 2K - tr Wv - 3 P_ext Vol.
Step t (step = step0 + t):
  1. p_eps += dt/2 G_eps  (K, tr Wv, Vol of the current state)
  2. alpha = p_eps / Wp, s = exp(-kappa alpha dt/4):  v = s v;  v += dt/2 f/m;  v = s v
  3. no thermostat:  q = exp(alpha dt/2):  r = q r;  r += dt v;  r = q r;  eps += alpha dt
     Langevin:       q = exp(alpha dt/4):  r = q r;  r += dt/2 v;  r = q r;  eps += alpha dt/2
                     v = c1 v + c2 sqrt(kT/m) xi_k;  p_eps = b1 p_eps + b2 sqrt(Wp kT) xi_3N;  alpha = p_eps / Wp
                     the same half drift with the new alpha
                     c1 = exp(-gamma dt), c2 = sqrt(1 - c1^2), b1 = exp(-gamma_baro dt), b2 = sqrt(1 - b1^2); xi = the stream of
                     run_md at (seed, step, replica, coordinate), the piston being coordinate 3N; Wp = inf: no piston noise
  4. E, F, W = predictor with virial for (r, L)
  5. s = exp(-kappa alpha dt/4) with the current alpha:  v = s v;  v += dt/2 f/m;  v = s v
  6. K;  p_eps += dt/2 G_eps
NPH conserves H = K + f_unit E + P_ext Vol + p_eps^2 / (2 Wp).
"""
import functools

import numpy as np

import _cellrelax_ref as cr
import _md_ref as mr

SCALARS = ('E_pot', 'E_kin', 'vol', 'pressure', 'p_eps', 'enthalpy')


def det3(M):
    return cr.adj_det(M)[1]


def cell(eps, L0, L0_inv, V0):
    """lambda = exp(eps): (L (B,3,3), L^-1, Vol (B,))."""
    lam = np.exp(eps)
    return lam[:, None, None] * L0, L0_inv / lam[:, None, None], lam * lam * lam * V0


def g_eps(kappa, K, W, vol, pressure, f_unit=1.0):
    return kappa * (2.0 * K) - f_unit * (W[:, 0, 0] + W[:, 1, 1] + W[:, 2, 2]) - 3.0 * pressure * vol


def run(virial_fn, R0, V0, masses, L0, dt, n_steps, pressure, piston_mass, record_every=1, thermostat=None, gamma=0.0,
        gamma_baro=0.0, kT=0.0, seed=0, step0=0, eps0=None, p_eps0=None, f_unit=1.0, kappa=None):
    """The integrator.  virial_fn(R (B,3N), lattices (B,3,3)) -> (E, F, W) scaled as predict_virial() scales them; L0 (B,3,3) or
    (3,3).  Returns a dict like GDMLPredict.run_npt's with every field recorded, and 'G_eps' (n_rec,B) after step 6.
    kappa: for tests that need a WRONG generalised force (default 1 + 3/N_f)."""
    R = np.array(R0, dtype=np.float64).reshape(-1, np.shape(R0)[-1])
    V = np.array(V0, dtype=np.float64).reshape(R.shape)
    B, n3 = R.shape
    L0 = np.array(np.broadcast_to(np.asarray(L0, dtype=np.float64), (B, 3, 3)))
    L0_inv = np.array([cr.inv3(L) for L in L0])
    vol0 = np.abs(np.array([det3(L) for L in L0]))
    m = np.repeat(np.asarray(masses, dtype=np.float64), 3)[None, :]
    eps = np.zeros(B) if eps0 is None else np.array(eps0, dtype=np.float64).reshape(B)
    p_eps = np.zeros(B) if p_eps0 is None else np.array(p_eps0, dtype=np.float64).reshape(B)
    Wp = float(piston_mass)
    kap = 1.0 + 3.0 / n3 if kappa is None else float(kappa)
    c1 = np.exp(-gamma * dt)
    c2 = np.sqrt(1.0 - c1 * c1)
    b1 = np.exp(-gamma_baro * dt)
    b2 = np.sqrt(1.0 - b1 * b1)
    col = lambda a: a[:, None]  # noqa: E731

    def kick(V, F, alpha):  # steps 2 and 5
        s = col(np.exp(-kap * alpha * dt / 4.0))
        V = s * V
        V = V + 0.5 * dt * (f_unit * F / m)
        return s * V

    def drift(R, V, eps, alpha, h):  # the exact flow of r' = alpha r + v over h at fixed v and alpha
        q = col(np.exp(alpha * h / 2.0))
        R = q * R
        R = R + h * V
        return q * R, eps + alpha * h

    ekin = lambda V: (0.5 * m * V * V).sum(axis=1)  # noqa: E731
    L, Li, vol = cell(eps, L0, L0_inv, vol0)
    E, F, W = virial_fn(R, L)
    K = ekin(V)
    out = {k: [] for k in ('R', 'V', 'F', 'lattice', 'G_eps') + SCALARS}
    for t in range(n_steps):
        p_eps = p_eps + 0.5 * dt * g_eps(kap, K, W, vol, pressure, f_unit)
        alpha = p_eps / Wp
        V = kick(V, F, alpha)
        if thermostat is None:
            R, eps = drift(R, V, eps, alpha, dt)
        else:
            R, eps = drift(R, V, eps, alpha, 0.5 * dt)
            xi = mr.normals(seed, step0 + t, B, n3 + 1)
            V = c1 * V + c2 * np.sqrt(kT / m) * xi[:, :n3]
            if np.isfinite(Wp):
                p_eps = b1 * p_eps + b2 * np.sqrt(Wp * kT) * xi[:, n3]
            alpha = p_eps / Wp
            R, eps = drift(R, V, eps, alpha, 0.5 * dt)
        L, Li, vol = cell(eps, L0, L0_inv, vol0)
        E, F, W = virial_fn(R, L)
        V = kick(V, F, alpha)
        K = ekin(V)
        G = g_eps(kap, K, W, vol, pressure, f_unit)
        p_eps = p_eps + 0.5 * dt * G
        if (t + 1) % record_every == 0:
            trW = f_unit * (W[:, 0, 0] + W[:, 1, 1] + W[:, 2, 2])
            H = K + f_unit * E + pressure * vol + p_eps * p_eps / (2.0 * Wp)
            for k, v in (('R', R), ('V', V), ('F', F), ('lattice', L), ('G_eps', G), ('E_pot', E), ('E_kin', K), ('vol', vol),
                         ('pressure', (2.0 * K - trW) / (3.0 * vol)), ('p_eps', p_eps), ('enthalpy', H)):
                out[k].append(np.array(v))
    tail = {'R': (n3,), 'V': (n3,), 'F': (n3,), 'lattice': (3, 3)}
    out = {k: np.array(v).reshape((len(v), B) + tail.get(k, ())) for k, v in out.items()}
    out.update(R_end=R, V_end=V, lattice_end=L, vol_end=vol, step_end=step0 + n_steps,
               state=dict(eps=eps, p_eps=p_eps, L0=L0))
    return out


def enthalpy_start(virial_fn, R0, V0, masses, L0, pressure, piston_mass, eps0=None, p_eps0=None, f_unit=1.0):
    """H of a start state (B,)."""
    R = np.asarray(R0, dtype=np.float64).reshape(-1, np.shape(R0)[-1])
    B = len(R)
    L0 = np.broadcast_to(np.asarray(L0, dtype=np.float64), (B, 3, 3))
    eps = np.zeros(B) if eps0 is None else np.asarray(eps0, dtype=np.float64)
    p_eps = np.zeros(B) if p_eps0 is None else np.asarray(p_eps0, dtype=np.float64)
    L, _, vol = cell(eps, L0, 1.0, np.abs(np.array([det3(x) for x in L0])))
    m = np.repeat(np.asarray(masses, dtype=np.float64), 3)[None, :]
    K = (0.5 * m * np.reshape(V0, R.shape) ** 2).sum(axis=1)
    return K + f_unit * virial_fn(R, L)[0] + pressure * vol + p_eps ** 2 / (2.0 * float(piston_mass))


def springs_batch_fn(d0):
    """_cellrelax_ref.springs_virial_fn(d0) for all geometries at once (the ensemble test takes 64 x 6000 evaluations): the same
    potential, minimum image by rint(L^-1 d) as there; tests/test_npt_cpu.py compares the two."""
    d0 = np.asarray(d0, dtype=np.float64)

    def fn(R, lats):
        R, lats = np.asarray(R, dtype=np.float64), np.asarray(lats, dtype=np.float64)
        M = len(R)
        r = R.reshape(M, -1, 3)
        N = r.shape[1]
        i, j = cr.orc.tril_pairs(N)
        d = r[:, i, :] - r[:, j, :]
        inv = np.linalg.inv(lats)
        d = d - np.einsum('mab,mdb->mda', lats, np.around(np.einsum('mab,mdb->mda', inv, d)))
        dist = np.sqrt((d ** 2).sum(-1))
        E = 0.5 * ((dist - d0) ** 2).sum(axis=1)
        pair = -((dist - d0) / dist)[:, :, None] * d
        F = np.zeros((M, N, 3))
        for k in range(len(i)):
            F[:, i[k]] += pair[:, k]
            F[:, j[k]] -= pair[:, k]
        W = -np.einsum('mka,mkc->mac', pair, d)
        return E, F.reshape(M, -1), W

    return fn


# ---- the ensemble identities (tests/test_npt_cpu.py on the springs, tests/test_npt_gpu.py on the toy model)

ENSEMBLE = dict(kT=0.002, piston_mass=20.0, gamma=0.2, gamma_baro=0.2, dt=0.1, seed=11)


def identities(E_kin, p_eps, G, n3, kT, Wp):
    """The three identities from scalar frames (n,B): per identity (mean over replicas of the per-replica time averages minus
    the expected value, standard error from the scatter of the replica means)."""
    out = {}
    for name, series, want in (('G_eps', G, 0.0), ('2K/3N', 2.0 * E_kin / n3, kT), ('p_eps^2/Wp', p_eps * p_eps / Wp, kT)):
        means = series.mean(axis=0)
        out[name] = (float(means.mean() - want), float(means.std(ddof=1) / np.sqrt(len(means))))
    return out


def g_from_frames(E_kin, pressure_int, vol, pressure, kappa):
    """G_eps = kappa 2K - tr Wv - 3 P_ext Vol from recorded frames: tr Wv = 2K - 3 Vol P_int."""
    return kappa * 2.0 * E_kin - (2.0 * E_kin - 3.0 * vol * pressure_int) - 3.0 * pressure * vol


# ---- step-by-step parity on the periodic fixtures (tests/test_npt_gpu.py, tools/npt_parity.py)

PARITY_FIXTURES = ('n4_p6_pbc', 'n10_p2_pbc')
PARITY_BATCHES = (1, 7)
PARITY_STEPS = 30
PARITY_PRESSURE = 0.01
# n4_p6_pbc has no entry in _md_ref.DT: it gets the step and velocity scale of that table's other small fixtures (30 steps move
# an atom by 0.12 at most, 5 % of the shortest pair distance of its starts)
PARITY_DT = {'n4_p6_pbc': 0.02, 'n10_p2_pbc': mr.DT['n10_p2_pbc']}
PARITY_V = {'n4_p6_pbc': 0.2, 'n10_p2_pbc': mr.V_SCALE['n10_p2_pbc']}
# Piston: alpha0 = p_eps0 / Wp is chosen so that the start rate alone changes the volume by 0.9 % over the 30 steps (3 alpha0
# 30 dt = 0.009) and Wp so large that G_eps changes alpha by little over them: the test asserts 0.1 % .. 2 % for every replica.
PARITY_DVOL = 0.009
PARITY_LANGEVIN = dict(gamma=0.5, gamma_baro=0.5, seed=7)
PARITY_KEYS = ('R', 'V', 'lattice', 'E_pot', 'E_kin', 'vol', 'pressure', 'p_eps', 'eps_end')
PLUS_PREDICTOR = ('E_pot', 'vol', 'pressure', 'enthalpy')  # keys allowed the predictor's agreed 1e-10 of the largest value
BOUND_FACTOR = cr.BOUND_FACTOR


@functools.lru_cache(maxsize=None)
def parity_case(name):
    """(model, kw) of a periodic fixture: seven starts, masses 1 + 0.5 (i mod 3), distinct eps0 of order 1e-2, nonzero p_eps0."""
    model, R7 = mr.case(name)
    R0 = np.ascontiguousarray(R7[np.arange(7) % len(R7)])
    n3 = R0.shape[1]
    N = n3 // 3
    masses = 1.0 + 0.5 * (np.arange(N) % 3)
    dt = PARITY_DT[name]
    eps0 = 0.01 * np.array([1.0, -0.8, 0.6, -0.4, 0.3, 1.2, -1.1])
    alpha0 = PARITY_DVOL / (3.0 * PARITY_STEPS * dt) * np.array([1.0, -1.0, 1.1, -0.9, 0.8, -1.2, 0.9])
    L0 = np.asarray(model['lattice'], dtype=np.float64)
    # r and L0 are strained together at the start: the replica's atoms sit in the cell exp(eps0) L0
    R0 = R0 * np.exp(eps0)[:, None]
    V0 = mr.start_velocities(7, n3, PARITY_V[name])
    kT = float((V0 * V0 * np.repeat(masses, 3)[None]).mean())
    # the piston's period of (3N + 3) kT tau^2 with tau = 100 steps, at least so heavy that 30 steps of the start's G_eps change
    # alpha by a quarter of alpha0 at most (worked out from the restated G_eps of the start below)
    fn = cr.model_virial_fn(model)
    L, _, vol = cell(eps0, np.broadcast_to(L0, (7, 3, 3)), 1.0, np.abs(det3(L0)))
    E, F, W = fn(R0, L)
    K = (0.5 * np.repeat(masses, 3)[None] * V0 * V0).sum(axis=1)
    G = g_eps(1.0 + 3.0 / n3, K, W, vol, PARITY_PRESSURE)
    Wp = max((n3 + 3) * kT * (100 * dt) ** 2, float((np.abs(G) * PARITY_STEPS * dt / (0.25 * np.abs(alpha0))).max()))
    kw = dict(R0=R0, V0=V0, masses=masses, dt=dt, n_steps=PARITY_STEPS, pressure=PARITY_PRESSURE, piston_mass=Wp,
              eps0=eps0, p_eps0=alpha0 * Wp, kT=kT, L0=L0)
    for a in kw.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return model, kw


def _ref_kw(kw, mode):
    kw = dict(kw)
    if mode == 'npt':
        kw.update(thermostat='langevin', **PARITY_LANGEVIN)
    return kw


@functools.lru_cache(maxsize=None)
def parity_reference(name, mode):
    """Restated run of parity_case(name) ('nph' or 'npt') and its sensitivity to the predictor's agreed error: the deviation of a
    second restated run whose E, F and W carry independent noise of 1e-10 relative.  Computed once per session, only read."""
    model, kw = parity_case(name)
    kw = _ref_kw(kw, mode)
    clean = run(cr.model_virial_fn(model), **kw)
    noisy = run(cr.model_virial_fn(model, rel_noise=1e-10, seed=1), **kw)
    dev = {k: float(np.abs(clean[k] - noisy[k]).max()) for k in PARITY_KEYS + ('enthalpy',) if k != 'eps_end'}
    dev['eps_end'] = float(np.abs(clean['state']['eps'] - noisy['state']['eps']).max())
    for o in (clean, noisy):
        for a in list(o.values()) + list(o['state'].values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return model, kw, clean, dev


def volume_change(kw, ref):
    """|Vol_end / Vol_start - 1| of every replica of a restated run started with kw (B,)."""
    vol_start = np.exp(3.0 * kw['eps0']) * np.abs(np.array([det3(L) for L in ref['state']['L0']]))
    return np.abs(ref['vol_end'] / vol_start - 1.0)


def parity_measure(pred, name, mode, B):
    """One parity case on the device: GDMLPredict.run_npt from parity_case(name)'s first B starts, every step recorded, against
    the restated run.  Per compared quantity the error, the restatement's sensitivity, what the test allows (BOUND_FACTOR x
    sensitivity; for E, vol, pressure and enthalpy plus the predictor's agreed 1e-10 of the largest value) and their ratio."""
    model, kw, ref, dev = parity_reference(name, mode)
    call = {k: v for k, v in kw.items() if k not in ('eps0', 'p_eps0', 'L0', 'R0', 'V0')}
    state = dict(eps=kw['eps0'][:B], p_eps=kw['p_eps0'][:B], L0=np.broadcast_to(kw['L0'], (B, 3, 3)))
    out = pred.run_npt(kw['R0'][:B], kw['V0'][:B], state=state, record=('R', 'V', 'F', 'lattice', 'E'), **call)
    got = dict(out, eps_end=out['state']['eps'])
    want = {k: ref[k][:, :B] for k in PARITY_KEYS + ('enthalpy',) if k != 'eps_end'}
    want['eps_end'] = ref['state']['eps'][:B]
    m = {}
    for k in PARITY_KEYS + ('enthalpy',):
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        full = ref['state']['eps'] if k == 'eps_end' else ref[k]
        allowed = BOUND_FACTOR * dev[k] + (1e-10 * np.abs(full).max() if k in PLUS_PREDICTOR else 0.0)
        err = float(np.abs(got[k] - want[k]).max())
        m[k] = dict(error=err, sensitivity=float(dev[k]), allowed=float(allowed), ratio=err / allowed if allowed > 0 else np.inf)
    m['frames_are_the_end'] = bool(np.array_equal(out['R'][-1], out['R_end']) and np.array_equal(out['V'][-1], out['V_end']) and
                                   # (lattice_end is formed on the host from the end eps: exp() may differ in the last bit)
                                   np.abs(out['lattice'][-1] - out['lattice_end']).max() <= 4e-16 * np.abs(out['lattice_end']).max() and
                                   np.array_equal(out['p_eps'][-1], out['state']['p_eps']))
    return m

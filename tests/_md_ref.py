"""NumPy restatement of the on-device integrators (gdml_md_run, csrc/md.hip): velocity Verlet and Langevin BAOAB around a
force callback, and the noise stream (Philox4x32-10 + Box-Muller).  The CPU forces come from the existing restatements."""
import functools
import os

import numpy as np

import _hessian_ref as hr
import _stress_ref as sr
from oracle import gdml_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(key, ctr):
    """key: two uint32 (scalars or arrays), ctr: four uint32 arrays (broadcastable).  Returns the four uint32 outputs."""
    k0, k1 = (np.asarray(k, dtype=np.uint64) & MASK for k in key)
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & MASK for c in ctr])
    for _ in range(10):
        p0 = M0 * c0  # 32 x 32 -> 64 bits, exact in uint64
        p1 = M1 * c2
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & MASK, (p0 >> S32) ^ c3 ^ k1, p0 & MASK
        k0 = (k0 + np.uint64(W0)) & MASK
        k1 = (k1 + np.uint64(W1)) & MASK
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def normals(seed, step, B, n3):
    """xi (B,n3): key = (low, high) half of seed, counter = (step low, step high, replica, block); the block's outputs
    (x0, x1), (x2, x3) are two Box-Muller pairs with u = (x + 0.5) 2^-32, for coordinates 4 block .. 4 block + 3."""
    seed, step = int(seed), int(step)
    nblk = (n3 + 3) // 4
    rep = np.arange(B, dtype=np.uint64)[:, None]
    blk = np.arange(nblk, dtype=np.uint64)[None, :]
    x = philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), (step & 0xFFFFFFFF, (step >> 32) & 0xFFFFFFFF, rep, blk))
    u = [(xi.astype(np.float64) + 0.5) * 2.0**-32 for xi in x]
    out = np.empty((B, nblk, 4))
    for a in (0, 2):
        rad = np.sqrt(-2.0 * np.log(u[a]))
        ang = 6.283185307179586 * u[a + 1]
        out[:, :, a] = rad * np.cos(ang)
        out[:, :, a + 1] = rad * np.sin(ang)
    return out.reshape(B, nblk * 4)[:, :n3]


def run(force_fn, R0, V0, masses, dt, n_steps, record_every=1, thermostat=None, gamma=0.0, kT=0.0, seed=0, step0=0,
        f_unit=1.0):
    """The two integrators.  force_fn(R (B,3N)) -> (E (B,), F (B,3N)), both scaled as predict() scales them.  Returns a dict
    like GDMLPredict.run_md's with every field recorded."""
    R = np.array(R0, dtype=np.float64).reshape(-1, np.shape(R0)[-1])
    V = np.array(V0, dtype=np.float64).reshape(R.shape)
    B, n3 = R.shape
    m = np.repeat(np.asarray(masses, dtype=np.float64), 3)[None, :]
    c1 = np.exp(-gamma * dt)
    c2 = np.sqrt(1.0 - c1 * c1)
    E, F = force_fn(R)
    out = {k: [] for k in ('R', 'V', 'F', 'E_pot', 'E_kin')}
    for t in range(n_steps):
        V = V + 0.5 * dt * (f_unit * F / m)
        if thermostat is None:
            R = R + dt * V
        else:
            R = R + 0.5 * dt * V
            V = c1 * V + c2 * np.sqrt(kT / m) * normals(seed, step0 + t, B, n3)
            R = R + 0.5 * dt * V
        E, F = force_fn(R)
        V = V + 0.5 * dt * (f_unit * F / m)
        if (t + 1) % record_every == 0:
            for k, v in (('R', R), ('V', V), ('F', F), ('E_pot', E), ('E_kin', (0.5 * m * V * V).sum(axis=1))):
                out[k].append(np.array(v))
    out = {k: np.array(v).reshape((len(v), B) + ((n3,) if k in 'RVF' else ())) for k, v in out.items()}
    out.update(R_end=R, V_end=V, step_end=step0 + n_steps)
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """(model, start geometries (up to seven), restated forces at them) of a fixture; read-only."""
    g = dict(np.load(os.path.join(GOLDEN, name + '.npz')))
    model, _, _ = hr.model_from_fixture(g)
    Rt = g['R_test'].reshape(len(g['R_test']), -1)
    R7 = np.concatenate([Rt[:6], g['R_train'][:1].reshape(1, -1)])
    R7.setflags(write=False)
    return model, R7


@functools.lru_cache(maxsize=None)
def synth_n12():
    """(model, seven start geometries) of the synthetic N = 12, M = 150 model of tests/test_hip_r5.py
    (test_single_launch_prediction_aspirin_size): D = 66, two descriptor entries per lane in the single-launch kernels.
    Random J alpha, sig = 20, identity permutation, std = 1, c = 0; read-only."""
    N, M = 12, 150
    ds = orc.synth_dataset(N, M + 7, seed=4, jitter=0.3)
    Rf = ds['R'].reshape(M + 7, -1)
    xo, _ = orc.desc_from_R(Rf[:M])
    JA = np.random.default_rng(1).standard_normal(xo.shape)
    perms = np.arange(N, dtype=np.int64)[None]
    tp = orc.tril_perms_from_atom_perms(perms)
    model = {'type': 'm', 'z': np.ones(N, dtype=np.int64), 'R_desc': np.ascontiguousarray(xo.T), 'R_d_desc_alpha': JA,
             'sig': 20.0, 'std': 1.0, 'c': 0.0, 'perms': perms, 'tril_perms_lin': orc.tril_perms_lin_from_tril_perms(tp)}
    R7 = np.ascontiguousarray(Rf[M:])
    R7.setflags(write=False)
    return model, R7


# Runs on synth_n12() (masses 1): time step and start-velocity scale of the MD runs, first time step and step cap of the
# relaxation.  Over six steps (evaluations) of the restatements (run() here, _relax_ref.run) the shortest pair distance of a
# replica changes by 0.48 % at most (NVE and Langevin) and by 0.21 % (FIRE from rest): below 1 %.
SYNTH_DT, SYNTH_V_SCALE = 0.0005, 0.2
SYNTH_RELAX = dict(dt_start=0.02, max_step=0.01)


def force_fn(model, rel_noise=0.0, seed=0):
    """Restated (E, F) of a model as predict() returns them; rel_noise: every force component perturbed by independent normal
    noise of rel_noise * max|F| (a fresh draw per call)."""
    rs = np.random.RandomState(seed)

    def fn(R):
        E, F, _ = sr.virial_of_model(model, R)
        if rel_noise:
            F = F + rel_noise * np.abs(F).max() * rs.standard_normal(F.shape)
        return E, F

    return fn


def min_pair_distance(model, R):
    d = np.linalg.norm(sr.pair_vectors(R, _lat_and_inv(model)), axis=-1)
    return d.min()


def _lat_and_inv(model):
    if 'lattice' not in model:
        return None
    lat = np.asarray(model['lattice'], dtype=np.float64)
    return lat, np.linalg.inv(lat)


def start_velocities(B, n3, scale, seed=5):
    """Seeded start velocities with zero total momentum per replica (masses 1)."""
    V = scale * np.random.RandomState(seed).standard_normal((B, n3 // 3, 3))
    V -= V.mean(axis=1, keepdims=True)
    return V.reshape(B, n3)


# Time steps and start-velocity scales of the tests (masses 1, f_unit 1).  Chosen so that the largest displacement of a step
# stays below 1 % of the shortest pair distance and the restated velocity-Verlet drift halves its step at second order
# (tests/test_md_cpu.py checks both for the fixtures of the drift test).
DT = {'n6_p1': 0.02, 'n5_p4': 0.02, 'n5_p2_ecstr': 0.02, 'n9_p1': 0.02, 'n10_p2_pbc': 0.002, 'cfg1_n21_m100': 0.004,
      'cfg3_n42_p27_m60': 0.002, 'n100_m3': 0.002}
V_SCALE = {'n6_p1': 0.2, 'n5_p4': 0.2, 'n5_p2_ecstr': 0.2, 'n9_p1': 0.2, 'n10_p2_pbc': 0.3, 'cfg1_n21_m100': 0.3,
           'cfg3_n42_p27_m60': 0.3, 'n100_m3': 0.3}


def drift(force, R0, V0, masses, dt, n_steps):
    """max_t |E_tot(t) - E_tot(0)| of an NVE run and the largest displacement of an atom in one step."""
    E0, _ = force(R0)
    e0 = E0 + (0.5 * np.repeat(masses, 3)[None] * V0 * V0).sum(axis=1)
    tr = run(force, R0, V0, masses, dt, n_steps)
    Rs = np.concatenate([np.asarray(R0)[None], tr['R']])
    step = np.linalg.norm(np.diff(Rs, axis=0).reshape(n_steps, len(Rs[0]), -1, 3), axis=-1)  # per atom
    return np.abs(tr['E_pot'] + tr['E_kin'] - e0[None]).max(), step.max()

"""NumPy restatement of the on-device path-integral integrator (gdml_pimd_run, csrc/pimd.hip; include/gdml_hip.h has the
equations): B rings of P beads, BAOAB with the exact free ring-polymer flow in normal-mode space and the PILE-L thermostat,
around a force callback.  The noise stream, fixtures and restated forces are those of _md_ref."""
import numpy as np

import _md_ref as mr


def modes(P, kT, hbar):
    """C (P,P) with C[j, k] the orthonormal real DFT over the bead index, and omega (P,) = 2 omega_P sin(k pi / P)."""
    j = np.arange(P)[:, None]
    k = np.arange(P)[None, :]
    ang = 2.0 * np.pi * ((j * k) % P) / P
    C = np.where(2 * k < P, np.sqrt(2.0 / P) * np.cos(ang), np.sqrt(2.0 / P) * np.sin(ang))
    C[:, 0] = 1.0 / np.sqrt(P)
    if P % 2 == 0:
        C[:, P // 2] = (1.0 - 2.0 * (np.arange(P) % 2)) / np.sqrt(P)
    omega = 2.0 * (P * kT / hbar) * np.sin(np.arange(P) * np.pi / P)
    return C, omega


def to_modes(C, X):
    """C^T X over the bead index, X (B,P,n3).  The internal modes (columns that sum to zero) are formed from x_j - x_0, as
    the device forms them: no cancellation against |x|, and exactly zero for a collapsed ring."""
    q = np.einsum('jk,bjc->bkc', C, X - X[:, :1])
    q[:, 0] = np.einsum('j,bjc->bc', C[:, 0], X)
    return q


def flow(q, v, omega, tau):
    """Exact flow of the free ring over tau in mode space; q, v (B,P,n3), omega (P,)."""
    w = omega[None, :, None]
    cs = np.cos(w * tau)
    sn = np.where(w > 0.0, np.sin(w * tau) / np.where(w > 0.0, w, 1.0), tau)
    return cs * q + sn * v, -w * np.sin(w * tau) * q + cs * v


def ring_quantities(R, V, E, F, m, P, kT, wP, f_unit):
    """(E_pot, E_kin, E_spring, K_cv, K_prim), each (B,), of rings R, V, F (B,P,n3), E (B,P); m (1,1,n3)."""
    n3 = R.shape[2]
    d = R - np.roll(R, -1, axis=1)
    e_spring = (0.5 * m * wP * wP * d * d).sum(axis=(1, 2))
    rc = R.mean(axis=1, keepdims=True)
    k_cv = 0.5 * n3 * kT - f_unit / (2.0 * P) * ((R - rc) * F).sum(axis=(1, 2))
    return E.mean(axis=1), (0.5 * m * V * V).sum(axis=(1, 2)), e_spring, k_cv, 0.5 * n3 * P * kT - e_spring / P


RING = ('E_pot', 'E_kin', 'E_spring', 'K_cv', 'K_prim')


def run(force_fn, R0, V0, masses, dt, n_steps, beads, kT, hbar, record_every=1, thermostat=None, gamma_centroid=0.0,
        pile_lambda=1.0, seed=0, step0=0, f_unit=1.0, record=('R', 'V', 'F', 'E', 'Rc'), dof_masses=False):
    """force_fn(R (B P,n3)) -> (E (B P,), F (B P,n3)), scaled as predict() scales them.  R0, V0 (B,P,n3).  masses (N,), or one
    per coordinate with dof_masses (the one-dimensional oscillator of the tests).  Returns a dict like GDMLPredict.run_pimd's."""
    P = int(beads)
    R = np.array(R0, dtype=np.float64)
    V = np.array(V0, dtype=np.float64)
    B, _, n3 = R.shape
    assert R.shape == (B, P, n3) and V.shape == R.shape
    m = np.asarray(masses, dtype=np.float64)
    m = (m if dof_masses else np.repeat(m, 3))[None, None, :]
    C, omega = modes(P, kT, hbar)
    wP = P * kT / hbar
    gam = pile_lambda * 2.0 * omega
    gam[0] = gamma_centroid
    c1 = np.exp(-gam * dt)[None, :, None]
    c2 = np.sqrt(1.0 - c1 * c1)

    def force(R):
        E, F = force_fn(R.reshape(B * P, n3))
        return E.reshape(B, P), F.reshape(B, P, n3)

    E, F = force(R)
    out = {k: [] for k in tuple(record) + RING}
    for t in range(n_steps):
        V = V + 0.5 * dt * (f_unit * F / m)
        q, v = to_modes(C, R), to_modes(C, V)
        if thermostat is None:
            q, v = flow(q, v, omega, dt)
        else:
            q, v = flow(q, v, omega, 0.5 * dt)
            v = c1 * v + c2 * np.sqrt(P * kT / m) * mr.normals(seed, step0 + t, B * P, n3).reshape(B, P, n3)
            q, v = flow(q, v, omega, 0.5 * dt)
        R = np.einsum('jk,bkc->bjc', C, q)
        V = np.einsum('jk,bkc->bjc', C, v)
        E, F = force(R)
        V = V + 0.5 * dt * (f_unit * F / m)
        if (t + 1) % record_every == 0:
            frame = dict(zip(RING, ring_quantities(R, V, E, F, m, P, kT, wP, f_unit)))
            frame.update(R=R, V=V, F=F, E=E, Rc=R.mean(axis=1))
            for k in out:
                out[k].append(np.array(frame[k]))
    shape = {'R': (B, P, n3), 'V': (B, P, n3), 'F': (B, P, n3), 'E': (B, P), 'Rc': (B, n3)}
    out = {k: np.array(v).reshape((len(v),) + shape.get(k, (B,))) for k, v in out.items()}
    out.update(R_end=R, V_end=V, step_end=step0 + n_steps)
    return out


def start(name, B, P, spread=0.01, seed=9):
    """Rings of the tests: the beads of ring b displaced by spread * N(0, 1) from start geometry b of the fixture, one seeded
    velocity (zero total momentum at masses 1) for all beads of a ring.  Returns (model, R0 (B,P,n3), V0 (B,P,n3))."""
    model, R7 = mr.case(name)
    n3 = R7.shape[1]
    R0 = R7[np.arange(B) % len(R7)][:, None, :] + spread * np.random.RandomState(seed).standard_normal((B, P, n3))
    V0 = np.repeat(mr.start_velocities(B, n3, mr.V_SCALE[name])[:, None, :], P, axis=1)
    return model, np.ascontiguousarray(R0), np.ascontiguousarray(V0)


def hamiltonian(out, P, f_unit=1.0):
    """H_P of every frame: f_unit P E_pot + E_kin + E_spring."""
    return f_unit * P * out['E_pot'] + out['E_kin'] + out['E_spring']

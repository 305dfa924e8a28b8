"""NumPy restatement of the strain derivative (virial) of the sGDML energy (csrc/predict.hip), on top of the
oracle's permuted tables and descriptors.  Test helper only: the package never imports it."""
import numpy as np

from oracle import gdml_oracle as orc


def pair_vectors(R, lat_and_inv=None):
    """Minimum-image pair vectors d_k = r_i - r_j (B,D,3) in the oracle's pair order (desc.py:44-77)."""
    R = np.asarray(R, dtype=np.float64)
    r = R.reshape(R.shape[0] if R.ndim > 1 else 1, -1, 3)
    i, j = orc.tril_pairs(r.shape[1])
    diff = r[:, i, :] - r[:, j, :]
    if lat_and_inv is not None:
        lat, lat_inv = lat_and_inv
        diff = diff - np.einsum('ab,mdb->mda', lat, np.around(np.einsum('ab,mdb->mda', lat_inv, diff)))
    return diff


def virial(R, R_desc, R_d_desc_alpha, tril_perms, sig, alphas_E=None, lat_and_inv=None):
    """Unscaled E' (B,), F (B,3N) and W = dE'/d eps (B,3,3) under r -> (I + eps) r, lattice -> (I + eps) lattice:
    W = sum_k F_x[k] g_k (x) d_k, with F_x the descriptor-space gradient of predict_from_desc and g_k = d_k / |d_k|^3."""
    R = np.asarray(R, dtype=np.float64).reshape(np.shape(R)[0] if np.ndim(R) > 1 else 1, -1)
    sig = float(sig)
    Xp, V = orc.perm_tables(np.asarray(R_desc, dtype=np.float64), np.asarray(R_d_desc_alpha, dtype=np.float64), tril_perms)
    P = tril_perms.shape[0]
    aE = np.zeros(Xp.shape[0]) if alphas_E is None else np.repeat(np.asarray(alphas_E, dtype=np.float64), P)
    x, g = orc.desc_from_R(R, lat_and_inv)
    dk = pair_vectors(R, lat_and_inv)
    B = x.shape[0]
    E, Fx = np.zeros(B), np.zeros_like(x)
    for q in range(B):
        d = x[q] - Xp
        n = np.sqrt(5.0) * np.sqrt(np.sum(d * d, axis=1))
        ex = np.exp(-n / sig)
        b = 5.0 / (3.0 * sig**3) * ex
        a = np.sum(d * V, axis=1)
        nps = n + sig
        E[q] = np.sum(a * b * nps + aE * (1.0 + n / sig + n * n / (3.0 * sig * sig)) * ex)
        Fx[q] = ((5.0 / sig) * a * b + aE * b * nps) @ d - (b * nps) @ V
    F = orc.vec_dot_d_desc(g, Fx)
    W = np.einsum('bk,bka,bkc->bac', Fx, g, dk)
    return E, F, W


def virial_of_model(model, R, lattice=None):
    """Scaled (E, F, W) of a model dict, like GDMLPredict.predict_virial; lattice overrides the model's."""
    tp = orc.tril_perms_from_lin(model['tril_perms_lin'], model['R_desc'].shape[0])
    if lattice is None and 'lattice' in model:
        lattice = model['lattice']
    lat_and_inv = None if lattice is None else (np.asarray(lattice, dtype=np.float64), np.linalg.inv(lattice))
    E, F, W = virial(R, np.asarray(model['R_desc']).T, model['R_d_desc_alpha'], tp, model['sig'], model.get('alphas_E'), lat_and_inv)
    std = model.get('std', 1.0)
    return E * std + model['c'], F * std, W * std


STRAINS = [(0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1)]


def fd_virial(energy_fn, R, lattice=None, h=1e-4):
    """4-point central differences of energy_fn(R (B,3N), lattice or None) -> E (B,) under symmetric strain of one geometry
    R (3N,): atoms and cell strained together.  Returns the symmetric (3,3) dE/d eps."""
    r = np.asarray(R, dtype=np.float64).reshape(-1, 3)
    W = np.zeros((3, 3))
    for a, c in STRAINS:
        e = []
        for s in (2.0, 1.0, -1.0, -2.0):
            eps = np.zeros((3, 3))
            eps[a, c] += 0.5 * s * h
            eps[c, a] += 0.5 * s * h
            S = np.eye(3) + eps
            e.append(energy_fn((r @ S.T).reshape(1, -1), None if lattice is None else S @ np.asarray(lattice))[0])
        d = (-e[0] + 8.0 * e[1] - 8.0 * e[2] + e[3]) / (12.0 * h)  # derivative along the symmetric direction (ac + ca) / 2
        W[a, c] = W[c, a] = d  # = (W_ac + W_ca) / 2 = W_ac for a symmetric W
    return W

"""NumPy restatement of the analytic Hessian of the sGDML energy (csrc/predict_hess.hip), on top of the oracle's
permuted tables and descriptors.  Test helper only: the package never imports it."""
import numpy as np

from oracle import gdml_oracle as orc


def hessian(R, R_desc, R_d_desc_alpha, tril_perms, sig, alphas_E=None, lat_and_inv=None):
    """Unscaled E' (B,), F (B,3N), H' = d^2 E'/dR^2 (B,3N,3N); R_desc (M,D), R_d_desc_alpha (M,D), tril_perms (P,D)."""
    R = np.asarray(R, dtype=np.float64).reshape(np.shape(R)[0] if np.ndim(R) > 1 else 1, -1)
    sig = float(sig)
    Xp, V = orc.perm_tables(np.asarray(R_desc, dtype=np.float64), np.asarray(R_d_desc_alpha, dtype=np.float64), tril_perms)
    P = tril_perms.shape[0]
    aE = np.zeros(Xp.shape[0]) if alphas_E is None else np.repeat(np.asarray(alphas_E, dtype=np.float64), P)
    x, g = orc.desc_from_R(R, lat_and_inv)
    B, D = x.shape
    N = orc.n_atoms_from_dim_d(D)
    ii, jj = orc.tril_pairs(N)
    k = np.arange(D)
    E, F, H = np.zeros(B), np.zeros((B, 3 * N)), np.zeros((B, 3 * N, 3 * N))
    for q in range(B):
        J = np.zeros((D, N, 3))  # dx_k / dR
        J[k, ii] = -g[q]
        J[k, jj] = g[q]
        J = J.reshape(D, 3 * N)
        d = x[q] - Xp
        n = np.sqrt(5.0) * np.sqrt(np.sum(d * d, axis=1))
        ex = np.exp(-n / sig)
        b = 5.0 / (3.0 * sig**3) * ex
        a = np.sum(d * V, axis=1)
        nps = n + sig
        E[q] = np.sum(a * b * nps + aE * (1.0 + n / sig + n * n / (3.0 * sig * sig)) * ex)
        Fx = ((5.0 / sig) * a * b + aE * b * nps) @ d - (b * nps) @ V
        with np.errstate(divide='ignore', invalid='ignore'):
            gam = np.where(n > 0.0, 25.0 * a * b / (sig * sig * n), 0.0) + (5.0 / sig) * aE * b
        s = -(5.0 / sig) * b
        tau = np.sum(-(5.0 / sig) * a * b - aE * b * nps)
        U, W = d @ J, V @ J
        Hq = (U * gam[:, None]).T @ U + (W * s[:, None]).T @ U + (U * s[:, None]).T @ W + tau * (J.T @ J)
        # - sum_k F_x[k] grad^2_R x_k: blocks [[Q, -Q], [-Q, Q]] on (i_k, j_k), Q = 3 g g^T / x - x^3 I
        gk, xk = g[q], x[q]
        Q = 3.0 * gk[:, :, None] * gk[:, None, :] / xk[:, None, None] - (xk**3)[:, None, None] * np.eye(3)
        FQ = Fx[:, None, None] * Q
        Hb = np.zeros((N, N, 3, 3))
        np.add.at(Hb, (ii, ii), -FQ)
        np.add.at(Hb, (jj, jj), -FQ)
        np.add.at(Hb, (ii, jj), FQ)
        np.add.at(Hb, (jj, ii), FQ)
        H[q] = Hq + Hb.transpose(0, 2, 1, 3).reshape(3 * N, 3 * N)
        F[q] = J.T @ Fx
    return E, F, H


def model_from_fixture(g):
    """GDMLPredict model dict of a golden fixture: its stored model tables, or tables built from its alphas."""
    perms = np.asarray(g['perms'])
    N = perms.shape[1]
    lat_and_inv = (g['lattice'], np.linalg.inv(g['lattice'])) if 'lattice' in g else None
    tp = orc.tril_perms_from_atom_perms(perms)
    if 'model_R_d_desc_alpha' in g:
        R_desc = np.asarray(g['R_desc'], dtype=np.float64)  # (M,D)
        jalpha = np.asarray(g['model_R_d_desc_alpha'], dtype=np.float64)
    else:
        M = g['R_train'].shape[0]
        R_desc, gd = orc.desc_from_R(g['R_train'].reshape(M, -1), lat_and_inv)
        jalpha = orc.d_desc_dot_vec(gd, np.asarray(g['alphas']).reshape(M, -1))
    model = {
        'type': 'm', 'z': np.ones(N, dtype=np.int64), 'R_desc': np.ascontiguousarray(R_desc.T), 'R_d_desc_alpha': jalpha,
        'sig': float(g['sig']), 'std': float(g['model_std']), 'c': float(g['model_c']), 'perms': perms,
        'tril_perms_lin': orc.tril_perms_lin_from_tril_perms(tp),
    }
    if 'lattice' in g:
        model['lattice'] = np.asarray(g['lattice'])
    if 'model_alphas_E' in g:
        model['alphas_E'] = np.asarray(g['model_alphas_E'])
    return model, tp, lat_and_inv


def hessian_of_model(model, R):
    """Scaled (E, F, H) of a model dict, like GDMLPredict.predict_hessian."""
    tp = orc.tril_perms_from_lin(model['tril_perms_lin'], model['R_desc'].shape[0])
    lat_and_inv = (model['lattice'], np.linalg.inv(model['lattice'])) if 'lattice' in model else None
    E, F, H = hessian(R, np.asarray(model['R_desc']).T, model['R_d_desc_alpha'], tp, model['sig'], model.get('alphas_E'),
                      lat_and_inv)
    std = model.get('std', 1.0)
    return E * std + model['c'], F * std, H * std


def fd_hessian(force_fn, R, h=1e-4):
    """4-point central difference -dF/dR of force_fn(R (B,3N)) -> F (B,3N) at one geometry R (3N,)."""
    R = np.asarray(R, dtype=np.float64).ravel()
    n = R.size
    steps = np.array([2.0, 1.0, -1.0, -2.0]) * h
    Rs = R[None, None, :] + steps[:, None, None] * np.eye(n)[None]
    Fs = force_fn(Rs.reshape(-1, n)).reshape(4, n, n)
    dF = (-Fs[0] + 8.0 * Fs[1] - 8.0 * Fs[2] + Fs[3]) / (12.0 * h)  # dF[j, :] = dF/dR_j
    return -dF.T

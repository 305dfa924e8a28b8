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


# --------------------------------------------------------------------------- long-double reference

LD = np.longdouble


def _scatter_pairs(gy, ii, jj, N):
    """J_x^T applied as a scatter over pairs: gy (..., D, 3) = g_k y_k; out[i_k] -= gy_k, out[j_k] += gy_k -> (..., 3N)."""
    out = np.zeros(gy.shape[:-2] + (N, 3), dtype=gy.dtype)
    lead = (slice(None),) * (gy.ndim - 2)
    np.subtract.at(out, lead + (ii,), gy)
    np.add.at(out, lead + (jj,), gy)
    return out.reshape(gy.shape[:-2] + (3 * N,))


def hessian_ld(R, R_desc, R_d_desc_alpha, tril_perms, sig, alphas_E=None, lat_and_inv=None):
    """hessian() in np.longdouble from the Cartesian geometries on (distances, x, g, d, coefficients, every sum), written
    without the dense Jacobian: the projections are scatters over pairs and tau J^T J - sum F_x grad^2 x is built as 3 x 3
    blocks on (i_k, j_k).  Returns unscaled E' (B,), F (B,3N), H' (B,3N,3N) as long doubles.  Where the host's long double is
    no wider than 1e-18 this falls back to hessian() and says so."""
    if not np.finfo(LD).eps < 1e-18:
        print('hessian_ld: np.longdouble has eps = %g on this host, falling back to the float64 restatement' % np.finfo(LD).eps)
        return hessian(R, R_desc, R_d_desc_alpha, tril_perms, sig, alphas_E, lat_and_inv)
    R = np.asarray(R, dtype=np.float64)
    R = R.reshape(R.shape[0] if R.ndim > 1 else 1, -1)
    B, N = R.shape[0], R.shape[1] // 3
    Xp, V = orc.perm_tables(np.asarray(R_desc, dtype=np.float64), np.asarray(R_d_desc_alpha, dtype=np.float64), tril_perms)
    Xp, V = Xp.astype(LD), V.astype(LD)
    P = tril_perms.shape[0]
    aE = np.zeros(Xp.shape[0], dtype=LD) if alphas_E is None else np.repeat(np.asarray(alphas_E, dtype=np.float64), P).astype(LD)
    ii, jj = orc.tril_pairs(N)
    sig = LD(sig)
    sqrt5, five, three, one = np.sqrt(LD(5)), LD(5), LD(3), LD(1)
    E, F, H = np.zeros(B, dtype=LD), np.zeros((B, 3 * N), dtype=LD), np.zeros((B, 3 * N, 3 * N), dtype=LD)
    eye3 = np.eye(3, dtype=LD)
    for q in range(B):
        r = R[q].astype(LD).reshape(N, 3)
        diff = r[ii] - r[jj]
        if lat_and_inv is not None:  # the oracle's rule: diff -= lat @ round(lat_inv @ diff)
            lat, lat_inv = (np.asarray(a, dtype=np.float64).astype(LD) for a in lat_and_inv)
            diff = diff - np.rint(diff @ lat_inv.T) @ lat.T
        x = one / np.sqrt(np.sum(diff * diff, axis=1))
        g = diff * (x * x * x)[:, None]
        d = x[None, :] - Xp
        n = sqrt5 * np.sqrt(np.sum(d * d, axis=1))
        ex = np.exp(-n / sig)
        b = five / (three * sig * sig * sig) * ex
        a = np.sum(d * V, axis=1)
        nps = n + sig
        E[q] = np.sum(a * b * nps + aE * (one + n / sig + n * n / (three * sig * sig)) * ex)
        Fx = (five / sig * a * b + aE * b * nps) @ d - (b * nps) @ V
        gam = five / sig * aE * b
        pos = n > 0
        gam[pos] += LD(25) * a[pos] * b[pos] / (sig * sig * n[pos])
        s = -five / sig * b
        tau = np.sum(-five / sig * a * b - aE * b * nps)
        U = _scatter_pairs(d[:, :, None] * g[None], ii, jj, N)
        W = _scatter_pairs(V[:, :, None] * g[None], ii, jj, N)
        T = U.T @ (LD(0.5) * gam[:, None] * U + s[:, None] * W)  # T + T^T = sum gam u u^T + s (u w^T + w u^T)
        # C_k = tau g g^T - F_x[k] Q_k enters as [[C, -C], [-C, C]] on the atom pair (i_k, j_k)
        gg = g[:, :, None] * g[:, None, :]
        Ck = tau * gg - Fx[:, None, None] * (three * gg / x[:, None, None] - (x * x * x)[:, None, None] * eye3)
        Hb = np.zeros((N, N, 3, 3), dtype=LD)
        Hb[ii, jj] = -Ck
        Hb[jj, ii] = -Ck.transpose(0, 2, 1)
        np.add.at(Hb, (ii, ii), Ck)
        np.add.at(Hb, (jj, jj), Ck)
        H[q] = T + T.T + Hb.transpose(0, 2, 1, 3).reshape(3 * N, 3 * N)
        F[q] = _scatter_pairs(g * Fx[:, None], ii, jj, N)
    return E, F, H


def hessian_ld_of_model(model, R):
    """Scaled (E, F, H) of a model dict from hessian_ld, as long doubles."""
    tp = orc.tril_perms_from_lin(model['tril_perms_lin'], model['R_desc'].shape[0])
    lat_and_inv = (model['lattice'], np.linalg.inv(model['lattice'])) if 'lattice' in model else None
    E, F, H = hessian_ld(R, np.asarray(model['R_desc']).T, model['R_d_desc_alpha'], tp, model['sig'], model.get('alphas_E'),
                         lat_and_inv)
    std = LD(model.get('std', 1.0))
    return E * std + LD(model['c']), F * std, H * std


# --------------------------------------------------------------------------- synthetic models


def synth_perms(N, P):
    """Identity; P = 2: and the swap (0 1); P = 6: the group of (0 1) and the 3-cycle on atoms 2, 3, 4."""
    e = np.arange(N)
    if P == 1:
        return e[None]
    swap = e.copy()
    swap[[0, 1]] = swap[[1, 0]]
    if P == 2:
        return np.array([e, swap])
    assert P == 6 and N >= 5
    cyc = e.copy()
    cyc[[2, 3, 4]] = cyc[[3, 4, 2]]
    cyc2 = cyc[cyc]
    return np.array([e, swap, cyc, swap[cyc], cyc2, swap[cyc2]])


def wrap_margin(R, L):
    """Smallest distance of any component of lat_inv @ diff (cubic cell of edge L) from a half-integer, and the number of
    components that wrap, over the geometries R (B,3N)."""
    r = np.asarray(R).reshape(len(R), -1, 3)
    i, j = orc.tril_pairs(r.shape[1])
    c = (r[:, i, :] - r[:, j, :]) / L
    return np.abs(c - np.floor(c) - 0.5).min(), int((np.abs(c) > 0.5).sum())


def synth_cell_edge(R, margin=1.5e-3):
    """Edge of a cubic cell in which a few of the longest pair components of the geometries R (B,3N) wrap and no component of
    lat_inv @ diff lies within `margin` of a half-integer: twice the midpoint of the widest gap among the 80 largest
    components (wrapping many more pairs than that leaves no gap of this width among 10^5 components)."""
    r = np.asarray(R).reshape(len(R), -1, 3)
    i, j = orc.tril_pairs(r.shape[1])
    a = np.sort(np.abs(r[:, i, :] - r[:, j, :]).ravel())[::-1][:81]
    k = int(np.argmax(a[:-1] - a[1:]))
    L = float(a[k] + a[k + 1])
    assert wrap_margin(R, L)[0] >= margin, (L, wrap_margin(R, L))
    return L


def synth_model(N, M, P=1, with_aE=False, lattice=False, seed=0):
    """(model dict, R_train (M,3N), R_query (4,3N)): geometries of the oracle's synthetic data set, random coefficients
    (standard normal J alpha and alphas_E), sigma = 25, std and c away from 1 and 0; with `lattice` a cubic cell in which a few
    of the longest pairs wrap (synth_cell_edge); every geometry then has one atom moved by a lattice vector, which leaves the
    periodic system and the distance of every component from a half-integer as they are and makes that atom's N - 1 pairs
    wrap."""
    ds = orc.synth_dataset(N, M + 4, seed=seed, jitter=0.3)
    R = ds['R'].reshape(M + 4, -1)
    perms = synth_perms(N, P)
    tp = orc.tril_perms_from_atom_perms(perms)
    lat = None
    if lattice:
        lat = np.eye(3) * synth_cell_edge(R)
        for m in range(M + 4):
            R[m, 3 * (m % N) + m % 3] += lat[0, 0] * (1 if m % 2 else -1)
    R_desc, _ = orc.desc_from_R(R[:M], None if lat is None else (lat, np.linalg.inv(lat)))
    rs = np.random.RandomState(1000 + seed)
    model = {
        'type': 'm', 'z': np.ones(N, dtype=np.int64), 'R_desc': np.ascontiguousarray(R_desc.T),
        'R_d_desc_alpha': rs.standard_normal(R_desc.shape), 'sig': 25.0, 'std': 1.75, 'c': -3.25, 'perms': perms,
        'tril_perms_lin': orc.tril_perms_lin_from_tril_perms(tp),
    }
    if with_aE:
        model['alphas_E'] = rs.standard_normal(M)
    if lat is not None:
        model['lattice'] = lat
    return model, R[:M].copy(), R[M:].copy()


# --------------------------------------------------------------------------- the host's plan

HT, HK, HE = 64, 16, 16
HESS_PANEL_BYTES = 256 << 20
HESS_LDS_MAX = 152 * 1024


def hess_plan(N, MP, B, generic=0, chunk_rows=0):
    """What hess_device (csrc/predict_hess.hip) does for N atoms, MP table rows and B queries under the options
    predict.hess_generic and predict.hess_chunk_rows: an independent restatement of the arithmetic that csrc/hess_plan.h
    compiles, written from the host code as it stood before that header existed.  tests/test_hess_plan_cpu.py pins the two to
    each other field by field.  None when the library refuses the size."""
    D, n3 = N * (N - 1) // 2, 3 * N
    if D * 8 > HESS_LDS_MAX:
        return None
    nb = (n3 + HT - 1) // HT
    ld, n_tp = nb * HT, nb * (nb + 1) // 2
    kt = (D + 255) // 256
    KT = 1
    while KT < kt:
        KT <<= 1
    if KT == 64 and kt <= 48:
        KT = 48
    if kt > 48 or generic:
        KT = 0
    KPL = 1
    while KPL * 64 < D:
        KPL <<= 1
    wave = D <= 512 and not generic
    v_lds = int(wave or 2 * D * 8 <= HESS_LDS_MAX)
    lds_bytes = 8 * D * 8 if wave else (2 if v_lds else 1) * D * 8
    Bs = min(B, 64)
    while Bs > 1 and Bs * ld * ld * 8 > HESS_PANEL_BYTES:
        Bs >>= 1
    nr_cap = HESS_PANEL_BYTES // (Bs * (ld * 16 + 16))
    if 0 < chunk_rows < nr_cap:
        nr_cap = chunk_rows
    nr_cap = min(nr_cap, MP)
    RG = 256
    while RG > (4 if wave else 8) and ((nr_cap + RG - 1) // RG) * Bs < 4096:
        RG >>= 1
    nr_cap = (nr_cap + RG - 1) // RG * RG
    G = (min(MP, nr_cap) + RG - 1) // RG
    JS = (1024 + n_tp * Bs - 1) // (n_tp * Bs)
    JS = max(1, min(JS, max(nr_cap // 64, 1)))
    nU = Bs * nr_cap * ld
    ws = [nU, nU, Bs * nr_cap * 2, G * Bs * D, G * Bs * 2, JS * Bs * ld * ld, Bs * D, Bs]  # U W cs part_F part_ET Hp fx tau
    slices = [min(Bs, B - b0) for b0 in range(0, B, Bs)]
    chunks = [min(nr_cap, MP - r0) for r0 in range(0, MP, nr_cap)]
    rps = [(nr + JS - 1) // JS for nr in chunks]
    groups = [(nr + RG - 1) // RG for nr in chunks]
    return dict(
        N=N, D=D, n3=n3, MP=MP, B=B, variant=('wave', KPL) if wave else ('block', KT), forced=bool(generic), v_lds=v_lds,
        lds_bytes=lds_bytes, nb=nb, ld=ld, n_tp=n_tp, Bs=Bs, slices=slices, RG=RG, nr_cap=nr_cap, G=G, JS=JS, ws=ws,
        ws_bytes=8 * sum(ws), chunks=chunks, rps=rps, groups=groups,
        last_group_rows=[nr - (ng - 1) * RG for nr, ng in zip(chunks, groups)],
        idle_waves=[(-ng) % 4 if wave else 0 for ng in groups],  # wavefronts of the last workgroup past the last group
        empty_splits=[JS - (nr + r - 1) // r for nr, r in zip(chunks, rps)],  # splits that begin at or past the chunk's end
        rps_mod16=[r % HK for r in rps])


# --------------------------------------------------------------------------- the grid of tests/test_hessian_grid_gpu.py

# size axis: both sides of every switch point of the projection dispatch and of the 64-wide tiles of the 3N axis; 171 is the
# one size with nine tiles (3N = 513: a last tile one column wide)
SIZE_N = [2, 3, 11, 12, 16, 17, 21, 22, 23, 24, 32, 33, 43, 45, 46, 64, 65, 91, 92, 128, 129, 139, 140, 157, 158, 197, 171]
SIZE_LATTICE = (12, 33, 158)
N_UNSUPPORTED = 198
# row and batch axis: (M P, B, predict.hess_chunk_rows).  The last two go beyond the issue's list: 265 rows in chunks of 128
# are three chunks with two splits each and a shorter last one; 1024 rows at 64 queries are the smallest table whose row
# groups exceed the minimum (RG = 16 for the block variants, 8 for the wave variants)
ROW_CASES = [(1, 1, 0), (4, 1, 0), (5, 3, 0), (63, 1, 0), (64, 1, 0), (65, 1, 0), (130, 1, 0), (130, 1, 40), (130, 3, 40),
             (600, 1, 0), (600, 64, 0), (600, 65, 0), (600, 129, 0), (600, 1, 200), (265, 1, 256), (70, 65, 16),
             (600, 65, 100), (265, 1, 128), (1024, 64, 0)]
ROW_N = (12, 33)


def grid_plan_inputs():
    """(N, M P, B, predict.hess_generic, predict.hess_chunk_rows) of every call of the grid."""
    inputs = [(N, size_case(N)['M'] * size_case(N)['P'], 2, 0, 0) for N in SIZE_N]
    return inputs + [(N, MP, B, generic, chunk) for N in ROW_N for generic in (0, 1) for MP, B, chunk in ROW_CASES]


def size_case(N):
    """Size axis: P = 2 at every second size, alphas_E at every third, a lattice at one size per projection family; M = 5
    below 100 atoms and 3 from there on."""
    i = SIZE_N.index(N)
    return dict(N=N, M=5 if N < 100 else 3, P=2 if i % 2 else 1, with_aE=i % 3 == 0, lattice=N in SIZE_LATTICE, seed=N)


def row_case(N, MP):
    """Row axis: two permutations where M P is even, alphas_E where it is a multiple of five."""
    P = 2 if MP % 2 == 0 else 1
    return dict(N=N, M=MP // P, P=P, with_aE=MP % 5 == 0, lattice=False, seed=1000 * N + MP)


_cache = {}


def grid_model(N, M, P, with_aE, lattice, seed):
    """(model, R5, (E, F, H) of hessian_ld on R5) of a grid case, computed once per process.  R5: an unseen geometry, training
    geometry 0 (with atoms 0 and 1 exchanged where P > 1, so that the zero distance falls on a non-identity table row), and
    three more unseen geometries."""
    key = (N, M, P, with_aE, lattice, seed)
    if key not in _cache:
        model, R_train, R_query = synth_model(N, M, P, with_aE, lattice, seed)
        r0 = R_train[0].reshape(N, 3)
        if P > 1:
            r0 = r0[synth_perms(N, 2)[1]]
        R5 = np.concatenate([R_query[:1], r0.reshape(1, -1), R_query[1:]])
        _cache[key] = [model, R5, None]
    return _cache[key]


def grid_reference(case, n_geoms):
    """Scaled long-double (E, F, H) of the first n_geoms of the case's five geometries; the largest request so far is kept."""
    ent = grid_model(**case)
    if ent[2] is None or len(ent[2][0]) < n_geoms:
        ent[2] = hessian_ld_of_model(ent[0], ent[1][:n_geoms])
    return tuple(a[:n_geoms] for a in ent[2])


def batch_index(B):
    """Which of the five geometries query q is: the first B for B <= 5, else tiled with stride 3."""
    return np.arange(B) if B <= 5 else (3 * np.arange(B)) % 5


def grid_measure(pred, case, B, generic=0, chunk_rows=0):
    """One predict_hessian call of B queries on predictor `pred` of a grid case under the two options (reset afterwards),
    against the long-double reference.  Returns the figures the test asserts on, each as error / bound (<= 1 passes) or as a
    flag: h, f, e (1e-10 max|H_ld| per geometry, 1e-10 max|F_ld|, 1e-10 max(1, |E_ld|)), sum_rule (1e-12 max|H|), symmetric,
    duplicates_equal, repeat_equal, and f_predict, e_predict against predict() with the floors of
    tests/test_hessian_gpu.py::test_hessian_matches_restatement."""
    model, R5, _ = grid_model(**case)
    idx = batch_index(B)
    R = np.ascontiguousarray(R5[idx])
    E_ref, F_ref, H_ref = grid_reference(case, int(idx.max()) + 1)
    N = case['N']
    opts = {'predict.hess_generic': generic, 'predict.hess_chunk_rows': chunk_rows}
    try:
        for k, v in opts.items():
            pred._ctx.set_option(k, v)
        E, F, H = pred.predict_hessian(R)
        E2, F2, H2 = pred.predict_hessian(R)
    finally:
        for k in opts:
            pred._ctx.set_option(k, 0)
    out = dict(h=0.0, f=0.0, e=0.0, sum_rule=0.0)
    for q in range(B):
        g = idx[q]
        out['h'] = max(out['h'], float(np.abs(H[q] - H_ref[g]).max() / (1e-10 * np.abs(H_ref[g]).max())))
        out['f'] = max(out['f'], float(np.abs(F[q] - F_ref[g]).max() / (1e-10 * np.abs(F_ref[g]).max())))
        out['e'] = max(out['e'], float(abs(E[q] - E_ref[g]) / (1e-10 * max(1.0, abs(E_ref[g])))))
        scale = np.abs(H[q]).max()
        out['sum_rule'] = max(out['sum_rule'], float(np.abs(H[q].reshape(3 * N, N, 3).sum(axis=1)).max() / (1e-12 * scale)))
    out['symmetric'] = bool(np.array_equal(H, H.transpose(0, 2, 1)))
    first = np.array([np.flatnonzero(idx == g)[0] for g in idx])
    out['duplicates_equal'] = bool(np.array_equal(H, H[first]) and np.array_equal(F, F[first]) and np.array_equal(E, E[first]))
    out['repeat_equal'] = bool(np.array_equal(H, H2) and np.array_equal(F, F2) and np.array_equal(E, E2))
    # E and F of the call are those of predict(), up to the floors of two correct summation orders
    Ep, Fp = pred.predict(R)
    eps = np.finfo(float).eps
    lat_and_inv = (model['lattice'], np.linalg.inv(model['lattice'])) if 'lattice' in model else None
    _, gq = orc.desc_from_R(R5[:int(idx.max()) + 1], lat_and_inv)
    rows = model['R_desc'].shape[1] * len(model['perms'])
    f_floor = (50 * eps * model['std'] * np.abs(model['R_d_desc_alpha']).max() * 5.0 / (3 * model['sig']**2) * np.sqrt(rows)
               * max(1.0, np.abs(gq).max()))
    e_floor = 5 * eps * model['std'] * np.abs(model['alphas_E']).max() * np.sqrt(rows) if 'alphas_E' in model else 0.0
    out['f_predict'] = float(np.abs(F - Fp).max() / (1e-12 * np.abs(Fp).max() + f_floor))
    out['e_predict'] = float(np.abs(E - Ep).max() / (1e-12 * np.abs(Ep).max() + e_floor + f_floor * model['sig']))
    return out

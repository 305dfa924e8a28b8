"""NumPy restatement of the harmonic vibrational analysis (gdml_vib_run, csrc/vib.hip) and of the batched Jacobi eigensolver
under it (gdml_sym_eig, csrc/sym_eig.hip; the sweep loop: csrc/sym_eig.h), with the conventions both state.  Test helper only: the package never imports it.

The eigensolver.  Cyclic two-sided Jacobi, round-robin ordering: with ne = n rounded up to even, m = ne - 1 and np = ne / 2, step
s = 0 .. m - 1 of a sweep rotates the pairs (s mod m, m) and ((s + t) mod m, (s + m - t) mod m), t = 1 .. np - 1 (the smaller
index is p; a pair with q = n, the padding index of an odd n, is skipped).  Angles come from the matrix as the step finds it:
tau = (a_qq - a_pp) / (2 a_pq), t = sign(tau) / (|tau| + sqrt(1 + tau^2)), c = 1 / sqrt(1 + t^2), s = t c (a_pq = 0: no
rotation); then all row updates, then all column updates of A and V; then a_pq = a_qp = 0 exactly.  A sweep starts only while
off > 1e-30 (off + dia), the sums of squares off and on the diagonal; at most 30 sweeps.
Conventions: eigenvalues ascending, ties by Jacobi column; eigenvectors as rows; the component of largest magnitude positive,
the lowest index on ties.

The projection.  D = h_scale sym(H) / sqrt(m_i m_j); candidates translations sqrt(m_i) e_c, then rotations sqrt(m_i) (e_c x (r_i -
r_cm)), c = x, y, z; modified Gram-Schmidt in that order, a candidate whose remainder has a squared norm below RANK_TOL of its
own is dropped; P = I - Q^T Q; D_s = P D P + Lambda Q^T Q, Lambda = 2 |P D P|_F (1 if that is 0); tau = 3N eps |D_s|_F."""
import numpy as np

EPS = np.finfo(np.float64).eps
MAX_SWEEPS = 30
RANK_TOL = 1e-10
PROJECT = {'none': 0, 'trans': 1, 'rigid': 2}


def bound(n, A):
    """The agreed error bound of the eigensolver on one matrix: 40 n eps |A|_F (at most 30 sweeps of n - 1 steps, each rounding
    once relative to the norm, plus the length-n dot products of the checks)."""
    return 40.0 * n * EPS * np.linalg.norm(A)


def order_and_sign(diag, V):
    """Jacobi diagonal and rotation matrix (eigenvectors in columns) -> (w ascending, rows with the sign convention)."""
    order = np.argsort(diag, kind='stable')  # ties: the lower column first
    w = diag[order]
    rows = V[:, order].T.copy()
    for k in range(len(w)):
        a = int(np.argmax(np.abs(rows[k])))  # the first of equal maxima
        if rows[k, a] < 0.0:
            rows[k] = -rows[k]
    return w, rows


def jacobi(A):
    """(w (n,), V (n,n) rows, sweeps) of one symmetric matrix by the device's iteration; sweeps = MAX_SWEEPS + 1 when the
    matrix is still above the threshold after the cap."""
    A = np.array(A, dtype=np.float64)
    n = A.shape[0]
    A = 0.5 * (A + A.T)
    V = np.eye(n)
    ne = (n + 1) & ~1
    npairs, m = ne // 2, ne - 1

    def converged():
        dia = float(np.sum(np.diag(A) ** 2))
        O = A - np.diag(np.diag(A))
        off = float(np.sum(O * O))
        return off <= 1e-30 * (dia + off)

    sweeps = 0
    while sweeps < MAX_SWEEPS:
        if converged():
            break
        for step in range(m):
            ps, qs, cs, ss = [], [], [], []
            for t in range(npairs):
                if t == 0:
                    p, q = step % m, m
                else:
                    p, q = (step + t) % m, (step + m - t) % m
                if p > q:
                    p, q = q, p
                if q >= n:
                    continue
                c, s = 1.0, 0.0
                apq = A[p, q]
                if apq != 0.0:
                    tau = (A[q, q] - A[p, p]) / (2.0 * apq)
                    tt = (1.0 if tau >= 0.0 else -1.0) / (abs(tau) + np.sqrt(1.0 + tau * tau))
                    c = 1.0 / np.sqrt(1.0 + tt * tt)
                    s = tt * c
                ps.append(p); qs.append(q); cs.append(c); ss.append(s)
            if not ps:
                continue
            ps, qs, cs, ss = np.array(ps), np.array(qs), np.array(cs), np.array(ss)
            ap, aq = A[ps, :].copy(), A[qs, :].copy()  # rows:  A <- J^T A
            A[ps, :] = cs[:, None] * ap - ss[:, None] * aq
            A[qs, :] = ss[:, None] * ap + cs[:, None] * aq
            ap, aq = A[:, ps].copy(), A[:, qs].copy()  # columns:  A <- A J,  V <- V J
            A[:, ps] = cs[None, :] * ap - ss[None, :] * aq
            A[:, qs] = ss[None, :] * ap + cs[None, :] * aq
            vp, vq = V[:, ps].copy(), V[:, qs].copy()
            V[:, ps] = cs[None, :] * vp - ss[None, :] * vq
            V[:, qs] = ss[None, :] * vp + cs[None, :] * vq
            A[ps, qs] = 0.0
            A[qs, ps] = 0.0
        sweeps += 1
    if sweeps == MAX_SWEEPS and not converged():
        sweeps = MAX_SWEEPS + 1
    w, rows = order_and_sign(np.diag(A).copy(), V)
    return w, rows, sweeps


def eig_errors(A, w, V):
    """(eigenvalue error against LAPACK, residual max_k |A v_k - w_k v_k|, orthogonality |V V^T - I|_max) of one matrix."""
    A = 0.5 * (A + A.T)
    w_ref = np.linalg.eigvalsh(A)
    res = np.sqrt((((A @ V.T) - V.T * w[None, :]) ** 2).sum(axis=0)).max()
    return np.abs(w - w_ref).max(), res, np.abs(V @ V.T - np.eye(len(w))).max()


def sign_convention_holds(V):
    a = np.argmax(np.abs(V), axis=-1)
    return bool((np.take_along_axis(V, a[..., None], axis=-1) > 0.0).all())


# ---- projection

def rigid_basis(R, masses, project):
    """(Q (k,3N) orthonormal rows, ratios): the rigid basis of one geometry R (3N,) and, per candidate, the squared norm of its
    remainder over its own squared norm (nan for a zero candidate) -- what the rank rule compares with RANK_TOL."""
    r = np.asarray(R, dtype=np.float64).reshape(-1, 3)
    m = np.asarray(masses, dtype=np.float64)
    N = len(m)
    sw = np.sqrt(np.repeat(m, 3))
    cands = []
    if project >= 1:
        for c in range(3):
            v = np.zeros((N, 3))
            v[:, c] = 1.0
            cands.append(v.ravel() * sw)
    if project == 2:
        cm = (m[:, None] * r).sum(axis=0) / m.sum()
        d = r - cm[None]
        for c in range(3):
            e = np.zeros(3)
            e[c] = 1.0
            cands.append(np.cross(e[None, :], d).ravel() * sw)
    Q, ratios = [], []
    for v in cands:
        orig2 = float(v @ v)
        for q in Q:
            v = v - (q @ v) * q
        rem2 = float(v @ v)
        ratios.append(rem2 / orig2 if orig2 > 0.0 else np.nan)
        if orig2 > 0.0 and rem2 >= RANK_TOL * orig2:
            Q.append(v / np.sqrt(rem2))
    return np.array(Q).reshape(len(Q), 3 * N), np.array(ratios)


def mass_weight(H, masses, h_scale=1.0):
    sw = np.sqrt(np.repeat(np.asarray(masses, dtype=np.float64), 3))
    return h_scale * (0.5 * (H + H.T)) / (sw[:, None] * sw[None, :])


def shifted(H, R, masses, h_scale=1.0, project=2):
    """(D_s, Q, Lambda, ratios) of one geometry: H (3N,3N) the unscaled Hessian."""
    D = mass_weight(H, masses, h_scale)
    Q, ratios = rigid_basis(R, masses, project)
    n = D.shape[0]
    P = np.eye(n) - Q.T @ Q
    PDP = P @ D @ P
    PDP = 0.5 * (PDP + PDP.T)
    lam = 0.0
    if len(Q):
        nrm = np.linalg.norm(PDP)
        lam = 2.0 * nrm if nrm > 0.0 else 1.0
    return PDP + lam * (Q.T @ Q), Q, lam, ratios


def vibrations(H, R, masses, h_scale=1.0, project=2):
    """Restated gdml_vib_run of one geometry with LAPACK's eigh: dict with 'w2' (3N; the vibrational entries ascending, then
    n_rigid zeros), 'modes' (rows), 'n_rigid', 'n_neg', 'tau', 'D_s', 'Q', 'ratios'."""
    D_s, Q, lam, ratios = shifted(H, R, masses, h_scale, project)
    n, k = D_s.shape[0], len(Q)
    w, U = np.linalg.eigh(D_s)
    tau = n * EPS * np.linalg.norm(D_s)
    w2 = w.copy()
    w2[n - k:] = 0.0
    return dict(w2=w2, modes=U.T.copy(), n_rigid=k, n_neg=int((w2[:n - k] < -tau).sum()), tau=tau, D_s=D_s, Q=Q, ratios=ratios,
                Lambda=lam)


# ---- the launch plan of the eigensolver and the slice of a spectrum (csrc/sym_eig_plan.h), restated

LDS_MAX = 160 * 1024
VIB_CHUNK_BYTES = 256 << 20


def sym_eig_plan(num_cus, M, N, cap_global):
    """NP, a_in_lds, v_in_lds, lds, grid, work_doubles.  LDS of a workgroup: cs [npairs][2] doubles, pq [npairs][2] ints padded to
    a multiple of 8 bytes, red [8] doubles, then A and V (N x NP doubles each) as far as they fit under 160 KiB; 4, 2 or 1
    workgroups per compute unit by the LDS they take, at most M, and with cap_global at most one per compute unit once A is in
    device memory; the device-memory work area is two matrices per workgroup unless V is in LDS."""
    NP = N + 1 if N % 2 == 0 else N
    npairs = (N + 1) // 2
    fixed = 2 * npairs * 8 + (2 * npairs + (npairs % 2) * 2) * 4 + 64
    mat = N * NP * 8
    a = fixed + mat <= LDS_MAX
    v = a and fixed + 2 * mat <= LDS_MAX
    lds = fixed + (mat if a else 0) + (mat if v else 0)
    grid = num_cus * (1 if lds > 80 * 1024 else 2 if lds > 40 * 1024 else 4)
    if cap_global and not a:
        grid = min(grid, num_cus)
    grid = min(grid, M)
    return dict(NP=NP, a_in_lds=int(a), v_in_lds=int(v), lds=lds, grid=grid, work_doubles=0 if v else grid * 2 * N * NP)


SPECTRUM_FIELDS = ('work', 'H', 'R', 'F', 'w', 'info', 'E', 'mass', 'sweeps', 'n_rigid', 'n_neg')


def spectrum_ws(len_, N, work_doubles, with_R):
    """[(field, offset, length)] of a slice's workspace in 8-byte words, in SPECTRUM_FIELDS' order, and the total."""
    n3 = 3 * N
    sizes = dict(work=work_doubles, H=len_ * n3 * n3, R=len_ * n3 if with_R else 0, F=len_ * n3, w=len_ * n3, info=4 * len_,
                 E=len_, mass=N, sweeps=len_, n_rigid=len_, n_neg=len_)
    out, o = [], 0
    for f in SPECTRUM_FIELDS:
        out.append((f, o, sizes[f]))
        o += sizes[f]
    return out, o


def spectrum_slice_len(num_cus, B, n3, option):
    """Geometries per slice: VIB_CHUNK_BYTES over the bytes one geometry brings (its share of the workspace with R and the work
    matrices of one workgroup), whole 64s above 64; a positive option instead; within 1 .. B."""
    p1 = sym_eig_plan(num_cus, 1, n3, True)
    per = (n3 * n3 + 3 * n3 + 8 + p1['work_doubles']) * 8
    chunk = VIB_CHUNK_BYTES // per
    if chunk > 64:
        chunk = chunk // 64 * 64
    if option > 0:
        chunk = option
    return min(max(chunk, 1), B)


# ---- inputs, geometries and toys of the tests

def eig_inputs(n, M=3, seed=0):
    """M random symmetric matrices of order n."""
    rs = np.random.RandomState(1000 * n + seed)
    A = rs.standard_normal((M, n, n))
    return A + A.transpose(0, 2, 1)


def eig_special(n):
    """diagonal, zero, c I + rank one (an (n - 1)-fold eigenvalue), random scaled by 2^30 and by 2^-30."""
    rs = np.random.RandomState(7 * n + 1)
    u = rs.standard_normal(n)
    R = eig_inputs(n, 1, seed=3)[0]
    return np.stack([np.diag(rs.standard_normal(n)), np.zeros((n, n)), 1.5 * np.eye(n) + np.outer(u, u), R * 2.0**30, R * 2.0**-30])


def geoms(g):
    """Seven geometries of a fixture: its first six test geometries and its first training geometry."""
    Rt = g['R_test'].reshape(len(g['R_test']), -1)
    return np.concatenate([Rt[:6], g['R_train'][:1].reshape(1, -1)])


def collinear(bent=False):
    """Five atoms on a line of direction (1, 2, 3) with unequal spacings 1.0 .. 1.7 and masses 1, 12, 16, 1, 12 ((15,), (5,));
    bent: the middle atom moved 0.3 off the line."""
    u = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    s = np.concatenate([[0.0], np.cumsum([1.0, 1.7, 1.2, 1.45])])
    r = np.array([0.3, -0.2, 0.1])[None, :] + s[:, None] * u[None, :]
    if bent:
        off = np.cross(u, [0.0, 0.0, 1.0])
        r[2] += 0.3 * off / np.linalg.norm(off)
    return r.ravel(), np.array([1.0, 12.0, 16.0, 1.0, 12.0])


def fixture_masses(N):
    """Masses drawn from {1, 12, 16} by atom index."""
    return np.array([1.0, 12.0, 16.0])[np.arange(N) % 3]


def band_tangent(R_band, E_band, i):
    """Unit improved tangent (Henkelman, Jonsson 2000) of interior image i of one band R_band (P,3N) with energies E_band (P,)."""
    tp, tm = R_band[i + 1] - R_band[i], R_band[i] - R_band[i - 1]
    Ep, E0, Em = E_band[i + 1], E_band[i], E_band[i - 1]
    if Ep > E0 > Em:
        t = tp
    elif Ep < E0 < Em:
        t = tm
    else:
        dmax, dmin = max(abs(Ep - E0), abs(Em - E0)), min(abs(Ep - E0), abs(Em - E0))
        t = tp * dmax + tm * dmin if Ep > Em else tp * dmin + tm * dmax
    return t / np.linalg.norm(t)

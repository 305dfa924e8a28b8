"""NumPy restatement of the on-device eigenvector following (gdml_ef_run, csrc/ef.hip; GDMLPredict.stationary_point) around a
Hessian callback, the margins of its decisions, and the toy runs of the tests.  Test helper only: the package never imports it.

The step (the contract; include/gdml_hip.h states the same).  g = -f_unit * F, D = f_unit * H with E, F, H those of
predict_hessian(); unit masses.  State per geometry: trust, E_prev, dE_pred, flags (bit 0: a previous step exists, bit 1: it was
clipped) and the follow vector t (or none).  Evaluation n = 0, 1, ... of an active geometry:
  1.-3. E, F, H = predictor(r);  D_s = P D P + Lambda Q^T Q (_vib_ref.shifted);  w ascending, v_i rows (_vib_ref.jacobi, the
        device's iteration, so that near-degenerate eigenvectors match the device's; eigensolve() below);  nv = 3N - n_rigid vibrational pairs
  a. f_atom = max over atoms |g_atom|
  d. followed mode k (order 1): 0 without t, else argmax_i |v_i . t| over i < nv, ties to the lowest i; order 0: k = 0
     f_atom < fmax: converged;  else n = max_steps: stops unconverged.  A frozen geometry keeps the state it entered with.
  b. if bit 0 and |dE_pred| > 1e-8 max(|E - c|, |E_prev - c|) f_unit:  rho = f_unit (E - E_prev) / dE_pred;
     rho < 0.25 or rho > 1.75: trust <- max(trust / 2, trust_min);  0.75 < rho < 1.25 and bit 1: trust <- min(2 trust, trust_max)
  c. gt_i = v_i . g, i < nv
  e. d_i = |w_i| + sqrt(w_i^2 + 4 gt_i^2);  s_i = -2 gt_i / d_i (minimised), +2 gt_i / d_i (i = k, order 1), 0 when d_i = 0
  f. |s| > trust: s <- s trust / |s|, bit 1 set; else cleared
  g. dE_pred <- sum gt_i s_i + w_i s_i^2 / 2;  E_prev <- E;  bit 0 set;  r <- r + sum s_i v_i;  t <- v_k (order 1 with t)
"""
import functools

import numpy as np

import _hessian_ref as hr
import _md_ref as mr
import _neb_ref as nr
import _relax_ref as rr
import _vib_ref as vr

RHO_EDGES = (0.25, 0.75, 1.25, 1.75)
DE_FLOOR = 1e-8
MARGIN_MIN = 1e-6  # no decision of a compared run may lie this close (relative) to its threshold


def fresh_state(B, trust_start=0.1, follow=None):
    return dict(trust=np.full(B, float(trust_start)), E_prev=np.zeros(B), dE_pred=np.zeros(B), flags=np.zeros(B, dtype=np.int64),
                t=None if follow is None else np.array(follow, dtype=np.float64))


def hessian_fn(model, rel_noise=0.0, seed=0):
    """Restated (E, F, H) of a model as predict_hessian() returns them; rel_noise: independent normal noise of rel_noise * max|F|
    on every force, rel_noise * max|H| on every Hessian entry and rel_noise * max|E - c| on every energy (a fresh draw per call)."""
    rs = np.random.RandomState(seed)
    c = float(model['c'])

    def fn(R):
        E, F, H = hr.hessian_of_model(model, R)
        if rel_noise:
            F = F + rel_noise * np.abs(F).max() * rs.standard_normal(F.shape)
            H = H + rel_noise * np.abs(H).max() * rs.standard_normal(H.shape)
            E = E + rel_noise * np.abs(E - c).max() * rs.standard_normal(E.shape)
        return E, F, H

    return fn


# Beyond this order the restatement takes LAPACK's eigh with _vib_ref's order and sign conventions instead of the Jacobi
# iteration (eight seconds per 300 x 300 matrix in NumPy, a hundred matrices per parity case).  The step is invariant under the sign of an
# eigenvector, and two solvers differ in an eigenvector by eps |D_s| / gap: on n100_m3, the one fixture beyond (|D_s|_F = 367,
# smallest gap 6.3e-4), 1.3e-10 -- six orders below what the noise of 1e-10 max|H| that defines the bounds does to it
# (tests/test_ef_cpu.py compares the two solvers on that fixture).
JACOBI_MAX_N = 100


def eigensolve(D_s):
    if D_s.shape[0] <= JACOBI_MAX_N:
        return vr.jacobi(D_s)
    w, U = np.linalg.eigh(0.5 * (D_s + D_s.T))
    w, rows = vr.order_and_sign(w, U)
    return w, rows, 0


def spectrum(H, R, f_unit, project):
    """Steps 2 and 3 of one geometry: (w (3N,), V rows, n_rigid, n_neg, sweeps); w as the eigensolver returns it."""
    n3 = len(R)
    D_s, Q, _, _ = vr.shifted(H, R, np.ones(n3 // 3), h_scale=f_unit, project=project)
    w, V, sweeps = eigensolve(D_s)
    k = len(Q)
    tau = n3 * vr.EPS * np.linalg.norm(D_s)
    return w, V, k, int((w[:n3 - k] < -tau).sum()), sweeps


def _rel(x, thr):
    return abs(x - thr) / abs(thr)


def run(hess_fn, R0, fmax, order=1, follow=None, max_steps=100, trust_start=0.1, trust_max=0.3, trust_min=1e-4, project=2,
        state=None, f_unit=1.0, e_offset=0.0):
    """hess_fn(R (B,3N)) -> (E, F, H) scaled as predict_hessian() scales them, called with all B geometries at every evaluation.
    Returns a dict like GDMLPredict.stationary_point's with the frames 'R' of every evaluation, 'trust_hist' and 'flags_hist'
    (the state AFTER each evaluation; a frozen geometry repeats), 'k_follow_hist', and 'margins': per geometry the smallest
    relative distance of a decision from its threshold, by kind ('rho', 'clip', 'fmax', 'floor', 'overlap'; inf where the
    decision never came up)."""
    R = np.array(R0, dtype=np.float64).reshape(-1, np.shape(R0)[-1])
    B, n3 = R.shape
    st = fresh_state(B, trust_start, follow) if state is None else {
        k: (None if v is None else np.array(v)) for k, v in state.items()}
    trust, E_prev, dE_pred, flags, tv = st['trust'], st['E_prev'], st['dE_pred'], st['flags'], st['t']
    active = np.ones(B, dtype=bool)
    conv = np.zeros(B, dtype=bool)
    n_steps = np.full(B, -1, dtype=np.int64)
    E_end, F_end, f_end = np.zeros(B), np.zeros((B, n3)), np.zeros(B)
    w_end, mode_end, w_fol, k_fol = np.zeros((B, n3)), np.zeros((B, n3)), np.zeros(B), np.zeros(B, dtype=np.int64)
    n_rigid, n_neg = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
    hist = {k: [] for k in ('E', 'f', 'w', 'k', 'R', 'trust', 'flags')}
    margins = {k: np.full(B, np.inf) for k in ('rho', 'clip', 'fmax', 'floor', 'overlap')}
    for n in range(max_steps + 1):
        if not active.any():
            break
        E, F, H = hess_fn(R)
        hist['R'].append(R.copy())
        for b in np.nonzero(active)[0]:
            g = -f_unit * F[b]
            w, V, k_r, neg, _ = spectrum(H[b], R[b], f_unit, project)
            nv = n3 - k_r
            f_atom = np.sqrt((g.reshape(-1, 3) ** 2).sum(axis=1)).max()
            k = 0
            if order == 1 and tv is not None:
                ov = np.abs(V[:nv] @ tv[b])
                k = int(np.argmax(ov))  # the first of equal maxima
                top = np.sort(ov)[::-1]
                if nv > 1:
                    margins['overlap'][b] = min(margins['overlap'][b], (top[0] - top[1]) / top[0])
            E_end[b], F_end[b], f_end[b] = E[b], F[b], f_atom
            w_end[b] = np.concatenate([w[:nv], np.zeros(k_r)])
            n_rigid[b], n_neg[b] = k_r, neg
            mode_end[b] = V[k] if order == 1 else 0.0
            w_fol[b], k_fol[b] = w[k], k
            margins['fmax'][b] = min(margins['fmax'][b], _rel(f_atom, fmax))
            if f_atom < fmax or n == max_steps:
                active[b], conv[b], n_steps[b] = False, f_atom < fmax, n
                continue
            if flags[b] & 1:
                floor = DE_FLOOR * max(abs(E[b] - e_offset), abs(E_prev[b] - e_offset)) * f_unit
                margins['floor'][b] = min(margins['floor'][b], _rel(abs(dE_pred[b]), floor))
                if abs(dE_pred[b]) > floor:
                    rho = f_unit * (E[b] - E_prev[b]) / dE_pred[b]
                    margins['rho'][b] = min(margins['rho'][b], min(_rel(rho, e) for e in RHO_EDGES))
                    if rho < 0.25 or rho > 1.75:
                        trust[b] = max(trust[b] / 2.0, trust_min)
                    elif 0.75 < rho < 1.25 and (flags[b] & 2):
                        trust[b] = min(2.0 * trust[b], trust_max)
            gt = V[:nv] @ g
            wv = w[:nv]
            d = np.abs(wv) + np.sqrt(wv * wv + 4.0 * gt * gt)
            s = np.where(d > 0.0, -2.0 * gt / np.where(d > 0.0, d, 1.0), 0.0)
            if order == 1 and nv > 0:
                s[k] = -s[k]
            s_nrm = np.sqrt(np.sum(s * s))
            margins['clip'][b] = min(margins['clip'][b], _rel(s_nrm, trust[b]))
            clip = s_nrm > trust[b]
            if clip:
                s = s * (trust[b] / s_nrm)
            dE_pred[b] = np.sum(gt * s + 0.5 * wv * s * s)
            E_prev[b] = E[b]
            flags[b] = 1 | (2 if clip else 0)
            R[b] = R[b] + s @ V[:nv]
            if order == 1 and tv is not None:
                tv[b] = V[k]
        for key, val in (('E', E_end), ('f', f_end), ('w', w_fol), ('k', k_fol), ('trust', trust), ('flags', flags)):
            hist[key].append(val.copy())
    return dict(R_end=R, E_end=E_end, F_end=F_end, fmax_end=f_end, n_steps=n_steps, converged=conv, w_end=w_end, n_rigid=n_rigid,
                n_neg=n_neg, mode_end=mode_end, E_hist=np.array(hist['E']), fmax_hist=np.array(hist['f']),
                w_follow_hist=np.array(hist['w']), k_follow_hist=np.array(hist['k']), R=np.array(hist['R']),
                trust_hist=np.array(hist['trust']), flags_hist=np.array(hist['flags']),
                state=dict(trust=trust, E_prev=E_prev, dE_pred=dE_pred, flags=flags, t=tv), margins=margins)


def smallest_margin(out):
    return min(float(v.min()) for v in out['margins'].values())


def _deviation(clean, noisy):
    """Largest deviation of every compared quantity between two restated runs; inf where a discrete decision differs."""
    dev = {}
    for k in ('R', 'R_end', 'E_hist', 'fmax_hist', 'w_follow_hist', 'w_end'):
        dev[k] = np.abs(clean[k] - noisy[k]).max() if clean[k].shape == noisy[k].shape else np.inf
    same = all(np.array_equal(clean[k], noisy[k]) for k in ('k_follow_hist', 'flags_hist', 'trust_hist', 'n_steps'))
    if not same:
        dev = {k: np.inf for k in dev}
    for o in (clean, noisy):
        for a in list(o.values()) + list(o['state'].values()) + list(o['margins'].values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return dev


# ---- step-by-step parity on the fixtures

PARITY_FIXTURES = ['n6_p1', 'n5_p4', 'n9_p1', 'n10_p2_pbc', 'cfg1_n21_m100', 'n100_m3']
# (order, with a follow vector)
PARITY_MODES = [(0, False), (1, False), (1, True)]
PARITY_N_EVAL = 6
PARITY_FMAX = 1e-12  # nothing converges
# the trust radius of the parity runs: steps of a few per cent of a bond so that both clipped and free steps occur
PARITY_TRUST = dict(trust_start=0.02, trust_max=0.05, trust_min=1e-4)
# Fixture starts whose run has a decision within MARGIN_MIN of its threshold are replaced here (tests/test_ef_cpu.py prints and
# asserts the margins): fixture -> indices of its seven starts used as geometries 0, 1, 2.
PARITY_STARTS = {}


def parity_start(name):
    model, R7 = mr.case(name)
    idx = PARITY_STARTS.get(name, (0, 1, 2))
    R0 = np.ascontiguousarray(R7[np.array(idx) % len(R7)])
    follow = np.random.RandomState(17).standard_normal(R0.shape)
    return model, R0, follow


def parity_project(model):
    return 1 if 'lattice' in model else 2


@functools.lru_cache(maxsize=None)
def parity_reference(name, order, with_follow):
    """Restated run of three starts of a fixture (PARITY_N_EVAL evaluations; nothing converges) and its sensitivity to the
    predictor's agreed error: the deviation of a second restated run under force and Hessian noise of 1e-10 max and energy
    noise of 1e-10 max|E'|.  The searches are independent, so geometry 0 alone is the B = 1 case.  Computed once per session."""
    model, R0, follow = parity_start(name)
    kw = dict(order=order, follow=follow if with_follow else None, max_steps=PARITY_N_EVAL - 1, project=parity_project(model),
              e_offset=float(model['c']), **PARITY_TRUST)
    clean = run(hessian_fn(model), R0, PARITY_FMAX, **kw)
    noisy = run(hessian_fn(model, rel_noise=1e-10, seed=1), R0, PARITY_FMAX, **kw)
    return model, R0, follow, clean, _deviation(clean, noisy)


# ---- the toy runs to convergence

TOY_JITTER, TOY_SEED = 0.02, 1
TOY_LINE = 0.3
# From TOY_LINE the mode of largest overlap with the line direction is the lowest one at every evaluation (the followed index
# never leaves 0, tests/test_ef_cpu.py prints it); from TOY_TRACK_LINE along the line with TOY_TRACK_JITTER normal jitter it is
# mode 1 at the first two evaluations and mode 0 from the third on, and the trust radius doubles twice on the way.
TOY_TRACK_LINE, TOY_TRACK_JITTER = 0.15, 0.05
TOY_MAX_STEPS = 40


@functools.lru_cache(maxsize=None)
def toy_starts():
    """(model, starts): 'mid' the midpoint of the band toy's two minima with TOY_JITTER normal jitter (RandomState(TOY_SEED));
    'line' the point TOY_LINE along the line between them; 'track' the point TOY_TRACK_LINE along it with TOY_TRACK_JITTER
    jitter; 'dir' the unit line direction."""
    model, A, Bm, _ = nr.toy()
    mid = 0.5 * (A + Bm) + TOY_JITTER * np.random.RandomState(TOY_SEED).standard_normal(A.shape)
    line = A + TOY_LINE * (Bm - A)
    track = A + TOY_TRACK_LINE * (Bm - A) + TOY_TRACK_JITTER * np.random.RandomState(TOY_SEED).standard_normal(A.shape)
    d = (Bm - A) / np.linalg.norm(Bm - A)
    for a in (mid, line, track, d):
        a.setflags(write=False)
    return model, dict(mid=mid, line=line, track=track, dir=d)


def toy_fmax(model, R0, rel=1e-9):
    """rel of the largest atomic force at the start."""
    _, F = mr.force_fn(model)(np.atleast_2d(R0))
    return rel * float(np.sqrt((F.reshape(len(F), -1, 3) ** 2).sum(-1)).max())


# key -> (model of, start, order, with the line direction as follow vector)
TOY_RUNS = {'saddle_mid': ('band', 'mid', 1, False), 'saddle_line': ('band', 'line', 1, True),
            'saddle_track': ('band', 'track', 1, True), 'min_line': ('band', 'line', 0, False), 'min_relax': ('relax', None, 0, False)}


def toy_case(key):
    """(model, R0 (B,3N), follow or None, order, fmax) of a toy run."""
    which, start, order, with_follow = TOY_RUNS[key]
    if which == 'relax':
        model, starts, _, _ = rr.toy()
        R0 = np.array(starts)
    else:
        model, st = toy_starts()
        R0 = np.array(st[start])[None]
    follow = np.array(toy_starts()[1]['dir'])[None] if with_follow else None
    return model, R0, follow, order, toy_fmax(model, R0)


@functools.lru_cache(maxsize=None)
def toy_reference(key):
    """Restated run of a toy case to convergence, and its deviation under noise of 1e-10."""
    model, R0, follow, order, fmax = toy_case(key)
    kw = dict(order=order, follow=follow, max_steps=TOY_MAX_STEPS, e_offset=float(model['c']))
    clean = run(hessian_fn(model), R0, fmax, **kw)
    noisy = run(hessian_fn(model, rel_noise=1e-10, seed=1), R0, fmax, **kw)
    return clean, _deviation(clean, noisy)


# ---- what the GPU test and tools/ef_parity.py measure

PARITY_KEYS = ('R', 'E_hist', 'fmax_hist', 'w_follow_hist')
PARITY_BATCHES = (3, 1)


def parity_chain(name, B):
    """Whether a parity case also runs the chain of one-step calls: the batch of three, except on n100_m3, where an evaluation
    takes most of a second on the device (a 300 x 300 Jacobi in device memory, one workgroup) and the chain would double ten
    more of them on a case that already compares R of every evaluation."""
    return B == 3 and name != 'n100_m3'
BOUND_FACTOR = 10.0  # a compared quantity may deviate by this many times the restatement's own deviation under the noise


def parity_measure(pred, name, order, with_follow, B, chain=False):
    """One parity case on predictor `pred` of the fixture: PARITY_N_EVAL evaluations of the first B starts against the
    restatement.  Returns per quantity of PARITY_KEYS dict(error, sensitivity, ratio) and the flags 'k_follow_equal',
    'trust_equal', 'flags_equal' (the end state; with `chain` also after every single step, from a chain of one-step calls,
    whose end must equal the uncut run's bit for bit: 'chain_equal')."""
    _, R0, follow, clean, dev = parity_reference(name, order, with_follow)
    fol = follow[:B] if with_follow else None
    kw = dict(order=order, **PARITY_TRUST)
    out = pred.stationary_point(R0[:B], PARITY_FMAX, follow=fol, max_steps=PARITY_N_EVAL - 1, record_every=1, **kw)
    m = {}
    for k in PARITY_KEYS:
        err = float(np.abs(out[k] - clean[k][:, :B]).max()) if out[k].shape == clean[k][:, :B].shape else np.inf
        m[k] = dict(error=err, sensitivity=float(dev[k]), ratio=err / float(dev[k]))
    m['k_follow_equal'] = bool(np.array_equal(out['k_follow_hist'], clean['k_follow_hist'][:, :B]))
    m['trust_equal'] = bool(np.array_equal(out['state']['trust'], clean['trust_hist'][-1, :B]))
    m['flags_equal'] = bool(np.array_equal(out['state']['flags'], clean['flags_hist'][-1, :B]))
    m['none_converged'] = bool(not out['converged'].any() and (out['n_steps'] == PARITY_N_EVAL - 1).all())
    if chain:
        R, st = R0[:B], None
        for n in range(PARITY_N_EVAL - 1):
            o = pred.stationary_point(R, PARITY_FMAX, follow=fol if n == 0 else None, state=st, max_steps=1, **kw)
            R, st = o['R_end'], o['state']
            m['trust_equal'] &= bool(np.array_equal(st['trust'], clean['trust_hist'][n, :B]))
            m['flags_equal'] &= bool(np.array_equal(st['flags'], clean['flags_hist'][n, :B]))
            m['k_follow_equal'] &= bool(np.array_equal(o['k_follow_hist'][0], clean['k_follow_hist'][n, :B]))
        m['chain_equal'] = bool(np.array_equal(R, out['R_end']) and all(
            np.array_equal(st[k], out['state'][k]) for k in ('trust', 'E_prev', 'dE_pred', 'flags')) and (
                (st['t'] is None and out['state']['t'] is None) or np.array_equal(st['t'], out['state']['t'])))
    return m

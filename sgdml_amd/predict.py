"""
``GDMLPredict`` with the reference's public interface (sgdml/predict.py:248-1294), evaluated by
the HIP prediction kernels (csrc/predict.hip).  Outputs, scaling (std, c) and the training-set
mode (``predict()`` with cached descriptors, predict.py:1221-1233) follow the reference.
"""
import logging
import re
import sys
import timeit

import numpy as np

from . import _lib
from .utils.desc import Desc


def integration_constant(E_ref, E_pred):
    """The reference's rule for the energy offset c (train.py:1090-1258): the mean of E_ref - E_pred, E_pred predicted at c = 0.
    Shared by GDMLTrain._recov_int_const and GDMLPredict.add_training_points."""
    return np.sum(E_ref - E_pred) / E_ref.shape[0]


def ascend(fun, x0, max_iter=20, gtol=1e-3, bounds=None, max_step=1.0):
    """Quasi-Newton ascent of a smooth function with backtracking: the stepping rule of
    GDMLPredict.optimize_hyperparameters, free of any GPU so that it can be tested on its own.

    fun(x) -> (value, gradient) for a 1-d array x; it may raise numpy.linalg.LinAlgError for a point it cannot evaluate (a
    matrix that is not positive definite), which counts as a failed step and halves the step.  BFGS on the inverse Hessian of
    -fun, started at the identity; a step is at most max_step in the largest component (the variables are logarithms: a factor
    e), projected onto bounds = (lower, upper) arrays, and accepted when the value rises by at least 1e-4 of the predicted
    first-order gain (Armijo); it is halved up to 30 times otherwise.  Ends after max_iter accepted steps, when the largest
    gradient component is at most gtol (components held by a bound do not count), or when no step is accepted.
    Returns (x_best, trace): trace holds one (x, value, gradient) per accepted point, the start included, and x_best is the
    last of them -- the values never decrease along the trace."""
    x = np.array(x0, dtype=np.float64).ravel()
    lo = np.full(x.shape, -np.inf) if bounds is None else np.asarray(bounds[0], dtype=np.float64)
    hi = np.full(x.shape, np.inf) if bounds is None else np.asarray(bounds[1], dtype=np.float64)
    x = np.clip(x, lo, hi)
    f, g = fun(x)
    g = np.asarray(g, dtype=np.float64)
    H = np.eye(x.size)
    trace = [(x.copy(), float(f), g.copy())]
    for _ in range(int(max_iter)):
        free = ~(((x <= lo) & (g < 0.0)) | ((x >= hi) & (g > 0.0)))
        if not free.any() or np.abs(g[free]).max() <= gtol:
            break
        p = H @ g
        if np.dot(p, g) <= 0.0:
            H = np.eye(x.size)
            p = g.copy()
        t = min(1.0, max_step / np.abs(p).max())
        accepted = None
        for _half in range(30):
            xn = np.clip(x + t * p, lo, hi)
            step = xn - x
            if not step.any():
                break
            try:
                fn, gn = fun(xn)
            except np.linalg.LinAlgError:
                t *= 0.5
                continue
            if np.isfinite(fn) and fn >= f + 1e-4 * np.dot(g, step):
                accepted = (xn, float(fn), np.asarray(gn, dtype=np.float64))
                break
            t *= 0.5
        if accepted is None:
            break
        xn, fn, gn = accepted
        sv, yv = xn - x, g - gn
        sy = np.dot(sv, yv)
        if sy > 1e-12 * np.linalg.norm(sv) * np.linalg.norm(yv):
            rho = 1.0 / sy
            V = np.eye(x.size) - rho * np.outer(sv, yv)
            H = V @ H @ V.T + rho * np.outer(sv, sv)
        else:
            H = np.eye(x.size)
        x, f, g = xn, fn, gn
        trace.append((x.copy(), f, g.copy()))
    return x, trace


def _cofactors3(lat):
    """Transposed cofactors (adjugate, row-major) and determinant of a 3 x 3 array, on Python floats: a per-call lattice sits
    in the single-geometry latency path, where numpy.linalg.inv / det / matrix_rank cost half of the whole call."""
    (a, b, c), (d, e, f), (g, h, i) = lat.tolist()
    adj = (e * i - f * h, c * h - b * i, b * f - c * e,
           f * g - d * i, a * i - c * g, c * d - a * f,
           d * h - e * g, b * g - a * h, a * e - b * d)
    return adj, a * adj[0] + b * adj[3] + c * adj[6], max(abs(v) for v in (a, b, c, d, e, f, g, h, i))


def det3(lat):
    """Determinant of a 3 x 3 array."""
    return _cofactors3(lat)[1]


def check_lattice(lattice):
    """(lattice, inverse) as float64 for a per-call lattice: 3 x 3, cell vectors in the COLUMNS (the reference's convention,
    desc.py:44-77); ValueError for any other shape, non-finite entries or a singular matrix (|det| at most 1e-12 of the cube
    of the largest entry).  The inverse is adjugate / det (it only feeds the rounding to the minimum image)."""
    lat = np.array(lattice, dtype=np.float64)
    if lat.shape != (3, 3):
        raise ValueError('lattice must be a 3 x 3 matrix (cell vectors in its columns), got shape {}'.format(lat.shape))
    adj, det, big = _cofactors3(lat)
    if not (big < float('inf') and abs(det) > 1e-12 * big ** 3):  # (a NaN fails both comparisons)
        raise ValueError('lattice is singular or not finite')
    return lat, np.array(adj, dtype=np.float64).reshape(3, 3) / det


# ---- input checks and result conversion shared by run_md(), run_pimd() and relax()

def _as_batch(A, n3=None):
    """(B,3N), (3N,) or (B,N,3) -> (B,3N) float64; with n3, anything else is a ValueError naming R0."""
    A = np.asarray(A, dtype=np.float64)
    if A.ndim == 1:
        A = A[None, :]
    if A.ndim == 3:
        A = A.reshape(A.shape[0], -1)
    if n3 is not None and (A.ndim != 2 or A.shape[1] != n3):
        raise ValueError('R0 must be (B, {}) for this model, got shape {}'.format(n3, A.shape))
    return A


def _check_finite(*named):
    for name, val in named:
        if not np.isfinite(val):
            raise ValueError('{} must be finite'.format(name))


def _record_fields(record, known):
    record = (record,) if isinstance(record, str) else tuple(record)
    for k in record:
        if k not in known:
            raise ValueError('record names an unknown field {!r} (known: {})'.format(k, ', '.join(map(repr, known))))
    return record


def _raise_first_bad(bad, noun, unit):
    if (bad >= 0).any():
        b = int(np.argmax(bad >= 0))
        raise FloatingPointError('{} {} stopped being finite at {} {}'.format(noun, b, unit, int(bad[b])))


def _fire_checks(fmax, dt_start, dt_max, max_step, f_inc, f_dec, alpha_start, f_alpha, f_unit, n_min, max_steps, record_every,
                 after_fmax=(), more=(), positive=None):
    """The checks relax(), relax_cell() and neb() share, in their order.  after_fmax, more: the entry's own (name, value)
    pairs for the finite check; positive: a (name, value) that must be > 0.  Returns dt_max (None: 10 dt_start)."""
    if dt_max is None:
        dt_max = 10.0 * dt_start
    _check_finite(('fmax', fmax), *after_fmax, ('dt_start', dt_start), ('dt_max', dt_max), ('max_step', max_step),
                  ('f_inc', f_inc), ('f_dec', f_dec), ('alpha_start', alpha_start), ('f_alpha', f_alpha), ('f_unit', f_unit), *more)
    if positive is not None and not positive[1] > 0.0:
        raise ValueError('{} must be positive'.format(positive[0]))
    if int(max_steps) != max_steps or int(record_every) != record_every or int(n_min) != n_min:
        raise ValueError('max_steps, record_every and n_min must be integers')
    return dt_max


def _fire_state(state, B, v_shape, dt_start, alpha_start, shapes, more_keys=()):
    """A fresh FIRE state (state None; V zeros of v_shape), or the caller's, checked: no key missing, then the shapes
    ((key, shape, message with {} for the shape wanted and the shape found), ...), then finite V, dt, alpha."""
    if state is None:
        return dict(V=np.zeros(v_shape), dt=np.full(B, float(dt_start)), alpha=np.full(B, float(alpha_start)),
                    n_pos=np.zeros(B, dtype=np.int64), n_taken=np.zeros(B, dtype=np.int64))
    missing = [k for k in more_keys + ('V', 'dt', 'alpha', 'n_pos', 'n_taken') if k not in state]
    if missing:
        raise ValueError('state lacks {}'.format(missing))
    for k, shp, msg in shapes:
        if np.shape(state[k]) != shp:
            raise ValueError(msg.format(shp, np.shape(state[k])))
    if not all(np.isfinite(np.asarray(state[k], dtype=np.float64)).all() for k in ('V', 'dt', 'alpha')):
        raise ValueError('state must be finite')
    return state


class GDMLPredict(object):
    def __init__(
        self,
        model,
        batch_size=None,
        num_workers=None,
        max_memory=None,
        max_processes=None,
        use_torch=False,
        log_level=None,
        _borrow_ctx=None,
        devices=None,
    ):
        """devices (no counterpart in the reference's signature; its torch path wraps the model in nn.DataParallel over every
        visible GPU, predict.py:375-378): list of GPU indices to replicate the model on -- query batches are then split over
        them (replicas + query sharding).  None: every visible GPU when `use_torch` is set (what the reference
        does), else GPU 0 only."""
        self.log = logging.getLogger(__name__)
        if log_level is not None:
            self.log.setLevel(log_level)

        if 'type' not in model or not (model['type'] == 'm' or model['type'] == b'm'):
            self.log.critical('The provided data structure is not a valid model.')
            sys.exit()

        self.n_atoms = model['z'].shape[0]
        self.desc = Desc(self.n_atoms, max_processes=max_processes)

        self.R_desc = None
        self.R_d_desc = None

        self.lat_and_inv = (
            (np.asarray(model['lattice'], dtype=np.float64), np.linalg.inv(model['lattice']))
            if 'lattice' in model
            else None
        )

        R_desc_train = np.ascontiguousarray(np.asarray(model['R_desc'], dtype=np.float64).T)  # stored D x M
        self.n_train = R_desc_train.shape[0]
        self.sig = float(model['sig'])
        self.std = float(model['std']) if 'std' in model else 1.0
        self.c = float(model['c'])
        self.n_perms = np.asarray(model['perms']).shape[0]
        self.tril_perms_lin = np.asarray(model['tril_perms_lin'])
        self._tril_perms = _lib.tril_perms_from_lin(self.tril_perms_lin, self.desc.dim)

        # parameters of the reference's CPU pool; accepted and ignored (no pools on the GPU path)
        self.max_memory, self.max_processes = max_memory, max_processes
        self.use_torch = use_torch
        self.bulk_mp, self.num_workers, self.chunk_size = False, 0, self.n_train
        self.pool = None

        # _borrow_ctx (internal): evaluate on a context somebody else owns -- the trainer's, for the short-lived predictors of
        # GDMLTrain._recov_int_const and sweep.sigma_sweep.  The model tables of a context belong to whoever uploaded last.
        self._owns_ctx = _borrow_ctx is None
        if devices is None:
            devices = list(range(_lib.device_count())) if (use_torch and _borrow_ctx is None) else [0]
        devices = [int(d) for d in devices] or [0]
        self._ctx = _lib.Context(devices[0]) if _borrow_ctx is None else _borrow_ctx
        # replicas on the other devices (one context per entry: the same index twice gives two contexts on one GPU, which is
        # how the sharded path is tested on a one-GPU box); the training-set mode and set_alphas stay on the first one
        self._replicas = [] if _borrow_ctx is not None else [_lib.Context(d) for d in devices[1:]]
        for ctx in [self._ctx] + self._replicas:
            ctx.predict_upload_model(
                R_desc_train,
                model['R_d_desc_alpha'],
                self._tril_perms,
                self.sig,
                model['alphas_E'] if 'alphas_E' in model else None,
            )
        self._replicas_stale = False
        self._min_shard = 64  # geometries per device below which a batch is not worth splitting
        self._min_shard_hessian = 4  # the same for predict_hessian (one Hessian is the arithmetic of ~10 predictions)
        self._train_resident = False

        # posterior covariances (prepare_uncertainty): what the factorisation needs beyond the prediction tables
        self._R_desc_train = R_desc_train
        self._lam = float(model['lam']) if 'lam' in model else None
        self._use_E_cstr = bool(model['use_E_cstr']) if 'use_E_cstr' in model else 'alphas_E' in model
        self._alphas_F = np.asarray(model['alphas_F'], dtype=np.float64).ravel() if 'alphas_F' in model else None
        self.uncertainty_scale = 1.0
        # add_training_points / export_model: the model's other keys, J alpha, and what prepare_uncertainty(R, F) leaves behind
        # (Cartesian geometries, compressed Jacobians and normalised labels of the training set)
        self._model = dict(model)
        self._R_d_desc_alpha = np.asarray(model['R_d_desc_alpha'], dtype=np.float64)
        self._unc_R = self._unc_gd = self._unc_y = None
        # idxs_train as export_model writes it once the training set was edited (-1 for added points, removed entries dropped)
        self._idxs_train = np.asarray(model['idxs_train']).astype(np.int64) if 'idxs_train' in model else None
        self._edited = False
        self._unc_prepared = False  # the factor of prepare_uncertainty() is resident (optimize_hyperparameters restores it)
        self._hyper_edited = False  # optimize_hyperparameters moved sig / lam: export_model writes them

    def __del__(self):
        for ctx in getattr(self, '_replicas', []):
            ctx.close()
        ctx = getattr(self, '_ctx', None)
        if ctx is not None and getattr(self, '_owns_ctx', True):
            ctx.close()

    def _sharded(self, n_items, fn, min_shard=None):
        """fn(ctx, lo, hi) for contiguous query shards, one per device, concurrently (ctypes releases the GIL inside the
        library calls); results in shard order.  One shard when the batch is small or the replicas do not hold the current
        coefficients (set_alphas re-targets only the first context)."""
        ctxs = [self._ctx] + ([] if self._replicas_stale else self._replicas)
        n_sh = min(len(ctxs), max(1, n_items // (self._min_shard if min_shard is None else min_shard)))
        if n_sh <= 1:
            return [fn(self._ctx, 0, n_items)]
        import threading

        cuts = [n_items * k // n_sh for k in range(n_sh + 1)]
        out, err = [None] * n_sh, []

        def run(k):
            try:
                out[k] = fn(ctxs[k], cuts[k], cuts[k + 1])
            except BaseException as e:  # re-raised in the caller's thread
                err.append(e)

        ths = [threading.Thread(target=run, args=(k,)) for k in range(1, n_sh)]
        for t in ths:
            t.start()
        run(0)
        for t in ths:
            t.join()
        if err:
            raise err[0]
        return out

    # ---- training-mode hooks (predict.py:510-601)

    def set_R_desc(self, R_desc):
        self.R_desc = R_desc
        self._train_resident = False

    def set_R_d_desc(self, R_d_desc):
        self.R_d_desc = R_d_desc
        self._train_resident = False

    def _ensure_train_resident(self):
        if self._train_resident:
            return
        if self.R_d_desc is None:
            raise AssertionError('set_R_d_desc() must be called first')
        R_desc = self.R_desc
        if R_desc is None:
            raise AssertionError('set_R_desc() must be called first')
        self._ctx.train_upload(R_desc, self.R_d_desc, self._tril_perms)
        self._train_resident = True

    def set_alphas(self, alphas_F, alphas_E=None):
        """Re-target the model with new coefficients (predict.py:551-601); J alpha runs on the GPU."""
        self._ensure_train_resident()
        self._ctx.set_alphas(alphas_F, alphas_E)
        self._replicas_stale = True  # the replicas still hold the constructor's coefficients

    # ---- CPU-tuning API of the reference: no-ops here, like its torch path (predict.py:826-830)

    def prepare_parallel(self, n_bulk=1, n_reps=1, return_is_from_cache=False):
        return None

    def set_opt_num_workers_and_batch_size_fast(self, n_bulk=1, n_reps=1):
        return None

    def _set_num_workers(self, num_workers=None, force_reset=False):
        self.num_workers = 0

    def _set_chunk_size(self, chunk_size=None):
        self.chunk_size = self.n_train

    def _set_batch_size(self, batch_size=None):
        self._set_chunk_size(batch_size)

    def _set_bulk_mp(self, bulk_mp=False):
        self.bulk_mp = False

    def get_GPU_batch(self):
        return self.n_train

    # ---- test / validation errors on the device (the loop body of sgdml/cli.py:1564-1605)

    def test_errors(self, R, F, E=None):
        """MAE / RMSE of energies, force components, force magnitudes and normalised force angles
        for labelled geometries, with the reference's definitions (cli.py:_online_err :1170).
        Predictions never leave the GPU.  Returns a dict of (mae, rmse) pairs."""
        R = np.asarray(R, dtype=np.float64)
        if R.ndim == 1:
            R = R[None, :]
        B = R.shape[0]
        R = R.reshape(B, -1)
        F = np.asarray(F, dtype=np.float64).reshape(B, -1)
        E = None if E is None else np.asarray(E, dtype=np.float64).reshape(B)
        parts = self._sharded(B, lambda ctx, lo, hi: ctx.predict_errors(
            R[lo:hi], F[lo:hi], None if E is None else E[lo:hi], std=self.std, c=self.c, lat_and_inv=self.lat_and_inv))
        s = np.sum(np.asarray(parts, dtype=np.float64), axis=0)  # the eight sums are additive over query shards
        n_f, n_a = B * 3 * self.n_atoms, B * self.n_atoms
        out = {
            'force': (s[2] / n_f, np.sqrt(s[3] / n_f)),
            'magnitude': (s[4] / n_a, np.sqrt(s[5] / n_a)),
            'angle': (s[6] / n_a, np.sqrt(s[7] / n_a)),
        }
        if E is not None:
            out['energy'] = (s[0] / B, np.sqrt(s[1] / B))
        return out

    # ---- prediction

    def _lat_and_inv(self, lattice):
        """The lattice of one call: the model's (or none) by default, else the validated per-call one."""
        if lattice is None:
            return self.lat_and_inv
        lat_and_inv = check_lattice(lattice)
        if self.lat_and_inv is not None and np.array_equal(lat_and_inv[0], self.lat_and_inv[0]):
            return self.lat_and_inv  # the model's own cell: its stored inverse, hence the bits of the default
        return lat_and_inv

    @staticmethod
    def _lats_and_invs(lattices, B, lattice=None):
        """Per-geometry lattices (B,3,3), cell vectors in the columns, and their inverses: each member validated like a
        per-call lattice (check_lattice); mutually exclusive with lattice=."""
        if lattice is not None:
            raise ValueError('give either lattice (one for the call) or lattices (one per geometry), not both')
        lats = np.array(lattices, dtype=np.float64)
        if lats.shape != (B, 3, 3):
            raise ValueError('lattices must be ({}, 3, 3), one 3 x 3 matrix per geometry, got shape {}'.format(B, lats.shape))
        invs = np.empty_like(lats)
        for b in range(B):
            try:
                invs[b] = check_lattice(lats[b])[1]
            except ValueError as e:
                raise ValueError('lattices[{}]: {}'.format(b, e))
        return lats, invs

    def _cells(self, R, lattices, lattice, return_E=True, virial=True):
        """Unscaled (E, F, W, lattices) of geometries R with one lattice each (gdml_predict_virial_cells)."""
        if R is None:
            raise ValueError('per-geometry lattices need geometries R (there is no training-set mode)')
        R = np.asarray(R, dtype=np.float64)
        if R.ndim == 1:
            R = R[None, :]
        R = R.reshape(R.shape[0], -1)
        lats, invs = self._lats_and_invs(lattices, R.shape[0], lattice)
        parts = self._sharded(R.shape[0], lambda ctx, lo, hi: ctx.predict_cells(R[lo:hi], lats[lo:hi], invs[lo:hi],
                                                                                return_E=return_E, virial=virial))
        E, F, W = (parts[0] if len(parts) == 1 else
                   [None if parts[0][i] is None else np.concatenate([p_[i] for p_ in parts]) for i in range(3)])
        return E, F, W, lats

    def predict_hessian(self, R, lattice=None):
        """Energies (B,), forces (B,3N) and analytic Hessians d^2E/dR^2 (B,3N,3N) for geometries R (B,3N) or (3N,),
        scaled like predict() (E std + c, F std, H std).  No training-set mode: R is required.  lattice: as in predict()."""
        if R is None:
            raise ValueError('predict_hessian needs geometries R (there is no training-set mode)')
        R = np.asarray(R, dtype=np.float64)
        if R.ndim == 1:
            R = R[None, :]
        R = R.reshape(R.shape[0], -1)
        lat_and_inv = self._lat_and_inv(lattice)
        parts = self._sharded(R.shape[0], lambda ctx, lo, hi: ctx.predict_hessian(R[lo:hi], lat_and_inv),
                              min_shard=self._min_shard_hessian)
        E, F, H = (parts[0] if len(parts) == 1 else [np.concatenate([p_[i] for p_ in parts]) for i in range(3)])
        E *= self.std
        E += self.c
        F *= self.std
        H *= self.std
        return E, F, H

    # ---- strain derivative and stress (gdml_predict_virial, csrc/predict.hip)

    def predict_virial(self, R, lattice=None, lattices=None):
        """Energies (B,), forces (B,3N) and the strain derivative W = dE/d eps (B,3,3) for geometries R (B,3N) or (3N,): the
        change of the energy when atoms and cell are strained together, r -> (I + eps) r, lattice -> (I + eps) lattice.  E and
        F are those of predict(R, lattice=lattice), bit for bit; W is symmetric and scaled by std like F.  Works for
        non-periodic models too (W = -sum_i f_i (x) r_i there).  lattice, lattices: as in predict().  No training-set mode."""
        if lattices is not None:
            return self._scaled(*self._cells(R, lattices, lattice)[:3])
        return self._virial(R, self._lat_and_inv(lattice))

    def _scaled(self, E, F, W):
        E *= self.std
        E += self.c
        F *= self.std
        W *= self.std
        return E, F, W

    def _virial(self, R, lat_and_inv):
        if R is None:
            raise ValueError('predict_virial needs geometries R (there is no training-set mode)')
        R = np.asarray(R, dtype=np.float64)
        if R.ndim == 1:
            R = R[None, :]
        R = R.reshape(R.shape[0], -1)
        parts = self._sharded(R.shape[0], lambda ctx, lo, hi: ctx.predict_virial(R[lo:hi], lat_and_inv))
        return self._scaled(*(parts[0] if len(parts) == 1 else [np.concatenate([p_[i] for p_ in parts]) for i in range(3)]))

    def predict_stress(self, R, lattice=None, voigt=False, lattices=None):
        """(E, F, S) with the stress S = W / |det lattice| (B,3,3) of predict_virial: +dE/d eps per volume, ASE's sign, in the
        model's energy unit per length unit cubed.  voigt=True: S (B,6) in ASE's order xx, yy, zz, yz, xz, xy.  lattices: one
        lattice per geometry as in predict(); each W is divided by its own geometry's volume.  ValueError when neither the
        model nor the call supplies a lattice (a volume)."""
        if lattices is not None:
            E, F, W, lats = self._cells(R, lattices, lattice)
            E, F, W = self._scaled(E, F, W)
            W /= np.array([abs(det3(lat)) for lat in lats]).reshape(-1, 1, 1)
        else:
            lat_and_inv = self._lat_and_inv(lattice)
            if lat_and_inv is None:
                raise ValueError('predict_stress needs a lattice: the model has none and none was given')
            E, F, W = self._virial(R, lat_and_inv)
            W /= abs(det3(lat_and_inv[0]))
        if voigt:
            W = np.ascontiguousarray(W.reshape(-1, 9)[:, [0, 4, 8, 5, 2, 1]])
        return E, F, W

    # ---- molecular dynamics on the device (gdml_md_run, csrc/md.hip)

    def run_md(self, R0, V0, masses, dt, n_steps, record_every=1, thermostat=None, gamma=0.0, kT=0.0, seed=0, step0=0,
               lattice=None, f_unit=1.0, record=('R', 'E')):
        """Advance B independent replicas of the molecule for n_steps on the device: velocity Verlet (thermostat=None) or
        Langevin BAOAB (thermostat='langevin', friction gamma, temperature kT in the units of mass * velocity^2).  R0, V0:
        (B,3N) or (3N,); masses (N,); accelerations are f_unit * F / mass with F the forces of predict().  seed and the
        absolute step counter step0 fix the noise (a run continued from R_end, V_end with step0 = step_end draws the
        continuation of the stream and equals the uninterrupted run bit for bit).  lattice: as in predict().
        record: which of 'R', 'V', 'F', 'E' to return for every record_every-th step.  Returns a dict: those of 'R', 'V', 'F'
        (n_rec,B,3N; F scaled by std), 'E_pot' (n_rec,B; E std + c as predict() scales it) and 'E_kin' (n_rec,B), the end
        state 'R_end', 'V_end' (B,3N) and 'step_end' = step0 + n_steps.  Runs on the predictor's first device.
        ValueError for non-finite or misshapen input before anything is launched; FloatingPointError naming replica and step
        when a trajectory stops being finite."""
        n3 = 3 * self.n_atoms
        R0, V0 = _as_batch(R0, n3), _as_batch(V0)
        if V0.shape != R0.shape:
            raise ValueError('V0 must have the shape of R0 {}, got {}'.format(R0.shape, V0.shape))
        masses = np.asarray(masses, dtype=np.float64)
        if masses.shape != (self.n_atoms,):
            raise ValueError('masses must be ({},), got shape {}'.format(self.n_atoms, masses.shape))
        if not (np.isfinite(R0).all() and np.isfinite(V0).all() and np.isfinite(masses).all()):
            raise ValueError('R0, V0 and masses must be finite')
        _check_finite(('dt', dt), ('gamma', gamma), ('kT', kT), ('f_unit', f_unit))
        if thermostat not in (None, 'langevin'):
            raise ValueError("thermostat must be None or 'langevin', got {!r}".format(thermostat))
        record = _record_fields(record, ('R', 'V', 'F', 'E'))
        seed, step0 = int(seed), int(step0)
        if not 0 <= seed < 2**64:
            raise ValueError('seed must fit into 64 unsigned bits')
        lat_and_inv = self._lat_and_inv(lattice)
        out = self._ctx.md_run(R0, V0, masses, dt, n_steps, record_every, f_scale=self.std * float(f_unit),
                               thermostat=0 if thermostat is None else 1, gamma=gamma, kT=kT, seed=seed, step0=step0,
                               lat_and_inv=lat_and_inv, record=record)
        _raise_first_bad(out.pop('first_bad_step'), 'replica', 'step')
        if 'F' in out:
            out['F'] *= self.std
        E = out.pop('E')
        E *= self.std
        E += self.c
        out['E_pot'] = E
        out['E_kin'] = out.pop('Ekin')
        out['step_end'] = step0 + int(n_steps)
        return out

    # ---- constant-pressure molecular dynamics on the device (gdml_npt_run, csrc/npt.hip)

    @staticmethod
    def piston_mass(n_atoms, kT, tau):
        """The piston mass (3N + 3) kT tau^2 that gives the cell of N atoms at temperature kT the period scale tau."""
        return (3 * int(n_atoms) + 3) * float(kT) * float(tau) ** 2

    def run_npt(self, R0, V0, masses, dt, n_steps, pressure, piston_mass, record_every=1, thermostat=None, gamma=0.0,
                gamma_baro=0.0, kT=0.0, seed=0, step0=0, lattice=None, lattices=None, state=None, f_unit=1.0,
                record=('R', 'E')):
        """Advance B independent replicas of a PERIODIC model for n_steps at the external pressure on the device: isotropic
        Martyna-Tobias-Klein dynamics of atoms and cell, the cell of replica b being exp(eps_b) L0_b.  thermostat=None is NPH
        (it conserves 'enthalpy'); thermostat='langevin' is NPT with a Langevin piston: friction gamma on the particles and
        gamma_baro on the piston at temperature kT, which samples the isothermal-isobaric ensemble.  R0, V0, masses, dt, seed,
        step0, f_unit, record_every: as in run_md().  pressure: in (f_unit * the model's energy unit) / length^3.
        piston_mass: in energy * time^2 (piston_mass(N, kT, tau) gives the usual choice; inf freezes the cell and the run is
        run_md()'s general route bit for bit).  lattice: one 3 x 3 reference lattice L0 (cell vectors in the columns) for all
        replicas, default the model's; lattices: (B,3,3), one per replica.  state: the 'state' of an earlier call ({'eps',
        'p_eps', 'L0'}) passed with its R_end, V_end and step0 = step_end continues that run bit for bit (the lattice arguments
        are then not used); None starts at eps = 0, p_eps = 0.
        record: which of 'R', 'V', 'F', 'lattice', 'E' to return per recorded step.  Returns a dict: those of 'R', 'V', 'F'
        (n_rec,B,3N; F scaled by std) and 'lattice' (n_rec,B,3,3); always 'E_pot' (n_rec,B; scaled like predict()), 'E_kin',
        'vol', 'pressure' (the internal pressure (2 E_kin - f_unit tr W) / (3 vol)), 'p_eps' and 'enthalpy' = E_kin + f_unit
        E_pot + pressure vol + p_eps^2 / (2 piston_mass); the end state 'R_end', 'V_end', 'lattice_end', 'vol_end',
        'step_end' and 'state'.  Runs on the predictor's first device, always on the general prediction route.
        Not offered: anisotropic or fully flexible cells, per-replica pressures, removal of the centre-of-mass momentum.
        ValueError before anything is launched; FloatingPointError naming replica and step when a trajectory stops being
        finite (a cell that collapses or blows up included)."""
        n3 = 3 * self.n_atoms
        R0, V0 = _as_batch(R0, n3), _as_batch(V0)
        B = R0.shape[0]
        if V0.shape != R0.shape:
            raise ValueError('V0 must have the shape of R0 {}, got {}'.format(R0.shape, V0.shape))
        masses = np.asarray(masses, dtype=np.float64)
        if masses.shape != (self.n_atoms,):
            raise ValueError('masses must be ({},), got shape {}'.format(self.n_atoms, masses.shape))
        if not (np.isfinite(R0).all() and np.isfinite(V0).all() and np.isfinite(masses).all()):
            raise ValueError('R0, V0 and masses must be finite')
        _check_finite(('dt', dt), ('gamma', gamma), ('gamma_baro', gamma_baro), ('kT', kT), ('f_unit', f_unit),
                      ('pressure', pressure))
        if not float(piston_mass) > 0.0:  # (a NaN fails the comparison; inf passes)
            raise ValueError('piston_mass must be positive (inf freezes the cell)')
        if thermostat not in (None, 'langevin'):
            raise ValueError("thermostat must be None or 'langevin', got {!r}".format(thermostat))
        record = _record_fields(record, ('R', 'V', 'F', 'lattice', 'E'))
        seed, step0 = int(seed), int(step0)
        if not 0 <= seed < 2**64:
            raise ValueError('seed must fit into 64 unsigned bits')
        if state is None:
            if lattices is not None:
                L0, L0_inv = self._lats_and_invs(lattices, B, lattice)
            else:
                lat_and_inv = self._lat_and_inv(lattice)
                if lat_and_inv is None:
                    raise ValueError('run_npt needs a lattice: the model has none and none was given')
                L0, L0_inv = (np.broadcast_to(a, (B, 3, 3)) for a in lat_and_inv)
            eps, p_eps = np.zeros(B), np.zeros(B)
        else:
            for k in ('eps', 'p_eps', 'L0'):
                if k not in state:
                    raise ValueError("state lacks '{}'".format(k))
            eps, p_eps = (np.array(state[k], dtype=np.float64) for k in ('eps', 'p_eps'))
            L0 = np.array(state['L0'], dtype=np.float64)
            if eps.shape != (B,) or p_eps.shape != (B,) or L0.shape != (B, 3, 3):
                raise ValueError("state must hold 'eps' and 'p_eps' of shape ({0},) and 'L0' of shape ({0}, 3, 3)".format(B))
            if not (np.isfinite(eps).all() and np.isfinite(p_eps).all()):
                raise ValueError("state['eps'] and state['p_eps'] must be finite")
            # the inverse that the run which made this state used: the model's stored one for the model's own cell
            L0_inv = np.empty_like(L0)
            for b in range(B):
                try:
                    L0_inv[b] = self._lat_and_inv(L0[b])[1]
                except ValueError as e:
                    raise ValueError("state['L0'][{}]: {}".format(b, e))
        rec = tuple({'lattice': 'lat', 'E': None}.get(k, k) for k in record)
        out = self._ctx.npt_run(R0, V0, eps, p_eps, L0, L0_inv, masses, dt, n_steps, pressure, piston_mass,
                                record_every=record_every, f_scale=self.std * float(f_unit),
                                thermostat=0 if thermostat is None else 1, gamma=gamma, gamma_baro=gamma_baro, kT=kT, seed=seed,
                                step0=step0, record=rec)
        _raise_first_bad(out.pop('first_bad_step'), 'replica', 'step')
        if 'F' in out:
            out['F'] *= self.std
        if 'lat' in out:
            out['lattice'] = out.pop('lat')
        E = out.pop('E')
        E *= self.std
        E += self.c
        out['E_pot'] = E
        out['E_kin'] = out.pop('Ekin')
        out['pressure'] = out.pop('press')
        p = out['p_eps'] = out.pop('peps')
        out['enthalpy'] = out['E_kin'] + float(f_unit) * E + float(pressure) * out['vol'] + p * p / (2.0 * float(piston_mass))
        eps_end = out.pop('eps_end')
        L0 = np.array(L0, dtype=np.float64)
        lam = np.exp(eps_end)
        out['lattice_end'] = lam[:, None, None] * L0
        out['vol_end'] = lam * lam * lam * np.abs(np.array([det3(L) for L in L0]))
        out['state'] = dict(eps=eps_end, p_eps=out.pop('p_eps_end'), L0=L0)
        out['step_end'] = step0 + int(n_steps)
        return out

    # ---- geometry relaxation on the device (gdml_relax_run, csrc/relax.hip)

    def relax(self, R0, fmax, max_steps=1000, dt_start=0.1, dt_max=None, max_step=0.2, n_min=5, f_inc=1.1, f_dec=0.5,
              alpha_start=0.1, f_alpha=0.99, state=None, lattice=None, f_unit=1.0, record_every=0):
        """Minimise the energy of B independent geometries on the device by FIRE (Bitzek et al., PRL 97, 170201 (2006)) in the
        form ASE's FIRE uses: unit masses, gradient g = f_unit * F with F the forces of predict(), the whole step clipped to
        max_step.  R0: (B,3N) or (3N,).  A geometry is converged when its largest atomic |g| is below fmax; every geometry
        takes at most max_steps steps in this call and stops on its own (the others run on).  dt_max=None: 10 dt_start.
        state: the 'state' of an earlier call ({'V', 'dt', 'alpha', 'n_pos', 'n_taken'}), passed back together with its R_end,
        continues that run bit for bit; None is a fresh start.  lattice: as in predict() (the cell is fixed, positions are not
        wrapped).  record_every > 0 also returns 'R' (every record_every-th evaluated geometry, the start included).
        Returns a dict: 'R_end' (B,3N), 'E_end' (B) and 'F_end' (B,3N) scaled like predict(), 'fmax_end' (B), 'n_steps' (B; steps
        taken in this call), 'converged' (B, bool), 'E_hist' and 'fmax_hist' (evaluations made, B; a geometry that has stopped
        repeats its last value) and 'state'.  Runs on the predictor's first device.  ValueError for non-finite or out-of-range
        parameters and misshapen input before anything is launched; FloatingPointError naming geometry and evaluation when a
        value is not finite (a NaN in R0 included: evaluation 0)."""
        n3 = 3 * self.n_atoms
        R0 = _as_batch(R0, n3)
        B = R0.shape[0]
        dt_max = _fire_checks(fmax, dt_start, dt_max, max_step, f_inc, f_dec, alpha_start, f_alpha, f_unit, n_min, max_steps,
                              record_every)
        state = _fire_state(state, B, R0.shape, dt_start, alpha_start,
                            (('V', R0.shape, "state['V'] must have the shape of R0 {}, got {}"),))
        # a NaN start is not a usage error: the run reports the geometry and the evaluation (FloatingPointError)
        out = self._ctx.relax_run(R0, fmax, max_steps, state, dt_max, max_step=max_step, n_min=n_min, f_inc=f_inc, f_dec=f_dec,
                                  alpha_start=alpha_start, f_alpha=f_alpha, f_scale=self.std * float(f_unit),
                                  record_every=record_every, lat_and_inv=self._lat_and_inv(lattice))
        return self._frozen_result(out, 'geometry', ('E_end', 'E_hist'))

    def _frozen_result(self, out, noun, energy_keys):
        """What relax(), relax_cell(), neb() and stationary_point() make of their entry's result: the first non-finite value
        is an error naming the `noun`; 'status' becomes 'n_steps', 'converged' and 'fmax_end'; 'F_end' and the energy_keys
        are scaled like predict()."""
        _raise_first_bad(out.pop('first_bad_step'), noun, 'evaluation')
        status = out.pop('status')
        out.pop('n_made')
        out['F_end'] *= self.std
        for k in energy_keys:
            out[k] *= self.std
            out[k] += self.c
        out['n_steps'] = status[:, 1].copy()
        out['converged'] = status[:, 0] == 1
        out['fmax_end'] = out['fmax_hist'][status[:, 1], np.arange(len(status))] if len(status) else np.empty(0)
        return out

    # ---- variable-cell relaxation on the device (gdml_cell_relax_run, csrc/cellrelax.hip)

    def relax_cell(self, R0, fmax, lattice=None, lattices=None, pressure=0.0, mask=None, cell_factor=None, max_steps=1000,
                   dt_start=0.1, dt_max=None, max_step=0.2, n_min=5, f_inc=1.1, f_dec=0.5, alpha_start=0.1, f_alpha=0.99,
                   state=None, f_unit=1.0, record_every=0):
        """Relax atoms AND cell of B independent periodic geometries on the device by FIRE, in the form of ASE's
        FIRE(UnitCellFilter(atoms)): the enthalpy H = f_unit * E + pressure * volume is minimised over the atoms' reference
        positions s and the deformation gradient Fd of the cell (positions Fd s, lattice Fd L0), one FIRE system of 3N + 9
        coordinates (s, cell_factor * Fd) per geometry; the FIRE parameters are relax()'s.  R0: (B,3N) or (3N,).  lattice: one
        3 x 3 start lattice (cell vectors in the columns) for all starts, default the model's; lattices: (B,3,3), one per
        start.  pressure: in (f_unit * the model's energy unit) / length^3.  mask: symmetric 3 x 3 of 0/1, the strain components
        that relax (default all; [[1,1,0],[1,1,0],[0,0,0]] relaxes a slab in its plane only).  cell_factor: default N, as in ASE.
        A geometry is converged when the largest row norm of the generalised force -- the atoms' Fd^T g and the three rows of
        -(mask o (f_unit W + pressure V I)) Fd^-T / cell_factor -- is below fmax.  state: the 'state' of an earlier call continues
        that run bit for bit (R0 then only fixes the batch size; the lattice arguments are not used).
        Returns a dict like relax()'s: 'R_end' (B,3N), 'lattice_end' (B,3,3), 'E_end', 'F_end' scaled like predict(),
        'stress_end' (B,3,3; W / volume scaled by std, ASE's sign, WITHOUT the external pressure), 'vol_end' (B), 'fmax_end',
        'n_steps', 'converged', 'E_hist', 'vol_hist', 'fmax_hist' (evaluations made, B), 'state', and with record_every > 0
        the frames 'R' and 'lattice'.  Runs on the predictor's first device, always on the general prediction route.
        Not offered: hydrostatic-only and constant-volume modes, the exponential cell parametrisation, L-BFGS (dynamics at a pressure:
        run_npt()).
        ValueError before anything is launched; FloatingPointError naming geometry and evaluation when a value is not finite
        (a cell that collapses to zero volume included)."""
        n3 = 3 * self.n_atoms
        R0 = _as_batch(R0, n3)
        B = R0.shape[0]
        if cell_factor is None:
            cell_factor = float(self.n_atoms)
        dt_max = _fire_checks(fmax, dt_start, dt_max, max_step, f_inc, f_dec, alpha_start, f_alpha, f_unit, n_min, max_steps,
                              record_every, more=(('pressure', pressure), ('cell_factor', cell_factor)),
                              positive=('cell_factor', cell_factor))
        if mask is not None:
            mask = np.asarray(mask, dtype=np.float64)
            if mask.shape != (3, 3) or not np.isin(mask, (0.0, 1.0)).all() or not np.array_equal(mask, mask.T):
                raise ValueError('mask must be a symmetric 3 x 3 array of 0 and 1')
        fire = _fire_state(state, B, (B, n3 + 9), dt_start, alpha_start,
                           tuple((k, shp, "state['" + k + "'] must have shape {}, got {}")
                                 for k, shp in (('S', (B, n3)), ('C', (B, 3, 3)), ('L0', (B, 3, 3)), ('V', (B, n3 + 9)))),
                           more_keys=('S', 'C', 'L0'))
        if state is None:
            if lattices is not None:
                L0 = self._lats_and_invs(lattices, B, lattice)[0]
            else:
                lat_and_inv = self._lat_and_inv(lattice)
                if lat_and_inv is None:
                    raise ValueError('relax_cell needs a lattice: the model has none and none was given')
                L0 = np.broadcast_to(lat_and_inv[0], (B, 3, 3))
            S, Cc = R0, np.broadcast_to(float(cell_factor) * np.eye(3), (B, 3, 3))
        else:
            S, Cc, L0 = state['S'], state['C'], state['L0']
        # a NaN start is not a usage error: the run reports the geometry and the evaluation (FloatingPointError)
        out = self._ctx.cell_relax_run(S, Cc, L0, fmax, max_steps, fire, dt_max, pressure=pressure, cell_factor=cell_factor,
                                       mask=mask, max_step=max_step, n_min=n_min, f_inc=f_inc, f_dec=f_dec,
                                       alpha_start=alpha_start, f_alpha=f_alpha, f_scale=self.std * float(f_unit),
                                       record_every=record_every)
        out = self._frozen_result(out, 'geometry', ('E_end', 'E_hist'))
        out['state'].update(S=out.pop('S'), C=out.pop('C'), L0=np.array(L0, dtype=np.float64))
        out['lattice_end'] = out.pop('lat_end')
        W = out.pop('W_end')
        W *= self.std
        W /= out['vol_end'].reshape(-1, 1, 1)
        out['stress_end'] = W
        if 'lat' in out:
            out['lattice'] = out.pop('lat')
        return out

    # ---- harmonic vibrational analysis on the device (gdml_vib_run, csrc/vib.hip)

    _VIB_PROJECT = {'none': 0, 'trans': 1, 'rigid': 2}

    def vibrations(self, R, masses, project=None, modes=False, lattice=None, f_unit=1.0):
        """Squared harmonic frequencies (and normal modes) of B geometries on the device: eigenvalues of the mass-weighted
        Hessian f_unit * H_ij / sqrt(m_i m_j), H the Hessian of predict_hessian(), with the rigid-body motion projected out.
        R: (B,3N) or (3N,); masses (N,); f_unit as in run_md (accelerations = f_unit * F / m), so w2 comes in the caller's time
        unit^-2.  project: 'rigid' (translations and rotations; the default without a lattice), 'trans' (translations; the
        default with one -- 'rigid' with a lattice is a ValueError), 'none'.  lattice: as in predict().
        Returns a dict: 'w2' (B,3N) -- the vibrational entries ascending (imaginary modes negative, first), then n_rigid exact
        zeros; 'freq' = sign(w2) sqrt|w2|; 'n_rigid' (B; 6, 5 for a linear molecule, 3 for an atom or 'trans'); 'n_imag' (B;
        vibrational w2 below -3N eps |D|_F); 'E' (B) and 'F' (B,3N) scaled like predict(); 'sweeps' (B; Jacobi sweeps); with
        modes=True 'modes' (B,3N,3N): row k the mass-weighted orthonormal vector of w2[k] (the last n_rigid rows span the
        rigid motions).  Batches are split over the predictor's devices like predict_hessian's.  ValueError for non-finite or
        misshapen input before anything is launched."""
        n3 = 3 * self.n_atoms
        if R is None:
            raise ValueError('vibrations needs geometries R (there is no training-set mode)')
        R = _as_batch(R, n3)
        masses = np.asarray(masses, dtype=np.float64)
        if masses.shape != (self.n_atoms,):
            raise ValueError('masses must be ({},), got shape {}'.format(self.n_atoms, masses.shape))
        if not (np.isfinite(R).all() and np.isfinite(masses).all()):
            raise ValueError('R and masses must be finite')
        if not (masses > 0.0).all():
            raise ValueError('masses must be positive')
        _check_finite(('f_unit', f_unit))
        if not float(f_unit) > 0.0:
            raise ValueError('f_unit must be positive')
        lat_and_inv = self._lat_and_inv(lattice)
        if project is None:
            project = 'rigid' if lat_and_inv is None else 'trans'
        if project not in self._VIB_PROJECT:
            raise ValueError("project must be None, 'none', 'trans' or 'rigid', got {!r}".format(project))
        if project == 'rigid' and lat_and_inv is not None:
            raise ValueError("project='rigid' with a lattice: rotations are no symmetry of a periodic cell (use 'trans')")
        h_scale, pj = self.std * float(f_unit), self._VIB_PROJECT[project]
        parts = self._sharded(R.shape[0], lambda ctx, lo, hi: ctx.vib_run(R[lo:hi], masses, h_scale=h_scale, project=pj,
                                                                          modes=modes, lat_and_inv=lat_and_inv),
                              min_shard=self._min_shard_hessian)
        out = parts[0] if len(parts) == 1 else {k: np.concatenate([p_[k] for p_ in parts]) for k in parts[0]}
        out['E'] *= self.std
        out['E'] += self.c
        out['F'] *= self.std
        out['n_imag'] = out.pop('n_neg')
        out['freq'] = np.sign(out['w2']) * np.sqrt(np.abs(out['w2']))
        return out

    # ---- eigenvector following on the device (gdml_ef_run, csrc/ef.hip)

    def stationary_point(self, R0, fmax, order=1, follow=None, max_steps=100, trust_start=0.1, trust_max=0.3, trust_min=1e-4,
                         project=None, state=None, lattice=None, f_unit=1.0, record_every=0):
        """Move B independent geometries to a stationary point of the energy on the device by eigenvector following: a minimum
        (order=0) or a first-order saddle (order=1), e.g. the climbing image of neb() tightened to any fmax.  Every evaluation
        takes the analytic Hessian of predict_hessian(), projects the rigid-body motion out as vibrations() does with unit
        masses (project: 'rigid' without a lattice, 'trans' with one, 'none'), diagonalises it and steps in its eigenbasis by
        the per-mode rational-function rule -- downhill along every mode, uphill along the followed one for order=1 -- inside
        a trust radius (trust_start, halved or doubled between trust_min and trust_max by the ratio of actual to predicted
        energy change; no step is rejected).  Gradient g = -f_unit * F with F the forces of predict(); Cartesian coordinates.
        R0: (B,3N) or (3N,).  follow: None (the lowest mode is maximised) or a (B,3N) direction, e.g. neb()'s tangent at
        i_climb: the mode of largest overlap is followed, and tracked from step to step.  A geometry is converged when its
        largest atomic |g| is below fmax; each takes at most max_steps steps in this call and stops on its own.
        state: the 'state' of an earlier call, passed back with its R_end, continues that run bit for bit.  lattice: as in
        predict().  record_every > 0 also returns 'R'.
        Returns a dict: 'R_end' (B,3N), 'E_end' (B) and 'F_end' (B,3N) scaled like predict(), 'fmax_end' (B), 'n_steps' (B),
        'converged' (B, bool), 'w_end' (B,3N; the spectrum at R_end in vibrations()' layout), 'n_rigid', 'n_neg' (B; the caller
        checks n_neg == order, the search does not enforce it), 'mode_end' (B,3N; the followed eigenvector, zeros for
        order=0), 'E_hist', 'fmax_hist', 'w_follow_hist', 'k_follow_hist' (evaluations made, B) and 'state'.  Runs on the
        predictor's first device.  ValueError for non-finite or out-of-range arguments before anything is launched;
        FloatingPointError naming geometry and evaluation when a value stops being finite."""
        n3 = 3 * self.n_atoms
        R0 = _as_batch(R0, n3)
        B = R0.shape[0]
        if not np.isfinite(R0).all():
            raise ValueError('R0 must be finite')
        _check_finite(('fmax', fmax), ('trust_start', trust_start), ('trust_max', trust_max), ('trust_min', trust_min),
                      ('f_unit', f_unit))
        if not float(fmax) > 0.0:
            raise ValueError('fmax must be positive')
        if not float(f_unit) > 0.0:
            raise ValueError('f_unit must be positive')
        if order not in (0, 1):
            raise ValueError('order must be 0 (minimum) or 1 (first-order saddle), got {!r}'.format(order))
        if int(max_steps) != max_steps or int(record_every) != record_every or max_steps < 0 or record_every < 0:
            raise ValueError('max_steps and record_every must be non-negative integers')
        if not 0.0 < float(trust_min) <= float(trust_start) <= float(trust_max):
            raise ValueError('need 0 < trust_min <= trust_start <= trust_max')
        lat_and_inv = self._lat_and_inv(lattice)
        if project is None:
            project = 'rigid' if lat_and_inv is None else 'trans'
        if project not in self._VIB_PROJECT:
            raise ValueError("project must be None, 'none', 'trans' or 'rigid', got {!r}".format(project))
        if project == 'rigid' and lat_and_inv is not None:
            raise ValueError("project='rigid' with a lattice: rotations are no symmetry of a periodic cell (use 'trans')")
        if follow is not None:
            if order == 0:
                raise ValueError('follow names the mode to maximise: it needs order=1')
            follow = _as_batch(follow)
            if follow.shape != R0.shape:
                raise ValueError('follow must have the shape of R0 {}, got {}'.format(R0.shape, follow.shape))
            if not np.isfinite(follow).all() or not (np.abs(follow).max(axis=1) > 0.0).all():
                raise ValueError('follow must be finite and non-zero for every geometry')
        if state is None:
            state = dict(trust=np.full(B, float(trust_start)), E_prev=np.zeros(B), dE_pred=np.zeros(B),
                         flags=np.zeros(B, dtype=np.int64), t=follow)
        else:
            missing = [k for k in ('trust', 'E_prev', 'dE_pred', 'flags', 't') if k not in state]
            if missing:
                raise ValueError('state lacks {}'.format(missing))
            if follow is not None:
                raise ValueError('follow starts a run; a continuation carries its own vector in state')
            if state['t'] is not None and order == 0:
                raise ValueError('state carries a follow vector: it needs order=1')
            for k in ('trust', 'E_prev', 'dE_pred', 'flags'):
                if np.shape(state[k]) != (B,):
                    raise ValueError("state['{}'] must have one entry per geometry ({})".format(k, B))
            if state['t'] is not None and np.shape(state['t']) != R0.shape:
                raise ValueError("state['t'] must have the shape of R0 {}, got {}".format(R0.shape, np.shape(state['t'])))
            tr = np.asarray(state['trust'], dtype=np.float64)
            if not all(np.isfinite(np.asarray(state[k], dtype=np.float64)).all() for k in ('trust', 'E_prev', 'dE_pred')):
                raise ValueError('state must be finite')
            if not ((tr >= float(trust_min)) & (tr <= float(trust_max))).all():
                raise ValueError("state['trust'] must lie in [trust_min, trust_max]")
        out = self._ctx.ef_run(R0, fmax, max_steps, state, order=order, trust_min=trust_min, trust_max=trust_max,
                               project=self._VIB_PROJECT[project], f_scale=self.std * float(f_unit),
                               record_every=record_every, lat_and_inv=lat_and_inv)
        return self._frozen_result(out, 'geometry', ('E_end', 'E_hist'))

    @staticmethod
    def harmonic_thermo(w2_vib, kT, hbar):
        """Quantum harmonic oscillators of squared frequencies w2_vib (the vibrational entries of vibrations()['w2'], any
        shape; summed over the last axis) at temperature kT: 'zpe' = sum hbar w / 2, 'F_vib' = zpe + kT sum ln(1 - exp(-hbar w
        / kT)), 'U_vib' = zpe + sum hbar w / (exp(hbar w / kT) - 1) and 'S_vib' = (U_vib - F_vib) / kT in units of k_B.  kT = 0
        gives the zero-point values.  ValueError for a negative or non-finite entry, kT < 0 or hbar <= 0.  Host only."""
        w2 = np.asarray(w2_vib, dtype=np.float64)
        if not np.isfinite(w2).all() or (w2 < 0.0).any():
            raise ValueError('harmonic_thermo needs finite squared frequencies >= 0 (leave imaginary and rigid modes out)')
        if not (np.isfinite(kT) and kT >= 0.0 and np.isfinite(hbar) and hbar > 0.0):
            raise ValueError('harmonic_thermo needs kT >= 0 and hbar > 0')
        e = float(hbar) * np.sqrt(w2)  # level spacings
        zpe = 0.5 * e.sum(axis=-1)
        if kT == 0.0:
            z = np.zeros_like(zpe)
            return dict(zpe=zpe, F_vib=zpe.copy(), U_vib=zpe.copy(), S_vib=z)
        x = e / float(kT)
        with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
            F = zpe + kT * np.log(-np.expm1(-x)).sum(axis=-1)
            U = zpe + np.where(x > 0.0, e / np.expm1(x), kT).sum(axis=-1)
        return dict(zpe=zpe, F_vib=F, U_vib=U, S_vib=(U - F) / kT)

    @staticmethod
    def htst_prefactor(w2_min, w2_saddle):
        """Prefactor of harmonic transition-state theory, (1 / 2 pi) prod w_min / prod' w_saddle, from the vibrational squared
        frequencies of the minimum (n entries, all positive) and of the saddle (n entries, exactly one negative: left out of
        the product), computed in logarithms.  With neb()'s 'barrier': rate = prefactor * exp(-barrier / kT).  Host only."""
        a, b = np.asarray(w2_min, dtype=np.float64).ravel(), np.asarray(w2_saddle, dtype=np.float64).ravel()
        if a.size != b.size:
            raise ValueError('htst_prefactor needs as many modes at the minimum as at the saddle, got {} and {}'.format(a.size, b.size))
        if not (np.isfinite(a).all() and np.isfinite(b).all()):
            raise ValueError('htst_prefactor needs finite squared frequencies')
        if not (a > 0.0).all():
            raise ValueError('htst_prefactor: every mode of the minimum must have w2 > 0')
        if int((b < 0.0).sum()) != 1 or (b == 0.0).any():
            raise ValueError('htst_prefactor: the saddle must have exactly one negative w2 and no zero one, got {} negative'.format(
                int((b < 0.0).sum())))
        return float(np.exp(0.5 * (np.log(a).sum() - np.log(b[b > 0.0]).sum())) / (2.0 * np.pi))

    # ---- nudged elastic band on the device (gdml_neb_run, csrc/neb.hip)

    @staticmethod
    def interpolate_path(R_a, R_b, n_images):
        """Linear interpolation between end points R_a and R_b ((B,3N), (3N,) or (B,N,3)): (B, n_images, 3N) with image 0 = R_a
        and image n_images - 1 = R_b, bit for bit.  Host only.  No minimum image: for a periodic model, unwrap R_b first."""
        if isinstance(n_images, bool) or int(n_images) != n_images or int(n_images) < 2:
            raise ValueError('n_images must be an integer of at least 2, got {!r}'.format(n_images))
        A, Bm = _as_batch(R_a), _as_batch(R_b)
        if A.ndim != 2 or A.shape != Bm.shape:
            raise ValueError('R_a and R_b must have the same shape (B, 3N), got {} and {}'.format(A.shape, Bm.shape))
        t = (np.arange(int(n_images)) / (int(n_images) - 1.0))[None, :, None]
        path = A[:, None, :] + t * (Bm - A)[:, None, :]
        path[:, 0], path[:, -1] = A, Bm
        return path

    def neb(self, R_path, fmax, k_spring=0.1, climb=False, max_steps=1000, dt_start=0.1, dt_max=None, max_step=0.2, n_min=5,
            f_inc=1.1, f_dec=0.5, alpha_start=0.1, f_alpha=0.99, state=None, lattice=None, f_unit=1.0, record_every=0):
        """Relax B independent bands of P images each to the minimum-energy path between their fixed end points (images 0 and
        P - 1) on the device: nudged elastic band with the improved tangent (Henkelman, Jonsson, JCP 113, 9978 (2000)), springs
        of constant k_spring (in units of f_unit * F per length) and, with climb=True, a climbing image (Henkelman, Uberuaga,
        Jonsson, JCP 113, 9901 (2000): the image of highest energy, chosen anew at every evaluation), driven by FIRE with the
        whole band as one system -- ASE's FIRE(NEB(...)); the FIRE parameters are relax()'s.  R_path: (B,P,3N) or (P,3N), 3 <= P
        <= 128 (interpolate_path() makes one).  A band is converged when the largest atomic |NEB force| of its interior images is
        below fmax; every band takes at most max_steps steps in this call and stops on its own.  state: the 'state' of an
        earlier call, passed back with its R_end, continues that run bit for bit (relaxing first without and then with climb is
        such a continuation); None is a fresh start.  lattice: as in predict(); positions are never wrapped.
        Returns a dict: 'R_end' (B,P,3N), 'E_end' (B,P) and 'F_end' (B,P,3N): the true energies and forces of R_end scaled like
        predict(), 'fmax_end', 'n_steps', 'converged' (B), 'i_climb' (B; the interior image of highest energy), 'barrier' (B,2;
        E(i_climb) - E of image 0 and of image P - 1), 's' (B,P; cumulative Euclidean arc length), 'f_tangent' (B,P; f_unit * F
        along the unit tangent at the interior images, 0 at the ends), 'fmax_hist' and 'Emax_hist' (evaluations made, B; the
        energy of the highest interior image), 'R' frames with record_every > 0, and 'state' ('V' (B,P,3N) with zero rows at the
        ends, 'dt', 'alpha', 'n_pos', 'n_taken' (B)).  ValueError for non-finite or out-of-range parameters and misshapen input
        before anything is launched; FloatingPointError naming band and evaluation when a value is not finite."""
        n3 = 3 * self.n_atoms
        R_path = np.asarray(R_path, dtype=np.float64)
        if R_path.ndim == 2:
            R_path = R_path[None]
        if R_path.ndim != 3 or R_path.shape[2] != n3:
            raise ValueError('R_path must be (B, P, {}) for this model, got shape {}'.format(n3, R_path.shape))
        B, P = R_path.shape[:2]
        if not 3 <= P <= 128:
            raise ValueError('a band needs 3 to 128 images, got {}'.format(P))
        dt_max = _fire_checks(fmax, dt_start, dt_max, max_step, f_inc, f_dec, alpha_start, f_alpha, f_unit, n_min, max_steps,
                              record_every, after_fmax=(('k_spring', k_spring),), positive=('k_spring', k_spring))
        state = _fire_state(state, B, R_path.shape, dt_start, alpha_start,
                            (('V', R_path.shape, "state['V'] must have the shape of R_path {}, got {}"),))
        # a NaN image is not a usage error: the run reports the band and the evaluation (FloatingPointError)
        out = self._ctx.neb_run(R_path, fmax, k_spring, max_steps, state, dt_max, climb=climb, max_step=max_step, n_min=n_min,
                                f_inc=f_inc, f_dec=f_dec, alpha_start=alpha_start, f_alpha=f_alpha,
                                f_scale=self.std * float(f_unit), record_every=record_every,
                                lat_and_inv=self._lat_and_inv(lattice))
        out = self._frozen_result(out, 'band', ('E_end', 'Emax_hist'))
        E_top = out['E_end'][np.arange(B), out['i_climb']] if B else np.empty(0)
        out['barrier'] = np.stack([E_top - out['E_end'][:, 0], E_top - out['E_end'][:, -1]], axis=1)
        return out

    # ---- path-integral molecular dynamics on the device (gdml_pimd_run, csrc/pimd.hip)

    def run_pimd(self, R0, V0, masses, dt, n_steps, beads, kT, hbar, record_every=1, thermostat=None, gamma_centroid=0.0,
                 pile_lambda=1.0, seed=0, step0=0, lattice=None, f_unit=1.0, record=('Rc', 'E')):
        """Advance B independent ring polymers of `beads` beads for n_steps on the device (nuclear quantum effects): ring-polymer
        MD with the exact free-ring flow (thermostat=None) or the same with the PILE-L thermostat in normal-mode space
        (thermostat='pile': friction pile_lambda * 2 omega_k on the internal modes, gamma_centroid on the centroid, 0 leaving
        it unthermostatted).  kT is the physical temperature in units of mass * velocity^2 (the beads are sampled at
        beads * kT), hbar Planck's constant over 2 pi in the caller's units.  R0, V0: (B,P,3N), or (B,3N) / (3N,) for a
        collapsed ring (every bead starts there); masses (N,); accelerations are f_unit * F / mass.  seed, step0, lattice,
        record_every: as in run_md().  record: which of 'R', 'V', 'F', 'E' (per bead) and 'Rc' (centroids) to return.
        Returns a dict: those of 'R', 'V', 'F' (n_rec,B,P,3N; F scaled by std), 'E' (n_rec,B,P; E std + c), 'Rc' (n_rec,B,3N);
        always 'E_pot' (n_rec,B; the bead average, E std + c), 'E_kin', 'E_spring', 'K_cv', 'K_prim' (n_rec,B; the
        centroid-virial and primitive kinetic-energy estimators, in the caller's kinetic units), the end state 'R_end', 'V_end'
        (B,P,3N) and 'step_end'.  Runs on the predictor's first device.  ValueError for non-finite or misshapen input before
        anything is launched; FloatingPointError naming ring and step when a trajectory stops being finite."""
        n3 = 3 * self.n_atoms
        if isinstance(beads, bool) or int(beads) != beads or not 1 <= int(beads) <= 128:
            raise ValueError('beads must be an integer from 1 to 128, got {!r}'.format(beads))
        P = int(beads)

        def ring(A, name):
            A = np.asarray(A, dtype=np.float64)
            if A.ndim == 1:
                A = A[None, :]
            if A.ndim == 2 and A.shape[1] == n3:  # a collapsed ring: every bead starts here
                A = np.repeat(A[:, None, :], P, axis=1)
            if A.ndim != 3 or A.shape[1:] != (P, n3):
                raise ValueError('{} must be (B, {}, {}), (B, {}) or ({},) for this model, got shape {}'.format(
                    name, P, n3, n3, n3, A.shape))
            return np.ascontiguousarray(A)

        R0, V0 = ring(R0, 'R0'), ring(V0, 'V0')
        if V0.shape != R0.shape:
            raise ValueError('V0 must have the shape of R0 {}, got {}'.format(R0.shape, V0.shape))
        masses = np.asarray(masses, dtype=np.float64)
        if masses.shape != (self.n_atoms,):
            raise ValueError('masses must be ({},), got shape {}'.format(self.n_atoms, masses.shape))
        if not (np.isfinite(R0).all() and np.isfinite(V0).all() and np.isfinite(masses).all()):
            raise ValueError('R0, V0 and masses must be finite')
        _check_finite(('dt', dt), ('gamma_centroid', gamma_centroid), ('pile_lambda', pile_lambda), ('kT', kT), ('hbar', hbar),
                      ('f_unit', f_unit))
        if thermostat not in (None, 'pile'):
            raise ValueError("thermostat must be None or 'pile', got {!r}".format(thermostat))
        record = _record_fields(record, ('R', 'V', 'F', 'E', 'Rc'))
        seed, step0 = int(seed), int(step0)
        if not 0 <= seed < 2**64:
            raise ValueError('seed must fit into 64 unsigned bits')
        lat_and_inv = self._lat_and_inv(lattice)
        out = self._ctx.pimd_run(R0, V0, masses, dt, n_steps, P, kT, hbar, record_every, f_scale=self.std * float(f_unit),
                                 thermostat=0 if thermostat is None else 1, gamma_centroid=gamma_centroid,
                                 pile_lambda=pile_lambda, seed=seed, step0=step0, lat_and_inv=lat_and_inv, record=record)
        _raise_first_bad(out.pop('first_bad_step'), 'ring', 'step')
        if 'F' in out:
            out['F'] *= self.std
        if 'E' in out:
            out['E'] *= self.std
            out['E'] += self.c
        q = out.pop('ring')
        out['E_pot'] = q[:, :, 0] * self.std + self.c
        for i, k in enumerate(('E_kin', 'E_spring', 'K_cv', 'K_prim')):
            out[k] = np.ascontiguousarray(q[:, :, i + 1])
        out['step_end'] = step0 + int(n_steps)
        return out

    # ---- posterior force covariance (csrc/uncert.hip)

    def prepare_uncertainty(self, R_train, F_train=None):
        """Build what predict_uncertainty() needs, once: the system matrix A = -K + lam I of the training set is assembled
        and factored on the first GPU (the fp64-MFMA Cholesky of the analytic solver) and the n x n factor, n = 3N M, STAYS
        RESIDENT there until release_uncertainty().  Models trained by the iterative solver are accepted as well: the factor
        is built from scratch, so whether n^2 * 8 bytes fit in HBM is the only limit (MemoryError otherwise;
        numpy.linalg.LinAlgError for a matrix that is not positive definite, as in the analytic solver).

        R_train (M,3N): the Cartesian training geometries in the model's order.  A model file holds only their descriptors,
        so they are checked against model['R_desc'] (rtol 1e-10) and a mismatch raises ValueError.

        Calibration: a Gaussian process fixes its covariance only up to the signal variance s^2.  Without F_train s^2 = 1 and
        ONLY THE RANKING of geometries by their variances is meaningful, not the magnitudes.  With F_train (M,3N), the labels
        the model was trained on, s^2 is the maximum-likelihood value y^T A^-1 y / n = -(y . alphas_F) / n, y =
        F_train.ravel() / std (needs model['alphas_F']); it is stored as `uncertainty_scale` and multiplies every covariance."""
        if self._use_E_cstr:
            raise NotImplementedError('posterior covariances of models with energy constraints are not supported')
        if self._lam is None:
            raise ValueError("the model carries no regularisation strength 'lam'")
        n3 = 3 * self.n_atoms
        R_train = np.asarray(R_train, dtype=np.float64)
        if R_train.size != self.n_train * n3:
            raise ValueError('R_train holds {} values, the model was trained on {} geometries of {} atoms'.format(
                R_train.size, self.n_train, self.n_atoms))
        R_train = R_train.reshape(self.n_train, n3)
        xd, gd = self._ctx.desc_from_R(R_train, self.n_atoms, self.lat_and_inv)
        if not np.allclose(xd, self._R_desc_train, rtol=1e-10, atol=0.0):
            raise ValueError("R_train does not reproduce the model's training descriptors (wrong geometries or order)")
        scale = 1.0
        y = None
        if F_train is not None:
            if self._alphas_F is None:
                raise ValueError("calibration needs the model's 'alphas_F'")
            y = np.asarray(F_train, dtype=np.float64).ravel() / self.std
            if y.size != self._alphas_F.size:
                raise ValueError('F_train holds {} values, the model has {} coefficients'.format(y.size, self._alphas_F.size))
            scale = float(-np.dot(y, self._alphas_F) / y.size)
        self._ctx.train_upload(xd, gd, self._tril_perms)
        self._train_resident = False  # the training-set mode uploads its own descriptors again when it is used next
        self._ctx.uncert_prepare(self.sig, self._lam)
        self.uncertainty_scale = scale
        self._unc_R, self._unc_gd, self._unc_y = (R_train.copy(), gd, y) if y is not None else (None, None, None)
        self._unc_prepared = True

    def release_uncertainty(self):
        """Free the resident factor of prepare_uncertainty()."""
        self._ctx.uncert_release()
        self._unc_prepared = False

    def predict_uncertainty(self, R, full_cov=False, low_latency=False):
        """(E, F, var) for geometries R (B,3N) or (3N,): E, F as predict(R); var (B,3N) the marginal posterior variances of
        the force components, or with full_cov the (B,3N,3N) posterior covariances, in the units of F squared (std^2 times
        `uncertainty_scale`: see prepare_uncertainty on what the magnitudes mean without calibration).  Runs on the first GPU
        only; set_alphas() does not invalidate the factor (it depends on the training geometries, sig and lam alone).

        low_latency=True takes the few-row solve (gdml_predict_cov_few) made for one or a few geometries per call, as in an MD
        loop that watches its own variance: up to 256 rows 3N B per call, a larger batch silently goes the default route.  Its
        covariances agree with the default's to rounding, not bit for bit; E, F, the scaling and the shapes are the same."""
        R = np.asarray(R, dtype=np.float64)
        if R.ndim == 1:
            R = R[None, :]
        R = R.reshape(R.shape[0], -1)
        cov_fn = self._ctx.predict_cov_few if low_latency else self._ctx.predict_cov
        cov = cov_fn(R, self.lat_and_inv, full=full_cov)
        E, F = self.predict(R)
        cov *= self.std * self.std * self.uncertainty_scale
        return E, F, cov

    # ---- leave-one-out errors and model evidence (csrc/loo.hip)

    def loo_errors(self, F_train=None, cov=None):
        """Leave-one-out force errors of the training set from the factor of prepare_uncertainty(), in one pass instead of M
        retrainings: for every training point j the error F_j - F_hat_j of the model trained WITHOUT point j (same sig, lam
        and permutations), exact up to rounding (Rasmussen & Williams 5.4.2).

        The coefficients are model['alphas_F'].  With F_train (M,3N), the labels the model was trained on, they are solved
        through the resident factor instead -- exact for this factor, and the right choice for models the iterative solver
        trained to a tolerance.  cov: None, 'diag' or 'full' -- the predictive (co)variances of the left-out labels.

        Returns a dict: 'F_resid' (M,3N) the errors in the units of F; 'F_loo' = F_train - F_resid, the left-out predictions
        (only with F_train); 'f_mae', 'f_rmse' over all M 3N components (the definitions of test_errors()['force']); 'cov'
        (M,3N) or (M,3N,3N) in units of F squared (std^2 times `uncertainty_scale`) when requested; 'log_det_A'; and
        'log_marginal_likelihood' of the normalised labels at signal variance s^2 = `uncertainty_scale`:
            -1/2 y^T A^-1 y / s^2 - 1/2 (log det A + n log s^2) - n/2 log 2 pi,    y^T A^-1 y = -y . alphas
        (with F_train; without it y is not known and the key is left out).  Leave-one-out energies are not offered: the
        integration constant is refitted per fold."""
        if self._use_E_cstr:
            raise NotImplementedError('leave-one-out errors of models with energy constraints are not supported')
        if cov not in (None, 'diag', 'full'):
            raise ValueError("cov must be None, 'diag' or 'full'")
        n = 3 * self.n_atoms * self.n_train
        y = None
        if F_train is not None:
            F_train = np.asarray(F_train, dtype=np.float64).reshape(self.n_train, -1)
            if F_train.size != n:
                raise ValueError('F_train holds {} values, the model has {} coefficients'.format(F_train.size, n))
            y = F_train.ravel() / self.std
            alphas = self._ctx.chol_solve(y)
        else:
            if self._alphas_F is None:
                raise ValueError("leave-one-out errors need the model's 'alphas_F' or F_train")
            alphas = self._alphas_F
        resid, c, logdet = self._ctx.loo(alphas, cov)
        resid *= self.std
        out = {'F_resid': resid, 'f_mae': float(np.abs(resid).sum() / n), 'f_rmse': float(np.sqrt((resid * resid).sum() / n)),
               'log_det_A': logdet}
        if c is not None:
            c *= self.std * self.std * self.uncertainty_scale
            out['cov'] = c
        if y is not None:
            s2 = self.uncertainty_scale
            out['F_loo'] = F_train - resid
            out['log_marginal_likelihood'] = float(-0.5 * (-np.dot(y, alphas)) / s2 - 0.5 * (logdet + n * np.log(s2))
                                                   - 0.5 * n * np.log(2.0 * np.pi))
        return out

    # ---- gradient of the model evidence in sig and lam, and its ascent (csrc/evidence.hip)

    @staticmethod
    def _evidence_from_terms(y, alphas, terms, sig, lam):
        n = y.size
        yAy = float(-np.dot(y, alphas))
        s2 = yAy / n
        tr, ik, aka, aa, logdet = (float(t) for t in terms)
        d_sig = 0.5 * (ik - aka / s2)
        d_lam = 0.5 * (aa / s2 - tr)
        return {'log_marginal_likelihood': float(-0.5 * yAy / s2 - 0.5 * (logdet + n * np.log(s2)) - 0.5 * n * np.log(2.0 * np.pi)),
                'signal_variance': s2, 'd_sig': d_sig, 'd_lam': d_lam, 'd_log_sig': sig * d_sig, 'd_log_lam': lam * d_lam,
                'log_det_A': logdet, 'terms': np.array(terms, dtype=np.float64)}

    def evidence_gradient(self, F_train=None):
        """The model evidence (log marginal likelihood of the normalised training labels) and its gradient in the length scale
        sig and the regularisation lam, from the factor of prepare_uncertainty(): what type-II maximum likelihood needs to
        set both without a grid of retrainings and without held-back data.

        The labels are F_train (M,3N), or those given to prepare_uncertainty(R_train, F_train); ValueError without either.
        The coefficients are solved through the resident factor, as in loo_errors(F_train), and the signal variance is its
        maximum-likelihood value s^2 = y^T A^-1 y / n, at which the partial derivatives below are the total derivatives of
        the profiled evidence.  Returns a dict:
            'log_marginal_likelihood'   -1/2 y^T A^-1 y / s^2 - 1/2 (log det A + n log s^2) - n/2 log 2 pi  (as loo_errors)
            'signal_variance'           s^2
            'd_sig', 'd_lam'            1/2 (<A^-1, K'> - a^T K' a / s^2),  1/2 (a^T a / s^2 - tr A^-1),  K' = dK/dsig
            'd_log_sig', 'd_log_lam'    sig d_sig, lam d_lam: the gradient in (log sig, log lam)
            'log_det_A', 'terms'        the raw sums (tr A^-1, <A^-1, K'>, a^T K' a, a^T a, log det A) of gdml_evidence_grad
        MEMORY: the call keeps the rows of L^-T in a second matrix as large as the factor, so it needs twice the factor's
        memory (MemoryError otherwise).  Models with energy constraints raise NotImplementedError."""
        if self._use_E_cstr:
            raise NotImplementedError('the evidence gradient of models with energy constraints is not supported')
        n = 3 * self.n_atoms * self.n_train
        if F_train is not None:
            y = np.asarray(F_train, dtype=np.float64).ravel() / self.std
            if y.size != n:
                raise ValueError('F_train holds {} values, the model has {} coefficients'.format(y.size, n))
        elif self._unc_y is not None:
            y = self._unc_y
        else:
            raise ValueError('evidence_gradient needs F_train, here or in prepare_uncertainty(R_train, F_train)')
        alphas = self._ctx.chol_solve(y)
        terms = self._ctx.evidence_grad(alphas)
        return self._evidence_from_terms(y, alphas, terms, self.sig, self._lam)

    def optimize_hyperparameters(self, R_train, F_train, E_train=None, params=('sig', 'lam'), max_iter=20, gtol=1e-3,
                                 bounds=None):
        """Set sig and / or lam by ascent of the profiled model evidence in (log sig, log lam) (type-II maximum likelihood): a
        BFGS step with backtracking on the evidence (`ascend`), every trial point one factorisation of the system matrix on the
        first GPU plus one evidence_gradient().  A trial point whose matrix is not positive definite counts as a failed step.

        R_train (M,3N), F_train (M,3N): the training geometries and labels in the model's order (checked as in
        prepare_uncertainty).  params: which of 'sig', 'lam' move.  gtol: the ascent ends when every component of the gradient
        in the logarithms is at most gtol.  bounds: {'sig': (lo, hi), 'lam': (lo, hi)}; default sig within a factor 100 of the
        model's, lam in [1e-14, 1e2].  E_train (M,): the integration constant c is recomputed by the trainer's rule.

        Afterwards the model's sig, lam and alphas_F are those of the best point (the coefficients solved through that point's
        factor, which stays resident as after prepare_uncertainty(R_train, F_train)), every replica predicts with them and
        export_model() returns them; the stored validation errors are reset to NaN.  On any exception the predictor -- and
        the resident factor, if there was one -- is left as it was.
        Returns the trace: one dict {'sig', 'lam', 'log_marginal_likelihood', 'd_log_sig', 'd_log_lam'} per accepted point,
        the start first."""
        if self._use_E_cstr:
            raise NotImplementedError('optimising the hyper-parameters of models with energy constraints is not supported')
        if self._lam is None:
            raise ValueError("the model carries no regularisation strength 'lam'")
        params = tuple(params)
        if not params or any(k not in ('sig', 'lam') for k in params) or len(set(params)) != len(params):
            raise ValueError("params must name 'sig', 'lam' or both")
        n3 = 3 * self.n_atoms
        R_train = np.asarray(R_train, dtype=np.float64)
        if R_train.size != self.n_train * n3:
            raise ValueError('R_train holds {} values, the model was trained on {} geometries of {} atoms'.format(
                R_train.size, self.n_train, self.n_atoms))
        R_train = R_train.reshape(self.n_train, n3)
        y = np.asarray(F_train, dtype=np.float64).ravel() / self.std
        if y.size != self.n_train * n3:
            raise ValueError('F_train holds {} values, the model has {} coefficients'.format(y.size, self.n_train * n3))
        if E_train is not None:
            E_train = np.asarray(E_train, dtype=np.float64).ravel()
            if E_train.size != self.n_train:
                raise ValueError('E_train holds {} energies, the model has {} training points'.format(E_train.size, self.n_train))
        dflt = {'sig': (self.sig / 100.0, self.sig * 100.0), 'lam': (1e-14, 1e2)}
        bounds = dict(dflt, **(bounds or {}))
        fixed = {'sig': self.sig, 'lam': self._lam}
        # the variables are the logarithms RELATIVE to the model's values: the start is 0, i.e. exactly the model's point
        lo = np.log([float(bounds[k][0]) / fixed[k] for k in params])
        hi = np.log([float(bounds[k][1]) / fixed[k] for k in params])
        ctx = self._ctx
        xd, gd = ctx.desc_from_R(R_train, self.n_atoms, self.lat_and_inv)
        if not np.allclose(xd, self._R_desc_train, rtol=1e-10, atol=0.0):
            raise ValueError("R_train does not reproduce the model's training descriptors (wrong geometries or order)")
        keys = ('sig', '_lam', '_alphas_F', '_R_d_desc_alpha', 'c', 'uncertainty_scale', '_unc_R', '_unc_gd', '_unc_y', '_edited',
                '_hyper_edited', '_unc_prepared', '_train_resident', '_replicas_stale')
        saved = {k: getattr(self, k) for k in keys}
        last = {}

        def point(xv):
            hp = dict(fixed)
            hp.update({k: fixed[k] * float(np.exp(v)) for k, v in zip(params, xv)})
            return hp

        def fun(xv):
            hp = point(xv)
            ctx.uncert_prepare(hp['sig'], hp['lam'])  # numpy.linalg.LinAlgError: a failed step
            alphas = ctx.chol_solve(y)
            ev = self._evidence_from_terms(y, alphas, ctx.evidence_grad(alphas), hp['sig'], hp['lam'])
            last.update(x=np.array(xv), alphas=alphas, ev=ev)
            return ev['log_marginal_likelihood'], np.array([ev['d_log_' + k] for k in params])

        try:
            ctx.train_upload(xd, gd, self._tril_perms)
            self._train_resident = False
            x_best, tr = ascend(fun, np.zeros(len(params)), max_iter=max_iter, gtol=gtol, bounds=(lo, hi))
            if not np.array_equal(last['x'], x_best):  # the last trial was rejected: the best point's factor once more
                fun(x_best)
            hp, alphas, ev = point(x_best), last['alphas'], last['ev']
            R_d_desc_alpha = self.desc.d_desc_dot_vec(gd, alphas.reshape(-1, n3))
            for c_ in [ctx] + self._replicas:
                c_.predict_upload_model(self._R_desc_train, R_d_desc_alpha, self._tril_perms, hp['sig'], None)
            self.sig, self._lam = hp['sig'], hp['lam']
            self._alphas_F, self._R_d_desc_alpha = alphas, R_d_desc_alpha
            self._replicas_stale = False
            self.uncertainty_scale = ev['signal_variance']
            self._unc_R, self._unc_gd, self._unc_y = R_train.copy(), gd, y
            self._unc_prepared = True
            self._edited = self._hyper_edited = True
            if E_train is not None:
                self.c = 0.0
                self.c = float(integration_constant(E_train, self.predict(R_train)[0]))
        except BaseException:
            for k, v in saved.items():
                setattr(self, k, v)
            try:
                for c_ in [ctx] + self._replicas:
                    c_.predict_upload_model(self._R_desc_train, self._R_d_desc_alpha, self._tril_perms, self.sig, None)
                if saved['_unc_prepared']:  # the same assembly and factorisation as before: the same bits
                    ctx.train_upload(xd, gd, self._tril_perms)
                    ctx.uncert_prepare(self.sig, self._lam)
                else:
                    ctx.uncert_release()
            except Exception:
                self.log.error('optimize_hyperparameters: the resident factor could not be restored')
            raise
        return [dict(point(xv), log_marginal_likelihood=f, **{'d_log_' + k: float(gk) for k, gk in zip(params, gv)})
                for xv, f, gv in tr]

    # ---- growing the training set through the resident factor (csrc/extend.hip)

    def add_training_points(self, R_new, F_new, E=None):
        """Add labelled geometries R_new (b,3N), F_new (b,3N) to the model WITHOUT retraining: the factor of
        prepare_uncertainty(R_train, F_train) -- which must have been called with F_train -- is bordered by the new points'
        rows on the first GPU (n^2 3N b flops instead of n'^3 / 3), the coefficients of the enlarged system are solved through it
        and every table the predictor holds is refreshed, on all replicas.  The labels are normalised with the model's
        EXISTING std: predictions do not depend on it (alphas = -A^-1 F / std, F_hat = std (... alphas)), so the result is the
        model a retraining on the enlarged set gives.  predict(), predict_uncertainty() and loo_errors() then work on M + b
        points; `uncertainty_scale` is recalibrated on the enlarged set.

        E: energies of ALL M + b training points in model order; the integration constant c is then recomputed by the
        trainer's rule (mean of E - E_pred at c = 0).  Without E, c is kept.

        Raises ValueError without the labelled prepare_uncertainty, NotImplementedError for models with energy constraints,
        numpy.linalg.LinAlgError when the enlarged matrix is not positive definite (a duplicate geometry at tiny lam) and
        MemoryError when old and new factor do not fit side by side; the model is unchanged after any of them.
        Returns {'n_train', 'c_updated', 'phase_ms': {'extend', 'solve'} device times, 'host_ms': {...} wall times of the
        steps, 'kernel_ms': per-phase kernel times when the context is profiling}."""
        if self._use_E_cstr:
            raise NotImplementedError('adding training points to models with energy constraints is not supported')
        if self._unc_y is None:
            raise ValueError('add_training_points needs prepare_uncertainty(R_train, F_train) with the training labels first')
        n3 = 3 * self.n_atoms
        R_new = np.asarray(R_new, dtype=np.float64)
        if R_new.size % n3:
            raise ValueError('R_new holds {} values, not a multiple of 3N = {}'.format(R_new.size, n3))
        R_new = R_new.reshape(-1, n3)
        b = R_new.shape[0]
        F_new = np.asarray(F_new, dtype=np.float64)
        if F_new.size != b * n3:
            raise ValueError('F_new holds {} values for {} geometries of {} atoms'.format(F_new.size, b, self.n_atoms))
        if E is not None:
            E = np.asarray(E, dtype=np.float64).ravel()
            if E.size != self.n_train + b:
                raise ValueError('E holds {} energies, the enlarged training set has {} points'.format(E.size, self.n_train + b))
        ctx = self._ctx
        t = [timeit.default_timer()]
        xd, gd = ctx.desc_from_R(R_new, self.n_atoms, self.lat_and_inv)
        t.append(timeit.default_timer())
        ctx.factor_extend(xd, gd)  # raises with the context untouched
        t.append(timeit.default_timer())
        y = np.concatenate([self._unc_y, F_new.ravel() / self.std])
        alphas = ctx.chol_solve(y)
        t.append(timeit.default_timer())
        self._unc_y = y
        self._unc_R = np.concatenate([self._unc_R, R_new])
        self._unc_gd = np.concatenate([self._unc_gd, gd])
        self._R_desc_train = np.ascontiguousarray(np.concatenate([self._R_desc_train, xd]))
        self._alphas_F = alphas
        self._R_d_desc_alpha = self.desc.d_desc_dot_vec(self._unc_gd, alphas.reshape(-1, n3))
        self.n_train += b
        self.chunk_size = self.n_train
        if b:
            self._edited = True
            if self._idxs_train is not None:
                self._idxs_train = np.concatenate([self._idxs_train, -np.ones(b, dtype=np.int64)])
        for c_ in [ctx] + self._replicas:
            c_.predict_upload_model(self._R_desc_train, self._R_d_desc_alpha, self._tril_perms, self.sig, None)
        self._replicas_stale = False
        self._train_resident = False
        self.uncertainty_scale = float(-np.dot(y, alphas) / y.size)
        if E is not None:
            self.c = 0.0
            self.c = float(integration_constant(E, self.predict(self._unc_R)[0]))
        t.append(timeit.default_timer())
        out = {'n_train': self.n_train, 'c_updated': E is not None,
               'phase_ms': {'extend': ctx.phase_ms('extend')[0] if b else 0.0, 'solve': ctx.phase_ms('solve')[0]},
               'host_ms': dict(zip(('desc', 'extend', 'solve', 'model'), [1e3 * (t[i + 1] - t[i]) for i in range(4)]))}
        kern = {k: ctx.kernel_stat(k)[0] for k in ('extend_copy', 'extend_cross', 'extend_solve', 'extend_schur', 'extend_chol')}
        if any(kern.values()):
            out['kernel_ms'] = kern
        return out

    # ---- shrinking the training set through the resident factor (csrc/remove.hip)

    def remove_training_points(self, idx, E=None):
        """Remove the training points idx (distinct integer indices in the model's current order) from the model WITHOUT
        retraining: their rows and columns leave the factor of prepare_uncertainty(R_train, F_train) -- which must have been
        called with F_train -- by a positive rank-3N b update of the rows behind them on the first GPU (O(3N b n^2) flops
        instead of n'^3 / 3), the coefficients of the reduced system are solved through it at the model's existing std and
        every table the predictor holds is refreshed, on all replicas.  The kept points keep their order; the result is the
        model a retraining on the kept points gives.  predict(), predict_uncertainty(), loo_errors() and
        add_training_points() then work on M - b points; `uncertainty_scale` is recalibrated on them.

        E: energies of the M - b KEPT points in their new order; the integration constant c is then recomputed by the
        trainer's rule (mean of E - E_pred at c = 0).  Without E, c is kept.

        Raises ValueError without the labelled prepare_uncertainty or for indices that are not distinct integers in
        [0, n_train) or that leave no point, NotImplementedError for models with energy constraints,
        numpy.linalg.LinAlgError when the reduced factor loses positivity and MemoryError when old and new factor do not fit
        side by side; the model is unchanged after any of them.
        Returns {'n_train', 'c_updated', 'phase_ms': {'remove', 'solve'} device times, 'host_ms': {...} wall times of the
        steps, 'kernel_ms': per-phase kernel times when the context is profiling}."""
        if self._use_E_cstr:
            raise NotImplementedError('removing training points from models with energy constraints is not supported')
        if self._unc_y is None:
            raise ValueError('remove_training_points needs prepare_uncertainty(R_train, F_train) with the training labels first')
        n3 = 3 * self.n_atoms
        raw = np.asarray(idx)
        if raw.size and raw.dtype.kind not in 'iu':
            raise ValueError('idx must hold integer indices of training points')
        idx = raw.astype(np.int64).ravel()
        b = idx.size
        if b and (idx.min() < 0 or idx.max() >= self.n_train):
            raise ValueError('idx must lie in [0, {})'.format(self.n_train))
        if np.unique(idx).size != b:
            raise ValueError('idx holds an index twice')
        if b >= self.n_train:
            raise ValueError('removing {} of {} training points leaves none'.format(b, self.n_train))
        if E is not None:
            E = np.asarray(E, dtype=np.float64).ravel()
            if E.size != self.n_train - b:
                raise ValueError('E holds {} energies, the reduced training set has {} points'.format(E.size, self.n_train - b))
        keep = np.ones(self.n_train, dtype=bool)
        keep[idx] = False
        ctx = self._ctx
        t = [timeit.default_timer()]
        ctx.factor_remove(idx)  # raises with the context untouched
        t.append(timeit.default_timer())
        y = np.ascontiguousarray(self._unc_y.reshape(self.n_train, n3)[keep]).ravel()
        alphas = ctx.chol_solve(y)
        t.append(timeit.default_timer())
        self._unc_y = y
        self._unc_R = np.ascontiguousarray(self._unc_R[keep])
        self._unc_gd = np.ascontiguousarray(self._unc_gd[keep])
        self._R_desc_train = np.ascontiguousarray(self._R_desc_train[keep])
        self._alphas_F = alphas
        self._R_d_desc_alpha = self.desc.d_desc_dot_vec(self._unc_gd, alphas.reshape(-1, n3))
        self.n_train -= b
        self.chunk_size = self.n_train
        if b:
            self._edited = True
            if self._idxs_train is not None:
                self._idxs_train = self._idxs_train[keep]
        for c_ in [ctx] + self._replicas:
            c_.predict_upload_model(self._R_desc_train, self._R_d_desc_alpha, self._tril_perms, self.sig, None)
        self._replicas_stale = False
        self._train_resident = False
        self.uncertainty_scale = float(-np.dot(y, alphas) / y.size)
        if E is not None:
            self.c = 0.0
            self.c = float(integration_constant(E, self.predict(self._unc_R)[0]))
        t.append(timeit.default_timer())
        out = {'n_train': self.n_train, 'c_updated': E is not None,
               'phase_ms': {'remove': ctx.phase_ms('remove')[0] if b else 0.0, 'solve': ctx.phase_ms('solve')[0]},
               'host_ms': dict(zip(('remove', 'solve', 'model'), [1e3 * (t[i + 1] - t[i]) for i in range(3)]))}
        kern = {k: ctx.kernel_stat(k)[0] for k in ('remove_compact', 'remove_panel', 'remove_apply')}
        if any(kern.values()):
            out['kernel_ms'] = kern
        return out

    # ---- choosing what to label next (csrc/select.hip)

    def select_training_points(self, R_pool, n_select, min_gain=None, prescreen=None):
        """Choose which n_select of the unlabelled geometries R_pool (B,3N) to label next, by the greedy batch rule on the
        JOINT information gain.  Sorting predict_uncertainty() by variance scores every geometry alone, and a pool cut from a
        trajectory is full of near-copies: the top of that ranking is one geometry several times.  Here every pick conditions
        the posterior on the points already picked (a block-pivoted Cholesky of the pool's joint posterior covariance on the
        first GPU), so a copy of a picked geometry only averages the label noise afterwards (at most 3N log 2).  The gain of
        candidate q at step t is
            log det(Sig_q^(t) / lam + I)    (nats)
        with Sig_q^(t) its posterior force covariance given the training set and the t earlier picks: twice the mutual
        information between the model and a noisy label at q.  It needs no labels and does not depend on std or
        `uncertainty_scale`; ties go to the lowest pool index.  Works after prepare_uncertainty(), with or without F_train;
        the model and the factor are only read.

        min_gain: stop before a pick whose gain is below it (None: always pick n_select).
        prescreen=K: the initial gains of the whole pool are computed in a streaming pass (any pool size), the joint
        selection runs on the K best candidates only and the indices are mapped back.  Greedy gains never increase (the
        criterion is submodular), so the result equals the un-screened one whenever the largest initial gain among the dropped
        candidates is below the last pick's gain (and below min_gain when that ended the sweep): that check is returned as
        'prescreen_exact'.  The same runs automatically, with the largest K that fits, when the joint selection on the whole
        pool does not fit in device memory.

        Returns a dict: 'idx' (k,) pool indices in pick order, k <= n_select; 'gain' (k,) their gains when picked;
        'gain_initial' (B,) the gains of all candidates before the first pick; 'total_gain' = sum of 'gain' = log det of the
        enlarged system matrix minus that of the present one minus 3N k log lam; 'prescreen_exact' (None without
        prescreening); 'phase_ms': {'select'} device time; 'kernel_ms' per-kernel times when the context is profiling.

        Raises ValueError without a prepared factor (prepare_uncertainty never called, released, or overwritten by an assembly
        since) or for arguments that do not fit, NotImplementedError for models with
        energy constraints, MemoryError when not even a prescreened pool fits, numpy.linalg.LinAlgError when a candidate's
        covariance is not positive definite."""
        if self._use_E_cstr:
            raise NotImplementedError('selecting training points for models with energy constraints is not supported')
        n3 = 3 * self.n_atoms
        R_pool = np.asarray(R_pool, dtype=np.float64)
        if R_pool.size % n3:
            raise ValueError('R_pool holds {} values, not a multiple of 3N = {}'.format(R_pool.size, n3))
        R_pool = np.ascontiguousarray(R_pool.reshape(-1, n3))
        B = R_pool.shape[0]
        if int(n_select) != n_select or not 0 <= n_select <= B:
            raise ValueError('n_select must be an integer in [0, {}]'.format(B))
        n_select = int(n_select)
        if prescreen is not None and (int(prescreen) != prescreen or prescreen < max(n_select, 1)):
            raise ValueError('prescreen must be an integer of at least max(n_select, 1)')
        ctx = self._ctx
        if not hasattr(ctx, 'n_atoms'):  # no training set was ever uploaded: the library would answer GDML_ERR_STATE
            raise ValueError('select_training_points needs prepare_uncertainty(R_train) first')
        kern_names = ('select_cross', 'select_solve', 'select_gram', 'select_score', 'select_column', 'select_update')
        phase = [0.0]
        kern0 = {k: ctx.kernel_stat(k)[0] for k in kern_names}

        def run(R, b):
            try:
                out = ctx.select_points(R, self.lat_and_inv, b, min_gain)
            except _lib.GDMLHipError as e:  # GDML_ERR_STATE: released, or overwritten by an assembly since
                if str(e).startswith('[{}]'.format(_lib.ERR_STATE)):
                    raise ValueError('select_training_points needs the factor of prepare_uncertainty(): ' + str(e)) from e
                raise
            if len(R):
                phase[0] += ctx.phase_ms('select')[0]
            return out

        keep = None
        if prescreen is None:
            try:
                idx, gain, gain0 = run(R_pool, n_select)
            except MemoryError as e:
                fits = re.search(r'largest pool that fits: (\d+)', str(e))
                if fits is None or int(fits.group(1)) < max(n_select, 1):
                    raise
                prescreen = int(fits.group(1))
        if prescreen is not None:
            gain0 = run(R_pool, 0)[2]
            K = min(int(prescreen), B)
            keep = np.sort(np.argsort(-gain0, kind='stable')[:K])  # the K best; in pool order, so that ties resolve as un-screened
            sub_idx, gain, _ = run(R_pool[keep], n_select)
            idx = keep[sub_idx]
        exact = None
        if keep is not None:
            dropped = np.ones(B, dtype=bool)
            dropped[keep] = False
            top = gain0[dropped].max() if dropped.any() else -np.inf
            exact = bool(top < gain[-1]) if len(gain) else True
            if len(gain) < n_select and min_gain is not None:
                exact = exact and bool(top < min_gain)
        out = {'idx': idx, 'gain': gain, 'gain_initial': gain0, 'total_gain': float(np.sum(gain)), 'prescreen_exact': exact,
               'phase_ms': {'select': phase[0]}}
        kern = {k: ctx.kernel_stat(k)[0] - kern0[k] for k in kern_names}
        if any(kern.values()):
            out['kernel_ms'] = kern
        return out

    def export_model(self):
        """The current model as a dict in the reference's schema (what GDMLPredict and the model files take): the keys the
        constructor was given, with R_desc, R_d_desc_alpha, alphas_F, c and std as they are now (and sig and lam after
        optimize_hyperparameters).  After add_training_points
        idxs_train carries -1 for every added point (they come from no dataset index), after remove_training_points it has
        lost the removed entries, and the stored validation errors are reset to NaN, as the trainer sets them for a model that
        has not been validated."""
        m = dict(self._model)
        m['R_desc'] = np.ascontiguousarray(self._R_desc_train.T)
        m['R_d_desc_alpha'] = self._R_d_desc_alpha
        if self._alphas_F is not None:
            m['alphas_F'] = self._alphas_F
        m['c'] = self.c
        m['std'] = self.std
        if self._hyper_edited:
            m['sig'], m['lam'] = self.sig, self._lam
        if self._edited:
            if self._idxs_train is not None:
                m['idxs_train'] = self._idxs_train.copy()
            m['f_err'] = {'mae': np.nan, 'rmse': np.nan}
            if 'e_err' in m:
                m['e_err'] = {'mae': np.nan, 'rmse': np.nan}
        return m

    def predict(self, R=None, return_E=True, lattice=None, lattices=None):
        """Energies (B,) and forces (B,3N) for geometries R (B,3N); R=None -> training-set mode.
        lattice: a 3 x 3 matrix with the cell vectors in its columns, used for THIS call instead of the model's (one lattice
        per call; ValueError unless 3 x 3 and regular).  None: the model's lattice, or none.
        lattices: (B,3,3), ONE LATTICE PER GEOMETRY (cell vectors in the columns), for B independent cells or the volumes of an
        equation-of-state scan in one batch; mutually exclusive with lattice; each member is validated like lattice.  Such a
        call takes the general prediction route for any B (the single launch holds one lattice)."""
        if lattices is not None:
            E, F, _, _ = self._cells(R, lattices, lattice, return_E=return_E, virial=False)
        elif R is not None:
            R = np.asarray(R, dtype=np.float64)
            if R.ndim == 1:
                R = R[None, :]
            R = R.reshape(R.shape[0], -1)
            lat_and_inv = self._lat_and_inv(lattice)
            parts = self._sharded(R.shape[0], lambda ctx, lo, hi: ctx.predict(R[lo:hi], lat_and_inv, return_E=return_E))
            F = parts[0][1] if len(parts) == 1 else np.concatenate([p_[1] for p_ in parts])
            E = None if not return_E else (parts[0][0] if len(parts) == 1 else np.concatenate([p_[0] for p_ in parts]))
        else:
            if lattice is not None:
                raise ValueError('a per-call lattice needs geometries R (the training-set mode uses cached descriptors)')
            if self.R_desc is None or self.R_d_desc is None:
                self.log.critical(
                    'A reference to the training geometry descriptors and Jacobians needs to be set '
                    'for this function to work without arguments.'
                )
                raise AssertionError('training descriptors not set')
            self._ensure_train_resident()
            E, F = self._ctx.predict(None, None, return_E=return_E)

        F *= self.std  # predict.py:1286-1288
        ret = (F,)
        if return_E:
            E *= self.std
            E += self.c
            ret = (E,) + ret
        return ret

"""ctypes binding of libgdml_hip.so (include/gdml_hip.h).  No compute happens in Python."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('GDML_HIP_LIB', os.path.join(_HERE, 'libgdml_hip.so'))  # override: A/B builds

GDML_OK = 0
ERR_INVALID, ERR_HIP, ERR_OOM, ERR_STATE, ERR_NOT_PD, ERR_UNSUPPORTED, ERR_COMM = -1, -2, -3, -4, -5, -6, -7
COLS_ALL, COLS_POINTS, COLS_INDEX = 0, 1, 2

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int64)
_vp = C.c_void_p
PCG_CB = C.CFUNCTYPE(C.c_int, C.c_int64, C.c_double, _vp)
HOST_COLL_CB = C.CFUNCTYPE(C.c_int, _dp, C.c_int64, _vp)  # gdml_host_allreduce / gdml_host_allgather



class MDParams(C.Structure):
    """gdml_md_params (include/gdml_hip.h)."""
    _fields_ = [('B', C.c_int64), ('N', C.c_int), ('dt', C.c_double), ('mass', _vp), ('f_scale', C.c_double), ('lat', _vp),
                ('lat_inv', _vp), ('thermostat', C.c_int), ('gamma', C.c_double), ('kT', C.c_double), ('seed', C.c_uint64),
                ('step0', C.c_int64)]


class NPTParams(C.Structure):
    """gdml_npt_params (include/gdml_hip.h)."""
    _fields_ = [('B', C.c_int64), ('N', C.c_int), ('dt', C.c_double), ('mass', _vp), ('f_scale', C.c_double),
                ('thermostat', C.c_int), ('gamma', C.c_double), ('gamma_baro', C.c_double), ('kT', C.c_double),
                ('seed', C.c_uint64), ('step0', C.c_int64), ('pressure', C.c_double), ('piston_mass', C.c_double)]


class PIMDParams(C.Structure):
    """gdml_pimd_params (include/gdml_hip.h)."""
    _fields_ = [('B', C.c_int64), ('N', C.c_int), ('beads', C.c_int), ('dt', C.c_double), ('mass', _vp), ('f_scale', C.c_double),
                ('lat', _vp), ('lat_inv', _vp), ('thermostat', C.c_int), ('gamma_centroid', C.c_double),
                ('pile_lambda', C.c_double), ('kT', C.c_double), ('hbar', C.c_double), ('seed', C.c_uint64), ('step0', C.c_int64)]


class RelaxParams(C.Structure):
    """gdml_relax_params (include/gdml_hip.h)."""
    _fields_ = [('B', C.c_int64), ('N', C.c_int), ('f_scale', C.c_double), ('lat', _vp), ('lat_inv', _vp), ('fmax', C.c_double),
                ('dt_max', C.c_double), ('max_step', C.c_double), ('f_inc', C.c_double), ('f_dec', C.c_double),
                ('alpha_start', C.c_double), ('f_alpha', C.c_double), ('n_min', C.c_int64)]


class CellRelaxParams(C.Structure):
    """gdml_cell_relax_params (include/gdml_hip.h)."""
    _fields_ = [('B', C.c_int64), ('N', C.c_int), ('f_scale', C.c_double), ('fmax', C.c_double), ('dt_max', C.c_double),
                ('max_step', C.c_double), ('f_inc', C.c_double), ('f_dec', C.c_double), ('alpha_start', C.c_double),
                ('f_alpha', C.c_double), ('n_min', C.c_int64), ('pressure', C.c_double), ('cell_factor', C.c_double),
                ('mask', _vp)]


class NebParams(C.Structure):
    """gdml_neb_params (include/gdml_hip.h)."""
    _fields_ = [('B', C.c_int64), ('N', C.c_int), ('P', C.c_int), ('f_scale', C.c_double), ('lat', _vp), ('lat_inv', _vp),
                ('fmax', C.c_double), ('dt_max', C.c_double), ('max_step', C.c_double), ('f_inc', C.c_double),
                ('f_dec', C.c_double), ('alpha_start', C.c_double), ('f_alpha', C.c_double), ('n_min', C.c_int64),
                ('k_spring', C.c_double), ('climb', C.c_int)]


class VibParams(C.Structure):
    """gdml_vib_params (include/gdml_hip.h)."""
    _fields_ = [('B', C.c_int64), ('N', C.c_int), ('h_scale', C.c_double), ('lat', _vp), ('lat_inv', _vp), ('project', C.c_int)]


class EfParams(C.Structure):
    """gdml_ef_params (include/gdml_hip.h)."""
    _fields_ = [('B', C.c_int64), ('N', C.c_int), ('order', C.c_int), ('f_scale', C.c_double), ('lat', _vp), ('lat_inv', _vp),
                ('fmax', C.c_double), ('trust_min', C.c_double), ('trust_max', C.c_double), ('project', C.c_int)]


# name -> (restype, argtypes).  Must list every symbol declared in include/gdml_hip.h.
SIGNATURES = {
    'gdml_abi_version': (C.c_int, []),
    'gdml_device_count': (C.c_int, [C.POINTER(C.c_int)]),
    'gdml_device_pci_bus_id': (C.c_int, [C.c_int, C.c_char_p, C.c_int]),
    'gdml_ctx_create': (C.c_int, [C.c_int, C.POINTER(_vp)]),
    'gdml_ctx_destroy': (C.c_int, [_vp]),
    'gdml_last_error': (C.c_char_p, [_vp]),
    'gdml_sync': (C.c_int, [_vp]),
    'gdml_mem_info': (C.c_int, [_vp, _ip, _ip, _ip]),
    'gdml_mem_reserve': (C.c_int, [_vp, C.c_int64, _ip]),
    'gdml_phase_ms': (C.c_int, [_vp, C.c_char_p, _dp, _ip]),
    'gdml_profile': (C.c_int, [_vp, C.c_int]),
    'gdml_kernel_stat': (C.c_int, [_vp, C.c_char_p, _dp, _ip, _dp]),
    'gdml_desc_from_R': (C.c_int, [_vp, _vp, C.c_int64, C.c_int, _vp, _vp, _vp, _vp]),
    'gdml_sym_eig_absv': (C.c_int, [_vp, _vp, C.c_int64, C.c_int, _vp]),
    'gdml_perm_match': (C.c_int, [_vp, _vp, _vp, _vp, C.c_int64, C.c_int, _vp, _vp, _vp, C.c_int64, C.POINTER(C.c_int64)]),
    'gdml_train_upload': (C.c_int, [_vp, _vp, _vp, C.c_int64, C.c_int, _vp, C.c_int]),
    'gdml_assemble_K': (C.c_int, [_vp, C.c_double, C.c_int, C.c_int, C.c_int64, C.c_int64, _vp, C.c_int64,
                                  C.c_int64, _vp, C.c_int64]),
    'gdml_assemble_A': (C.c_int, [_vp, C.c_double, C.c_double, C.c_int, C.c_int64]),
    'gdml_K_shape': (C.c_int, [_vp, _ip, _ip, _ip]),
    'gdml_chol_set_rhs': (C.c_int, [_vp, _vp, C.c_int64]),
    'gdml_chol_factor': (C.c_int, [_vp, C.c_double, C.POINTER(C.c_int)]),
    'gdml_lu_solve': (C.c_int, [_vp, C.c_double, _vp, C.c_int64, _vp, C.POINTER(C.c_int)]),
    'gdml_chol_solve': (C.c_int, [_vp, _vp, C.c_int64, C.c_int, _vp]),
    'gdml_predict_upload_model': (C.c_int, [_vp, _vp, _vp, C.c_int64, C.c_int, _vp, C.c_int, C.c_double, _vp]),
    'gdml_set_alphas': (C.c_int, [_vp, _vp, _vp]),
    'gdml_predict': (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, _vp, _vp]),
    'gdml_predict_dev': (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, _vp, _vp]),
    'gdml_md_run': (C.c_int, [_vp, C.POINTER(MDParams), _vp, _vp, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp]),
    'gdml_md_noise': (C.c_int, [C.c_uint64, C.c_int64, C.c_int64, C.c_int, _vp, _vp]),
    'gdml_pimd_run': (C.c_int, [_vp, C.POINTER(PIMDParams), _vp, _vp, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'gdml_pimd_modes': (C.c_int, [C.c_int, C.c_double, C.c_double, _vp, _vp]),
    'gdml_relax_run': (C.c_int, [_vp, C.POINTER(RelaxParams), _vp, _vp, _vp, _vp, _vp, _vp, C.c_int64, C.c_int64, _vp, _vp, _vp,
                                 _vp, _vp, _vp, _vp]),
    'gdml_neb_run': (C.c_int, [_vp, C.POINTER(NebParams), _vp, _vp, _vp, _vp, _vp, _vp, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp,
                               _vp, _vp, _vp, _vp, _vp, _vp]),
    'gdml_predict_virial': (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, _vp, _vp, _vp]),
    'gdml_predict_virial_dev': (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, _vp, _vp, _vp]),
    'gdml_predict_virial_cells': (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, _vp, _vp, _vp]),
    'gdml_predict_virial_cells_dev': (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, _vp, _vp, _vp]),
    'gdml_cell_relax_run': (C.c_int, [_vp, C.POINTER(CellRelaxParams), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int64,
                                      C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'gdml_npt_run': (C.c_int, [_vp, C.POINTER(NPTParams), _vp, _vp, _vp, _vp, _vp, _vp, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp,
                               _vp, _vp, _vp, _vp, _vp, _vp]),
    'gdml_predict_hessian': (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, _vp, _vp, _vp]),
    'gdml_predict_hessian_dev': (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, _vp, _vp, _vp]),
    'gdml_sym_eig': (C.c_int, [_vp, _vp, C.c_int64, C.c_int, _vp, _vp, _vp]),
    'gdml_sym_eig_dev': (C.c_int, [_vp, _vp, C.c_int64, C.c_int, _vp, _vp, _vp]),
    'gdml_vib_run': (C.c_int, [_vp, C.POINTER(VibParams), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'gdml_ef_run': (C.c_int, [_vp, C.POINTER(EfParams), _vp, _vp, _vp, _vp, _vp, _vp, C.c_int64, C.c_int64, _vp, _vp, _vp, _vp,
                              _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'gdml_uncert_prepare': (C.c_int, [_vp, C.c_double, C.c_double, C.POINTER(C.c_int)]),
    'gdml_uncert_release': (C.c_int, [_vp]),
    'gdml_uncert_cross': (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, _vp, _vp]),
    'gdml_predict_cov': (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, C.c_int, _vp]),
    'gdml_predict_cov_dev': (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, C.c_int, _vp]),
    'gdml_predict_cov_few': (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, C.c_int, _vp]),
    'gdml_predict_cov_few_dev': (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, C.c_int, _vp]),
    'gdml_loo': (C.c_int, [_vp, _vp, C.c_int64, C.c_int, _vp, _vp, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    'gdml_evidence_grad': (C.c_int, [_vp, _vp, C.c_int64, _vp, C.POINTER(C.c_int)]),
    'gdml_factor_extend': (C.c_int, [_vp, _vp, _vp, C.c_int64, C.POINTER(C.c_int)]),
    'gdml_factor_remove': (C.c_int, [_vp, _vp, C.c_int64, C.POINTER(C.c_int)]),
    'gdml_select_points': (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, C.c_int64, C.c_double, _vp, _vp, _vp, _ip,
                                     C.POINTER(C.c_int)]),
    'gdml_kernel_matvec': (C.c_int, [_vp, C.c_double, C.c_int, _vp, C.c_int64, _vp]),
    'gdml_predict_errors': (C.c_int, [_vp, _vp, C.c_int64, _vp, _vp, C.c_double, C.c_double, _vp, _vp, _vp]),
    'gdml_nystroem_factor': (C.c_int, [_vp, C.c_double, _vp, C.c_int64, _vp, _vp, C.POINTER(C.c_int)]),
    'gdml_nystroem_lev_scores': (C.c_int, [_vp, _vp]),
    'gdml_precon_apply': (C.c_int, [_vp, C.c_double, _vp, C.c_int64, _vp]),
    'gdml_pcg': (C.c_int, [_vp, C.c_double, C.c_int, _vp, _vp, C.c_int64, C.c_double, C.c_int64, C.c_int,
                           PCG_CB, C.c_int64, _vp, _vp, _ip, _dp, C.POINTER(C.c_int)]),
    'gdml_pcg_x': (C.c_int, [_vp, _vp]),
    'gdml_dist_chol_solve': (C.c_int, [_vp, C.c_double, C.c_double, _vp, C.c_int64, _vp, C.POINTER(C.c_int)]),
    'gdml_comm_unique_id': (C.c_int, [_vp]),
    'gdml_comm_init': (C.c_int, [_vp, _vp, C.c_int, C.c_int]),
    'gdml_comm_info': (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    'gdml_comm_suspend': (C.c_int, [_vp, C.c_int]),
    'gdml_comm_init_host': (C.c_int, [_vp, C.c_int, C.c_int, HOST_COLL_CB, HOST_COLL_CB, _vp]),
    'gdml_comm_stats': (C.c_int, [_vp, _ip, _dp]),
    'gdml_set_option': (C.c_int, [_vp, C.c_char_p, C.c_double]),
    'gdml_get_option': (C.c_int, [_vp, C.c_char_p, _dp, C.POINTER(C.c_int)]),
    'gdml_dev_alloc': (C.c_int, [_vp, C.c_int64, C.POINTER(_vp)]),
    'gdml_dev_free': (C.c_int, [_vp, _vp]),
    'gdml_memcpy_h2d': (C.c_int, [_vp, _vp, _vp, C.c_int64]),
    'gdml_memcpy_d2h': (C.c_int, [_vp, _vp, _vp, C.c_int64]),
    'gdml_K_dev': (C.c_int, [_vp, C.POINTER(_vp), _ip]),
}

_lib = None


class GDMLHipError(RuntimeError):
    pass


def load():
    """Load libgdml_hip.so (built by __graft_entry__.build() / make -C sgdml_amd/csrc)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            'libgdml_hip.so not found at {} -- build it with `python -c "import __graft_entry__ as g; '
            'g.build()"` or `make -C sgdml_amd/csrc`. There is no CPU fallback.'.format(LIB_PATH)
        )
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # raises AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def device_count():
    """Number of visible HIP devices (0 without a GPU)."""
    n = C.c_int(0)
    load().gdml_device_count(C.byref(n))
    return n.value


def device_pci_bus_id(device):
    """PCI bus id of visible device `device` (its physical identity), or None if the runtime cannot tell."""
    buf = C.create_string_buffer(64)
    if load().gdml_device_pci_bus_id(int(device), buf, 64) != 0:
        return None
    return buf.value.decode() or None


def preflight(attempts=3, timeout=180):
    """First touch of the GPU in a CHILD process: create a context and run one tiny kernel.  On a freshly leased box the
    very first kernel launch of a process has aborted inside the HIP runtime twice in ~40 runs (no message, before any of
    our code ran on the device); an abort cannot be caught, so callers that must not die with it (the test session, the
    benchmark, smoke) let a child take that first touch, and retry it.  Returns the number of attempts used (0: no GPU
    visible, nothing to do); raises RuntimeError when every attempt failed."""
    import subprocess
    import sys

    if device_count() < 1:
        return 0
    code = ('import numpy as np; from sgdml_amd import _lib; c = _lib.Context(0); '
            'c.desc_from_R(np.arange(18.0).reshape(2, 9) ** 1.5, 3); c.close()')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    err = ''
    for k in range(1, attempts + 1):
        try:
            p = subprocess.run([sys.executable, '-c', code], cwd=root, capture_output=True, text=True, timeout=timeout)
            if p.returncode == 0:
                return k
            err = (p.stderr or '')[-400:]
        except subprocess.TimeoutExpired:
            err = 'timeout'
    raise RuntimeError('GPU preflight failed %d times: %s' % (attempts, err))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_vp)


def f64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def i64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int64)


def _lat_pair(lat_and_inv):
    """(lattice, inverse) as contiguous fp64 arrays for _ptr(), or (None, None)."""
    if lat_and_inv is None:
        return None, None
    return f64(lat_and_inv[0]), f64(lat_and_inv[1])


def _state_copies(R, V, shape):
    """Copies of R and V in `shape` (the trajectory entries overwrite them with the end state)."""
    R = np.array(R, dtype=np.float64).reshape(shape)
    V = np.array(V, dtype=np.float64).reshape(shape)
    if V.shape != R.shape:
        raise ValueError('R and V differ in shape: {} and {}'.format(R.shape, V.shape))
    return R, V


def _record_arrays(record, shapes):
    """One uninitialised array per field of `shapes` that `record` names, None for the others."""
    return {k: (np.empty(shp) if k in record else None) for k, shp in shapes.items()}


def _recorded(rec):
    return {k: v for k, v in rec.items() if v is not None}


def _replica_state(state, B, noun, f_keys=('dt', 'alpha'), i_keys=('n_pos', 'n_taken')):
    """Fresh (B,) arrays of the per-replica entries of `state`, float64 for f_keys and int64 for i_keys, in that order (the
    run-until-frozen entries overwrite them with the end state).  noun: what a replica is, for the message."""
    arrays = [np.array(state[k], dtype=np.float64).ravel() for k in f_keys]
    arrays += [np.array(state[k], dtype=np.int64).ravel() for k in i_keys]
    for k, a in zip(f_keys + i_keys, arrays):
        if a.shape != (B,):
            raise ValueError("state['{}'] must have one entry per {} ({}), got shape {}".format(k, noun, B, a.shape))
    return arrays


def _frozen_arrays(B, max_steps, record_every, n_hist, frame_shapes):
    """What every run-until-frozen entry fills: status (B,2) and first_bad_step (B) at -1, n_hist uninitialised histories
    (max_steps + 1, B) and, per shape of frame_shapes, the frames (max_steps // record_every + 1, B) + shape (None without
    record_every > 0)."""
    n_eval = max(max_steps, 0) + 1
    n_rec = max(max_steps, 0) // record_every + 1 if record_every > 0 else 0
    hists = [np.empty((n_eval, B)) for _ in range(n_hist)]
    frames = [np.empty((n_rec, B) + shp) if record_every > 0 else None for shp in frame_shapes]
    return np.full((B, 2), -1, dtype=np.int64), np.full(B, -1, dtype=np.int64), hists, frames


def _frozen_out(status, bad, record_every, hists, frames):
    """The shared part of such an entry's result: 'status', 'first_bad_step', 'n_made' (evaluations made), the histories
    (dict name -> array) cut to n_made rows and the recorded frames (dict name -> array or None) to those of n_made."""
    n_made = int(status[:, 1].max()) + 1 if len(status) and (status[:, 1] >= 0).all() else 0
    out = dict(status=status, first_bad_step=bad, n_made=n_made)
    out.update((k, h[:n_made]) for k, h in hists.items())
    out.update((k, f[:(n_made + record_every - 1) // record_every]) for k, f in frames.items() if f is not None)
    return out


def _digest(a):
    """Content fingerprint of a contiguous array (xxhash when present, else md5)."""
    try:
        import xxhash

        return xxhash.xxh64(memoryview(a).cast('B')).hexdigest()
    except ImportError:  # pragma: no cover
        import hashlib

        return hashlib.md5(memoryview(a).cast('B')).hexdigest()


def tril_perms_from_lin(tril_perms_lin, dim_d):
    """Undo the linearisation of sgdml/train.py:903-904: returns the (P,D) int64 table."""
    lin = np.asarray(tril_perms_lin, dtype=np.int64).ravel()
    n_perms = lin.size // dim_d
    return np.ascontiguousarray(lin.reshape(dim_d, n_perms).T - np.arange(n_perms)[:, None] * dim_d)


class Context(object):
    """One gdml_ctx (one GPU, own streams and device buffers)."""

    max_query_batch = 1 << 17  # queries per gdml_predict call (bounds the device work buffers)

    def __init__(self, device=None):
        self._h = None
        lib = load()
        if device is None:
            device = int(os.environ.get('LOCAL_RANK', '0'))
            n = C.c_int(0)
            lib.gdml_device_count(C.byref(n))
            if n.value > 0:
                device %= n.value
        h = _vp()
        rc = lib.gdml_ctx_create(int(device), C.byref(h))
        if rc != GDML_OK:
            msg = lib.gdml_last_error(None).decode()
            raise GDMLHipError('cannot create GPU context (device {}): {}'.format(device, msg))
        self._lib = lib
        self._h = h
        self.device = device

    def close(self):
        if self._h is not None:
            self._lib.gdml_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- error mapping (SURVEY.md section 8b "Error conventions")
    def _check(self, rc):
        if rc == GDML_OK:
            return
        msg = self._lib.gdml_last_error(self._h).decode()
        cause = getattr(self, '_coll_exc', None)
        if cause is not None:  # a host-collective callback failed: that exception is the real reason of this error code
            self._coll_exc = None
            raise GDMLHipError('[{}] {}'.format(rc, msg)) from cause
        if rc == ERR_INVALID:
            raise ValueError(msg)
        if rc == ERR_OOM:
            raise MemoryError(msg)
        if rc == ERR_NOT_PD:
            raise np.linalg.LinAlgError(msg)
        if rc == ERR_UNSUPPORTED:
            raise NotImplementedError(msg)
        raise GDMLHipError('[{}] {}'.format(rc, msg))

    def sync(self):
        self._check(self._lib.gdml_sync(self._h))

    # -- multi-GPU (one process per GPU, RCCL bound inside the library)
    @staticmethod
    def comm_unique_id():
        """128-byte RCCL unique id (call on one rank, ship to the others by any host channel)."""
        lib = load()
        buf = C.create_string_buffer(128)
        rc = lib.gdml_comm_unique_id(buf)
        if rc != GDML_OK:
            raise GDMLHipError('gdml_comm_unique_id failed: ' + lib.gdml_last_error(None).decode())
        return buf.raw

    def comm_init(self, unique_id, rank, world):
        """unique_id=None creates a 'virtual rank' (shard arithmetic, no collectives; tests only)."""
        self._check(self._lib.gdml_comm_init(self._h, unique_id, int(rank), int(world)))

    def comm_init_host(self, rank, world, allreduce, allgather):
        """Host-staged collectives (gdml_comm_init_host).  allreduce(buf) / allgather(buf, chunk) receive a
        float64 NumPy view of the pinned staging buffer and must complete the collective in place."""
        def _ar(p, count, _user):
            try:
                allreduce(np.ctypeslib.as_array(p, shape=(count,)))
                return 0
            except BaseException as e:  # never let an exception cross the C frame
                self._coll_exc = e
                return 1

        def _ag(p, chunk, _user):
            try:
                allgather(np.ctypeslib.as_array(p, shape=(chunk * world,)), int(chunk))
                return 0
            except BaseException as e:
                self._coll_exc = e
                return 1

        self._coll_cbs = (HOST_COLL_CB(_ar), HOST_COLL_CB(_ag))  # keep the thunks alive
        self._check(self._lib.gdml_comm_init_host(self._h, int(rank), int(world), self._coll_cbs[0],
                                                  self._coll_cbs[1], None))

    def comm_suspended(self):
        """Context manager: inside it this context behaves like a single GPU without a communicator
        (gdml_comm_suspend) -- for solves every rank performs redundantly."""
        import contextlib

        @contextlib.contextmanager
        def _cm():
            self._check(self._lib.gdml_comm_suspend(self._h, 1))
            try:
                yield self
            finally:
                self._check(self._lib.gdml_comm_suspend(self._h, 0))

        return _cm()

    def comm_stats(self):
        """(collectives issued, payload bytes handed to them by this rank)."""
        n, b = C.c_int64(), C.c_double()
        self._check(self._lib.gdml_comm_stats(self._h, C.byref(n), C.byref(b)))
        return n.value, b.value

    def set_option(self, key, value):
        """Tuning / ablation option of this context (keys: include/gdml_hip.h)."""
        self._check(self._lib.gdml_set_option(self._h, key.encode(), float(value)))

    def get_option(self, key):
        """Value of an option, or None when it was never set (built-in default applies)."""
        v, is_set = C.c_double(), C.c_int()
        self._check(self._lib.gdml_get_option(self._h, key.encode(), C.byref(v), C.byref(is_set)))
        return v.value if is_set.value else None

    def comm_info(self):
        r, w = C.c_int(), C.c_int()
        self._check(self._lib.gdml_comm_info(self._h, C.byref(r), C.byref(w)))
        return r.value, w.value

    def mem_info(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._lib.gdml_mem_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def mem_reserve(self, n_bytes=None):
        """Reserve the process-level device arena (gdml_mem_reserve): one block the large matrices of every context on
        this device are carved from, kept until the process ends.  n_bytes=None: 85 % of the memory that is free right
        now; 0 releases it.  Returns the bytes held."""
        if n_bytes is None:
            n_bytes = int(0.85 * self.mem_info()[1]) // 2**30 * 2**30
        got = C.c_int64()
        self._check(self._lib.gdml_mem_reserve(self._h, int(n_bytes), C.byref(got)))
        return got.value

    def phase_ms(self, name):
        ms, n = C.c_double(), C.c_int64()
        self._check(self._lib.gdml_phase_ms(self._h, name.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def profile(self, enable=True):
        self._check(self._lib.gdml_profile(self._h, int(bool(enable))))

    def kernel_stat(self, name):
        """(summed ms, launches, summed algorithmic work) of a hot kernel since profile(True)."""
        ms, n, w = C.c_double(), C.c_int64(), C.c_double()
        self._check(self._lib.gdml_kernel_stat(self._h, name.encode(), C.byref(ms), C.byref(n), C.byref(w)))
        return ms.value, n.value, w.value

    def desc_from_R(self, R, n_atoms, lat_and_inv=None):
        R = f64(R).reshape(-1, 3 * n_atoms)
        M = R.shape[0]
        D = n_atoms * (n_atoms - 1) // 2
        xd = np.empty((M, D))
        gd = np.empty((M, D, 3))
        lat, lat_inv = _lat_pair(lat_and_inv)
        self._check(self._lib.gdml_desc_from_R(self._h, _ptr(R), M, n_atoms, _ptr(lat), _ptr(lat_inv),
                                               _ptr(xd), _ptr(gd)))
        return xd, gd

    def sym_eig_absv(self, adj):
        """|eigenvectors| (M,N,N) of symmetric matrices, columns by decreasing eigenvalue (batched Jacobi on the device)."""
        adj = f64(adj)
        M, N = adj.shape[0], adj.shape[1]
        out = np.empty((M, N, N))
        self._check(self._lib.gdml_sym_eig_absv(self._h, _ptr(adj), M, N, _ptr(out)))
        return out

    def perm_match(self, absv, adj, species):
        """Pairwise atom matching of the symmetry search on the device (gdml_perm_match).  absv = None: the eigenvectors of the
        distance matrices are computed on the device too (batched Jacobi).  Returns (cost (M,M) with the entries i < j set,
        ij (n,2), perms (n,N)): the kept assignments."""
        adj = f64(adj)
        M, N = adj.shape[0], adj.shape[1]
        if adj.shape != (M, N, N):
            raise ValueError('adj must be (M,N,N)')
        if absv is not None:
            absv = f64(absv)
            if absv.shape != (M, N, N):
                raise ValueError('absv must be (M,N,N)')
        sp = np.ascontiguousarray(species, dtype=np.int32)
        cost = np.zeros((M, M))
        cap = max(1, min(M * (M - 1) // 2, 4 * M))  # a tree's worth of kept pairs and then some; repeated with full room if short
        while True:
            ij = np.empty((cap, 2), dtype=np.int32)
            pm = np.empty((cap, N), dtype=np.int32)
            n = C.c_int64(0)
            self._check(self._lib.gdml_perm_match(self._h, _ptr(absv), _ptr(adj), _ptr(sp), M, N, _ptr(cost), _ptr(ij),
                                                  _ptr(pm), cap, C.byref(n)))
            if n.value <= cap:
                return cost, ij[:n.value], pm[:n.value]
            cap = M * (M - 1) // 2

    def train_upload(self, R_desc, R_d_desc, tril_perms):
        R_desc, R_d_desc, tril_perms = f64(R_desc), f64(R_d_desc), i64(tril_perms)
        M, D = R_desc.shape
        n_atoms = int((1 + np.sqrt(8 * D + 1)) / 2)
        if R_d_desc.shape != (M, D, 3):
            raise ValueError('R_d_desc must be the compressed (M,D,3) Jacobian')
        # the training set (descriptors, Jacobians, permutations and the dense tables derived from them on
        # the device) is sigma-independent: a hyper-parameter sweep over the same points uploads it once
        fp = (R_desc.shape, tril_perms.shape, _digest(R_desc), _digest(R_d_desc), _digest(tril_perms))
        if getattr(self, '_train_fp', None) == fp:
            return
        self._train_fp = None
        self._check(self._lib.gdml_train_upload(self._h, _ptr(R_desc), _ptr(R_d_desc), M, n_atoms,
                                                _ptr(tril_perms), tril_perms.shape[0]))
        self._train_fp = fp
        self.n_train, self.n_atoms = M, n_atoms

    def assemble_K(self, sig, use_E_cstr=False, points=None, idx=None, alloc_extra_rows=0, to_host=False,
                   for_cholesky=None):
        """Returns the host copy (rows+extra, cols) if to_host else None (matrix stays on the GPU).
        for_cholesky=lam: all columns, device only, assembled as A = -K + lam I for chol_factor (gdml_assemble_A)."""
        self._last_use_E = bool(use_E_cstr)
        if for_cholesky is not None:
            if points is not None or idx is not None or to_host:
                raise ValueError('for_cholesky assembles the full device-resident system matrix')
            self._check(self._lib.gdml_assemble_A(self._h, float(sig), float(for_cholesky), int(bool(use_E_cstr)),
                                                  int(alloc_extra_rows)))
            return None
        kind, a, b, ip, n_idx = COLS_ALL, 0, 0, None, 0
        if points is not None:
            kind, (a, b) = COLS_POINTS, points
        elif idx is not None:
            idx = i64(idx)
            kind, ip, n_idx = COLS_INDEX, _ptr(idx), idx.size
        if not to_host:
            self._check(self._lib.gdml_assemble_K(self._h, float(sig), int(bool(use_E_cstr)), kind, a, b, ip,
                                                  n_idx, int(alloc_extra_rows), None, 0))
            return None
        # two-step: the shape is only known to the library -> query after a device-only assembly
        n_rows = self.n_train * 3 * self.n_atoms + (self.n_train if use_E_cstr else 0)
        if kind == COLS_ALL:
            n_cols = n_rows
        elif kind == COLS_POINTS:
            n_cols = (min(b, self.n_train) - min(a, self.n_train)) * 3 * self.n_atoms + \
                     (max(b, self.n_train) - max(a, self.n_train))
        else:
            n_cols = n_idx
        K = np.empty((n_rows + alloc_extra_rows, n_cols))
        self._check(self._lib.gdml_assemble_K(self._h, float(sig), int(bool(use_E_cstr)), kind, a, b, ip,
                                              n_idx, int(alloc_extra_rows), _ptr(K), n_cols))
        return K

    def resident_K_bytes(self):
        """Bytes of the kernel-matrix buffer the context keeps for reuse (0 if none)."""
        try:
            rows, cols, extra = self.K_shape()
        except GDMLHipError:
            return 0
        ld = (cols + 15) // 16 * 16
        return (rows + extra) * ld * 8

    def K_shape(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._lib.gdml_K_shape(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def K_to_host(self):
        """Copy of the resident matrix / factor (tests only)."""
        rows, cols, extra = self.K_shape()
        p, ld = _vp(), C.c_int64()
        self._check(self._lib.gdml_K_dev(self._h, C.byref(p), C.byref(ld)))
        buf = np.empty((rows + extra, ld.value))
        self._check(self._lib.gdml_memcpy_d2h(self._h, _ptr(buf), p, buf.nbytes))
        return buf[:, :cols]

    def chol_factor(self, lam):
        info = C.c_int(0)
        self._check(self._lib.gdml_chol_factor(self._h, float(lam), C.byref(info)))
        return info.value

    def lu_solve(self, lam, y):
        """alphas = -(A^-1 y), A = -K + lam I, by LU with partial pivoting (the full K of assemble_K must be
        resident and is consumed).  Raises numpy.linalg.LinAlgError for an exactly singular matrix."""
        y = f64(y).ravel()
        out = np.empty_like(y)
        info = C.c_int(0)
        self._check(self._lib.gdml_lu_solve(self._h, float(lam), _ptr(y), y.size, _ptr(out), C.byref(info)))
        return out

    def dist_chol_solve(self, sig, lam, y):
        """Distributed analytic solve over the ranks of this context's communicator (gdml_dist_chol_solve):
        alphas = -(A^-1 y), A = -K + lam I, on every rank."""
        y = f64(y).ravel()
        out = np.empty_like(y)
        info = C.c_int(0)
        self._check(self._lib.gdml_dist_chol_solve(self._h, float(sig), float(lam), _ptr(y), y.size, _ptr(out),
                                                   C.byref(info)))
        return out

    def chol_set_rhs(self, y):
        """Hands y over before chol_factor (K must have been assembled with alloc_extra_rows >= 1): the
        factorisation then performs the forward substitution and chol_solve(None) only the backward one."""
        y = f64(y).ravel()
        self._check(self._lib.gdml_chol_set_rhs(self._h, _ptr(y), y.size))

    def chol_solve(self, y=None, n_refine=0):
        if y is None:
            n = self.K_shape()[0]
            out = np.empty(n)
            self._check(self._lib.gdml_chol_solve(self._h, None, n, int(n_refine), _ptr(out)))
            return out
        y = f64(y).ravel()
        out = np.empty_like(y)
        self._check(self._lib.gdml_chol_solve(self._h, _ptr(y), y.size, int(n_refine), _ptr(out)))
        return out

    def predict_upload_model(self, R_desc, R_d_desc_alpha, tril_perms, sig, alphas_E=None):
        R_desc, R_d_desc_alpha, tril_perms = f64(R_desc), f64(R_d_desc_alpha), i64(tril_perms)
        alphas_E = f64(alphas_E)
        M, D = R_desc.shape
        n_atoms = int((1 + np.sqrt(8 * D + 1)) / 2)
        self._check(self._lib.gdml_predict_upload_model(self._h, _ptr(R_desc), _ptr(R_d_desc_alpha), M, n_atoms,
                                                        _ptr(tril_perms), tril_perms.shape[0], float(sig),
                                                        _ptr(alphas_E)))
        self.model_n_train, self.model_n_atoms = M, n_atoms

    def set_alphas(self, alphas_F, alphas_E=None):
        alphas_F, alphas_E = f64(alphas_F).ravel(), f64(alphas_E)
        self._check(self._lib.gdml_set_alphas(self._h, _ptr(alphas_F), _ptr(alphas_E)))

    def predict(self, R=None, lat_and_inv=None, return_E=True):
        n_atoms = self.model_n_atoms
        if R is None:
            B = self.n_train
        else:
            R = f64(R).reshape(-1, 3 * n_atoms)
            B = R.shape[0]
        E = np.empty(B) if return_E else None
        F = np.empty((B, 3 * n_atoms))
        lat, lat_inv = _lat_pair(lat_and_inv)
        if R is None or B <= self.max_query_batch:
            self._check(self._lib.gdml_predict(self._h, _ptr(R), B, _ptr(lat), _ptr(lat_inv), _ptr(E), _ptr(F)))
            return E, F
        # very large batches go through in slices so that the device work buffers stay bounded (the reference's
        # GPU path re-batches instead of failing as well, torchtools.py:349-387)
        for b0 in range(0, B, self.max_query_batch):
            b1 = min(B, b0 + self.max_query_batch)
            Ec = None if E is None else E[b0:b1]
            self._check(self._lib.gdml_predict(self._h, _ptr(R[b0:b1]), b1 - b0, _ptr(lat), _ptr(lat_inv), _ptr(Ec),
                                               _ptr(F[b0:b1])))
        return E, F

    def _masses(self, mass):
        mass = f64(mass).ravel()
        if mass.size != self.model_n_atoms:
            raise ValueError('{} masses for {} atoms'.format(mass.size, self.model_n_atoms))
        return mass

    def md_run(self, R, V, mass, dt, n_steps, record_every=1, f_scale=1.0, thermostat=0, gamma=0.0, kT=0.0, seed=0, step0=0,
               lat_and_inv=None, record=('R',)):
        """gdml_md_run: B replicas (R, V: (B,3N)) advance n_steps on the device.  Returns a dict with the end state 'R_end',
        'V_end', the frames 'E' (n_rec,B; unscaled E'), 'Ekin' (n_rec,B) and those of 'R', 'V', 'F' (n_rec,B,3N) named in
        `record`, and 'first_bad_step' (B; -1 = every value stayed finite)."""
        n3 = 3 * self.model_n_atoms
        R, V = _state_copies(R, V, (-1, n3))
        B = R.shape[0]
        mass = self._masses(mass)
        lat, lat_inv = _lat_pair(lat_and_inv)
        n_steps, record_every = int(n_steps), int(record_every)
        n_rec = n_steps // record_every if (n_steps > 0 and record_every > 0) else 0
        rec = _record_arrays(record, {k: (n_rec, B, n3) for k in ('R', 'V', 'F')})
        E, Ek = np.empty((n_rec, B)), np.empty((n_rec, B))
        bad = np.full(B, -1, dtype=np.int64)
        prm = MDParams(B, self.model_n_atoms, float(dt), _ptr(mass), float(f_scale), _ptr(lat), _ptr(lat_inv), int(thermostat),
                       float(gamma), float(kT), int(seed), int(step0))
        self._check(self._lib.gdml_md_run(self._h, C.byref(prm), _ptr(R), _ptr(V), n_steps, record_every, _ptr(rec['R']),
                                          _ptr(rec['V']), _ptr(rec['F']), _ptr(E), _ptr(Ek), _ptr(bad)))
        out = _recorded(rec)
        out.update(R_end=R, V_end=V, E=E, Ekin=Ek, first_bad_step=bad)
        return out

    def md_noise(self, seed, step, B, n3):
        """gdml_md_noise: the standard normals (B,n3) a Langevin step of absolute index `step` consumes."""
        xi = np.empty((int(B), int(n3)))
        self._check(self._lib.gdml_md_noise(int(seed), int(step), int(B), int(n3), _ptr(xi), self._h))
        return xi

    def pimd_run(self, R, V, mass, dt, n_steps, beads, kT, hbar, record_every=1, f_scale=1.0, thermostat=0, gamma_centroid=0.0,
                 pile_lambda=1.0, seed=0, step0=0, lat_and_inv=None, record=('Rc', 'E')):
        """gdml_pimd_run: B rings of `beads` beads (R, V: (B,P,3N)) advance n_steps on the device.  Returns a dict with the end
        state 'R_end', 'V_end', the frames 'ring' (n_rec,B,5: E_pot unscaled, E_kin, E_spring, K_cv, K_prim), those of 'R', 'V',
        'F' (n_rec,B,P,3N), 'E' (n_rec,B,P; unscaled E') and 'Rc' (n_rec,B,3N) named in `record`, and 'first_bad_step' (B)."""
        n3, P = 3 * self.model_n_atoms, int(beads)
        if P < 1:
            raise ValueError('beads must be at least 1, got {}'.format(beads))
        R, V = _state_copies(R, V, (-1, P, n3))
        B = R.shape[0]
        mass = self._masses(mass)
        lat, lat_inv = _lat_pair(lat_and_inv)
        n_steps, record_every = int(n_steps), int(record_every)
        n_rec = n_steps // record_every if (n_steps > 0 and record_every > 0) else 0
        rec = _record_arrays(record, {'R': (n_rec, B, P, n3), 'V': (n_rec, B, P, n3), 'F': (n_rec, B, P, n3), 'E': (n_rec, B, P),
                                      'Rc': (n_rec, B, n3)})
        ring = np.empty((n_rec, B, 5))
        bad = np.full(B, -1, dtype=np.int64)
        prm = PIMDParams(B, self.model_n_atoms, P, float(dt), _ptr(mass), float(f_scale), _ptr(lat), _ptr(lat_inv),
                         int(thermostat), float(gamma_centroid), float(pile_lambda), float(kT), float(hbar), int(seed), int(step0))
        self._check(self._lib.gdml_pimd_run(self._h, C.byref(prm), _ptr(R), _ptr(V), n_steps, record_every, _ptr(rec['R']),
                                            _ptr(rec['V']), _ptr(rec['F']), _ptr(rec['E']), _ptr(rec['Rc']), _ptr(ring),
                                            _ptr(bad)))
        out = _recorded(rec)
        out.update(R_end=R, V_end=V, ring=ring, first_bad_step=bad)
        return out

    @staticmethod
    def pimd_modes(beads, kT, hbar):
        """gdml_pimd_modes: the normal-mode matrix C (P,P; row = bead j, column = mode k) and the mode frequencies (P,) a ring
        of `beads` beads uses.  Host only: no context, no device."""
        lib, P = load(), int(beads)
        Cm, omega = np.empty((max(P, 0), max(P, 0))), np.empty(max(P, 0))
        if lib.gdml_pimd_modes(P, float(kT), float(hbar), _ptr(Cm), _ptr(omega)) != GDML_OK:
            raise ValueError(lib.gdml_last_error(None).decode())
        return Cm, omega

    def relax_run(self, R, fmax, max_steps, state, dt_max, max_step=0.2, n_min=5, f_inc=1.1, f_dec=0.5, alpha_start=0.1,
                  f_alpha=0.99, f_scale=1.0, record_every=0, lat_and_inv=None):
        """gdml_relax_run: B geometries (R: (B,3N)) descend by FIRE on the device for at most max_steps steps each.  state: dict
        with 'V' (B,3N), 'dt', 'alpha' (B), 'n_pos', 'n_taken' (B, int) -- the optimiser's state at the start.  Returns a dict:
        'R_end', 'E_end' (B; unscaled E'), 'F_end' (B,3N; unscaled), the end 'state', 'status' (B,2; see the header), 'n_made'
        (evaluations made), 'E_hist', 'fmax_hist' (n_made,B), the frames 'R' (every record_every-th evaluation; only with
        record_every > 0) and 'first_bad_step' (B; -1 = every value stayed finite)."""
        n3 = 3 * self.model_n_atoms
        R, V = _state_copies(R, state['V'], (-1, n3))
        B = R.shape[0]
        dt, alpha, n_pos, n_taken = _replica_state(state, B, 'geometry')
        lat, lat_inv = _lat_pair(lat_and_inv)
        max_steps, record_every = int(max_steps), int(record_every)
        status, bad, (E_hist, f_hist), (R_rec,) = _frozen_arrays(B, max_steps, record_every, 2, [(n3,)])
        E_end, F_end = np.empty(B), np.empty((B, n3))
        prm = RelaxParams(B, self.model_n_atoms, float(f_scale), _ptr(lat), _ptr(lat_inv), float(fmax), float(dt_max),
                          float(max_step), float(f_inc), float(f_dec), float(alpha_start), float(f_alpha), int(n_min))
        self._check(self._lib.gdml_relax_run(self._h, C.byref(prm), _ptr(R), _ptr(V), _ptr(dt), _ptr(alpha), _ptr(n_pos),
                                             _ptr(n_taken), max_steps, record_every, _ptr(R_rec), _ptr(E_hist), _ptr(f_hist),
                                             _ptr(E_end), _ptr(F_end), _ptr(status), _ptr(bad)))
        return dict(R_end=R, E_end=E_end, F_end=F_end, state=dict(V=V, dt=dt, alpha=alpha, n_pos=n_pos, n_taken=n_taken),
                    **_frozen_out(status, bad, record_every, dict(E_hist=E_hist, fmax_hist=f_hist), dict(R=R_rec)))

    def neb_run(self, R, fmax, k_spring, max_steps, state, dt_max, climb=False, max_step=0.2, n_min=5, f_inc=1.1, f_dec=0.5,
                alpha_start=0.1, f_alpha=0.99, f_scale=1.0, record_every=0, lat_and_inv=None):
        """gdml_neb_run: B bands of P images (R: (B,P,3N), images 0 and P - 1 fixed) relax by FIRE on the NEB force, a band being
        one FIRE system, for at most max_steps steps each.  state: dict with 'V' (B,P,3N; the end points' rows are not used and
        come back zero), 'dt', 'alpha' (B), 'n_pos', 'n_taken' (B, int).  Returns a dict: 'R_end', 'E_end' (B,P; unscaled E'),
        'F_end' (B,P,3N; unscaled), 'i_climb' (B), 's', 'f_tangent' (B,P), the end 'state', 'status' (B,2; see the header),
        'n_made', 'Emax_hist' (unscaled), 'fmax_hist' (n_made,B), the frames 'R' (only with record_every > 0) and
        'first_bad_step' (B)."""
        n3 = 3 * self.model_n_atoms
        R = np.asarray(R, dtype=np.float64)
        if R.ndim != 3 or R.shape[2] != n3:
            raise ValueError('R must be (B, P, {}), got shape {}'.format(n3, R.shape))
        B, P = R.shape[:2]
        R, V = _state_copies(R, state['V'], (B, P, n3))
        if P >= 1:
            V[:, 0] = 0.0
            V[:, -1] = 0.0
        dt, alpha, n_pos, n_taken = _replica_state(state, B, 'band')
        lat, lat_inv = _lat_pair(lat_and_inv)
        max_steps, record_every = int(max_steps), int(record_every)
        status, bad, (E_hist, f_hist), (R_rec,) = _frozen_arrays(B, max_steps, record_every, 2, [(P, n3)])
        E_end, F_end = np.zeros((B, P)), np.zeros((B, P, n3))
        s, f_tan = np.zeros((B, P)), np.zeros((B, P))
        i_climb = np.zeros(B, dtype=np.int64)
        prm = NebParams(B, self.model_n_atoms, P, float(f_scale), _ptr(lat), _ptr(lat_inv), float(fmax), float(dt_max),
                        float(max_step), float(f_inc), float(f_dec), float(alpha_start), float(f_alpha), int(n_min),
                        float(k_spring), int(bool(climb)))
        self._check(self._lib.gdml_neb_run(self._h, C.byref(prm), _ptr(R), _ptr(V), _ptr(dt), _ptr(alpha), _ptr(n_pos),
                                           _ptr(n_taken), max_steps, record_every, _ptr(R_rec), _ptr(E_hist), _ptr(f_hist),
                                           _ptr(E_end), _ptr(F_end), _ptr(i_climb), _ptr(s), _ptr(f_tan), _ptr(status),
                                           _ptr(bad)))
        return dict(R_end=R, E_end=E_end, F_end=F_end, i_climb=i_climb, s=s, f_tangent=f_tan,
                    state=dict(V=V, dt=dt, alpha=alpha, n_pos=n_pos, n_taken=n_taken),
                    **_frozen_out(status, bad, record_every, dict(Emax_hist=E_hist, fmax_hist=f_hist), dict(R=R_rec)))

    def predict_virial(self, R, lat_and_inv=None):
        """Unscaled E' (B,), F (B,3N) and strain derivative W = dE'/d eps (B,3,3) of geometries R (B,3N) (gdml_predict_virial);
        batches beyond max_query_batch go through in slices, as in predict()."""
        if R is None:
            raise ValueError('predict_virial needs geometries (there is no training-set mode)')
        n3 = 3 * self.model_n_atoms
        R = f64(R).reshape(-1, n3)
        B = R.shape[0]
        E, F, W = np.empty(B), np.empty((B, n3)), np.empty((B, 3, 3))
        lat, lat_inv = _lat_pair(lat_and_inv)
        for b0 in range(0, max(B, 1), self.max_query_batch):
            b1 = min(B, b0 + self.max_query_batch)
            self._check(self._lib.gdml_predict_virial(self._h, _ptr(R[b0:b1]), b1 - b0, _ptr(lat), _ptr(lat_inv),
                                                      _ptr(E[b0:b1]), _ptr(F[b0:b1]), _ptr(W[b0:b1])))
        return E, F, W

    def predict_virial_dev(self, R_dev, B, E_dev, F_dev, W_dev, lat_and_inv=None):
        """gdml_predict_virial_dev on device pointers (ints or c_void_p; E_dev / F_dev may be None)."""
        lat, lat_inv = _lat_pair(lat_and_inv)
        self._check(self._lib.gdml_predict_virial_dev(self._h, R_dev, int(B), _ptr(lat), _ptr(lat_inv), E_dev, F_dev,
                                                      W_dev))

    def predict_cells(self, R, lats, lat_invs, return_E=True, virial=True):
        """gdml_predict_virial_cells: unscaled E' (B,) or None, F (B,3N) and, with virial, W (B,3,3) (else None) of geometries R
        (B,3N), geometry b in lattice lats[b] with inverse lat_invs[b] (B,3,3; cell vectors in the columns).  Batches beyond
        max_query_batch go through in slices, as in predict()."""
        if R is None:
            raise ValueError('per-geometry lattices need geometries (there is no training-set mode)')
        n3 = 3 * self.model_n_atoms
        R = f64(R).reshape(-1, n3)
        B = R.shape[0]
        lats, lat_invs = f64(lats), f64(lat_invs)
        if lats.shape != (B, 3, 3) or lat_invs.shape != (B, 3, 3):
            raise ValueError('lattices and inverses must be ({}, 3, 3), got {} and {}'.format(B, lats.shape, lat_invs.shape))
        E = np.empty(B) if return_E else None
        F = np.empty((B, n3))
        W = np.empty((B, 3, 3)) if virial else None
        for b0 in range(0, max(B, 1), self.max_query_batch):
            b1 = min(B, b0 + self.max_query_batch)
            self._check(self._lib.gdml_predict_virial_cells(
                self._h, _ptr(R[b0:b1]), b1 - b0, _ptr(lats[b0:b1]), _ptr(lat_invs[b0:b1]),
                None if E is None else _ptr(E[b0:b1]), _ptr(F[b0:b1]), None if W is None else _ptr(W[b0:b1])))
        return E, F, W

    def predict_cells_dev(self, R_dev, B, lats_dev, lat_invs_dev, E_dev, F_dev, W_dev):
        """gdml_predict_virial_cells_dev on device pointers (ints or c_void_p; E_dev / F_dev / W_dev may be None)."""
        self._check(self._lib.gdml_predict_virial_cells_dev(self._h, R_dev, int(B), lats_dev, lat_invs_dev, E_dev, F_dev, W_dev))

    def cell_relax_run(self, S, Cc, L0, fmax, max_steps, state, dt_max, pressure=0.0, cell_factor=1.0, mask=None, max_step=0.2,
                       n_min=5, f_inc=1.1, f_dec=0.5, alpha_start=0.1, f_alpha=0.99, f_scale=1.0, record_every=0):
        """gdml_cell_relax_run: B periodic geometries relax atoms and cell by FIRE on the device.  S (B,3N): reference positions,
        Cc (B,3,3): cell_factor times the deformation gradient, L0 (B,3,3): reference lattices; state: dict with 'V' (B,3N+9),
        'dt', 'alpha' (B), 'n_pos', 'n_taken' (B, int).  Returns a dict: 'S', 'C' (the end coordinates), 'R_end' (B,3N;
        Cartesian), 'lat_end' (B,3,3), 'E_end', 'F_end', 'W_end' (unscaled), 'vol_end', the end 'state', 'status' (B,2),
        'n_made', 'E_hist', 'vol_hist', 'fmax_hist' (n_made,B), the frames 'R', 'lat' (only with record_every > 0) and
        'first_bad_step' (B)."""
        n3a = 3 * self.model_n_atoms
        S = np.array(S, dtype=np.float64, order='C').reshape(-1, n3a)
        B = S.shape[0]
        Cc, L0 = np.array(Cc, dtype=np.float64, order='C'), f64(L0)  # (order: a broadcast view would keep its strides)
        if Cc.shape != (B, 3, 3) or L0.shape != (B, 3, 3):
            raise ValueError('C and L0 must be ({}, 3, 3), got {} and {}'.format(B, Cc.shape, L0.shape))
        V = np.array(state['V'], dtype=np.float64, order='C')
        if V.shape != (B, n3a + 9):
            raise ValueError("state['V'] must be ({}, {}), got {}".format(B, n3a + 9, V.shape))
        dt, alpha, n_pos, n_taken = _replica_state(state, B, 'geometry')
        mask = None if mask is None else f64(mask)
        if mask is not None and mask.shape != (3, 3):
            raise ValueError('mask must be 3 x 3, got shape {}'.format(mask.shape))
        max_steps, record_every = int(max_steps), int(record_every)
        status, bad, (E_hist, v_hist, f_hist), (R_rec, lat_rec) = _frozen_arrays(B, max_steps, record_every, 3,
                                                                                 [(n3a,), (3, 3)])
        R_end, lat_end = np.empty((B, n3a)), np.empty((B, 3, 3))
        E_end, F_end, W_end, vol_end = np.empty(B), np.empty((B, n3a)), np.empty((B, 3, 3)), np.empty(B)
        prm = CellRelaxParams(B, self.model_n_atoms, float(f_scale), float(fmax), float(dt_max), float(max_step), float(f_inc),
                              float(f_dec), float(alpha_start), float(f_alpha), int(n_min), float(pressure), float(cell_factor),
                              _ptr(mask))
        self._check(self._lib.gdml_cell_relax_run(
            self._h, C.byref(prm), _ptr(S), _ptr(Cc), _ptr(L0), _ptr(V), _ptr(dt), _ptr(alpha), _ptr(n_pos), _ptr(n_taken),
            max_steps, record_every, _ptr(R_rec), _ptr(lat_rec), _ptr(E_hist), _ptr(v_hist), _ptr(f_hist), _ptr(R_end),
            _ptr(lat_end), _ptr(E_end), _ptr(F_end), _ptr(W_end), _ptr(vol_end), _ptr(status), _ptr(bad)))
        return dict(S=S, C=Cc, R_end=R_end, lat_end=lat_end, E_end=E_end, F_end=F_end, W_end=W_end, vol_end=vol_end,
                    state=dict(V=V, dt=dt, alpha=alpha, n_pos=n_pos, n_taken=n_taken),
                    **_frozen_out(status, bad, record_every, dict(E_hist=E_hist, vol_hist=v_hist, fmax_hist=f_hist),
                                  dict(R=R_rec, lat=lat_rec)))

    def npt_run(self, R, V, eps, p_eps, L0, L0_inv, mass, dt, n_steps, pressure, piston_mass, record_every=1, f_scale=1.0,
                thermostat=0, gamma=0.0, gamma_baro=0.0, kT=0.0, seed=0, step0=0, record=('R',)):
        """gdml_npt_run: B periodic replicas (R, V: (B,3N); eps, p_eps: (B); L0, L0_inv: (B,3,3)) advance n_steps at the
        pressure on the device.  Returns a dict with the end state 'R_end', 'V_end', 'eps_end', 'p_eps_end', the frames 'E' (n_rec,B;
        unscaled E'), 'Ekin', 'vol', 'press' (P_int), 'peps' (n_rec,B), those of 'R', 'V', 'F' (n_rec,B,3N) and 'lat'
        (n_rec,B,3,3) named in `record`, and 'first_bad_step' (B; -1 = every value stayed finite)."""
        n3 = 3 * self.model_n_atoms
        R, V = _state_copies(R, V, (-1, n3))
        B = R.shape[0]
        mass = self._masses(mass)
        eps, p_eps = np.array(eps, dtype=np.float64).ravel(), np.array(p_eps, dtype=np.float64).ravel()
        L0, L0_inv = f64(L0), f64(L0_inv)
        if eps.shape != (B,) or p_eps.shape != (B,):
            raise ValueError('eps and p_eps must have one entry per replica ({}), got {} and {}'.format(B, eps.shape, p_eps.shape))
        if L0.shape != (B, 3, 3) or L0_inv.shape != (B, 3, 3):
            raise ValueError('L0 and L0_inv must be ({}, 3, 3), got {} and {}'.format(B, L0.shape, L0_inv.shape))
        n_steps, record_every = int(n_steps), int(record_every)
        n_rec = n_steps // record_every if (n_steps > 0 and record_every > 0) else 0
        rec = _record_arrays(record, dict({k: (n_rec, B, n3) for k in ('R', 'V', 'F')}, lat=(n_rec, B, 3, 3)))
        E, Ek, vol, press, peps = (np.empty((n_rec, B)) for _ in range(5))
        bad = np.full(B, -1, dtype=np.int64)
        prm = NPTParams(B, self.model_n_atoms, float(dt), _ptr(mass), float(f_scale), int(thermostat), float(gamma),
                        float(gamma_baro), float(kT), int(seed), int(step0), float(pressure), float(piston_mass))
        self._check(self._lib.gdml_npt_run(self._h, C.byref(prm), _ptr(R), _ptr(V), _ptr(eps), _ptr(p_eps), _ptr(L0), _ptr(L0_inv),
                                           n_steps, record_every, _ptr(rec['R']), _ptr(rec['V']), _ptr(rec['F']), _ptr(rec['lat']),
                                           _ptr(E), _ptr(Ek), _ptr(vol), _ptr(press), _ptr(peps), _ptr(bad)))
        out = _recorded(rec)
        out.update(R_end=R, V_end=V, eps_end=eps, p_eps_end=p_eps, E=E, Ekin=Ek, vol=vol, press=press, peps=peps, first_bad_step=bad)
        return out

    def hessian_batch(self):
        """Geometries per gdml_predict_hessian call: max_query_batch scaled down by the 3N-fold larger output (9N^2 vs 3N)."""
        return max(1, self.max_query_batch // (3 * self.model_n_atoms))

    def predict_hessian(self, R, lat_and_inv=None):
        """Unscaled E' (B,), F (B,3N) and Hessian H' = d^2 E'/dR^2 (B,3N,3N) of geometries R (B,3N) (gdml_predict_hessian)."""
        if R is None:
            raise ValueError('predict_hessian needs geometries (there is no training-set mode)')
        n3 = 3 * self.model_n_atoms
        R = f64(R).reshape(-1, n3)
        B = R.shape[0]
        E, F, H = np.empty(B), np.empty((B, n3)), np.empty((B, n3, n3))
        lat, lat_inv = _lat_pair(lat_and_inv)
        step = self.hessian_batch()
        for b0 in range(0, max(B, 1), step):
            b1 = min(B, b0 + step)
            self._check(self._lib.gdml_predict_hessian(self._h, _ptr(R[b0:b1]), b1 - b0, _ptr(lat), _ptr(lat_inv),
                                                       _ptr(E[b0:b1]), _ptr(F[b0:b1]), _ptr(H[b0:b1])))
        return E, F, H

    def predict_hessian_dev(self, R_dev, B, E_dev, F_dev, H_dev, lat_and_inv=None):
        """gdml_predict_hessian_dev on device pointers (ints or c_void_p; E_dev / F_dev may be None)."""
        lat, lat_inv = _lat_pair(lat_and_inv)
        self._check(self._lib.gdml_predict_hessian_dev(self._h, R_dev, int(B), _ptr(lat), _ptr(lat_inv), E_dev, F_dev,
                                                       H_dev))

    def sym_eig(self, A, vectors=True):
        """gdml_sym_eig: eigenvalues w (M,n) ascending, eigenvectors V (M,n,n) as rows (largest component positive; None without
        `vectors`) and the Jacobi sweeps (M,) of symmetric matrices A (M,n,n)."""
        A = f64(A)
        if A.ndim != 3 or A.shape[1] != A.shape[2]:
            raise ValueError('A must be (M,n,n), got shape {}'.format(A.shape))
        M, n = A.shape[0], A.shape[1]
        w, V = np.empty((M, n)), (np.empty((M, n, n)) if vectors else None)
        sweeps = np.zeros(M, dtype=np.int64)
        self._check(self._lib.gdml_sym_eig(self._h, _ptr(A), M, n, _ptr(w), _ptr(V), _ptr(sweeps)))
        return w, V, sweeps

    def sym_eig_dev(self, A_dev, M, n, w_dev, V_dev, sweeps_dev=None):
        """gdml_sym_eig_dev on device pointers (ints or c_void_p; V_dev / sweeps_dev may be None, V_dev may be A_dev)."""
        self._check(self._lib.gdml_sym_eig_dev(self._h, A_dev, int(M), int(n), w_dev, V_dev, sweeps_dev))

    def vib_run(self, R, mass, h_scale=1.0, project=2, modes=False, lat_and_inv=None):
        """gdml_vib_run: squared frequencies of B geometries R (B,3N).  Returns a dict: 'w2' (B,3N), 'n_rigid', 'n_neg',
        'sweeps' (B), 'E' (B) and 'F' (B,3N) unscaled, and 'modes' (B,3N,3N) when asked for."""
        n3 = 3 * self.model_n_atoms
        R = f64(R).reshape(-1, n3)
        B = R.shape[0]
        mass = self._masses(mass)
        lat, lat_inv = _lat_pair(lat_and_inv)
        w2, E, F = np.empty((B, n3)), np.empty(B), np.empty((B, n3))
        md = np.empty((B, n3, n3)) if modes else None
        n_rigid, n_neg, sweeps = (np.zeros(B, dtype=np.int64) for _ in range(3))
        prm = VibParams(B, self.model_n_atoms, float(h_scale), _ptr(lat), _ptr(lat_inv), int(project))
        self._check(self._lib.gdml_vib_run(self._h, C.byref(prm), _ptr(R), _ptr(mass), _ptr(w2), _ptr(md), _ptr(n_rigid),
                                           _ptr(n_neg), _ptr(E), _ptr(F), _ptr(sweeps)))
        out = dict(w2=w2, n_rigid=n_rigid, n_neg=n_neg, sweeps=sweeps, E=E, F=F)
        if modes:
            out['modes'] = md
        return out

    def ef_run(self, R, fmax, max_steps, state, order=1, trust_min=1e-4, trust_max=0.3, project=2, f_scale=1.0, record_every=0,
               lat_and_inv=None):
        """gdml_ef_run: B geometries (R: (B,3N)) follow the Hessian's eigenvectors to a minimum (order=0) or a first-order saddle
        (order=1) on the device, at most max_steps steps each.  state: dict with 'trust', 'E_prev', 'dE_pred' (B), 'flags' (B,
        int) and 't' ((B,3N) follow vector, or None).  Returns a dict: 'R_end', 'E_end' (B; unscaled E'), 'F_end' (B,3N;
        unscaled), 'w_end' (B,3N), 'n_rigid', 'n_neg' (B), 'mode_end' (B,3N), the end 'state', 'status' (B,2; see the header),
        'n_made', 'E_hist', 'fmax_hist', 'w_follow_hist', 'k_follow_hist' (n_made,B), the frames 'R' (only with record_every > 0)
        and 'first_bad_step' (B; -1 = every value stayed finite)."""
        n3 = 3 * self.model_n_atoms
        R = np.array(R, dtype=np.float64).reshape(-1, n3)
        B = R.shape[0]
        trust, E_prev, dE_pred, flags = _replica_state(state, B, 'geometry', ('trust', 'E_prev', 'dE_pred'), ('flags',))
        t = state.get('t')
        if t is not None:
            t = np.array(t, dtype=np.float64)
            if t.shape != R.shape:
                raise ValueError("state['t'] must have the shape of R {}, got {}".format(R.shape, t.shape))
        lat, lat_inv = _lat_pair(lat_and_inv)
        max_steps, record_every = int(max_steps), int(record_every)
        status, bad, (E_hist, f_hist, w_hist), (R_rec,) = _frozen_arrays(B, max_steps, record_every, 3, [(n3,)])
        k_hist = np.zeros(E_hist.shape, dtype=np.int64)
        E_end, F_end, w_end, mode_end = np.empty(B), np.empty((B, n3)), np.empty((B, n3)), np.empty((B, n3))
        n_rigid, n_neg = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
        prm = EfParams(B, self.model_n_atoms, int(order), float(f_scale), _ptr(lat), _ptr(lat_inv), float(fmax), float(trust_min),
                       float(trust_max), int(project))
        self._check(self._lib.gdml_ef_run(self._h, C.byref(prm), _ptr(R), _ptr(trust), _ptr(E_prev), _ptr(dE_pred), _ptr(flags),
                                          _ptr(t), max_steps, record_every, _ptr(R_rec), _ptr(E_hist), _ptr(f_hist), _ptr(w_hist),
                                          _ptr(k_hist), _ptr(E_end), _ptr(F_end), _ptr(w_end), _ptr(n_rigid), _ptr(n_neg),
                                          _ptr(mode_end), _ptr(status), _ptr(bad)))
        return dict(R_end=R, E_end=E_end, F_end=F_end, w_end=w_end, n_rigid=n_rigid, n_neg=n_neg, mode_end=mode_end,
                    state=dict(trust=trust, E_prev=E_prev, dE_pred=dE_pred, flags=flags, t=t),
                    **_frozen_out(status, bad, record_every,
                                  dict(E_hist=E_hist, fmax_hist=f_hist, w_follow_hist=w_hist, k_follow_hist=k_hist), dict(R=R_rec)))

    def uncert_prepare(self, sig, lam):
        """Factor A = -K + lam I of the resident training set and keep it for predict_cov (gdml_uncert_prepare).  Raises
        numpy.linalg.LinAlgError when A is not positive definite, MemoryError when the n x n matrix does not fit."""
        info = C.c_int(0)
        self._check(self._lib.gdml_uncert_prepare(self._h, float(sig), float(lam), C.byref(info)))
        return info.value

    def uncert_release(self):
        """Free the factor and the work buffers of predict_cov (gdml_uncert_release)."""
        self._check(self._lib.gdml_uncert_release(self._h))

    def uncert_cross(self, R, lat_and_inv=None):
        """Un-negated cross-kernel rows Kx (B 3N, n) between geometries R and the resident training set, and k_qq (B,3N,3N)
        (gdml_uncert_cross)."""
        if not hasattr(self, 'n_atoms'):
            raise GDMLHipError('uncert_cross: no training set resident (train_upload)')
        n3 = 3 * self.n_atoms
        R = f64(R).reshape(-1, n3)
        B = R.shape[0]
        lat, lat_inv = _lat_pair(lat_and_inv)
        Kx, kqq = np.empty((B * n3, self.n_train * n3)), np.empty((B, n3, n3))
        self._check(self._lib.gdml_uncert_cross(self._h, _ptr(R), B, _ptr(lat), _ptr(lat_inv), _ptr(Kx), _ptr(kqq)))
        return Kx, kqq

    def predict_cov(self, R, lat_and_inv=None, full=False):
        """Posterior force covariance in normalised units (gdml_predict_cov): (B,3N) variances, or (B,3N,3N) with full."""
        if not hasattr(self, 'n_atoms'):
            raise GDMLHipError('predict_cov: no training set resident (train_upload, uncert_prepare)')
        n3 = 3 * self.n_atoms
        R = f64(R).reshape(-1, n3)
        B = R.shape[0]
        lat, lat_inv = _lat_pair(lat_and_inv)
        out = np.empty((B, n3, n3) if full else (B, n3))
        self._check(self._lib.gdml_predict_cov(self._h, _ptr(R), B, _ptr(lat), _ptr(lat_inv), int(bool(full)), _ptr(out)))
        return out

    def predict_cov_dev(self, R_dev, B, cov_dev, lat_and_inv=None, full=False):
        """gdml_predict_cov_dev on device pointers (ints or c_void_p)."""
        lat, lat_inv = _lat_pair(lat_and_inv)
        self._check(self._lib.gdml_predict_cov_dev(self._h, R_dev, int(B), _ptr(lat), _ptr(lat_inv), int(bool(full)),
                                                   cov_dev))

    def predict_cov_few(self, R, lat_and_inv=None, full=False):
        """predict_cov for a handful of geometries at low latency (gdml_predict_cov_few): the same quantity and shapes through a
        solve made for up to COV_FEW_ROWS = 256 rows 3N B; a larger batch is predict_cov itself, bit for bit."""
        if not hasattr(self, 'n_atoms'):
            raise GDMLHipError('predict_cov_few: no training set resident (train_upload, uncert_prepare)')
        n3 = 3 * self.n_atoms
        R = f64(R).reshape(-1, n3)
        B = R.shape[0]
        lat, lat_inv = _lat_pair(lat_and_inv)
        out = np.empty((B, n3, n3) if full else (B, n3))
        self._check(self._lib.gdml_predict_cov_few(self._h, _ptr(R), B, _ptr(lat), _ptr(lat_inv), int(bool(full)), _ptr(out)))
        return out

    def predict_cov_few_dev(self, R_dev, B, cov_dev, lat_and_inv=None, full=False):
        """gdml_predict_cov_few_dev on device pointers (ints or c_void_p)."""
        lat, lat_inv = _lat_pair(lat_and_inv)
        self._check(self._lib.gdml_predict_cov_few_dev(self._h, R_dev, int(B), _ptr(lat), _ptr(lat_inv), int(bool(full)),
                                                       cov_dev))

    def loo(self, alphas, cov=None):
        """Leave-one-out pass over the resident Cholesky factor (gdml_loo), in normalised units: (resid (M,3N), cov, logdet) with
        cov None, the (M,3N) diagonals ('diag') or the (M,3N,3N) covariances ('full') of the left-out labels, logdet = log det A.
        alphas: the library's coefficients -A^-1 y of this factor.  Raises numpy.linalg.LinAlgError when a diagonal block of
        A^-1 is not positive definite."""
        if cov not in (None, 'diag', 'full'):
            raise ValueError("cov must be None, 'diag' or 'full'")
        if not hasattr(self, 'n_atoms'):
            raise GDMLHipError('loo: no training set resident (train_upload)')
        alphas = f64(alphas).ravel()
        M, n3 = self.n_train, 3 * self.n_atoms
        resid = np.empty((M, n3))
        c = None if cov is None else np.empty((M, n3) if cov == 'diag' else (M, n3, n3))
        logdet, info = C.c_double(0.0), C.c_int(0)
        self._check(self._lib.gdml_loo(self._h, _ptr(alphas), alphas.size, {None: 0, 'diag': 1, 'full': 2}[cov], _ptr(resid),
                                       _ptr(c), C.byref(logdet), C.byref(info)))
        return resid, c, logdet.value

    def evidence_grad(self, alphas):
        """The five sums behind the gradient of the model evidence in sig and lam (gdml_evidence_grad), in normalised units:
        array (tr A^-1, <A^-1, K'>, a^T K' a, a^T a, log det A) with K' = dK/dsig at the factor's sig and a = -alphas, alphas
        the library's coefficients -A^-1 y of this factor.  The caller combines them with s^2:
        d lml / d sig = (<A^-1, K'> - a^T K' a / s^2) / 2, d lml / d lam = (a^T a / s^2 - tr A^-1) / 2.  The rows of L^-T are
        kept in a second matrix as large as the factor for the duration of the call: MemoryError when it does not fit."""
        if not hasattr(self, 'n_atoms'):
            raise GDMLHipError('evidence_grad: no training set resident (train_upload)')
        alphas = f64(alphas).ravel()
        terms, info = np.empty(5), C.c_int(0)
        self._check(self._lib.gdml_evidence_grad(self._h, _ptr(alphas), alphas.size, _ptr(terms), C.byref(info)))
        return terms

    def factor_extend(self, R_desc_new, R_d_desc_new):
        """Append training points (descriptors (b,D), compressed Jacobians (b,D,3)) to the training set and to the factor of
        uncert_prepare without factoring again (gdml_factor_extend).  Raises numpy.linalg.LinAlgError when the enlarged matrix
        is not positive definite and MemoryError when the second matrix buffer does not fit; the context is then unchanged."""
        if not hasattr(self, 'n_atoms'):
            raise GDMLHipError('factor_extend: no training set resident (train_upload, uncert_prepare)')
        D = self.n_atoms * (self.n_atoms - 1) // 2
        R_desc_new = f64(R_desc_new).reshape(-1, D)
        b = R_desc_new.shape[0]
        R_d_desc_new = f64(R_d_desc_new)
        if R_d_desc_new.shape != (b, D, 3):
            raise ValueError('R_d_desc_new must be the compressed (b,D,3) Jacobian')
        info = C.c_int(0)
        self._check(self._lib.gdml_factor_extend(self._h, _ptr(R_desc_new), _ptr(R_d_desc_new), b, C.byref(info)))
        if b:
            self._train_fp = None  # the resident set is no longer the one train_upload fingerprinted
            self.n_train += b
        return info.value

    def factor_remove(self, idx):
        """Remove the training points idx (distinct indices in the resident order) from the training set and from the factor
        of uncert_prepare without factoring again (gdml_factor_remove); the kept points keep their order.  Raises
        numpy.linalg.LinAlgError when a diagonal entry of the reduced factor is not positive and MemoryError when the second
        matrix buffer does not fit; the context is then unchanged."""
        if not hasattr(self, 'n_atoms'):
            raise GDMLHipError('factor_remove: no training set resident (train_upload, uncert_prepare)')
        idx = i64(idx).ravel()
        b = idx.size
        info = C.c_int(0)
        self._check(self._lib.gdml_factor_remove(self._h, _ptr(idx), b, C.byref(info)))
        if b:
            self._train_fp = None  # the resident set is no longer the one train_upload fingerprinted
            self.n_train -= b
        return info.value

    def select_points(self, R, lat_and_inv=None, n_select=0, min_gain=None):
        """Greedy selection of n_select of the candidate geometries R (B,3N) by joint information gain against the factor of
        uncert_prepare (gdml_select_points): (idx (k,) pool indices in pick order, gain (k,) their gains when picked,
        gain_initial (B,)), k <= n_select (fewer when the best remaining gain falls below min_gain).  n_select = 0 computes the
        initial gains only, streaming the pool.  Raises MemoryError when the retained rows of the pool do not fit (the
        message names the largest pool that would), numpy.linalg.LinAlgError for a candidate whose covariance is not
        positive definite."""
        if not hasattr(self, 'n_atoms'):
            raise GDMLHipError('select_points: no training set resident (train_upload, uncert_prepare)')
        n3 = 3 * self.n_atoms
        R = f64(R).reshape(-1, n3)
        B = R.shape[0]
        lat, lat_inv = _lat_pair(lat_and_inv)
        n_select = int(n_select)
        idx, gain, gain0 = np.zeros(max(n_select, 0), dtype=np.int64), np.zeros(max(n_select, 0)), np.empty(B)
        k, info = C.c_int64(0), C.c_int(0)
        self._check(self._lib.gdml_select_points(self._h, _ptr(R), B, _ptr(lat), _ptr(lat_inv), n_select,
                                                 -np.inf if min_gain is None else float(min_gain), _ptr(idx), _ptr(gain),
                                                 _ptr(gain0), C.byref(k), C.byref(info)))
        return idx[:k.value].copy(), gain[:k.value].copy(), gain0

    def predict_errors(self, R, F_ref, E_ref=None, std=1.0, c=0.0, lat_and_inv=None):
        """Eight error sums of a labelled batch, evaluated on the GPU (see gdml_predict_errors)."""
        n_atoms = self.model_n_atoms
        R = f64(R).reshape(-1, 3 * n_atoms)
        F_ref = f64(F_ref).reshape(R.shape[0], 3 * n_atoms)
        E_ref = None if E_ref is None else f64(E_ref).ravel()
        lat, lat_inv = _lat_pair(lat_and_inv)
        out = np.empty(8)
        self._check(self._lib.gdml_predict_errors(self._h, _ptr(R), R.shape[0], _ptr(lat), _ptr(lat_inv), float(std),
                                                  float(c), _ptr(E_ref), _ptr(F_ref), _ptr(out)))
        return out

    def kernel_matvec(self, lam, use_E_cstr, v):
        v = f64(v).ravel()
        out = np.empty_like(v)
        self._check(self._lib.gdml_kernel_matvec(self._h, float(lam), int(bool(use_E_cstr)), _ptr(v), v.size,
                                                 _ptr(out)))
        return out

    def _n_lev(self):
        n_rows, _, _ = self.K_shape()  # rows held by this rank
        _, world = self.comm_info()
        if world <= 1:
            return n_rows
        # sharded: the scores of ALL rows come back, in the reference order (forces, then energy constraints)
        return self.n_train * 3 * self.n_atoms + (self.n_train if getattr(self, '_last_use_E', False) else 0)

    def nystroem_factor(self, lam, idx, want_factor=False, want_lev=True):
        """(leverage scores or None, factor or None, info).  info is a bit field (gdml_nystroem_factor): bit 0 = the second
        Cholesky failed and the QR-equivalent branch ran (iterative.py:313-324); bit 1 = the preconditioner is applied
        matrix-free (option pcg.precon_form); info >> 8 = jitter escalations of the first Cholesky (iterative.py:442-463).
        want_lev=False: the scores are computed on demand by nystroem_lev_scores()."""
        idx = i64(idx)
        n_rows, _, _ = self.K_shape()
        lev = np.empty(self._n_lev()) if want_lev else None
        fac = np.empty((idx.size, n_rows)) if want_factor else None
        info = C.c_int(0)
        self._check(self._lib.gdml_nystroem_factor(self._h, float(lam), _ptr(idx), idx.size, _ptr(lev),
                                                   _ptr(fac), C.byref(info)))
        return lev, fac, info.value

    def nystroem_lev_scores(self):
        """Leverage scores of the resident Nystroem factor (gdml_nystroem_lev_scores): valid until the next assembly."""
        lev = np.empty(self._n_lev())
        self._check(self._lib.gdml_nystroem_lev_scores(self._h, _ptr(lev)))
        return lev

    def precon_apply(self, lam, v):
        v = f64(v).ravel()
        out = np.empty_like(v)
        self._check(self._lib.gdml_precon_apply(self._h, float(lam), _ptr(v), v.size, _ptr(out)))
        return out

    def pcg(self, lam, use_E_cstr, y, x0=None, rtol=1e-4, maxiter=1000, use_precon=True, callback=None,
            cb_every=1):
        """Preconditioned CG on the device (gdml_pcg).  callback(it, resid, fetch_x) is called every cb_every iterations;
        fetch_x() copies the iterate of THAT iteration to the host (the only way it crosses PCIe before the solve ends);
        a true return value stops the solve with that iterate.  Returns (x, info, iterations, residual norm)."""
        y = f64(y).ravel()
        n = y.size
        x0 = f64(x0)
        x = np.empty(n)
        iters, resid, info = C.c_int64(), C.c_double(), C.c_int()
        exc = []

        def _fetch_x():
            xk = np.empty(n)
            self._check(self._lib.gdml_pcg_x(self._h, _ptr(xk)))
            return xk

        def _cb(it, res, _user):
            try:
                return int(bool(callback(int(it), float(res), _fetch_x)))
            except BaseException as e:  # propagate after the C call returns
                exc.append(e)
                return 1

        cb = PCG_CB(_cb) if callback is not None else C.cast(None, PCG_CB)
        rc = self._lib.gdml_pcg(self._h, float(lam), int(bool(use_E_cstr)), _ptr(y), _ptr(x0), n, float(rtol),
                                int(maxiter), int(bool(use_precon)), cb, int(cb_every if callback else 0), None,
                                _ptr(x), C.byref(iters), C.byref(resid), C.byref(info))
        if exc:
            raise exc[0]
        self._check(rc)
        return x, info.value, iters.value, resid.value

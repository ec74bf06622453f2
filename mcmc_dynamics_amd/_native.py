"""ctypes binding of the C-ABI in ``include/mcd.h`` (``libmcd_hip.so``, built by ``csrc/Makefile``).

This is the only route from the Python host code to the GPU: there is no CPU fallback.  If the
library is missing or no gfx950 device is usable, the functions here raise ``NativeError``.
"""
import atexit
import ctypes
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MCD_LIB_PATH: A/B builds of the same library for kernel experiments (csrc/Makefile: variant); default = the in-tree build
LIB_PATH = os.environ.get("MCD_LIB_PATH") or os.path.join(_HERE, "libmcd_hip.so")

MODEL_CONST, MODEL_CONST_BGFIXED, MODEL_CONST_BGGAUSS = 0, 1, 2
MODEL_PROFILE, MODEL_PROFILE_BGGAUSS, MODEL_PROFILE_BGDENS, MODEL_PROFILE_BGFIXED = 3, 4, 5, 6
MODEL_DOUBLE, MODEL_DOUBLE_BGGAUSS = 7, 8        # two Lynden-Bell components (analysis/double_model.py); float64 only
# CONST / PROFILE with a fitted velocity-error scale: variance = err_scale^2 verr^2 + sigma_los^2 (analysis/error_scale.py);
# err_scale follows the cluster columns, in front of the centre; float64 only, no background
MODEL_CONST_ESCALE, MODEL_PROFILE_ESCALE = 10, 11      # (9 is not a model: mcd_catalog_create answers "unknown model")
CENTRE_FIXED, CENTRE_FREE = 0, 1
F64, F32, F32_ACC64 = 0, 1, 2
PRECISIONS = {"f64": F64, "f32": F32, "f32acc64": F32_ACC64}
UNIQUE_ID_BYTES = 128

_c_double_p = ctypes.POINTER(ctypes.c_double)
_c_int64_p = ctypes.POINTER(ctypes.c_int64)

# every symbol include/mcd.h declares: (restype, argtypes)
SYMBOLS = {
    "mcd_ctx_create": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_void_p)]),
    "mcd_get_unique_id": (ctypes.c_int, [ctypes.c_void_p]),
    "mcd_ctx_create_rank": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                           ctypes.POINTER(ctypes.c_void_p)]),
    "mcd_ctx_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "mcd_ctx_set_option": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64]),
    "mcd_ctx_abort": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p]),
    "mcd_ctx_failed": (ctypes.c_int, [ctypes.c_void_p]),
    "mcd_ctx_n_devices": (ctypes.c_int, [ctypes.c_void_p]),
    "mcd_ctx_comm_info": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                         ctypes.POINTER(ctypes.c_int)]),
    "mcd_catalog_create": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]),
    "mcd_catalog_destroy": (ctypes.c_int, [ctypes.c_void_p]),
    "mcd_catalog_param_count": (ctypes.c_int, [ctypes.c_void_p]),
    "mcd_catalog_n_stars": (ctypes.c_int64, [ctypes.c_void_p]),
    "mcd_catalog_n_outputs": (ctypes.c_int64, [ctypes.c_void_p, ctypes.c_int64]),
    "mcd_loglike_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, _c_double_p, _c_double_p]),
    "mcd_loglike_grad_batch": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, _c_double_p, _c_double_p,
                                              _c_double_p]),
    "mcd_params_upload": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, _c_double_p]),
    "mcd_loglike_enqueue": (ctypes.c_int, [ctypes.c_void_p]),
    "mcd_loglike_fetch": (ctypes.c_int, [ctypes.c_void_p, _c_double_p]),
    "mcd_sync": (ctypes.c_int, [ctypes.c_void_p]),
    "mcd_membership": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _c_double_p, _c_double_p]),
    "mcd_loglike_per_star": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _c_double_p, _c_double_p]),
    "mcd_pointwise_posterior": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, _c_double_p, _c_double_p,
                                               _c_double_p, _c_double_p, _c_double_p]),
    "mcd_psis_loo": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, _c_double_p, ctypes.c_double,
                                    _c_double_p, _c_double_p, _c_double_p, _c_double_p]),
    "mcd_posterior_predictive": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, _c_double_p, _c_double_p,
                                                _c_double_p]),
    "mcd_psis_loo_expect": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, _c_double_p, ctypes.c_double,
                                           ctypes.c_int32, _c_double_p, _c_double_p, _c_double_p, _c_double_p, _c_double_p,
                                           _c_double_p]),
    "mcd_holdout_loglike": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _c_int64_p, ctypes.c_int64, ctypes.c_int32, _c_double_p,
                                           _c_double_p, _c_double_p]),
    "mcd_holdout_pointwise": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, _c_int64_p, ctypes.c_int64, ctypes.c_int32,
                                             _c_double_p, _c_double_p, _c_double_p]),
    "mcd_replicate_check": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, _c_double_p, ctypes.c_uint64,
                                           ctypes.c_int32, _c_int64_p, _c_int64_p, ctypes.c_double, ctypes.c_double, _c_double_p]),
    "mcd_replicate_numbers": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                             _c_double_p, _c_double_p]),
    "mcd_weighted_loglike_grad": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, _c_double_p, ctypes.c_void_p,
                                                 _c_double_p, _c_double_p]),
    "mcd_weighted_loglike": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, _c_double_p, ctypes.c_void_p,
                                            _c_double_p]),
    "mcd_simulate": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, _c_double_p, ctypes.c_uint64, ctypes.c_int64,
                                    ctypes.c_double, ctypes.c_double, _c_double_p]),
    "mcd_simulated_set": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, _c_double_p, ctypes.c_double, ctypes.c_double]),
    "mcd_simulated_loglike": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, _c_double_p, _c_int64_p,
                                             _c_double_p]),
    "mcd_simulated_loglike_grad": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, _c_double_p, _c_int64_p,
                                                  _c_double_p, _c_double_p]),
    "mcd_simulated_info": (ctypes.c_int, [ctypes.c_void_p, _c_int64_p]),
    "mcd_bootstrap_weights": (ctypes.c_int, [ctypes.c_int32, ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                             ctypes.c_int64, _c_double_p]),
    "mcd_moment_match": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, _c_double_p,
                                        ctypes.c_int64, _c_int64_p, _c_double_p, _c_double_p, _c_double_p, _c_double_p,
                                        _c_double_p, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                        _c_double_p, _c_double_p]),
    "mcd_kde_background": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, _c_double_p, ctypes.c_int64, _c_double_p,
                                          _c_double_p, ctypes.c_double, _c_double_p, _c_double_p]),
    "mcd_stretch_move": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, _c_double_p, _c_double_p,
                                        ctypes.POINTER(ctypes.c_int32), _c_double_p, _c_double_p,
                                        ctypes.POINTER(ctypes.c_int32), _c_double_p, _c_double_p, _c_int64_p]),
    "mcd_stretch_move_seeded": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, _c_double_p, _c_double_p,
                                               ctypes.c_uint64, ctypes.c_int64, _c_double_p, _c_double_p, _c_int64_p]),
    "mcd_chain_numbers": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                         ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), _c_double_p, _c_double_p,
                                         ctypes.POINTER(ctypes.c_int32)]),
    "mcd_stretch_info": (ctypes.c_int, [ctypes.c_void_p, _c_int64_p, _c_int64_p, _c_int64_p, ctypes.POINTER(ctypes.c_int32)]),
    "mcd_de_move": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, _c_double_p, _c_double_p,
                                   ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32),
                                   ctypes.POINTER(ctypes.c_int32), _c_double_p, _c_double_p, _c_double_p, _c_double_p,
                                   _c_int64_p]),
    "mcd_de_move_seeded": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_double,
                                          ctypes.c_int64, _c_double_p, _c_double_p, ctypes.c_uint64, ctypes.c_int64,
                                          _c_double_p, _c_double_p, _c_int64_p]),
    "mcd_de_numbers": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                      ctypes.c_int32, ctypes.c_double, ctypes.c_double, ctypes.POINTER(ctypes.c_int32),
                                      ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32), _c_double_p,
                                      _c_double_p]),
    "mcd_de_info": (ctypes.c_int, [ctypes.c_void_p, _c_int64_p, _c_int64_p, _c_int64_p, ctypes.POINTER(ctypes.c_int32)]),
    "mcd_hmc_block": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, _c_double_p, _c_double_p,
                                     ctypes.c_uint64, ctypes.c_int64, _c_double_p, _c_double_p, _c_int64_p, _c_double_p]),
    "mcd_hmc_numbers": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32,
                                       _c_double_p, _c_double_p, _c_double_p]),
    "mcd_hmc_info": (ctypes.c_int, [ctypes.c_void_p, _c_int64_p, _c_int64_p]),
    "mcd_prior_eval": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, _c_double_p, _c_double_p, _c_double_p]),
    "mcd_stretch_move_prior": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, _c_double_p, _c_double_p,
                                              ctypes.POINTER(ctypes.c_int32), _c_double_p, _c_double_p,
                                              ctypes.POINTER(ctypes.c_int32), _c_double_p, _c_double_p, _c_int64_p,
                                              ctypes.c_void_p]),
    "mcd_stretch_move_seeded_prior": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, _c_double_p,
                                                     _c_double_p, ctypes.c_uint64, ctypes.c_int64, _c_double_p, _c_double_p,
                                                     _c_int64_p, ctypes.c_void_p]),
    "mcd_hmc_block_prior": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, _c_double_p, _c_double_p,
                                           ctypes.c_uint64, ctypes.c_int64, _c_double_p, _c_double_p, _c_int64_p, _c_double_p,
                                           ctypes.c_void_p]),
    "mcd_temper_block": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, _c_double_p, _c_double_p, _c_double_p,
                                        ctypes.c_uint64, ctypes.c_int64, _c_double_p, _c_double_p, _c_int64_p, _c_int64_p,
                                        _c_int64_p]),
    "mcd_temper_block_prior": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, _c_double_p, _c_double_p,
                                              _c_double_p, ctypes.c_uint64, ctypes.c_int64, _c_double_p, _c_double_p,
                                              _c_int64_p, _c_int64_p, _c_int64_p, ctypes.c_void_p]),
    "mcd_temper_numbers": (ctypes.c_int, [ctypes.c_uint64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int32, ctypes.c_int64,
                                          _c_double_p]),
    "mcd_temper_info": (ctypes.c_int, [ctypes.c_void_p, _c_int64_p, _c_int64_p]),
    "mcd_chain_diagnostics": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, _c_double_p, _c_double_p, _c_int64_p,
                                             ctypes.POINTER(ctypes.c_int32), _c_double_p, _c_double_p, _c_double_p,
                                             _c_double_p]),
    "mcd_chain_diagnostics_info": (ctypes.c_int, [_c_int64_p, _c_int64_p, _c_double_p]),
    "mcd_last_error": (ctypes.c_char_p, []),
    "mcd_abi_version": (ctypes.c_int, []),
    "mcd_last_kernel_ms": (ctypes.c_double, [ctypes.c_void_p]),
    "mcd_last_device_ms": (ctypes.c_double, [ctypes.c_void_p]),
    "mcd_timing_collect": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_int64_p]),
    "mcd_rerun_count": (ctypes.c_int64, [ctypes.c_void_p]),
    "mcd_last_prefetch": (ctypes.c_int, [ctypes.c_void_p]),
    "mcd_last_narrow_bounded": (ctypes.c_int, [ctypes.c_void_p]),
    "mcd_last_series_chunks": (ctypes.c_int64, [ctypes.c_void_p]),
    "mcd_last_direct_chunks": (ctypes.c_int64, [ctypes.c_void_p]),
    "mcd_last_exp_split": (ctypes.c_int, [ctypes.c_void_p]),
    "mcd_last_root_quad": (ctypes.c_int, [ctypes.c_void_p]),
    "mcd_last_quad_chunks": (ctypes.c_int64, [ctypes.c_void_p]),
    "mcd_last_block_step": (ctypes.c_int, [ctypes.c_void_p]),
    "mcd_last_fast_level": (ctypes.c_int, [ctypes.c_void_p]),
    "mcd_last_f32_domain": (ctypes.c_int, [ctypes.c_void_p, _c_double_p, _c_double_p]),
    "mcd_f32_outside": (ctypes.c_int, [ctypes.c_void_p, _c_int64_p, _c_double_p, _c_double_p, ctypes.POINTER(ctypes.c_char_p)]),
    "mcd_set_option": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64]),
    "mcd_last_launch_info": (ctypes.c_int, [ctypes.c_void_p, _c_int64_p, ctypes.POINTER(ctypes.c_int32), _c_int64_p,
                                            ctypes.POINTER(ctypes.c_int32)]),
}


class NativeError(RuntimeError):
    """Raised when the HIP library is missing, fails to load, or a call returns an error status."""


class CatalogDesc(ctypes.Structure):
    """Mirror of ``mcd_catalog_desc``."""
    _fields_ = [
        ("n_stars", ctypes.c_int64),
        ("ra", _c_double_p), ("dec", _c_double_p), ("v", _c_double_p), ("verr", _c_double_p),
        ("lnlike_bg", _c_double_p), ("pmember", _c_double_p), ("density", _c_double_p),
        ("model", ctypes.c_int32), ("centre", ctypes.c_int32), ("precision", ctypes.c_int32),
        ("reserved", ctypes.c_int32),
        ("ra_center", ctypes.c_double), ("dec_center", ctypes.c_double),
        ("n_bins", ctypes.c_int64), ("bin_offsets", _c_int64_p),
    ]


class StretchDesc(ctypes.Structure):
    """Mirror of ``mcd_stretch_desc``."""
    _fields_ = [
        ("n_walkers", ctypes.c_int64), ("n_dim", ctypes.c_int32), ("k", ctypes.c_int32),
        ("col_source", ctypes.POINTER(ctypes.c_int32)), ("col_const", _c_double_p), ("col_factor", _c_double_p),
        ("lo", _c_double_p), ("hi", _c_double_p), ("fixed_ok", ctypes.c_int32), ("n_bins", ctypes.c_int32),
    ]


class PriorDesc(ctypes.Structure):
    """Mirror of ``mcd_prior_desc``."""
    _fields_ = [("n_dim", ctypes.c_int32), ("kind", ctypes.POINTER(ctypes.c_int32)), ("p0", _c_double_p), ("p1", _c_double_p)]


PRIOR_FLAT, PRIOR_NORMAL, PRIOR_LOGNORMAL = 0, 1, 2


class WeightDesc(ctypes.Structure):
    """Mirror of ``mcd_weight_desc``."""
    _fields_ = [("scheme", ctypes.c_int32), ("seed", ctypes.c_uint64), ("n_replicates", ctypes.c_int64),
                ("row_replicate", _c_int64_p), ("weights", _c_double_p)]


WEIGHT_EXPONENTIAL, WEIGHT_POISSON, WEIGHT_EXPLICIT = 0, 1, 2
WEIGHT_SCHEMES = {"exponential": WEIGHT_EXPONENTIAL, "poisson": WEIGHT_POISSON, "explicit": WEIGHT_EXPLICIT}


def _weight_scheme(scheme):
    if isinstance(scheme, str):
        if scheme not in WEIGHT_SCHEMES:
            raise ValueError("scheme must be one of {0}".format(sorted(WEIGHT_SCHEMES)))
        return WEIGHT_SCHEMES[scheme]
    return int(scheme)


def _prior_desc(prior):
    """``prior``: (kind int32 [P], p0 float64 [P], p1 float64 [P]) -> (PriorDesc, the arrays it points to)."""
    kind = np.ascontiguousarray(prior[0], dtype=np.int32)
    p0, p1 = _f64(prior[1]), _f64(prior[2])
    if kind.ndim != 1 or p0.shape != kind.shape or p1.shape != kind.shape:
        raise ValueError("a prior is three arrays of one length: kind, p0, p1")
    d = PriorDesc()
    d.n_dim = kind.size
    d.kind, d.p0, d.p1 = kind.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _ptr(p0), _ptr(p1)
    return d, (kind, p0, p1)


def prior_eval(prior, x, want_grad=False):
    """``mcd_prior_eval``: the log-prior of the rows ``x`` (n, P) under the structured priors ``prior`` = (kind, p0, p1)
    (include/mcd.h: 0 flat, 1 normal (loc, scale), 2 lognormal (mu, s)), WITHOUT the box: -inf where a lognormal coordinate
    is <= 0.  Host code of the library (csrc/mcd_prior.h, the text the device kernels compile): the library's own bits, no
    device involved.  -> values (n,) [, derivatives (n, P)]"""
    lib = load_library()
    x = _f64(np.atleast_2d(x))
    d, _keep = _prior_desc(prior)
    if x.shape[1] != d.n_dim:
        raise ValueError("prior_eval: x must have shape (n, {0})".format(d.n_dim))
    value = np.empty(x.shape[0])
    grad = np.empty(x.shape) if want_grad else None
    _check(lib, lib.mcd_prior_eval(ctypes.byref(d), x.shape[0], _ptr(x), _ptr(value), _ptr(grad)), "mcd_prior_eval")
    return (value, grad) if want_grad else value


class DiagDesc(ctypes.Structure):
    """Mirror of ``mcd_diag_desc``."""
    _fields_ = [("n_steps", ctypes.c_int64), ("n_groups", ctypes.c_int64), ("n_walkers", ctypes.c_int64),
                ("n_dim", ctypes.c_int32), ("max_lag", ctypes.c_int64), ("c", ctypes.c_double), ("scratch_mb", ctypes.c_int64)]


def chain_diagnostics(chain, max_lag, c=5.0, context=None, scratch_mb=0, want_rho=False):
    """``mcd_chain_diagnostics`` on ``chain`` (T, G, W, P) float64, steps first (include/mcd.h; csrc/mcd_diag.h): a dict of
    ``tau``, ``window``, ``found``, ``rhat``, ``mean``, ``var`` of shape (G, P) [, ``rho`` (G, P, max_lag + 1)].
    ``context=None``: the library's host loop, no device involved; a ``Context``: its first device, the chain going up in
    tiles of whole groups within ``scratch_mb`` MiB (0: 1024) -- the same bits either way."""
    lib = load_library()
    chain = _f64(chain)
    if chain.ndim != 4:
        raise ValueError("chain_diagnostics: chain must have shape (steps, groups, walkers, parameters)")
    T, G, W, P = chain.shape
    d = DiagDesc(T, G, W, P, int(max_lag), float(c), int(scratch_mb))
    out = {"tau": np.empty((G, P)), "window": np.empty((G, P), dtype=np.int64), "found": np.empty((G, P), dtype=np.int32),
           "rhat": np.empty((G, P)), "mean": np.empty((G, P)), "var": np.empty((G, P))}
    if want_rho:
        out["rho"] = np.empty((G, P, max(int(max_lag), 0) + 1))
    handle = None
    if context is not None:
        handle = getattr(context, "handle", None)
        if not handle:
            raise NativeError("context is closed")
    rc = lib.mcd_chain_diagnostics(handle, ctypes.byref(d), _ptr(chain), _ptr(out["tau"]),
                                   out["window"].ctypes.data_as(_c_int64_p),
                                   out["found"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _ptr(out["rhat"]),
                                   _ptr(out["mean"]), _ptr(out["var"]), _ptr(out.get("rho")))
    _check(lib, rc, "mcd_chain_diagnostics")
    return out


def chain_diagnostics_info():
    """Of this thread's last ``chain_diagnostics``: {'tile_groups', 'n_tiles', 'kernel_ms'} (include/mcd.h)."""
    lib = load_library()
    tg, nt, ms = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_double()
    _check(lib, lib.mcd_chain_diagnostics_info(ctypes.byref(tg), ctypes.byref(nt), ctypes.byref(ms)),
           "mcd_chain_diagnostics_info")
    return {"tile_groups": tg.value, "n_tiles": nt.value, "kernel_ms": ms.value}


class HmcDesc(ctypes.Structure):
    """Mirror of ``mcd_hmc_desc``."""
    _fields_ = [("map", StretchDesc), ("chol", _c_double_p), ("step_size", ctypes.c_double), ("jitter", ctypes.c_double),
                ("n_leap", ctypes.c_int32)]


class MmatchDesc(ctypes.Structure):
    """Mirror of ``mcd_mmatch_desc``."""
    _fields_ = [("map", StretchDesc), ("max_iters", ctypes.c_int32), ("cov", ctypes.c_int32), ("split", ctypes.c_int32),
                ("k_threshold", ctypes.c_double), ("r_eff", ctypes.c_double)]


class TemperDesc(ctypes.Structure):
    """Mirror of ``mcd_temper_desc``."""
    _fields_ = [("map", StretchDesc), ("n_temps", ctypes.c_int32), ("betas", _c_double_p), ("n_chain_temps", ctypes.c_int32)]


# Environment switches the library or this binding reads (INTEGRATION.md lists them).  None is needed in production: they
# select test stand-ins or tuning values, so load_library() says so on the package logger when one is set.
TEST_SWITCHES = ("MCD_LIB_PATH", "MCD_RCCL_LIBRARY", "MCD_ALLOW_SHARED_DEVICE", "MCD_FORCE_RCCL", "MCD_TARGET_WAVES",
                 "MCD_CHAIN_PART_BYTES", "MCD_CHAIN_PARTS", "MCD_COLLECTIVE_TIMEOUT_MS")

_lib = None
_live_catalogs = weakref.WeakSet()
_live_contexts = weakref.WeakSet()


@atexit.register
def _shutdown():
    """Release device objects in dependency order (catalogues, then contexts) while the interpreter
    and the HIP runtime are both still fully alive; nothing is left for __del__ at teardown."""
    for cat in list(_live_catalogs):
        try:
            cat.close()
        except Exception:
            pass
    for ctx in list(_live_contexts):
        try:
            ctx.close()
        except Exception:
            pass


def load_library(path=None):
    """Load ``libmcd_hip.so`` and declare every entry point.  Raises NativeError if it is absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise NativeError(
            "HIP library not found at {0}: build it with `make -C mcmc_dynamics_amd/csrc` "
            "(or __graft_entry__.build()); there is no CPU fallback.".format(p))
    try:
        lib = ctypes.CDLL(p)
    except OSError as exc:
        raise NativeError("could not load {0}: {1}".format(p, exc))
    for name, (restype, argtypes) in SYMBOLS.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise NativeError("{0} does not export {1}".format(p, name))
        fn.restype = restype
        fn.argtypes = argtypes
    if path is None:
        _lib = lib
        active = ["{0}={1}".format(k, os.environ[k]) for k in TEST_SWITCHES if os.environ.get(k)]
        if active:
            import logging
            logging.getLogger("mcmc_dynamics_amd").warning(
                "test / tuning switches active (none is needed in production, see INTEGRATION.md): %s", ", ".join(active))
    return lib


def _check(lib, rc, what):
    if rc != 0:
        msg = lib.mcd_last_error()
        raise NativeError("{0} failed (status {1}): {2}".format(what, rc, msg.decode() if msg else ""))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
    return a.ctypes.data_as(_c_double_p) if a is not None else None


class Context(object):
    """HIP devices + streams (+ RCCL communicator).  One per process."""

    def __init__(self, n_devices=1, device_ids=None, rank=None, n_ranks=None, unique_id=None, device=None):
        self.lib = load_library()
        handle = ctypes.c_void_p()
        if rank is not None:
            uid = ctypes.create_string_buffer(bytes(unique_id), UNIQUE_ID_BYTES) if unique_id is not None else None
            rc = self.lib.mcd_ctx_create_rank(int(device or 0), int(rank), int(n_ranks), uid, ctypes.byref(handle))
            _check(self.lib, rc, "mcd_ctx_create_rank")
            self.rank, self.n_ranks = int(rank), int(n_ranks)
        else:
            ids = None
            if device_ids is not None:
                ids = (ctypes.c_int * len(device_ids))(*[int(d) for d in device_ids])
                n_devices = len(device_ids)
            rc = self.lib.mcd_ctx_create(int(n_devices), ids, ctypes.byref(handle))
            _check(self.lib, rc, "mcd_ctx_create")
            self.rank, self.n_ranks = 0, 1
        self.handle = handle
        self.host_group = None                    # hostgroup.HostGroup of a multi-rank job (distributed.rank_context)
        self._catalogs = weakref.WeakSet()        # catalogues living on this context: closed before it
        _live_contexts.add(self)

    @staticmethod
    def unique_id():
        lib = load_library()
        buf = ctypes.create_string_buffer(UNIQUE_ID_BYTES)
        _check(lib, lib.mcd_get_unique_id(buf), "mcd_get_unique_id")
        return buf.raw

    @property
    def n_devices(self):
        return self.lib.mcd_ctx_n_devices(self.handle)

    def set_option(self, key, value):
        """Context options (include/mcd.h): ``collective_timeout_ms`` -- how long a wait on a stream that carries an
        all-reduce may last before the call returns an error and the context is marked failed (0: for ever)."""
        _check(self.lib, self.lib.mcd_ctx_set_option(self.handle, key.encode(), int(value)), "mcd_ctx_set_option")

    def abort(self, reason=""):
        """Make a call of ANOTHER thread that is waiting for a collective on this context return an error now (thread-safe;
        what ``hostgroup.HostGroup`` calls when a peer rank reports a failure)."""
        if getattr(self, "handle", None):
            self.lib.mcd_ctx_abort(self.handle, str(reason).encode()[:400])

    @property
    def failed(self):
        """True after a collective deadline, an abort, or an error in the middle of a resident block: every later call on
        this context raises; the process is expected to exit non-zero (no fallback inside it)."""
        return bool(getattr(self, "handle", None)) and bool(self.lib.mcd_ctx_failed(self.handle))

    def comm_info(self):
        """What RCCL reports for this context's communicator: {'size', 'rank', 'rccl_version'} (size 0: none)."""
        n, r, v = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _check(self.lib, self.lib.mcd_ctx_comm_info(self.handle, ctypes.byref(n), ctypes.byref(r), ctypes.byref(v)),
               "mcd_ctx_comm_info")
        return {"size": n.value, "rank": r.value, "rccl_version": v.value}

    def kde_background(self, comp, v, verr, sigma_int=0.0, return_kernel_ms=False):
        """``background.SingleStars.__call__`` (single_stars.py:42-77) for km/s arrays: (n,) log-likelihoods."""
        if not getattr(self, "handle", None):
            raise NativeError("context is closed")
        comp, v, verr = _f64(comp).ravel(), _f64(v).ravel(), _f64(verr).ravel()
        if v.shape != verr.shape:
            raise ValueError("v and verr must have the same shape")
        out = np.empty(v.size, dtype=np.float64)
        ms = ctypes.c_double(0.0)
        rc = self.lib.mcd_kde_background(self.handle, comp.size, _ptr(comp), v.size, _ptr(v), _ptr(verr),
                                         float(sigma_int), _ptr(out), ctypes.byref(ms))
        _check(self.lib, rc, "mcd_kde_background")
        return (out, ms.value) if return_kernel_ms else out

    def close(self):
        if getattr(self, "handle", None):
            for cat in list(getattr(self, "_catalogs", ())):
                cat.close()
            self.lib.mcd_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = None


def default_context():
    """Process-wide single-GPU context (device 0), created on first use."""
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(n_devices=1)
    return _default_ctx


def chain_numbers(seed, step0, n_steps, n_bins, n_walkers, n_dim, squeeze=False):
    """``mcd_chain_numbers``: the random numbers of steps ``step0 .. step0 + n_steps - 1`` of the seeded chain (host code, no
    device involved): order (steps, B, W) int32, zz / thr / pick (steps, 2, B, W/2), in the layout ``stretch_move`` takes.
    ``squeeze``: drop the ensemble axis (n_bins <= 1, a catalogue without bins)."""
    lib = load_library()
    b, w = max(int(n_bins), 1), int(n_walkers)
    order = np.empty((n_steps, b, w), dtype=np.int32)
    zz = np.empty((n_steps, 2, b, w // 2), dtype=np.float64)
    thr = np.empty_like(zz)
    pick = np.empty((n_steps, 2, b, w // 2), dtype=np.int32)
    rc = lib.mcd_chain_numbers(int(seed) & 0xFFFFFFFFFFFFFFFF, int(step0), int(n_steps), b, w, int(n_dim),
                               order.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _ptr(zz), _ptr(thr),
                               pick.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    _check(lib, rc, "mcd_chain_numbers")
    if squeeze:
        return order[:, 0], zz[:, :, 0], thr[:, :, 0], pick[:, :, 0]
    return order, zz, thr, pick


def de_numbers(seed, step0, n_steps, n_bins, n_walkers, n_dim, gamma0, sigma, squeeze=False):
    """``mcd_de_numbers``: the random numbers of steps ``step0 .. step0 + n_steps - 1`` of the seeded differential-evolution
    chain (host code, no device involved; csrc/mcd_de.h): order (steps, B, W) int32, pick_a / pick_b int32 and gamma / thr
    float64 (steps, 2, B, W/2), in the layout ``de_move`` takes.  ``squeeze``: drop the ensemble axis (n_bins <= 1)."""
    lib = load_library()
    b, w, n = max(int(n_bins), 1), int(n_walkers), int(n_steps)
    i32 = ctypes.POINTER(ctypes.c_int32)
    order = np.empty((n, b, w), dtype=np.int32)
    pick_a = np.empty((n, 2, b, w // 2), dtype=np.int32)
    pick_b = np.empty_like(pick_a)
    gamma = np.empty((n, 2, b, w // 2), dtype=np.float64)
    thr = np.empty_like(gamma)
    rc = lib.mcd_de_numbers(int(seed) & 0xFFFFFFFFFFFFFFFF, int(step0), n, b, w, int(n_dim), float(gamma0), float(sigma),
                            order.ctypes.data_as(i32), pick_a.ctypes.data_as(i32), pick_b.ctypes.data_as(i32), _ptr(gamma),
                            _ptr(thr))
    _check(lib, rc, "mcd_de_numbers")
    if squeeze:
        return order[:, 0], pick_a[:, :, 0], pick_b[:, :, 0], gamma[:, :, 0], thr[:, :, 0]
    return order, pick_a, pick_b, gamma, thr


def hmc_numbers(seed, step0, n_steps, n_walkers, n_dim):
    """``mcd_hmc_numbers``: the numbers of steps ``step0 .. step0 + n_steps - 1`` of the HMC chain that ``seed`` names (host
    code, no device involved): standard normals z (steps, W, P), acceptance thresholds thr = log(u) (steps, W) and the
    step-size jitter variables r in [-1, 1) (steps, W); a step runs with eps = step_size (1 + jitter r)."""
    lib = load_library()
    z = np.empty((int(n_steps), int(n_walkers), int(n_dim)), dtype=np.float64)
    thr = np.empty((int(n_steps), int(n_walkers)), dtype=np.float64)
    r = np.empty_like(thr)
    rc = lib.mcd_hmc_numbers(int(seed) & 0xFFFFFFFFFFFFFFFF, int(step0), int(n_steps), int(n_walkers), int(n_dim), _ptr(z),
                             _ptr(thr), _ptr(r))
    _check(lib, rc, "mcd_hmc_numbers")
    return z, thr, r


def replicate_numbers(seed, sample0, n_samples, star0, n_stars):
    """``mcd_replicate_numbers``: the numbers of ``replicate_check`` for sample rows ``sample0 ..`` and stars ``star0 ..``
    (host code, no device involved): standard normals g and membership uniforms u, both (n_samples, n_stars)."""
    lib = load_library()
    g = np.empty((int(n_samples), int(n_stars)), dtype=np.float64)
    u = np.empty_like(g)
    rc = lib.mcd_replicate_numbers(int(seed) & 0xFFFFFFFFFFFFFFFF, int(sample0), int(n_samples), int(star0), int(n_stars),
                                   _ptr(g), _ptr(u))
    _check(lib, rc, "mcd_replicate_numbers")
    return g, u


def bootstrap_weights(scheme, seed, rep0, n_reps, star0, n_stars):
    """``mcd_bootstrap_weights``: the star weights that ``Catalog.weighted_loglike_grad`` generates on the device for
    replicates ``rep0 ..`` and stars ``star0 ..`` (host code, no device involved, the same bits), (n_reps, n_stars).
    ``scheme``: "exponential" (Exp(1), the weighted-likelihood bootstrap) or "poisson" (Poisson(1) counts)."""
    lib = load_library()
    w = np.empty((int(n_reps), int(n_stars)), dtype=np.float64)
    rc = lib.mcd_bootstrap_weights(_weight_scheme(scheme), int(seed) & 0xFFFFFFFFFFFFFFFF, int(rep0), int(n_reps), int(star0),
                                   int(n_stars), _ptr(w))
    _check(lib, rc, "mcd_bootstrap_weights")
    return w


def temper_numbers(seed, step0, n_steps, n_temps, n_walkers):
    """``mcd_temper_numbers``: the swap thresholds log(u) of steps ``step0 .. step0 + n_steps - 1`` of the tempered chain that
    ``seed`` names (host code, no device involved), shape (steps, T - 1, W): pair t is rungs (t, t + 1); a step exchanges the
    pairs of its own parity only.  The stretch-move numbers of the rungs are ``chain_numbers(..., n_bins=T, ...)``."""
    lib = load_library()
    thr = np.empty((int(n_steps), max(int(n_temps) - 1, 0), int(n_walkers)), dtype=np.float64)
    rc = lib.mcd_temper_numbers(int(seed) & 0xFFFFFFFFFFFFFFFF, int(step0), int(n_steps), int(n_temps), int(n_walkers), _ptr(thr))
    _check(lib, rc, "mcd_temper_numbers")
    return thr


class Catalog(object):
    """Star records resident in HBM; evaluates the log-likelihood of batches of walkers."""

    def __init__(self, ctx, ra, dec, v, verr, model=MODEL_CONST, centre=None, lnlike_bg=None, pmember=None,
                 density=None, bin_offsets=None, precision="f64"):
        self.ctx = ctx
        self.lib = ctx.lib
        cols = [_f64(ra), _f64(dec), _f64(v), _f64(verr)]
        n = cols[0].size
        if any(c.size != n for c in cols):
            raise ValueError("ra, dec, v, verr must have the same length")
        extras = [None if a is None else _f64(a) for a in (lnlike_bg, pmember, density)]
        if any(a is not None and a.size != n for a in extras):
            raise ValueError("background columns must have the same length as the catalogue")
        d = CatalogDesc()
        d.n_stars = n
        d.ra, d.dec, d.v, d.verr = (_ptr(c) for c in cols)
        d.lnlike_bg, d.pmember, d.density = (_ptr(a) for a in extras)
        d.model = int(model)
        d.precision = PRECISIONS[precision] if isinstance(precision, str) else int(precision)
        if centre is None:
            d.centre = CENTRE_FREE
        else:
            d.centre = CENTRE_FIXED
            d.ra_center, d.dec_center = float(centre[0]), float(centre[1])
        offs = None
        if bin_offsets is not None and len(bin_offsets) > 2:
            offs = np.ascontiguousarray(bin_offsets, dtype=np.int64)
            d.n_bins = offs.size - 1
            d.bin_offsets = offs.ctypes.data_as(_c_int64_p)
        else:
            d.n_bins = 0
        handle = ctypes.c_void_p()
        rc = self.lib.mcd_catalog_create(ctx.handle, ctypes.byref(d), ctypes.byref(handle))
        _check(self.lib, rc, "mcd_catalog_create")
        self.handle = handle
        self.n_stars = n
        self.n_sets = max(1, int(d.n_bins))
        self.k = self.lib.mcd_catalog_param_count(handle)
        self._walkers = 0
        _live_catalogs.add(self)
        ctx._catalogs.add(self)

    def _params(self, params):
        p = _f64(params)
        if p.ndim == 1:
            p = p[None, :]
        if self.n_sets > 1:
            if p.ndim != 3 or p.shape[0] != self.n_sets:
                raise ValueError("binned catalogue expects params of shape (n_bins, W, K)")
            w = p.shape[1]
        else:
            if p.ndim == 3 and p.shape[0] == 1:
                p = p[0]
            if p.ndim != 2:
                raise ValueError("params must have shape (W, K)")
            w = p.shape[0]
        if p.shape[-1] != self.k:
            raise ValueError("params have {0} columns, catalogue expects {1}".format(p.shape[-1], self.k))
        return np.ascontiguousarray(p), w

    def _alive(self):
        if not getattr(self, "handle", None):
            raise NativeError("catalogue is closed")

    def loglike(self, params):
        """(W, K) -> (W,)   [binned: (B, W, K) -> (B, W)]   synchronous."""
        self._alive()
        p, w = self._params(params)
        out = np.empty((self.n_sets, w) if self.n_sets > 1 else (w,), dtype=np.float64)
        rc = self.lib.mcd_loglike_batch(self.handle, w, self.k, _ptr(p), _ptr(out))
        _check(self.lib, rc, "mcd_loglike_batch")
        self._walkers = w
        return out

    def loglike_grad(self, params, want_value=True):
        """Value and gradient with respect to the K kernel columns (kernel units: km/s, arcsec, degrees):
        (W, K) -> ((W,), (W, K))   [binned: (B, W, K) -> ((B, W), (B, W, K))].  float64 catalogues only; synchronous and
        bit-identical from run to run.  ``want_value=False`` passes a null value pointer and returns (None, grad)."""
        self._alive()
        p, w = self._params(params)
        lead = (self.n_sets, w) if self.n_sets > 1 else (w,)
        out = np.empty(lead, dtype=np.float64) if want_value else None
        grad = np.empty(lead + (self.k,), dtype=np.float64)
        rc = self.lib.mcd_loglike_grad_batch(self.handle, w, self.k, _ptr(p), _ptr(out), _ptr(grad))
        _check(self.lib, rc, "mcd_loglike_grad_batch")
        self._walkers = w
        return out, grad

    def upload_params(self, params):
        p, w = self._params(params)
        _check(self.lib, self.lib.mcd_params_upload(self.handle, w, self.k, _ptr(p)), "mcd_params_upload")
        self._walkers = w

    def enqueue(self):
        _check(self.lib, self.lib.mcd_loglike_enqueue(self.handle), "mcd_loglike_enqueue")

    def sync(self):
        _check(self.lib, self.lib.mcd_sync(self.handle), "mcd_sync")

    def fetch(self):
        w = self._walkers
        out = np.empty((self.n_sets, w) if self.n_sets > 1 else (w,), dtype=np.float64)
        _check(self.lib, self.lib.mcd_loglike_fetch(self.handle, _ptr(out)), "mcd_loglike_fetch")
        return out

    def membership(self, params_row):
        p = _f64(params_row).reshape(-1)
        out = np.empty(self.n_stars, dtype=np.float64)
        _check(self.lib, self.lib.mcd_membership(self.handle, p.size, _ptr(p), _ptr(out)), "mcd_membership")
        return out

    def loglike_per_star(self, params_row):
        p = _f64(params_row).reshape(-1)
        out = np.empty(self.n_stars, dtype=np.float64)
        _check(self.lib, self.lib.mcd_loglike_per_star(self.handle, p.size, _ptr(p), _ptr(out)), "mcd_loglike_per_star")
        return out

    def pointwise_posterior(self, table, membership=False):
        """Per-star summaries over S posterior samples: ``table`` (S, K) in the kernel's column order -> dict of (n_stars,)
        arrays ``lppd`` (log of the sample mean of exp(lnL_is)) and ``lnl_var`` (sample variance of lnL_is), and with
        ``membership`` (background models only) ``pmem_mean`` / ``pmem_std`` of the membership probability."""
        self._alive()
        if self.n_sets > 1:
            raise ValueError("pointwise_posterior is defined for un-binned catalogues only")
        p = _f64(table)
        if p.ndim == 1:
            p = p[None, :]
        if p.ndim != 2 or p.shape[1] != self.k:
            raise ValueError("table must have shape (S, {0})".format(self.k))
        p = np.ascontiguousarray(p)
        names = ("lppd", "lnl_var") + (("pmem_mean", "pmem_std") if membership else ())
        out = {k: np.empty(self.n_stars, dtype=np.float64) for k in names}
        ptrs = [_ptr(out[k]) if k in out else None for k in ("lppd", "lnl_var", "pmem_mean", "pmem_std")]
        rc = self.lib.mcd_pointwise_posterior(self.handle, p.shape[0], self.k, _ptr(p), *ptrs)
        _check(self.lib, rc, "mcd_pointwise_posterior")
        return out

    def psis_loo(self, table, r_eff=1.0):
        """PSIS-LOO per star over S posterior samples: ``table`` (S, K) in the kernel's column order -> dict of (n_stars,)
        arrays ``elpd_loo``, ``pareto_k`` (the fitted shape k^), ``lppd`` and ``n_eff`` (include/mcd.h: mcd_psis_loo)."""
        self._alive()
        if self.n_sets > 1:
            raise ValueError("psis_loo is defined for un-binned catalogues only")
        p = _f64(table)
        if p.ndim == 1:
            p = p[None, :]
        if p.ndim != 2 or p.shape[1] != self.k:
            raise ValueError("table must have shape (S, {0})".format(self.k))
        p = np.ascontiguousarray(p)
        names = ("elpd_loo", "pareto_k", "lppd", "n_eff")
        out = {k: np.empty(self.n_stars, dtype=np.float64) for k in names}
        rc = self.lib.mcd_psis_loo(self.handle, p.shape[0], self.k, _ptr(p), float(r_eff), *[_ptr(out[k]) for k in names])
        _check(self.lib, rc, "mcd_psis_loo")
        return out

    PREDICTIVE_FIELDS = ("z_mean", "z_std", "tail_p", "pit", "vlos_mean", "vlos_std", "sigma_mean", "sigma_std")

    def posterior_predictive(self, table, mixture=False):
        """Per-star posterior predictive checks over S posterior samples: ``table`` (S, K) in the kernel's column order ->
        dict of (n_stars,) arrays ``z_mean`` / ``z_std`` (standardised residual against the cluster component), ``tail_p``
        (mean two-sided tail probability), ``pit`` (mean cluster-component CDF at v_i), ``vlos_mean`` / ``vlos_std`` and
        ``sigma_mean`` / ``sigma_std`` (the model's v_los and sigma_los at the star), and with ``mixture`` (the two models
        with a Gaussian background only) ``pit_mix``, the CDF of the whole mixture (include/mcd.h: mcd_posterior_predictive)."""
        self._alive()
        if self.n_sets > 1:
            raise ValueError("posterior_predictive is defined for un-binned catalogues only")
        p = _f64(table)
        if p.ndim == 1:
            p = p[None, :]
        if p.ndim != 2 or p.shape[1] != self.k:
            raise ValueError("table must have shape (S, {0})".format(self.k))
        p = np.ascontiguousarray(p)
        block = np.empty((len(self.PREDICTIVE_FIELDS), self.n_stars), dtype=np.float64)
        mix = np.empty(self.n_stars, dtype=np.float64) if mixture else None
        rc = self.lib.mcd_posterior_predictive(self.handle, p.shape[0], self.k, _ptr(p), _ptr(block),
                                               _ptr(mix) if mixture else None)
        _check(self.lib, rc, "mcd_posterior_predictive")
        out = {k: block[f] for f, k in enumerate(self.PREDICTIVE_FIELDS)}
        if mixture:
            out["pit_mix"] = mix
        return out

    LOO_EXPECT_FIELDS = ("pit", "z", "vlos", "sigma")
    LOO_MAX_FUNC = 16

    def psis_loo_expect(self, table, r_eff=1.0, func=None, predictive=True, mixture=False):
        """Leave-one-out expectations per star under the PSIS weights of ``psis_loo`` (include/mcd.h: mcd_psis_loo_expect):
        ``table`` (S, K) in the kernel's column order -> dict of (n_stars,) arrays ``pareto_k`` and ``n_eff`` (bit for bit
        those of ``psis_loo``); with ``predictive`` the expectations ``pit`` (the LOO-PIT), ``z``, ``vlos`` and ``sigma`` of
        the (star, sample) term of ``posterior_predictive``; with ``mixture`` (the two models with a Gaussian background
        only) ``pit_mix``; and with ``func`` (S, Q), Q <= 16 star-independent functions of the sample, ``func`` (n_stars, Q):
        the expectation of every column with each star left out."""
        self._alive()
        if self.n_sets > 1:
            raise ValueError("psis_loo_expect is defined for un-binned catalogues only")
        p = _f64(table)
        if p.ndim == 1:
            p = p[None, :]
        if p.ndim != 2 or p.shape[1] != self.k:
            raise ValueError("table must have shape (S, {0})".format(self.k))
        p = np.ascontiguousarray(p)
        n_func, f, loo_func = 0, None, None
        if func is not None:
            f = _f64(func)
            if f.ndim == 1:
                f = f[:, None]
            if f.ndim != 2 or f.shape[0] != p.shape[0]:
                raise ValueError("func must have shape ({0}, Q)".format(p.shape[0]))
            f = np.ascontiguousarray(f)
            n_func = f.shape[1]
            loo_func = np.empty((n_func, self.n_stars), dtype=np.float64)
        pred = np.empty((len(self.LOO_EXPECT_FIELDS), self.n_stars), dtype=np.float64) if predictive else None
        mix = np.empty(self.n_stars, dtype=np.float64) if mixture else None
        out = {k: np.empty(self.n_stars, dtype=np.float64) for k in ("pareto_k", "n_eff")}
        rc = self.lib.mcd_psis_loo_expect(self.handle, p.shape[0], self.k, _ptr(p), float(r_eff), n_func,
                                          _ptr(f) if n_func else None, _ptr(loo_func) if n_func else None, _ptr(pred) if predictive else None,
                                          _ptr(mix) if mixture else None, _ptr(out["pareto_k"]), _ptr(out["n_eff"]))
        _check(self.lib, rc, "mcd_psis_loo_expect")
        if predictive:
            out.update({k: pred[i] for i, k in enumerate(self.LOO_EXPECT_FIELDS)})
        if mixture:
            out["pit_mix"] = mix
        if func is not None:
            out["func"] = np.ascontiguousarray(loo_func.T)
        return out

    def _holdout_args(self, set_offsets, table):
        offs = np.ascontiguousarray(set_offsets, dtype=np.int64).reshape(-1)
        if offs.size < 2:
            raise ValueError("set_offsets must hold n_sets + 1 >= 2 offsets")
        p = _f64(table)
        if p.ndim != 3 or p.shape[0] != offs.size - 1 or p.shape[2] != self.k:
            raise ValueError("table must have shape ({0}, rows, {1})".format(offs.size - 1, self.k))
        return offs, np.ascontiguousarray(p)

    def holdout_loglike(self, set_offsets, table, want_test=True):
        """Hold-out evaluation (include/mcd.h: mcd_holdout_loglike): ``set_offsets`` (E + 1,) star offsets of the sets, which
        are consecutive prefixes of the catalogue, ``table`` (E, W, K) kernel rows -> (train (E, W), test (E, W)): the sum of
        the per-star terms outside / inside row e's set.  ``want_test=False`` passes a null pointer and returns (train, None).
        Un-binned float64 catalogues on one device; synchronous and bit-identical from run to run."""
        self._alive()
        offs, p = self._holdout_args(set_offsets, table)
        train = np.empty(p.shape[:2], dtype=np.float64)
        test = np.empty(p.shape[:2], dtype=np.float64) if want_test else None
        rc = self.lib.mcd_holdout_loglike(self.handle, offs.size - 1, offs.ctypes.data_as(_c_int64_p), p.shape[1], p.shape[2],
                                          _ptr(p), _ptr(train), _ptr(test))
        _check(self.lib, rc, "mcd_holdout_loglike")
        return train, test

    def holdout_pointwise(self, set_offsets, table):
        """Hold-out pointwise summaries (include/mcd.h: mcd_holdout_pointwise): ``table`` (E, S, K), the S sample rows of
        every set's own refit -> dict of (set_offsets[E],) arrays ``lppd`` and ``lnl_var`` for the held-out stars, each
        under its own set's samples."""
        self._alive()
        offs, p = self._holdout_args(set_offsets, table)
        n = int(offs[-1]) if 0 <= int(offs[-1]) <= self.n_stars else 0
        out = {k: np.empty(n, dtype=np.float64) for k in ("lppd", "lnl_var")}
        rc = self.lib.mcd_holdout_pointwise(self.handle, offs.size - 1, offs.ctypes.data_as(_c_int64_p), p.shape[1], p.shape[2],
                                            _ptr(p), _ptr(out["lppd"]), _ptr(out["lnl_var"]))
        _check(self.lib, rc, "mcd_holdout_pointwise")
        return out

    def weighted_loglike_grad(self, table, row_replicate, scheme="exponential", seed=0, weights=None, want_value=True,
                              want_grad=True):
        """Value and gradient under per-row star weights (include/mcd.h: mcd_weighted_loglike_grad): ``table`` (R, K) kernel
        rows, ``row_replicate`` (R,) int64 the replicate of every row -> ((R,), (R, K)): sum_i w(b, i) l_i and its gradient
        with respect to the K kernel columns.  ``scheme``: "exponential" or "poisson" (weights generated on the device from
        (seed, replicate, star); ``bootstrap_weights`` gives the same numbers), or "explicit" with ``weights``
        (n_replicates, n_stars), finite and >= 0, which ``row_replicate`` indexes.  Weights are not normalised; a star of
        weight 0 adds exactly +0.0 whatever its term.  ``want_value`` / ``want_grad`` = False pass a null pointer and return
        None in its place.  Un-binned float64 catalogues on one device; synchronous and bit-identical from run to run."""
        p, d, keep = self._weight_desc(table, row_replicate, scheme, seed, weights)
        out = np.empty(p.shape[0], dtype=np.float64) if want_value else None
        grad = np.empty(p.shape, dtype=np.float64) if want_grad else None
        rc = self.lib.mcd_weighted_loglike_grad(self.handle, p.shape[0], self.k, _ptr(p), ctypes.byref(d), _ptr(out), _ptr(grad))
        _check(self.lib, rc, "mcd_weighted_loglike_grad")
        return out, grad

    def _weight_desc(self, table, row_replicate, scheme, seed, weights):
        """The checked table, the mcd_weight_desc of a weighted call and the arrays it points into (to be kept alive)."""
        self._alive()
        p = _f64(table)
        if p.ndim == 1:
            p = p[None, :]
        if p.ndim != 2 or p.shape[1] != self.k:
            raise ValueError("table must have shape (R, {0})".format(self.k))
        p = np.ascontiguousarray(p)
        rep = np.ascontiguousarray(row_replicate, dtype=np.int64).reshape(-1)
        if rep.size != p.shape[0]:
            raise ValueError("row_replicate must hold one replicate per row of the table")
        d = WeightDesc()
        d.scheme = _weight_scheme(scheme)
        d.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        d.row_replicate = rep.ctypes.data_as(_c_int64_p)
        w = None
        if weights is not None:
            w = np.ascontiguousarray(_f64(weights))
            if w.ndim != 2 or w.shape[1] != self.n_stars:
                raise ValueError("weights must have shape (n_replicates, {0})".format(self.n_stars))
            d.n_replicates = w.shape[0]
        d.weights = _ptr(w)
        return p, d, (rep, w)

    def weighted_loglike(self, table, row_replicate, scheme="exponential", seed=0, weights=None):
        """The value alone under per-row star weights (include/mcd.h: mcd_weighted_loglike): the arguments of
        ``weighted_loglike_grad`` -> (R,) sum_i w(b, i) l_i, from a kernel that carries one sum per row and no partial
        derivative: what a chain under bootstrap weights (``Runner.bagged``) evaluates twice per step.  Agrees with
        ``weighted_loglike_grad``'s value to rounding.  Un-binned float64 catalogues on one device; synchronous and
        bit-identical from run to run."""
        p, d, keep = self._weight_desc(table, row_replicate, scheme, seed, weights)
        out = np.empty(p.shape[0], dtype=np.float64)
        rc = self.lib.mcd_weighted_loglike(self.handle, p.shape[0], self.k, _ptr(p), ctypes.byref(d), _ptr(out))
        _check(self.lib, rc, "mcd_weighted_loglike")
        return out

    def simulate(self, truth_table, seed, sim0=0, bg_mean=float("nan"), bg_sigma=float("nan"), want_velocities=True):
        """Simulated catalogues drawn on the device (include/mcd.h: mcd_simulate): ``truth_table`` (E, K) kernel rows ->
        (E, n_stars) velocities, simulation ``sim0 + e`` drawn from the model at row e on the observed positions and
        ``verr``, with the numbers ``replicate_numbers(seed, sim0 + e, 1, 0, n_stars)``.  The set stays resident on the
        catalogue's device for ``simulated_loglike`` and replaces the previous one.  ``bg_mean`` / ``bg_sigma``: the
        background's Gaussian for the fixed-background models.  ``want_velocities`` = False passes a null pointer and
        returns None.  Un-binned float64 catalogues on one device; synchronous and bit-identical from run to run."""
        self._alive()
        p = _f64(truth_table)
        if p.ndim == 1:
            p = p[None, :]
        if p.ndim != 2 or p.shape[1] != self.k:
            raise ValueError("truth_table must have shape (E, {0})".format(self.k))
        p = np.ascontiguousarray(p)
        out = np.empty((p.shape[0], self.n_stars), dtype=np.float64) if want_velocities else None
        rc = self.lib.mcd_simulate(self.handle, p.shape[0], self.k, _ptr(p), int(seed) & 0xFFFFFFFFFFFFFFFF, int(sim0),
                                   float(bg_mean), float(bg_sigma), _ptr(out))
        _check(self.lib, rc, "mcd_simulate")
        return out

    def simulated_set(self, velocities, bg_mean=float("nan"), bg_sigma=float("nan")):
        """Make the caller's own mock velocities the resident set (include/mcd.h: mcd_simulated_set): ``velocities``
        (E, n_stars), finite -- an N-body snapshot, or a catalogue with injected binaries that the model cannot draw.
        ``bg_mean`` / ``bg_sigma``: the Gaussian the fixed-background models evaluate the background term with."""
        self._alive()
        v = _f64(velocities)
        if v.ndim == 1:
            v = v[None, :]
        if v.ndim != 2 or v.shape[1] != self.n_stars:
            raise ValueError("velocities must have shape (E, {0})".format(self.n_stars))
        v = np.ascontiguousarray(v)
        rc = self.lib.mcd_simulated_set(self.handle, v.shape[0], _ptr(v), float(bg_mean), float(bg_sigma))
        _check(self.lib, rc, "mcd_simulated_set")

    def simulated_loglike(self, table, row_sim):
        """Every row against the velocities of its own simulation (include/mcd.h: mcd_simulated_loglike): ``table`` (R, K)
        kernel rows, ``row_sim`` (R,) int64 the simulation of the resident set that every row is evaluated on -> (R,)
        sum_i l_i with the simulated velocity in place of the observed one: what the lock-stepped fits of
        ``Runner.simulated_fits`` evaluate twice per step.  Several rows may share a simulation.  Un-binned float64
        catalogues on one device; synchronous and, given the resident set, bit-identical from run to run."""
        self._alive()
        p = _f64(table)
        if p.ndim == 1:
            p = p[None, :]
        if p.ndim != 2 or p.shape[1] != self.k:
            raise ValueError("table must have shape (R, {0})".format(self.k))
        p = np.ascontiguousarray(p)
        sim = np.ascontiguousarray(row_sim, dtype=np.int64).reshape(-1)
        if sim.size != p.shape[0]:
            raise ValueError("row_sim must hold one simulation per row of the table")
        out = np.empty(p.shape[0], dtype=np.float64)
        rc = self.lib.mcd_simulated_loglike(self.handle, p.shape[0], self.k, _ptr(p), sim.ctypes.data_as(_c_int64_p), _ptr(out))
        _check(self.lib, rc, "mcd_simulated_loglike")
        return out

    def simulated_loglike_grad(self, table, row_sim, want_value=True):
        """``simulated_loglike`` with its gradient (include/mcd.h: mcd_simulated_loglike_grad): ``table`` (R, K) kernel rows,
        ``row_sim`` (R,) -> (values (R,), grad (R, K)) with respect to the kernel columns, in their units, every row on the
        velocities of its own simulation: what a MAP fit per simulated catalogue climbs (``Runner.simulated_maximize``).
        The values have ``simulated_loglike``'s bits.  ``want_value=False`` passes no value buffer and returns (None,
        grad) with the same gradient.  Un-binned float64 catalogues on one device; synchronous and, given the resident
        set, bit-identical from run to run."""
        self._alive()
        p = _f64(table)
        if p.ndim == 1:
            p = p[None, :]
        if p.ndim != 2 or p.shape[1] != self.k:
            raise ValueError("table must have shape (R, {0})".format(self.k))
        p = np.ascontiguousarray(p)
        sim = np.ascontiguousarray(row_sim, dtype=np.int64).reshape(-1)
        if sim.size != p.shape[0]:
            raise ValueError("row_sim must hold one simulation per row of the table")
        out = np.empty(p.shape[0], dtype=np.float64) if want_value else None
        grad = np.empty((p.shape[0], self.k), dtype=np.float64)
        rc = self.lib.mcd_simulated_loglike_grad(self.handle, p.shape[0], self.k, _ptr(p), sim.ctypes.data_as(_c_int64_p),
                                                 _ptr(out) if want_value else None, _ptr(grad))
        _check(self.lib, rc, "mcd_simulated_loglike_grad")
        return out, grad

    @property
    def simulated_sims(self):
        """Simulations of the resident set (include/mcd.h: mcd_simulated_info), 0 when there is none."""
        self._alive()
        n = ctypes.c_int64(0)
        _check(self.lib, self.lib.mcd_simulated_info(self.handle, ctypes.byref(n)), "mcd_simulated_info")
        return int(n.value)

    REPLICATE_FIELDS = ("s1", "s2", "s3", "s4", "sin", "cos", "max", "tail3")

    def replicate_check(self, table, seed, range_offsets, order, bg_mean=float("nan"), bg_sigma=float("nan"), row0=0):
        """Replicated-data predictive checks per range of stars (include/mcd.h: mcd_replicate_check): ``table`` (S, K)
        kernel rows, ``order`` the star indices of range 0, then of range 1, ..., ``range_offsets`` (R + 1,) the ranges'
        offsets into it -> (S, R, 8, 2) float64: the fields ``REPLICATE_FIELDS`` of the observed ([..., 0]) and of the
        replicated ([..., 1]) standardised residuals.  ``bg_mean`` / ``bg_sigma``: the background's Gaussian for the
        fixed-background models.  ``row0``: the generator's index of the first row (option ``replicate_row0``), for
        tables that are split over several calls.  Un-binned float64 catalogues on one device; synchronous and
        bit-identical from run to run."""
        self._alive()
        p = _f64(table)
        if p.ndim == 1:
            p = p[None, :]
        if p.ndim != 2 or p.shape[1] != self.k:
            raise ValueError("table must have shape (S, {0})".format(self.k))
        p = np.ascontiguousarray(p)
        offs = np.ascontiguousarray(range_offsets, dtype=np.int64).reshape(-1)
        if offs.size < 2:
            raise ValueError("range_offsets must hold n_ranges + 1 >= 2 offsets")
        order = np.ascontiguousarray(order, dtype=np.int64).reshape(-1)
        if order.size != int(offs[-1]):
            raise ValueError("order must hold range_offsets[-1] = {0} indices".format(int(offs[-1])))
        out = np.empty((p.shape[0], offs.size - 1, len(self.REPLICATE_FIELDS), 2), dtype=np.float64)
        self.set_option("replicate_row0", int(row0))
        rc = self.lib.mcd_replicate_check(self.handle, p.shape[0], self.k, _ptr(p), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                          offs.size - 1, offs.ctypes.data_as(_c_int64_p), order.ctypes.data_as(_c_int64_p),
                                          float(bg_mean), float(bg_sigma), _ptr(out))
        _check(self.lib, rc, "mcd_replicate_check")
        return out

    def moment_match(self, plan, draws, stars, k_threshold, max_iters=30, cov=True, split=True, r_eff=1.0, out=None):
        """Moment matching for PSIS-LOO (include/mcd.h: mcd_moment_match; csrc/mcd_mmatch.h): ``plan`` as for
        ``stretch_move`` (column map, box, ``fixed_ok``, optional ``prior``), ``draws`` (S, P) posterior draws of the free
        parameters, ``stars`` ascending distinct star indices -> dict of per-star arrays ``elpd``, ``pareto_k``, ``n_eff``,
        ``k_before``, ``k_loop`` (n,), ``iterations`` (n,), ``accepted`` (n, 3) int32, and the total affine maps ``A``
        (n, P, P), ``b`` (n, P).  ``max_iters=0`` is the baseline: plain PSIS by the hold-out terms.  ``out``: such a dict
        of C-contiguous arrays to write into (a refused call leaves them as they were)."""
        self._alive()
        x = np.ascontiguousarray(_f64(draws))
        if x.ndim != 2:
            raise ValueError("moment_match: draws must have shape (S, P)")
        S, P = x.shape
        idx = np.ascontiguousarray(stars, dtype=np.int64).reshape(-1)
        head, _tail, _keep = self._stretch_args("moment_match", plan, x[:2], np.zeros(min(S, 2)), 0, None, None, None)
        d = MmatchDesc()
        d.map = head[1]._obj
        d.map.n_bins = 1
        d.max_iters, d.cov, d.split = int(max_iters), int(bool(cov)), int(bool(split))
        d.k_threshold, d.r_eff = float(k_threshold), float(r_eff)
        n = idx.size
        if out is None:
            out = {k: np.empty(n) for k in ("elpd", "pareto_k", "n_eff", "k_before", "k_loop")}
            out["iterations"] = np.empty(n, dtype=np.int32)
            out["accepted"] = np.empty((n, 3), dtype=np.int32)
            out["A"], out["b"] = np.empty((n, P, P)), np.empty((n, P))
        shapes = {"iterations": (n,), "accepted": (n, 3), "A": (n, P, P), "b": (n, P)}
        for key, a in out.items():
            want = np.int32 if key in ("iterations", "accepted") else np.float64
            if a.dtype != want or not a.flags.c_contiguous or a.shape != shapes.get(key, (n,)):
                raise ValueError("moment_match: out['{0}'] has the wrong dtype, layout or shape".format(key))
        i32 = ctypes.POINTER(ctypes.c_int32)
        prior = self._prior_arg[0] if self._prior_arg is not None else None
        rc = self.lib.mcd_moment_match(self.handle, ctypes.byref(d), prior, S, _ptr(x), n, idx.ctypes.data_as(_c_int64_p),
                                       _ptr(out["elpd"]), _ptr(out["pareto_k"]), _ptr(out["n_eff"]), _ptr(out["k_before"]),
                                       _ptr(out["k_loop"]), out["iterations"].ctypes.data_as(i32),
                                       out["accepted"].ctypes.data_as(i32), _ptr(out["A"]), _ptr(out["b"]))
        _check(self.lib, rc, "mcd_moment_match")
        return out

    def _stretch_args(self, name, plan, pos, lnp, n_steps, chain, lnprob_chain, accepted):
        """What both kinds of block check and pass: ``pos`` ([B,] W, P) and ``lnp`` ([B,] W), the descriptor built from
        ``plan``, the optional outputs.  Returns the C call's leading and trailing arguments and the arrays they point to."""
        self._alive()
        for a in (pos, lnp):
            if a.dtype != np.float64 or not a.flags.c_contiguous:
                raise ValueError(name + " needs C-contiguous arrays of the documented dtypes")
        if pos.ndim not in (2, 3) or lnp.shape != pos.shape[:-1]:
            raise ValueError(name + ": inconsistent array shapes")
        lead, (w, p) = pos.shape[:-2], pos.shape[-2:]
        cols = [np.ascontiguousarray(plan["col_source"], dtype=np.int32), _f64(plan["col_const"]), _f64(plan["col_factor"]),
                _f64(plan["lo"]), _f64(plan["hi"])]
        if cols[0].size != self.k or cols[1].size != self.k or cols[2].size != self.k or cols[3].size != p or cols[4].size != p:
            raise ValueError("stretch_move: plan does not match the catalogue / the number of free parameters")
        d = StretchDesc()
        d.n_walkers, d.n_dim, d.k, d.n_bins = w, p, self.k, lead[0] if lead else 1
        d.col_source = cols[0].ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
        d.col_const, d.col_factor, d.lo, d.hi = (_ptr(c) for c in cols[1:])
        d.fixed_ok = 1 if plan.get("fixed_ok", True) else 0
        for a, shape in ((chain, (n_steps,) + lead + (w, p)), (lnprob_chain, (n_steps,) + lead + (w,))):
            if a is not None and (a.dtype != np.float64 or not a.flags.c_contiguous or a.shape != shape):
                raise ValueError("stretch_move: chain buffers must be C-contiguous float64 of shape (steps, [B,] W, P) / (steps, [B,] W)")
        if accepted is not None and (accepted.dtype != np.int64 or accepted.shape != lead + (w,) or not accepted.flags.c_contiguous):
            raise ValueError("stretch_move: accepted must be a C-contiguous int64 array of shape ([B,] W)")
        # a plan with a "prior" entry ((kind, p0, p1) over the free parameters, or None) takes the *_prior entry points
        self._prior_arg = None
        if "prior" in plan:
            pd = None
            if plan["prior"] is not None:
                pd, keep = _prior_desc(plan["prior"])
                cols.append(keep)
            self._prior_arg = (ctypes.byref(pd) if pd is not None else None,)
        return ((self.handle, ctypes.byref(d), n_steps, _ptr(pos), _ptr(lnp)),
                (_ptr(chain), _ptr(lnprob_chain), accepted.ctypes.data_as(_c_int64_p) if accepted is not None else None), cols)

    def stretch_move(self, plan, pos, lnp, order, zz, thr, pick, chain=None, lnprob_chain=None, accepted=None):
        """``mcd_stretch_move``: advance the ensemble by ``len(order)`` stretch-move steps with the half-step loop inside
        the library.  ``plan``: dict with ``col_source`` (int32 [K]), ``col_const``, ``col_factor`` (float64 [K]), ``lo``,
        ``hi`` (float64 [P]) and ``fixed_ok``; an entry ``prior`` -- ``(kind, p0, p1)`` over the free parameters
        (``prior_eval``) or None -- selects ``mcd_stretch_move_prior`` (and the ``_prior`` form of the seeded and the HMC
        block), whose ``lnp`` is log-likelihood plus log-prior.  ``pos`` (W, P) and ``lnp`` (W,) are C-contiguous float64 arrays updated
        in place; random numbers as drawn by ``sampler.EnsembleSampler``.

        Binned catalogues: ``pos`` (B, W, P), ``lnp`` (B, W), ``order`` (steps, B, W), ``zz`` / ``thr`` / ``pick``
        (steps, 2, B, W/2), ``chain`` (steps, B, W, P), ``lnprob_chain`` (steps, B, W), ``accepted`` (B, W): B independent
        ensembles in lockstep, one per radial bin, as ``analysis.binned.BinnedSampler`` draws them."""
        head, tail, _keep = self._stretch_args("stretch_move", plan, pos, lnp, order.shape[0], chain, lnprob_chain, accepted)
        for a, dt in ((zz, np.float64), (thr, np.float64), (order, np.int32), (pick, np.int32)):
            if a.dtype != dt or not a.flags.c_contiguous:
                raise ValueError("stretch_move needs C-contiguous arrays of the documented dtypes")
        half_shape = (order.shape[0], 2) + pos.shape[:-2] + (pos.shape[-2] // 2,)
        if order.shape != order.shape[:1] + lnp.shape or zz.shape != half_shape or thr.shape != half_shape or \
                pick.shape != half_shape:
            raise ValueError("stretch_move: inconsistent array shapes")
        numbers = (order.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), _ptr(zz), _ptr(thr),
                   pick.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        if self._prior_arg is not None:
            rc = self.lib.mcd_stretch_move_prior(*head, *numbers, *tail, *self._prior_arg)
        else:
            rc = self.lib.mcd_stretch_move(*head, *numbers, *tail)
        _check(self.lib, rc, "mcd_stretch_move")
        self._walkers = pos.shape[-2] // 2

    def stretch_move_seeded(self, plan, pos, lnp, seed, step0, n_steps, chain=None, lnprob_chain=None, accepted=None):
        """``mcd_stretch_move_seeded``: the same block with its random numbers generated inside the library from the
        counter-based generator of csrc/mcd_rng.h -- steps ``step0 .. step0 + n_steps - 1`` of the chain that ``seed`` names.
        ``chain_numbers(seed, step0, n_steps, ...)`` returns the numbers those steps use."""
        if n_steps < 0 or step0 < 0:
            raise ValueError("stretch_move_seeded: inconsistent array shapes")
        head, tail, _keep = self._stretch_args("stretch_move_seeded", plan, pos, lnp, n_steps, chain, lnprob_chain, accepted)
        if self._prior_arg is not None:
            rc = self.lib.mcd_stretch_move_seeded_prior(*head, int(seed) & 0xFFFFFFFFFFFFFFFF, int(step0), *tail, *self._prior_arg)
        else:
            rc = self.lib.mcd_stretch_move_seeded(*head, int(seed) & 0xFFFFFFFFFFFFFFFF, int(step0), *tail)
        _check(self.lib, rc, "mcd_stretch_move_seeded")
        self._walkers = pos.shape[-2] // 2

    def _de_prior(self, plan):
        """The ``prior`` argument of the DE entry points from a plan's optional ``prior`` entry (and what keeps it alive)."""
        if plan.get("prior") is None:
            return None, None
        pd, keep = _prior_desc(plan["prior"])
        return ctypes.byref(pd), (pd, keep)

    def de_move(self, plan, pos, lnp, order, pick_a, pick_b, gamma, thr, chain=None, lnprob_chain=None, accepted=None):
        """``mcd_de_move``: advance the ensemble(s) by ``len(order)`` differential-evolution steps (csrc/mcd_de.h) with the
        half-step loop inside the library.  ``plan``, ``pos``, ``lnp`` and the outputs as for ``stretch_move`` (a ``prior``
        entry of the plan is handed on); ``order`` (steps, [B,] W) int32, ``pick_a`` / ``pick_b`` int32 and ``gamma`` / ``thr``
        float64 (steps, 2, [B,] W/2), as ``de_numbers`` returns them."""
        head, tail, _keep = self._stretch_args("de_move", plan, pos, lnp, order.shape[0], chain, lnprob_chain, accepted)
        for a, dt in ((gamma, np.float64), (thr, np.float64), (order, np.int32), (pick_a, np.int32), (pick_b, np.int32)):
            if a.dtype != dt or not a.flags.c_contiguous:
                raise ValueError("de_move needs C-contiguous arrays of the documented dtypes")
        half_shape = (order.shape[0], 2) + pos.shape[:-2] + (pos.shape[-2] // 2,)
        if order.shape != order.shape[:1] + lnp.shape or any(a.shape != half_shape for a in (pick_a, pick_b, gamma, thr)):
            raise ValueError("de_move: inconsistent array shapes")
        prior, _keep_prior = self._de_prior(plan)
        i32 = ctypes.POINTER(ctypes.c_int32)
        rc = self.lib.mcd_de_move(head[0], head[1], prior, *head[2:], order.ctypes.data_as(i32), pick_a.ctypes.data_as(i32),
                                  pick_b.ctypes.data_as(i32), _ptr(gamma), _ptr(thr), *tail)
        _check(self.lib, rc, "mcd_de_move")
        self._walkers = pos.shape[-2] // 2

    def de_move_seeded(self, plan, pos, lnp, gamma0, sigma, seed, step0, n_steps, chain=None, lnprob_chain=None, accepted=None):
        """``mcd_de_move_seeded``: the same block with its random numbers generated inside the library -- steps ``step0 ..
        step0 + n_steps - 1`` of the chain that ``seed`` names; ``de_numbers(seed, step0, n_steps, ...)`` returns them."""
        if n_steps < 0 or step0 < 0:
            raise ValueError("de_move_seeded: inconsistent array shapes")
        head, tail, _keep = self._stretch_args("de_move_seeded", plan, pos, lnp, n_steps, chain, lnprob_chain, accepted)
        prior, _keep_prior = self._de_prior(plan)
        rc = self.lib.mcd_de_move_seeded(head[0], head[1], prior, float(gamma0), float(sigma), *head[2:],
                                         int(seed) & 0xFFFFFFFFFFFFFFFF, int(step0), *tail)
        _check(self.lib, rc, "mcd_de_move_seeded")
        self._walkers = pos.shape[-2] // 2

    def de_info(self):
        """Where the blocks of ``de_move`` / ``de_move_seeded`` ran: {'device_blocks', 'host_blocks', 'discarded_blocks',
        'last_discard_status'} (``mcd_de_info``; ``stretch_info`` keeps counting stretch blocks only)."""
        a, b, c, st = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int32(0)
        _check(self.lib, self.lib.mcd_de_info(self.handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(st)),
               "mcd_de_info")
        return {"device_blocks": a.value, "host_blocks": b.value, "discarded_blocks": c.value, "last_discard_status": st.value}

    @property
    def last_prefetch(self):
        """1 / 0: the last main-kernel launch used / did not use the record-prefetching instantiation; -1 before any launch."""
        return self.lib.mcd_last_prefetch(self.handle)

    @property
    def last_narrow_bounded(self):
        """R (16 or 32): the last main-kernel launch ran the bounded narrow-range BGFIXED loop with a rescale every R
        factors (option ``narrow_bounded``); 0 another loop; -1 before any launch."""
        return self.lib.mcd_last_narrow_bounded(self.handle)

    @property
    def last_series_chunks(self):
        """Chunks of the last main-kernel launch in which every wave took the series reciprocal root (options
        ``verr_sorted``, ``root_series``; counted on the host); 0 none; -1 before any launch."""
        return self.lib.mcd_last_series_chunks(self.handle)

    @property
    def last_direct_chunks(self):
        """... of which chunks in which every wave took the direct form of the series (option ``root_direct``; counted on
        the host); 0 none; -1 before any launch."""
        return self.lib.mcd_last_direct_chunks(self.handle)

    @property
    def last_exp_split(self):
        """1: the direct chunks of the last main-kernel launch ran with the split exponent offset (option ``exp_split``);
        0 not; -1 before any launch."""
        return self.lib.mcd_last_exp_split(self.handle)

    @property
    def last_root_quad(self):
        """1: the last main-kernel launch offered its direct chunks the quadratic series root on 32-star bands (option
        ``root_quad`` on a launch with the split exponent offset); 0 not; -1 before any launch."""
        return self.lib.mcd_last_root_quad(self.handle)

    @property
    def last_quad_chunks(self):
        """... and the chunks in which every wave took it (counted on the host; never more than ``last_direct_chunks``);
        0 none; -1 before any launch."""
        return self.lib.mcd_last_quad_chunks(self.handle)

    @property
    def last_block_step(self):
        """1: the last main-kernel launch ran the bounded kernel whose quadratic loop takes one block step per 32-star band
        (option ``block_step`` on a bounded launch with R = 32 that offers the quadratic form, where 56 raw factors fit
        between two rescales); 0 not; -1 before any launch."""
        return self.lib.mcd_last_block_step(self.handle)

    def hmc_block(self, plan, chol, step_size, n_leap, pos, lnp, seed, step0, n_steps, chain=None, lnprob_chain=None,
                  accepted=None, energy_error=None, jitter=0.1):
        """``mcd_hmc_block``: advance W independent chains by ``n_steps`` Hamiltonian Monte Carlo steps of ``n_leap``
        leapfrog points on the device gradient.  ``plan`` as for ``stretch_move``; ``chol`` (P, P): lower Cholesky factor
        of the inverse mass matrix (a posterior covariance estimate).  ``pos`` (W, P) is updated in place, ``lnp`` (W,) is
        written; ``chain`` (steps, W, P), ``lnprob_chain`` (steps, W), ``energy_error`` (steps, W) and ``accepted`` (W,)
        int64 (incremented) are optional.  Steps ``step0 .. step0 + n_steps - 1`` of the chain that ``seed`` names."""
        if n_steps < 0 or step0 < 0 or pos.ndim != 2:
            raise ValueError("hmc_block: inconsistent array shapes")
        head, tail, _keep = self._stretch_args("hmc_block", plan, pos, lnp, n_steps, chain, lnprob_chain, accepted)
        chol = np.ascontiguousarray(chol, dtype=np.float64)
        if chol.shape != (pos.shape[1], pos.shape[1]):
            raise ValueError("hmc_block: chol must have shape (P, P)")
        if energy_error is not None and (energy_error.dtype != np.float64 or not energy_error.flags.c_contiguous or
                                         energy_error.shape != (n_steps, pos.shape[0])):
            raise ValueError("hmc_block: energy_error must be a C-contiguous float64 array of shape (steps, W)")
        d = HmcDesc()
        d.map = head[1]._obj
        d.chol, d.step_size, d.jitter, d.n_leap = _ptr(chol), float(step_size), float(jitter), int(n_leap)
        if self._prior_arg is not None:
            rc = self.lib.mcd_hmc_block_prior(self.handle, ctypes.byref(d), int(n_steps), head[3], head[4],
                                              int(seed) & 0xFFFFFFFFFFFFFFFF, int(step0), *tail, _ptr(energy_error),
                                              *self._prior_arg)
        else:
            rc = self.lib.mcd_hmc_block(self.handle, ctypes.byref(d), int(n_steps), head[3], head[4],
                                        int(seed) & 0xFFFFFFFFFFFFFFFF, int(step0), *tail, _ptr(energy_error))
        _check(self.lib, rc, "mcd_hmc_block")

    def hmc_info(self):
        """Where the blocks of ``hmc_block`` ran: {'device_blocks', 'host_blocks'} (``mcd_hmc_info``)."""
        a, b = ctypes.c_int64(), ctypes.c_int64()
        _check(self.lib, self.lib.mcd_hmc_info(self.handle, ctypes.byref(a), ctypes.byref(b)), "mcd_hmc_info")
        return {"device_blocks": a.value, "host_blocks": b.value}

    def temper_block(self, plan, betas, pos, lnlike, lnprior, seed, step0, n_steps, chain=None, lnlike_chain=None,
                     accepted=None, swap_proposed=None, swap_accepted=None):
        """``mcd_temper_block``: advance T ensembles of W walkers, one per inverse temperature of ``betas`` (T,), by
        ``n_steps`` parallel-tempering steps (csrc/mcd_temper.h).  ``plan`` as for ``stretch_move`` (a ``prior`` entry selects
        ``mcd_temper_block_prior``).  ``pos`` (T, W, P) and ``lnlike`` (T, W) are updated in place, ``lnprior`` (T, W) is
        written; ``chain`` (steps, C, W, P) stores the positions of rungs 0 .. C - 1, ``lnlike_chain`` (steps, T, W) the
        log-likelihood of every rung; ``accepted`` (T, W), ``swap_proposed`` and ``swap_accepted`` (T - 1,) int64 are
        incremented.  Steps ``step0 .. step0 + n_steps - 1`` of the chain that ``seed`` names."""
        if n_steps < 0 or step0 < 0 or pos.ndim != 3 or lnlike.shape != pos.shape[:2] or lnprior.shape != pos.shape[:2]:
            raise ValueError("temper_block: inconsistent array shapes")
        t, w, p = pos.shape
        betas = _f64(betas)
        if betas.shape != (t,):
            raise ValueError("temper_block: betas must have one entry per rung")
        if lnprior.dtype != np.float64 or not lnprior.flags.c_contiguous or not pos.flags.c_contiguous or \
                not lnlike.flags.c_contiguous:
            raise ValueError("temper_block needs C-contiguous arrays of the documented dtypes")
        head, _tail, _keep = self._stretch_args("temper_block", plan, pos[0], lnlike[0], n_steps, None, None, None)
        n_chain = 1
        if chain is not None:
            if chain.dtype != np.float64 or not chain.flags.c_contiguous or chain.ndim != 4 or \
                    chain.shape[0] != n_steps or chain.shape[2:] != (w, p):
                raise ValueError("temper_block: chain must be a C-contiguous float64 array of shape (steps, C, W, P)")
            n_chain = chain.shape[1]
        if lnlike_chain is not None and (lnlike_chain.dtype != np.float64 or not lnlike_chain.flags.c_contiguous or
                                         lnlike_chain.shape != (n_steps, t, w)):
            raise ValueError("temper_block: lnlike_chain must be a C-contiguous float64 array of shape (steps, T, W)")
        for a, shape in ((accepted, (t, w)), (swap_proposed, (t - 1,)), (swap_accepted, (t - 1,))):
            if a is not None and (a.dtype != np.int64 or a.shape != shape or not a.flags.c_contiguous):
                raise ValueError("temper_block: accepted (T, W) and the swap counts (T - 1,) are C-contiguous int64 arrays")
        d = TemperDesc()
        d.map = head[1]._obj
        d.n_temps, d.betas, d.n_chain_temps = t, _ptr(betas), n_chain

        def ip(a):
            return a.ctypes.data_as(_c_int64_p) if a is not None else None
        args = (self.handle, ctypes.byref(d), int(n_steps), _ptr(pos), _ptr(lnlike), _ptr(lnprior),
                int(seed) & 0xFFFFFFFFFFFFFFFF, int(step0), _ptr(chain), _ptr(lnlike_chain), ip(accepted), ip(swap_proposed),
                ip(swap_accepted))
        if self._prior_arg is not None:
            rc = self.lib.mcd_temper_block_prior(*args, *self._prior_arg)
        else:
            rc = self.lib.mcd_temper_block(*args)
        _check(self.lib, rc, "mcd_temper_block")
        self._walkers = t * (w // 2)

    def temper_info(self):
        """Where the blocks of ``temper_block`` ran: {'device_blocks', 'host_blocks'} (``mcd_temper_info``)."""
        a, b = ctypes.c_int64(), ctypes.c_int64()
        _check(self.lib, self.lib.mcd_temper_info(self.handle, ctypes.byref(a), ctypes.byref(b)), "mcd_temper_info")
        return {"device_blocks": a.value, "host_blocks": b.value}

    def stretch_info(self):
        """Where the blocks of ``stretch_move`` ran: {'device_blocks', 'host_blocks', 'discarded_blocks', 'last_discard_status'}
        (``mcd_stretch_info``: resident on the device / host-driven / discarded by the device and re-run host-driven)."""
        a, b, c, st = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int32()
        _check(self.lib, self.lib.mcd_stretch_info(self.handle, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(st)),
               "mcd_stretch_info")
        return {"device_blocks": a.value, "host_blocks": b.value, "discarded_blocks": c.value, "last_discard_status": st.value}

    def set_option(self, key, value):
        _check(self.lib, self.lib.mcd_set_option(self.handle, key.encode(), int(value)), "mcd_set_option")
        self.__dict__.setdefault("_options", {})[key] = int(value)

    def get_option(self, key, default=None):
        """The value ``set_option`` last gave option ``key`` through this object, else ``default`` (the library has no
        query: a caller that changes an option for one evaluation restores what it found with this)."""
        return self.__dict__.get("_options", {}).get(key, default)

    @property
    def last_kernel_ms(self):
        return self.lib.mcd_last_kernel_ms(self.handle)

    @property
    def last_device_ms(self):
        return self.lib.mcd_last_device_ms(self.handle)

    def timing_collect(self):
        """(summed main-kernel milliseconds, number of launches) since the last collect ("timing" = 2)."""
        total, n = ctypes.c_double(), ctypes.c_int64()
        _check(self.lib, self.lib.mcd_timing_collect(self.handle, ctypes.byref(total), ctypes.byref(n)),
               "mcd_timing_collect")
        return total.value, n.value

    @property
    def rerun_count(self):
        """Batches re-evaluated with the plain kernels (denormal regime of the reference's log-sum-exp)."""
        return self.lib.mcd_rerun_count(self.handle)

    @property
    def fast_level(self):
        """Kernel family of the batch staged last: 0 plain, 1 fast, 2 narrow-range fixed-background variant."""
        return self.lib.mcd_last_fast_level(self.handle)

    @property
    def f32_in_domain(self):
        """Was the table staged last inside the float32 accuracy domain (include/mcd.h)?  Always True for float64."""
        return bool(self.lib.mcd_last_f32_domain(self.handle, None, None))

    @property
    def f32_condition(self):
        """(kappa_v, kappa_theta) of the table staged last: the two condition numbers the float32 domain bounds."""
        kv, kt = ctypes.c_double(), ctypes.c_double()
        self.lib.mcd_last_f32_domain(self.handle, ctypes.byref(kv), ctypes.byref(kt))
        return kv.value, kt.value

    def f32_outside(self):
        """The float32 domain verdict over every table staged since the catalogue was created (``mcd_f32_outside``; a
        library block stages two per step): {'calls': tables outside the domain, 'worst_kappa_v', 'worst_kappa_theta': the
        largest condition numbers of any staged table, 'reason': of the last table outside, '' without one}."""
        self._alive()
        calls, kv, kt, why = ctypes.c_int64(), ctypes.c_double(), ctypes.c_double(), ctypes.c_char_p()
        _check(self.lib, self.lib.mcd_f32_outside(self.handle, ctypes.byref(calls), ctypes.byref(kv), ctypes.byref(kt),
                                                  ctypes.byref(why)), "mcd_f32_outside")
        return {"calls": calls.value, "worst_kappa_v": kv.value, "worst_kappa_theta": kt.value,
                "reason": (why.value or b"").decode()}

    def launch_info(self):
        wg, ch = ctypes.c_int64(), ctypes.c_int64()
        tile, rb = ctypes.c_int32(), ctypes.c_int32()
        _check(self.lib, self.lib.mcd_last_launch_info(self.handle, ctypes.byref(wg), ctypes.byref(tile),
                                                       ctypes.byref(ch), ctypes.byref(rb)), "mcd_last_launch_info")
        return {"workgroups": wg.value, "walker_tile": tile.value, "chunks": ch.value, "record_bytes": rb.value,
                "series_chunks": self.last_series_chunks, "direct_chunks": self.last_direct_chunks,
                "exp_split": self.last_exp_split, "root_quad": self.last_root_quad, "quad_chunks": self.last_quad_chunks,
                "block_step": self.last_block_step}

    def close(self):
        if getattr(self, "handle", None):
            self.lib.mcd_catalog_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

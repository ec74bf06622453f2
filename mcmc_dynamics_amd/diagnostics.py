"""Convergence diagnostics of a stored chain: the integrated autocorrelation time, the effective sample size and
split-R-hat, computed by ``mcd_chain_diagnostics`` (include/mcd.h; csrc/mcd_diag.h) -- on the device beside the sampler
that produced the chain, or by the library's host loop when ``context=None``; both give the same bits.

The estimator is emcee's ``autocorr.integrated_time`` (Goodman & Weare 2010; Sokal's automatic window): per walker the
normalised autocorrelation function, averaged over the walkers, summed up to the smallest lag ``M`` with ``M >= c tau(M)``.
One difference in how it is evaluated: the lags are taken up to ``max_lag`` (default ``T // 10``) instead of all ``T`` of
them.  An estimate emcee would trust (``T >= tol tau`` with ``tol = 50``) has its window near ``c tau <= T / 10``, and an
estimate whose window lies below ``max_lag`` is the all-lags estimate exactly; where no window exists up to ``max_lag`` the
chain is too short and the call says so (``AutocorrError``), as emcee does.

Chains are steps-first, as ``sampler.get_chain()`` returns them: ``(T, W, P)``, or ``(T, G, W, P)`` for ``G`` independent
ensembles (``BinnedSampler``)."""
import warnings

import numpy as np

from . import _native

DEFAULT_CONTEXT = "default"          # the ``context`` argument: the process-wide device context (``None``: host loop)


class AutocorrError(Exception):
    """The chain is too short for a reliable autocorrelation time; ``tau`` holds the estimate (as emcee's AutocorrError)."""

    def __init__(self, tau, *args, **kwargs):
        self.tau = tau
        super(AutocorrError, self).__init__(*args, **kwargs)


def _as_groups(chain):
    chain = np.asarray(chain, dtype=np.float64)
    if chain.ndim == 3:
        return chain[:, None], True
    if chain.ndim == 4:
        return chain, False
    raise ValueError("a chain is steps-first: (steps, walkers, parameters) or (steps, ensembles, walkers, parameters)")


def _context(context):
    return _native.default_context() if isinstance(context, str) and context == DEFAULT_CONTEXT else context


def _raw(chain, c, max_lag, context, scratch_mb=0):
    chain, squeeze = _as_groups(chain)
    T = chain.shape[0]
    if T < 2:
        raise ValueError("a chain of {0} step(s) has no autocorrelation".format(T))
    L = max(1, T // 10) if max_lag is None else int(max_lag)
    out = _native.chain_diagnostics(chain, L, c=c, context=_context(context), scratch_mb=scratch_mb)
    out["n_steps"], out["n_walkers"] = T, chain.shape[2]
    return out, squeeze


def _too_short(out, tol):
    """(G, P) bool: no window up to max_lag, or fewer than tol autocorrelation times of steps."""
    flag = out["found"] == 0
    if tol > 0:
        with np.errstate(invalid="ignore"):
            flag = flag | (tol * out["tau"] > out["n_steps"])
    return flag


def integrated_time(chain, c=5.0, tol=50.0, max_lag=None, quiet=False, context=DEFAULT_CONTEXT, scratch_mb=0):
    """The integrated autocorrelation time per parameter, ``(P,)`` or ``(G, P)``, in steps.  Raises ``AutocorrError``
    (carrying ``.tau``) when no window exists up to ``max_lag`` or the chain is shorter than ``tol`` autocorrelation times;
    ``quiet=True`` warns instead and returns the estimate; ``tol=0`` switches the length test off."""
    out, squeeze = _raw(chain, c, max_lag, context, scratch_mb)
    tau = out["tau"][0] if squeeze else out["tau"]
    short = _too_short(out, tol)
    if short.any():
        no_window = int((out["found"] == 0).sum())
        msg = ("The chain is too short for a reliable integrated autocorrelation time for {0} parameter(s) ({1} without a "
               "window up to max_lag, the others shorter than tol = {2} times tau). Use this estimate with caution and run a "
               "longer chain!\nN = {3};\ntau: {4}").format(int(short.sum()), no_window, tol, out["n_steps"], tau)
        if not quiet:
            raise AutocorrError(tau, msg)
        warnings.warn(msg)
    return tau


def summary(chain, c=5.0, tol=50.0, max_lag=None, context=DEFAULT_CONTEXT, scratch_mb=0):
    """Everything ``mcd_chain_diagnostics`` returns, per parameter ((P,) or (G, P) arrays): ``tau``, ``window``, ``found``,
    ``converged`` (a window was found and the chain holds ``tol`` autocorrelation times), ``ess`` = W T / tau, ``rhat``
    (split-R-hat over the 2 W half-chains), ``mean``, ``std`` (pooled), and ``n_steps``."""
    out, squeeze = _raw(chain, c, max_lag, context, scratch_mb)
    with np.errstate(invalid="ignore", divide="ignore"):
        res = {"tau": out["tau"], "window": out["window"], "found": out["found"].astype(bool),
               "converged": ~_too_short(out, tol), "ess": out["n_walkers"] * out["n_steps"] / out["tau"],
               "rhat": out["rhat"], "mean": out["mean"], "std": np.sqrt(out["var"])}
    if squeeze:
        res = {k: v[0] for k, v in res.items()}
    res["n_steps"] = out["n_steps"]
    return res


def sampler_autocorr_time(sampler, discard=0, thin=1, **kwargs):
    """What the samplers' ``get_autocorr_time`` runs: ``integrated_time`` of ``get_chain(discard)`` thinned by ``thin``,
    times ``thin`` (as emcee)."""
    thin = int(thin)
    if thin < 1:
        raise ValueError("thin must be >= 1")
    chain = sampler.get_chain(discard=int(discard))
    return thin * integrated_time(chain[::thin], **kwargs)

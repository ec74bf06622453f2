"""``Runner``: posterior API and MCMC driver, GPU-backed.

Mirror of the reference's ``mcmc_dynamics/analysis/runner.py`` for the hot path: the method names,
arguments and error behaviour of ``lnprior`` / ``lnlike`` / ``lnprob`` / ``fetch_parameter_values`` /
``get_initials`` / ``__call__`` are kept (runner.py:143-443) so that emcee drives the outer loop
unchanged, and a batched entry ``lnprob_batch((W, P)) -> (W,)`` is added, which is what the sampler
is handed (``vectorize=True``).  The per-star arithmetic of ``_calculate_lnlike`` (runner.py:240-286)
does not exist on the host: it runs in ``libmcd_hip.so`` on the star catalogue pinned in HBM.

Differences that follow from dropping astropy: values are plain floats in the unit recorded in each
``Parameter`` (the reference returns ``Quantity`` objects); ``lnprob`` returns a Python float.
"""
import logging
import pickle
import warnings
from collections import OrderedDict

import numpy as np

from .. import _native, units
from ..background import Gaussian, SingleStars
from ..parameter import Parameters
from ..utils.coordinates import calc_xy_offset
from ..utils.data_reader import DataReader
from ..utils.results import ResultsTable

logger = logging.getLogger(__name__)


class _BatchPlan(object):
    """Everything `lnprob_batch` needs from `self.parameters`, flattened into index arrays once per
    parameter configuration: the per-call host work is then a handful of NumPy operations on a (W, n_all)
    array instead of a Python loop over parameters (the reference spends ~0.1 ms per walker here,
    SURVEY.md section 8(a) A2/A3)."""

    def __init__(self, runner):
        pars = runner.parameters
        self.names = list(pars)
        index = {n: i for i, n in enumerate(self.names)}
        self.n_all = len(self.names)
        self.free_idx = np.array([i for i, p in enumerate(pars.values()) if not p.fixed], dtype=np.intp)
        fixed = [(i, p) for i, p in enumerate(pars.values()) if p.fixed and p._expr is None]
        self.fixed_idx = np.array([i for i, _ in fixed], dtype=np.intp)
        self.fixed_val = np.array([float(p._value) for _, p in fixed], dtype=np.float64)
        self.simple = all(p._expr is None and p._lnprior is None for p in pars.values())
        # structured priors (Parameter.prior) over the FREE parameters: (kind, p0, p1) arrays, or None.  They do not end
        # `simple`: the library evaluates them, on the device inside resident blocks (csrc/mcd_prior.h).
        self.prior = pars.structured_prior()
        self.lo, self.hi = pars.bounds()
        self.unbounded = bool(np.all(np.isneginf(self.lo)) and np.all(np.isposinf(self.hi)))
        # kernel table columns (C-ABI order) and unit factors
        key, _ = runner._catalog_spec()
        cols = list(runner._KERNEL_HEAD)
        if key[1] is None:
            cols += [("ra_center", "deg"), ("dec_center", "deg")]
        cols += list(runner._KERNEL_TAIL)
        self.kernel_idx = np.array([index[n] for n, _ in cols], dtype=np.intp)
        fac = [units.conversion_factor(pars[n].unit, u) if (pars[n].unit and u) else 1.0 for n, u in cols]
        self.kernel_fac = None if all(f == 1.0 for f in fac) else np.array(fac, dtype=np.float64)
        self.catalog_key = key
        # Direct route for the common case (every kernel column is a FREE parameter, flat bounds): the (W, P) proposal array
        # is checked and handed to the kernel without building the (W, n_all) table first.  The fixed parameters are
        # constants: their bounds are verified here once (the reference re-checks them per call, runner.py:207-214).
        free_pos = {int(i): pos for pos, i in enumerate(self.free_idx)}
        self.direct_cols = None
        if self.simple and all(int(i) in free_pos for i in self.kernel_idx):
            cols_ = np.array([free_pos[int(i)] for i in self.kernel_idx], dtype=np.intp)
            self.direct_cols = cols_
            self.direct_identity = bool(cols_.size == self.free_idx.size and np.array_equal(cols_, np.arange(cols_.size)))
            self.fixed_ok = bool(np.all((self.fixed_val >= self.lo[self.fixed_idx]) & (self.fixed_val <= self.hi[self.fixed_idx]))) \
                if self.fixed_idx.size else True
            free_lo, free_hi = self.lo[self.free_idx], self.hi[self.free_idx]
            self.lo_cols = np.flatnonzero(~np.isneginf(free_lo))
            self.hi_cols = np.flatnonzero(~np.isposinf(free_hi))
            self.lo_vals, self.hi_vals = free_lo[self.lo_cols], free_hi[self.hi_cols]

    @staticmethod
    def signature(runner):
        return tuple((p.fixed, p._value if p.fixed else None, p.min, p.max, p._expr, p._lnprior, p.unit, p._prior)
                     for p in runner.parameters.values())

    def prior_free(self, values, ok):
        """Structured priors of the (W, P) free-parameter rows: (log-prior (W,), `ok` without the rows whose prior is -inf
        -- a log-normal coordinate <= 0), by one ``mcd_prior_eval`` call; (None, ok) without structured priors."""
        if self.prior is None:
            return None, ok
        lp = _native.prior_eval(self.prior, values)
        return lp, ok & (lp > -np.inf)

    def full(self, values):
        out = np.empty((values.shape[0], self.n_all), dtype=np.float64)
        out[:, self.free_idx] = values
        if self.fixed_idx.size:
            out[:, self.fixed_idx] = self.fixed_val
        return out

    def prior_ok(self, full):
        """Boolean (W,): every parameter inside its inclusive bounds (NaN counts as outside)."""
        if self.unbounded:
            return ~np.isnan(full).any(axis=1)
        return ((full >= self.lo) & (full <= self.hi)).all(axis=1)

    def table(self, full):
        t = full[:, self.kernel_idx]
        return t if self.kernel_fac is None else t * self.kernel_fac

    def prior_ok_free(self, values):
        """`prior_ok` from the (W, P) proposals alone (direct route)."""
        if not self.fixed_ok:
            return np.zeros(values.shape[0], dtype=bool)
        ok = ~np.isnan(values).any(axis=1)
        if self.lo_cols.size:
            ok &= (values[:, self.lo_cols] >= self.lo_vals).all(axis=1)
        if self.hi_cols.size:
            ok &= (values[:, self.hi_cols] <= self.hi_vals).all(axis=1)
        return ok

    def table_direct(self, values):
        t = values if self.direct_identity else values[:, self.direct_cols]
        return t if self.kernel_fac is None else t * self.kernel_fac


# Vehtari, Gelman & Gabry (2017): WAIC's estimate is unreliable when the posterior variance of a star's lnL exceeds 0.4
WAIC_VAR_WARNING = 0.4


def waic_summary(lppd, lnl_var, n_samples, group=None):
    """WAIC from the per-star arrays of ``Runner.pointwise_posterior`` (Watanabe; Gelman, Hwang & Vehtari 2014):
    elpd_i = lppd_i - Var_s(lnL_is), elpd_waic = sum_i elpd_i, p_waic = sum_i Var_s(lnL_is), waic = -2 elpd_waic,
    se = sqrt(N Var_i(elpd_i)) (sample variance over the N stars).  ``group``: the host group of a multi-rank job, whose
    ranks hold disjoint stars -- the totals (sums of lppd, p_waic, elpd, elpd^2, N and the warning count) are summed over
    it, so every rank returns the same scalars; ``pointwise`` stays this rank's stars."""
    lppd = np.asarray(lppd, dtype=np.float64)
    var = np.asarray(lnl_var, dtype=np.float64)
    elpd = lppd - var
    totals = np.array([lppd.sum(), var.sum(), elpd.sum(), np.dot(elpd, elpd), float(elpd.size),
                       float(np.count_nonzero(var > WAIC_VAR_WARNING))])
    if group is not None:
        totals = np.asarray(group.allreduce(totals), dtype=np.float64)
    s_lppd, s_p, s_elpd, s_elpd2, n, n_warn = (float(t) for t in totals)
    var_i = (s_elpd2 - s_elpd * s_elpd / n) / (n - 1.0) if n > 1 else 0.0
    return {"elpd_waic": s_elpd, "p_waic": s_p, "waic": -2.0 * s_elpd, "se": float(np.sqrt(n * max(var_i, 0.0))),
            "lppd": s_lppd, "n_samples": int(n_samples), "n_stars": int(n), "n_high_variance": int(n_warn),
            "pointwise": elpd}


def loo_k_threshold(n_samples):
    """The Pareto k^ above which a star's PSIS-LOO estimate is unreliable: min(1 - 1/log10(S), 0.7) (Vehtari et al. 2024)."""
    return min(1.0 - 1.0 / np.log10(float(n_samples)), 0.7) if n_samples > 1 else -np.inf


def loo_summary(elpd_loo, lppd, pareto_k, n_samples, group=None):
    """PSIS-LOO totals from the per-star arrays of ``Catalog.psis_loo``: elpd_loo = sum_i elpd_loo_i, p_loo = sum_i (lppd_i -
    elpd_loo_i), looic = -2 elpd_loo, se = sqrt(N Var_i(elpd_loo_i)), and the count of stars whose k^ exceeds
    ``loo_k_threshold(S)`` (k^ = +inf, a tail too short to fit, counts).  ``group``: the host group of a multi-rank job
    (ranks hold disjoint stars) -- the totals are summed over it, so every rank returns the same scalars; ``pointwise``
    and ``pareto_k`` stay this rank's stars."""
    elpd = np.asarray(elpd_loo, dtype=np.float64)
    lppd = np.asarray(lppd, dtype=np.float64)
    k = np.asarray(pareto_k, dtype=np.float64)
    thr = loo_k_threshold(n_samples)
    totals = np.array([lppd.sum(), elpd.sum(), np.dot(elpd, elpd), float(elpd.size), float(np.count_nonzero(k > thr))])
    if group is not None:
        totals = np.asarray(group.allreduce(totals), dtype=np.float64)
    s_lppd, s_elpd, s_elpd2, n, n_bad = (float(t) for t in totals)
    var_i = (s_elpd2 - s_elpd * s_elpd / n) / (n - 1.0) if n > 1 else 0.0
    return {"elpd_loo": s_elpd, "p_loo": s_lppd - s_elpd, "looic": -2.0 * s_elpd,
            "se": float(np.sqrt(n * max(var_i, 0.0))), "lppd": s_lppd, "n_samples": int(n_samples), "n_stars": int(n),
            "k_threshold": float(thr), "n_bad_k": int(n_bad), "pareto_k": k, "pointwise": elpd}


def _elpd_totals(elpd, group=None):
    """(sum, se, N) of per-star elpd values by the arithmetic of ``loo_summary``: se = sqrt(N Var_i(elpd_i))."""
    elpd = np.asarray(elpd, dtype=np.float64)
    totals = np.array([elpd.sum(), np.dot(elpd, elpd), float(elpd.size)])
    if group is not None:
        totals = np.asarray(group.allreduce(totals), dtype=np.float64)
    s_elpd, s_elpd2, n = (float(t) for t in totals)
    var_i = (s_elpd2 - s_elpd * s_elpd / n) / (n - 1.0) if n > 1 else 0.0
    return s_elpd, float(np.sqrt(n * max(var_i, 0.0))), int(n)


def kfold_summary(pointwise, folds=None):
    """K-fold cross-validation totals from the per-star predictive densities of ``Runner.kfold`` (each star under the
    refit that left its fold out; Vehtari, Gelman & Gabry 2017, section 2.4): ``elpd_kfold`` = sum_i elpd_i, ``se`` =
    sqrt(N Var_i(elpd_i)) as in ``loo_summary``, ``pointwise``, ``n_stars``, ``n_folds`` and ``folds`` (the fold id per
    star, or None).  A higher ``elpd_kfold`` is the better model for the same stars; ``elpd_compare`` takes the result."""
    elpd = np.asarray(pointwise, dtype=np.float64)
    if elpd.ndim != 1 or not np.all(np.isfinite(elpd)):
        raise ValueError("pointwise must hold one finite value per star (every star in exactly one fold)")
    if folds is not None:
        folds = np.asarray(folds, dtype=np.int64)
        if folds.shape != elpd.shape:
            raise ValueError("folds must hold one fold id per star")
    s_elpd, se, n = _elpd_totals(elpd)
    return {"elpd_kfold": s_elpd, "se": se, "pointwise": elpd, "n_stars": n,
            "n_folds": int(np.unique(folds).size) if folds is not None else None, "folds": folds}


def elpd_compare(a, b, group=None):
    """Difference of two models' expected log predictive densities on the same stars: ``a``, ``b`` are ``waic()`` or
    ``loo()`` results.  elpd_diff = sum_i (a_i - b_i) (positive: ``a`` predicts better), se_diff = sqrt(N Var_i(a_i - b_i)),
    the paired standard error (not the difference or the quadrature sum of the two ``se``).  ``group``: as in
    ``loo_summary`` (each rank passes its own stars' results)."""
    pa, pb = np.asarray(a["pointwise"], dtype=np.float64), np.asarray(b["pointwise"], dtype=np.float64)
    if pa.shape != pb.shape:
        raise ValueError("the two results hold different stars ({0} and {1} pointwise values)".format(pa.size, pb.size))
    d = pa - pb
    totals = np.array([d.sum(), np.dot(d, d), float(d.size)])
    if group is not None:
        totals = np.asarray(group.allreduce(totals), dtype=np.float64)
    s_d, s_d2, n = (float(t) for t in totals)
    var_i = (s_d2 - s_d * s_d / n) / (n - 1.0) if n > 1 else 0.0
    return {"elpd_diff": s_d, "se_diff": float(np.sqrt(n * max(var_i, 0.0))), "n_stars": int(n), "pointwise": d}


# importance-sampling effective sample size of a stepping-stone pair below which ``evidence_summary`` warns
EVIDENCE_PAIR_ESS_WARNING = 100.0
EVIDENCE_BATCHES = 20              # batches of steps behind ``evidence_summary``'s ``se_batch``


def _series_tau(series):
    """Integrated autocorrelation time of a (W, steps) series in steps, >= 1 (``diagnostics.integrated_time`` on the
    library's host loop; the estimate carried by its AutocorrError when the chain is short; the number of steps -- one
    effective sample per walker -- when there is none)."""
    from .. import diagnostics
    chain = np.ascontiguousarray(np.swapaxes(series, 0, 1)[:, :, None])
    n = chain.shape[0]
    if n < 2 or np.all(chain == chain[0]):
        return float(max(n, 1))
    try:
        tau = diagnostics.integrated_time(chain, context=None)
    except diagnostics.AutocorrError as exc:
        tau = exc.tau
    tau = float(np.asarray(tau).reshape(-1)[0])
    return min(max(tau, 1.0), float(n)) if np.isfinite(tau) else float(n)


def evidence_summary(lnlike, betas, discard=0):
    """Log marginal likelihood from a tempered run: ``lnlike`` (T, W, steps), the log-likelihood series of the rungs
    (``TemperedSampler.lnlikelihood``), ``betas`` (T,) with ``betas[0] == 1`` and ``betas[-1] == 0`` (ValueError
    otherwise), the first ``discard`` steps left out.

    ``log_evidence``: the STEPPING-STONE estimator (Xie et al. 2011), sum over the pairs k of
    ``pair_log_ratio[k]`` = log mean over rung k + 1's samples of exp((beta_k - beta_{k+1}) lnL), each by log-mean-exp.
    It has no discretisation bias.  ``se``: per pair the delta-method variance Var(w) / (mean(w)^2 n_eff) over
    n_eff = n / tau effective samples, tau the integrated autocorrelation time of that rung's lnL series
    (``diagnostics.integrated_time``; its ``.tau`` when it raises for a short chain); the pair variances are summed
    (``pair_se``).  The correlation BETWEEN rungs that the swaps introduce is neglected, which makes ``se`` optimistic;
    ``se_batch`` is the cross-check that neglects nothing -- the standard error of the mean of the estimate on 20
    consecutive batches of steps (it needs batches much longer than tau).  ``pair_ess``: the
    importance-sampling effective sample size (sum w)^2 / sum w^2 of each pair; a value below 100 means the ladder is too
    coarse there, and the function warns.

    ``log_evidence_ti``: the thermodynamic integral, the trapezoid of the rungs' mean lnL over beta, with ``se_ti`` from
    the same effective sample sizes -- a cross-check that is BIASED by the ladder's spacing (the trapezoid's error), which
    ``se_ti`` does not contain.

    The estimate is relative to the prior as the library evaluates it: int L pi~ / int pi~, where pi~ is the box times the
    un-normalised truncated priors and the rung at beta = 0 samples pi~ / int pi~.  That IS the evidence under the
    normalised prior, whatever the box volume or the truncation: nothing like log(hi - lo) is to be added."""
    ll = np.asarray(lnlike, dtype=np.float64)
    betas = np.asarray(betas, dtype=np.float64).reshape(-1)
    if ll.ndim != 3 or ll.shape[0] != betas.size:
        raise ValueError("lnlike must have shape (T, W, steps) with one rung per beta")
    if betas.size < 2 or betas[0] != 1.0 or betas[-1] != 0.0 or np.any(np.diff(betas) >= 0.0):
        raise ValueError("the evidence needs a ladder that decreases strictly from beta = 1 to beta = 0")
    ll = ll[:, :, int(discard):]
    T, W, steps = ll.shape
    if steps < 2:
        raise ValueError("no steps left after discard")
    n = float(W * steps)
    tau = np.array([_series_tau(ll[t]) for t in range(T)])
    n_eff = n / tau
    ratio, var, ess = np.empty(T - 1), np.empty(T - 1), np.empty(T - 1)
    for k in range(T - 1):
        a = (betas[k] - betas[k + 1]) * ll[k + 1].reshape(-1)
        top = a.max()
        w = np.exp(a - top)
        mean = w.mean()
        ratio[k] = top + np.log(mean)
        var[k] = w.var(ddof=1) / (mean * mean * n_eff[k + 1])
        ess[k] = w.sum() ** 2 / np.dot(w, w)
    if np.any(ess < EVIDENCE_PAIR_ESS_WARNING):
        bad = ", ".join("{0:g} -> {1:g} (ESS {2:.0f})".format(betas[k + 1], betas[k], ess[k])
                        for k in np.flatnonzero(ess < EVIDENCE_PAIR_ESS_WARNING))
        warnings.warn("evidence_summary: the ladder is too coarse between beta " + bad + ": the stepping-stone ratio of such "
                      "a pair rests on a handful of samples; add rungs there")
    # cross-check of `se` that neglects nothing: the estimate on EVIDENCE_BATCHES consecutive batches of steps (all rungs and
    # walkers of a batch together, so the correlation between rungs and between walkers is in it), the standard error of
    # their mean.  Needs batches much longer than tau; NaN when there are fewer than two steps per batch.
    se_batch = float("nan")
    if steps >= 2 * EVIDENCE_BATCHES:
        edges = np.linspace(0, steps, EVIDENCE_BATCHES + 1).astype(int)
        per_batch = np.zeros(EVIDENCE_BATCHES)
        for k in range(T - 1):
            a = (betas[k] - betas[k + 1]) * ll[k + 1]
            top = a.max()
            w = np.exp(a - top)
            per_batch += [top + np.log(w[:, i0:i1].mean()) for i0, i1 in zip(edges[:-1], edges[1:])]
        se_batch = float(per_batch.std(ddof=1) / np.sqrt(EVIDENCE_BATCHES))
    means = ll.reshape(T, -1).mean(axis=1)
    var_mean = ll.reshape(T, -1).var(axis=1, ddof=1) / n_eff
    weight = np.zeros(T)
    weight[:-1] += 0.5 * (betas[:-1] - betas[1:])
    weight[1:] += 0.5 * (betas[:-1] - betas[1:])
    return {"log_evidence": float(ratio.sum()), "se": float(np.sqrt(var.sum())), "se_batch": se_batch, "pair_log_ratio": ratio,
            "pair_se": np.sqrt(var), "pair_ess": ess, "log_evidence_ti": float(np.dot(weight, means)),
            "se_ti": float(np.sqrt(np.dot(weight * weight, var_mean))), "mean_lnlike": means, "tau": tau,
            "betas": betas, "n_samples": int(n)}


def bayes_factor(a, b):
    """Log Bayes factor of two models from their ``evidence_summary`` results (``TemperedSampler.log_evidence``):
    ``log_bf`` = a - b (positive: the data favour ``a``), ``se`` = hypot of the two standard errors (independent runs)."""
    return {"log_bf": float(a["log_evidence"] - b["log_evidence"]), "se": float(np.hypot(a["se"], b["se"]))}


# the central interval of the PIT whose complement ``ppc_summary`` reports: 5 % of the weight for a calibrated model
PPC_TAIL = 0.025


def ppc_summary(pit, weights=None, n_bins=20, group=None):
    """Calibration of a fitted model from its stars' probability integral transforms (``Runner.posterior_predictive``:
    ``pit_mix``, or ``pit`` weighted by the membership probability): ``hist`` = weighted counts in ``n_bins`` equal PIT
    bins on [0, 1], ``n`` = the sum of the weights, ``chi2`` = sum_b (hist_b - n/B)^2 / (n/B) (for unit weights and a
    calibrated model approximately chi^2 with B - 1 degrees of freedom), ``tail_fraction`` = the share of the weight with
    a PIT outside [0.025, 0.975] (0.05 for a calibrated model), ``n_stars`` = the stars counted.  Stars whose PIT is not
    finite are left out.  ``group``: the host group of a multi-rank job, whose ranks hold disjoint stars -- every entry
    is additive over stars, so the totals are summed over it and every rank returns the same values."""
    pit = np.asarray(pit, dtype=np.float64)
    w = np.ones_like(pit) if weights is None else np.asarray(weights, dtype=np.float64)
    if w.shape != pit.shape:
        raise ValueError("weights must have the shape of pit")
    n_bins = int(n_bins)
    if n_bins < 1:
        raise ValueError("n_bins must be >= 1")
    ok = np.isfinite(pit) & np.isfinite(w)
    pit, w = pit[ok], w[ok]
    hist = np.histogram(pit, bins=n_bins, range=(0.0, 1.0), weights=w)[0]
    tail = w[(pit < PPC_TAIL) | (pit > 1.0 - PPC_TAIL)].sum()
    totals = np.concatenate([hist, [w.sum(), tail, float(pit.size)]])
    if group is not None:
        totals = np.asarray(group.allreduce(totals), dtype=np.float64)
    hist, n, tail, n_stars = totals[:n_bins], float(totals[n_bins]), float(totals[n_bins + 1]), int(totals[n_bins + 2])
    expect = n / n_bins
    chi2 = float(np.sum((hist - expect) ** 2) / expect) if n > 0 else 0.0
    return {"hist": hist, "n": n, "chi2": chi2, "tail_fraction": tail / n if n > 0 else 0.0, "n_stars": n_stars}


REPLICATE_NAMES = ("mean", "var_ratio", "skew", "kurt_excess", "rot_amp", "max_abs_z", "n_tail3")


def _replicate_discrepancies(f, n):
    """The discrepancies REPLICATE_NAMES (last axis) from the eight additive fields ``f`` (..., 8) of ``n`` stars (shape
    broadcastable against f[..., 0]); n == 0 gives NaN."""
    with np.errstate(divide="ignore", invalid="ignore"):
        n = np.where(np.asarray(n, dtype=np.float64) > 0, n, np.nan)
        m1, r2, r3, r4 = f[..., 0] / n, f[..., 1] / n, f[..., 2] / n, f[..., 3] / n
        c2 = r2 - m1 * m1
        c3 = r3 - 3.0 * m1 * r2 + 2.0 * m1 ** 3
        c4 = r4 - 4.0 * m1 * r3 + 6.0 * m1 * m1 * r2 - 3.0 * m1 ** 4
        rot = 2.0 * np.hypot(f[..., 4], f[..., 5]) / n
        return np.stack([m1, r2, c3 / c2 ** 1.5, c4 / (c2 * c2) - 3.0, rot, f[..., 6] + 0.0 * n, f[..., 7] + 0.0 * n], axis=-1)


def replicate_summary(out, counts):
    """Posterior predictive p-values with realized discrepancies (Gelman, Meng & Stern 1996) from the fields of
    ``Catalog.replicate_check``: ``out`` (S, R, 8, 2) and ``counts`` (R,), the stars per range.  Rows: "all" (the ranges
    combined in ascending order: sums and counts added, the maximum taken), then one per range.  For the observed and
    the replicated residuals alike the discrepancies ``names`` are derived per sample: ``mean`` = S1/n, ``var_ratio`` =
    S2/n, ``skew`` and ``kurt_excess`` from the raw moments, ``rot_amp`` = 2 hypot(SIN, COS)/n, ``max_abs_z``,
    ``n_tail3``.  Returns ``names``, ``n_stars`` (R + 1,), ``obs`` / ``rep`` (S, R + 1, 7), ``p_value`` (R + 1, 7) =
    mean_s[T_rep >= T_obs], ``extreme`` = min(p, 1 - p), ``bands`` (R + 1, 7, 2, 3): the 16 / 50 / 84 % quantiles over the
    samples of observed ([..., 0, :]) and replicated.  A row without stars is NaN throughout.  Every field is additive
    over stars, so the fields of disjoint star sets may be added before the summary."""
    out = np.asarray(out, dtype=np.float64)
    counts = np.asarray(counts, dtype=np.float64).reshape(-1)
    if out.ndim != 4 or out.shape[2:] != (8, 2) or out.shape[1] != counts.size:
        raise ValueError("out must have shape (S, R, 8, 2) and counts (R,)")
    total = np.zeros((out.shape[0], 8, 2))
    for r in range(out.shape[1]):
        total[:, :6] += out[:, r, :6]
        total[:, 7] += out[:, r, 7]
        total[:, 6] = np.maximum(total[:, 6], out[:, r, 6])                         # (keeps a NaN)
    fields = np.concatenate([total[:, None], out], axis=1)                          # (S, R + 1, 8, 2)
    n = np.concatenate([[counts.sum()], counts])
    obs = _replicate_discrepancies(fields[..., 0], n[None, :])
    rep = _replicate_discrepancies(fields[..., 1], n[None, :])
    p = np.mean(rep >= obs, axis=0)
    p[n == 0] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        bands = np.stack([np.nanpercentile(x, [16, 50, 84], axis=0) for x in (obs, rep)], axis=0)     # (2, 3, R + 1, 7)
    return {"names": REPLICATE_NAMES, "n_stars": n.astype(np.int64), "obs": obs, "rep": rep, "p_value": p,
            "extreme": np.minimum(p, 1.0 - p), "bands": np.transpose(bands, (2, 3, 0, 1))}


BOOTSTRAP_PERCENTILES = (2.5, 16.0, 50.0, 84.0, 97.5)


def bootstrap_summary(x, x_hat, converged, names, laplace_covariance=None):
    """Moments of the bootstrap replicates ``x`` (B, P) of ``Runner.bootstrap`` around the estimate ``x_hat`` (P,), over the
    CONVERGED replicates only: ``mean``, ``covariance`` (sample, B - 1; the sandwich covariance of the estimate when the
    model is misspecified), ``std``, ``bias`` = mean - x_hat, ``percentiles`` ({2.5, 16, 50, 84, 97.5} -> (P,)),
    ``n_converged``, ``n_replicates``, ``names``.  With ``laplace_covariance`` (``Runner.laplace(x_hat)["covariance"]``)
    also ``std_ratio`` = std / sqrt(diag laplace_covariance): about 1 when the model describes the scatter of the data,
    above 1 where the model-based width is too narrow.  Warns when fewer than 90 % of the replicates converged."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    x_hat = np.asarray(x_hat, dtype=np.float64).reshape(-1)
    converged = np.asarray(converged, dtype=bool).reshape(-1)
    if x.shape != (converged.size, x_hat.size):
        raise ValueError("bootstrap_summary: x must have shape (len(converged), len(x_hat))")
    n_b, n_p = x.shape
    n_ok = int(np.count_nonzero(converged))
    if n_ok < 0.9 * n_b:
        warnings.warn("bootstrap_summary: only {0} of {1} replicates converged; the moments are those of the converged "
                      "ones (raise max_iter, or look at the replicates in x)".format(n_ok, n_b))
    good = x[converged]
    nan = np.full(n_p, np.nan)
    mean = good.mean(axis=0) if n_ok else nan
    cov = np.atleast_2d(np.cov(good, rowvar=False, ddof=1)) if n_ok > 1 else np.full((n_p, n_p), np.nan)
    std = np.sqrt(np.diag(cov))
    pct = {q: (np.percentile(good, q, axis=0) if n_ok else nan.copy()) for q in BOOTSTRAP_PERCENTILES}
    out = {"mean": mean, "covariance": cov, "std": std, "bias": mean - x_hat, "percentiles": pct, "n_converged": n_ok,
           "n_replicates": int(n_b), "names": list(names)}
    if laplace_covariance is not None:
        lap = np.atleast_2d(np.asarray(laplace_covariance, dtype=np.float64))
        if lap.shape != (n_p, n_p):
            raise ValueError("bootstrap_summary: laplace_covariance must have shape (P, P)")
        out["std_ratio"] = std / np.sqrt(np.diag(lap))
    return out


def bagged_summary(chain, n_burn, names, thin=1):
    """The bagged posterior of ``Runner.bagged`` from its chains ``chain`` (B, W, steps, P): bag b sampled the posterior of
    the catalogue under the bootstrap weights of replicate b.  Over the kept draws (every ``thin``-th step after
    ``n_burn``; T_kept per walker):

    * pooled over all bags -- the bagged posterior itself: ``mean``, ``covariance`` (sample, all B W T_kept draws), ``std``,
      ``percentiles`` ({2.5, 16, 50, 84, 97.5} -> (P,));
    * per bag: ``bag_mean`` (B, P), ``bag_var`` (B, P), ``tau`` (B,) the largest integrated autocorrelation time in kept
      steps and ``converged`` (B,) whether the bag keeps 50 of them (``diagnostics.summary`` on the host), and
      ``mean_mcse`` (B, P) = sqrt(bag_var tau / (W T_kept)), the Monte-Carlo standard error of ``bag_mean``;
    * ``within`` (P, P): the mean over the bags of the within-bag covariance; ``between`` (P, P): the sample covariance of
      the bag means; ``mismatch_ratio`` (P,) = diag(between) / diag(within); ``n_bags``, ``n_samples`` (per bag), ``names``.

    What the ratio means.  By the law of total covariance the pooled covariance is within + between (up to the (B - 1) / B
    of the sample formulas).  A bag's posterior is, to first order, a Gaussian around the weighted maximum theta_b with the
    covariance H^-1 of the curvature; weights of mean 1 leave the expected curvature as it is, so ``within`` estimates
    the covariance the standard posterior reports.  The bag means scatter as the weighted maxima do: with weights of
    variance 1 (and ``bag_fraction`` = 1) that is the sandwich H^-1 J H^-1 of the bootstrap, J the covariance of the
    per-star score -- the sampling covariance of the posterior mean whether or not the model describes the data.  Where it
    does, J = H: ``between`` and ``within`` agree, the ratio is about 1 and the bagged covariance is about twice the
    standard posterior's.  A ratio well above 1 says the data scatter more than the model allows (understated errors, a
    background that misses non-members): the symptom ``bootstrap()``'s ``std_ratio`` shows for the point estimate, here
    carried into the intervals.  ``mean_mcse`` tells how much of ``between`` is Monte-Carlo noise of the bag means: its
    mean square adds to diag(between).

    Warns when fewer than 90 % of the bags converged."""
    from .. import diagnostics
    chain = np.asarray(chain, dtype=np.float64)
    if chain.ndim != 4:
        raise ValueError("bagged_summary: chain must have shape (B, W, steps, P)")
    if int(thin) < 1:
        raise ValueError("bagged_summary: thin must be >= 1")
    if not 0 <= int(n_burn) < chain.shape[2]:
        raise ValueError("bagged_summary: n_burn must lie in [0, steps)")
    kept = chain[:, :, int(n_burn)::int(thin), :]
    n_b, n_w, n_t, n_p = kept.shape
    if len(names) != n_p:
        raise ValueError("bagged_summary: names must hold one name per parameter")
    draws = kept.reshape(n_b, n_w * n_t, n_p)
    pooled = draws.reshape(-1, n_p)
    cov = np.atleast_2d(np.cov(pooled, rowvar=False, ddof=1))
    bag_mean = draws.mean(axis=1)
    bag_cov = np.stack([np.atleast_2d(np.cov(d, rowvar=False, ddof=1)) for d in draws])
    bag_var = np.stack([np.diag(c) for c in bag_cov])
    within = bag_cov.mean(axis=0)
    between = np.atleast_2d(np.cov(bag_mean, rowvar=False, ddof=1)) if n_b > 1 else np.full((n_p, n_p), np.nan)
    diag = diagnostics.summary(np.ascontiguousarray(np.transpose(kept, (2, 0, 1, 3))), context=None)
    with np.errstate(invalid="ignore"):
        tau = np.max(np.atleast_2d(diag["tau"]), axis=1)
    converged = np.all(np.atleast_2d(diag["converged"]), axis=1)
    n_ok = int(np.count_nonzero(converged))
    if n_ok < 0.9 * n_b:
        warnings.warn("bagged_summary: only {0} of {1} bags keep 50 autocorrelation times of steps; the bag means carry more "
                      "Monte-Carlo error than the sample count suggests (see mean_mcse; run longer)".format(n_ok, n_b))
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.diag(between) / np.diag(within)
    return {"mean": pooled.mean(axis=0), "covariance": cov, "std": np.sqrt(np.diag(cov)),
            "percentiles": {q: np.percentile(pooled, q, axis=0) for q in BOOTSTRAP_PERCENTILES},
            "bag_mean": bag_mean, "bag_var": bag_var, "within": within, "between": between, "mismatch_ratio": ratio,
            "tau": tau, "converged": converged, "n_converged": n_ok,
            "mean_mcse": np.sqrt(bag_var * tau[:, None] / float(n_w * n_t)), "n_bags": int(n_b), "n_samples": int(n_w * n_t),
            "names": list(names)}


SIMULATED_PERCENTILES = (2.275, 2.5, 15.865, 50.0, 84.135, 97.5, 97.725)     # the central 68.27 % and 95.45 % intervals' ends


def _simulated_kept(chain, n_burn, thin, who):
    chain = np.asarray(chain, dtype=np.float64)
    if chain.ndim != 4:
        raise ValueError("{0}: chain must have shape (E, W, steps, P)".format(who))
    if int(thin) < 1:
        raise ValueError("{0}: thin must be >= 1".format(who))
    if not 0 <= int(n_burn) < chain.shape[2]:
        raise ValueError("{0}: n_burn must lie in [0, steps)".format(who))
    return chain[:, :, int(n_burn)::int(thin), :]


def simulated_fit_summary(chain, n_burn, truths=None, thin=1):
    """Per-fit summaries of the lock-stepped fits of ``Runner.simulated_fits`` from their chains ``chain`` (E, W, steps, P),
    over every ``thin``-th step after ``n_burn``: ``mean``, ``std`` (E, P), ``percentiles`` ({q: (E, P)} for
    ``SIMULATED_PERCENTILES``), ``tau`` (E, P) the integrated autocorrelation times in kept steps and ``converged`` (E,)
    whether the fit keeps 50 of its largest (``diagnostics.summary`` on the host), ``n_samples`` per fit and, with
    ``truths`` (E, P), ``z`` = (mean - truth) / std."""
    from .. import diagnostics
    kept = _simulated_kept(chain, n_burn, thin, "simulated_fit_summary")
    n_e, n_w, n_t, n_p = kept.shape
    draws = kept.reshape(n_e, n_w * n_t, n_p)
    mean, std = draws.mean(axis=1), draws.std(axis=1, ddof=1)
    diag = diagnostics.summary(np.ascontiguousarray(np.transpose(kept, (2, 0, 1, 3))), context=None)
    tau = np.atleast_2d(diag["tau"]).reshape(n_e, n_p)
    out = {"mean": mean, "std": std, "percentiles": {q: np.percentile(draws, q, axis=1) for q in SIMULATED_PERCENTILES},
           "tau": tau, "converged": np.all(np.atleast_2d(diag["converged"]).reshape(n_e, -1), axis=1), "n_samples": int(n_w * n_t)}
    if truths is not None:
        truths = np.asarray(truths, dtype=np.float64).reshape(n_e, n_p)
        with np.errstate(invalid="ignore", divide="ignore"):
            out["z"] = (mean - truths) / std
    return out


def sbc_summary(chain, truths, n_burn, thin=None, n_bins=8, prior_variance=None):
    """Simulation-based calibration (Cook, Gelman & Rubin 2006; Talts et al. 2018) of the fits ``chain`` (E, W, steps, P)
    of E catalogues simulated at ``truths`` (E, P), themselves draws from the prior: if sampler, likelihood and prior
    handling are right, the rank of a truth among the posterior draws of its own catalogue is uniform.

    * ``rank`` (E, P): the number of pooled draws below the truth; the draws are all walkers of every ``thin``-th step
      after ``n_burn``, ``n_draws`` of them per fit.  ``thin`` = None: the largest integrated autocorrelation time over fits
      and parameters, rounded up (``thin`` in the result tells), so that the draws of a walker are nearly independent;
    * ``hist`` (P, n_bins): the ranks 0 .. n_draws in ``n_bins`` bins of equal width, ``expected`` (n_bins,) the uniform
      expectation of every bin, ``chi2`` (P,) against it, ``dof`` = n_bins - 1 and ``p_value`` (P,) its upper tail;
    * ``ecdf_max`` (P,): the largest distance between the ranks' empirical distribution function and the uniform one;
    * ``contraction`` (P,): 1 - mean posterior variance / ``prior_variance`` (P,), NaN where that is not finite or not given.

    Too narrow posteriors (or a fit told too small errors) pile the ranks up at both ends (a U shape), too wide ones in the
    middle; a biased fit tilts the histogram."""
    from scipy.special import gammaincc
    from .. import diagnostics
    truths = np.atleast_2d(np.asarray(truths, dtype=np.float64))
    if int(n_bins) < 2:
        raise ValueError("sbc_summary: n_bins must be >= 2")
    n_bins = int(n_bins)
    if thin is None:
        full = _simulated_kept(chain, n_burn, 1, "sbc_summary")
        diag = diagnostics.summary(np.ascontiguousarray(np.transpose(full, (2, 0, 1, 3))), context=None)
        tau = np.asarray(diag["tau"], dtype=np.float64)
        worst = np.nanmax(tau) if np.any(np.isfinite(tau)) else 1.0
        thin = max(1, int(np.ceil(worst)))
    kept = _simulated_kept(chain, n_burn, thin, "sbc_summary")
    n_e, n_w, n_t, n_p = kept.shape
    if truths.shape != (n_e, n_p):
        raise ValueError("sbc_summary: truths must have shape {0}".format((n_e, n_p)))
    draws = kept.reshape(n_e, n_w * n_t, n_p)
    n_draws = n_w * n_t
    rank = np.count_nonzero(draws < truths[:, None, :], axis=1).astype(np.int64)
    bin_of = np.arange(n_draws + 1, dtype=np.int64) * n_bins // (n_draws + 1)
    expected = np.bincount(bin_of, minlength=n_bins) * (float(n_e) / (n_draws + 1))
    hist = np.stack([np.bincount(bin_of[rank[:, p]], minlength=n_bins) for p in range(n_p)])
    chi2 = ((hist - expected) ** 2 / expected).sum(axis=1)
    u = np.sort((rank + 0.5) / (n_draws + 1.0), axis=0)
    i = np.arange(1, n_e + 1, dtype=np.float64)[:, None]
    ecdf_max = np.maximum(np.max(i / n_e - u, axis=0), np.max(u - (i - 1.0) / n_e, axis=0))
    contraction = np.full(n_p, np.nan)
    if prior_variance is not None:
        pv = np.asarray(prior_variance, dtype=np.float64).reshape(n_p)
        good = np.isfinite(pv) & (pv > 0)
        contraction[good] = 1.0 - draws.var(axis=1, ddof=1).mean(axis=0)[good] / pv[good]
    return {"rank": rank, "n_draws": int(n_draws), "thin": int(thin), "hist": hist, "expected": expected, "chi2": chi2,
            "dof": n_bins - 1, "p_value": gammaincc(0.5 * (n_bins - 1), 0.5 * chi2), "ecdf_max": ecdf_max,
            "contraction": contraction, "n_sims": int(n_e), "n_bins": n_bins}


def _recovery_stats(samples, truth):
    """samples (E, n) of one scalar per fit, its true value -> the recovery figures of that scalar."""
    n_e = samples.shape[0]
    mean, std = samples.mean(axis=1), samples.std(axis=1, ddof=1)
    q = np.percentile(samples, [2.275, 15.865, 84.135, 97.725, 2.5], axis=1)
    c68 = float(np.mean((q[1] <= truth) & (truth <= q[2])))
    c95 = float(np.mean((q[0] <= truth) & (truth <= q[3])))
    with np.errstate(invalid="ignore", divide="ignore"):
        z = (mean - truth) / std
    return {"truth": float(truth), "bias": float(np.mean(mean - truth)), "scatter": float(np.std(mean, ddof=1)) if n_e > 1 else np.nan,
            "rmse": float(np.sqrt(np.mean((mean - truth) ** 2))),
            "coverage": {68: c68, 95: c95},
            "coverage_se": {68: float(np.sqrt(c68 * (1.0 - c68) / n_e)), 95: float(np.sqrt(c95 * (1.0 - c95) / n_e))},
            "z_mean": float(np.mean(z)), "z_std": float(np.std(z, ddof=1)) if n_e > 1 else np.nan, "q2.5": q[4]}


def recovery_summary(chain, truth, n_burn, names, thin=1, functions=None, null=None):
    """Injection-recovery figures of the fits ``chain`` (E, W, steps, P) of E catalogues simulated at the one ``truth`` (P,),
    over every ``thin``-th step after ``n_burn``.  Per parameter, as (P,) arrays: ``bias`` (the mean over the fits of
    posterior mean - truth), ``scatter`` (the standard deviation of the posterior means), ``rmse``, ``coverage`` ({68, 95}:
    the share of fits whose central 68.27 % / 95.45 % interval holds the truth) with ``coverage_se`` (binomial, from the
    share itself), and ``z_mean`` / ``z_std`` of z = (mean - truth) / std (0 and 1 for a calibrated fit).

    ``functions``: {name: f}, f maps draws (n, P) to (n,) (e.g. a rotation amplitude); ``functions[name]`` in the result
    holds the same figures as scalars for f, with its value at the truth, and, with ``null`` (a parameter row, P), ``exceeds``:
    the share of fits whose 2.5 % quantile of f lies above f(null) -- how often the effect is detected."""
    kept = _simulated_kept(chain, n_burn, thin, "recovery_summary")
    n_e, n_w, n_t, n_p = kept.shape
    truth = np.asarray(truth, dtype=np.float64).reshape(-1)
    if truth.size != n_p or len(names) != n_p:
        raise ValueError("recovery_summary: truth and names must hold one entry per parameter")
    draws = kept.reshape(n_e, n_w * n_t, n_p)
    per = [_recovery_stats(draws[:, :, p], truth[p]) for p in range(n_p)]
    out = {k: np.array([s[k] for s in per]) for k in ("bias", "scatter", "rmse", "z_mean", "z_std")}
    out["coverage"] = {c: np.array([s["coverage"][c] for s in per]) for c in (68, 95)}
    out["coverage_se"] = {c: np.array([s["coverage_se"][c] for s in per]) for c in (68, 95)}
    out.update({"truth": truth, "n_sims": int(n_e), "n_samples": int(n_w * n_t), "names": list(names), "functions": {}})
    for name, f in (functions or {}).items():
        samples = np.stack([np.asarray(f(d), dtype=np.float64).reshape(-1) for d in draws])
        s = _recovery_stats(samples, float(np.asarray(f(truth[None, :])).reshape(-1)[0]))
        low = s.pop("q2.5")
        if null is not None:
            at_null = float(np.asarray(f(np.asarray(null, dtype=np.float64).reshape(1, n_p))).reshape(-1)[0])
            s["null"], s["exceeds"] = at_null, float(np.mean(low > at_null))
        out["functions"][name] = s
    return out


def parametric_bootstrap_summary(x, x_hat, converged, names, laplace_covariance=None):
    """Moments of the refits ``x`` (E, P) of ``Runner.parametric_bootstrap`` -- the maxima of E catalogues simulated at the
    estimate ``x_hat`` (P,) -- over the CONVERGED refits only: ``mean``, ``bias`` = mean - x_hat (the bias of the estimator
    under the fitted model), ``covariance`` (sample, E - 1: the model-based sampling covariance of the estimate), ``std``,
    ``percentiles`` ({2.5, 16, 50, 84, 97.5} -> (P,)), ``n_converged``, ``n_sims``, ``names``, and with
    ``laplace_covariance`` (``Runner.laplace(x_hat)["covariance"]``) ``std_ratio`` = std / sqrt(diag laplace_covariance):
    about 1 where the likelihood is quadratic over the estimate's scatter.  Against ``bootstrap_summary``'s ``std``, which
    makes no use of the model, the ratio tells whether the model describes the scatter of the data.  Warns when fewer than
    90 % of the refits converged."""
    out = bootstrap_summary(x, x_hat, converged, names, laplace_covariance)
    out["n_sims"] = out.pop("n_replicates")
    return out


LRT_QUANTILES = (50.0, 90.0, 95.0, 99.0, 99.9)


def lrt_summary(lnprob_null, lnprob_full, converged_null, converged_full, stat_obs, df, tolerance=0.0):
    """The simulated null distribution of a likelihood-ratio statistic (``Runner.lrt``): ``lnprob_null`` / ``lnprob_full``
    (E,) the maxima of the null and of the full fit on E catalogues simulated under the null, ``converged_*`` (E,) whether
    each fit converged, ``stat_obs`` the statistic of the data and ``df`` the number of parameters the null fixes.

    ``stat`` (E,) = 2 (lnprob_full - lnprob_null); ``used`` (E,): both fits converged; ``n_used``; ``p_value`` =
    (1 + #{used, stat >= stat_obs}) / (1 + n_used), the Monte-Carlo p-value that counts the data among the draws (Davison &
    Hinkley 1997), never 0; ``p_se`` its binomial standard error; ``p_asymptotic`` the upper tail of chi2(``df``) at
    ``stat_obs`` (Wilks), for comparison; ``quantiles`` ({50, 90, 95, 99, 99.9} -> the null statistic's quantile over the
    used simulations); ``n_negative``: used statistics below -``tolerance`` -- nested models cannot give one, so a count
    above 0 is a defect of the fits (a full fit stuck below its null)."""
    from scipy.special import gammaincc
    l0, l1 = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (lnprob_null, lnprob_full))
    c0, c1 = (np.asarray(a, dtype=bool).reshape(-1) for a in (converged_null, converged_full))
    if not (l0.size == l1.size == c0.size == c1.size):
        raise ValueError("lrt_summary: the four arrays must hold one entry per simulation")
    if int(df) < 1:
        raise ValueError("lrt_summary: df must be >= 1")
    stat = 2.0 * (l1 - l0)
    used = c0 & c1 & np.isfinite(stat)
    n_used = int(np.count_nonzero(used))
    if n_used < 0.9 * stat.size:
        warnings.warn("lrt_summary: only {0} of {1} simulations have both fits converged; the p-value is taken over "
                      "those".format(n_used, stat.size))
    stat_obs = float(stat_obs)
    p = (1.0 + np.count_nonzero(stat[used] >= stat_obs)) / (1.0 + n_used)
    quantiles = {q: (float(np.percentile(stat[used], q)) if n_used else np.nan) for q in LRT_QUANTILES}
    return {"stat": stat, "used": used, "n_used": n_used, "stat_obs": stat_obs, "p_value": float(p),
            "p_se": float(np.sqrt(p * (1.0 - p) / (1.0 + n_used))), "df": int(df),
            "p_asymptotic": float(gammaincc(0.5 * int(df), 0.5 * max(stat_obs, 0.0))), "quantiles": quantiles,
            "n_negative": int(np.count_nonzero(stat[used] < -float(tolerance))), "n_sims": int(stat.size)}


class Runner(object):
    """Parent of the analysis classes.  Sub-classes name the observables and model parameters they
    need (``OBSERVABLES``, ``MODEL_PARAMETERS``) and implement ``_lnlike_batch``."""

    MODEL_PARAMETERS = []
    OBSERVABLES = {"v": "km/s", "verr": "km/s"}
    parameters_file = None

    def __init__(self, data, parameters, seed=123, background=None, context=None, precision="f64", **kwargs):
        """
        Parameters
        ----------
        data : DataReader
            The observed data.
        parameters : Parameters
            The model parameters.
        seed : int, optional
            Seed of the global NumPy random number generator (runner.py:59).
        background : Gaussian or SingleStars, optional
            Fixed background population; needs a ``pmember`` column in the data (runner.py:96-103).
        context : _native.Context, optional
            GPU context (devices / rank).  Default: one process-wide context on device 0.
        precision : {'f64', 'f32', 'f32acc64'}
            Arithmetic of the kernels; 'f64' is the parity mode.  The float32 kernels keep their stated tolerances
            only inside the float32 accuracy domain (include/mcd.h); a walker can leave it in the middle of a chain, so
            the catalogues this class creates for 'f32' / 'f32acc64' evaluate such tables regardless (option
            ``f32_domain`` = 0; ``_native.Catalog``'s own default refuses them) and count them.  The first time a
            catalogue's count is non-zero one ``UserWarning`` gives the library's reason and the condition numbers;
            ``f32_outside()`` returns the counters.
        """
        assert not kwargs, "Unknown keyword arguments provided: {0}".format(kwargs)      # runner.py:56

        np.random.seed(seed)                                                              # runner.py:59

        assert isinstance(data, DataReader), "'data' must be instance of {0}".format(DataReader.__module__)
        self.data = data

        if "ra" in self.OBSERVABLES or "dec" in self.OBSERVABLES:
            if not data.has_coordinates:
                raise IOError("Missing WCS coordinates of observed data.")                # runner.py:70-72

        for required, unit in self.OBSERVABLES.items():
            assert required in data.data.columns, "Input data missing required column <{0}>".format(required)
            if unit is not None and data.data.unit(required) is None:
                logger.warning("Missing units for <%s> values. Assuming %s.", required, unit)
            setattr(self, required, data.column(required, unit))

        assert isinstance(parameters, Parameters), "'parameters' must be instance of {0}".format(Parameters.__module__)
        self.parameters = parameters

        missing = set(self.MODEL_PARAMETERS).difference(self.parameters)
        if missing:
            raise IOError("Missing required parameter(s): '{0}'".format(missing))          # runner.py:87-89
        unused = set(self.parameters).difference(self.MODEL_PARAMETERS)
        if unused:
            logger.warning("Superfluous parameter(s) provided: '%s'", unused)

        self.background = background
        if self.background:
            assert isinstance(background, (SingleStars, Gaussian)), \
                "'background' must be an instance of a Background class."
            if "pmember" not in self.data.data.columns:
                logger.error("Inclusion of background population requires prior probabilities for membership.")
            if isinstance(background, SingleStars):        # O(N M) kernel-density precompute: on the device
                lnbg = self.background(self.v, self.verr, context=context)
            else:
                lnbg = self.background(self.v, self.verr)
            self.lnlike_background = np.asarray(lnbg, dtype=np.float64)
            self.pmember = data.column("pmember")
        else:
            self.lnlike_background = None
            self.pmember = None

        self._context = context
        self._precision = precision
        self._catalog = None
        self._catalog_key = None

    # ------------------------------------------------------------------ bookkeeping
    @classmethod
    def default_parameters(cls):
        if cls.parameters_file is None:
            raise NotImplementedError
        return Parameters().load(cls.parameters_file)

    @property
    def n_data(self):
        return self.data.sample_size

    @property
    def fitted_parameters(self):
        return [p for p in self.parameters if not self.parameters[p].fixed]

    @property
    def n_fitted_parameters(self):
        return len(self.fitted_parameters)

    @property
    def units(self):
        return {p: self.parameters[p].unit for p in self.parameters}

    @property
    def labels(self):
        return [par.label for par in self.parameters.values() if not par.fixed]

    @property
    def context(self):
        if self._context is None:
            self._context = _native.default_context()
        return self._context

    # ------------------------------------------------------------------ single-walker API (reference names)
    def fetch_parameter_values(self, values):
        """Dictionary with one value per model parameter, fixed or not (runner.py:143-180).  As in the
        reference, the values are also written back into ``self.parameters``."""
        values = np.asarray(values, dtype=np.float64).reshape(-1)
        resolved = self.parameters.resolve_batch(values[None, :])
        current = OrderedDict((name, float(col[0])) for name, col in resolved.items())
        for name, val in current.items():
            if self.parameters[name].expr is None:
                self.parameters[name].value = val                                          # runner.py:176
        return current

    def lnprior(self, values, parameters_to_ignore=None):
        """0 when every parameter lies inside its inclusive bounds (plus optional ``lnprior``
        expressions), -inf otherwise (runner.py:182-217)."""
        values = np.asarray(values, dtype=np.float64).reshape(-1)
        lnlike = 0
        for name, value in self.fetch_parameter_values(values).items():
            lnlike += self.parameters[name].evaluate_lnprior(value)
            if not np.isfinite(lnlike):
                return -np.inf
        return lnlike

    def lnlike(self, values):
        """Log-likelihood of one parameter vector, without priors (place-holder in the reference,
        runner.py:219-238; sub-classes evaluate it on the GPU)."""
        values = np.asarray(values, dtype=np.float64).reshape(1, -1)
        self.fetch_parameter_values(values[0])
        return float(self.lnlike_batch(values)[0])

    def lnprob(self, values):
        """Log-posterior of one parameter vector (runner.py:288-306): the likelihood is not evaluated
        when the prior is not finite."""
        lp = self.lnprior(values)
        if not np.isfinite(lp):
            return -np.inf
        return self.lnlike(values) + lp

    # ------------------------------------------------------------------ batched API (new)
    def lnprior_batch(self, values):
        return self.parameters.lnprior_batch(self.parameters.resolve_batch(values))

    def lnlike_batch(self, values):
        """(W, P) free-parameter vectors -> (W,) log-likelihoods, one kernel launch."""
        resolved = self.parameters.resolve_batch(values)
        return self._lnlike_batch(resolved)

    def _plan(self):
        sig = _BatchPlan.signature(self)
        if getattr(self, "_plan_sig", None) != sig:
            self._plan_cache = _BatchPlan(self)
            self._plan_sig = sig
        return self._plan_cache

    def lnprob_batch(self, values):
        """(W, P) -> (W,) log-posteriors.  Walkers outside the prior get -inf; their rows are replaced by
        a valid row for the launch and masked afterwards (the reference skips the evaluation)."""
        values = np.atleast_2d(np.asarray(values, dtype=np.float64))
        if self._context is not None and getattr(self._context, "n_ranks", 1) > 1:
            self._check_ranks_agree(values)
        plan = self._plan()
        if plan.direct_cols is not None and values.shape[1] == plan.free_idx.size:
            ok = plan.prior_ok_free(values)
            lp, ok = plan.prior_free(values, ok)
            n_ok = int(np.count_nonzero(ok))
            if n_ok == 0:
                return np.full(values.shape[0], -np.inf)
            if n_ok != ok.size:
                values = values.copy()
                values[~ok] = values[int(np.flatnonzero(ok)[0])]
            cat = self._catalog
            if cat is None or plan.catalog_key != self._catalog_key:
                cat = self._ensure_catalog()
            ll = cat.loglike(plan.table_direct(values))
            if self._precision != "f64":
                self._note_f32(cat)
            if lp is not None:
                ll = ll + lp
            if n_ok == ok.size:
                return ll
            out = np.full(values.shape[0], -np.inf)
            out[ok] = ll[ok]
            return out
        if plan.simple and values.shape[1] == plan.free_idx.size:
            # fast host path: flat bounds, no expression priors / constraints
            full = plan.full(values)
            lp, ok = plan.prior_free(values, plan.prior_ok(full))
            out = np.full(values.shape[0], -np.inf)
            n_ok = int(ok.sum())
            if n_ok == 0:
                return out
            if n_ok != ok.size:
                full[~ok] = full[int(np.flatnonzero(ok)[0])]
            cat = self._catalog
            if cat is None or plan.catalog_key != self._catalog_key:
                cat = self._ensure_catalog()
            ll = cat.loglike(plan.table(full))
            if self._precision != "f64":
                self._note_f32(cat)
            if lp is not None:
                ll = ll + lp
            if n_ok == ok.size:
                return ll
            out[ok] = ll[ok]
            return out
        resolved = self.parameters.resolve_batch(values)
        lp = self.parameters.lnprior_batch(resolved)
        ok = np.isfinite(lp)
        out = np.full(values.shape[0], -np.inf)
        if not ok.any():
            return out
        if not ok.all():
            donor = int(np.flatnonzero(ok)[0])
            resolved = OrderedDict((k, np.where(ok, col, col[donor])) for k, col in resolved.items())
        ll = self._lnlike_batch(resolved)
        out[ok] = ll[ok] + lp[ok]
        return out

    # ------------------------------------------------------------------ first-order methods (new)
    def _grad_plan(self):
        """The plan, refused unless every parameter is a box-bounded one with a flat or a structured prior: the chain rule
        below has no term for an ``expr`` constraint or an ``lnprior`` expression."""
        plan = self._plan()
        if not plan.simple:
            for name, par in self.parameters.items():
                if par._expr is not None:
                    raise NotImplementedError("gradients through the expr constraint of parameter '{0}' are not "
                                              "implemented".format(name))
                if par._lnprior is not None:
                    raise NotImplementedError("gradients through the lnprior expression of parameter '{0}' are not "
                                              "implemented".format(name))
        return plan

    def lnlike_grad_batch(self, values):
        """(W, P) free-parameter vectors -> ((W,) log-likelihoods, (W, P) gradients with respect to the FREE parameters, in
        their own units), one launch of the device's value-and-gradient kernel.  The chain rule of the batch plan is
        applied on the host: a kernel column fed by free parameter j contributes its unit factor times the column's
        partial derivative, columns fed by fixed parameters are dropped.  Rows outside the prior get (-inf, zero row)."""
        return self._lnlike_grad_rows(values, lambda cat, table: cat.loglike_grad(table))

    def _lnlike_grad_rows(self, values, evaluate):
        """``lnlike_grad_batch`` around ``evaluate(catalogue, kernel table) -> (values, kernel-column gradients)``."""
        values = np.atleast_2d(np.asarray(values, dtype=np.float64))
        plan = self._grad_plan()
        if values.shape[1] != plan.free_idx.size:
            raise ValueError("expected {0} free parameters per row, got {1}".format(plan.free_idx.size, values.shape[1]))
        if self._context is not None and getattr(self._context, "n_ranks", 1) > 1:
            self._check_ranks_agree(values)
        n = values.shape[0]
        out, grad = np.full(n, -np.inf), np.zeros((n, plan.free_idx.size))
        full = plan.full(values)
        ok = plan.prior_ok(full)
        if not ok.any():
            return out, grad
        if not ok.all():
            full[~ok] = full[int(np.flatnonzero(ok)[0])]
        cat = self._catalog
        if cat is None or plan.catalog_key != self._catalog_key:
            cat = self._ensure_catalog()
        if cat.n_sets != 1:
            raise NotImplementedError("gradients are defined for un-binned analyses")
        ll, g_cols = evaluate(cat, plan.table(full))
        if plan.kernel_fac is not None:
            g_cols = g_cols * plan.kernel_fac
        free_pos = {int(i): j for j, i in enumerate(plan.free_idx)}
        g_free = np.zeros((n, plan.free_idx.size))
        for c, i in enumerate(plan.kernel_idx):
            if int(i) in free_pos:
                g_free[:, free_pos[int(i)]] += g_cols[:, c]
        out[ok] = ll[ok]
        grad[ok] = g_free[ok]
        return out, grad

    def lnprob_grad_batch(self, values):
        """As ``lnlike_grad_batch`` for the log-posterior: inside the box, value and gradient of the likelihood plus those of
        the structured priors (``Parameter.prior``; one ``mcd_prior_eval`` call) -- with flat priors the likelihood's own --
        and (-inf, zero row) outside the box or where a log-normal coordinate is <= 0."""
        values = np.atleast_2d(np.asarray(values, dtype=np.float64))
        plan = self._grad_plan()
        if plan.prior is None:
            return self.lnlike_grad_batch(values)
        return self._lnprob_grad_rows(values, plan, self.lnlike_grad_batch)

    def _lnprob_grad_rows(self, values, plan, lnlike_grad):
        """The structured priors of ``plan`` around ``lnlike_grad(rows) -> (values, gradients)``."""
        if values.shape[1] != plan.free_idx.size:
            raise ValueError("expected {0} free parameters per row, got {1}".format(plan.free_idx.size, values.shape[1]))
        lp, g_lp = _native.prior_eval(plan.prior, values, want_grad=True)
        inside = lp > -np.inf
        if not inside.any():
            return np.full(values.shape[0], -np.inf), np.zeros(values.shape)
        rows = values
        if not inside.all():                       # such a row takes a valid row's place in the launch and is masked
            rows = values.copy()
            rows[~inside] = values[int(np.flatnonzero(inside)[0])]
        out, grad = lnlike_grad(rows)
        ok = inside & np.isfinite(out)
        out = np.where(ok, out + np.where(inside, lp, 0.0), -np.inf)
        grad = np.where(ok[:, None], grad + np.where(inside[:, None], g_lp, 0.0), 0.0)
        return out, grad

    def maximize(self, n_starts=64, x0=None, max_iter=200, gtol=1e-8):
        """Maximum of the log-posterior inside the prior box (MAP: structured priors count; with flat boxes the
        maximum-likelihood estimate), by a
        batched projected BFGS on the device gradient (``optimize.maximize_batch``) from ``n_starts`` rows of
        ``get_initials`` or from the rows of ``x0``.

        The default of 64 starts fills a wavefront: the kernel's lane = walker layout evaluates 64 parameter rows per
        wave for the price of one, and idles the lanes below that.

        Returns a dict: ``x`` the best start's position, ``lnprob`` and ``grad`` there, ``n_iter`` and ``converged`` of that
        start, and ``all_x`` (W, P), ``all_lnprob`` (W,), ``all_converged`` (W,) for every start."""
        from ..optimize import maximize_batch
        plan = self._grad_plan()
        starts = self.get_initials(int(n_starts)) if x0 is None else np.atleast_2d(np.asarray(x0, dtype=np.float64))
        lo, hi = plan.lo[plan.free_idx], plan.hi[plan.free_idx]
        res = maximize_batch(self.lnprob_grad_batch, starts, lo, hi, max_iter=max_iter, gtol=gtol)
        f = np.where(np.isfinite(res["f"]), res["f"], -np.inf)
        # the best converged start, or the best of all when none converged
        pool = np.flatnonzero(res["converged"]) if res["converged"].any() else np.arange(f.size)
        best = int(pool[np.argmax(f[pool])])
        return {"x": res["x"][best].copy(), "lnprob": float(f[best]), "grad": res["grad"][best].copy(),
                "n_iter": int(res["n_iter"][best]), "converged": bool(res["converged"][best]), "all_x": res["x"],
                "all_lnprob": f, "all_converged": res["converged"]}

    def laplace(self, x, rel_step=1e-4):
        """Laplace approximation at ``x`` (a maximum inside the box): the Hessian of the log-posterior (likelihood plus
        structured priors) by central
        differences of the device gradient -- all 2 P displaced rows in ONE ``lnprob_grad_batch`` call -- symmetrised, and
        ``covariance = inv(-H)``.  The step of parameter j is ``rel_step * max(|x_j|, width of a finite prior box / 100,
        1e-3)``.  ValueError when ``x`` sits on a bound or when -H is not positive definite (not a maximum)."""
        plan = self._grad_plan()
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        lo, hi = plan.lo[plan.free_idx], plan.hi[plan.free_idx]
        n_p = x.size
        if np.any(x <= lo) or np.any(x >= hi):
            raise ValueError("laplace: x sits on a bound of the prior in parameter(s) {0}".format(
                [plan.names[int(plan.free_idx[j])] for j in np.flatnonzero((x <= lo) | (x >= hi))]))
        width = np.where(np.isfinite(hi - lo), (hi - lo) / 100.0, 0.0)
        h = rel_step * np.maximum(np.maximum(np.abs(x), width), 1e-3)
        h = np.minimum(h, 0.5 * np.minimum(x - lo, hi - x))
        rows = np.tile(x, (2 * n_p, 1))
        rows[np.arange(n_p), np.arange(n_p)] += h
        rows[n_p + np.arange(n_p), np.arange(n_p)] -= h
        step = rows[:n_p].diagonal() - rows[n_p:].diagonal()          # the steps as represented
        value, grad = self.lnprob_grad_batch(rows)
        if not np.all(np.isfinite(value)):
            raise ValueError("laplace: a displaced point left the prior")
        hess = (grad[:n_p] - grad[n_p:]) / step[:, None]              # row j: d grad / d x_j
        hess = 0.5 * (hess + hess.T)
        try:
            np.linalg.cholesky(-hess)
        except np.linalg.LinAlgError:
            raise ValueError("laplace: -H is not positive definite at x (not a maximum)")
        return {"hessian": hess, "covariance": np.linalg.inv(-hess)}

    def get_initials_laplace(self, n_walkers, x, covariance):
        """(n_walkers, P) start positions drawn from the Gaussian N(x, covariance) of ``laplace`` and clipped into the
        prior box."""
        plan = self._grad_plan()
        x = np.asarray(x, dtype=np.float64).reshape(-1)
        chol = np.linalg.cholesky(np.asarray(covariance, dtype=np.float64))
        draws = x + np.random.standard_normal((int(n_walkers), x.size)) @ chol.T      # (NumPy's global generator, as get_initials)
        return np.clip(draws, plan.lo[plan.free_idx], plan.hi[plan.free_idx])

    # ------------------------------------------------------------------ weighted-likelihood bootstrap (new)
    def lnprob_weighted_grad_batch(self, values, row_replicate, scheme="exponential", seed=0, weights=None):
        """``lnprob_grad_batch`` with the stars of row r weighted by its replicate ``row_replicate[r]``: (W, P) free-parameter
        vectors -> ((W,) values, (W, P) gradients) of  sum_i w(b, i) lnL_i + ln prior,  one launch of the device's weighted
        value-and-gradient kernel (``_native.Catalog.weighted_loglike_grad``: the weights of "exponential" and "poisson"
        are generated on the device from (seed, replicate, star); "explicit" reads ``weights`` (n_replicates, N)).  The
        chain rule, the prior handling and the donor rows are ``lnprob_grad_batch``'s; structured priors enter UNWEIGHTED
        (the weighted-likelihood bootstrap of Newton & Raftery 1994).  The refusals of gradients apply, and the call runs on
        one device in one process."""
        self._holdout_check("lnprob_weighted_grad_batch")
        values = np.atleast_2d(np.asarray(values, dtype=np.float64))
        rep = np.ascontiguousarray(row_replicate, dtype=np.int64).reshape(-1)
        if rep.size != values.shape[0]:
            raise ValueError("row_replicate must hold one replicate per row of values")
        plan = self._grad_plan()

        def lnlike_grad(rows):
            return self._lnlike_grad_rows(rows, lambda cat, table: cat.weighted_loglike_grad(
                table, rep, scheme=scheme, seed=seed, weights=weights))
        if plan.prior is None:
            return lnlike_grad(values)
        return self._lnprob_grad_rows(values, plan, lnlike_grad)

    def bootstrap(self, n_replicates=256, scheme="exponential", seed=None, x_hat=None, max_iter=200, gtol=1e-8):
        """Weighted-likelihood bootstrap of the maximum (Rubin 1981; Newton & Raftery 1994; Lyddon, Holmes & Walker 2019):
        ``n_replicates`` refits of the catalogue under random star weights -- ``scheme`` "exponential": Exp(1) weights, the
        smooth Bayesian bootstrap; "poisson": Poisson(1) counts, the nonparametric bootstrap -- as ONE lock-stepped
        ``optimize.maximize_batch`` run: replicate b = row b starts at ``x_hat`` (default: ``maximize()["x"]``) and climbs
        ``lnprob_weighted_grad_batch`` with replicate id b.  The weights are a function of (seed, b, star) alone
        (``_native.bootstrap_weights`` replays them); the same seed gives the same result bit for bit.

        Returns ``bootstrap_summary`` of the replicates (with ``std_ratio`` against ``laplace(x_hat)`` where that exists)
        plus ``x`` (B, P), ``converged`` (B,), ``n_iter`` (B,), ``x_hat``, ``seed`` and ``scheme``.  The spread of the
        replicates is the sampling (sandwich) covariance of the estimate whether or not the model describes the data;
        ``covariance`` is accepted wherever ``laplace()["covariance"]`` is: ``get_initials_laplace`` and
        ``hmc(covariance=...)``."""
        from ..optimize import maximize_batch
        self._holdout_check("bootstrap")
        plan = self._grad_plan()
        n_b = int(n_replicates)
        if n_b < 1:
            raise ValueError("bootstrap: n_replicates must be >= 1")
        if scheme not in ("exponential", "poisson"):
            raise ValueError("bootstrap: scheme must be 'exponential' or 'poisson'")
        if seed is None:
            seed = int(np.random.SeedSequence().entropy % (2 ** 63))
        x_hat = self.maximize(max_iter=max_iter, gtol=gtol)["x"] if x_hat is None else \
            np.asarray(x_hat, dtype=np.float64).reshape(-1)
        if x_hat.size != plan.free_idx.size:
            raise ValueError("bootstrap: x_hat must hold the {0} free parameters".format(plan.free_idx.size))
        rep = np.arange(n_b, dtype=np.int64)
        lo, hi = plan.lo[plan.free_idx], plan.hi[plan.free_idx]

        def value_and_grad(x):
            return self.lnprob_weighted_grad_batch(x, rep, scheme=scheme, seed=seed)
        res = maximize_batch(value_and_grad, np.tile(x_hat, (n_b, 1)), lo, hi, max_iter=max_iter, gtol=gtol)
        try:
            laplace = self.laplace(x_hat)["covariance"]
        except ValueError:
            laplace = None
        out = bootstrap_summary(res["x"], x_hat, res["converged"], [plan.names[int(i)] for i in plan.free_idx], laplace)
        out.update({"x": res["x"], "converged": res["converged"], "n_iter": res["n_iter"], "x_hat": x_hat, "seed": int(seed),
                    "scheme": scheme})
        return out

    # ------------------------------------------------------------------ bagged posterior (new)
    def lnprob_weighted_batch(self, values, row_replicate, scheme="exponential", seed=0, weights=None, weight_scale=1.0):
        """``lnprob_batch`` with the stars of every row weighted by the row's replicate: ``values`` (..., P) free-parameter
        vectors and ``row_replicate``, one replicate id per row in C order, -> (...) values of
        weight_scale sum_i w(b, i) lnL_i + ln prior,  one launch of the device's weighted VALUE kernel
        (``_native.Catalog.weighted_loglike``; no gradient is computed: what a stretch move reads).  Weights as in
        ``lnprob_weighted_grad_batch``.  Box and structured priors as in ``lnprob_batch``: rows outside the prior are
        -inf and take a donor row for the launch; structured priors enter unweighted and unscaled.  Runs on one device
        in one process, on un-binned float64 catalogues."""
        self._holdout_check("lnprob_weighted_batch")
        values = np.asarray(values, dtype=np.float64)
        n_p = self.n_fitted_parameters
        if values.ndim < 1 or values.shape[-1] != n_p:
            raise ValueError("values must have shape (..., {0})".format(n_p))
        lead = values.shape[:-1]
        rep = np.ascontiguousarray(row_replicate, dtype=np.int64).reshape(-1)
        rows = values.reshape(-1, n_p)
        if rep.size != rows.shape[0]:
            raise ValueError("row_replicate must hold one replicate per row of values")
        pars = self.parameters
        resolved = pars.resolve_batch(rows)
        lp = pars.lnprior_batch(resolved)
        ok = np.isfinite(lp)
        out = np.full(lp.shape, -np.inf)
        if ok.any():
            if not ok.all():
                donor = int(np.flatnonzero(ok)[0])
                resolved = OrderedDict((k, np.where(ok, col, col[donor])) for k, col in resolved.items())
            lnl = self._ensure_catalog().weighted_loglike(self._kernel_table(resolved), rep, scheme=scheme, seed=seed,
                                                          weights=weights)
            out[ok] = float(weight_scale) * lnl[ok] + lp[ok]
        return out.reshape(lead)

    def bagged(self, n_bags=64, n_walkers=64, n_steps=600, n_burn=200, scheme="exponential", seed=None, pos=None,
               bag_fraction=1.0, thin=1, move="stretch", gamma0=None, sigma=1e-5):
        """The bagged posterior ("BayesBag": Huggins & Miller 2019, 2023): ``n_bags`` posteriors of the same model, bag b on
        the catalogue under the bootstrap weights of replicate b (``scheme`` "exponential": Exp(1), "poisson": Poisson(1)
        counts; the weights of ``bootstrap`` -- a function of (seed, b, star), ``_native.bootstrap_weights`` replays them),
        sampled in lock step and pooled.  B ensembles of ``n_walkers`` walkers take ``n_steps`` stretch-move steps
        (``BinnedSampler``, ``rng="device"``: the chains are a function of ``seed``); one launch of the weighted value
        kernel (``lnprob_weighted_batch``) evaluates all B W / 2 proposals of a half step, row (b, w) under replicate b.
        ``bag_fraction`` scales every bag's log-likelihood: the M / N of a bag of M stars drawn from N; 1.0 is the standard
        choice.  ``pos``: start positions (B, W, P), default B W rows of ``get_initials``.

        Returns ``bagged_summary`` of the chains -- the pooled moments are the bagged posterior, ``within`` / ``between`` /
        ``mismatch_ratio`` compare the model's own width with the sampling scatter (see there) -- plus ``sampler``
        (``chain``: (B, W, steps, P)), ``seed``, ``scheme`` and ``bag_fraction``.  Unlike every interval taken from one
        chain, the bagged intervals keep their coverage when the model understates the scatter of the data.
        ``move``, ``gamma0``, ``sigma``: the sampler's move (``BinnedSampler``: "stretch" or "de")."""
        self._holdout_check("bagged")
        from .binned import BinnedSampler
        n_b, n_w, n_p = int(n_bags), int(n_walkers), self.n_fitted_parameters
        if n_b < 1:
            raise ValueError("bagged: n_bags must be >= 1")
        if scheme not in ("exponential", "poisson"):
            raise ValueError("bagged: scheme must be 'exponential' or 'poisson'")
        if int(thin) < 1:
            raise ValueError("bagged: thin must be >= 1")
        if not 0 <= int(n_burn) < int(n_steps):
            raise ValueError("bagged: n_burn must lie in [0, n_steps)")
        if not (np.isfinite(bag_fraction) and bag_fraction > 0.0):
            raise ValueError("bagged: bag_fraction must be positive")
        if seed is None:
            seed = int(np.random.SeedSequence().entropy % (2 ** 63))
        if pos is None:
            pos = self.get_initials(n_b * n_w).reshape(n_b, n_w, n_p)
        pos = np.ascontiguousarray(pos, dtype=np.float64)
        if pos.shape != (n_b, n_w, n_p):
            raise ValueError("Array with starting values has invalid shape: expected {0}".format((n_b, n_w, n_p)))
        pars = self.parameters
        if not np.all(np.isfinite(pars.lnprior_batch(pars.resolve_batch(pos.reshape(-1, n_p))))):
            raise ValueError("Invalid initial guesses: start positions outside the prior")

        def log_prob(values):
            # (B, rows, P): bag b's rows under replicate b
            rep = np.repeat(np.arange(n_b, dtype=np.int64), values.shape[1])
            return self.lnprob_weighted_batch(values, rep, scheme=scheme, seed=seed, weight_scale=bag_fraction)

        sampler = BinnedSampler(n_b, n_w, n_p, log_prob, seed=seed, rng="device", move=move, gamma0=gamma0, sigma=sigma)
        logger.info("bagged posterior: %d bags (%s weights), %d walkers each, %d steps", n_b, scheme, n_w, n_steps)
        sampler.reserve(int(n_steps))
        sampler.run_mcmc(pos, int(n_steps))
        out = bagged_summary(sampler.chain, n_burn, self.fitted_parameters, thin=thin)
        out.update({"sampler": sampler, "seed": int(seed), "scheme": scheme, "bag_fraction": float(bag_fraction)})
        return out

    # ------------------------------------------------------------------ fits of simulated catalogues: SBC, recovery (new)
    def _proper_prior(self, who):
        """(plan, lo, hi, kind, p0, p1) over the free parameters of a fit whose prior can be sampled."""
        plan = self._plan()
        if not plan.simple:
            raise NotImplementedError("Runner.{0}: expr / lnprior-expression parameters have no prior to draw from".format(who))
        improper = self.improper_parameters()
        if improper:
            raise ValueError("Runner.{0}: the prior of {1} is improper (give two finite bounds, or a normal / log-normal "
                             "prior)".format(who, ", ".join(improper)))
        n_p = plan.free_idx.size
        kind, p0, p1 = (np.zeros(n_p, dtype=np.int32), np.zeros(n_p), np.ones(n_p)) if plan.prior is None else \
            (np.asarray(a) for a in plan.prior)
        return plan, plan.lo[plan.free_idx], plan.hi[plan.free_idx], kind, p0, p1

    def _prior_quantile(self, u, who):
        """u (n, P) in (0, 1) -> the prior's quantiles: the inverse CDF of every free parameter's prior, truncated to its box."""
        from scipy.special import ndtr, ndtri
        _, lo, hi, kind, p0, p1 = self._proper_prior(who)
        u = np.asarray(u, dtype=np.float64)
        out = np.empty_like(u)
        for j in range(u.shape[1]):
            if kind[j] == _native.PRIOR_FLAT:
                x = lo[j] + u[:, j] * (hi[j] - lo[j])
            else:
                log = kind[j] == _native.PRIOR_LOGNORMAL
                with np.errstate(divide="ignore"):
                    a, b = (np.log(max(lo[j], 0.0)), np.log(hi[j])) if log else (lo[j], hi[j])
                ca, cb = ndtr((a - p0[j]) / p1[j]), ndtr((b - p0[j]) / p1[j])
                x = p0[j] + p1[j] * ndtri(ca + u[:, j] * (cb - ca))
                x = np.exp(x) if log else x
            out[:, j] = np.clip(x, lo[j], hi[j])
        return out

    def sample_prior(self, n, seed=None):
        """``n`` draws from the prior itself, (n, P) free-parameter vectors: a finite box gives a uniform draw, a normal or
        log-normal prior is truncated to its box by inverse CDF.  Host NumPy, a function of ``seed``.  ValueError, naming
        ``improper_parameters()``, when a free parameter has no proper prior; NotImplementedError for ``expr`` /
        ``lnprior``-expression parameters."""
        n_p = self._proper_prior("sample_prior")[0].free_idx.size
        rng = np.random.default_rng(seed)
        # (the open interval: ndtri(0) is -inf)
        u = (rng.integers(0, 1 << 53, size=(int(n), n_p)).astype(np.float64) + 0.5) * 2.0 ** -53
        return self._prior_quantile(u, "sample_prior")

    def prior_variance(self, n_nodes=1 << 16):
        """(P,) variances of the free parameters' priors, by the midpoint rule on ``n_nodes`` quantiles."""
        n_p = self._proper_prior("prior_variance")[0].free_idx.size
        u = np.repeat(((np.arange(int(n_nodes)) + 0.5) / int(n_nodes))[:, None], n_p, axis=1)
        return self._prior_quantile(u, "prior_variance").var(axis=0)

    def _simulated_background(self):
        try:
            return self._replicate_background()
        except NotImplementedError as exc:
            raise NotImplementedError(str(exc).replace("Runner.replicate_check", "Runner.simulate"))

    def _truth_table(self, truths, who):
        """truths (E, P) free-parameter vectors inside the prior -> ((E, P) array, the resolved parameter columns)."""
        n_p = self.n_fitted_parameters
        truths = np.atleast_2d(np.asarray(truths, dtype=np.float64))
        if truths.ndim != 2 or truths.shape[1] != n_p:
            raise ValueError("{0}: truths must have shape (E, {1})".format(who, n_p))
        pars = self.parameters
        resolved = pars.resolve_batch(truths)
        if not np.all(np.isfinite(pars.lnprior_batch(resolved))):
            raise ValueError("{0}: a truth row lies outside the prior".format(who))
        return truths, resolved

    def simulate(self, truths, seed, sim0=0):
        """Simulated catalogues: ``truths`` (E, P) free-parameter vectors -> (E, n_data) velocities in km/s, catalogue e
        drawn on the device from the model at truths[e], on the observed positions and velocity errors (simulation id
        ``sim0 + e``; a velocity is a function of (seed, id, star, truth) alone and ``_native.replicate_numbers`` replays
        its random numbers).  The set stays resident on the device for ``lnprob_simulated_batch``.  Fixed-background
        classes draw background stars from their ``background.Gaussian``."""
        self._holdout_check("simulate")
        _, resolved = self._truth_table(truths, "simulate")
        bg = self._simulated_background()
        cat = self._ensure_catalog()
        return cat.simulate(self._kernel_table(resolved), seed, sim0=sim0, bg_mean=bg[0], bg_sigma=bg[1])

    def simulated_set(self, velocities):
        """Make the caller's own mock velocities (E, n_data), in km/s, the resident set of ``lnprob_simulated_batch``."""
        self._holdout_check("simulated_set")
        bg = self._simulated_background()
        velocities = np.atleast_2d(np.asarray(velocities, dtype=np.float64))
        self._ensure_catalog().simulated_set(velocities, bg_mean=bg[0], bg_sigma=bg[1])
        return velocities

    def lnprob_simulated_batch(self, values, row_sim):
        """``lnprob_batch`` with every row evaluated on the velocities of its own simulation: ``values`` (..., P)
        free-parameter vectors and ``row_sim``, one simulation id of the resident set (``simulate``, ``simulated_set``) per
        row in C order, -> (...) values of  sum_i lnL_i(v' of the row's simulation) + ln prior,  one launch of the device's
        simulated VALUE kernel (``_native.Catalog.simulated_loglike``).  Box and structured priors as in ``lnprob_batch``:
        rows outside the prior are -inf and take a donor row for the launch.  Runs on one device in one process, on
        un-binned float64 catalogues."""
        self._holdout_check("lnprob_simulated_batch")
        values = np.asarray(values, dtype=np.float64)
        n_p = self.n_fitted_parameters
        if values.ndim < 1 or values.shape[-1] != n_p:
            raise ValueError("values must have shape (..., {0})".format(n_p))
        lead = values.shape[:-1]
        sim = np.ascontiguousarray(row_sim, dtype=np.int64).reshape(-1)
        rows = values.reshape(-1, n_p)
        if sim.size != rows.shape[0]:
            raise ValueError("row_sim must hold one simulation per row of values")
        pars = self.parameters
        resolved = pars.resolve_batch(rows)
        lp = pars.lnprior_batch(resolved)
        ok = np.isfinite(lp)
        out = np.full(lp.shape, -np.inf)
        if ok.any():
            if not ok.all():
                donor = int(np.flatnonzero(ok)[0])
                resolved = OrderedDict((k, np.where(ok, col, col[donor])) for k, col in resolved.items())
            lnl = self._ensure_catalog().simulated_loglike(self._kernel_table(resolved), sim)
            out[ok] = lnl[ok] + lp[ok]
        return out.reshape(lead)

    def _simulated_start(self, truths, n_walkers, seed):
        """(E, W, P) start positions: a ball about each truth, truth + 0.01 x prior scale x normal, redrawn until inside
        the prior.  The prior scale: the width of a finite box, the scale of a normal prior, s x truth of a log-normal one,
        max(|truth|, 1) where there is neither."""
        plan = self._plan()
        lo, hi = plan.lo[plan.free_idx], plan.hi[plan.free_idx]
        n_e, n_p = truths.shape
        scale = np.where(np.isfinite(hi - lo), hi - lo, np.maximum(np.abs(truths), 1.0))
        scale = np.broadcast_to(scale, truths.shape).copy()
        if plan.prior is not None:
            kind, _, p1 = (np.asarray(a) for a in plan.prior)
            scale[:, kind == _native.PRIOR_NORMAL] = p1[kind == _native.PRIOR_NORMAL]
            log = kind == _native.PRIOR_LOGNORMAL
            scale[:, log] = p1[log] * np.maximum(np.abs(truths[:, log]), 1e-300)
        rng = np.random.default_rng([int(seed) & 0xFFFFFFFFFFFFFFFF, 0x73696D])
        pars = self.parameters
        pos = truths[:, None, :] + 0.01 * scale[:, None, :] * rng.normal(size=(n_e, n_walkers, n_p))
        for _ in range(100):
            bad = ~np.isfinite(pars.lnprior_batch(pars.resolve_batch(pos.reshape(-1, n_p)))).reshape(n_e, n_walkers)
            if not bad.any():
                return pos
            e, _w = np.nonzero(bad)
            pos[bad] = truths[e] + 0.01 * scale[e] * rng.normal(size=(int(bad.sum()), n_p))
        raise ValueError("simulated_fits: no start positions inside the prior around a truth (it sits on a bound)")

    def simulated_fits(self, truths, n_walkers=64, n_steps=600, n_burn=200, seed=None, velocities=None, pos=None, thin=1,
                       move="stretch", gamma0=None, sigma=1e-5):
        """Fit E simulated catalogues in lock step: catalogue e is drawn from the model at ``truths[e]`` (``simulate``), or is
        row e of the caller's ``velocities`` (E, n_data) in km/s (``simulated_set``).  E ensembles of ``n_walkers`` walkers
        take ``n_steps`` stretch-move steps (``BinnedSampler``, ``rng="device"``: the chains are a function of ``seed``);
        one launch of the simulated value kernel (``lnprob_simulated_batch``) evaluates all E W / 2 proposals of a half
        step, row (e, w) on simulation e.  ``pos``: start positions (E, W, P), default a small ball about each truth.
        The velocities and the chains take the one ``seed``; their generators have different keys.

        Returns ``simulated_fit_summary`` of the chains (per fit: ``mean``, ``std``, ``percentiles``, ``tau``, ``converged``,
        ``z`` = (mean - truth) / std) plus ``truths``, ``velocities``, ``sampler`` (``chain``: (E, W, steps, P)) and
        ``seed``.  ``move``, ``gamma0``, ``sigma``: the sampler's move (``BinnedSampler``: "stretch" or "de")."""
        self._holdout_check("simulated_fits")
        from .binned import BinnedSampler
        n_w, n_p = int(n_walkers), self.n_fitted_parameters
        if int(thin) < 1:
            raise ValueError("simulated_fits: thin must be >= 1")
        if not 0 <= int(n_burn) < int(n_steps):
            raise ValueError("simulated_fits: n_burn must lie in [0, n_steps)")
        if seed is None:
            seed = int(np.random.SeedSequence().entropy % (2 ** 63))
        truths, _ = self._truth_table(truths, "simulated_fits")
        n_e = truths.shape[0]
        if velocities is None:
            velocities = self.simulate(truths, seed)
        else:
            velocities = np.atleast_2d(np.asarray(velocities, dtype=np.float64))
            if velocities.shape != (n_e, self.n_data):
                raise ValueError("simulated_fits: velocities must have shape {0}".format((n_e, self.n_data)))
            velocities = self.simulated_set(velocities)
        if pos is None:
            pos = self._simulated_start(truths, n_w, seed)
        pos = np.ascontiguousarray(pos, dtype=np.float64)
        if pos.shape != (n_e, n_w, n_p):
            raise ValueError("Array with starting values has invalid shape: expected {0}".format((n_e, n_w, n_p)))
        pars = self.parameters
        if not np.all(np.isfinite(pars.lnprior_batch(pars.resolve_batch(pos.reshape(-1, n_p))))):
            raise ValueError("Invalid initial guesses: start positions outside the prior")

        def log_prob(values):
            # (E, rows, P): the rows of ensemble e on simulation e
            return self.lnprob_simulated_batch(values, np.repeat(np.arange(n_e, dtype=np.int64), values.shape[1]))

        sampler = BinnedSampler(n_e, n_w, n_p, log_prob, seed=seed, rng="device", move=move, gamma0=gamma0, sigma=sigma)
        logger.info("simulated fits: %d catalogues, %d walkers each, %d steps", n_e, n_w, n_steps)
        sampler.reserve(int(n_steps))
        sampler.run_mcmc(pos, int(n_steps))
        out = simulated_fit_summary(sampler.chain, n_burn, truths, thin=thin)
        out.update({"truths": truths, "velocities": velocities, "sampler": sampler, "seed": int(seed),
                    "names": list(self.fitted_parameters)})
        return out

    def sbc(self, n_sims=256, n_walkers=32, n_steps=600, n_burn=200, seed=None, n_bins=8, thin=None, truths=None, move="stretch", gamma0=None, sigma=1e-5):
        """Simulation-based calibration of this fit: ``n_sims`` truths drawn from the prior (``sample_prior(n_sims, seed)``;
        or the caller's ``truths``), one simulated catalogue each, all fitted in lock step (``simulated_fits``), and the
        rank statistics of ``sbc_summary`` (``thin`` = None: the largest autocorrelation time).  Returns that summary plus
        ``fits`` (what ``simulated_fits`` returned), ``truths``, ``names`` and ``seed``."""
        if seed is None:
            seed = int(np.random.SeedSequence().entropy % (2 ** 63))
        if truths is None:
            truths = self.sample_prior(int(n_sims), seed=seed)
        fits = self.simulated_fits(truths, n_walkers=n_walkers, n_steps=n_steps, n_burn=n_burn, seed=seed, move=move, gamma0=gamma0, sigma=sigma)
        try:
            prior_variance = self.prior_variance()
        except (ValueError, NotImplementedError):
            prior_variance = None
        out = sbc_summary(fits["sampler"].chain, fits["truths"], n_burn, thin=thin, n_bins=n_bins, prior_variance=prior_variance)
        out.update({"fits": fits, "truths": fits["truths"], "names": fits["names"], "seed": int(seed)})
        return out

    def recovery(self, truth, n_sims=64, n_walkers=32, n_steps=600, n_burn=200, seed=None, thin=1, functions=None, null=None,
                 move="stretch", gamma0=None, sigma=1e-5):
        """Injection-recovery: ``n_sims`` catalogues simulated at the one ``truth`` (P,) -- or at every row of a grid (G, P),
        ``n_sims`` each -- on the data's positions and velocity errors, fitted in lock step (``simulated_fits``), and
        ``recovery_summary`` per truth: bias, scatter, interval coverage, z scores, and for every entry of ``functions`` the
        same plus ``exceeds``, the share of fits whose 2.5 % quantile of the function lies above its value at the
        parameter row ``null`` (the detection rate).  Returns the summary of a single truth, or ``{"grid": [summary per
        row]}`` for a grid; both carry ``fits`` and ``seed``."""
        truth = np.asarray(truth, dtype=np.float64)
        grid = np.atleast_2d(truth)
        n_s = int(n_sims)
        if n_s < 1:
            raise ValueError("recovery: n_sims must be >= 1")
        if seed is None:
            seed = int(np.random.SeedSequence().entropy % (2 ** 63))
        fits = self.simulated_fits(np.repeat(grid, n_s, axis=0), n_walkers=n_walkers, n_steps=n_steps, n_burn=n_burn, seed=seed, move=move, gamma0=gamma0, sigma=sigma)
        chain = fits["sampler"].chain
        per = [recovery_summary(chain[g * n_s:(g + 1) * n_s], grid[g], n_burn, fits["names"], thin=thin, functions=functions,
                                null=null) for g in range(grid.shape[0])]
        out = dict(per[0]) if truth.ndim == 1 else {"grid": per}
        out.update({"fits": fits, "seed": int(seed)})
        return out

    # ------------------------------------------------------------------ MAP fits of simulated catalogues (new)
    def simulated_sims(self):
        """Simulations of the set resident on the device (``simulate``, ``simulated_set``), 0 when there is none."""
        self._holdout_check("simulated_sims")
        return self._ensure_catalog().simulated_sims

    def lnprob_simulated_grad_batch(self, values, row_sim):
        """``lnprob_grad_batch`` with every row evaluated on the velocities of its own simulation: (R, P) free-parameter
        vectors and ``row_sim`` (R,), one simulation id of the resident set per row, -> ((R,) values, (R, P) gradients) of
        sum_i lnL_i(v' of the row's simulation) + ln prior,  one launch of the device's simulated value-and-gradient kernel
        (``_native.Catalog.simulated_loglike_grad``).  The chain rule, the prior handling, the donor rows and the refusals
        are ``lnprob_grad_batch``'s.  Runs on one device in one process, on un-binned float64 catalogues."""
        self._holdout_check("lnprob_simulated_grad_batch")
        values = np.atleast_2d(np.asarray(values, dtype=np.float64))
        sim = np.ascontiguousarray(row_sim, dtype=np.int64).reshape(-1)
        if sim.size != values.shape[0]:
            raise ValueError("row_sim must hold one simulation per row of values")
        plan = self._grad_plan()

        def lnlike_grad(rows):
            return self._lnlike_grad_rows(rows, lambda cat, table: cat.simulated_loglike_grad(table, sim))
        if plan.prior is None:
            return lnlike_grad(values)
        return self._lnprob_grad_rows(values, plan, lnlike_grad)

    def _inside_box(self, x, plan):
        """x clipped strictly inside the box of the free parameters: 1e-6 of a finite width (of max(|bound|, 1) on a
        one-sided one) away from every bound."""
        lo, hi = plan.lo[plan.free_idx], plan.hi[plan.free_idx]
        room = 1e-6 * np.where(np.isfinite(hi - lo), hi - lo,
                               np.maximum(np.where(np.isfinite(lo), np.abs(lo), 0.0), np.where(np.isfinite(hi), np.abs(hi), 0.0)) + 1.0)
        return np.clip(x, lo + room, hi - room)

    def simulated_maximize(self, truths=None, velocities=None, seed=None, x0=None, max_iter=200, gtol=1e-8):
        """MAP fits of E simulated catalogues in lock step: catalogue e is drawn from the model at ``truths[e]``
        (``simulate(truths, seed)``), or is row e of the caller's ``velocities`` (E, n_data) in km/s (``simulated_set``); with
        neither, the set already resident on the device is fitted.  ``x0``: the starts, (P,) for all, (E, P) one per
        catalogue, or (E, S, P) S per catalogue; default the truths, clipped strictly inside the box.  All E S rows climb
        ``lnprob_simulated_grad_batch`` in ONE ``optimize.maximize_batch`` run, row (e, s) on simulation e: one launch of
        the simulated value-and-gradient kernel per trial step.  Per catalogue the best converged start wins (the best of
        all where none converged).

        Returns ``x`` (E, P), ``lnprob`` (E,), ``converged`` (E,), ``n_iter`` (E,) of the winning starts, ``all_x`` (E, S, P),
        ``all_lnprob`` (E, S), ``all_converged`` (E, S), ``names``, ``seed`` and, when they were drawn here, ``velocities``.
        A few dozen launches per fit where ``simulated_fits`` takes two per step of a chain."""
        from ..optimize import maximize_batch
        self._holdout_check("simulated_maximize")
        plan = self._grad_plan()
        n_p = plan.free_idx.size
        out = {}
        if truths is not None:
            truths, _ = self._truth_table(truths, "simulated_maximize")
        if velocities is not None:
            velocities = np.atleast_2d(np.asarray(velocities, dtype=np.float64))
            if velocities.ndim != 2 or velocities.shape[1] != self.n_data or \
                    (truths is not None and velocities.shape[0] != truths.shape[0]):
                raise ValueError("simulated_maximize: velocities must have shape (E, {0})".format(self.n_data))
            self.simulated_set(velocities)
            n_e = velocities.shape[0]
        elif truths is not None:
            if seed is None:
                seed = int(np.random.SeedSequence().entropy % (2 ** 63))
            out["velocities"] = self.simulate(truths, seed)
            n_e = truths.shape[0]
        else:
            n_e = int(self.simulated_sims())
            if n_e < 1:
                raise ValueError("simulated_maximize: no simulated set is resident (give truths or velocities)")
        if x0 is None:
            if truths is None:
                raise ValueError("simulated_maximize: x0 is needed where there are no truths to start from")
            x0 = self._inside_box(truths, plan)
        x0 = np.asarray(x0, dtype=np.float64)
        if x0.ndim == 1:
            x0 = np.broadcast_to(x0, (n_e, 1, x0.size))
        elif x0.ndim == 2:
            x0 = x0[:, None, :]
        if x0.ndim != 3 or x0.shape[0] != n_e or x0.shape[1] < 1 or x0.shape[2] != n_p:
            raise ValueError("simulated_maximize: x0 must have shape ({1},), ({0}, {1}) or ({0}, S, {1})".format(n_e, n_p))
        n_s = x0.shape[1]
        sim = np.repeat(np.arange(n_e, dtype=np.int64), n_s)
        lo, hi = plan.lo[plan.free_idx], plan.hi[plan.free_idx]
        logger.info("simulated MAP fits: %d catalogues, %d start(s) each", n_e, n_s)
        res = maximize_batch(lambda x: self.lnprob_simulated_grad_batch(x, sim), np.ascontiguousarray(x0).reshape(n_e * n_s, n_p),
                             lo, hi, max_iter=max_iter, gtol=gtol)
        f = np.where(np.isfinite(res["f"]), res["f"], -np.inf).reshape(n_e, n_s)
        conv = np.asarray(res["converged"], dtype=bool).reshape(n_e, n_s)
        # per catalogue the best converged start, or the best of all where none converged
        pool = np.where(conv.any(axis=1)[:, None], conv, True)
        best = np.argmax(np.where(pool, f, -np.inf), axis=1)
        rows = np.arange(n_e)
        all_x = res["x"].reshape(n_e, n_s, n_p)
        out.update({"x": all_x[rows, best].copy(), "lnprob": f[rows, best].copy(), "converged": conv[rows, best].copy(),
                    "n_iter": np.asarray(res["n_iter"]).reshape(n_e, n_s)[rows, best].copy(), "all_x": all_x, "all_lnprob": f,
                    "all_converged": conv, "names": list(self.fitted_parameters), "seed": None if seed is None else int(seed)})
        return out

    def parametric_bootstrap(self, n_sims=256, x_hat=None, seed=None, max_iter=200, gtol=1e-8):
        """Parametric bootstrap of the maximum (Efron & Tibshirani 1993, ch. 6): ``n_sims`` catalogues simulated from the
        model at ``x_hat`` (default: ``maximize()["x"]``) on the data's positions and velocity errors, each refitted from
        ``x_hat`` (``simulated_maximize``: one lock-stepped run), and ``parametric_bootstrap_summary`` of the refits: the bias
        and the covariance of the estimator UNDER THE FITTED MODEL, with ``std_ratio`` against ``laplace(x_hat)`` where that
        exists.  ``bootstrap()`` gives the same moments without the model (resampled stars); the ratio of the two ``std``
        tells whether the model describes the scatter of the data.  ``covariance`` is accepted wherever
        ``laplace()["covariance"]`` is.  Also returns ``x`` (E, P), ``converged``, ``n_iter``, ``lnprob``, ``x_hat``, ``seed``."""
        self._holdout_check("parametric_bootstrap")
        plan = self._grad_plan()
        n_e = int(n_sims)
        if n_e < 1:
            raise ValueError("parametric_bootstrap: n_sims must be >= 1")
        if seed is None:
            seed = int(np.random.SeedSequence().entropy % (2 ** 63))
        x_hat = self.maximize(max_iter=max_iter, gtol=gtol)["x"] if x_hat is None else \
            np.asarray(x_hat, dtype=np.float64).reshape(-1)
        if x_hat.size != plan.free_idx.size:
            raise ValueError("parametric_bootstrap: x_hat must hold the {0} free parameters".format(plan.free_idx.size))
        fits = self.simulated_maximize(np.tile(x_hat, (n_e, 1)), seed=seed, x0=self._inside_box(x_hat, plan), max_iter=max_iter,
                                       gtol=gtol)
        try:
            laplace = self.laplace(x_hat)["covariance"]
        except ValueError:
            laplace = None
        out = parametric_bootstrap_summary(fits["x"], x_hat, fits["converged"], fits["names"], laplace)
        out.update({"x": fits["x"], "converged": fits["converged"], "n_iter": fits["n_iter"], "lnprob": fits["lnprob"],
                    "x_hat": x_hat, "seed": int(seed)})
        return out

    def _lrt_embedding(self, null):
        """What makes ``null`` a sub-model of this fit: (positions of null's free parameters among this fit's free ones,
        positions of the others, null's fixed values there), or ValueError with the reason."""
        if type(null) is not type(self):
            raise ValueError("lrt: the null fit is a {0}, this one a {1}".format(type(null).__name__, type(self).__name__))
        if null.n_data != self.n_data:
            raise ValueError("lrt: the null fit has {0} stars, this one {1}".format(null.n_data, self.n_data))
        for col in list(self.OBSERVABLES) + ["pmember", "lnlike_background"]:
            a, b = getattr(self, col, None), getattr(null, col, None)
            if (a is None) != (b is None) or (a is not None and not np.array_equal(np.asarray(a), np.asarray(b))):
                raise ValueError("lrt: the null fit's data column '{0}' differs from this fit's".format(col))
        free, free0 = list(self.fitted_parameters), list(null.fitted_parameters)
        for name in free0:
            if name not in free:
                raise ValueError("lrt: '{0}' is free in the null fit but not in this one (the models are not nested)".format(name))
        if len(free0) == len(free):
            raise ValueError("lrt: the null fit fixes no parameter that is free here")
        plan = self._grad_plan()
        lo, hi = plan.lo[plan.free_idx], plan.hi[plan.free_idx]
        extra = [j for j, name in enumerate(free) if name not in free0]
        fixed = np.array([float(null.parameters[free[j]]._value) for j in extra])
        for j, val in zip(extra, fixed):
            if not lo[j] <= val <= hi[j]:
                raise ValueError("lrt: the null fit fixes '{0}' at {1}, outside this fit's box [{2}, {3}]".format(
                    free[j], val, lo[j], hi[j]))
        for name, par in self.parameters.items():
            if par.fixed and par._expr is None and float(par._value) != float(null.parameters[name]._value):
                raise ValueError("lrt: '{0}' is fixed at {1} here and at {2} in the null fit".format(
                    name, float(par._value), float(null.parameters[name]._value)))
        return np.array([free.index(name) for name in free0], dtype=np.intp), np.array(extra, dtype=np.intp), fixed

    def lrt(self, null, n_sims=1024, seed=None, max_iter=200, gtol=1e-8):
        """Likelihood-ratio test of this fit against the nested fit ``null`` -- the same class on the same stars, its free
        parameters a subset of this fit's and the others fixed (rotation amplitudes at zero: "does the cluster rotate?")
        -- with the null distribution of the statistic SIMULATED at the data's own positions and velocity errors (a
        parametric bootstrap of the test, Davison & Hinkley 1997 ch. 4), because Wilks' chi2 is not to be trusted with a
        few hundred stars, a background mixture or a parameter near a bound.

        x0 = ``null.maximize()``, x1 = ``self.maximize()``, ``stat_obs`` = 2 (lnprob1 - lnprob0); ``n_sims`` catalogues are
        drawn from the null at x0 (``null.simulate``) and handed to this fit (``simulated_set``); the null refits them
        from x0 and this fit from two starts each -- x0 embedded (the null's fixed values in the other coordinates), so
        that the full fit starts where the null ends and the statistic cannot be negative, and x1 -- by
        ``simulated_maximize``.  Returns ``lrt_summary`` (``stat``, ``used``, ``p_value``, ``p_se``, ``df``,
        ``p_asymptotic``, ``quantiles``, ``n_negative``) plus ``x_null``, ``x_full``, ``lnprob_null``, ``lnprob_full``,
        ``fits_null``, ``fits_full``, ``tolerance`` and ``seed``.  ValueError, with the reason, when ``null`` is not a
        sub-model of this fit."""
        self._holdout_check("lrt")
        if not isinstance(null, Runner):
            raise ValueError("lrt: null must be a fit of the same class on the same stars")
        shared, extra, fixed = self._lrt_embedding(null)
        n_e = int(n_sims)
        if n_e < 1:
            raise ValueError("lrt: n_sims must be >= 1")
        if seed is None:
            seed = int(np.random.SeedSequence().entropy % (2 ** 63))
        plan = self._grad_plan()
        fit0 = null.maximize(max_iter=max_iter, gtol=gtol)
        fit1 = self.maximize(max_iter=max_iter, gtol=gtol)
        x0, x1 = fit0["x"], fit1["x"]
        embedded = np.empty(plan.free_idx.size)
        embedded[shared], embedded[extra] = x0, fixed
        lnprob1 = float(fit1["lnprob"])
        stat_obs = 2.0 * (lnprob1 - float(fit0["lnprob"]))
        vel = null.simulate(np.tile(x0, (n_e, 1)), seed)
        fits_null = null.simulated_maximize(x0=null._inside_box(x0, null._grad_plan()), max_iter=max_iter, gtol=gtol)
        self.simulated_set(vel)
        starts = np.stack([self._inside_box(embedded, plan), self._inside_box(x1, plan)])
        fits_full = self.simulated_maximize(x0=np.broadcast_to(starts, (n_e,) + starts.shape), max_iter=max_iter, gtol=gtol)
        scale = max(float(np.max(np.abs(fits_null["lnprob"]))), float(np.max(np.abs(fits_full["lnprob"]))), float(self.n_data))
        tolerance = 4e-12 * scale
        out = lrt_summary(fits_null["lnprob"], fits_full["lnprob"], fits_null["converged"], fits_full["converged"], stat_obs,
                          len(extra), tolerance=tolerance)
        out.update({"x_null": x0, "x_full": x1, "lnprob_null": float(fit0["lnprob"]), "lnprob_full": lnprob1,
                    "fits_null": fits_null, "fits_full": fits_full, "velocities": vel, "tolerance": tolerance, "seed": int(seed)})
        return out

    # ------------------------------------------------------------------ Hamiltonian Monte Carlo (new)
    HMC_TARGET_ACCEPT = 0.8

    def _hmc_block(self, pos, lnp, chol, step_size, n_leap, jitter, seed, step0, n_steps, chain, lnprob_chain, accepted,
                   energy_error):
        """One block of HMC steps inside the library (``_native.Catalog.hmc_block``)."""
        self._stretch_catalog(pos).hmc_block(self._stretch_plan(), chol, step_size, n_leap, pos, lnp, seed, step0, n_steps,
                                             chain, lnprob_chain, accepted, energy_error, jitter=jitter)

    # the resident HMC and tempering blocks hold a walker's coordinates in registers (csrc/mcd_hmc.h: kHmcMaxDim,
    # csrc/mcd_temper.h: kTemperMaxDim)
    RESIDENT_MAX_DIM = 12

    def _check_resident_dim(self, what, n_p):
        if n_p > self.RESIDENT_MAX_DIM:
            raise NotImplementedError("Runner.{0}: {1} free parameters, the resident blocks take at most {2} (fix some, e.g. "
                                      "the centre; the stretch move has no such limit)".format(what, n_p, self.RESIDENT_MAX_DIM))

    def hmc(self, n_walkers=64, n_steps=500, pos=None, covariance=None, step_size=None, n_leap=8, n_warmup=None, seed=None,
            jitter=0.1, warmup_block=10):
        """Sample the posterior with Hamiltonian Monte Carlo on the device gradient (``sampler.HMCSampler``; csrc/mcd_hmc.h):
        ``n_walkers`` independent chains of ``n_steps`` steps of ``n_leap`` leapfrog points each, after ``n_warmup`` steps
        (default ``min(200, n_steps // 2)``) that are not kept.  Returns the sampler; its chain holds the ``n_steps`` steps.

        ``covariance`` (P, P) defines the metric: its lower Cholesky factor is the factor of the inverse mass matrix.  When
        ``pos`` or ``covariance`` is None, ``maximize`` + ``laplace`` supply the covariance and ``get_initials_laplace`` the
        start positions; when ``laplace`` raises (the maximum sits on a bound, or -H is not positive definite there) the
        metric falls back to a DIAGONAL one, (prior width / 10)^2 or (max(|x|, 1) / 10)^2 for an unbounded parameter, with
        a warning.  A diagonal metric reflects at the prior box, a dense one rejects trajectories that leave it.

        Step size: ``step_size`` or, by default, ``1.5 * P ** -0.25`` in the units of the metric (a leapfrog step in a
        well-estimated metric is stable below 2 and the optimal step shrinks as P^(-1/4), Neal 2011).  During warm-up the
        step size is adapted BETWEEN blocks of ``warmup_block`` steps by a plain multiplicative rule on the host,
        ``eps *= exp(acceptance of the block - HMC_TARGET_ACCEPT)``: a block that accepts everything grows eps by 22 %, one
        that accepts nothing shrinks it by 55 %, and the rule is stationary at an acceptance of 0.8.  After warm-up eps
        is frozen (``sampler.step_size``; the adaptation's path is in ``sampler.warmup_step_sizes``).

        Structured priors (``Parameter.prior``) are part of the target: the potential is -(lnlike + lnprior), on the device.
        ``expr`` / ``lnprior``-expression parameters and binned or non-float64 catalogues raise NotImplementedError: the
        gradient's own limits."""
        plan = self._grad_plan()
        self._check_resident_dim("hmc", int(plan.free_idx.size))
        ok, why_not = self.resident_ok()
        if not ok:
            raise NotImplementedError("Runner.hmc: " + why_not)
        if self._precision != "f64":
            raise NotImplementedError("Runner.hmc: gradients need a float64 catalogue")
        n_p = int(plan.free_idx.size)
        lo, hi = plan.lo[plan.free_idx], plan.hi[plan.free_idx]
        x_map = None
        if covariance is None:
            x_map = self.maximize()["x"]
            try:
                covariance = self.laplace(x_map)["covariance"]
            except ValueError as exc:
                width = np.where(np.isfinite(hi - lo), hi - lo, np.maximum(np.abs(x_map), 1.0))
                covariance = np.diag((width / 10.0) ** 2)
                warnings.warn("Runner.hmc: no Laplace covariance ({0}); using a diagonal metric from the prior widths".format(exc))
        covariance = np.asarray(covariance, dtype=np.float64)
        if covariance.shape != (n_p, n_p):
            raise ValueError("covariance must have shape ({0}, {0})".format(n_p))
        chol = np.linalg.cholesky(covariance)
        if pos is None:
            if x_map is None:
                x_map = self.maximize()["x"]
            pos = self.get_initials_laplace(n_walkers, x_map, covariance)
        pos = np.ascontiguousarray(pos, dtype=np.float64)
        if pos.shape != (n_walkers, n_p):
            raise ValueError("Array with starting values has invalid shape.")
        if np.any(pos < lo) or np.any(pos > hi):
            raise ValueError("Runner.hmc: a start position lies outside the prior box")
        from ..sampler import HMCSampler
        eps = float(step_size) if step_size is not None else 1.5 * n_p ** -0.25
        sampler = HMCSampler(n_walkers, n_p, self._hmc_block, chol, eps, n_leap=n_leap, jitter=jitter, seed=seed)
        n_warmup = min(200, int(n_steps) // 2) if n_warmup is None else int(n_warmup)
        logger.info("MCMC driver: Hamiltonian Monte Carlo, %d chains, %d leapfrog points per step, %d warm-up steps",
                    n_walkers, n_leap, n_warmup)
        sampler.warmup_step_sizes = [sampler.step_size]
        done = 0
        while done < n_warmup:
            n = min(max(1, int(warmup_block)), n_warmup - done)
            before = sampler._accepted.sum()
            pos, _, _ = sampler.run_mcmc(pos, n)
            rate = float(sampler._accepted.sum() - before) / (n * n_walkers)
            sampler.step_size *= float(np.exp(rate - self.HMC_TARGET_ACCEPT))
            sampler.warmup_step_sizes.append(sampler.step_size)
            done += n
        # (reset() leaves the generator's step counter ``rng_step`` alone -- as every sampler of mcmc_dynamics_amd.sampler and
        # analysis.binned does: the run below never replays the warm-up's numbers)
        sampler.reset()
        sampler.reserve(n_steps)
        sampler.run_mcmc(pos, n_steps)
        return sampler

    # ------------------------------------------------------------------ parallel tempering (new)
    def _temper_block(self, betas, pos, lnlike, lnprior, seed, step0, n_steps, chain, lnlike_chain, accepted, swap_proposed,
                      swap_accepted):
        """One block of parallel-tempering steps inside the library (``_native.Catalog.temper_block``)."""
        self._stretch_catalog(pos).temper_block(self._stretch_plan(), betas, pos, lnlike, lnprior, seed, step0, n_steps, chain,
                                                lnlike_chain, accepted, swap_proposed, swap_accepted)

    def _temper_lnlike(self, values):
        """(n, P) -> (n,) log-likelihoods through the PLAIN kernels (option ``fast_path`` = 0 for this evaluation, then
        back to what it was): what a tempered block evaluates with, so that the start of a run carries the same kernels'
        values as every later row of ``lnlikelihood``."""
        cat = self._stretch_catalog(values)
        found = cat.get_option("fast_path", 1)
        cat.set_option("fast_path", 0)
        try:
            return self.lnlike_batch(values)
        finally:
            cat.set_option("fast_path", found)

    def improper_parameters(self):
        """Names of the free parameters whose prior is improper: not two finite bounds and no normal / log-normal prior."""
        plan = self._plan()
        lo, hi = plan.lo[plan.free_idx], plan.hi[plan.free_idx]
        kind = np.zeros(plan.free_idx.size, dtype=np.int32) if plan.prior is None else np.asarray(plan.prior[0])
        return [plan.names[int(i)] for j, i in enumerate(plan.free_idx)
                if not (np.isfinite(lo[j]) and np.isfinite(hi[j])) and kind[j] == _native.PRIOR_FLAT]

    def tempered(self, n_temps=16, n_walkers=64, n_steps=500, betas=None, beta_ratio=0.5, pos=None, seed=None, store_temps=1):
        """Sample with parallel tempering (``sampler.TemperedSampler``; csrc/mcd_temper.h): ``n_temps`` ensembles of
        ``n_walkers`` walkers on a ladder of inverse temperatures, ``n_steps`` steps.  Returns the sampler: its ``chain`` is
        rung 0, the posterior; ``log_evidence(discard)`` the log marginal likelihood.  Burn-in is the caller's ``discard``.

        ``betas``: the ladder, or by default ``sampler.default_ladder(n_temps, beta_ratio, proper)`` -- geometric with ratio
        ``beta_ratio`` over ``n_temps - 1`` rungs and a final beta = 0 whenever the prior is proper (every free parameter
        has two finite bounds or a normal / log-normal prior); with an improper prior there is no zero rung, and
        ``log_evidence`` raises with the names of the unbounded parameters.  ``pos`` (W, P): the start of every rung,
        default ``get_initials``; its log-likelihood is evaluated with the plain kernels in the block's launch shape
        (``_temper_lnlike``).  ``store_temps``: positions are kept for that many rungs from 0.

        ``expr`` / ``lnprior``-expression parameters and binned or non-float64 catalogues raise NotImplementedError, as for
        ``hmc``."""
        plan = self._plan()
        self._check_resident_dim("tempered", int(plan.free_idx.size))
        ok, why_not = self.resident_ok()
        if not ok:
            raise NotImplementedError("Runner.tempered: " + why_not)
        if self._precision != "f64":
            raise NotImplementedError("Runner.tempered: tempered blocks need a float64 catalogue")
        from ..sampler import TemperedSampler, default_ladder
        improper = self.improper_parameters()
        if betas is None:
            betas = default_ladder(n_temps, beta_ratio, proper=not improper)
        n_p = int(plan.free_idx.size)
        pos = self.get_initials(n_walkers) if pos is None else pos
        pos = np.ascontiguousarray(pos, dtype=np.float64)
        if pos.shape != (n_walkers, n_p):
            raise ValueError("Array with starting values has invalid shape.")
        lnprior_fn = None
        if plan.prior is not None:
            prior = plan.prior
            lnprior_fn = lambda x: _native.prior_eval(prior, x)               # noqa: E731
        sampler = TemperedSampler(n_walkers, n_p, betas, self._temper_block, self._temper_lnlike, lnprior_fn=lnprior_fn,
                                  seed=seed, store_temps=store_temps, improper=improper)
        logger.info("MCMC driver: parallel tempering, %d rungs of %d walkers, beta %g .. %g", sampler.ntemps, n_walkers,
                    sampler.betas[0], sampler.betas[-1])
        sampler.reserve(n_steps)
        sampler.run_mcmc(pos, n_steps)
        return sampler

    # ------------------------------------------------------------------ several ranks (one process per GPU)
    RANK_CHECK_EVERY = 256

    def _rank_group(self):
        """Host group of a multi-rank context (``distributed.rank_context``), None for a single process."""
        ctx = self._context
        if ctx is None or getattr(ctx, "n_ranks", 1) <= 1:
            return None
        group = getattr(ctx, "host_group", None)
        if group is None:
            raise RuntimeError("this Runner sits on a multi-rank context without a host group: create the context with "
                               "mcmc_dynamics_amd.distributed.rank_context(), which keeps the group for the start-up hand-offs")
        return group

    def _check_ranks_agree(self, values):
        """The all-reduce at the end of every evaluation adds the ranks' partial sums row by row: it is only meaningful
        when every rank passes the SAME (W, P) table.  Verified on the first call and every RANK_CHECK_EVERY-th call
        (a CRC over the host group); a mismatch raises instead of producing a silently wrong chain."""
        n = getattr(self, "_n_rank_batches", 0)
        self._n_rank_batches = n + 1
        if n % self.RANK_CHECK_EVERY:
            return
        if not self._rank_group().same_everywhere(values):
            raise RuntimeError("the ranks of this job evaluate different walker tables: their partial log-likelihoods must not "
                               "be summed (seed every rank's sampler identically, e.g. through Runner.__call__)")

    # ------------------------------------------------------------------ sampler driver
    def get_initials(self, n_walkers):
        """Initial positions from each free parameter's ``initials`` recipe (runner.py:308-330)."""
        initials = np.zeros((n_walkers, self.n_fitted_parameters))
        i = 0
        for parameter in self.parameters.values():
            if parameter.fixed:
                continue
            initials[:, i] = parameter.evaluate_initials(n_walkers)
            i += 1
        return initials

    # Which sampler drives ``__call__``.  The reference hands ``Runner.lnprob`` to ``emcee.EnsembleSampler`` and lets emcee
    # drive the outer loop (runner.py:403, 416-419); so does this class whenever emcee can be imported:
    #   "auto" (default)  emcee (gets ``lnprob_batch`` with ``vectorize=True``) if importable, otherwise the built-in sampler
    #                     (``mcmc_dynamics_amd.sampler``: emcee's default move and attributes), with whole blocks of steps
    #                     inside the library where that is possible (see "resident");
    #   "emcee"           the real ``emcee.EnsembleSampler`` or ImportError;
    #   "resident"        the built-in sampler with the ensemble resident on the device (``mcd_stretch_move``: 87 - 95 % of
    #                     the kernel rate against ~60 % through one Python call per half step).  Needs box priors and the
    #                     package's own posterior methods (``resident_ok``); ValueError otherwise;
    #   "builtin"         never emcee: resident blocks where possible, else the built-in Python loop around ``lnprob_batch``.
    # One INFO line per run names the driver.
    SAMPLER = "auto"

    # methods that define the posterior: a sub-class that overrides one of them OUTSIDE this package (the reference's
    # Runner is meant to be sub-classed: its ``lnlike`` is a placeholder, runner.py:219-238) changes what emcee would
    # sample -- the library's block entry evaluates the built-in model and would silently ignore it
    _POSTERIOR_METHODS = ("lnprob", "lnprob_batch", "lnlike", "lnlike_batch", "_lnlike_batch", "lnprior", "lnprior_batch",
                          "fetch_parameter_values")

    def resident_ok(self):
        """(bool, reason): may whole blocks of steps run inside the library (``mcd_stretch_move``)?"""
        if not self.NATIVE_STRETCH:
            return False, "this class evaluates more than one un-binned catalogue per call (NATIVE_STRETCH is off)"
        for name in self._POSTERIOR_METHODS:
            fn = getattr(type(self), name, None)
            module = getattr(fn, "__module__", None) or ""
            if fn is not None and not module.startswith(__name__.rsplit(".", 2)[0] + "."):
                return False, "{0}.{1} overrides the posterior outside the package".format(type(self).__name__, name)
        if not self._plan().simple:
            return False, "the priors are not plain boxes with flat / normal / log-normal priors (expression priors / constrained parameters)"
        return True, ""

    MOVE = "stretch"               # the built-in sampler's move when ``__call__`` is not told one: "stretch" or "de"

    def _make_sampler(self, n_walkers, seed=None, move=None, gamma0=None, sigma=1e-5):
        if self.SAMPLER not in ("auto", "emcee", "resident", "builtin"):
            raise ValueError("Runner.SAMPLER must be 'auto', 'emcee', 'resident' or 'builtin'")
        move = move or self.MOVE
        resident, why_not = self.resident_ok()
        if self.SAMPLER == "resident" and not resident:
            raise ValueError("Runner.SAMPLER = 'resident' is not possible here: " + why_not)
        if move == "de":
            # the differential-evolution move (csrc/mcd_de.h) is the built-in sampler's: it runs whether or not emcee can be
            # imported, on the counter-based stream, resident where resident_ok() allows and in the NumPy loop otherwise
            from ..sampler import EnsembleSampler, default_gamma0
            if self._context is not None and getattr(self._context, "n_ranks", 1) > 1:
                raise NotImplementedError("move='de' on a multi-rank context: the collective resident DE block is not built")
            g0 = default_gamma0(self.n_fitted_parameters) if gamma0 is None else float(gamma0)
            logger.info("MCMC driver: built-in differential-evolution move (gamma0 = %.4g), %s", g0,
                        "blocks of steps inside the library, ensemble resident on the device" if resident
                        else "Python loop around lnprob_batch (" + why_not + ")")
            seeded = (lambda *block: self._de_block_seeded(g0, sigma, *block)) if resident else None
            return EnsembleSampler(n_walkers, self.n_fitted_parameters, self.lnprob_batch, vectorize=True, seed=seed,
                                   rng="device", seeded_block_fn=seeded, move="de", gamma0=g0, sigma=sigma)
        if move != "stretch":
            raise ValueError("move must be 'stretch' or 'de'")
        if self.SAMPLER in ("auto", "emcee"):
            try:
                import emcee
                sampler = emcee.EnsembleSampler(n_walkers, self.n_fitted_parameters, self.lnprob_batch, vectorize=True)
                if seed is not None:
                    sampler._random.seed(seed)
                logger.info("MCMC driver: emcee.EnsembleSampler around lnprob_batch (vectorize=True), as runner.py:403")
                return sampler
            except ImportError:
                if self.SAMPLER == "emcee":
                    raise
        from ..sampler import EnsembleSampler
        logger.info("MCMC driver: built-in stretch move (emcee's default move), %s",
                    "blocks of steps inside the library, ensemble resident on the device" if resident
                    else "Python loop around lnprob_batch (" + why_not + ")")
        if self.RNG not in ("host", "device"):
            raise ValueError("Runner.RNG must be 'host' or 'device'")
        return EnsembleSampler(n_walkers, self.n_fitted_parameters, self.lnprob_batch, vectorize=True, seed=seed,
                               block_fn=self._stretch_block if resident else None, rng=self.RNG,
                               seeded_block_fn=self._stretch_block_seeded if resident else None)

    # the built-in move's random numbers: "device" (default) -- the counter-based generator of csrc/mcd_rng.h, generated on
    # the device for resident blocks and by the library's host code for the Python loop (a function of (seed, step, walker):
    # no numbers cross PCIe, the chain does not depend on how it is run or cut into blocks); "host" -- NumPy's Mersenne
    # twister, drawn on the host as emcee does (the draws of 256 walkers then bound small catalogues: 26 000 steps/s at 1e5
    # stars against 30 000).  emcee itself, when it drives (SAMPLER), draws as it always does.
    RNG = "device"
    NATIVE_STRETCH = True          # sub-classes whose posterior is not ONE un-binned catalogue switch this off

    def _stretch_plan(self):
        """Arguments of ``mcd_stretch_move_prior`` for the current parameter configuration (``plan.simple``: boxes with
        flat or structured priors): which free parameter feeds each kernel column, constants for fixed parameters, unit
        factors, bounds, and the structured priors (None without one)."""
        plan = self._plan()
        cached = getattr(self, "_stretch_cache", None)
        if cached is not None and cached[0] is plan:
            return cached[1]
        free_pos = {int(i): j for j, i in enumerate(plan.free_idx)}
        fixed_val = {int(i): float(v) for i, v in zip(plan.fixed_idx, plan.fixed_val)}
        k = len(plan.kernel_idx)
        fac = np.ones(k) if plan.kernel_fac is None else np.asarray(plan.kernel_fac, dtype=np.float64)
        src, const = np.full(k, -1, dtype=np.int32), np.zeros(k)
        for c, i in enumerate(plan.kernel_idx):
            if int(i) in free_pos:
                src[c] = free_pos[int(i)]
            else:
                const[c] = fixed_val[int(i)] * fac[c] if plan.kernel_fac is not None else fixed_val[int(i)]
        fixed_ok = bool(np.all((plan.fixed_val >= plan.lo[plan.fixed_idx]) & (plan.fixed_val <= plan.hi[plan.fixed_idx]))) \
            if plan.fixed_idx.size else True
        out = {"col_source": src, "col_const": const, "col_factor": fac, "lo": plan.lo[plan.free_idx].copy(),
               "hi": plan.hi[plan.free_idx].copy(), "fixed_ok": fixed_ok, "prior": plan.prior}
        self._stretch_cache = (plan, out)
        return out

    def _stretch_catalog(self, pos):
        """The catalogue a library block runs on, after the checks both kinds of block share."""
        plan = self._plan()
        if not plan.simple:
            raise RuntimeError("the parameter configuration changed to one with expression priors / constraints during a run")
        if self._context is not None and getattr(self._context, "n_ranks", 1) > 1:
            self._check_ranks_agree(pos)
        cat = self._catalog
        if cat is None or plan.catalog_key != self._catalog_key:
            cat = self._ensure_catalog()
        return cat

    def _stretch_block_seeded(self, pos, lnp, seed, step0, n_steps, chain, lnprob_chain, accepted):
        """One block of steps with the random numbers generated inside the library (``_native.Catalog.stretch_move_seeded``)."""
        cat = self._stretch_catalog(pos)
        cat.stretch_move_seeded(self._stretch_plan(), pos, lnp, seed, step0, n_steps, chain, lnprob_chain, accepted)
        if self._precision != "f64":
            self._note_f32(cat)

    def _de_block_seeded(self, gamma0, sigma, pos, lnp, seed, step0, n_steps, chain, lnprob_chain, accepted):
        """One block of differential-evolution steps inside the library (``_native.Catalog.de_move_seeded``)."""
        cat = self._stretch_catalog(pos)
        cat.de_move_seeded(self._stretch_plan(), pos, lnp, gamma0, sigma, seed, step0, n_steps, chain, lnprob_chain, accepted)
        if self._precision != "f64":
            self._note_f32(cat)

    def _stretch_block(self, pos, lnp, order, zz, thr, pick, chain, lnprob_chain, accepted):
        """One block of stretch-move steps inside the library (``_native.Catalog.stretch_move``)."""
        cat = self._stretch_catalog(pos)
        cat.stretch_move(self._stretch_plan(), pos, lnp, order, zz, thr, pick, chain, lnprob_chain, accepted)
        if self._precision != "f64":
            self._note_f32(cat)

    def __call__(self, n_walkers=100, n_steps=500, n_burn=100, n_threads=1, n_out=None, pos=None, lnprob0=None,
                 plot=False, prefix="sampler", true_values=None, move=None, gamma0=None, sigma=1e-5, **kwargs):
        """Run the MCMC (runner.py:332-443).  Same arguments as the reference; ``n_threads`` must be 1
        because the likelihood of all walkers is one GPU launch (a process pool would fork after HIP
        initialisation and hold W copies of the catalogue).  ``move``: ``"stretch"`` (the default of the class attribute
        ``MOVE``; what emcee runs) or ``"de"``, the built-in sampler's differential-evolution move with scale ``gamma0``
        (None: 2.38 / sqrt(2 P)) and jitter ``sigma`` (``sampler.EnsembleSampler``)."""
        if kwargs:
            if "filename" in kwargs or "plotfilename" in kwargs:
                logger.warning("Parameters <filename> and <plotfilename> not used anymore. Use <prefix> instead.")
        if n_threads != 1:
            raise ValueError("n_threads > 1 is not supported by the GPU backend: walkers are batched on the device.")

        fig = None
        if plot:
            import matplotlib.pyplot as plt
            fig, _ = plt.subplots(self.n_fitted_parameters, 1, sharex="all", figsize=(8, 9))

        if pos is not None:
            pos = np.asarray(pos, dtype=np.float64)
            assert pos.shape == (n_walkers, self.n_fitted_parameters), "Array with starting values has invalid shape."
        else:
            pos = self.get_initials(n_walkers=n_walkers)

        # Several ranks (stars sharded, one process per GPU): rank 0's start positions and one sampler seed go to every
        # rank, so that all of them propose the same walkers at every step (the reference has one process, runner.py:403).
        group, seed = self._rank_group(), None
        if group is not None:
            pos = group.bcast_array(pos, src=0)
            seed = int(group.bcast_json(int(np.random.SeedSequence().entropy % (2 ** 32)), src=0))

        lp0 = self.lnprior_batch(pos)
        for i in range(n_walkers):
            if not np.isfinite(lp0[i]):
                raise ValueError("Invalid initial guesses for walker {0}: {1}={2}".format(
                    i, self.fitted_parameters, pos[i]))                                      # runner.py:392-395

        sampler = self._make_sampler(n_walkers, seed=seed, move=move, gamma0=gamma0, sigma=sigma)
        logger.info("Running MCMC chain ...")
        if n_out is not None:
            logger.info("Iter. <log like>   " + "".join(" {0:12s}".format("<" + n + ">") for n in self.fitted_parameters))

        state = None
        while sampler.iteration < n_steps:
            # runner.py:418-419.  One deliberate difference: the reference re-passes the caller's
            # `lnprob0` on every chunk although the positions have moved; it is used for the first chunk only.
            try:
                result = sampler.run_mcmc(pos, n_out if n_out is not None else n_steps, log_prob0=lnprob0,
                                          rstate0=state, progress=False)
            except BaseException as exc:
                # several ranks: the peers are inside (or about to enter) an all-reduce this rank will not join any more.
                # Tell them before the exception travels on (hostgroup.abort -> mcd_ctx_abort on their side): they leave
                # their wait with an error at once instead of at the library's collective deadline.  Every rank ends with
                # an exception; nothing is retried or re-routed inside the process.
                if group is not None:
                    group.abort("{0}: {1}".format(type(exc).__name__, exc))
                raise
            pos, lnp, state = tuple(result)[:3]
            lnprob0 = None
            if n_out is not None:
                output = " {0:4d} {1:12.5e}".format(sampler.iteration, np.mean(lnp[:]))
                output += "".join(" {0:12.5e}".format(np.mean(pos[:, i])) for i in range(self.n_fitted_parameters))
                if sampler.iteration % n_out == 0:
                    if prefix is not None:
                        self.save_current_status(sampler, prefix=prefix)
                    if plot:
                        for ax in fig.axes:
                            ax.cla()
                        self.plot_chain(sampler.chain, true_values=true_values, figure=fig,
                                        filename="{0}_chains.png".format(prefix) if prefix is not None else None)
                logger.info(output)
        return sampler

    # ------------------------------------------------------------------ convergence (no counterpart in the reference)
    def _diagnostics_context(self):
        """Where the chain diagnostics run: this runner's device context."""
        return self.context

    def run_converged(self, n_walkers=100, max_steps=20000, check_every=500, tol=50.0, rtol=0.01, **call_kwargs):
        """Run the MCMC until the integrated autocorrelation time says it is long enough (emcee's documented pattern):
        increments of ``check_every`` steps, after each one ``tau`` from ``diagnostics.integrated_time(..., quiet=True)``;
        stops when ``steps > tol max(tau)`` and ``max |tau - previous tau| / tau < rtol``, or at ``max_steps``.  Works with
        whichever sampler ``SAMPLER`` selects (it needs ``run_mcmc`` and ``get_chain()``); ``pos``, ``lnprob0``, ``move``,
        ``gamma0`` and ``sigma`` as in ``__call__``.  Returns ``(sampler, history)``, ``history`` a list of ``(steps, tau)`` per check."""
        from .. import diagnostics
        pos, lnprob0 = call_kwargs.pop("pos", None), call_kwargs.pop("lnprob0", None)
        move = {k: call_kwargs.pop(k) for k in ("move", "gamma0", "sigma") if k in call_kwargs}
        if call_kwargs:
            raise TypeError("run_converged: unknown argument(s) {0}".format(sorted(call_kwargs)))
        if pos is None:
            pos = self.get_initials(n_walkers=n_walkers)
        pos = np.asarray(pos, dtype=np.float64)
        group, seed = self._rank_group(), None
        if group is not None:
            pos = group.bcast_array(pos, src=0)
            seed = int(group.bcast_json(int(np.random.SeedSequence().entropy % (2 ** 32)), src=0))
        if not np.all(np.isfinite(self.lnprior_batch(pos))):
            raise ValueError("Invalid initial guesses for some walker(s).")
        sampler = self._make_sampler(n_walkers, seed=seed, **move)
        history, previous, steps = [], None, 0
        while steps < max_steps:
            n = int(min(check_every, max_steps - steps))
            try:
                result = sampler.run_mcmc(pos, n, log_prob0=lnprob0, progress=False)
            except BaseException as exc:
                if group is not None:
                    group.abort("{0}: {1}".format(type(exc).__name__, exc))
                raise
            pos, lnprob0 = tuple(result)[0], None
            steps += n
            if steps < 2:
                continue
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")                     # (a chain that is still too short is the normal case here)
                tau = np.array(diagnostics.integrated_time(sampler.get_chain(), tol=tol, quiet=True,
                                                           context=self._diagnostics_context()))
            history.append((steps, tau))
            logger.info("convergence check at %d steps: tau = %s", steps, tau)
            if np.all(np.isfinite(tau)) and steps > tol * np.max(tau) and previous is not None and \
                    np.max(np.abs(tau - previous) / tau) < rtol:
                break
            previous = tau
        return sampler, history

    def chain_diagnostics(self, chain, n_burn, c=5.0, tol=50.0):
        """``diagnostics.summary`` of a chain in the reference's layout (W, steps, P) after ``n_burn`` steps -- tau, window,
        found, converged, ess, rhat, mean, std per fitted parameter -- plus ``names``."""
        from .. import diagnostics
        chain = np.asarray(chain, dtype=np.float64)
        if chain.ndim != 3:
            raise ValueError("chain must have shape (walkers, steps, parameters)")
        out = diagnostics.summary(np.swapaxes(chain[:, n_burn:, :], 0, 1), c=c, tol=tol, context=self._diagnostics_context())
        out["names"] = list(self.fitted_parameters)
        return out

    # ------------------------------------------------------------------ checkpoints (runner.py:445-519)
    @staticmethod
    def save_chain(sampler, filename="samplerchain.pkl"):
        warnings.warn("Method Runner.save_chain() is deprecated. Use Runner.save_current_status() instead.",
                      DeprecationWarning)
        prefix = filename.split(".")[0]
        if len(prefix) > 5 and prefix[-5:] == "chain":
            prefix = prefix[:-5]
        Runner.save_current_status(sampler, prefix=prefix)

    @staticmethod
    def save_current_status(sampler, prefix="sampler"):
        """Pickle ``sampler.chain`` (W, steps, P) and ``sampler.lnprobability`` (W, steps) to
        ``{prefix}_chain.pkl`` / ``{prefix}_lnprob.pkl`` -- the reference's on-disk format."""
        with open("{0}_chain.pkl".format(prefix), "wb") as f:
            pickle.dump(np.asarray(sampler.chain), f)
        with open("{0}_lnprob.pkl".format(prefix), "wb") as f:
            pickle.dump(np.asarray(sampler.lnprobability), f)

    @staticmethod
    def read_chain(filename="samplerchain.pkl"):
        with open(filename, "rb") as f:
            return pickle.load(f)

    @staticmethod
    def read_final_chain(filename="restart.plk"):
        with open(filename, "rb") as f:
            chain = pickle.load(f)
        return chain[:, -1, :]

    # ------------------------------------------------------------------ chain statistics (runner.py:521-660)
    def convert_to_parameters(self, chain, n_burn):
        """Chain (W, steps, P) -> dict name -> flat samples, including fixed and constrained parameters."""
        chain = np.asarray(chain)
        flat = chain[:, n_burn:, :].reshape(-1, chain.shape[2])
        resolved = self.parameters.resolve_batch(flat)
        return {name: np.array(col) for name, col in resolved.items()}

    def compute_percentiles(self, chain, n_burn, pct=None):
        if pct is None:
            pct = [16, 50, 84]
        samples = np.asarray(chain)[:, n_burn:, :].reshape((-1, self.n_fitted_parameters))
        return np.percentile(samples, pct, axis=0)

    def compute_bestfit_values(self, chain, n_burn):
        """Median and upper / lower 1-sigma uncertainties per fitted parameter; the medians are also
        written into ``self.parameters`` as in the reference (runner.py:649)."""
        percentiles = self.compute_percentiles(chain, n_burn=n_burn, pct=[16, 50, 84])
        results = ResultsTable()
        i = 0
        for name, parameter in self.parameters.items():
            if parameter.fixed:
                continue
            parameter.value = percentiles[1, i]
            results.add_column(name, percentiles[1, i], percentiles[2, i] - percentiles[1, i],
                               percentiles[1, i] - percentiles[0, i], unit=parameter.unit)
            i += 1
        return results

    def plot_chain(self, chain, filename="chains.png", true_values=None, figure=None, lnprob=None, plot_median=False):
        """Trace plot of every fitted parameter (simplified form of runner.py:675-770)."""
        import matplotlib.pyplot as plt
        chain = np.asarray(chain)
        if figure is None:
            figure, _ = plt.subplots(self.n_fitted_parameters, 1, sharex="all", figsize=(8, 9))
        for i, ax in enumerate(figure.axes[:self.n_fitted_parameters]):
            ax.plot(chain[:, :, i].T, color="k", alpha=0.3, lw=0.6)
            if plot_median:
                ax.plot(np.median(chain[:, :, i], axis=0), color="C3", lw=1.5)
            if true_values is not None:
                ax.axhline(true_values[i], color="C0", lw=1.5)
            ax.set_ylabel(self.labels[i])
        if filename is not None:
            figure.savefig(filename)
        return figure

    def sample_chain(self, chain, n_burn, n_samples=1):
        """``n_samples`` random parameter sets from the post-burn-in chain, each as the dictionary
        ``fetch_parameter_values`` returns (runner.py:820-850)."""
        flat = np.reshape(np.asarray(chain)[:, n_burn:], (-1, np.shape(chain)[-1]))
        indices = np.random.randint(0, flat.shape[0], (n_samples,))
        return [self.fetch_parameter_values(row) for row in flat[indices]]

    # ------------------------------------------------------------------ per-star posterior summaries (new)
    def _has_background(self):
        model = self._catalog_spec()[0][0]
        return model not in (_native.MODEL_CONST, _native.MODEL_PROFILE, _native.MODEL_DOUBLE,
                             _native.MODEL_CONST_ESCALE, _native.MODEL_PROFILE_ESCALE)

    def _pointwise_posterior(self, chain, n_burn, thin, membership):
        """mcd_pointwise_posterior over the post-burn-in samples of ``chain`` (W, steps, P), every ``thin``-th step, in the
        order of ``convert_to_parameters``; fixed parameters, constraints and unit factors as in ``lnprob_batch``."""
        table, n_samples = self._posterior_table(chain, n_burn, thin)
        out = self._ensure_catalog().pointwise_posterior(table, membership=membership)
        out["n_samples"] = n_samples
        return out

    def _posterior_table(self, chain, n_burn, thin):
        """The kernel table (S, K) of the post-burn-in samples of ``chain`` and S; refuses ranks with different chains."""
        chain = np.asarray(chain, dtype=np.float64)
        if chain.ndim != 3 or chain.shape[2] != self.n_fitted_parameters:
            raise ValueError("chain must have shape (n_walkers, n_steps, {0})".format(self.n_fitted_parameters))
        if int(thin) < 1:
            raise ValueError("thin must be >= 1")
        flat = chain[:, n_burn::int(thin), :].reshape(-1, chain.shape[2])
        if flat.shape[0] == 0:
            raise ValueError("no samples left after n_burn = {0}".format(n_burn))
        group = self._rank_group()
        if group is not None and not group.same_everywhere(flat):
            raise RuntimeError("the ranks of this job passed different chains: their stars' summaries would not belong to "
                               "one posterior (every rank must pass the same chain)")
        resolved = self.parameters.resolve_batch(flat)
        self._ensure_catalog()
        return self._kernel_table(resolved), flat.shape[0]

    def pointwise_posterior(self, chain, n_burn, thin=1):
        """Per-star summaries over the S post-burn-in samples of ``chain`` (W, steps, P), computed on the device in one
        call: ``lppd`` = log of the posterior mean of exp(lnL_i), ``lnl_var`` = posterior variance of lnL_i (lnL_i: the
        star's term of ``lnlike``), and for the models with a background ``pmem_mean`` / ``pmem_std``, the posterior mean
        and standard deviation of the membership probability; plus ``n_samples``.  Several ranks: this rank's stars."""
        return self._pointwise_posterior(chain, n_burn, thin, self._has_background())

    def waic(self, chain, n_burn, thin=1):
        """Widely applicable information criterion of the model for the post-burn-in samples of ``chain``
        (``waic_summary``): ``elpd_waic``, ``p_waic``, ``waic`` = -2 elpd_waic, ``se``, ``lppd``, ``n_samples``,
        ``n_stars``, ``n_high_variance`` (stars whose posterior variance of lnL exceeds 0.4, logged) and ``pointwise``
        (elpd_i of this rank's stars).  A lower ``waic`` is the better model for the same stars."""
        pp = self._pointwise_posterior(chain, n_burn, thin, False)
        out = waic_summary(pp["lppd"], pp["lnl_var"], pp["n_samples"], self._rank_group())
        if out["n_high_variance"]:
            logger.warning("WAIC: %d of %d stars have a posterior variance of lnL above %.1f; the estimate may be "
                           "unreliable (Vehtari, Gelman & Gabry 2017)", out["n_high_variance"], out["n_stars"],
                           WAIC_VAR_WARNING)
        return out

    def loo(self, chain, n_burn, thin=1, r_eff=1.0):
        """Pareto-smoothed importance-sampling leave-one-out cross-validation (PSIS-LOO; Vehtari, Gelman & Gabry 2017) of
        the model for the post-burn-in samples of ``chain``, computed on the device (``loo_summary``): ``elpd_loo``,
        ``p_loo``, ``looic`` = -2 elpd_loo, ``se``, ``lppd``, ``n_samples``, ``n_stars``, ``k_threshold``, ``n_bad_k``
        (stars whose Pareto k^ exceeds the threshold, logged), and this rank's per-star ``pareto_k``, ``pointwise``
        (elpd_loo_i) and ``n_eff``.  ``r_eff``: the relative efficiency of the samples (a scalar; 1 for independent
        draws).  A higher ``elpd_loo`` is the better model for the same stars; compare two with ``elpd_compare``."""
        table, n_samples = self._posterior_table(chain, n_burn, thin)
        res = self._ensure_catalog().psis_loo(table, r_eff=r_eff)
        out = loo_summary(res["elpd_loo"], res["lppd"], res["pareto_k"], n_samples, self._rank_group())
        out["n_eff"] = res["n_eff"]
        if out["n_bad_k"]:
            logger.warning("PSIS-LOO: %d of %d stars have a Pareto k above %.2f; their leave-one-out estimates are "
                           "unreliable (see pareto_k)", out["n_bad_k"], out["n_stars"], out["k_threshold"])
        return out

    # ------------------------------------------------------------------ exact leave-out refits (new)
    def _holdout_check(self, what):
        """Hold-out refits run on one un-binned float64 catalogue of one device in one process."""
        ctx = self._context
        if ctx is not None and getattr(ctx, "n_ranks", 1) > 1:
            raise NotImplementedError("Runner.{0}: hold-out refits run in one process on one device; this runner sits on a "
                                      "context of {1} ranks".format(what, ctx.n_ranks))
        if ctx is not None and int(getattr(ctx, "n_devices", 1)) > 1:
            raise NotImplementedError("Runner.{0}: hold-out refits run on one device; this runner's context has "
                                      "{1}".format(what, int(ctx.n_devices)))
        if self._precision != "f64":
            raise NotImplementedError("Runner.{0}: hold-out refits need a float64 catalogue".format(what))

    def _holdout_sibling(self, data):
        """A runner of this class on ``data``: a deep copy of the parameters, the same background object, context and
        precision (NumPy's global generator, which every Runner seeds, is left as found)."""
        state = np.random.get_state()
        try:
            kwargs = {"parameters": self.parameters.copy(), "context": self._context, "precision": self._precision}
            if self.background is not None:
                kwargs["background"] = self.background
            return type(self)(data, **kwargs)
        finally:
            np.random.set_state(state)

    @staticmethod
    def _holdout_layout(sets, n_data):
        """(sets as index arrays, permutation with the held-out stars first, set by set, offsets (E + 1,))."""
        sets = [np.asarray(s, dtype=np.intp).reshape(-1) for s in sets]
        if not sets:
            raise ValueError("sets must hold at least one index array")
        held = np.concatenate(sets) if sets else np.zeros(0, dtype=np.intp)
        if held.size and (held.min() < 0 or held.max() >= n_data):
            raise ValueError("star indices must lie in [0, {0})".format(n_data))
        if np.unique(held).size != held.size:
            raise ValueError("the hold-out sets must be disjoint")
        rest = np.setdiff1d(np.arange(n_data, dtype=np.intp), held, assume_unique=True)
        offsets = np.concatenate([[0], np.cumsum([s.size for s in sets])]).astype(np.int64)
        return sets, np.concatenate([held, rest]), offsets

    def holdout_fit(self, sets, n_walkers=64, n_steps=600, n_burn=200, pos=None, seed=None, thin=1, move="stretch", gamma0=None, sigma=1e-5):
        """Refit the model once per hold-out set, all refits in lock step, and evaluate every held-out star under the
        refit that left it out (Vehtari, Gelman & Gabry 2017, sections 2.3 and 2.4).  ``sets``: a list of E disjoint
        arrays of star indices.  E ensembles of ``n_walkers`` walkers take ``n_steps`` stretch-move steps
        (``BinnedSampler``, ``rng="device"``: the chain is a function of ``seed``); ensemble e samples the posterior of
        all stars but set e -- one device launch evaluates all E W proposals against the whole catalogue and keeps each
        set's sum apart (``_native.Catalog.holdout_loglike``).  ``pos``: start positions (E, W, P), default E W rows of
        ``get_initials``.  The post-burn-in samples (every ``thin``-th step after ``n_burn``) of ensemble e then give
        the predictive density of set e's stars (``_native.Catalog.holdout_pointwise``).

        Returns ``elpd`` and ``lnl_var`` (n_data,) in this runner's star order (NaN for stars in no set), ``sets``,
        ``sampler`` (``chain``: (E, W, steps, P)), ``tau`` (E,) the largest integrated autocorrelation time of each
        refit and ``converged`` (E,) whether its post-burn-in chain holds 50 of them (``diagnostics.summary``; logged
        where not), and ``n_samples`` per set.  ``move``, ``gamma0``, ``sigma``: the sampler's move (``BinnedSampler``:
        "stretch" or "de")."""
        self._holdout_check("holdout_fit")
        from .binned import BinnedSampler
        from .. import diagnostics
        if int(thin) < 1:
            raise ValueError("thin must be >= 1")
        if not 0 <= int(n_burn) < int(n_steps):
            raise ValueError("n_burn must lie in [0, n_steps)")
        sets, perm, offsets = self._holdout_layout(sets, self.n_data)
        n_sets, n_p = len(sets), self.n_fitted_parameters
        sib = self._holdout_sibling(self.data.take(perm))
        try:
            if pos is None:
                pos = self.get_initials(n_sets * n_walkers).reshape(n_sets, n_walkers, n_p)
            pos = np.ascontiguousarray(pos, dtype=np.float64)
            if pos.shape != (n_sets, n_walkers, n_p):
                raise ValueError("Array with starting values has invalid shape: expected {0}".format((n_sets, n_walkers, n_p)))
            pars = sib.parameters
            if not np.all(np.isfinite(pars.lnprior_batch(pars.resolve_batch(pos.reshape(-1, n_p))))):
                raise ValueError("Invalid initial guesses: start positions outside the prior")
            cat = sib._ensure_catalog()

            def log_prob(values):
                # box and structured priors as in lnprob_batch; rows outside the prior take a donor row for the launch
                lead = values.shape[:-1]
                resolved = pars.resolve_batch(values.reshape(-1, n_p))
                lp = pars.lnprior_batch(resolved)
                ok = np.isfinite(lp)
                out = np.full(lp.shape, -np.inf)
                if ok.any():
                    if not ok.all():
                        donor = int(np.flatnonzero(ok)[0])
                        resolved = OrderedDict((k, np.where(ok, col, col[donor])) for k, col in resolved.items())
                    table = sib._kernel_table(resolved)
                    train, _ = cat.holdout_loglike(offsets, table.reshape(lead + (table.shape[1],)), want_test=False)
                    out[ok] = train.reshape(-1)[ok] + lp[ok]
                return out.reshape(lead)

            sampler = BinnedSampler(n_sets, n_walkers, n_p, log_prob, seed=seed, rng="device", move=move, gamma0=gamma0, sigma=sigma)
            logger.info("hold-out refits: %d sets of %d .. %d stars, %d walkers each, %d steps", n_sets,
                        min(s.size for s in sets), max(s.size for s in sets), n_walkers, n_steps)
            sampler.reserve(n_steps)
            sampler.run_mcmc(pos, n_steps)
            chain = sampler.chain                                           # (E, W, steps, P)
            kept = chain[:, :, int(n_burn)::int(thin), :]
            n_samples = kept.shape[1] * kept.shape[2]
            resolved = pars.resolve_batch(kept.reshape(-1, n_p))
            table = sib._kernel_table(resolved).reshape(n_sets, n_samples, -1)
            pw = cat.holdout_pointwise(offsets, table)
        finally:
            sib.close()
        elpd, var = np.full(self.n_data, np.nan), np.full(self.n_data, np.nan)
        held = perm[:int(offsets[-1])]
        elpd[held], var[held] = pw["lppd"], pw["lnl_var"]
        diag = diagnostics.summary(np.transpose(chain[:, :, int(n_burn):, :], (2, 0, 1, 3)), context=self._diagnostics_context())
        with np.errstate(invalid="ignore"):
            tau = np.max(np.atleast_2d(diag["tau"]), axis=1)
        converged = np.all(np.atleast_2d(diag["converged"]), axis=1)
        for e in np.flatnonzero(~converged):
            logger.warning("hold-out refit %d: %d post-burn-in steps are fewer than 50 autocorrelation times (tau = %.1f); "
                           "its stars' estimates carry more Monte-Carlo error than the sample count suggests", int(e),
                           n_steps - int(n_burn), float(tau[e]))
        return {"elpd": elpd, "lnl_var": var, "sets": sets, "sampler": sampler, "tau": tau, "converged": converged,
                "n_samples": int(n_samples)}

    def reloo(self, loo_result, chain, n_burn, stars=None, max_refits=16, **fit):
        """Exact leave-one-out values for the stars PSIS cannot handle: refit without each of them (``holdout_fit`` with
        singleton sets) and put the exact elpd_i in place of the PSIS estimate.  ``loo_result``: what ``loo`` returned for
        ``chain`` / ``n_burn``.  ``stars``: the stars to refit; default those with ``pareto_k`` above ``k_threshold``,
        largest k^ first, at most ``max_refits`` (a logged line says how many were left out).  The refits start from
        draws of the post-burn-in rows of ``chain`` -- the full posterior is an excellent start for a leave-one-out
        posterior; ``fit``: further arguments of ``holdout_fit`` (``n_burn`` here is the burn-in of ``chain``: the refits' own
        is ``refit_burn``, default ``holdout_fit``'s).

        Returns a copy of ``loo_result`` with ``pointwise`` replaced for the refitted stars, ``elpd_loo``, ``p_loo``,
        ``looic`` and ``se`` recomputed (the arithmetic of ``loo_summary``), ``refit`` (their indices), ``n_bad_k``
        counting only the stars that still rely on PSIS, ``refit_converged`` / ``refit_tau`` of the refits and ``fit``
        (what ``holdout_fit`` returned).
        ``elpd_compare`` takes the result."""
        self._holdout_check("reloo")
        k = np.asarray(loo_result["pareto_k"], dtype=np.float64)
        thr = float(loo_result["k_threshold"])
        if stars is None:
            bad = np.flatnonzero(k > thr)
            bad = bad[np.argsort(-k[bad], kind="stable")]
            stars = bad[:int(max_refits)]
            logger.info("reloo: %d of %d stars have a Pareto k above %.2f; refitting %d, %d left to PSIS", bad.size, k.size,
                        thr, stars.size, bad.size - stars.size)
        stars = np.asarray(stars, dtype=np.intp).reshape(-1)
        out = dict(loo_result)
        pointwise = np.array(loo_result["pointwise"], dtype=np.float64)
        out["pareto_k"] = k.copy()
        out["refit"] = stars.copy()
        if stars.size:
            fit = dict(fit)
            refit_burn = fit.pop("refit_burn", None)
            if refit_burn is not None:
                fit["n_burn"] = refit_burn
            n_walkers = int(fit.get("n_walkers", 64))
            if fit.get("pos") is None:
                chain = np.asarray(chain, dtype=np.float64)
                flat = chain[:, int(n_burn):, :].reshape(-1, chain.shape[2])
                need = stars.size * n_walkers
                if flat.shape[0] == 0:
                    raise ValueError("no samples left after n_burn = {0}".format(n_burn))
                rng = np.random.RandomState(fit.get("seed"))
                rows = rng.choice(flat.shape[0], size=need, replace=flat.shape[0] < need)
                fit["pos"] = flat[rows].reshape(stars.size, n_walkers, chain.shape[2])
            res = self.holdout_fit([[int(i)] for i in stars], **fit)
            pointwise[stars] = res["elpd"][stars]
            out["refit_converged"], out["refit_tau"], out["fit"] = res["converged"], res["tau"], res
        s_elpd, se, _ = _elpd_totals(pointwise)
        still = np.ones(k.size, dtype=bool)
        still[stars] = False
        out.update({"pointwise": pointwise, "elpd_loo": s_elpd, "p_loo": float(loo_result["lppd"]) - s_elpd,
                    "looic": -2.0 * s_elpd, "se": se, "n_bad_k": int(np.count_nonzero((k > thr) & still))})
        return out

    def loo_moment_match(self, loo_result, chain, n_burn, thin=1, stars=None, max_stars=256, max_iters=30, k_threshold=None,
                         cov=True, split=True, r_eff=1.0):
        """Moment matching (Paananen et al. 2021; ``loo_moment_match`` of the R package loo) for the stars PSIS cannot
        handle: the cheaper remedy to try before ``reloo``.  The post-burn-in draws of ``chain`` (every ``thin``-th step)
        are moved towards each star's leave-one-out posterior by affine maps that match the importance-weighted mean,
        variances and (``cov``) covariance, on the device (``_native.Catalog.moment_match``; csrc/mcd_mmatch.h), with the
        ``split`` step that removes the bias of choosing the map with the draws that carry the estimate.
        ``loo_result``: what ``loo`` returned for the same ``chain`` / ``n_burn`` / ``thin``.  ``stars``: the stars to
        match; default those with ``pareto_k`` above ``k_threshold`` (default ``loo_result["k_threshold"]``), largest k^
        first, at most ``max_stars``.

        Returns a copy of ``loo_result`` with ``pointwise``, ``pareto_k`` and ``n_eff`` replaced for the matched stars,
        ``elpd_loo``, ``p_loo``, ``looic`` and ``se`` recomputed (the arithmetic of ``reloo``), ``n_bad_k`` recounted, and
        ``matched`` (their indices, ascending), ``k_before``, ``k_loop``, ``iterations``, ``accepted`` (n, 3) and
        ``transform`` (``A`` (n, P, P), ``b`` (n, P)) per matched star.  ``reloo`` on the result refits only what is still
        above the threshold; ``elpd_compare`` takes it."""
        self._holdout_check("loo_moment_match")
        self._grad_plan()                      # refuses expr constraints and lnprior expressions
        k = np.asarray(loo_result["pareto_k"], dtype=np.float64)
        thr = float(loo_result["k_threshold"]) if k_threshold is None else float(k_threshold)
        if stars is None:
            bad = np.flatnonzero(k > thr)
            bad = bad[np.argsort(-k[bad], kind="stable")]
            stars = bad[:int(max_stars)]
            logger.info("loo_moment_match: %d of %d stars have a Pareto k above %.2f; matching %d", bad.size, k.size, thr,
                        stars.size)
        stars = np.unique(np.asarray(stars, dtype=np.int64).reshape(-1))
        if stars.size and (stars[0] < 0 or stars[-1] >= k.size):
            raise ValueError("star indices must lie in [0, {0})".format(k.size))
        out = dict(loo_result)
        pointwise = np.array(loo_result["pointwise"], dtype=np.float64)
        pareto_k, n_eff = k.copy(), np.array(loo_result["n_eff"], dtype=np.float64)
        n_p = self.n_fitted_parameters
        res = {"k_before": np.zeros(0), "k_loop": np.zeros(0), "iterations": np.zeros(0, dtype=np.int32),
               "accepted": np.zeros((0, 3), dtype=np.int32), "A": np.zeros((0, n_p, n_p)), "b": np.zeros((0, n_p))}
        if stars.size:
            chain = np.asarray(chain, dtype=np.float64)
            if chain.ndim != 3 or chain.shape[2] != n_p:
                raise ValueError("chain must have shape (n_walkers, n_steps, {0})".format(n_p))
            if int(thin) < 1:
                raise ValueError("thin must be >= 1")
            draws = np.ascontiguousarray(chain[:, n_burn::int(thin), :].reshape(-1, n_p))
            if draws.shape[0] != int(loo_result["n_samples"]):
                raise ValueError("chain, n_burn and thin give {0} draws, loo_result was made from {1}".format(
                    draws.shape[0], int(loo_result["n_samples"])))
            res = self._stretch_catalog(draws).moment_match(self._stretch_plan(), draws, stars, thr, max_iters=max_iters,
                                                            cov=cov, split=split, r_eff=r_eff)
            pointwise[stars], pareto_k[stars], n_eff[stars] = res["elpd"], res["pareto_k"], res["n_eff"]
        s_elpd, se, _ = _elpd_totals(pointwise)
        out.update({"pointwise": pointwise, "pareto_k": pareto_k, "n_eff": n_eff, "elpd_loo": s_elpd,
                    "p_loo": float(loo_result["lppd"]) - s_elpd, "looic": -2.0 * s_elpd, "se": se,
                    "n_bad_k": int(np.count_nonzero(pareto_k > float(loo_result["k_threshold"]))), "matched": stars,
                    "k_before": res["k_before"], "k_loop": res["k_loop"], "iterations": res["iterations"],
                    "accepted": res["accepted"], "transform": {"A": res["A"], "b": res["b"]}})
        self._warn_bad_k("loo_moment_match", out["n_bad_k"], k.size, float(loo_result["k_threshold"]))
        return out

    def kfold(self, n_folds=10, seed=None, **fit):
        """K-fold cross-validation: a random partition of the stars into ``n_folds`` sets drawn from ``seed``, one refit
        per fold in lock step (``holdout_fit``; ``fit``: its further arguments, ``seed`` by default this one), every star
        evaluated under the refit that left its fold out.  Returns ``kfold_summary`` -- ``elpd_kfold``, ``se``,
        ``pointwise``, ``n_stars``, ``n_folds``, ``folds`` -- plus ``converged`` and ``tau`` per fold, ``n_samples`` and ``fit`` (what
        ``holdout_fit`` returned).
        The remedy when many Pareto k^ are bad; ``elpd_compare`` takes the result."""
        self._holdout_check("kfold")
        n, n_folds = self.n_data, int(n_folds)
        if not 2 <= n_folds <= n:
            raise ValueError("n_folds must lie in [2, n_data]")
        folds = np.empty(n, dtype=np.int64)
        folds[np.random.RandomState(seed).permutation(n)] = np.arange(n) % n_folds
        fit = dict(fit)
        fit.setdefault("seed", seed)
        res = self.holdout_fit([np.flatnonzero(folds == f) for f in range(n_folds)], **fit)
        out = kfold_summary(res["elpd"], folds)
        out.update({"converged": res["converged"], "tau": res["tau"], "n_samples": res["n_samples"], "fit": res})
        return out

    def _warn_bad_k(self, what, n_bad, n_stars, threshold):
        if n_bad:
            logger.warning("%s: %d of %d stars have a Pareto k above %.2f; their leave-one-out estimates are "
                           "unreliable (see pareto_k)", what, n_bad, n_stars, threshold)

    def _count_bad_k(self, pareto_k, n_samples):
        """(threshold, stars above it, stars) over all ranks."""
        thr = loo_k_threshold(n_samples)
        totals = np.array([float(np.count_nonzero(pareto_k > thr)), float(pareto_k.size)])
        group = self._rank_group()
        if group is not None:
            totals = np.asarray(group.allreduce(totals), dtype=np.float64)
        return float(thr), int(totals[0]), int(totals[1])

    def loo_pit(self, chain, n_burn, thin=1, r_eff=1.0, n_bins=20):
        """Leave-one-out probability integral transform of every star for the post-burn-in samples of ``chain``: the CDF of
        the model at v_i averaged under the PSIS weights of ``loo`` (sum_s w~_is F_is), so that star i is judged by a fit
        it took no part in -- the posterior average of ``ppc`` uses the data twice and is too central for small samples.
        Computed on the device in one call.  Per star (this rank's): ``loo_pit`` (the mixture CDF ``pit_mix`` where the
        model has one, else the cluster component's ``pit``), the leave-one-out means ``z``, ``vlos`` and ``sigma``,
        ``pareto_k``, ``n_eff`` and ``weight`` (the posterior mean membership probability, 1 without a background).  The
        entries of ``ppc_summary`` of ``loo_pit`` with the weighting rule of ``ppc`` (``hist``, ``n``, ``chi2``,
        ``tail_fraction``, ``n_stars``; summed over the ranks), ``n_samples``, ``k_threshold`` and ``n_bad_k`` (logged)."""
        table, n_samples = self._posterior_table(chain, n_burn, thin)
        mix = self._has_mixture_cdf()
        res = self._ensure_catalog().psis_loo_expect(table, r_eff=r_eff, predictive=True, mixture=mix)
        out = {"loo_pit": res["pit_mix"] if mix else res["pit"], "z": res["z"], "vlos": res["vlos"], "sigma": res["sigma"],
               "pareto_k": res["pareto_k"], "n_eff": res["n_eff"], "n_samples": n_samples}
        if mix:
            out["pit"] = res["pit"]
        weighted = self._has_background() and not mix
        if self._has_background():
            out["weight"] = self._pointwise_posterior(chain, n_burn, thin, True)["pmem_mean"]
        else:
            out["weight"] = np.ones(out["loo_pit"].size)
        out.update(ppc_summary(out["loo_pit"], out["weight"] if weighted else None, n_bins, self._rank_group()))
        out["k_threshold"], out["n_bad_k"], n_all = self._count_bad_k(out["pareto_k"], n_samples)
        self._warn_bad_k("LOO-PIT", out["n_bad_k"], n_all, out["k_threshold"])
        return out

    def loo_influence(self, chain, n_burn, thin=1, r_eff=1.0, functions=None):
        """Influence of every star on the fit: the case-deletion posterior means E[h | y_-i] = sum_s w~_is h(theta_s) under
        the PSIS weights of ``loo``, computed on the device.  ``functions``: dict name -> callable on the flat post-burn-in
        samples (S, P) returning (S,), e.g. ``{"v_rot": lambda t: np.hypot(t[:, 2], t[:, 3])}``; default: the fitted
        parameters.  Returns ``names``, ``mean`` and ``std`` (Q,) of the functions over the posterior, ``shift``
        (n_stars, Q) = (E[h | y_-i] - mean) / std -- positive: the estimate rises when the star is removed -- and
        ``loo_mean`` = mean + std shift, ``pareto_k`` (a shift is as reliable as its star's k^), ``k_threshold``,
        ``n_bad_k`` (logged), ``n_samples`` and ``ranking``: this rank's star indices by max_q |shift|, descending.  The
        columns reach the device standardised, (h - mean) / std, so nothing cancels for a v_sys of 300 km/s known to 0.1;
        a function that is constant over the samples has shift 0.  More than 16 functions run in batches of 16."""
        table, n_samples = self._posterior_table(chain, n_burn, thin)
        flat = np.asarray(chain, dtype=np.float64)[:, n_burn::int(thin), :].reshape(-1, self.n_fitted_parameters)
        if functions is None:
            names = list(self.fitted_parameters)
            cols = flat
        else:
            names = list(functions)
            cols = np.empty((flat.shape[0], len(names)))
            for q, name in enumerate(names):
                col = np.asarray(functions[name](flat), dtype=np.float64)
                if col.shape != (flat.shape[0],):
                    raise ValueError("function '{0}' must return one value per sample, shape ({1},)".format(name,
                                                                                                             flat.shape[0]))
                cols[:, q] = col
        if not names:
            raise ValueError("no functions to follow")
        mean, std = cols.mean(axis=0), cols.std(axis=0)
        zcols = np.where(std > 0.0, (cols - mean) / np.where(std > 0.0, std, 1.0), 0.0)
        cat = self._ensure_catalog()
        shift, res = [], None
        for q0 in range(0, len(names), cat.LOO_MAX_FUNC):
            res = cat.psis_loo_expect(table, r_eff=r_eff, func=zcols[:, q0:q0 + cat.LOO_MAX_FUNC], predictive=False)
            shift.append(res["func"])
        shift = np.concatenate(shift, axis=1)
        out = {"names": names, "mean": mean, "std": std, "shift": shift, "loo_mean": mean + std * shift,
               "pareto_k": res["pareto_k"], "n_samples": n_samples}
        with np.errstate(invalid="ignore"):
            score = np.max(np.abs(np.where(np.isfinite(shift), shift, np.inf)), axis=1) if shift.size else np.zeros(0)
        out["ranking"] = np.argsort(-score, kind="stable")
        out["k_threshold"], out["n_bad_k"], n_all = self._count_bad_k(out["pareto_k"], n_samples)
        self._warn_bad_k("LOO influence", out["n_bad_k"], n_all, out["k_threshold"])
        return out

    def posterior_membership_probabilities(self, chain, n_burn, thin=1):
        """(mean, std) per star of the membership probability over the post-burn-in samples of ``chain`` -- the posterior
        average that ``calculate_membership_probabilities`` (the reference's value at the median parameters) leaves out."""
        if not self._has_background():
            raise ValueError("{0} has no background component: every star is a member".format(type(self).__name__))
        pp = self._pointwise_posterior(chain, n_burn, thin, True)
        return pp["pmem_mean"], pp["pmem_std"]

    def _has_mixture_cdf(self):
        """The two models whose background has a CDF (a Gaussian fitted with the cluster)."""
        return self._catalog_spec()[0][0] in (_native.MODEL_CONST_BGGAUSS, _native.MODEL_PROFILE_BGGAUSS,
                                             _native.MODEL_DOUBLE_BGGAUSS)

    def posterior_predictive(self, chain, n_burn, thin=1):
        """Per-star posterior predictive checks over the S post-burn-in samples of ``chain`` (W, steps, P), computed on the
        device in one call (chain handling as ``pointwise_posterior``): posterior mean and standard deviation of the
        standardised residual z = (v_i - v_los) / sqrt(verr_i^2 + sigma_los^2) (``z_mean``, ``z_std``), the posterior mean
        of its two-sided tail probability (``tail_p``) and of the cluster component's CDF at v_i (``pit``), mean and
        standard deviation of the model's v_los and sigma_los at the star (``vlos_*``, ``sigma_*``), and for
        ConstantFitGB / ModelFitGB ``pit_mix``, the CDF of the whole cluster + background mixture; plus ``n_samples``.
        Several ranks: this rank's stars."""
        table, n_samples = self._posterior_table(chain, n_burn, thin)
        out = self._ensure_catalog().posterior_predictive(table, mixture=self._has_mixture_cdf())
        out["n_samples"] = n_samples
        return out

    def ppc(self, chain, n_burn, thin=1, n_bins=20, outlier_p=None):
        """Posterior predictive check of the fitted model: the per-star arrays of ``posterior_predictive``, the entries of
        ``ppc_summary`` (``hist``, ``n``, ``chi2``, ``tail_fraction``, ``n_stars``; summed over the ranks) and ``outliers``.
        The summary is taken of ``pit_mix`` where it exists, else of ``pit`` weighted by the posterior mean of the
        membership probability for the other background models (one ``pointwise_posterior`` call), else unweighted.
        ``weight`` is that membership probability (1 without a background) and ``outliers`` are this rank's star indices
        with ``weight`` > 0.5 and ``tail_p`` < ``outlier_p`` (default: 0.05 / n_stars over all ranks, Bonferroni):
        likely members many sigma off the model -- binary candidates and bad measurements."""
        out = self.posterior_predictive(chain, n_burn, thin)
        n_local = out["pit"].size
        if self._has_background():
            weight = self._pointwise_posterior(chain, n_burn, thin, True)["pmem_mean"]
        else:
            weight = np.ones(n_local)
        group = self._rank_group()
        if "pit_mix" in out:
            summary = ppc_summary(out["pit_mix"], None, n_bins, group)
        else:
            summary = ppc_summary(out["pit"], weight if self._has_background() else None, n_bins, group)
        out.update(summary)
        if outlier_p is None:
            total = float(group.allreduce(np.array([float(n_local)]))[0]) if group is not None else float(n_local)
            outlier_p = 0.05 / max(total, 1.0)
        out["weight"] = weight
        out["outlier_p"] = float(outlier_p)
        out["outliers"] = np.flatnonzero((weight > 0.5) & (out["tail_p"] < outlier_p))
        return out

    # ------------------------------------------------------------------ replicated-data checks per group of stars (new)
    def _replicate_background(self):
        """(mean, sigma) in km/s of the fixed background a replicate is drawn from; NaN for the other models."""
        model = self._catalog_spec()[0][0]
        if model not in (_native.MODEL_CONST_BGFIXED, _native.MODEL_PROFILE_BGFIXED, _native.MODEL_PROFILE_BGDENS):
            return float("nan"), float("nan")
        if not isinstance(self.background, Gaussian):
            raise NotImplementedError("Runner.replicate_check: a {0} background cannot be sampled from its log-likelihood "
                                      "column alone; replicated data need a background.Gaussian"
                                      .format(type(self.background).__name__))
        return self.background.mean, self.background.sigma

    def _replicate_groups(self, annuli, groups):
        """(range_offsets, order, (label key, label value)) of the groups of a replicate_check."""
        n = self.n_data
        if groups is not None:
            groups = np.asarray(groups)
            if groups.shape != (n,) or not np.issubdtype(groups.dtype, np.integer):
                raise ValueError("groups must be an int array with one entry per star")
            if groups.size and groups.min() < -1:
                raise ValueError("groups: -1 leaves a star out; other negative labels are not allowed")
            n_groups = int(groups.max()) + 1 if groups.size and groups.max() >= 0 else 1
            label = ("groups", np.arange(n_groups))
        else:
            pr, pd = self.parameters["ra_center"], self.parameters["dec_center"]
            dx, dy = calc_xy_offset(self.ra, self.dec, units.to_unit(pr.value, "deg", pr.unit),
                                    units.to_unit(pd.value, "deg", pd.unit))
            r = np.hypot(dx, dy)
            if np.ndim(annuli) == 0:
                n_groups = int(annuli)
                if n_groups < 1:
                    raise ValueError("annuli must be >= 1")
                rank = np.empty(n, dtype=np.int64)
                rank[np.argsort(r, kind="stable")] = np.arange(n)
                groups = rank * n_groups // max(n, 1)
                by_r = np.sort(r)
                cuts = [by_r[min(n - 1, -(-n * g // n_groups))] for g in range(1, n_groups)] if n else []
                edges = np.array([by_r[0] if n else 0.0] + cuts + [by_r[-1] if n else 0.0])
            else:
                edges = np.asarray(annuli, dtype=np.float64).reshape(-1)
                if edges.size < 2 or np.any(np.diff(edges) <= 0):
                    raise ValueError("annuli: the edges must increase")
                n_groups = edges.size - 1
                groups = np.searchsorted(edges, r, side="right") - 1
                groups[(r < edges[0]) | (r >= edges[-1])] = -1
            label = ("edges", edges)
        order = np.argsort(groups, kind="stable").astype(np.int64)
        order = order[groups[order] >= 0]
        counts = np.bincount(groups[order], minlength=n_groups)
        return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), order, label

    def replicate_check(self, chain, n_burn, thin=1, annuli=8, groups=None, seed=None):
        """Posterior predictive check with replicated data, per group of stars (Gelman, Meng & Stern 1996): for every
        post-burn-in sample of ``chain`` (handled as by ``posterior_predictive``) the device draws a replicated catalogue
        from the model at that sample and accumulates, per group, eight additive fields of the standardised residuals
        of the observed and of the replicated velocities (``Catalog.replicate_check``); ``replicate_summary`` turns them
        into discrepancies and p-values P(T_rep >= T_obs) for all grouped stars and for every group.
        ``groups``: an int array per star, -1 leaves the star out.  Otherwise ``annuli``: an int for that many annuli of
        equal star count in projected radius about the parameters' current centre value, or a list of edges in arcmin.
        Fixed-background classes draw background replicates from their ``background.Gaussian``.  Returns the entries of
        ``replicate_summary`` plus ``edges`` (arcmin) or ``groups`` (the labels), ``seed`` and ``n_samples``.
        NotImplementedError: a SingleStars background, several ranks or devices, float32 catalogues."""
        ctx = self._context
        if ctx is not None and getattr(ctx, "n_ranks", 1) > 1:
            raise NotImplementedError("Runner.replicate_check runs in one process on one device; this runner sits on a "
                                      "context of {0} ranks".format(ctx.n_ranks))
        if ctx is not None and int(getattr(ctx, "n_devices", 1)) > 1:
            raise NotImplementedError("Runner.replicate_check runs on one device; this runner's context has "
                                      "{0}".format(int(ctx.n_devices)))
        if self._precision != "f64":
            raise NotImplementedError("Runner.replicate_check needs a float64 catalogue")
        bg_mean, bg_sigma = self._replicate_background()
        offsets, order, label = self._replicate_groups(annuli, groups)
        if seed is None:
            seed = int(np.random.SeedSequence().entropy % (2 ** 63))
        table, n_samples = self._posterior_table(chain, n_burn, thin)
        fields = self._ensure_catalog().replicate_check(table, seed, offsets, order, bg_mean, bg_sigma)
        out = replicate_summary(fields, np.diff(offsets))
        out[label[0]] = label[1]
        out["seed"] = int(seed)
        out["n_samples"] = n_samples
        return out

    # ------------------------------------------------------------------ device catalogue
    # Sub-classes set `_model_id` and the ordered (name, canonical unit) columns of the kernel's parameter
    # table before (`_KERNEL_HEAD`) and after (`_KERNEL_TAIL`) the optional centre columns (include/mcd.h).
    _model_id = None
    _KERNEL_HEAD = ()
    _KERNEL_TAIL = ()

    def _canonical(self, resolved, name, unit):
        """Resolved column of parameter ``name`` expressed in the kernel's canonical unit."""
        f = units.conversion_factor(self.parameters[name].unit, unit) if self.parameters[name].unit else 1.0
        return resolved[name] if f == 1.0 else resolved[name] * f

    def _centre_is_fixed(self):
        pr, pd = self.parameters["ra_center"], self.parameters["dec_center"]
        return pr.fixed and pd.fixed and pr.expr is None and pd.expr is None

    def _catalog_model(self):
        """(model id, extra per-star columns) of the device catalogue."""
        return self._model_id, {}

    def _catalog_spec(self):
        """(key, constructor kwargs) of the device catalogue for the current parameter configuration:
        a fixed centre lets the walker-independent geometry be precomputed at upload."""
        if self._centre_is_fixed():
            centre = (float(units.to_unit(self.parameters["ra_center"].value, "deg", self.parameters["ra_center"].unit)),
                      float(units.to_unit(self.parameters["dec_center"].value, "deg", self.parameters["dec_center"].unit)))
        else:
            centre = None
        model, extra = self._catalog_model()
        return (model, centre), dict(model=model, centre=centre, **extra)

    def _catalog_kwargs(self):
        return {}

    def _ensure_catalog(self):
        plan = getattr(self, "_plan_cache", None)
        if (self._catalog is not None and plan is not None and self._plan_sig == _BatchPlan.signature(self)
                and plan.catalog_key == self._catalog_key):
            return self._catalog                          # nothing about the parameters changed since the plan was built
        key, spec = self._catalog_spec()
        if self._catalog is None or key != self._catalog_key:
            if self._catalog is not None:
                self._catalog.close()
            self._catalog = _native.Catalog(self.context, self.ra, self.dec, self.v, self.verr,
                                            precision=self._precision, **self._catalog_kwargs(), **spec)
            self._catalog_key = key
            if self._precision != "f64":
                # a chain must not end because one proposal leaves the float32 accuracy domain: evaluate regardless, and
                # tell (``_note_f32``)
                self._catalog.set_option("f32_domain", 0)
        return self._catalog

    def _note_f32(self, cat):
        """float32 catalogues: one ``UserWarning`` per catalogue, the first time it has staged a table outside the float32
        accuracy domain (in a direct evaluation or anywhere inside a library block)."""
        if getattr(self, "_f32_warned", None) is cat:
            return
        out = cat.f32_outside()
        if out["calls"]:
            self._f32_warned = cat
            warnings.warn("{0} (precision={1!r}): {2} evaluation(s) outside the float32 accuracy domain, where the stated "
                          "float32 tolerances do not hold: {3} (largest kappa_v = {4:.4g}, kappa_theta = {5:.4g} so far; "
                          "f32_outside() has the counters, precision='f64' evaluates exactly)".format(
                              type(self).__name__, self._precision, out["calls"], out["reason"], out["worst_kappa_v"],
                              out["worst_kappa_theta"]), UserWarning, stacklevel=3)

    def f32_outside(self):
        """Evaluations of this fit's current catalogue outside the float32 accuracy domain since it was created:
        ``{'calls', 'worst_kappa_v', 'worst_kappa_theta', 'reason'}`` (``_native.Catalog.f32_outside``).  Zeros for
        precision 'f64' and before the first evaluation."""
        if self._precision == "f64" or self._catalog is None:
            return {"calls": 0, "worst_kappa_v": 0.0, "worst_kappa_theta": 0.0, "reason": ""}
        return self._catalog.f32_outside()

    def _kernel_table(self, resolved):
        """(W, K) float64 table in the column order and canonical units the C-ABI expects."""
        cols = [self._canonical(resolved, n, u) for n, u in self._KERNEL_HEAD]
        if self._catalog_key[1] is None:
            cols += [self._canonical(resolved, "ra_center", "deg"), self._canonical(resolved, "dec_center", "deg")]
        cols += [self._canonical(resolved, n, u) for n, u in self._KERNEL_TAIL]
        return np.stack(cols, axis=1)

    def _lnlike_batch(self, resolved):
        cat = self._ensure_catalog()
        ll = cat.loglike(self._kernel_table(resolved))
        if self._precision != "f64":
            self._note_f32(cat)
        return ll

    def _per_star(self, values, what):
        """Per-star device outputs for ONE parameter vector: 'membership' or 'lnlike'."""
        resolved = self.parameters.resolve_batch(np.asarray(values, dtype=np.float64).reshape(1, -1))
        cat = self._ensure_catalog()
        row = self._kernel_table(resolved)[0]
        return cat.membership(row) if what == "membership" else cat.loglike_per_star(row)

    def close(self):
        if self._catalog is not None:
            self._catalog.close()
            self._catalog = None
            self._catalog_key = None

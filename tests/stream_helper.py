"""The small catalogue of tests/test_gpu_sampler_stream.py, and the check (tests/test_sampler_stream_cpu.py) that it sits
where those tests need it with respect to the float32 accuracy domain of csrc/mcd_guard.h.

N = 257 stars (ragged against 8-, 16- and 64-star iterations), W = 16 walkers.  Two configurations:

* inside: velocities centred, |v| <= 40 km/s, verr in [1, 3], walkers start at sigma in [5, 15]; the prior box (|v_sys|,
  |v_maxx|, |v_maxy| <= 15, 0 <= sigma <= 50) holds kappa_v = (max|v| + |v_sys| + |v_maxx| + |v_maxy|) / sqrt(min verr^2 +
  min sigma^2) at or below 85 / 1: EVERY table a chain can stage is inside the domain (kappa_v <= 96);
* outside: the same stars shifted by +300 km/s, walkers around v_sys = 300, the box shifted with them: kappa_v runs from
  about 40 (sigma = 15) to about 130 (sigma = 5) -- some tables inside, some outside.
"""
import numpy as np

N, W = 257, 16
NAMES = ["v_sys", "sigma_max", "v_maxx", "v_maxy"]
SHIFT = {"inside": 0.0, "outside": 300.0}
BG_SIGMA = 40.0


def centre():
    from mcmc_dynamics_amd import synthetic
    return (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)


def stars(config="inside"):
    """Columns ra, dec, v, verr, pmember: positions of the synthetic cluster, a 7 km/s dispersion, no rotation."""
    from mcmc_dynamics_amd import synthetic
    c = synthetic.make_catalog(N, config=2)
    rng = np.random.default_rng(20)
    verr = rng.uniform(1.0, 3.0, size=N)
    v = np.clip(7.0 * rng.normal(size=N) + verr * rng.normal(size=N), -40.0, 40.0)
    return {"ra": c["ra"], "dec": c["dec"], "v": v + SHIFT[config], "verr": verr, "pmember": rng.uniform(0.5, 0.95, size=N)}


def box(config="inside"):
    s = SHIFT[config]
    return {"v_sys": (s - 15.0, s + 15.0), "sigma_max": (0.0, 50.0), "v_maxx": (-15.0, 15.0), "v_maxy": (-15.0, 15.0)}


def walkers(config="inside", n=W, seed=21):
    rng = np.random.default_rng(seed)
    return np.column_stack([SHIFT[config] + rng.normal(size=n), rng.uniform(5.0, 15.0, size=n), 2.0 * rng.normal(size=n),
                            2.0 * rng.normal(size=n)])


def bins():
    """Three radial bins of 86, 86 and 85 stars: the ``bin`` column for ``stars()``."""
    from oracle import lnprob_numpy as oracle
    c = stars()
    r = np.hypot(*oracle.calc_xy_offset(c["ra"], c["dec"], *centre()))
    rank = np.empty(N, dtype=np.int64)
    rank[np.argsort(r, kind="stable")] = np.arange(N)
    return np.minimum(rank // 86, 2).astype(np.int16)


def make_fit(config="inside", background=False, precision="f64", binned=False, context=None, rows=None):
    """ConstantFit (or BinnedConstantFit over ``bins()``) on the configuration, fixed centre, the box as bounds.  ``rows``:
    the stars this fit holds (a rank's share), default all."""
    from mcmc_dynamics_amd import DataReader, Gaussian
    from mcmc_dynamics_amd.analysis import BinnedConstantFit, ConstantFit
    cols = stars(config)
    if not background:
        del cols["pmember"]
    if binned:
        cols["bin"] = bins()
    if rows is not None:
        cols = {k: v[rows] for k, v in cols.items()}
    kwargs = {"precision": precision, "context": context}
    if background:
        kwargs["background"] = Gaussian(SHIFT[config], BG_SIGMA)
    fit = (BinnedConstantFit if binned else ConstantFit)(DataReader(cols), **kwargs)
    fit.SAMPLER = "builtin"                                  # never emcee: the tests must not depend on its presence
    fit.parameters["ra_center"].set(value=centre()[0], fixed=True)
    fit.parameters["dec_center"].set(value=centre()[1], fixed=True)
    for name, (lo, hi) in box(config).items():
        fit.parameters[name].set(min=lo, max=hi)
    return fit


def domain_columns(config, background):
    """``stars()`` as tests/emul_helper.f32_domain wants them (model 1: with the fixed background's log-likelihood)."""
    from oracle import lnprob_numpy as oracle
    c = stars(config)
    if background:
        c["lnlike_bg"] = oracle.gaussian_background(c["v"], c["verr"], SHIFT[config], BG_SIGMA)
    else:
        del c["pmember"]
    return c

#!/usr/bin/env python3
"""Golden vectors for the double Lynden-Bell models (analysis/double_model.py), from the REFERENCE's own functions.

Run under the recipe at the top of oracle/make_golden.py (conda python 3.9, oracle/ref_shims and the reference on the
path), with tools/make_golden_double.py in place of oracle/make_golden.py.

The reference's own double_model.py no longer runs against its Runner, and its curve is not nested in ModelFit's.  What
is pinned here is the model this package defines: a subclass of the reference's ``ModelFit`` (and of ``ModelFitGB``)
whose ``rotation_model`` is TWO calls of the reference's ``ModelFit.rotation_model`` -- the second with v_sys = 0, the
``_c`` amplitudes and the peak radius r_peak_ratio * r_peak.  Priors, the dispersion profile, the Gaussian / mixture
likelihood, ``lnprob`` and the membership probabilities are the unmodified reference methods; every number written comes
out of them.

Outputs: tests/golden/double_model{,_free,_gb,_gb_free}.npz -- plain float64 arrays (and the parameter names).
"""
import importlib.util
import os
import sys

import numpy

numpy.asscalar = lambda a: a.item()     # removed in numpy 1.23; astropy 4.3.1 still references it
numpy.alen = len

import numpy as np                      # noqa: E402
from astropy import units as u          # noqa: E402

from mcmc_dynamics.analysis import ModelFit, ModelFitGB        # noqa: E402
from mcmc_dynamics.parameter import Parameters                 # noqa: E402
from mcmc_dynamics.utils.files import DataReader               # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")

_spec = importlib.util.spec_from_file_location("synthetic", os.path.join(REPO, "mcmc_dynamics_amd", "synthetic.py"))
synthetic = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(synthetic)

KMS = u.km / u.s
SECOND = ["v_maxx_c", "v_maxy_c", "r_peak_ratio"]


def two_components(self, v_sys, v_maxx, v_maxy, ra_center, dec_center, r_peak=None, v_maxx_c=0.0, v_maxy_c=0.0,
                   r_peak_ratio=1.0, **kwargs):
    outer = ModelFit.rotation_model(self, v_sys=v_sys, v_maxx=v_maxx, v_maxy=v_maxy, ra_center=ra_center,
                                    dec_center=dec_center, r_peak=r_peak, **kwargs)
    inner = ModelFit.rotation_model(self, v_sys=0.0 * KMS, v_maxx=v_maxx_c, v_maxy=v_maxy_c, ra_center=ra_center,
                                    dec_center=dec_center, r_peak=r_peak_ratio * r_peak)
    return outer + inner


class DoubleRef(ModelFit):
    MODEL_PARAMETERS = ModelFit.MODEL_PARAMETERS + SECOND
    rotation_model = two_components


class DoubleRefGB(ModelFitGB):
    MODEL_PARAMETERS = ModelFitGB.MODEL_PARAMETERS + SECOND
    rotation_model = two_components


def parameters_of(cls):
    pars = Parameters().load(cls.parameters_file)
    pars.add("v_maxx_c", unit="km/s", min=-50.0, max=50.0, initials="rng.normal(size=n)")
    pars.add("v_maxy_c", unit="km/s", min=-50.0, max=50.0, initials="rng.normal(size=n)")
    pars.add("r_peak_ratio", unit=u.dimensionless_unscaled, min=1e-3, max=1.0, initials="rng.uniform(size=n)")
    return pars


def reader(cat, extra=()):
    cols = {"ra": cat["ra"] * u.deg, "dec": cat["dec"] * u.deg, "v": cat["v"] * KMS, "verr": cat["verr"] * KMS}
    for name in extra:
        cols[name] = cat[name]
    return DataReader(cols)


def plain(x):
    return np.asarray(getattr(x, "value", x), dtype=np.float64)


def walkers(names, truth, n, seed):
    rng = np.random.default_rng(seed)
    pos = np.empty((n, len(names)))
    for j, name in enumerate(names):
        t = truth[name]
        g = rng.normal(size=n)
        if name in ("ra_center", "dec_center"):
            pos[:, j] = t + (0.05 / 60.0) * g
        elif name == "r_peak_ratio":
            pos[:, j] = np.clip(t * (1.0 + 0.3 * g), 0.02, 0.98)
        elif t == 0.0:
            pos[:, j] = 0.5 * g
        else:
            pos[:, j] = t * (1.0 + 0.05 * g)
    col = names.index
    # rows that sit on a bound (accepted: the bounds are inclusive) and rows the prior rejects
    pos[0, col("v_maxx_c")] = 0.0
    pos[0, col("v_maxy_c")] = 0.0                    # no second component: ModelFit itself
    pos[1, col("r_peak_ratio")] = 1.0                # both peaks at the same radius
    pos[2, col("r_peak_ratio")] = 1e-3               # lower bound
    pos[3, col("v_maxx_c")] = 50.0
    pos[-1, col("r_peak_ratio")] = 1.2               # rejected
    pos[-2, col("v_maxy_c")] = -50.5                 # rejected
    pos[-3, col("r_peak")] = -5.0                    # rejected
    pos[-4, col("r_peak_ratio")] = 5e-4              # rejected
    if "f_back" in names:
        pos[:, col("f_back")] = np.clip(pos[:, col("f_back")], 0.0, 1.0)
        pos[4, col("f_back")] = 0.0                  # accepted
        pos[-5, col("f_back")] = 1.2                 # rejected
    return pos


def main():
    ra_c, dec_c = synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG
    second = {"v_maxx_c": -4.0, "v_maxy_c": 2.5, "r_peak_ratio": 0.25}
    cat = synthetic.make_catalog(1500, config=2)
    cat["ra"][7], cat["dec"][7] = ra_c, dec_c            # a star exactly on the centre
    catb = synthetic.make_catalog(1500, config=3, background=True)
    for gb in (False, True):
        cls, c = (DoubleRefGB, catb) if gb else (DoubleRef, cat)
        truth = dict(c["truth"], a=30.0, r_peak=60.0, **second)
        for free in (False, True):
            obj = cls(reader(c, extra=("density",) if gb else ()), parameters=parameters_of(cls))
            if free:
                obj.parameters["ra_center"].set(value=ra_c * u.deg)
                obj.parameters["dec_center"].set(value=dec_c * u.deg)
            else:
                obj.parameters["ra_center"].set(value=ra_c * u.deg, fixed=True)
                obj.parameters["dec_center"].set(value=dec_c * u.deg, fixed=True)
            names = list(obj.fitted_parameters)
            pos = walkers(names, truth, 24, 51 + (2 if gb else 0) + (1 if free else 0))
            out = dict(ra=c["ra"], dec=c["dec"], v=c["v"], verr=c["verr"], ra_center=ra_c, dec_center=dec_c,
                       names=np.asarray(names).astype("U32"), values=pos,
                       lnprob=np.array([float(obj.lnprob(np.array(row))) for row in pos]),
                       lnprior=np.array([float(obj.lnprior(np.array(row))) for row in pos]))
            if gb:
                out["density"] = c["density"]
                rows = [5, 1, 2]                          # ModelFitGB.calculate_membership_probabilities at these rows
                member = []
                for i in rows:
                    chain = np.tile(pos[i], (2, 3, 1))     # a chain that is this row throughout: its median is the row
                    member.append(plain(obj.calculate_membership_probabilities(chain, n_burn=0)))
                out["membership_rows"] = np.asarray(rows, dtype=np.float64)
                out["membership"] = np.stack(member)
            name = "double_model" + ("_gb" if gb else "") + ("_free" if free else "")
            np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
            print("wrote", name, {k: tuple(np.shape(v)) for k, v in out.items()},
                  "finite rows:", int(np.isfinite(out["lnprob"]).sum()))
    with open(os.path.join(OUT, "PROVENANCE_double.txt"), "w") as f:
        import astropy
        f.write("double_model{{,_free,_gb,_gb_free}}.npz: tools/make_golden_double.py, python {0}, numpy {1}, astropy {2}\n"
                .format(sys.version.split()[0], np.__version__, astropy.__version__))


if __name__ == "__main__":
    main()

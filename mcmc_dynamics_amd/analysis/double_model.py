"""``DoubleModelFit`` / ``DoubleModelFitGB``: two Lynden-Bell rotation components on one Plummer dispersion profile, the
model of a decoupled or counter-rotating core (the reference has the family in analysis/double_model.py, written against
an older ``Runner`` and no longer runnable there; restated here on today's ``ModelFit``).

    cross_k = v_maxx_k dy - v_maxy_k dx          k = 1: (v_maxx, v_maxy),  k = 2: (v_maxx_c, v_maxy_c)
    rho_1   = r_peak,  rho_2 = r_peak_ratio r_peak                                                    [arcsec]
    v_los   = v_sys + sum_k 2 rho_k cross_k / (rho_k^2 + r^2)
    sigma_los(r) as ``ModelFit``

Each component has the form of ``ModelFit.rotation_model`` (r^2 in the denominator), so that ``v_maxx_c = v_maxy_c = 0``
IS ``ModelFit``: the two families are nested, which is what ``elpd_compare`` and ``bayes_factor`` between them need.
The reference orders the two peaks with a prior between two parameters, ``0 < r_peak_c <= r_peak``; here the free
parameter is the dimensionless ratio ``r_peak_ratio`` in [1e-3, 1], which makes the ordering a box (every device prior,
reflection and tempering ladder knows boxes) and removes the label-swap mode.  ``r_peak_c`` is derived
(``DoubleModelFit.r_peak_c``, and a band in ``create_profiles``).

Out of scope, refused with a message: a fixed ``background=`` instance, the constant-background form, float32
catalogues.  ``hmc`` / ``tempered`` take at most 12 free parameters (``DoubleModelFitGB`` with a fixed centre fits).
"""
import logging

import numpy as np

from .. import _native, units
from ..parameter import Parameter
from ..utils.coordinates import get_amplitude_and_angle
from ..utils.data_reader import ColumnTable
from .model import _MODEL_BG_ORDER, _MODEL_ORDER, ModelFit, _build

logger = logging.getLogger(__name__)

# name, unit, min, max, label, initials -- the second component; amplitudes within +-50 km/s as in the reference
_SECOND = (
    ("v_maxx_c", "km/s", -50.0, 50.0, r"$v_{\rm max,\,x}^{\rm c}$", "rng.normal(size=n)"),
    ("v_maxy_c", "km/s", -50.0, 50.0, r"$v_{\rm max,\,y}^{\rm c}$", "rng.normal(size=n)"),
    ("r_peak_ratio", None, 1e-3, 1.0, r"$r_{\rm peak}^{\rm c}/r_{\rm peak}$", "rng.uniform(0.1, 0.9, size=n)"),
)
_SECOND_NAMES = tuple(row[0] for row in _SECOND)


def _build_double(order):
    pars = _build(order)
    for name, unit, lo, hi, label, initials in _SECOND:
        pars.add(Parameter(name, unit=unit, min=lo, max=hi, label=label, initials=initials))
    return pars


class DoubleModelFit(ModelFit):
    """``ModelFit`` with a second, inner Lynden-Bell component (device model ``MODEL_DOUBLE``)."""

    MODEL_PARAMETERS = ModelFit.MODEL_PARAMETERS + list(_SECOND_NAMES)

    _default_order = _MODEL_ORDER
    _model_id = _native.MODEL_DOUBLE
    _KERNEL_HEAD = ModelFit._KERNEL_HEAD + (("v_maxx_c", "km/s"), ("v_maxy_c", "km/s"), ("r_peak_ratio", None))

    def __init__(self, data, parameters=None, **kwargs):
        if kwargs.get("background") is not None:
            raise NotImplementedError("{0}: a fixed background= instance is out of scope for the double Lynden-Bell "
                                      "models; use DoubleModelFitGB for a background fitted with the cluster"
                                      .format(type(self).__name__))
        if kwargs.get("precision", "f64") != "f64":
            raise NotImplementedError("{0}: the double Lynden-Bell models are float64 only (precision={1!r} is out of "
                                      "scope)".format(type(self).__name__, kwargs.get("precision")))
        super(DoubleModelFit, self).__init__(data=data, parameters=parameters, **kwargs)

    @classmethod
    def default_parameters(cls):
        """``ModelFit``'s parameters plus ``v_maxx_c``, ``v_maxy_c`` (+-50 km/s) and ``r_peak_ratio`` ([1e-3, 1])."""
        return _build_double(cls._default_order)

    # ------------------------------------------------------------------ host-side model functions
    def rotation_model(self, v_sys, v_maxx, v_maxy, ra_center, dec_center, r_peak=None, v_maxx_c=0.0, v_maxy_c=0.0,
                       r_peak_ratio=1.0, **kwargs):
        """v_los at every data point: ``ModelFit.rotation_model`` plus the same curve with the second amplitudes at the
        peak radius ``r_peak_ratio * r_peak``."""
        if kwargs:
            raise IOError('Unknown keyword argument(s) "{0}" for method {1}.rotation_model.'.format(
                ", ".join(kwargs.keys()), self.__class__.__name__))
        dx, dy = self._offsets_arcsec(ra_center, dec_center)
        r2 = dx ** 2 + dy ** 2
        rho_1 = np.median(np.sqrt(r2)) if r_peak is None else float(units.to_unit(r_peak, "arcsec"))
        rho_2 = r_peak_ratio * rho_1
        v_los = v_sys + 2.0 * rho_1 * (v_maxx * dy - v_maxy * dx) / (rho_1 ** 2 + r2)
        return v_los + 2.0 * rho_2 * (v_maxx_c * dy - v_maxy_c * dx) / (rho_2 ** 2 + r2)

    def _catalog_model(self):
        return self._model_id, {}

    # ------------------------------------------------------------------ post-processing
    def _chain_column(self, pars, name, unit):
        f = units.conversion_factor(self.parameters[name].unit, unit) if self.parameters[name].unit else 1.0
        return np.asarray(pars[name]) * f

    def r_peak_c(self, chain, n_burn):
        """Samples of the inner component's peak radius ``r_peak_ratio * r_peak`` [arcsec] from a chain."""
        pars = self.convert_to_parameters(chain, n_burn)
        return self._chain_column(pars, "r_peak_ratio", None) * self._chain_column(pars, "r_peak", "arcsec")

    def create_profiles(self, chains, n_burn, radii=None, filename=None):
        """Radial profiles with 1 / 3 sigma bands from a chain: ``v_rot`` the SUM of the two components' amplitude curves
        (signed along each component's own axis, as the reference adds them), ``v_rot_c`` the inner component alone,
        ``sigma``, and ``r_peak_c`` (the same five percentiles of the derived radius, constant over ``r``)."""
        pars = self.convert_to_parameters(chains, n_burn)
        v_max = np.hypot(self._chain_column(pars, "v_maxx", "km/s"), self._chain_column(pars, "v_maxy", "km/s"))
        v_max_c = np.hypot(self._chain_column(pars, "v_maxx_c", "km/s"), self._chain_column(pars, "v_maxy_c", "km/s"))
        r_peak = self._chain_column(pars, "r_peak", "arcsec")
        r_peak_c = self._chain_column(pars, "r_peak_ratio", None) * r_peak
        sigma_max, a = self._chain_column(pars, "sigma_max", "km/s"), self._chain_column(pars, "a", "arcsec")
        radii = np.logspace(-1, 2.5, 50) if radii is None else np.atleast_1d(units.to_unit(radii, "arcsec"))
        rr = radii[:, np.newaxis]
        v_rot_c = 2.0 * r_peak_c * v_max_c * rr / (r_peak_c ** 2 + rr ** 2)
        v_rot = 2.0 * r_peak * v_max * rr / (r_peak ** 2 + rr ** 2) + v_rot_c
        sigma = sigma_max / (1.0 + rr ** 2 / a ** 2) ** 0.25
        levels = [50, 16, 84, 0.15, 99.85]
        names = ("", "_lower_1s", "_upper_1s", "_lower_3s", "_upper_3s")
        table = {"r": radii}
        for key, samples in (("v_rot", v_rot), ("v_rot_c", v_rot_c), ("sigma", sigma)):
            p = np.percentile(samples, levels, axis=-1)
            table.update({key + n: p[i] for i, n in enumerate(names)})
        pc = np.percentile(r_peak_c, levels)
        table.update({"r_peak_c" + n: np.full(radii.shape, pc[i]) for i, n in enumerate(names)})
        unit_of = {k: ("arcsec" if k == "r" or k.startswith("r_peak_c") else "km/s") for k in table}
        profile = ColumnTable(table, units_=unit_of)
        if filename is not None:
            np.savetxt(filename, np.stack([profile[k] for k in profile.columns], axis=1), delimiter=",",
                       header=",".join(profile.columns), comments="")
        return profile

    def compute_theta_vmax(self, chain, n_burn, return_samples=False, component=1):
        """Position angle and amplitude of one component's rotation field from a chain: ``component=1`` the outer one
        (``ModelFit.compute_theta_vmax``), ``component=2`` the inner one from ``v_maxx_c`` / ``v_maxy_c``."""
        if component == 1:
            return super(DoubleModelFit, self).compute_theta_vmax(chain, n_burn, return_samples=return_samples)
        if component != 2:
            raise ValueError("component must be 1 (outer) or 2 (inner)")
        pars = self.convert_to_parameters(chain=chain, n_burn=n_burn)
        inner = {"v_maxx": pars["v_maxx_c"], "v_maxy": pars["v_maxy_c"]}
        results, v_max, theta = get_amplitude_and_angle(inner, return_samples=return_samples)
        if results is None:
            logger.error("Could not recover paramaters of rotation field in %s.compute_theta_vmax().",
                         self.__class__.__name__)
            return None
        results.units["v_max"] = self.units["v_maxx_c"]
        if return_samples:
            return results, v_max, theta, pars["sigma_max"]
        return results


class DoubleModelFitGB(DoubleModelFit):
    """``DoubleModelFit`` plus the per-walker Gaussian background (v_back, sigma_back, f_back) and the ``density``
    membership prior of ``ModelFitGB`` (device model ``MODEL_DOUBLE_BGGAUSS``)."""

    MODEL_PARAMETERS = DoubleModelFit.MODEL_PARAMETERS + ["v_back", "sigma_back", "f_back"]
    OBSERVABLES = dict(DoubleModelFit.OBSERVABLES, **{"density": None})

    _default_order = _MODEL_BG_ORDER
    _model_id = _native.MODEL_DOUBLE_BGGAUSS
    _KERNEL_TAIL = (("v_back", "km/s"), ("sigma_back", "km/s"), ("f_back", None))

    def __init__(self, data, parameters=None, **kwargs):
        self.density = None
        super(DoubleModelFitGB, self).__init__(data=data, parameters=parameters, **kwargs)

    def _catalog_model(self):
        return self._model_id, {"density": self.density}

    def calculate_membership_probabilities(self, chain, n_burn):
        """Posterior membership probability of every star at the chain's median parameters."""
        bestfit = self.compute_bestfit_values(chain=chain, n_burn=n_burn)
        median = np.array([bestfit.loc["median"][name] for name in self.fitted_parameters])
        return self.membership_probabilities(median)

    def membership_probabilities(self, values):
        return self._per_star(values, "membership")

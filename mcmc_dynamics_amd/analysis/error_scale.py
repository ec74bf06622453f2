"""``ConstantFitES`` / ``ModelFitES``: ``ConstantFit`` / ``ModelFit`` with a fitted velocity-error scale.

    variance_i = err_scale^2 verr_i^2 + sigma_los^2(r_i)            v_los as the base class

``err_scale`` is dimensionless, one value per walker, in the box [0.1, 10] by default; it is the nuisance parameter that
radial-velocity work fits along with the kinematics when the stated errors may be wrong, so that ``sigma_max`` is
marginalised over it.  ``bootstrap()``, ``bagged()`` and ``sbc()`` diagnose wrongly stated errors; these classes fit them.

With ``err_scale`` fixed at 1 the classes ARE their base classes, bit for bit (device models ``MODEL_CONST_ESCALE`` /
``MODEL_PROFILE_ESCALE`` form the variance as ``fma(err_scale^2, verr^2, sigma_max^2)`` and ``fma(sigma_max^2 a, t,
err_scale^2 verr^2)``): ``elpd_compare``, ``bayes_factor`` and ``lrt(null)`` between the two are nested comparisons.  No
prior is set by default; ``Parameter.prior`` (for example a log-normal about 0) works as for every other parameter.

Out of scope, refused with a message: backgrounds of every kind (the fixed background column is computed from ``verr`` at
upload; the per-walker Gaussian background is a follow-up), float32 catalogues, radial bins (``BinnedConstantFit``).
"""
import numpy as np

from .. import _native
from ..parameter import Parameter
from .constant import ConstantFit
from .model import ModelFit

_ERR_SCALE = dict(value=1.0, unit=None, min=0.1, max=10.0, label=r"$s_{\rm err}$", initials="rng.uniform(0.8, 1.2, size=n)")

_HALF_LN_2PI = 0.5 * np.log(2.0 * np.pi)


def _refuse(self, kwargs):
    name = type(self).__name__
    if kwargs.get("background") is not None:
        raise NotImplementedError("{0}: a background= instance is out of scope for the error-scale models (the fixed "
                                  "background column is computed from verr when the catalogue is uploaded)".format(name))
    if kwargs.get("precision", "f64") != "f64":
        raise NotImplementedError("{0}: the error-scale models are float64 only (precision={1!r} is out of scope)"
                                  .format(name, kwargs.get("precision")))
    from .binned import BinnedConstantFit
    if isinstance(self, BinnedConstantFit):
        raise NotImplementedError("{0}: radial bins (BinnedConstantFit) are out of scope for the error-scale models"
                                  .format(name))


class _ErrorScale(object):
    """What the two classes share: the parameter, the refusals, the host restatement and the accessor."""

    @classmethod
    def default_parameters(cls):
        """The base class's parameters plus ``err_scale`` (initial value 1, box [0.1, 10], initials uniform in
        [0.8, 1.2], no prior)."""
        pars = super(_ErrorScale, cls).default_parameters()
        pars.add(Parameter("err_scale", **_ERR_SCALE))
        return pars

    def _catalog_model(self):
        return self._model_id, {}

    def lnlike_host(self, values):
        """The log-likelihood of one parameter vector in NumPy on the host, from the class's own ``rotation_model`` and
        ``dispersion_model`` with the error column multiplied by ``err_scale`` -- the reference's expressions, for
        inspection; ``lnlike`` evaluates the same on the device."""
        current = self.fetch_parameter_values(np.asarray(values, dtype=np.float64).reshape(-1))
        s = current.pop("err_scale")
        profile = isinstance(self, ModelFit)
        rot = {k: current[k] for k in ("v_sys", "v_maxx", "v_maxy", "ra_center", "dec_center")}
        disp = {"sigma_max": current["sigma_max"]}
        if profile:
            rot["r_peak"] = current["r_peak"]
            disp.update(a=current["a"], ra_center=current["ra_center"], dec_center=current["dec_center"])
        v_los = self.rotation_model(**rot)
        sigma_los = self.dispersion_model(**disp)
        verr = s * np.asarray(self.verr, dtype=np.float64)
        norm = verr * verr + sigma_los * sigma_los
        d = np.asarray(self.v, dtype=np.float64) - v_los
        return float(np.sum(-0.5 * np.log(norm) - 0.5 * d * d / norm - _HALF_LN_2PI))

    def err_scale(self, chain, n_burn):
        """Samples of ``err_scale`` from a chain (walkers, steps, P) after ``n_burn`` steps."""
        return np.asarray(self.convert_to_parameters(chain, n_burn)["err_scale"])


class ConstantFitES(_ErrorScale, ConstantFit):
    """``ConstantFit`` with the velocity-error scale ``err_scale`` (device model ``MODEL_CONST_ESCALE``)."""

    MODEL_PARAMETERS = ConstantFit.MODEL_PARAMETERS + ["err_scale"]

    _model_id = _native.MODEL_CONST_ESCALE
    _KERNEL_HEAD = ConstantFit._KERNEL_HEAD + (("err_scale", None),)

    def __init__(self, data, parameters=None, **kwargs):
        _refuse(self, kwargs)
        super(ConstantFitES, self).__init__(data=data, parameters=parameters, **kwargs)


class ModelFitES(_ErrorScale, ModelFit):
    """``ModelFit`` with the velocity-error scale ``err_scale`` (device model ``MODEL_PROFILE_ESCALE``)."""

    MODEL_PARAMETERS = ModelFit.MODEL_PARAMETERS + ["err_scale"]

    _model_id = _native.MODEL_PROFILE_ESCALE
    _KERNEL_HEAD = ModelFit._KERNEL_HEAD + (("err_scale", None),)

    def __init__(self, data, parameters=None, **kwargs):
        _refuse(self, kwargs)
        super(ModelFitES, self).__init__(data=data, parameters=parameters, **kwargs)

"""Test helper: an independent NumPy restatement of the double Lynden-Bell models (device models 7 and 8,
analysis/double_model.py) in float64 or numpy.longdouble: value, per-star terms, membership, gradient.  Test
infrastructure only.

The value is written the way the golden vectors were made (tools/make_golden_double.py): the line-of-sight velocity is
TWO calls of the oracle's ``model_rotation`` (oracle/lnprob_numpy.py, the reference's own expression with theta and x_pa),
the second with v_sys = 0, the ``_c`` amplitudes and the peak radius r_peak_ratio * r_peak; dispersion, Gaussian term and
log-sum-exp mixture are the oracle's.  With zero second amplitudes the second call returns exact zeros and the value IS
the oracle's ModelFit value.  The gradient is written in the style of grad_helper.per_star (arcmin offsets, the factors
3600 and 120 of the units trap) with two components; it shares no expression with csrc/mcd_grad.h, which works in arcsec
on packed records with the component sum over one shared reciprocal (csrc/mcd_math.h: star_d_n).

Column order (include/mcd.h): v_sys, sigma_max, a, v_maxx, v_maxy, r_peak, v_maxx_c, v_maxy_c, r_peak_ratio
[, ra_center, dec_center] [, v_back, sigma_back, f_back]."""
import numpy as np

import emul_helper as eh
import variant_helper as vh
from oracle import lnprob_numpy as oracle

L = vh.L
DOUBLE, DOUBLE_GB = 7, 8
MODELS = (DOUBLE, DOUBLE_GB)
BASE = {DOUBLE: 3, DOUBLE_GB: 4}                 # the single-component model each one reduces to
HEAD = eh.DOUBLE_HEAD                             # the column list exists once, in emul_helper
GEOMETRY_COLUMNS = ("v_maxx", "v_maxy", "r_peak", "v_maxx_c", "v_maxy_c", "r_peak_ratio", "ra_center", "dec_center")


def n_columns(model, free):
    return 9 + (2 if free else 0) + (3 if model == DOUBLE_GB else 0)


def column_names(model, free):
    return HEAD + (["ra_center", "dec_center"] if free else []) + (["v_back", "sigma_back", "f_back"] if model == DOUBLE_GB else [])


def abi_columns(names, values, model, free):
    """Golden `values` (columns named `names`, the reference's ordering) in the C-ABI order."""
    names = [str(n) for n in names]
    return np.ascontiguousarray(np.asarray(values)[:, [names.index(k) for k in column_names(model, free)]])


def make_case(model, free, n, seed=None):
    """vh.make_case of the single-component counterpart with the three columns of the second component inserted: amplitudes
    of the size of the first component's, r_peak_ratio uniform within [0.05, 1]."""
    case = vh.make_case(BASE[model], free, n, seed=seed)
    rng = np.random.default_rng(7000000 + 100000 * model + 50000 * int(free) + n if seed is None else seed + 1)
    p, sv, w = case["params"], case["scale"], case["params"].shape[0]
    extra = np.stack([rng.normal(0, 0.3 * sv, w), rng.normal(0, 0.3 * sv, w), rng.uniform(0.05, 1.0, w)], axis=1)
    case["params"] = np.ascontiguousarray(np.concatenate([p[:, :6], extra, p[:, 6:]], axis=1))
    case["base_model"] = BASE[model]
    case["model"] = model
    return case


def nested_rows(params):
    """(rows with zero second amplitudes, the same rows without the second component's three columns)."""
    p = np.array(params, copy=True)
    p[:, 6:8] = 0.0
    return np.ascontiguousarray(p), np.ascontiguousarray(np.delete(p, [6, 7, 8], axis=1))


def column_scales(model, free, row, scale):
    out = []
    for name, value in zip(column_names(model, free), row):
        if name in ("a", "r_peak"):
            out.append(abs(float(value)))
        elif name in ("ra_center", "dec_center"):
            out.append(0.01)
        elif name in ("f_back", "r_peak_ratio"):
            out.append(1.0)
        else:
            out.append(float(scale))
    return np.array(out)


def _split(row, centre, dtype):
    row = np.asarray(row).astype(dtype)
    if centre is None:
        return row[:9], row[9], row[10], row[11:]
    return row[:9], dtype(centre[0]), dtype(centre[1]), row[9:]


def per_star(model, cat, row, centre, dtype=L):
    """(per-star log-likelihood, membership probability or None for model 7) of one row in `dtype`."""
    c = {k: np.asarray(v).astype(dtype) for k, v in cat.items()}
    head, rc, dc, tail = _split(row, centre, dtype)
    v_sys, sigma, a, vx, vy, rp, vxc, vyc, ratio = head
    v_los = oracle.model_rotation(c["ra"], c["dec"], v_sys, vx, vy, rp, rc, dc) + \
        oracle.model_rotation(c["ra"], c["dec"], dtype(0), vxc, vyc, ratio * rp, rc, dc)
    sig = oracle.model_dispersion(c["ra"], c["dec"], sigma, a, rc, dc)
    norm = c["verr"] * c["verr"] + sig * sig
    lc = -0.5 * np.log(2. * np.pi * norm) - 0.5 * np.power(c["v"] - v_los, 2) / norm
    if model == DOUBLE:
        assert lc.dtype == dtype
        return lc, None
    lb = oracle.gaussian_background(c["v"], c["verr"], tail[0], tail[1])
    m = c["density"] / (c["density"] + tail[2])
    mx = np.maximum(lc, lb)
    ec, eb = m * np.exp(lc - mx), (1. - m) * np.exp(lb - mx)
    assert lc.dtype == dtype and ec.dtype == dtype
    return mx + np.log(ec + eb), ec / (ec + eb)


def value(model, cat, row, centre, dtype=np.float64):
    return per_star(model, cat, row, centre, dtype)[0].sum()


def exact(model, cat, row, centre):
    return value(model, cat, row, centre, L)


def grad_terms(model, cat, row, centre, dtype=L):
    """(K, N) array of d lnL_i / d theta_k for one row (C-ABI column order)."""
    c = {k: np.asarray(v).astype(dtype) for k, v in cat.items()}
    free = centre is None
    head, rc, dc, tail = _split(row, centre, dtype)
    v_sys, sigma, a, vx, vy, rp, vxc, vyc, ratio = head
    one, half = dtype(1), dtype(0.5)
    pi = np.arctan(dtype(1)) * 4
    deg = pi / dtype(180)
    r0 = dtype(10800) / pi
    ra, dec, v, verr = c["ra"], c["dec"], c["v"], c["verr"]
    dra = (ra - rc) * deg
    dx = -r0 * np.cos(dec * deg) * np.sin(dra)
    dy = r0 * (np.sin(dec * deg) * np.cos(dc * deg) - np.cos(dec * deg) * np.sin(dc * deg) * np.cos(dra))
    dx_ra = r0 * np.cos(dec * deg) * np.cos(dra) * deg
    dy_ra = -r0 * np.cos(dec * deg) * np.sin(dc * deg) * np.sin(dra) * deg
    dy_dec = -r0 * (np.sin(dec * deg) * np.sin(dc * deg) + np.cos(dec * deg) * np.cos(dc * deg) * np.cos(dra)) * deg
    rr = dx * dx + dy * dy                                                      # arcmin^2

    def component(ux, uy, rho):
        """v_los contribution and its partials with respect to (ux, uy, rho, dx, dy)."""
        cross = ux * dy - uy * dx
        big_d = one + dtype(3600) * rr / (rho * rho)
        val = dtype(120) * cross / (rho * big_d)
        d_ux, d_uy = dtype(120) * dy / (rho * big_d), -dtype(120) * dx / (rho * big_d)
        d_rho = -dtype(120) * cross * (one - dtype(3600) * rr / (rho * rho)) / (rho * rho * big_d * big_d)
        d_dx = dtype(120) / rho * (-uy / big_d - cross * dtype(7200) * dx / (rho * rho) / (big_d * big_d))
        d_dy = dtype(120) / rho * (ux / big_d - cross * dtype(7200) * dy / (rho * rho) / (big_d * big_d))
        return val, d_ux, d_uy, d_rho, d_dx, d_dy

    rho2 = ratio * rp
    c1, c2 = component(vx, vy, rp), component(vxc, vyc, rho2)
    v_los = v_sys + c1[0] + c2[0]
    big_e = one + dtype(3600) * rr / (a * a)
    norm = verr * verr + sigma * sigma / np.sqrt(big_e)
    vl = {"v_sys": one + 0 * v, "v_maxx": c1[1], "v_maxy": c1[2], "v_maxx_c": c2[1], "v_maxy_c": c2[2],
          "r_peak": c1[3] + ratio * c2[3], "r_peak_ratio": rp * c2[3]}
    nn = {"sigma_max": 2 * sigma / np.sqrt(big_e), "a": sigma * sigma * dtype(3600) * rr / (a ** 3 * big_e ** dtype(1.5))}
    if free:
        vl_dx, vl_dy = c1[4] + c2[4], c1[5] + c2[5]
        n_dx = -half * sigma * sigma * big_e ** dtype(-1.5) * dtype(7200) * dx / (a * a)
        n_dy = -half * sigma * sigma * big_e ** dtype(-1.5) * dtype(7200) * dy / (a * a)
        vl["ra_center"], vl["dec_center"] = vl_dx * dx_ra + vl_dy * dy_ra, vl_dy * dy_dec
        nn["ra_center"], nn["dec_center"] = n_dx * dx_ra + n_dy * dy_ra, n_dy * dy_dec
    resid = v - v_los
    lc_d = -resid / norm
    lc_n = half * (resid * resid / (norm * norm) - one / norm)
    names = column_names(model, free)
    out = np.zeros((len(names), len(v)), dtype=dtype)
    for k, name in enumerate(names):
        if name in vl:
            out[k] += lc_d * (-vl[name])
        if name in nn:
            out[k] += lc_n * nn[name]
    if model == DOUBLE:
        return out
    lc = -half * np.log(2 * pi * norm) - half * resid * resid / norm
    v_back, sigma_back, f_back = tail
    nb = verr * verr + sigma_back * sigma_back
    db = v - v_back
    lb = -half * np.log(2 * pi * nb) - half * db * db / nb
    rho = c["density"]
    m = rho / (rho + f_back)
    mx = np.maximum(lc, lb)
    ec, eb = np.exp(lc - mx), np.exp(lb - mx)
    tot = m * ec + (one - m) * eb
    gamma, rest = m * ec / tot, (one - m) * eb / tot
    out *= gamma
    out[names.index("v_back")] = rest * db / nb
    out[names.index("sigma_back")] = rest * sigma_back * (db * db / (nb * nb) - one / nb)
    out[names.index("f_back")] = (ec - eb) / tot * (-rho / ((rho + f_back) * (rho + f_back)))
    assert out.dtype == dtype
    return out


def grad(model, cat, row, centre, dtype=L):
    terms = grad_terms(model, cat, row, centre, dtype)
    return terms.sum(axis=1), np.abs(terms).sum(axis=1)


_cache = {}


def reference(case, w):
    """{"g", "s", "err64", "value"} of walker row w of `case`, computed once: the longdouble gradient, its scale S_k, what
    the float64 run of the same restatement loses against it, and the longdouble value."""
    key = (case["model"], case["free"], case["n"], w, case["params"][w].tobytes(), case["cat"]["v"].tobytes(),
           case["cat"]["ra"].tobytes())
    if key not in _cache:
        args = (case["model"], case["cat"], case["params"][w], case["centre"])
        g80, s80 = grad(*args, L)
        g64, _ = grad(*args, np.float64)
        from grad_helper import col_err
        _cache[key] = {"g": g80, "s": s80, "err64": col_err(g64, g80, s80), "value": exact(*args)}
    return _cache[key]


def floors(model, free, n):
    """grad_bounds.floors of the single-component counterpart at the same cell; the second component's columns are
    geometry columns like the first's."""
    import grad_bounds as gb
    base = BASE[model]
    geometry, other = (gb.FREE_FLOOR.get((base, n), (gb.FLOOR, gb.FLOOR)) if free else (gb.FLOOR, gb.FLOOR))
    return np.array([geometry if name in GEOMETRY_COLUMNS else other for name in column_names(model, free)])


# ---- host build of the kernels' arithmetic (tests/emul/double_emul.cpp): records and derived walker rows --------------
def pack_records(cat, model, centre):
    """The records of the single-component counterpart: the double models read the same fields."""
    return eh.pack_records(cat, BASE[model], centre)


def pack_walkers(params, model, free, kd):
    """csrc/mcd_prep.h: walker_constants for the double models, on a row of `kd` values."""
    return eh.pack_double_walkers(params, model, free, kd)

"""Test helper: an independent NumPy restatement of the analytic log-likelihood gradient (tests/test_grad_*.py,
tests/test_gpu_grad*.py, tests/test_gpu_map.py).  Test infrastructure only.

Written from the reference's formulas in the reference's own variables, as variant_helper.per_star writes the value:
offsets dx, dy in arcmin from calc_xy_offset, theta = arctan2(dy, dx), v_los = v_sys + v_maxx sin(theta) - v_maxy
cos(theta) (constant.py:106-111), the profile's v_los = v_sys + 120 (cross / r_peak) / (1 + 3600 r^2 / r_peak^2) and
sigma_los = sigma_max (1 + 3600 r^2 / a^2)^(-1/4) (model.py:127, 180), the log-sum-exp mixture of runner.py:280-284.  It
shares no expression with csrc/mcd_grad.h (which works in arcsec / radians on packed records) and runs in float64 or
numpy.longdouble.  test_grad_oracle_cpu.py pins it to central differences of the 80-bit value oracle."""
import numpy as np

from variant_helper import BG_FIXED, BG_FIXED_DENSITY, BG_GAUSS, BG_NONE, BG_OF, L, PROFILE_MODELS, _split


def n_columns(model, free):
    return (6 if model in PROFILE_MODELS else 4) + (2 if free else 0) + {BG_NONE: 0, BG_FIXED: 0, BG_GAUSS: 3,
                                                                         BG_FIXED_DENSITY: 1}[BG_OF[model]]


def column_names(model, free):
    prof = model in PROFILE_MODELS
    names = ["v_sys", "sigma_max"] + (["a"] if prof else []) + ["v_maxx", "v_maxy"] + (["r_peak"] if prof else [])
    if free:
        names += ["ra_center", "dec_center"]
    return names + {BG_NONE: [], BG_FIXED: [], BG_GAUSS: ["v_back", "sigma_back", "f_back"],
                    BG_FIXED_DENSITY: ["f_back"]}[BG_OF[model]]


def column_scales(model, free, row, scale):
    """The natural size of each column of `row`: the catalogue's velocity scale, the row's own a and r_peak, 0.01 deg for
    the centre (the closest star of make_case), 1 for f_back."""
    out = []
    for name, value in zip(column_names(model, free), row):
        if name in ("a", "r_peak"):
            out.append(abs(float(value)))
        elif name in ("ra_center", "dec_center"):
            out.append(0.01)
        elif name == "f_back":
            out.append(1.0)
        else:
            out.append(float(scale))
    return np.array(out)


def per_star(model, cat, row, centre, dtype=L):
    """(K, N) array of d lnL_i / d theta_k for one walker row (C-ABI column order), every input cast to `dtype`.  A star
    exactly on a free centre of a constant-rotation model (theta undefined) gets 0 in the two centre columns."""
    c = {k: np.asarray(v).astype(dtype) for k, v in cat.items()}
    free = centre is None
    head, rc, dc, tail = _split(model, row, centre, dtype)
    prof = model in PROFILE_MODELS
    one, half = dtype(1), dtype(0.5)
    pi = np.arctan(dtype(1)) * 4
    deg = pi / dtype(180)
    r0 = dtype(10800) / pi
    ra, dec, v, verr = c["ra"], c["dec"], c["v"], c["verr"]
    dra = (ra - rc) * deg
    dx = -r0 * np.cos(dec * deg) * np.sin(dra)                                                    # calc_xy_offset.py:30
    dy = r0 * (np.sin(dec * deg) * np.cos(dc * deg) - np.cos(dec * deg) * np.sin(dc * deg) * np.cos(dra))     # :31
    # offsets with respect to the centre (per degree)
    dx_ra = r0 * np.cos(dec * deg) * np.cos(dra) * deg
    dy_ra = -r0 * np.cos(dec * deg) * np.sin(dc * deg) * np.sin(dra) * deg
    dy_dec = -r0 * (np.sin(dec * deg) * np.sin(dc * deg) + np.cos(dec * deg) * np.cos(dc * deg) * np.cos(dra)) * deg
    rr = dx * dx + dy * dy
    if prof:
        v_sys, sigma, a, vx, vy, rp = head
        cross = vx * dy - vy * dx
        big_d = one + dtype(3600) * rr / (rp * rp)
        v_los = v_sys + dtype(120) * cross / (rp * big_d)
        big_e = one + dtype(3600) * rr / (a * a)
        norm = verr * verr + sigma * sigma / np.sqrt(big_e)
        vl = {"v_sys": one + 0 * v, "v_maxx": dtype(120) * dy / (rp * big_d), "v_maxy": -dtype(120) * dx / (rp * big_d),
              "r_peak": -dtype(120) * cross * (one - dtype(3600) * rr / (rp * rp)) / (rp * rp * big_d * big_d)}
        nn = {"sigma_max": 2 * sigma / np.sqrt(big_e), "a": sigma * sigma * dtype(3600) * rr / (a ** 3 * big_e ** dtype(1.5))}
        vl_dx = dtype(120) / rp * (-vy / big_d - cross * dtype(7200) * dx / (rp * rp) / (big_d * big_d))
        vl_dy = dtype(120) / rp * (vx / big_d - cross * dtype(7200) * dy / (rp * rp) / (big_d * big_d))
        n_dx = -half * sigma * sigma * big_e ** dtype(-1.5) * dtype(7200) * dx / (a * a)
        n_dy = -half * sigma * sigma * big_e ** dtype(-1.5) * dtype(7200) * dy / (a * a)
    else:
        v_sys, sigma, vx, vy = head
        theta = np.arctan2(dy, dx)
        st, ct = np.sin(theta), np.cos(theta)
        v_los = v_sys + vx * st - vy * ct
        norm = verr * verr + sigma * sigma + 0 * v
        vl = {"v_sys": one + 0 * v, "v_maxx": st, "v_maxy": -ct}
        nn = {"sigma_max": 2 * sigma + 0 * v}
        safe = np.where(rr > 0, rr, one)
        vl_theta = np.where(rr > 0, vx * ct + vy * st, 0 * v)
        vl_dx, vl_dy = vl_theta * (-dy / safe), vl_theta * (dx / safe)
        n_dx = n_dy = 0 * v
    if free:
        vl["ra_center"], vl["dec_center"] = vl_dx * dx_ra + vl_dy * dy_ra, vl_dy * dy_dec
        nn["ra_center"], nn["dec_center"] = n_dx * dx_ra + n_dy * dy_ra, n_dy * dy_dec
    resid = v - v_los
    lc_d = -resid / norm                                   # d lc / d (v - v_los)
    lc_n = half * (resid * resid / (norm * norm) - one / norm)
    names = column_names(model, free)
    out = np.zeros((len(names), len(v)), dtype=dtype)
    for k, name in enumerate(names):
        if name in vl:
            out[k] += lc_d * (-vl[name])
        if name in nn:
            out[k] += lc_n * nn[name]
    bg = BG_OF[model]
    if bg == BG_NONE:
        return out
    lc = -half * np.log(2 * pi * norm) - half * resid * resid / norm
    if bg == BG_GAUSS:
        v_back, sigma_back, f_back = tail
        nb = verr * verr + sigma_back * sigma_back
        db = v - v_back
        lb = -half * np.log(2 * pi * nb) - half * db * db / nb
    else:
        lb = c["lnlike_bg"]
    m = c["pmember"] if bg == BG_FIXED else c["density"] / (c["density"] + tail[-1])
    mx = np.maximum(lc, lb)
    ec, eb = np.exp(lc - mx), np.exp(lb - mx)
    tot = m * ec + (one - m) * eb
    gamma, rest = m * ec / tot, (one - m) * eb / tot
    out *= gamma
    if bg == BG_GAUSS:
        out[names.index("v_back")] = rest * db / nb
        out[names.index("sigma_back")] = rest * sigma_back * (db * db / (nb * nb) - one / nb)
    if bg in (BG_GAUSS, BG_FIXED_DENSITY):
        rho, f_back = c["density"], tail[-1]
        out[names.index("f_back")] = (ec - eb) / tot * (-rho / ((rho + f_back) * (rho + f_back)))
    assert out.dtype == dtype
    return out


def grad(model, cat, row, centre, dtype=L):
    """(g, S): the gradient g_k = sum_i d lnL_i / d theta_k and S_k = sum_i |d lnL_i / d theta_k|, the scale against which
    a cancelling sum is judged."""
    terms = per_star(model, cat, row, centre, dtype)
    return terms.sum(axis=1), np.abs(terms).sum(axis=1)


def col_err(got, want, scale):
    """|got - want| / S_k per column, as float64."""
    got, want, scale = (np.asarray(a, dtype=L) for a in (got, want, scale))
    return (np.abs(got - want) / np.where(scale > 0, scale, L(1))).astype(np.float64)     # (S_k = 0: absolute)

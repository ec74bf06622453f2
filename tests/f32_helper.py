"""Test helper: inputs inside the float32 accuracy domain, for the float32 matrix (tests/test_f32_emul_cpu.py on the host
build tests/emul/f32_emul.cpp, tests/test_gpu_f32_matrix.py on the device).  Test infrastructure only.

variant_helper.make_case is outside the domain of csrc/mcd_guard.h: f32_domain for most cells -- its compact catalogues
with a free centre have kappa_theta ~ 5e-4 (bound 2e-5), and the profile models with `a` down to 3 arcsec and errors down
to 0.1 velocity scales have kappa_v > 96.  f32_case() moves it inside:
  * verr within 0.3 .. 0.6 velocity scales (lnlike_bg recomputed from it);
  * a and r_peak within 30 .. 100 arcsec for the profile models;
  * free centre: separations |N(0, 0.5 deg)| + 0.1 deg from CENTRE and both rotation amplitudes x 0.03 (the wide, slow
    field of tests/test_guard_random_cpu.py: test_float32_accuracy_domain, with more room).  kappa_theta = (rotation /
    sqrt(n_min)) 2^-23 / sep_harm: every separation is >= 0.1 deg = 1.7e-3 rad, the largest |v_maxx| + |v_maxy| of 257 rows
    drawn from 0.03 N(0, 0.3 scale) stays below 0.06 scales (6.7 sigma) and sqrt(n_min) >= 0.3 scales (verr alone), so kappa_theta <=
    1.4e-5 whatever the draw -- with a floor of 0.05 deg and a factor 0.05, catalogues of 3 stars came out at 2.1e-5 .. 2.7e-5;
  * RANGES: the velocity scale within 10^0.5 .. 10^1.5 instead of 10^0.5 .. 10^2, every velocity (v, verr, v_sys, sigma_max,
    v_maxx, v_maxy, v_back, sigma_back) rescaled alike.  guard_verdict(f32 = true) wants the largest total variance within
    2^15 = 32768: make_case's sigma_max reaches 2 scales and sigma_back 3.8 scales, so a scale above 86 (47 with the
    per-walker Gaussian background) leaves the float32 ranges -- the cells that came out at level 0 (some of every model,
    whichever N drew a large scale).  At 31.6 the largest variance is (3.8^2 + 0.6^2) 1000 = 1.5e4.
Every cell of the two tests must be inside the domain AND be given the fast formulations by the guard
(fast_level(f32) == 1); tests/test_f32_emul_cpu.py asserts both for every cell, nothing is skipped."""
import numpy as np

import variant_helper as vh
from oracle import lnprob_numpy as oracle

CENTRE = vh.CENTRE
CHUNK_LEN = vh.CHUNK_LEN                  # 96

# Star counts and the tail branches they take (csrc/mcd_math.h: chunk_const_f32, chunk_mixture_f32), chunk_len 96:
#   1, 2, 3  singles only                       4   one 4-tree                   7   one 4-tree + 3 singles
#   8        two 4-trees                        15  three 4-trees + 3 singles    16  one 16-tree (CONST, fixed centre)
#   23       16 + 4 + 3                         33  2 x 16 + 1                   4099  43 chunks, the last of 67 = 4 x 16 + 3
F32_STARS = (1, 2, 3, 4, 7, 8, 15, 16, 23, 33, 4099)
F32_WALKERS = (1, 65, 257)                # idle lanes, a ragged second tile, the grid above 256 walkers
CPU_WALKERS = 65                          # the host-build test: sample_rows(65)
PRECISIONS = ("f32acc64", "f32")
BIN_OFFSETS = (0, 5, 705, 4099)           # the binned cells: bins of 5, 700 and 3394 stars in one launch
BIN_WALKERS = 65                          # ... each with rows b * 65 .. b * 65 + 64 of the table
N_ROWS = max(F32_WALKERS)

# Stated tolerances of the float32 modes inside the domain (csrc/mcd_guard.h, above kF32KappaV), on the scale
# max(|lnL|, N, 32): (free centre, accumulator in float64) -> bound
TOLERANCE = {(False, True): 1e-6, (False, False): 2e-5, (True, True): 2e-5, (True, False): 1e-4}


def stars(free):
    """A free centre with one star cannot be inside the domain: the star is the catalogue's centroid, its separation 0."""
    return tuple(n for n in F32_STARS if not (free and n == 1))


def tolerance(free, precision):
    return TOLERANCE[(bool(free), precision == "f32acc64")]


def f32_case(model, free, n):
    """variant_helper.make_case(model, free, n) moved into the float32 accuracy domain; the walker table has N_ROWS rows."""
    case = vh.make_case(model, free, n)
    rng = np.random.default_rng(7000000 + 100000 * model + 50000 * int(free) + n)
    prof = model in vh.PROFILE_MODELS
    bg = vh.BG_OF[model]
    cat = dict(case["cat"])
    p = case["params"][:N_ROWS].copy()
    # velocity scale 10^0.5 .. 10^1.5 instead of make_case's 10^0.5 .. 10^2, every velocity rescaled alike (RANGES above)
    sv = 10.0 ** rng.uniform(0.5, 1.5)
    f = sv / case["scale"]
    cat["v"] = cat["v"] * f
    vel = [0, 1] + ([3, 4] if prof else [2, 3])
    if bg == vh.BG_GAUSS:
        vel += [p.shape[1] - 3, p.shape[1] - 2]                          # v_back, sigma_back
    p[:, vel] *= f
    cat["verr"] = sv * rng.uniform(0.3, 0.6, n)
    if prof:
        p[:, 2] = rng.uniform(30.0, 100.0, N_ROWS)                       # a [arcsec]
        p[:, 5] = rng.uniform(30.0, 100.0, N_ROWS)                       # r_peak
    if free:
        sep = np.abs(rng.normal(0.0, 0.5, n)) + 0.1                      # degrees
        th = rng.uniform(-np.pi, np.pi, n)
        cat["ra"] = CENTRE[0] + sep * np.cos(th) / np.cos(np.radians(CENTRE[1]))
        cat["dec"] = CENTRE[1] + sep * np.sin(th)
        ix = 3 if prof else 2
        p[:, ix:ix + 2] *= 0.03
    if bg in (vh.BG_FIXED, vh.BG_FIXED_DENSITY):
        cat["lnlike_bg"] = oracle.gaussian_background(cat["v"], cat["verr"], 0.1 * sv, 3 * sv)
    case.update(cat=cat, params=np.ascontiguousarray(p), scale=sv)
    return case


def binned_params(case):
    """(3, BIN_WALKERS, K): a walker table of its own for each bin of BIN_OFFSETS."""
    return np.ascontiguousarray(np.stack([case["params"][b * BIN_WALKERS:(b + 1) * BIN_WALKERS]
                                          for b in range(len(BIN_OFFSETS) - 1)]))


def drop_last_star(case):
    """The same case without its last star (N - 1 stars): what a kernel that loses the tail star would evaluate."""
    out = dict(case)
    out["cat"] = {k: v[:-1] for k, v in case["cat"].items()}
    out["n"] = case["n"] - 1
    return out


def scaled_err(got, want, n):
    """|got - want| / max(|want|, N, 32): the scale of the stated tolerances (a single float32 term has an absolute floor of
    a few 1e-6, csrc/mcd_guard.h)."""
    got, want = np.asarray(got, dtype=vh.L), np.asarray(want, dtype=vh.L)
    return (np.abs(got - want) / np.maximum(np.abs(want), vh.L(max(n, 32)))).astype(np.float64)


class Oracle(object):
    """numpy.longdouble values of the rows of one case, computed once per row and shared by the tests of a module."""

    def __init__(self, case):
        self.case, self.exact = case, {}

    def rows(self, rows):
        c = self.case
        for r in rows:
            if r not in self.exact:
                self.exact[r] = vh.exact(c["model"], c["cat"], c["params"][r], c["centre"])
        return np.array([self.exact[r] for r in rows], dtype=vh.L)


_CASES = {}


def cached_case(model, free, n):
    """(case, its Oracle), built once per process."""
    key = (model, bool(free), n)
    if key not in _CASES:
        case = f32_case(model, free, n)
        _CASES[key] = (case, Oracle(case))
    return _CASES[key]

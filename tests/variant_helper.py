"""Test helper: inputs, oracles and launch control for the kernel-variant matrix (tests/test_variant_inputs_cpu.py,
tests/test_gpu_variant_matrix.py, tests/test_gpu_reduce_shapes.py).  Test infrastructure only.

The main kernel (csrc/mcd_kernels.hip: loglike_kernel) is one template with many instantiations: model x centre x kernel
family (plain / general fast / narrow-range) x record prefetch x 4-, 8-, 16-wave workgroups x the bounded BGFIXED loop.
This module builds catalogues and walker tables INSIDE the narrow-range domain of every model, so that each family can be
demanded by option and the tests can assert which one ran, and evaluates the reference's formulas (oracle/lnprob_numpy.py)
in float64 and in numpy.longdouble."""
import numpy as np

from oracle import lnprob_numpy as oracle

CENTRE = (56.345, -26.675)
L = np.longdouble
HAVE_LONGDOUBLE = np.finfo(L).eps < 1e-18

PROFILE_MODELS = (3, 4, 5, 6)
BG_NONE, BG_FIXED, BG_GAUSS, BG_FIXED_DENSITY = 0, 1, 2, 3
BG_OF = {0: BG_NONE, 1: BG_FIXED, 2: BG_GAUSS, 3: BG_NONE, 4: BG_GAUSS, 5: BG_FIXED_DENSITY, 6: BG_FIXED}
MIXTURE_MODELS = (1, 2, 4, 5, 6)

# The matrix (issue: every variant, at the walker and star counts where kernels go wrong)
WALKERS = (1, 64, 65, 256, 257, 520)      # idle lanes, 1 / 2 / 4 / 5 / 9 walker tiles, the XCD-grouped grid above 256
STARS = (1, 7, 33, 4099, 20011)           # fewer stars than one 8 / 16-star iteration, ragged tails, many chunks
PLANT_STARS = (4099, 20011)               # four planted exceptions stay far below N / 8 only there
FAMILIES = ("plain", "general", "narrow")
FAST_PATH = {"plain": 0, "general": 2, "narrow": 1}     # option "fast_path" (include/mcd.h)
LEVEL = {"plain": 0, "general": 1, "narrow": 2}         # what mcd_last_fast_level reports
CHUNK_LEN = 96                            # multi-round plans of catalogues this small: the minimum nominal length

# Which (model, free centre) has a narrow-range variant, written out from mcd_guard.h: level_verdict and
# mcd_kernels.hip: launch_precision -- MODEL_CONST has none; MODEL_PROFILE only with a fixed centre (ProfileNarrowAcc
# needs r_max_fixed); the BG_GAUSS and BG_FIXED_DENSITY models and MODEL_BGFIXED for either centre; MODEL_PROFILE_BGFIXED
# is never given level 2 by the guard.
HAS_NARROW = {(0, False): False, (0, True): False, (1, False): True, (1, True): True, (2, False): True, (2, True): True,
              (3, False): True, (3, True): False, (4, False): True, (4, True): True, (5, False): True, (5, True): True,
              (6, False): False, (6, True): False}
# The bounded loop (mcd_guard.h: bounded_rescale; launch_one: kCanBound) exists for MODEL_BGFIXED with a fixed centre only,
# in the prefetching kernels.  For the catalogues of make_case (pmember <= 0.98, |v - v_los| < 13 velocity scales,
# sigma >= scale / 2) its two products stay within 2^+-1000 for 32 factors: R = 32 for every N and W of the matrix.
BOUNDED_R = {(1, False): 32}


def families(model, free):
    return FAMILIES if HAS_NARROW[(model, free)] else FAMILIES[:2]


def n_wtiles(w):
    return (w + 63) // 64


def sample_rows(w):
    """At least six walker rows where there are six, row 0 and row W - 1 among them."""
    return sorted({min(max(i, 0), w - 1) for i in (0, 1, 2, w // 2, w - 2, w - 1)})


# ---- work decomposition the options of force() select (mcd_chunks.h, mcd_api_catalog.hip: build_workset) -----------------
def balanced_chunks(n, w, m):
    """Chunks of the one-round plan with m workgroups per CU, 0 where the catalogue is too small for it (fewer than 16
    stars per chunk).  Only the walker-tile counts whose workgroups can combine (1, 2, 4) are of interest here."""
    t = n_wtiles(w)
    if t not in (1, 2, 4):
        return 0
    g = 256 * m * (4 // t)
    return g if n // g // 8 * 8 >= 16 else 0


def combine_cells(n, w):
    """Workgroup sizes beyond 4 waves that option "balance" 2 / 4 with "combine" 8 / 16 can give this (N, W)."""
    return tuple(waves for waves, m in ((8, 2), (16, 4)) if balanced_chunks(n, w, m))


def expected_waves(model, family, waves):
    """launch_one has no 16-wave case for the per-walker Gaussian background models (more than 128 VGPRs): the library
    runs them as 8-wave workgroups on the same plan.  The plain kernels never combine."""
    if family == "plain" or waves == 4:
        return 4
    return 8 if waves == 16 and BG_OF[model] == BG_GAUSS else waves


def expected_launch(model, family, n, w, waves):
    """(chunks, workgroups) of the main-kernel launch."""
    t = n_wtiles(w)
    if waves == 4:
        chunks = -(-n // CHUNK_LEN)
    else:
        chunks = balanced_chunks(n, w, 2 if waves == 8 else 4)
        assert chunks, "cell outside combine_cells()"
    ran = expected_waves(model, family, waves)
    if ran > 4:
        return chunks, -(-chunks * t // ran)
    return chunks, (-(-chunks * t // 4) if t <= 4 else -(-chunks // 8) * 8 * -(-t // 4))


# ---- inputs ---------------------------------------------------------------------------------------------------------
def plant_positions(n):
    """Star 0, star N - 1, the last star of an interior chunk of the multi-round plan and the first star of the next."""
    c = (n // CHUNK_LEN) // 2
    return [0, CHUNK_LEN * (c + 1) - 1, CHUNK_LEN * (c + 1), n - 1]


def make_case(model, free, n, plant=False, seed=None):
    """Catalogue columns, a (520, K) walker table in the C-ABI column order and the centre (None: free), inside the
    narrow-range domain of `model`.  After _realistic_case of tests/test_gpu_kernels.py, with
      * pmember within [0.02, 0.98], density and f_back within [0.05, 0.95], a and r_peak within [3, 100] arcsec;
      * errors of 0.1 .. 0.6 and dispersions of 0.5 .. 2 velocity scales, walkers within ~1 scale of the truth and the two
        gross outliers at 3x (not 20x): |v - v_los|^2 <= 2e6 min(verr^2) holds with room (the narrow-range condition of
        the profile models, whose dispersion decays to 0) and BGFIXED stays inside the bounded loop's domain;
      * stars at least 0.01 deg from the fixed centre and free centres within +-0.005 deg of it: theta = arctan2(dy, dx)
        is ill-conditioned next to the centre in the reference's own formula (one ulp of sin / cos moves it by 1e-16 / r).
    plant: four certain members (exceptions of the narrow-range variants, mcd_guard.h: narrow_exception) at
    plant_positions(n) -- pmember = 1 for the pmember mixtures, density = 2^21 (membership prior 1 - 4e-7 f_back) for the
    density mixtures -- with velocities well inside the cluster's distribution."""
    rng = np.random.default_rng(100000 * model + 50000 * int(free) + n if seed is None else seed)
    sv = 10.0 ** rng.uniform(0.5, 2.0)
    sep = np.maximum(np.abs(rng.normal(0, 2.0 / 60.0, n)), 0.01)
    th = rng.uniform(-np.pi, np.pi, n)
    cat = {"ra": CENTRE[0] + sep * np.cos(th) / np.cos(np.radians(CENTRE[1])), "dec": CENTRE[1] + sep * np.sin(th),
           "v": rng.normal(0, sv, n), "verr": sv * rng.uniform(0.1, 0.6, n)}
    cat["v"][: min(2, n)] *= 3.0
    density = rng.uniform(0.05, 0.95, n)
    pmember = np.clip(rng.random(n) * 1.1 - 0.05, 0.02, 0.98)
    w = max(WALKERS)
    cols = [rng.normal(0, 0.3 * sv, w), sv * 10.0 ** rng.uniform(-0.3, 0.3, w)]
    if model in PROFILE_MODELS:
        cols.append(10.0 ** rng.uniform(np.log10(3.0), 2.0, w))                   # a [arcsec]
    cols += [rng.normal(0, 0.3 * sv, w), rng.normal(0, 0.3 * sv, w)]
    if model in PROFILE_MODELS:
        cols.append(10.0 ** rng.uniform(np.log10(3.0), 2.0, w))                   # r_peak
    if free:
        cols += [CENTRE[0] + rng.uniform(-0.005, 0.005, w), CENTRE[1] + rng.uniform(-0.005, 0.005, w)]
    bg = BG_OF[model]
    if bg == BG_GAUSS:
        cols += [rng.normal(0, 0.3 * sv, w), 3 * sv * 10.0 ** rng.uniform(-0.1, 0.1, w), rng.uniform(0.05, 0.95, w)]
    if bg == BG_FIXED_DENSITY:
        cols.append(rng.uniform(0.05, 0.95, w))
    planted = plant_positions(n) if plant else []
    if plant:
        assert model in MIXTURE_MODELS and 8 * len(planted) * 4 <= n
        cat["v"][planted] = 0.2 * sv * np.array([1.0, -1.0, 0.5, -0.5])
        pmember[planted] = 1.0
        density[planted] = 2.0 ** 21
    if bg in (BG_FIXED, BG_FIXED_DENSITY):
        cat["lnlike_bg"] = oracle.gaussian_background(cat["v"], cat["verr"], 0.1 * sv, 3 * sv)
    if bg == BG_FIXED:
        cat["pmember"] = pmember
    if bg in (BG_GAUSS, BG_FIXED_DENSITY):
        cat["density"] = density
    return {"model": model, "free": free, "n": n, "cat": cat, "params": np.ascontiguousarray(np.stack(cols, axis=1)),
            "centre": None if free else CENTRE, "planted": planted, "scale": sv}


def catalog(native, ctx, case, sl=slice(None), **more):
    c = case["cat"]
    kw = {k: c[k][sl] for k in ("lnlike_bg", "pmember", "density") if k in c}
    kw.update(more)
    return native.Catalog(ctx, c["ra"][sl], c["dec"][sl], c["v"][sl], c["verr"][sl], model=case["model"],
                          centre=case["centre"], **kw)


# ---- oracles ------------------------------------------------------------------------------------------------------------
def _split(model, row, centre, dtype):
    row = np.asarray(row).astype(dtype)
    head = 6 if model in PROFILE_MODELS else 4
    if centre is None:
        return row[:head], row[head], row[head + 1], row[head + 2:]
    return row[:head], dtype(centre[0]), dtype(centre[1]), row[head:]


def value(model, cat, row, centre, dtype=np.float64):
    """The reference's log-likelihood of one walker row (oracle.faithful_*) with every input cast to `dtype`."""
    c = {k: np.asarray(v).astype(dtype) for k, v in cat.items()}
    head, rc, dc, tail = _split(model, row, centre, dtype)
    if model == 0:
        return oracle.faithful_constant_lnlike(c, *head, rc, dc)
    if model == 1:
        return oracle.faithful_constant_lnlike(c, *head, rc, dc, c["lnlike_bg"], c["pmember"])
    if model == 2:
        return oracle.faithful_constant_gb_lnlike(c, *head, rc, dc, *tail)
    if model == 3:
        return oracle.faithful_model_lnlike(c, *head, rc, dc)
    if model == 4:
        return oracle.faithful_model_gb_lnlike(c, *head, rc, dc, *tail)
    if model == 5:
        return oracle.faithful_model_cb_lnlike(c, *head, rc, dc, tail[0], c["lnlike_bg"])
    return oracle.faithful_model_lnlike(c, *head, rc, dc, c["lnlike_bg"], c["pmember"])


def exact(model, cat, row, centre):
    """value() in numpy.longdouble (80-bit on x86: 11 more bits than the kernels and the float64 oracle)."""
    return value(model, cat, row, centre, L)


def per_star(model, cat, row, centre, dtype=L):
    """(per-star log-likelihood, membership probability or None without a background) of one row, in `dtype`: the
    log-sum-exp of runner.py:280-284 and the posterior weight of the cluster component (constant.py:366-374,
    model.py:505-510)."""
    c = {k: np.asarray(v).astype(dtype) for k, v in cat.items()}
    head, rc, dc, tail = _split(model, row, centre, dtype)
    if model in PROFILE_MODELS:
        v_los = oracle.model_rotation(c["ra"], c["dec"], head[0], head[3], head[4], head[5], rc, dc)
        sig = oracle.model_dispersion(c["ra"], c["dec"], head[1], head[2], rc, dc)
    else:
        v_los = oracle.rotation_model(c["ra"], c["dec"], head[0], head[2], head[3], rc, dc)
        sig = head[1]
    norm = c["verr"] * c["verr"] + sig * sig
    lc = -0.5 * np.log(2. * np.pi * norm) - 0.5 * np.power(c["v"] - v_los, 2) / norm
    bg = BG_OF[model]
    if bg == BG_NONE:
        return lc, None                                    # no mixture: the Gaussian term itself (runner.py:269-271)
    lb = oracle.gaussian_background(c["v"], c["verr"], tail[0], tail[1]) if bg == BG_GAUSS else c["lnlike_bg"]
    m = c["pmember"] if bg == BG_FIXED else c["density"] / (c["density"] + tail[-1])
    mx = np.maximum(lc, lb)
    ec, eb = m * np.exp(lc - mx), (1. - m) * np.exp(lb - mx)
    assert lc.dtype == dtype and ec.dtype == dtype
    return mx + np.log(ec + eb), ec / (ec + eb)


def scaled_err(got, want, n):
    """|got - want| on the scale max(|want|, N): every term is O(1 .. 10), a total that cancels below N is judged on N."""
    got, want = np.asarray(got, dtype=L), np.asarray(want, dtype=L)
    return (np.abs(got - want) / np.maximum(np.abs(want), L(n))).astype(np.float64)


# ---- launch control -----------------------------------------------------------------------------------------------------
def force(cat, family, prefetch, waves, bounded=1):
    """Demand one instantiation: kernel family, record prefetch, workgroup size (4: the multi-round plan; 8 / 16: the
    one-round plan with 2 / 4 workgroups per CU, combined), the bounded BGFIXED loop on or off."""
    cat.set_option("fast_path", FAST_PATH[family])
    cat.set_option("prefetch", int(prefetch))
    cat.set_option("narrow_bounded", int(bounded))
    cat.set_option("balance", {4: 0, 8: 2, 16: 4}[waves])
    cat.set_option("combine", {4: 0, 8: 8, 16: 16}[waves])


def assert_ran(cat, model, free, family, prefetch, waves, n, w, bounded=1, planted=False):
    """What the last launch actually was.  A cell that was not admitted as requested fails."""
    cell = (model, free, family, prefetch, waves, n, w, bounded, planted)
    assert cat.fast_level == LEVEL[family], ("kernel family", cat.fast_level, cell)
    assert cat.rerun_count == 0, ("re-run with the plain kernels", cell)
    assert cat.last_prefetch == int(bool(prefetch) and family != "plain"), ("prefetch", cat.last_prefetch, cell)
    r = BOUNDED_R.get((model, free), 0) if family == "narrow" and prefetch and bounded and not planted else 0
    assert cat.last_narrow_bounded == r, ("bounded loop", cat.last_narrow_bounded, cell)
    info = cat.launch_info()
    chunks, groups = expected_launch(model, family, n, w, waves)
    assert (info["chunks"], info["workgroups"]) == (chunks, groups), ("launch shape", info, cell)
    if expected_waves(model, family, waves) > 4:
        assert 4 * info["workgroups"] < info["chunks"] * n_wtiles(w), ("workgroups did not combine", info, cell)

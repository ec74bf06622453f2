"""GPU: mcd_replicate_check (csrc/mcd_replicate.hip, csrc/mcd_api_replicate.hip) against the exact side of
tests/replicate_helper.py under the accuracy rule stated there (the device tolerance of DESIGN 3.12 is the same rule; its
rtol of 1e-10 applies to spreads, of which there are none here; counts are exact), the invariances of a replicate, the pass
path, determinism, the refusals, and Runner.replicate_check for every model class."""
import ctypes

import numpy as np
import pytest

import emul_helper as eh
import posterior_helper as ph
import predictive_helper as pr
import replicate_helper as rh
from test_replicate_cpu import CAL_SEEDS, _recombine

pytestmark = pytest.mark.gpu
MODELS = [0, 1, 2, 3, 4, 5, 6]
_I64P = ctypes.POINTER(ctypes.c_int64)
_F64P = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def ctx():
    from mcmc_dynamics_amd import _native
    return _native.default_context()


def run(gpu, model, table, offs, order, seed=rh.SEED, row0=0, bg=None):
    bg = rh.background_of(model) if bg is None else bg
    return gpu.replicate_check(table, seed, offs, order, bg[0], bg[1], row0=row0)


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("free", [False, True])
def test_device_follows_the_rule(ctx, model, free):
    """7 models x {fixed, free} x N in {1, 65, 4099} x S in {1, 65, 257} x the three range layouts."""
    gpus = {}

    def on_device(cat, table, centre, offs, order):
        n = len(cat["v"])
        if n not in gpus:
            gpus[n] = pr.device_catalog(ctx, cat, model, centre)
        got = run(gpus[n], model, table, offs, order)
        assert got.shape == (table.shape[0], len(offs) - 1, 8, 2)
        return got
    rh.check_matrix_cell(model, free, on_device)
    for g in gpus.values():
        g.close()


@pytest.mark.parametrize("model,free", [(0, False), (2, True), (6, False)])
def test_a_replicate_does_not_depend_on_ranges_or_chunks(ctx, model, free):
    """N = 4099, S = 257: one range against sixteen recombined, two forced chunk lengths, a range on its own."""
    cat, table, centre = rh.matrix_case(model, free)
    ref = rh.matrix_reference(model, free)
    n = len(cat["v"])
    gpu = pr.device_catalog(ctx, cat, model, centre)
    one, sixteen = rh.layout("one", n), rh.layout("sixteen", n)
    exact, np64, scale = ref.at(*one)
    base = run(gpu, model, table, *one)
    split = run(gpu, model, table, *sixteen)
    combined = _recombine(split)
    rh.check_rule(combined, exact, np64, scale, cell="16 ranges recombined")
    assert np.array_equal(combined[:, :, 6:], base[:, :, 6:])                  # max and count: exactly
    for forced in (64, 1024):
        gpu.set_option("chunk_len", forced)
        got = run(gpu, model, table, *one)
        rh.check_rule(got, exact, np64, scale, cell="chunk length {0}".format(forced))
        assert np.array_equal(got[:, :, 6:], base[:, :, 6:])
    gpu.set_option("chunk_len", 0)
    assert np.array_equal(run(gpu, model, table, *one), base)                  # ... and back: the same bits as before
    offs, order = sixteen
    lone = run(gpu, model, table, [0, offs[6] - offs[5]], order[offs[5]:offs[6]])
    assert np.array_equal(lone[:, 0], split[:, 5])
    three = rh.layout("three", n)
    got = run(gpu, model, table, *three)
    assert np.all(got[:, 0] == 0.0) and not np.signbit(got[:, 0]).any()        # the empty range: +0.0 everywhere
    gpu.close()


def test_membership_one_zero_and_repeated_rows(ctx):
    cat = pr.clear_of_centres(ph.model_catalog(4099, 0, seed=7), *ph.CENTRE)
    n = len(cat["v"])
    offs, order = rh.layout("sixteen", n)
    # m = 1: the model without a background, bit for bit
    for bg_model, plain in ((1, 0), (4, 3)):
        t_plain = ph.samples(cat, plain, False, 257)
        t_bg = ph.samples(cat, bg_model, False, 257)
        t_bg[:, :t_plain.shape[1]] = t_plain
        c = {k: (x.copy() if isinstance(x, np.ndarray) else x) for k, x in cat.items()}
        if eh.BG_OF[bg_model] == 1:
            c["pmember"] = np.ones(n)
        else:
            t_bg[:, -1] = 0.0
        a, b = pr.device_catalog(ctx, c, plain, ph.CENTRE), pr.device_catalog(ctx, c, bg_model, ph.CENTRE)
        assert np.array_equal(run(b, bg_model, t_bg, offs, order, seed=99), run(a, plain, t_plain, offs, order, seed=99))
        a.close()
        b.close()
    # m = 0: pure background, against the restatement
    c = {k: (x.copy() if isinstance(x, np.ndarray) else x) for k, x in cat.items()}
    c["pmember"] = np.zeros(n)
    table = ph.samples(cat, 1, False, 257)
    gpu = pr.device_catalog(ctx, c, 1, ph.CENTRE)
    ref = rh.Reference(c, table[:9], 1, ph.CENTRE, seed=99)
    assert np.all(ref.exact["m"] == 0)
    got = run(gpu, 1, table, offs, order, seed=99)
    rh.check_rule(got[:9], *ref.at(offs, order), cell="m = 0")
    # one repeated row: equal observed fields in every row, other replicates
    rows = np.repeat(table[3:4], 257, axis=0)
    got = run(gpu, 1, rows, offs, order)
    assert np.all(got[..., 0] == got[:1, ..., 0]) and not np.array_equal(got[1, ..., 1], got[0, ..., 1])
    gpu.close()


def test_passes_over_the_rows_concatenate(ctx):
    """65 537 rows on 65 stars: one full pass and a pass of one row; equal to two calls over the split rows, bit for bit."""
    cat, table, centre = rh.matrix_case(5, True)
    gpu = pr.device_catalog(ctx, pr.head(cat, 65), 5, centre)
    rows = np.ascontiguousarray(np.tile(table, (256, 1))[:65537])
    rows[65536] = table[100]
    offs, order = rh.layout("three", 65)
    full = run(gpu, 5, rows, offs, order)
    assert np.array_equal(full[:65536], run(gpu, 5, rows[:65536], offs, order))
    assert np.array_equal(full[65536:], run(gpu, 5, rows[65536:], offs, order, row0=65536))
    # the generator follows the row index, not the row: equal rows 257 apart have equal observed fields only
    assert np.array_equal(full[0, ..., 0], full[257, ..., 0]) and not np.array_equal(full[0, ..., 1], full[257, ..., 1])
    # ... and the rows of the second pass obey the rule like any other
    ref = rh.Reference(pr.head(cat, 65), rows[65536:], 5, centre, row0=65536)
    rh.check_rule(full[65536:], *ref.at(offs, order), cell="second pass")
    gpu.close()


def test_bits_repeat_across_an_interleaved_call(ctx):
    cat, table, centre = rh.matrix_case(4, False)
    gpu = pr.device_catalog(ctx, cat, 4, centre)
    sixteen, three = rh.layout("sixteen", 4099), rh.layout("three", 4099)
    first = run(gpu, 4, table, *sixteen)
    run(gpu, 4, table[:65], *three, seed=7)
    gpu.loglike(table[:64])
    assert np.array_equal(run(gpu, 4, table, *sixteen), first)
    assert not np.array_equal(run(gpu, 4, table, *sixteen, seed=rh.SEED + 1)[..., 1], first[..., 1])
    gpu.set_option("timing", 1)
    run(gpu, 4, table, *sixteen)
    assert gpu.last_kernel_ms > 0.0
    gpu.close()


def test_refusals_leave_the_output_untouched(ctx):
    from mcmc_dynamics_amd import _native
    small = pr.head(ph.model_catalog(200, 0), 200)
    row = np.ascontiguousarray(ph.samples(small, 0, False, 3))
    const = pr.device_catalog(ctx, small, 0, ph.CENTRE)
    fixed = pr.device_catalog(ctx, small, 1, ph.CENTRE)
    lib = const.lib
    out = np.full((3, 2, 8, 2), 7.0)
    nan = float("nan")

    def call(cat, offs, order, k=4, S=3, bg=(nan, nan), params=row, dst=out):
        offs, order = np.asarray(offs, np.int64), np.asarray(order, np.int64)
        return lib.mcd_replicate_check(cat.handle if cat is not None else None, S, k,
                                       params.ctypes.data_as(_F64P) if params is not None else None, 5, offs.size - 1,
                                       offs.ctypes.data_as(_I64P), order.ctypes.data_as(_I64P), bg[0], bg[1],
                                       dst.ctypes.data_as(_F64P) if dst is not None else None)
    good = ([0, 2, 5], [9, 3, 199, 0, 7])
    assert call(const, [0, 3, 2], [1, 2, 3]) == -1 and b"non-decreasing" in lib.mcd_last_error()
    assert call(const, [1, 2, 3], [1, 2, 3]) == -1 and b"must be 0" in lib.mcd_last_error()
    assert call(const, [0, 2, 5], [9, 3, 200, 0, 7]) == -1 and b"outside" in lib.mcd_last_error()
    assert call(const, [0, 2, 5], [9, 3, -1, 0, 7]) == -1 and b"outside" in lib.mcd_last_error()
    assert call(const, [0, 2, 5], [9, 3, 7, 0, 7]) == -1 and b"twice" in lib.mcd_last_error()
    assert call(const, *good, k=5) == -1 and b"columns" in lib.mcd_last_error()
    assert call(const, *good, S=0) == -1 and b"sample row" in lib.mcd_last_error()
    assert call(const, *good, params=None) == -1 and call(const, *good, dst=None) == -1 and call(None, *good) == -1
    for bad in ((nan, nan), (20.0, nan), (20.0, -1.0), (np.inf, 40.0)):
        assert call(fixed, *good, bg=bad) == -1 and b"fixed-background" in lib.mcd_last_error()
    binned = _native.Catalog(ctx, small["ra"], small["dec"], small["v"], small["verr"], centre=ph.CENTRE,
                             bin_offsets=[0, 80, 200])
    assert call(binned, *good) == -1 and b"un-binned" in lib.mcd_last_error()
    f32 = pr.device_catalog(ctx, small, 0, ph.CENTRE, precision="f32")
    assert call(f32, *good) == -1 and b"MCD_F64" in lib.mcd_last_error()
    assert np.all(out == 7.0)                                                  # every refusal left the output untouched
    assert call(const, *good) == 0 and call(fixed, *good, bg=(20.0, 0.0)) == 0
    assert np.isfinite(out).all() and np.all(out[:, :, 7] >= 0)
    assert np.array_equal(out, fixed.replicate_check(row, 5, *good, 20.0, 0.0))
    with pytest.raises(ValueError, match="order must hold"):
        const.replicate_check(row, 5, [0, 2, 5], [1, 2, 3])
    for c in (const, fixed, binned, f32):
        c.close()


def _classes():
    from mcmc_dynamics_amd.analysis import ConstantFit, ConstantFitGB, ModelFit, ModelFitConstantBackground, ModelFitGB
    from mcmc_dynamics_amd.background import Gaussian
    bg = Gaussian(rh.BG_MEAN, rh.BG_SIGMA)
    base, dens = ("ra", "dec", "v", "verr"), ("ra", "dec", "v", "verr", "density")
    return {0: (ConstantFit, base, {}), 1: (ConstantFit, base + ("pmember",), {"background": bg}), 2: (ConstantFitGB, dens, {}),
            3: (ModelFit, base, {}), 4: (ModelFitGB, dens, {}), 5: (ModelFitConstantBackground, dens, {"background": bg}),
            6: (ModelFit, base + ("pmember",), {"background": bg})}


@pytest.mark.parametrize("model", MODELS)
def test_runner_replicate_check_of_every_model_class(model):
    """2 000 stars, 6 x 8 samples after burn-in, 5 annuli: shapes, finiteness, and the emulation's summary."""
    from mcmc_dynamics_amd import DataReader
    from mcmc_dynamics_amd.analysis.runner import REPLICATE_NAMES, replicate_summary
    cls, columns, kw = _classes()[model]
    cat = ph.model_catalog(2000, 0)
    fit = cls(DataReader({k: cat[k] for k in columns}), **kw)
    fit.parameters["ra_center"].set(value=ph.CENTRE[0], fixed=True)
    fit.parameters["dec_center"].set(value=ph.CENTRE[1], fixed=True)
    table = ph.samples(cat, model, False, 6 * 10)
    names = ph.abi_names(model, False)
    # (a class may fit parameters its kernel does not read: they keep their default value)
    chain = np.stack([table[:, names.index(n)] if n in names else np.full(60, float(fit.parameters[n].value))
                      for n in fit.fitted_parameters], axis=1).reshape(6, 10, -1)
    out = fit.replicate_check(chain, n_burn=2, annuli=5, seed=1234)
    assert out["names"] == REPLICATE_NAMES and out["seed"] == 1234 and out["n_samples"] == 48
    assert out["n_stars"].tolist() == [2000, 400, 400, 400, 400, 400] and out["edges"].shape == (6,)
    assert out["obs"].shape == out["rep"].shape == (48, 6, 7) and out["p_value"].shape == out["extreme"].shape == (6, 7)
    assert out["bands"].shape == (6, 7, 2, 3)
    assert all(np.isfinite(out[k]).all() for k in ("obs", "rep", "p_value", "extreme", "bands"))
    assert np.all((out["p_value"] >= 0) & (out["p_value"] <= 1)) and np.all(out["extreme"] <= 0.5)
    # the same call on the emulation, with the rows the Runner hands the kernel
    kernel_rows, _ = fit._posterior_table(chain, 2, 1)
    offs, order, _ = fit._replicate_groups(5, None)
    assert np.array_equal(offs, rh.annuli_of(cat, ph.CENTRE, 5)[0])
    want = replicate_summary(rh.replicate(cat, kernel_rows, model, ph.CENTRE, 1234, offs, order), np.diff(offs))
    for k in ("obs", "rep", "bands"):
        assert np.allclose(out[k], want[k], rtol=1e-9, atol=1e-9), k
    assert np.max(np.abs(out["p_value"] - want["p_value"])) <= 1.0 / 48 + 1e-15
    # groups instead of annuli; a second call with the same seed repeats the bits
    labels = np.full(2000, -1)
    labels[::3], labels[1::3] = 1, 0
    by_group = fit.replicate_check(chain, n_burn=2, groups=labels, seed=1234)
    assert by_group["groups"].tolist() == [0, 1] and by_group["n_stars"].tolist() == [1334, 667, 667]
    again = fit.replicate_check(chain, n_burn=2, groups=labels, seed=1234)
    assert all(np.array_equal(by_group[k], again[k]) for k in ("obs", "rep", "p_value"))
    fit.close()


def test_calibration_on_the_device(ctx):
    """Data drawn from the model itself at N = 4000, S = 256, 4 annuli: the verdicts of the host test."""
    from mcmc_dynamics_amd.analysis.runner import replicate_summary
    cat, table, offs, order = rh.calibration_case("model", CAL_SEEDS["model"])
    gpu = pr.device_catalog(ctx, cat, 0, ph.CENTRE)
    got = replicate_summary(gpu.replicate_check(table, 31, offs, order), np.diff(offs))
    want = replicate_summary(rh.replicate(cat, table, 0, ph.CENTRE, 31, offs, order), np.diff(offs))
    print(got["p_value"][0])
    assert np.all(got["p_value"][0] >= 0.01) and np.all(got["p_value"][0] <= 0.99)
    assert np.max(np.abs(got["p_value"] - want["p_value"])) <= 1.0 / 256 + 1e-15
    gpu.close()

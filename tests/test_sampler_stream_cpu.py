"""The random stream of the stretch samplers (mcmc_dynamics_amd/sampler.py: EnsembleSampler, analysis/binned.py:
BinnedSampler) as a user drives them: ``reset()`` between a burn-in and a production run, seeds of any size, and the
float32 bookkeeping of the Runner around them.  No GPU: a NumPy Gaussian log-probability, the device generator's numbers from
the library's host code (``_native.chain_numbers``) or from the host build of tests/emul."""
import ctypes
import warnings

import numpy as np
import pytest

import emul_helper as em
from mcmc_dynamics_amd.analysis.binned import BinnedSampler
from mcmc_dynamics_amd.sampler import EnsembleSampler

W, P, B = 8, 2, 3
EVAL = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_int64, ctypes.POINTER(ctypes.c_double))
MASK64 = 0xFFFFFFFFFFFFFFFF


def _lnprob(values):
    """A Gaussian with unequal widths, centred off the origin: (..., P) -> (...)."""
    v = np.asarray(values, dtype=np.float64)
    return -0.5 * ((v[..., 0] - 0.5) ** 2 / 0.7 + (v[..., 1] + 0.25) ** 2 / 1.9)


def _seeded_block_fn(n_bins, calls):
    """The library's host block loop (csrc/mcd_stretch.h, CPU build of tests/emul) fed with the host build's numbers of
    csrc/mcd_rng.h: what ``mcd_stretch_move_seeded`` does when it runs host-driven.  ``calls`` collects (seed, step0, n)."""
    lib = em.lib()
    src, const, fac = np.arange(P, dtype=np.int32), np.zeros(P), np.ones(P)
    lo, hi = np.full(P, -np.inf), np.full(P, np.inf)

    @EVAL
    def cb(tab, n, out):
        table = np.ctypeslib.as_array(tab, shape=(n_bins * n, P))
        np.ctypeslib.as_array(out, shape=(n_bins * n,))[:] = _lnprob(table)
        return 0

    def run(pos, lnp, seed, step0, n, chain, lnprob_chain, accepted):
        calls.append((int(seed), int(step0), int(n)))
        order, zz, thr, pick = em.chain_numbers(seed, step0, n, n_bins, W, P)       # (n, B, W) / (n, 2, B, W/2): B = 1 is flat
        p = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t)) if a is not None else None
        rc = lib.emul_stretch_block(ctypes.c_int64(n_bins), ctypes.c_int64(W), P, P, p(src, ctypes.c_int32),
                                    p(const, ctypes.c_double), p(fac, ctypes.c_double), p(lo, ctypes.c_double),
                                    p(hi, ctypes.c_double), 1, ctypes.c_int64(n), p(pos, ctypes.c_double),
                                    p(lnp, ctypes.c_double), p(order, ctypes.c_int32), p(zz, ctypes.c_double),
                                    p(thr, ctypes.c_double), p(pick, ctypes.c_int32), p(chain, ctypes.c_double),
                                    p(lnprob_chain, ctypes.c_double), p(accepted, ctypes.c_int64), cb)
        assert rc == 0, rc
    run.keep = cb
    return run


def _make(kind, way="numpy", seed=123, rng="device", block=None, calls=None):
    """A sampler of ``kind`` ("ensemble" / "binned") driven the ``way`` asked for: the NumPy loop, or library blocks."""
    calls = [] if calls is None else calls
    if kind == "ensemble":
        s = EnsembleSampler(W, P, _lnprob, vectorize=True, seed=seed, rng=rng,
                            seeded_block_fn=_seeded_block_fn(1, calls) if way == "library" else None)
        if block is not None:
            s.block_steps = block
    else:
        s = BinnedSampler(B, W, P, _lnprob, seed=seed, rng=rng,
                          seeded_block_fn=_seeded_block_fn(B, calls) if way == "library" else None)
        if block is not None:
            s.device_block_steps = s.block_steps = block
    s.calls = calls
    return s


def _start(kind):
    start = np.random.default_rng(7).normal(size=(B, W, P))
    return start[0] if kind == "ensemble" else start


def _rows(s):
    """(positions, log-probabilities) of the steps a sampler holds, steps first."""
    return s._chain[:s.iteration].copy(), s._lnprob[:s.iteration].copy()


_FULL = {}


def _uninterrupted(kind):
    """12 steps of a fresh sampler in one call (the NumPy loop), computed once: chain, log-probabilities, and the accepted
    counts after 5 and after 12 steps."""
    if kind not in _FULL:
        s = _make(kind)
        s.run_mcmc(_start(kind), 12)
        five = _make(kind)
        five.run_mcmc(_start(kind), 5)
        chain, lnp = _rows(s)
        for a in (chain, lnp):
            a.setflags(write=False)
        _FULL[kind] = (chain, lnp, five._accepted.copy(), s._accepted.copy())
        assert np.array_equal(_rows(five)[0], chain[:5])
        assert 0.1 < s.acceptance_fraction.mean() < 0.95 and np.unique(chain.reshape(12, -1), axis=0).shape[0] == 12
    return _FULL[kind]


@pytest.mark.parametrize("way", ["numpy", "library"])
@pytest.mark.parametrize("kind", ["ensemble", "binned"])
def test_reset_continues_the_device_stream(kind, way, built_library):
    """Burn-in, ``reset()``, production: the production run takes the generator's steps 5 .. 11, the rows an uninterrupted
    12-step run stores there -- not steps 0 .. 6 again, the numbers that produced its own start."""
    chain12, lnp12, acc5, acc12 = _uninterrupted(kind)
    s = _make(kind, way)
    pos, _, _ = s.run_mcmc(_start(kind), 5)
    assert np.array_equal(_rows(s)[0], chain12[:5]) and np.array_equal(s._accepted, acc5)
    s.reset()
    assert s.iteration == 0 and s.get_chain().shape[0] == 0 and not s._accepted.any()
    s.run_mcmc(pos, 7)
    assert np.array_equal(s.get_chain(), chain12[5:12])                # (a rewound generator gives rows 0 .. 6 again)
    assert s.iteration == 7 and s.rng_step == 12
    assert np.array_equal(_rows(s)[1], lnp12[5:12])
    assert np.array_equal(s._accepted, acc12 - acc5)
    assert not np.array_equal(s.get_chain()[:5], chain12[:5])
    if way == "library":
        assert s.calls == [(123, 0, 5), (123, 5, 7)]
    if kind == "binned":
        s.close()


def test_reset_asks_the_library_for_the_next_steps(monkeypatch, built_library):
    """What the NumPy loop asks ``_native.chain_numbers`` for: (seed, 0, 5), then -- after ``reset()`` -- (seed, 5, 5)."""
    from mcmc_dynamics_amd import _native
    asked, real = [], _native.chain_numbers

    def recording(seed, step0, n, *rest, **kw):
        asked.append((seed, step0, n))
        return real(seed, step0, n, *rest, **kw)
    monkeypatch.setattr(_native, "chain_numbers", recording)
    for kind in ("ensemble", "binned"):
        del asked[:]
        s = _make(kind, seed=9)
        pos, _, _ = s.run_mcmc(_start(kind), 5)
        s.reset()
        s.run_mcmc(pos, 5)
        assert asked == [(9, 0, 5), (9, 5, 5)], (kind, asked)


CUTS = [((12,), 256, False), ((5, 7), 256, True), ((5, 7), 3, False), ((1, 4, 7), 1, True), ((3, 3, 3, 3), 2, True),
        ((7, 5), 4, True), ((11, 1), 5, False)]


@pytest.mark.parametrize("way", ["numpy", "library"])
@pytest.mark.parametrize("kind", ["ensemble", "binned"])
def test_any_cut_of_the_run_gives_the_same_positions(kind, way, built_library):
    """``rng="device"``: the 12 positions do not depend on how the steps are cut into ``run_mcmc`` calls and blocks, nor on a
    ``reset()`` between two calls."""
    chain12, lnp12, _, acc12 = _uninterrupted(kind)
    for cuts, block, with_reset in CUTS:
        s = _make(kind, way, block=block)
        pos, lnp, got, got_lnp, accepted = _start(kind), None, [], [], 0
        for n in cuts:
            pos, lnp, _ = s.run_mcmc(pos, n, log_prob0=lnp)
            if with_reset:
                rows = _rows(s)
                got.append(rows[0])
                got_lnp.append(rows[1])
                accepted = accepted + s._accepted
                s.reset()
        if not with_reset:
            got, got_lnp, accepted = [_rows(s)[0]], [_rows(s)[1]], s._accepted
        assert np.array_equal(np.concatenate(got), chain12), (cuts, block, with_reset)
        assert np.array_equal(np.concatenate(got_lnp), lnp12) and np.array_equal(accepted, acc12)
        assert s.rng_step == 12 and s.iteration == (0 if with_reset else 12)
        if way == "library":
            assert [c[1] for c in s.calls] == list(np.cumsum([0] + [c[2] for c in s.calls])[:-1])      # consecutive steps
            assert max(c[2] for c in s.calls) <= block and sum(c[2] for c in s.calls) == 12
        if kind == "binned":
            s.close()


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and tuple(a[2:]) == tuple(b[2:])


@pytest.mark.parametrize("kind", ["ensemble", "binned"])
def test_reset_leaves_the_host_generators_alone(kind):
    """``rng="host"``: the NumPy generators carry on across ``reset()``, so the next block's draws are not the first's."""
    s = _make(kind, seed=5, rng="host")
    s.run_mcmc(_start(kind), 5)
    first = _rows(s)[0]
    before = [s._random.get_state()] + [g.get_state() for g in getattr(s, "_streams", ())]
    s.reset()
    after = [s._random.get_state()] + [g.get_state() for g in getattr(s, "_streams", ())]
    assert all(_same_state(a, b) for a, b in zip(before, after)) and s.iteration == 0 and s.rng_step == 5
    s.run_mcmc(_start(kind), 5)                                         # the same start: only the numbers differ
    assert not np.array_equal(_rows(s)[0], first)
    again = _make(kind, seed=5, rng="host")
    again.run_mcmc(_start(kind), 5)
    assert np.array_equal(_rows(again)[0], first)                       # (what a replayed stream would have given)
    for x in (s, again):
        if kind == "binned":
            x.close()


@pytest.mark.parametrize("kind", ["ensemble", "binned"])
def test_any_integer_seeds_the_device_generator(kind, built_library):
    """``rng="device"``: a seed wraps to 64 bits as ``stretch_move_seeded`` takes it (-1 is 2^64 - 1); nothing narrower."""
    chains = {}
    for seed in (0, 2 ** 32, 2 ** 40, 2 ** 64 - 1, -1, 2 ** 64 + 3, 3):
        s = _make(kind, seed=seed)
        assert s.seed64 == seed & MASK64
        s.run_mcmc(_start(kind), 4)
        chains[seed] = _rows(s)[0]
        assert np.all(np.isfinite(chains[seed])) and s.rng_step == 4
        if kind == "binned":
            s.close()
    assert np.array_equal(chains[-1], chains[2 ** 64 - 1])
    assert np.array_equal(chains[2 ** 64 + 3], chains[3])
    assert not np.array_equal(chains[2 ** 32], chains[0])              # (a seed cut to 32 bits would make these equal)
    assert not np.array_equal(chains[2 ** 40], chains[0]) and not np.array_equal(chains[2 ** 40], chains[2 ** 32])
    # library blocks get the same 64-bit name
    lib = _make(kind, "library", seed=-1)
    lib.run_mcmc(_start(kind), 4)
    assert lib.calls == [(2 ** 64 - 1, 0, 4)] and np.array_equal(_rows(lib)[0], chains[-1])
    if kind == "binned":
        lib.close()


@pytest.mark.parametrize("kind", ["ensemble", "binned"])
def test_host_mode_keeps_numpys_seed_range(kind):
    with pytest.raises(ValueError):
        _make(kind, seed=2 ** 40, rng="host")
    with pytest.raises(ValueError):
        _make(kind, seed=-1, rng="host")
    s = _make(kind, seed=2 ** 32 - 1, rng="host")
    s.run_mcmc(_start(kind), 2)
    if kind == "binned":
        s.close()


# ---------------------------------------------------------------------------------------------------------------------
# Runner-level float32 bookkeeping, no device: a stub catalogue (as tests/hostgroup_worker.py) that counts what it is asked.

class _StubCatalog(object):
    """Stands in for a float32 ``_native.Catalog``: the oracle's likelihood, a block that leaves the ensemble where it is,
    and ``f32_outside`` counters that count the direct evaluations and / or the blocks' evaluations as outside the domain."""

    def __init__(self, cols, centre, outside_direct=False, outside_block=False):
        self.cols, self.centre = cols, centre
        self.outside_direct, self.outside_block = outside_direct, outside_block
        self.n_outside, self.evaluations, self.blocks, self.options = 0, 0, 0, {}

    def set_option(self, key, value):
        self.options[key] = int(value)

    def loglike(self, table):
        from oracle import lnprob_numpy as oracle
        self.evaluations += 1
        self.n_outside += int(self.outside_direct)
        return oracle.batched_constant_lnlike(self.cols, np.asarray(table), *self.centre)

    def stretch_move_seeded(self, plan, pos, lnp, seed, step0, n_steps, chain=None, lnprob_chain=None, accepted=None):
        self.blocks += 1
        self.n_outside += 2 * n_steps * int(self.outside_block)
        if chain is not None:
            chain[:], lnprob_chain[:] = pos, lnp

    def f32_outside(self):
        hit = self.n_outside > 0
        return {"calls": self.n_outside, "worst_kappa_v": 120.5 if hit else 31.0, "worst_kappa_theta": 0.0,
                "reason": "kappa_v exceeds 96 (stub)" if hit else ""}

    def close(self):
        pass


def _stub_fit(**stub):
    from mcmc_dynamics_amd import DataReader, synthetic
    from mcmc_dynamics_amd.analysis import ConstantFit
    centre = (synthetic.CENTER_RA_DEG, synthetic.CENTER_DEC_DEG)
    cols = synthetic.make_catalog(64, config=2)
    fit = ConstantFit(DataReader({k: cols[k] for k in ("ra", "dec", "v", "verr")}), precision="f32")
    fit.SAMPLER = "builtin"
    fit.parameters["ra_center"].set(value=centre[0], fixed=True)
    fit.parameters["dec_center"].set(value=centre[1], fixed=True)
    fit._catalog = _StubCatalog(cols, centre, **stub)
    fit._catalog_key = fit._plan().catalog_key
    fit._ensure_catalog = lambda: fit._catalog
    names = ["v_sys", "sigma_max", "v_maxx", "v_maxy"]
    pos = synthetic.make_walkers(8, names, cols["truth"], config=2)
    return fit, pos


def _domain_warnings(caught):
    return [w for w in caught if issubclass(w.category, UserWarning) and "float32 accuracy domain" in str(w.message)]


def test_runner_warns_once_when_a_direct_evaluation_leaves_the_float32_domain():
    fit, pos = _stub_fit(outside_direct=True)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        first = fit.lnprob_batch(pos)
        fit.lnprob_batch(pos)
        fit.lnlike_batch(pos)
        assert np.all(np.isfinite(first))
    found = _domain_warnings(caught)
    assert len(found) == 1 and fit._catalog.evaluations == 3
    text = str(found[0].message)
    assert "kappa_v exceeds 96 (stub)" in text and "120.5" in text and "f32" in text
    assert fit.f32_outside()["calls"] == 3 and fit.f32_outside()["worst_kappa_v"] == 120.5


def test_runner_warns_once_when_a_block_leaves_the_float32_domain():
    """Only the blocks see a table outside: the evaluation of the start does not warn, the first block does, no later one."""
    fit, pos = _stub_fit(outside_block=True)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        fit.lnprob_batch(pos)
        assert not _domain_warnings(caught)
        sampler = fit(n_walkers=8, n_steps=6, n_out=2, pos=pos, prefix=None)         # three run_mcmc calls: three blocks
    assert sampler.seeded_block_fn is not None and fit._catalog.blocks == 3 and sampler.iteration == 6
    assert len(_domain_warnings(caught)) == 1 and fit.f32_outside()["calls"] == 12


def test_runner_does_not_warn_inside_the_float32_domain():
    fit, pos = _stub_fit()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        fit.lnprob_batch(pos)
        fit(n_walkers=8, n_steps=4, n_out=2, pos=pos, prefix=None)
    assert not _domain_warnings(caught) and fit._catalog.blocks == 2
    assert fit.f32_outside() == {"calls": 0, "worst_kappa_v": 31.0, "worst_kappa_theta": 0.0, "reason": ""}
    # a float64 fit has nothing to count and asks its catalogue nothing
    fit._precision = "f64"
    assert fit.f32_outside() == {"calls": 0, "worst_kappa_v": 0.0, "worst_kappa_theta": 0.0, "reason": ""}


def test_runner_creates_float32_catalogues_that_evaluate_regardless(monkeypatch):
    """Catalogues a Runner creates for 'f32' / 'f32acc64' get option ``f32_domain`` = 0; a float64 one is left alone."""
    from mcmc_dynamics_amd import _native
    made = []

    class Recording(_StubCatalog):
        def __init__(self, ctx, ra, dec, v, verr, precision="f64", **kwargs):
            _StubCatalog.__init__(self, None, None)
            self.precision = precision
            made.append(self)
    monkeypatch.setattr(_native, "Catalog", Recording)
    for precision, want in (("f32", {"f32_domain": 0}), ("f32acc64", {"f32_domain": 0}), ("f64", {})):
        fit, _ = _stub_fit()
        del fit._ensure_catalog                                # the class's own method again
        fit._catalog, fit._catalog_key, fit._context, fit._precision = None, None, object(), precision
        cat = fit._ensure_catalog()
        assert cat is made[-1] and cat.precision == precision and cat.options == want
        assert fit._ensure_catalog() is cat and len(made) == 1 + ("f32", "f32acc64", "f64").index(precision)


# ---------------------------------------------------------------------------------------------------------------------
# Where the catalogue of tests/test_gpu_sampler_stream.py sits with respect to the float32 accuracy domain (host build of
# csrc/mcd_guard.h: f32_domain): what its "inside" and "outside" runs rely on.

@pytest.mark.parametrize("background", [False, True])
def test_the_gpu_tests_configurations_sit_where_they_should(background):
    import itertools
    import stream_helper as sh
    model = 1 if background else 0
    cols = sh.domain_columns("inside", background)
    assert len(cols["v"]) == 257 and np.max(np.abs(cols["v"])) <= 40.0 and 1.0 <= cols["verr"].min() and cols["verr"].max() <= 3.0
    start = sh.walkers("inside")
    assert start.shape == (16, 4) and 5.0 <= start[:, 1].min() and start[:, 1].max() <= 15.0
    lo, hi = np.array([b for b in sh.box("inside").values()]).T
    corners = np.array(list(itertools.product(*zip(lo, hi))))               # the 16 corners of the prior box, sigma = 0 included
    for table in (start, start[:8], corners, np.vstack([start, corners])):
        inside, kv, kt, _, why = em.f32_domain(cols, table, model, sh.centre())
        assert inside and kv <= 85.0 + 1e-9 and kt == 0.0, (kv, why)
    # outside: the same stars + 300 km/s; kappa_v crosses 96 as sigma moves between 15 and 5
    far = sh.domain_columns("outside", background)
    assert np.array_equal(far["v"], cols["v"] + 300.0)
    pos = sh.walkers("outside")
    kappa = {}
    for sigma in (5.0, 6.0, 7.5, 15.0):
        table = pos.copy()
        table[:, 1] = sigma
        inside, kappa[sigma], _, _, why = em.f32_domain(far, table, model, sh.centre())
        assert inside == (sigma > 7.0) and (inside or "exceeds 96" in why), (sigma, kappa[sigma], why)
    assert 35.0 < kappa[15.0] < 50.0 and 110.0 < kappa[5.0] < 140.0
    assert not em.f32_domain(far, pos, model, sh.centre())[0]              # the start itself: its lowest sigma is below 6.6

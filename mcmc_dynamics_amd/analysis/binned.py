"""Radial-binned dispersion / rotation profile: B independent ``ConstantFit`` posteriors evaluated in ONE
kernel launch per proposal batch.

The reference has no multi-bin class: its "profile" is a Python loop that builds one ``ConstantFit`` per
radial bin and runs B separate MCMCs one after the other (bin/run_tests.py:75-124, bin/run.py:146-259;
bins from ``DataReader.make_radial_bins``, utils/files/data_reader.py:71-140).  Here the stars are sorted
by bin once, the catalogue carries ``bin_offsets``, every bin owns its own walker ensemble, and the B
ensembles advance in lockstep: a stretch-move half-step proposes ``(B, W/2)`` positions and one segmented
launch returns the ``(B, W/2)`` log-likelihoods.
"""
import logging
from collections import OrderedDict

import numpy as np

from ..sampler import _clear, _host_seed, _reserve, _run_blocks, _setup, default_gamma0
from .constant import ConstantFit

logger = logging.getLogger(__name__)


class BinnedSampler(object):
    """B lock-stepped affine-invariant ensembles (same move as ``sampler.EnsembleSampler``, same driver: ``sampler._run_blocks``),
    one per radial bin: the reference runs one MCMC per bin (bin/run_tests.py:75-124); here the bins share every evaluation.

    ``block_fn`` (what ``BinnedConstantFit`` passes for box priors): a callable that advances all ensembles by a whole block
    of steps from the random numbers drawn here -- ``mcd_stretch_move`` with ``n_bins = B`` runs the same half-step loop in
    C++ (csrc/mcd_stretch.h), bit-identical to the NumPy loop.  The NumPy loop costs ~7 ms per step at 55 bins x 512
    walkers against 0.17 ms of device time per step; the library's loop ~0.2 ms."""

    N_STREAMS = 8          # part of the definition of the random stream (2: 334, 4: 313, 8: 297 us per step at 55 x 512)

    def __init__(self, n_bins, nwalkers, ndim, log_prob_fn, a=2.0, seed=None, block_fn=None, rng="host", seeded_block_fn=None,
                 move="stretch", gamma0=None, sigma=1e-5):
        """``rng``: where the move's random numbers come from.

        ``"host"``: NumPy's Mersenne twister on the host, as emcee draws (B x W numbers per step cross PCIe: the draws, not
        the device, bound the rate -- 3400 steps/s at 55 bins x 512 walkers against 6000 of device time).

        ``"device"``: the counter-based generator of csrc/mcd_rng.h: every number is a function of (seed, step, half step,
        bin, walker) alone (``sampler._setup``).  ``seeded_block_fn`` (``Runner._stretch_block_seeded``) runs whole blocks
        with the numbers generated on the device; without it (expression priors) the NumPy loop takes the SAME numbers
        from ``_native.chain_numbers`` -- one chain whichever way it is run, and however it is cut into blocks.

        ``move``: ``"stretch"`` or ``"de"``, the differential-evolution move (``sampler._setup``; ``gamma0``, ``sigma``); it
        needs ``rng="device"``, and ``seeded_block_fn`` is then the DE block (``Runner._de_block_seeded``)."""
        self.n_bins = int(n_bins)
        _setup(self, (self.n_bins,), nwalkers, ndim, a, rng, seed, block_fn, seeded_block_fn, move, gamma0, sigma)
        self.log_prob_fn = log_prob_fn
        self.block_steps = 64                     # steps whose random numbers are drawn together (defines the stream)
        self.device_block_steps = 256             # rng="device": steps per library call (NOT part of the stream's definition)
        self._random = np.random.RandomState(_host_seed(self, seed))
        # the steps of a block are drawn by N_STREAMS generators seeded from the master (see _draw)
        self._streams = [np.random.RandomState(int(s)) for s in self._random.randint(0, 2 ** 31 - 1, size=self.N_STREAMS)]
        self._pool = None

    def close(self):
        """Release the drawing threads (also done when the sampler is garbage-collected; the next run starts them again)."""
        pool, self._pool = getattr(self, "_pool", None), None
        if pool is not None:
            pool.shutdown(wait=False)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        """Drop the chain, the log-probabilities, the acceptance counts and ``n_calls``, as ``sampler.EnsembleSampler.reset``:
        the random stream carries on where it stands (``rng_step`` and the NumPy generators are left alone)."""
        _clear(self)

    @property
    def chain(self):
        """(B, W, steps, P): per bin the (W, steps, P) layout of the reference's pickles."""
        return np.transpose(self._chain[:self.iteration], (1, 2, 0, 3))

    @property
    def lnprobability(self):
        return np.transpose(self._lnprob[:self.iteration], (1, 2, 0))

    @property
    def acceptance_fraction(self):
        return self._accepted / max(1, self.iteration)

    def get_chain(self, discard=0):
        """(steps, B, W, P): the steps-first layout of ``sampler.EnsembleSampler.get_chain`` with the bin axis after it."""
        return self._chain[discard:self.iteration]

    def get_autocorr_time(self, discard=0, thin=1, **kwargs):
        """(B, P): the integrated autocorrelation time per bin and parameter in steps (``diagnostics.integrated_time``)."""
        from ..diagnostics import sampler_autocorr_time
        return sampler_autocorr_time(self, discard=discard, thin=thin, **kwargs)

    def reserve(self, total_steps):
        """Chain storage for ``total_steps`` steps in all (a run continued by further ``run_mcmc`` calls otherwise grows its
        storage geometrically and copies the rows it holds: 1.1 MB per step at 55 bins x 512 walkers)."""
        _reserve(self, total_steps)

    def _draw(self, n):
        # B x W numbers per step make the draws the bottleneck (1.3 ms per step at 55 x 512 on one core, against 0.2 ms of
        # device time): the block is cut into len(streams) slices of steps, every slice drawn from its own generator on its
        # own thread (NumPy releases the interpreter lock).  Which numbers a step gets depends only on (seed, block_steps,
        # the step's place in the block), never on thread timing.
        B, W, half = self.n_bins, self.nwalkers, self.nwalkers // 2
        am1, inv_a, dm1 = self.a - 1.0, 1.0 / self.a, self.ndim - 1.0
        order, zz, thr, pick = out = (np.empty((n, B, W), dtype=np.int32), np.empty((n, 2, B, half)),
                                      np.empty((n, 2, B, half)), np.empty((n, 2, B, half), dtype=np.int32))

        def draw_slice(rnd, lo, hi):
            # steps lo..hi in a handful of vectorised draws (as sampler.EnsembleSampler draws): split of every ensemble =
            # argsort of uniform keys, stretch factors z ~ g(z), log acceptance thresholds (accept iff thr < new_lnp -
            # old_lnp), partner indices; written straight into the block's arrays
            order[lo:hi] = np.argsort(rnd.rand(hi - lo, B, W), axis=2)
            u = rnd.rand(hi - lo, 4, B, half)
            z = zz[lo:hi]
            np.multiply(u[:, :2], am1, out=z)
            z += 1.0
            z *= z
            z *= inv_a
            np.subtract(np.log(u[:, 2:]), dm1 * np.log(z), out=thr[lo:hi])
            pick[lo:hi] = rnd.randint(half, size=(hi - lo, 2, B, half))

        k = len(self._streams)
        cuts = [n * i // k for i in range(k + 1)]
        jobs = [(self._streams[i], cuts[i], cuts[i + 1]) for i in range(k) if cuts[i + 1] > cuts[i]]
        if len(jobs) > 1:
            list(self._pool.map(lambda job: draw_slice(*job), jobs))
        else:
            draw_slice(*jobs[0])
        return out

    def _log_prob(self, values):
        lnp = np.asarray(self.log_prob_fn(values), dtype=np.float64)
        self.n_calls += 1
        if np.any(np.isnan(lnp)):
            raise ValueError("Probability function returned NaN")
        return lnp

    def run_mcmc(self, pos, nsteps, log_prob0=None):
        pos = np.ascontiguousarray(pos, dtype=np.float64).copy()
        B, W, P = self.n_bins, self.nwalkers, self.ndim
        if pos.shape != (B, W, P):
            raise ValueError("incompatible input dimensions {0}".format(pos.shape))
        # (C order: the NumPy loop updates pos and lnp through flat views of them)
        lnp = np.array(self._log_prob(pos) if log_prob0 is None else log_prob0, dtype=np.float64, order="C")
        if np.any(np.isnan(lnp)):
            raise ValueError("Probability function returned NaN")
        if self._pool is None:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(max_workers=self.N_STREAMS)
        # (blocks of very many ensembles are kept below ~8 M walker-steps: 200 MB of numbers in, 340 MB of rows out)
        steps = self.device_block_steps if self.rng == "device" else self.block_steps
        chunk = max(1, min(int(steps), (1 << 23) // (B * W)))
        _run_blocks(self, pos, lnp, nsteps, chunk, chunk, self._draw, self._log_prob)
        return pos, lnp, self._random.get_state()


class BinnedConstantFit(ConstantFit):
    """``ConstantFit`` in every radial bin of ``data`` (column ``bin``) simultaneously.

    ``lnprob_batch`` maps ``(B, W, P)`` positions to ``(B, W)`` log-posteriors; ``lnlike_total`` sums the
    bins for one shared parameter set (== the un-binned ``ConstantFit`` value)."""

    def __init__(self, data, parameters=None, **kwargs):
        if "bin" not in data.data.columns:
            raise IOError("BinnedConstantFit needs a 'bin' column: call DataReader.make_radial_bins() first.")
        data_sorted, self.bin_offsets = data.sorted_by_bin()
        self.n_bins = len(self.bin_offsets) - 1
        super(BinnedConstantFit, self).__init__(data=data_sorted, parameters=parameters, **kwargs)
        if self.background is not None:
            raise IOError("BinnedConstantFit does not take a background population.")

    def _catalog_kwargs(self):
        return {"bin_offsets": self.bin_offsets}

    def _resolve(self, values):
        values = np.asarray(values, dtype=np.float64)
        if values.ndim == 2:                       # one parameter set shared by all bins
            values = np.broadcast_to(values, (self.n_bins,) + values.shape)
        if values.ndim != 3 or values.shape[0] != self.n_bins:
            raise ValueError("expected positions of shape (n_bins, W, P)")
        flat = self.parameters.resolve_batch(values.reshape(-1, values.shape[2]))
        return values.shape[1], flat

    def _launch(self, w, flat):
        cat = self._ensure_catalog()
        table = self._kernel_table(flat)
        ll = cat.loglike(table.reshape(self.n_bins, w, -1)) if self.n_bins > 1 else \
            cat.loglike(table.reshape(w, -1))[None, :]
        if self._precision != "f64":
            self._note_f32(cat)
        return ll

    def lnlike_batch(self, values):
        w, flat = self._resolve(values)
        return self._launch(w, flat)

    def lnprob_batch(self, values):
        plan = self._plan()
        values = np.asarray(values, dtype=np.float64)
        if plan.simple and values.ndim == 3 and values.shape[0] == self.n_bins and values.shape[2] == plan.free_idx.size:
            # flat bounds, no expression priors / constraints: the vectorised plan of Runner.lnprob_batch over all bins
            w = values.shape[1]
            free = values.reshape(-1, values.shape[2])
            full = plan.full(free)
            lp, ok = plan.prior_free(free, plan.prior_ok(full))          # (structured priors: shared by the bins)
            out = np.full(self.n_bins * w, -np.inf)
            if ok.any():
                if not ok.all():
                    full[~ok] = full[int(np.flatnonzero(ok)[0])]
                cat = self._ensure_catalog()
                table = plan.table(full)
                ll = (cat.loglike(table.reshape(self.n_bins, w, -1)) if self.n_bins > 1 else
                      cat.loglike(table.reshape(w, -1))[None, :]).reshape(-1)
                if self._precision != "f64":
                    self._note_f32(cat)
                out[ok] = ll[ok] if lp is None else ll[ok] + lp[ok]
            return out.reshape(self.n_bins, w)
        w, flat = self._resolve(values)
        lp = self.parameters.lnprior_batch(flat)
        ok = np.isfinite(lp)
        out = np.full(self.n_bins * w, -np.inf)
        if ok.any():
            if not ok.all():
                donor = int(np.flatnonzero(ok)[0])
                flat = OrderedDict((k, np.where(ok, col, col[donor])) for k, col in flat.items())
            ll = self._launch(w, flat).reshape(-1)
            out[ok] = ll[ok] + lp[ok]
        return out.reshape(self.n_bins, w)

    def lnlike_total(self, values):
        """(W, P) -> (W,): sum over bins with one shared parameter set."""
        return self.lnlike_batch(np.atleast_2d(values)).sum(axis=0)

    def lnlike(self, values):
        return float(self.lnlike_total(np.asarray(values, dtype=np.float64).reshape(1, -1))[0])

    RNG = "device"                 # where BinnedSampler's random numbers come from ("host": NumPy's generator, as emcee)
    MOVE = "stretch"               # the move when ``__call__`` is not told one: "stretch" or "de" (sampler._setup)

    def __call__(self, n_walkers=100, n_steps=100, pos=None, seed=None, rng=None, move=None, gamma0=None, sigma=1e-5, **kwargs):
        """Run the B ensembles in lockstep; returns a ``BinnedSampler`` (``.chain``: (B, W, steps, P)).  ``rng``: see
        ``BinnedSampler`` (default: the class attribute ``RNG``).  ``move``: ``"stretch"`` or ``"de"`` (default: the class
        attribute ``MOVE``), with ``gamma0`` and ``sigma`` as ``BinnedSampler`` takes them."""
        if kwargs.get("n_threads", 1) != 1:
            raise ValueError("n_threads > 1 is not supported by the GPU backend.")
        move = move or self.MOVE
        if move == "de" and self._rank_group() is not None:
            raise NotImplementedError("move='de' on a multi-rank context: the collective resident DE block is not built")
        if pos is None:
            pos = np.stack([self.get_initials(n_walkers) for _ in range(self.n_bins)])
        pos = np.asarray(pos, dtype=np.float64)
        # several ranks (stars sharded): rank 0's start positions and ONE seed go to every rank, as in Runner.__call__
        group = self._rank_group()
        if group is not None:
            pos = group.bcast_array(pos, src=0)
            # (a seed the sampler takes in the mode it runs in: 64 bits for the device generator, 32 for NumPy's)
            bits = 64 if (rng or self.RNG) == "device" else 32
            seed = int(group.bcast_json(int(seed) if seed is not None else int(np.random.SeedSequence().entropy % (2 ** bits)), src=0))
        lp = self.parameters.lnprior_batch(self.parameters.resolve_batch(pos.reshape(-1, pos.shape[-1])))
        if not np.all(np.isfinite(lp)):
            raise ValueError("Invalid initial guesses for {0} walker(s).".format(int(np.sum(~np.isfinite(lp)))))
        # box priors: whole blocks of steps inside the library (mcd_stretch_move with n_bins = B, Runner._stretch_block)
        # (library blocks only for the package's own posterior and box priors: a subclass that overrides a posterior method
        # outside the package is driven by the NumPy loop around ITS lnprob_batch -- Runner.resident_ok)
        native_ok = self.resident_ok()[0] and self.n_bins > 1
        if move == "de":
            g0 = default_gamma0(self.n_fitted_parameters) if gamma0 is None else float(gamma0)
            seeded = (lambda *block: self._de_block_seeded(g0, sigma, *block)) if native_ok else None
            sampler = BinnedSampler(self.n_bins, n_walkers, self.n_fitted_parameters, self.lnprob_batch, seed=seed,
                                    rng=rng or self.RNG, seeded_block_fn=seeded, move="de", gamma0=g0, sigma=sigma)
        else:
            sampler = BinnedSampler(self.n_bins, n_walkers, self.n_fitted_parameters, self.lnprob_batch, seed=seed,
                                    block_fn=self._stretch_block if native_ok else None, rng=rng or self.RNG,
                                    seeded_block_fn=self._stretch_block_seeded if native_ok else None, move=move)
        sampler.run_mcmc(pos, n_steps)
        return sampler

    def _pointwise_posterior(self, chain, n_burn, thin, membership):
        raise NotImplementedError("BinnedConstantFit: per-star posterior summaries (pointwise_posterior, waic) are defined "
                                  "for un-binned fits only; fit the bins' stars with ConstantFit to compare models")

    def posterior_predictive(self, chain, n_burn, thin=1):
        raise NotImplementedError("BinnedConstantFit: per-star posterior predictive checks (posterior_predictive, ppc) are "
                                  "defined for un-binned fits only; fit the bins' stars with ConstantFit to check the model")

    def ppc(self, chain, n_burn, thin=1, n_bins=20, outlier_p=None):
        return self.posterior_predictive(chain, n_burn, thin)

    def replicate_check(self, *args, **kwargs):
        raise NotImplementedError("BinnedConstantFit: replicated-data checks (replicate_check) are defined for un-binned fits "
                                  "only; fit the bins' stars with ConstantFit and pass the bins as groups")

    def loo(self, chain, n_burn, thin=1, r_eff=1.0):
        raise NotImplementedError("BinnedConstantFit: PSIS-LOO is defined for un-binned fits only; fit the bins' stars "
                                  "with ConstantFit to compare models")

    def loo_pit(self, chain, n_burn, thin=1, r_eff=1.0, n_bins=20):
        return self.loo(chain, n_burn, thin, r_eff)

    def loo_influence(self, chain, n_burn, thin=1, r_eff=1.0, functions=None):
        return self.loo(chain, n_burn, thin, r_eff)

    def holdout_fit(self, *args, **kwargs):
        raise NotImplementedError("BinnedConstantFit: hold-out refits (holdout_fit, reloo, kfold) are defined for un-binned "
                                  "fits only; fit the bins' stars with ConstantFit to cross-validate")

    def reloo(self, *args, **kwargs):
        return self.holdout_fit()

    def kfold(self, *args, **kwargs):
        return self.holdout_fit()

    def bootstrap(self, *args, **kwargs):
        raise NotImplementedError("BinnedConstantFit: the weighted-likelihood bootstrap (bootstrap, "
                                  "lnprob_weighted_grad_batch) is defined for un-binned fits only; fit the bins' stars "
                                  "with ConstantFit")

    def lnprob_weighted_grad_batch(self, *args, **kwargs):
        return self.bootstrap()

    def bagged(self, *args, **kwargs):
        raise NotImplementedError("BinnedConstantFit: the bagged posterior (bagged, lnprob_weighted_batch) is defined "
                                  "for un-binned fits only; fit the bins' stars with ConstantFit")

    def lnprob_weighted_batch(self, *args, **kwargs):
        return self.bagged()

    def simulated_fits(self, *args, **kwargs):
        raise NotImplementedError("BinnedConstantFit: fits of simulated catalogues (sample_prior, simulate, simulated_set, "
                                  "lnprob_simulated_batch, simulated_fits, sbc, recovery) are defined for un-binned fits "
                                  "only; fit the bins' stars with ConstantFit")

    def sample_prior(self, *args, **kwargs):
        return self.simulated_fits()

    def simulate(self, *args, **kwargs):
        return self.simulated_fits()

    def simulated_set(self, *args, **kwargs):
        return self.simulated_fits()

    def lnprob_simulated_batch(self, *args, **kwargs):
        return self.simulated_fits()

    def sbc(self, *args, **kwargs):
        return self.simulated_fits()

    def recovery(self, *args, **kwargs):
        return self.simulated_fits()

    def simulated_maximize(self, *args, **kwargs):
        raise NotImplementedError("BinnedConstantFit: MAP fits of simulated catalogues (lnprob_simulated_grad_batch, "
                                  "simulated_maximize, parametric_bootstrap, lrt) are defined for un-binned fits only; fit "
                                  "the bins' stars with ConstantFit")

    def lnprob_simulated_grad_batch(self, *args, **kwargs):
        return self.simulated_maximize()

    def simulated_sims(self, *args, **kwargs):
        return self.simulated_maximize()

    def parametric_bootstrap(self, *args, **kwargs):
        return self.simulated_maximize()

    def lrt(self, *args, **kwargs):
        return self.simulated_maximize()

    def hmc(self, *args, **kwargs):
        raise NotImplementedError("BinnedConstantFit: Hamiltonian Monte Carlo is defined for un-binned fits only (the "
                                  "lock-stepped ensembles of the bins have no HMC block)")

    def tempered(self, *args, **kwargs):
        raise NotImplementedError("BinnedConstantFit: parallel tempering is defined for un-binned fits only (its rungs "
                                  "take the place of the bins' lock-stepped ensembles)")

    def run_converged(self, *args, **kwargs):
        raise NotImplementedError("BinnedConstantFit: run_converged drives one un-binned ensemble; run the bins with "
                                  "__call__ and judge them with chain_diagnostics / sampler.get_autocorr_time()")

    def chain_diagnostics(self, chain, n_burn, c=5.0, tol=50.0):
        """``diagnostics.summary`` of a chain (B, W, steps, P) after ``n_burn`` steps: (B, P) arrays, plus ``names``."""
        from .. import diagnostics
        chain = np.asarray(chain, dtype=np.float64)
        if chain.ndim != 4:
            raise ValueError("chain must have shape (bins, walkers, steps, parameters)")
        out = diagnostics.summary(np.transpose(chain[:, :, n_burn:, :], (2, 0, 1, 3)), c=c, tol=tol,
                                  context=self._diagnostics_context())
        out["names"] = list(self.fitted_parameters)
        return out

    def compute_bestfit_values(self, chain, n_burn):
        """List of per-bin result tables (median / uperr / loerr), as the per-bin loop of
        bin/run_tests.py:105-113 collects them."""
        saved = {k: p.value for k, p in self.parameters.items()}
        out = [super(BinnedConstantFit, self).compute_bestfit_values(chain[b], n_burn) for b in range(self.n_bins)]
        for k, v in saved.items():
            if self.parameters[k].expr is None:
                self.parameters[k].value = v
        return out

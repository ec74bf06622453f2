"""Affine-invariant ensemble sampler (Goodman & Weare 2010 stretch move) with emcee's interface.

The reference hands ``Runner.lnprob`` to ``emcee.EnsembleSampler`` (analysis/runner.py:403) and lets
emcee drive the outer loop.  emcee is not installed in the target image, so ``Runner.__call__`` uses
the real emcee when it can be imported and this class otherwise.  It implements the part of emcee 3's
``EnsembleSampler`` that the reference touches -- ``run_mcmc``, ``chain``, ``lnprobability``,
``iteration``, ``acceptance_fraction`` -- with emcee's default move: the ensemble is split in two
random halves, each half is updated against the other (``z ~ g(z) \\propto 1/sqrt(z)`` on [1/a, a],
``a = 2``), so one step costs two batched posterior calls of W/2 proposals each.

``vectorize=True`` (the mode the GPU backend uses) passes a ``(n, ndim)`` array to ``log_prob_fn`` and
expects ``(n,)`` back; otherwise the function is mapped over the rows (optionally with ``pool.map``).

``block_fn`` (optional, what ``Runner`` passes for box priors): a callable that advances the ensemble by a whole block
of steps from the random numbers drawn here -- ``libmcd_hip.so``'s ``mcd_stretch_move`` runs the same half-step loop in
C++ (csrc/mcd_stretch.h), bit-identical to the Python loop below, with a few microseconds of host time between two
kernel launches instead of ~50.

The stretch-move driver itself -- argument checks, chain storage, the block loop with its three ways of running a block
and the NumPy half-step -- is written once below (``_setup`` / ``_reserve`` / ``_run_blocks``) for B lock-stepped
ensembles; ``EnsembleSampler`` runs one ensemble without an ensemble axis, ``analysis.binned.BinnedSampler`` B of them.
Each sampler keeps what defines its random stream: how a block's numbers are drawn and how a run is cut into blocks.
"""
import numpy as np


_DRAW_POOL = None


def _draw_pool():
    """A few helper threads shared by all samplers of the process for the row-wise part of the draws (see ``draw``)."""
    global _DRAW_POOL
    if _DRAW_POOL is None:
        try:
            from concurrent.futures import ThreadPoolExecutor
            _DRAW_POOL = ThreadPoolExecutor(max_workers=4, thread_name_prefix="mcd-draw")
        except Exception:                                    # pragma: no cover
            _DRAW_POOL = False
    return _DRAW_POOL or None


# ---------------------------------------------------------------------------------------------------------------------
# The driver shared by EnsembleSampler and analysis.binned.BinnedSampler.  It works on the sampler's attributes: ``lead``
# is the shape of the ensemble axis, () for one ensemble without one, (B,) for B ensembles; pos is lead + (W, P), lnp and
# the acceptance counts lead + (W,), a block's numbers (steps,) + lead + (W,) (order) and (steps, 2) + lead + (W/2,).

MOVES = ("stretch", "de")


def default_gamma0(ndim):
    """The differential-evolution scale ter Braak (2006) derives for a Gaussian target: 2.38 / sqrt(2 P)."""
    return 2.38 / np.sqrt(2.0 * int(ndim))


def _setup(s, lead, nwalkers, ndim, a, rng, seed, block_fn, seeded_block_fn, move="stretch", gamma0=None, sigma=1e-5):
    """Checks and state common to both samplers.  ``rng="device"``: the move's random numbers come from the counter-based
    generator of csrc/mcd_rng.h (Philox4x64-10) instead of NumPy's Mersenne twister -- a function of (seed, step, half
    step, ensemble, walker) alone, generated on the device (csrc/mcd_stretch.hip: chain_numbers_kernel) by
    ``seeded_block_fn`` (``Runner._stretch_block_seeded``), or taken from ``_native.chain_numbers`` by the NumPy loop when
    there is none: the same chain either way, and however it is cut into blocks.

    ``rng_step`` is that generator's step counter: it advances with ``iteration`` and ``reset()`` leaves it alone, so the
    steps after a ``reset()`` take the numbers that follow the ones already used (as ``HMCSampler`` and
    ``TemperedSampler``).  ``seed`` may be any Python integer there: it wraps to 64 bits (-1 is 2^64 - 1), as
    ``_native.Catalog.stretch_move_seeded`` takes it.

    ``move``: ``"stretch"`` (Goodman & Weare, emcee's default) or ``"de"``, the differential-evolution move of csrc/mcd_de.h:
    a walker of one half proposes ``s + g (x_a - x_b)`` from two distinct walkers of the other half, ``g = gamma0 (1 + sigma
    n)`` with a standard normal ``n`` (``gamma0`` None: ``default_gamma0(ndim)``), accepted with probability min(1, ratio of
    the posteriors).  Same half steps, same cost per step; on correlated posteriors it decorrelates in about a third of the
    steps.  It is defined on the counter-based stream (a key of its own: never the stretch move's numbers of the same
    seed), so it needs ``rng="device"``, and an ensemble of at least 4 walkers.  ``seeded_block_fn`` is then the DE block
    (``Runner._de_block_seeded``) and the NumPy loop takes its numbers from ``_native.de_numbers``."""
    if rng not in ("host", "device"):
        raise ValueError("rng must be 'host' or 'device'")
    if move not in MOVES:
        raise ValueError("move must be 'stretch' or 'de'")
    s.move, s.gamma0, s.sigma = move, None, float(sigma)
    if move == "de":
        if rng != "device":
            raise ValueError("move='de' is defined on the counter-based stream: it needs rng='device'")
        if nwalkers < 4:
            raise ValueError("move='de' needs at least 4 walkers: two distinct partners in each half of the ensemble")
        s.gamma0 = default_gamma0(ndim) if gamma0 is None else float(gamma0)
        if not (s.gamma0 > 0.0 and np.isfinite(s.gamma0)) or not (s.sigma >= 0.0 and np.isfinite(s.sigma)):
            raise ValueError("move='de' needs a finite gamma0 > 0 and a finite sigma >= 0")
    if rng == "device" and move == "stretch" and float(a) != 2.0:
        raise ValueError("rng='device' implements the stretch move with a = 2 (emcee's default)")
    # rng="device": the 64-bit name of the chain (no seed: from NumPy's global generator, which the reference seeds at
    # analysis/runner.py:59 -- `np.random.seed` before the run makes it reproducible, as with emcee).  Only then: drawing
    # a seed moves NumPy's global generator.
    s.seed64 = None
    if rng == "device":
        s.seed64 = int(seed) & 0xFFFFFFFFFFFFFFFF if seed is not None else \
            (int(np.random.randint(0, 2 ** 32)) << 32) | int(np.random.randint(0, 2 ** 32))
    if nwalkers < 2 * ndim:
        raise ValueError("The number of walkers must be at least twice the dimension.")   # as emcee
    if nwalkers % 2:
        raise ValueError("The number of walkers must be even.")
    s._lead, s.nwalkers, s.ndim, s.a = tuple(lead), int(nwalkers), int(ndim), float(a)
    s.rng, s.block_fn, s.seeded_block_fn = rng, block_fn, seeded_block_fn
    s.rng_step = 0                                           # the device generator's step counter: never rewound
    _clear(s)


def _host_seed(s, seed):
    """What seeds the sampler's NumPy generator.  ``rng="host"``: the caller's seed as it is (one NumPy refuses raises
    NumPy's ValueError, as with emcee).  ``rng="device"``: that generator draws nothing for the move; it gets the 64-bit
    seed folded to the 32 bits NumPy takes (a seed below 2^32 is its own fold)."""
    if seed is None or s.rng != "device":
        return seed
    return (s.seed64 ^ (s.seed64 >> 32)) & 0xFFFFFFFF


def _clear(s):
    """No steps, no storage, no accepted moves, no posterior calls.  The random stream is not rewound: neither the NumPy
    generators (``rng="host"``) nor ``rng_step`` (``rng="device"``)."""
    s.iteration = 0
    s._chain = np.empty((0,) + s._lead + (s.nwalkers, s.ndim))
    s._lnprob = np.empty((0,) + s._lead + (s.nwalkers,))
    s._accepted = np.zeros(s._lead + (s.nwalkers,))
    s.n_calls = 0


def _reserve(s, total_steps):
    """Chain storage for ``total_steps`` steps in all; the rows already held are kept."""
    total = int(total_steps)
    if total > s._chain.shape[0]:
        chain, lnprob = np.empty((total,) + s._chain.shape[1:]), np.empty((total,) + s._lnprob.shape[1:])
        chain[:s.iteration], lnprob[:s.iteration] = s._chain[:s.iteration], s._lnprob[:s.iteration]
        s._chain, s._lnprob = chain, lnprob


def _run_blocks(s, pos, lnp, nsteps, first, chunk, draw, evaluate, store=True):
    """Advance ``pos`` / ``lnp`` (C-contiguous, updated in place) by ``nsteps`` steps in blocks of ``first``, then ``chunk``
    steps.  A block runs in one of three ways:

    * ``rng="device"`` with ``seeded_block_fn``: inside the library, its numbers generated there;
    * ``rng="host"`` with ``block_fn``: inside the library (csrc/mcd_stretch.h), from the numbers ``draw(n)`` returns.  The
      numbers of the NEXT block are drawn by a helper thread while the library call of this one waits for the device
      (both release the interpreter lock).  One drawing thread at a time, blocks drawn in order: the stream of random
      numbers is the serial one.  (If the library call raises, the generators have already moved past the block that
      was never run.)
    * otherwise the NumPy half-step loop below, around ``evaluate`` (proposals lead + (W/2, P) -> lead + (W/2,); it
      counts its calls in ``n_calls``), with the numbers of ``draw`` -- or, with ``rng="device"``, of ``_native.chain_numbers``: the ones the device generates.

    ``move="de"`` (always ``rng="device"``): the numbers are ``_native.de_numbers``' and ``seeded_block_fn`` is the DE block.
    """
    nsteps = int(nsteps)
    if store and s.iteration + nsteps > s._chain.shape[0]:    # geometric growth: amortised O(1) per stored step
        _reserve(s, max(s.iteration + nsteps, 2 * s._chain.shape[0]))
    device = s.rng == "device"
    if device:
        from . import _native

        def draw(n):                                          # noqa: F811 -- the same numbers the device generates
            if s.move == "de":
                return _native.de_numbers(s.seed64, s.rng_step, n, lnp.size // s.nwalkers, s.nwalkers, s.ndim, s.gamma0,
                                          s.sigma, squeeze=not s._lead)
            return _native.chain_numbers(s.seed64, s.rng_step, n, lnp.size // s.nwalkers, s.nwalkers, s.ndim,
                                         squeeze=not s._lead)
    library = s.seeded_block_fn if device else s.block_fn
    lookahead = None
    if library is not None and not device and nsteps > first:
        from concurrent.futures import ThreadPoolExecutor
        lookahead = ThreadPoolExecutor(max_workers=1)
    pending, done = None, 0
    try:
        while done < nsteps:
            n = min(first if done == 0 else chunk, nsteps - done)
            it = s.iteration
            rows = (s._chain[it:it + n], s._lnprob[it:it + n]) if store else (None, None)
            if device and library is not None:
                numbers = (s.seed64, s.rng_step, n)
            else:
                numbers = pending.result() if pending is not None else draw(n)
                pending = None
                if lookahead is not None and done + n < nsteps:
                    pending = lookahead.submit(draw, min(chunk, nsteps - done - n))
            if library is None:
                _half_steps(s, pos, lnp, numbers, evaluate, store)
            else:
                accepted = np.zeros(s._lead + (s.nwalkers,), dtype=np.int64)
                library(pos, lnp, *numbers, *rows, accepted)
                s._accepted += accepted
                s.iteration += n
                s.rng_step += n
                s.n_calls += 2 * n
            done += n
    finally:
        if lookahead is not None:
            lookahead.shutdown()                              # (waits for a pending draw: only when the library call raised)


def _half_steps(s, pos, lnp, numbers, evaluate, store):
    """The move in NumPy, one block of steps: every half step proposes for one half of every ensemble against the
    other half, in one ``evaluate`` call.  Walkers are addressed as rows of the flat (B * W, P) ensemble.  ``move="de"``:
    ``numbers`` are ``_native.de_numbers``' (order, pick_a, pick_b, gamma, thr); the proposal is ``s + (x_a - x_b) * g`` --
    three separate roundings, as csrc/mcd_de.h writes them."""
    de = s.move == "de"
    pick2_b = None
    if de:
        order_b, pick_b, pick2_b, zz_b, thr_b = numbers
    else:
        order_b, zz_b, thr_b, pick_b = numbers
    n, W, P = order_b.shape[0], s.nwalkers, s.ndim
    B, half = lnp.size // W, W // 2
    flat_pos, flat_lnp, flat_acc = pos.reshape(B * W, P), lnp.reshape(B * W), s._accepted.reshape(B * W)
    if not (np.may_share_memory(flat_pos, pos) and np.may_share_memory(flat_lnp, lnp)):
        raise ValueError("the NumPy loop updates pos and lnp in place: they must be C-contiguous")
    order_b = order_b.reshape(n, B, W) + (W * np.arange(B))[:, None]                 # ensemble b's walkers: rows b * W + j
    pick_b = pick_b.reshape(n, 2, B, half) + (half * np.arange(B))[:, None]          # partner of half-row b * half + j
    if de:
        pick2_b = pick2_b.reshape(n, 2, B, half) + (half * np.arange(B))[:, None]
    zz_b, thr_b = zz_b.reshape(n, 2, B * half), thr_b.reshape(n, 2, B * half)
    for i in range(n):
        order = order_b[i]
        halves = (order[:, :half].ravel(), order[:, half:].ravel())
        for h in (0, 1):
            first, second = halves[h], halves[1 - h]
            s_pos = flat_pos[first]
            partners = flat_pos[second[pick_b[i, h].ravel()]]
            if de:
                proposal = s_pos + (partners - flat_pos[second[pick2_b[i, h].ravel()]]) * zz_b[i, h][:, None]
            else:
                proposal = partners - (partners - s_pos) * zz_b[i, h][:, None]
            new_lnp = np.reshape(evaluate(proposal.reshape(s._lead + (half, P))), B * half)
            accept = thr_b[i, h] < new_lnp - flat_lnp[first]
            idx = first[accept]
            flat_pos[idx] = proposal[accept]
            flat_lnp[idx] = new_lnp[accept]
            flat_acc[idx] += 1
        if store:
            s._chain[s.iteration] = pos
            s._lnprob[s.iteration] = lnp
        s.iteration += 1
        s.rng_step += 1


class EnsembleSampler(object):

    def __init__(self, nwalkers, ndim, log_prob_fn, pool=None, a=2.0, vectorize=False, seed=None, block_fn=None, rng="host",
                 seeded_block_fn=None, move="stretch", gamma0=None, sigma=1e-5):
        """``rng``: ``"host"`` (NumPy's Mersenne twister, as emcee) or ``"device"`` (the counter-based generator of
        csrc/mcd_rng.h, see ``_setup``).  ``move``: ``"stretch"`` or ``"de"`` (differential evolution with scale ``gamma0``
        and jitter ``sigma``, see ``_setup``; needs ``rng="device"``)."""
        _setup(self, (), nwalkers, ndim, a, rng, seed, block_fn, seeded_block_fn, move, gamma0, sigma)
        self.log_prob_fn = log_prob_fn
        self.pool = pool
        self.vectorize = bool(vectorize)
        # steps whose random numbers are drawn together (and, with block_fn, run as one library call: the device then
        # idles only once per block while the results travel back and the next block goes up, ~0.1 ms).  Part of the
        # definition of the random stream: samplers that should produce the same chain need the same value.  Also the
        # block length of rng="device" runs (there NOT part of the stream's definition).
        self.block_steps = 256
        # ... except the FIRST block of a run with several blocks: its draws cannot overlap anything (nothing runs yet), so it
        # is kept short -- the device starts after 0.8 ms of draws instead of 3 ms (1e5 stars x 256 walkers: 3 of 39 us per
        # step over a 1024-step run).  Also part of the definition of the random stream.
        self.first_block_steps = 64
        self._random = np.random.RandomState(_host_seed(self, seed))

    def reset(self):
        """Drop the chain, the log-probabilities, the acceptance counts and ``n_calls``; ``iteration`` is 0 again.  The
        random stream carries on where it stands, in both modes (``_clear``): a production run after a burn-in never
        replays the numbers that produced its own starting point."""
        _clear(self)

    # ------------------------------------------------------------------ emcee-compatible views
    @property
    def chain(self):
        """(nwalkers, nsteps, ndim), the layout the reference pickles (runner.py:471-472)."""
        return np.swapaxes(self._chain[:self.iteration], 0, 1)

    @property
    def lnprobability(self):
        return np.swapaxes(self._lnprob[:self.iteration], 0, 1)

    @property
    def flatchain(self):
        return self._chain[:self.iteration].reshape(-1, self.ndim)

    @property
    def acceptance_fraction(self):
        return self._accepted / max(1, self.iteration)

    def get_chain(self, discard=0, flat=False):
        c = self._chain[discard:self.iteration]
        return c.reshape(-1, self.ndim) if flat else c

    def get_log_prob(self, discard=0, flat=False):
        lp = self._lnprob[discard:self.iteration]
        return lp.reshape(-1) if flat else lp

    def get_autocorr_time(self, discard=0, thin=1, **kwargs):
        """The integrated autocorrelation time per parameter in steps, as emcee's method of this name (``c``, ``tol``,
        ``quiet``; ``diagnostics.integrated_time`` has the rest): computed on the device beside the chain."""
        from .diagnostics import sampler_autocorr_time
        return sampler_autocorr_time(self, discard=discard, thin=thin, **kwargs)

    @property
    def random_state(self):
        return self._random.get_state()

    # ------------------------------------------------------------------ posterior calls
    def compute_log_prob(self, coords):
        return self._log_prob(coords, checked=True)

    def _log_prob(self, coords, checked):
        """(n, P) -> (n,) with emcee's checks, one call in ``n_calls``.  ``checked``: convert and check the coordinates
        first (the half steps of a vectorised run skip that: its proposals are finite float64 arrays already)."""
        if checked:
            coords = np.asarray(coords, dtype=np.float64)
            if not np.isfinite(coords).all():
                raise ValueError("At least one parameter value was infinite or NaN")
        if self.vectorize:
            lp = np.asarray(self.log_prob_fn(coords), dtype=np.float64)
        elif self.pool is not None:
            lp = np.array([float(x) for x in self.pool.map(self.log_prob_fn, list(coords))], dtype=np.float64)
        else:
            lp = np.array([float(self.log_prob_fn(c)) for c in coords], dtype=np.float64)
        self.n_calls += 1
        if lp.shape != (coords.shape[0],):
            raise ValueError("log_prob_fn returned shape {0} for {1} positions".format(lp.shape, coords.shape[0]))
        if np.isnan(lp).any():
            raise ValueError("Probability function returned NaN")
        return lp

    # ------------------------------------------------------------------ sampling
    def _draw(self, block):
        # Random numbers for a block of steps in a handful of vectorised draws (the per-step host cost is what limits the
        # sampler once the posterior call takes ~0.1 ms): split of the ensemble = argsort of uniform keys, stretch factors
        # z ~ g(z) and log acceptance thresholds, partner indices.  The generator is consumed in this order by ONE thread
        # (the stream is the serial one); what follows the raw draws -- the row-wise argsort and the logarithms, 80 % of the
        # time -- is a pure function of them and is spread over a few threads by rows (NumPy releases the interpreter lock
        # there): at 1e5 stars a 256-step block of 256 walkers takes the device 9 ms and one host thread 8 ms to draw.
        half = self.nwalkers // 2
        inv_a, am1, dm1 = 1.0 / self.a, self.a - 1.0, self.ndim - 1.0
        keys = self._random.rand(block, self.nwalkers)
        u = self._random.rand(block, 4, half)
        pick_b = self._random.randint(half, size=(block, 2, half)).astype(np.int32)
        order_b = np.empty((block, self.nwalkers), dtype=np.int32)
        zz_b = np.empty((block, 2, half))
        thr_b = np.empty((block, 2, half))

        def rows(lo, hi):
            order_b[lo:hi] = np.argsort(keys[lo:hi], axis=1)
            z = am1 * u[lo:hi, :2] + 1.0
            z *= z
            z *= inv_a
            zz_b[lo:hi] = z
            thr_b[lo:hi] = np.log(u[lo:hi, 2:]) - dm1 * np.log(z)      # accept iff thr < new_lnp - old_lnp

        workers = _draw_pool()
        if workers is None or block < 32:
            rows(0, block)
        else:
            n_parts = 4
            edges = [block * k // n_parts for k in range(n_parts + 1)]
            for f in [workers.submit(rows, edges[k], edges[k + 1]) for k in range(n_parts)]:
                f.result()
        return order_b, zz_b, thr_b, pick_b

    def run_mcmc(self, initial_state, nsteps, log_prob0=None, rstate0=None, progress=False, store=True, **kwargs):
        """Advance the ensemble by ``nsteps``.  Returns ``(pos, log_prob, random_state)``."""
        pos = np.array(initial_state, dtype=np.float64)
        if pos.shape != (self.nwalkers, self.ndim):
            raise ValueError("incompatible input dimensions {0}".format(pos.shape))
        if rstate0 is not None:
            self._random.set_state(rstate0)
        lnp = np.array(self.compute_log_prob(pos) if log_prob0 is None else log_prob0, dtype=np.float64)
        if np.shape(lnp) != (self.nwalkers,):
            raise ValueError("incompatible input dimensions for log_prob0")
        # (the same partition into blocks with and without block_fn: the two then consume the generator alike; rng="device"
        # has no draws to hide: equal blocks)
        chunk = max(1, int(self.block_steps))
        first = chunk if self.rng == "device" or int(nsteps) <= chunk else max(1, min(chunk, int(self.first_block_steps)))
        _run_blocks(self, pos, lnp, nsteps, first, chunk, self._draw,
                    lambda proposal: self._log_prob(proposal, checked=not self.vectorize), store=store)
        return pos, lnp, self._random.get_state()


class HMCSampler(object):
    """Hamiltonian Monte Carlo on the device gradient: ``nwalkers`` independent chains, each step ``n_leap`` leapfrog
    points with step size ``step_size`` (jittered by ``jitter`` per walker and step) in the metric whose INVERSE mass
    matrix is ``chol @ chol.T`` -- the lower Cholesky factor of a posterior covariance estimate (csrc/mcd_hmc.h; the
    reference has no gradient-based sampler).  A sampler the user asks for by name (``Runner.hmc``), with the attributes
    the other samplers expose plus ``energy_error``.

    ``block_fn(pos, lnp, chol, step_size, n_leap, jitter, seed, step0, n_steps, chain, lnprob_chain, accepted,
    energy_error)`` advances ``pos`` (W, P) in place by a block of steps and writes ``lnp`` (``Runner._hmc_block``:
    ``mcd_hmc_block``, resident on the device where it can be).

    The numbers of a step are a function of (seed, step counter, walker).  The step counter ``rng_step`` only ever grows:
    ``reset()`` empties the chain and the acceptance counts and leaves it alone, so a production run after a burn-in
    never replays the numbers that produced its own starting point."""

    def __init__(self, nwalkers, ndim, block_fn, chol, step_size, n_leap=8, jitter=0.1, seed=None):
        chol = np.array(chol, dtype=np.float64)
        if chol.shape != (ndim, ndim):
            raise ValueError("chol must have shape (ndim, ndim)")
        if np.any(np.triu(chol, 1) != 0.0) or np.any(np.diag(chol) <= 0.0) or not np.isfinite(chol).all():
            raise ValueError("chol must be a finite lower-triangular matrix with a positive diagonal")
        if not (step_size > 0.0) or not (0.0 <= jitter < 1.0) or int(n_leap) < 1 or int(nwalkers) < 1:
            raise ValueError("step_size > 0, 0 <= jitter < 1, n_leap >= 1 and nwalkers >= 1")
        self.nwalkers, self.ndim, self.block_fn = int(nwalkers), int(ndim), block_fn
        self.chol, self.step_size, self.n_leap, self.jitter = chol, float(step_size), int(n_leap), float(jitter)
        self.seed64 = int(seed) & 0xFFFFFFFFFFFFFFFF if seed is not None else \
            (int(np.random.randint(0, 2 ** 32)) << 32) | int(np.random.randint(0, 2 ** 32))
        self.block_steps = 64                    # steps per library call (NOT part of the stream's definition)
        self.rng_step = 0                        # the generator's step counter: never rewound
        self.reset()

    def reset(self):
        """Drop the chain, the acceptance counts and the energy errors.  The generator's step counter stays."""
        self.iteration = 0
        self._chain = np.empty((0, self.nwalkers, self.ndim))
        self._lnprob = np.empty((0, self.nwalkers))
        self._energy = np.empty((0, self.nwalkers))
        self._accepted = np.zeros(self.nwalkers)
        self.n_calls = 0                         # value-and-gradient evaluations of W rows

    def reserve(self, total_steps):
        """Chain storage for ``total_steps`` steps in all; the rows already held are kept."""
        total = int(total_steps)
        if total > self._chain.shape[0]:
            for name in ("_chain", "_lnprob", "_energy"):
                old = getattr(self, name)
                new = np.empty((total,) + old.shape[1:])
                new[:self.iteration] = old[:self.iteration]
                setattr(self, name, new)

    @property
    def chain(self):
        """(nwalkers, nsteps, ndim), the layout the reference pickles (runner.py:471-472)."""
        return np.swapaxes(self._chain[:self.iteration], 0, 1)

    @property
    def lnprobability(self):
        return np.swapaxes(self._lnprob[:self.iteration], 0, 1)

    @property
    def energy_error(self):
        """(nwalkers, nsteps): |H1 - H0| of every proposal, +inf for a trajectory that ended early (left the box in a
        dense metric, or met a non-finite value)."""
        return np.swapaxes(self._energy[:self.iteration], 0, 1)

    @property
    def flatchain(self):
        return self._chain[:self.iteration].reshape(-1, self.ndim)

    @property
    def acceptance_fraction(self):
        return self._accepted / max(1, self.iteration)

    def get_chain(self, discard=0, flat=False):
        c = self._chain[discard:self.iteration]
        return c.reshape(-1, self.ndim) if flat else c

    def get_log_prob(self, discard=0, flat=False):
        lp = self._lnprob[discard:self.iteration]
        return lp.reshape(-1) if flat else lp

    def get_autocorr_time(self, discard=0, thin=1, **kwargs):
        """The integrated autocorrelation time per parameter in steps, as emcee's method of this name (``c``, ``tol``,
        ``quiet``; ``diagnostics.integrated_time`` has the rest): computed on the device beside the chain."""
        from .diagnostics import sampler_autocorr_time
        return sampler_autocorr_time(self, discard=discard, thin=thin, **kwargs)

    def run_mcmc(self, initial_state, nsteps, **kwargs):
        """Advance the chains by ``nsteps``.  Returns ``(pos, log_prob, None)``."""
        pos = np.array(initial_state, dtype=np.float64)
        if pos.shape != (self.nwalkers, self.ndim):
            raise ValueError("incompatible input dimensions {0}".format(pos.shape))
        if not np.isfinite(pos).all():
            raise ValueError("At least one parameter value was infinite or NaN")
        nsteps = int(nsteps)
        if self.iteration + nsteps > self._chain.shape[0]:
            self.reserve(max(self.iteration + nsteps, 2 * self._chain.shape[0]))
        lnp = np.full(self.nwalkers, np.nan)
        done = 0
        while done < nsteps:
            n = min(max(1, int(self.block_steps)), nsteps - done)
            it = self.iteration
            accepted = np.zeros(self.nwalkers, dtype=np.int64)
            self.block_fn(pos, lnp, self.chol, self.step_size, self.n_leap, self.jitter, self.seed64, self.rng_step, n,
                          self._chain[it:it + n], self._lnprob[it:it + n], accepted, self._energy[it:it + n])
            self._accepted += accepted
            self.iteration += n
            self.rng_step += n
            self.n_calls += 1 + n * self.n_leap
            done += n
        return pos, lnp, None


def default_ladder(n_temps, beta_ratio=0.5, proper=True):
    """The default ladder of inverse temperatures: geometric from 1 with ratio ``beta_ratio``, ending -- when the prior is
    ``proper`` -- with a rung at beta = 0, which samples the prior and anchors the evidence: ``n_temps - 1`` geometric
    rungs and the zero.  With an improper prior beta = 0 has no distribution: ``n_temps`` geometric rungs, no zero."""
    n_temps = int(n_temps)
    if n_temps < 1 or not (0.0 < beta_ratio < 1.0):
        raise ValueError("n_temps >= 1 and 0 < beta_ratio < 1")
    if proper and n_temps > 1:
        return np.concatenate([float(beta_ratio) ** np.arange(n_temps - 1), [0.0]])
    return float(beta_ratio) ** np.arange(n_temps)


class TemperedSampler(object):
    """Parallel tempering: ``len(betas)`` ensembles of ``nwalkers`` walkers, rung t sampling prior(x) L(x)^betas[t]
    (``betas[0] == 1``, strictly decreasing, >= 0), each advanced by the stretch move, adjacent rungs exchanging walkers by
    a Metropolis swap (csrc/mcd_temper.h; the reference has one ensemble at one temperature).  It crosses between separated
    modes, which one ensemble cannot, and its rungs' log-likelihood series give the marginal likelihood
    (``log_evidence``).  A sampler the user asks for by name (``Runner.tempered``); rung 0 is the posterior and carries the
    attributes the other samplers expose.

    ``block_fn(betas, pos, lnlike, lnprior, seed, step0, n_steps, chain, lnlike_chain, accepted, swap_proposed,
    swap_accepted)`` advances ``pos`` (T, W, P) and ``lnlike`` (T, W) in place by a block of steps and writes ``lnprior``
    (``Runner._temper_block``: ``mcd_temper_block``, resident on the device where it can be).  ``lnlike_fn((n, P)) ->
    (n,)`` evaluates the start, in two calls of T W/2 rows (``Runner._temper_lnlike``: the plain kernels, as the block); ``lnprior_fn((n, P)) -> (n,)``, or None for a flat prior, is what ``lnprobability`` adds
    to rung 0's log-likelihood.  ``store_temps``: the positions of rungs 0 .. store_temps - 1 are kept (the log-likelihood
    of every rung always is).  ``improper``: names of the free parameters without a proper prior (``log_evidence`` then
    raises).

    The numbers of a step are a function of (seed, step counter, rung, walker); the step counter ``rng_step`` only ever
    grows, as ``HMCSampler``'s."""

    def __init__(self, nwalkers, ndim, betas, block_fn, lnlike_fn, lnprior_fn=None, seed=None, store_temps=1, improper=()):
        betas = np.array(betas, dtype=np.float64).reshape(-1)
        if betas.size < 1 or betas[0] != 1.0 or np.any(np.diff(betas) >= 0.0) or betas[-1] < 0.0 or not np.isfinite(betas).all():
            raise ValueError("betas must start at 1 and decrease strictly to a value >= 0")
        if int(nwalkers) < 2 or int(nwalkers) % 2:
            raise ValueError("nwalkers must be even and >= 2")
        if not 1 <= int(store_temps) <= betas.size:
            raise ValueError("store_temps must lie in 1 .. len(betas)")
        self.nwalkers, self.ndim, self.betas, self.ntemps = int(nwalkers), int(ndim), betas, int(betas.size)
        self.block_fn, self.lnlike_fn, self.lnprior_fn = block_fn, lnlike_fn, lnprior_fn
        self.store_temps, self.improper = int(store_temps), tuple(improper)
        self.seed64 = int(seed) & 0xFFFFFFFFFFFFFFFF if seed is not None else \
            (int(np.random.randint(0, 2 ** 32)) << 32) | int(np.random.randint(0, 2 ** 32))
        self.block_steps = 64                    # steps per library call (NOT part of the stream's definition)
        self.rng_step = 0                        # the generator's step counter: never rewound
        self.reset()

    def reset(self):
        """Drop the chain and the counts.  The generator's step counter stays."""
        self.iteration = 0
        self._chain = np.empty((0, self.store_temps, self.nwalkers, self.ndim))
        self._lnlike = np.empty((0, self.ntemps, self.nwalkers))
        self._accepted = np.zeros((self.ntemps, self.nwalkers), dtype=np.int64)
        self._swap_proposed = np.zeros(self.ntemps - 1, dtype=np.int64)
        self._swap_accepted = np.zeros(self.ntemps - 1, dtype=np.int64)

    def reserve(self, total_steps):
        """Chain storage for ``total_steps`` steps in all; the rows already held are kept."""
        total = int(total_steps)
        if total > self._chain.shape[0]:
            for name in ("_chain", "_lnlike"):
                old = getattr(self, name)
                new = np.empty((total,) + old.shape[1:])
                new[:self.iteration] = old[:self.iteration]
                setattr(self, name, new)

    @property
    def chain(self):
        """Rung 0, the posterior: (nwalkers, nsteps, ndim), the layout the reference pickles (runner.py:471-472)."""
        return np.swapaxes(self._chain[:self.iteration, 0], 0, 1)

    @property
    def flatchain(self):
        return self._chain[:self.iteration, 0].reshape(-1, self.ndim)

    @property
    def lnlikelihood(self):
        """(ntemps, nwalkers, nsteps): the log-likelihood of every rung's walkers after every step."""
        return np.transpose(self._lnlike[:self.iteration], (1, 2, 0))

    @property
    def lnprobability(self):
        """Rung 0: log-likelihood plus log-prior, (nwalkers, nsteps)."""
        ll = np.swapaxes(self._lnlike[:self.iteration, 0], 0, 1)
        if self.lnprior_fn is None:
            return ll
        lp = np.asarray(self.lnprior_fn(self._chain[:self.iteration, 0].reshape(-1, self.ndim)))
        return ll + np.swapaxes(lp.reshape(self.iteration, self.nwalkers), 0, 1)

    @property
    def acceptance_fraction(self):
        """(ntemps, nwalkers): accepted stretch-move proposals per step, by slot (rung, walker index)."""
        return self._accepted / float(max(1, self.iteration))

    @property
    def swap_acceptance_fraction(self):
        """(ntemps - 1,): accepted over proposed swaps of the pairs (t, t + 1)."""
        return self._swap_accepted / np.maximum(1, self._swap_proposed).astype(np.float64)

    def get_chain(self, temp=0, discard=0, flat=False):
        """Steps first: (nsteps, nwalkers, ndim) of rung ``temp`` (< store_temps)."""
        if not 0 <= int(temp) < self.store_temps:
            raise ValueError("positions are stored for rungs 0 .. {0} (store_temps)".format(self.store_temps - 1))
        c = self._chain[discard:self.iteration, int(temp)]
        return c.reshape(-1, self.ndim) if flat else c

    def get_log_prob(self, discard=0, flat=False):
        lp = np.swapaxes(self.lnprobability, 0, 1)[discard:]
        return lp.reshape(-1) if flat else lp

    def get_autocorr_time(self, discard=0, thin=1, **kwargs):
        """The integrated autocorrelation time per parameter of rung 0, in steps (``diagnostics.integrated_time``)."""
        from .diagnostics import sampler_autocorr_time
        return sampler_autocorr_time(self, discard=discard, thin=thin, **kwargs)

    def log_evidence(self, discard=0):
        """``analysis.runner.evidence_summary`` of this run's log-likelihood series after ``discard`` steps."""
        if self.improper:
            raise ValueError("log_evidence needs a proper prior: no finite bounds and no normal / log-normal prior on " +
                             ", ".join(self.improper))
        from .analysis.runner import evidence_summary
        return evidence_summary(self.lnlikelihood, self.betas, discard=discard)

    def run_mcmc(self, initial_state, nsteps, **kwargs):
        """Advance every rung by ``nsteps``.  ``initial_state``: (W, P), the same start for every rung, or (T, W, P).
        Returns ``(pos (T, W, P), lnlike (T, W), None)``."""
        pos = np.array(initial_state, dtype=np.float64)
        if pos.shape == (self.nwalkers, self.ndim):
            pos = np.repeat(pos[None], self.ntemps, axis=0)
        if pos.shape != (self.ntemps, self.nwalkers, self.ndim):
            raise ValueError("incompatible input dimensions {0}".format(pos.shape))
        if not np.isfinite(pos).all():
            raise ValueError("At least one parameter value was infinite or NaN")
        pos = np.ascontiguousarray(pos)
        nsteps = int(nsteps)
        if self.iteration + nsteps > self._chain.shape[0]:
            self.reserve(max(self.iteration + nsteps, 2 * self._chain.shape[0]))
        # the start's log-likelihood in the launch shape of a half step, T W/2 rows: with ``Runner._temper_lnlike`` behind
        # ``lnlike_fn`` these are the values the block's own kernels would give (the order of a sum belongs to the row count)
        flat = pos.reshape(-1, self.ndim)
        rows = flat.shape[0] // 2
        lnlike = np.ascontiguousarray(np.concatenate([np.asarray(self.lnlike_fn(flat[:rows]), dtype=np.float64),
                                                      np.asarray(self.lnlike_fn(flat[rows:]), dtype=np.float64)])
                                      .reshape(self.ntemps, self.nwalkers))
        lnprior = np.zeros((self.ntemps, self.nwalkers))
        done = 0
        while done < nsteps:
            n = min(max(1, int(self.block_steps)), nsteps - done)
            it = self.iteration
            self.block_fn(self.betas, pos, lnlike, lnprior, self.seed64, self.rng_step, n, self._chain[it:it + n],
                          self._lnlike[it:it + n], self._accepted, self._swap_proposed, self._swap_accepted)
            self.iteration += n
            self.rng_step += n
            done += n
        return pos, lnlike, None

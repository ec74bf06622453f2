"""mcmc_dynamics_amd.optimize.maximize_batch on log-densities with known maxima (no GPU, no library)."""
import numpy as np

from mcmc_dynamics_amd.optimize import maximize_batch

P = 6


def gaussian(seed=3):
    """A 6-dimensional correlated Gaussian log-density with axis scales over two decades: (callable, mode, sd, precision)."""
    rng = np.random.default_rng(seed)
    sd = 10.0 ** rng.uniform(-1, 1, P)
    q, _ = np.linalg.qr(rng.normal(size=(P, P)))
    corr = q @ np.diag(rng.uniform(0.2, 1.8, P)) @ q.T
    dinv = np.diag(1.0 / np.sqrt(np.diag(corr)))
    corr = dinv @ corr @ dinv
    cov = corr * np.outer(sd, sd)
    prec = np.linalg.inv(cov)
    mode = rng.normal(0, 3, P) * sd

    def f(x):
        d = x - mode
        return -0.5 * np.einsum("wi,ij,wj->w", d, prec, d), -d @ prec
    return f, mode, sd, prec


def starts(mode, sd, seed=5, n=64):
    return mode + np.random.default_rng(seed).normal(0, 5, (n, P)) * sd


def test_correlated_gaussian_from_64_starts():
    f, mode, sd, _ = gaussian()
    # (the correlation matrix has condition number ~9: a scaled gradient of 1e-10 bounds the scaled distance by ~1e-9)
    res = maximize_batch(f, starts(mode, sd), -np.inf, np.inf, max_iter=200, gtol=1e-10, scale=sd)
    assert res["converged"].all() and res["n_iter"].max() <= 200
    assert np.max(np.abs(res["x"] - mode) / sd) < 1e-8
    assert res["x"].shape == (64, P) and res["f"].shape == (64,) and res["grad"].shape == (64, P)


def test_mode_outside_the_box_gives_the_constrained_maximum():
    f, mode, sd, prec = gaussian()
    lo, hi = mode - 20 * sd, mode + 20 * sd
    hi[1] = mode[1] - 2 * sd[1]                       # the mode lies above the box in coordinate 1
    lo[4] = mode[4] + 1 * sd[4]                       # ... and below it in coordinate 4
    x0 = np.clip(starts(mode, sd), lo, hi)
    res = maximize_batch(f, x0, lo, hi, max_iter=200, gtol=1e-8, scale=sd)
    assert res["converged"].all()
    assert np.all(res["x"][:, 1] == hi[1]) and np.all(res["x"][:, 4] == lo[4])
    # the constrained maximum of a Gaussian: the free coordinates solve prec_ff (x_f - m_f) = -prec_fc (x_c - m_c)
    fixed = np.array([1, 4])
    free = np.array([0, 2, 3, 5])
    dc = np.array([hi[1], lo[4]]) - mode[fixed]
    want = mode.copy()
    want[fixed] += dc
    want[free] += np.linalg.solve(prec[np.ix_(free, free)], -prec[np.ix_(free, fixed)] @ dc)
    assert np.max(np.abs(res["x"] - want) / sd) < 1e-7
    g = res["grad"].copy()
    assert np.all(g[:, 1] > 0) and np.all(g[:, 4] < 0)              # pushing out of the box: removed by the projection
    g[:, fixed] = 0.0
    assert np.all(np.max(np.abs(g) * sd, axis=1) <= 1e-8)              # per start: projected gradient <= gtol


def test_minus_infinity_beyond_a_wall_backtracks():
    f, mode, sd, _ = gaussian()
    wall = mode[0] + 0.5 * sd[0]                      # the density is -inf (gradient NaN) beyond a wall the box does not know

    def walled(x):
        v, g = f(x)
        out = x[:, 0] > wall
        v = np.where(out, -np.inf, v)
        g = np.where(out[:, None], np.nan, g)
        return v, g
    x0 = starts(mode, sd)
    x0[:, 0] = mode[0] - np.abs(x0[:, 0] - mode[0])   # every start on the finite side; first full steps overshoot the wall
    res = maximize_batch(walled, x0, -np.inf, np.inf, max_iter=200, gtol=1e-8, scale=sd)
    assert np.all(np.isfinite(res["x"])) and np.all(np.isfinite(res["f"])) and np.all(np.isfinite(res["grad"]))
    assert np.all(res["x"][:, 0] <= wall)
    assert res["converged"].all()
    assert np.max(np.abs(res["x"] - mode) / sd) < 1e-7
    # a start that is itself infeasible stays where it is, flagged as not converged
    x0[0, 0] = wall + sd[0]
    res = maximize_batch(walled, x0, -np.inf, np.inf, max_iter=50, scale=sd)
    assert not res["converged"][0] and res["f"][0] == -np.inf and np.all(res["x"][0] == x0[0]) and res["converged"][1:].all()


def test_repetition_is_bit_identical():
    f, mode, sd, _ = gaussian()
    a = maximize_batch(f, starts(mode, sd), mode - 3 * sd, mode + 30 * sd, scale=sd)
    b = maximize_batch(f, starts(mode, sd), mode - 3 * sd, mode + 30 * sd, scale=sd)
    for key in ("x", "f", "grad", "n_iter", "converged"):
        assert a[key].tobytes() == b[key].tobytes(), key

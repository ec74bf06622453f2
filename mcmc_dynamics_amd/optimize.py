"""Batched, box-constrained quasi-Newton maximisation (NumPy only).

``maximize_batch`` advances W independent starts in lockstep: every trial step of every start goes into ONE call of
``value_and_grad`` on a (W, P) array, which is what the device gradient kernel wants (lane = walker: 64 rows fill a
wavefront).  It is a pure function of its callable, so it is testable without a GPU."""
import numpy as np


def _projected_gradient(x, g, lo, hi):
    """The gradient of a maximisation with the components that push out of the box removed."""
    pg = g.copy()
    pg[(x <= lo) & (g < 0)] = 0.0
    pg[(x >= hi) & (g > 0)] = 0.0
    return pg


def maximize_batch(value_and_grad, x0, lo, hi, max_iter=200, gtol=1e-8, scale=None):
    """Maximise ``f`` from every row of ``x0`` (W, P) inside the box ``lo <= x <= hi`` (each (P,), +-inf: no bound).

    ``value_and_grad(x)`` takes (W, P) and returns (f (W,), g (W, P)); ``-inf`` (or NaN) values mark infeasible rows.
    Projected BFGS: per start an inverse-Hessian estimate (of -f), restricted to the variables that are not held at a
    bound, gives the direction; the step is projected into the box and halved until the value rises enough (all
    starts backtrack in lockstep, a start that has its step simply repeats its point).  A start is converged when
    max_j |projected gradient_j| * scale_j <= gtol; ``scale`` (P,) defaults to max(|x0_j|, 1) over the starts -- the
    parameter scale that makes the criterion independent of units.

    Returns a dict: x (W, P), f (W,), grad (W, P), n_iter (W,) iterations each start took, converged (W,) bool,
    n_calls (value_and_grad calls).  Deterministic: the same callable and starts give the same bits."""
    x = np.array(x0, dtype=np.float64, copy=True)
    if x.ndim != 2:
        raise ValueError("x0 must have shape (W, P)")
    n_w, n_p = x.shape
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float64), (n_p,))
    hi = np.broadcast_to(np.asarray(hi, dtype=np.float64), (n_p,))
    if np.any(lo > hi):
        raise ValueError("empty box: lo > hi")
    x = np.clip(x, lo, hi)
    scale = np.maximum(np.max(np.abs(x), axis=0), 1.0) if scale is None else np.asarray(scale, dtype=np.float64)
    calls = [0]

    def evaluate(points):
        f, g = value_and_grad(points)
        calls[0] += 1
        f = np.array(f, dtype=np.float64, copy=True)
        g = np.array(g, dtype=np.float64, copy=True)
        bad = ~np.isfinite(f) | ~np.all(np.isfinite(g), axis=1)
        f[bad] = -np.inf
        g[bad] = 0.0
        return f, g

    f, g = evaluate(x)
    h_inv = np.broadcast_to(np.diag(scale * scale), (n_w, n_p, n_p)).copy()     # inverse Hessian of -f, per start
    n_iter = np.zeros(n_w, dtype=np.int64)
    converged = np.zeros(n_w, dtype=bool)
    dead = ~np.isfinite(f)                                   # infeasible starts: nothing to climb from

    def pg_norm(x, g):
        return np.max(np.abs(_projected_gradient(x, g, lo, hi)) * scale, axis=1)

    def is_converged(x, g):
        return pg_norm(x, g) <= gtol

    converged = is_converged(x, g) & ~dead
    for _ in range(int(max_iter)):
        active = ~converged & ~dead
        if not active.any():
            break
        pg = _projected_gradient(x, g, lo, hi)
        free = pg != 0.0                                      # variables not held at a bound (and not already flat)
        # direction of ascent in the free subspace: d = H_ff g_f
        hm = h_inv * (free[:, :, None] & free[:, None, :])
        d = np.einsum("wij,wj->wi", hm, pg)
        # not an ascent direction (stale curvature): fall back to the scaled gradient
        slope = np.einsum("wi,wi->w", d, pg)
        weak = ~(slope > 0) | ~np.all(np.isfinite(d), axis=1)
        d[weak] = (pg * scale * scale)[weak]
        slope = np.einsum("wi,wi->w", d, pg)
        t = np.ones(n_w)
        x_new, f_new, g_new = x.copy(), f.copy(), g.copy()
        todo = active.copy()
        for ls in range(60):
            if not todo.any():
                break
            trial = np.where(todo[:, None], np.clip(x + t[:, None] * d, lo, hi), x_new)
            ft, gt = evaluate(trial)
            step = trial - x
            # Armijo on the projected step: f must rise by 1e-4 of the first-order prediction (never fall).  From the
            # tenth halving on any strict rise is taken: next to a pole of the gradient (a mixture weight on its bound,
            # where df/dw ~ 1 / density) no step short of 1e-10 meets a first-order prediction, yet the climb is real.
            armijo = ft >= f + 1e-4 * np.einsum("wi,wi->w", pg, step)
            ok = todo & np.isfinite(ft) & (ft >= f) & (armijo | ((ls >= 10) & (ft > f)))
            # Close to the maximum the rise a step can still give, ~|pg|^2 / curvature, falls below the rounding of f
            # itself: there a step counts when f is unchanged to a few ulps and the scaled projected gradient shrinks
            # (the approximate Wolfe test of Hager & Zhang 2005).
            with np.errstate(invalid="ignore"):
                flat = np.isfinite(ft) & (np.abs(ft - f) <= 8 * np.finfo(np.float64).eps * np.abs(f))
            ok |= todo & flat & (pg_norm(trial, gt) < pg_norm(x, g))
            x_new[ok], f_new[ok], g_new[ok] = trial[ok], ft[ok], gt[ok]
            todo &= ~ok
            t[todo] *= 0.5
        moved = active & ~todo
        # a start whose line search found nothing keeps its point; with a reset matrix it tries the gradient next time,
        # and when that fails too it has converged as far as float64 allows
        stuck = active & todo
        # BFGS update of the inverse Hessian of -f:  s = x+ - x,  y = -(g+ - g)
        s = x_new - x
        y = -(g_new - g)
        sy = np.einsum("wi,wi->w", s, y)
        upd = moved & (sy > 1e-12 * np.sqrt(np.einsum("wi,wi->w", s, s) * np.einsum("wi,wi->w", y, y)))
        if upd.any():
            rho = np.zeros(n_w)
            rho[upd] = 1.0 / sy[upd]
            eye = np.eye(n_p)[None]
            a = eye - rho[:, None, None] * s[:, :, None] * y[:, None, :]
            new_h = np.einsum("wij,wjk,wlk->wil", a, h_inv, a) + rho[:, None, None] * s[:, :, None] * s[:, None, :]
            h_inv[upd] = new_h[upd]
        was_reset = np.all(h_inv == np.diag(scale * scale)[None], axis=(1, 2))
        h_inv[stuck] = np.diag(scale * scale)
        x, f, g = x_new, f_new, g_new
        n_iter[active] += 1
        converged = converged | (is_converged(x, g) & ~dead)
        dead = dead | (stuck & was_reset & ~converged)        # no progress along the plain gradient either
    return {"x": x, "f": f, "grad": g, "n_iter": n_iter, "converged": converged, "n_calls": calls[0]}

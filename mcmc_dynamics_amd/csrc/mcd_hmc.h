// mcd_hmc.h -- host+device: the per-walker algebra of Hamiltonian Monte Carlo (Duane et al. 1987; Neal 2011) on the device
// gradient of mcd_loglike_grad_batch.  Written once and used by the device kernels (mcd_hmc.hip), by the host-driven block
// (mcd_api_chain.hip: the same loop around mcd_loglike_grad_batch) and by the CPU harness tests/emul/hmc_emul.cpp.  No HIP
// types; compiled with -ffp-contract=off everywhere, and every operation below is an IEEE +, -, *, / or sqrt in a fixed
// order (no libm call: the logarithm is mcd_rng.h's det_log), so that host and device produce the same bits.  The reference
// has no gradient-based sampler: emcee's stretch move is its only one (analysis/runner.py:403-419).
//
// One step of walker w (absolute step index `step`), W independent chains:
//   numbers   a function of (seed, step, walker) alone: P standard normals z, the acceptance threshold thr = log(u), the
//             jitter variable r = 2 u' - 1 (hmc_normal, hmc_aux below)
//   momentum  p = L^-T z, where the caller's INVERSE mass matrix is M^-1 = L L^T (L lower triangular, P x P, row-major;
//             the Cholesky factor of a posterior covariance estimate).  Kinetic energy 1/2 |L^T p|^2, drift q += eps L (L^T p).
//             A diagonal mass is a diagonal L: there is one code path.
//   step size eps = step_size (1 + jitter r): per walker and step, which avoids periodic trajectories
//   leapfrog  half kick p += eps/2 g, then n_leap times { drift, evaluate (l, g) at q, kick } with a half kick last
//   box prior inclusive bounds lo <= q <= hi, as in mcd_stretch_desc.  DIAGONAL L: after a drift a coordinate beyond a bound
//             is mirrored at it and its momentum component negated, repeated until it is inside (at most kHmcMaxReflect
//             times, then the proposal is rejected) -- the exact dynamics of a hard wall, volume preserving and reversible.
//             DENSE L (any non-zero below the diagonal): negating one component of p is no reflection in the metric M, so
//             a trajectory that leaves the box is ENDED and its proposal rejected.  That is the Metropolis rule for a
//             target that is zero outside the box: the proposal map stays the reversible, volume-preserving leapfrog, only
//             its acceptance probability is zero there.  Detailed balance holds either way.
//   accept    iff thr < H0 - H1, H = -(lnlike + lnprior) + kinetic
//   priors    the structured priors of mcd_prior.h (HmcShared::prior; none: lnprior = 0 inside the box): their value is added
//             to the log-likelihood and their derivative to the chain rule's result at every evaluated point.  A log-normal
//             coordinate <= 0 on a trajectory is a non-finite value: the proposal is rejected; at the block's start it is
//             HMC_NONFINITE like a walker outside the box
//   rejected  also: a non-finite lnlike or gradient at any leapfrog point (a divergent trajectory), and everything when
//             fixed_ok == 0 (a fixed parameter violates its own bounds: every lnprob is -inf, as in the stretch move)
// A rejected trajectory keeps being "evaluated" at its start point (the launch needs a valid row for every walker) and
// ignores the results.
#pragma once

#include <cstdint>

#include "mcd_prior.h"
#include "mcd_rng.h"

namespace mcd {

constexpr int kHmcMaxDim = 12;                 // P <= 12 free parameters (K <= 14 kernel columns today: some stay fixed)
constexpr uint64_t kHmcKey1 = 0x6d63645f686d63ull;          // "mcd_hmc": never the stretch move's stream (kChainKey1)
// Marsaglia's polar method accepts a pair with probability pi / 4.  Each generator call holds two pairs; after
// kHmcNormalCalls calls (32 pairs) the draw gives up and returns 0.0: probability (1 - pi/4)^32 = 4.1e-22 per normal,
// i.e. never in 1e12 steps of 512 walkers x 12 dimensions (6e15 normals), and harmless if it ever did (z = 0 is the mode).
constexpr int kHmcNormalCalls = 16;
constexpr uint64_t kHmcAuxSlot = (uint64_t)1 << 32;          // counter word 2 of the per-step pair (thr, r); normals use 0 .. P-1
constexpr int kHmcMaxReflect = 8;              // mirrorings of one coordinate after one drift (more: a step larger than 4 boxes)

MCD_HD bool hmc_finite(double x) { return x - x == 0.0; }    // false for NaN and +-inf

// Standard normal of (seed, step, walker, component): u, v = 2 uniform53 - 1, s = u^2 + v^2, accepted for 0 < s < 1,
// z = u sqrt(-2 log(s) / s).  Rejected pairs advance the sub-counter (word 3 of the counter: pairs 2 c, 2 c + 1 of call c).
// `max_calls` is kHmcNormalCalls everywhere but in the test that walks into the fallback; *pairs_used (may be null): pairs drawn.
MCD_HD double hmc_normal(uint64_t seed, int64_t step, int64_t walker, int comp, int max_calls = kHmcNormalCalls,
                         int* pairs_used = nullptr) {
    int used = 0;
    for (int c = 0; c < max_calls; ++c) {
        const Philox4x64 r = philox4x64_10((uint64_t)step, (uint64_t)walker, (uint64_t)comp, (uint64_t)c, seed, kHmcKey1);
        for (int h = 0; h < 2; ++h) {
            const double u = 2.0 * uniform53(r.v[2 * h]) - 1.0, v = 2.0 * uniform53(r.v[2 * h + 1]) - 1.0;
            const double s = u * u + v * v;
            ++used;
            if (s > 0.0 && s < 1.0) {
                if (pairs_used) *pairs_used = used;
                return u * sqrt_(-2.0 * det_log(s) / s);
            }
        }
    }
    if (pairs_used) *pairs_used = used;
    return 0.0;                                                // documented fallback, see kHmcNormalCalls
}

// The step's other two numbers: thr = det_log(u) of the acceptance uniform (word 0), r = 2 u' - 1 in [-1, 1) (word 1).
MCD_HD void hmc_aux(uint64_t seed, int64_t step, int64_t walker, double& thr, double& r) {
    const Philox4x64 x = philox4x64_10((uint64_t)step, (uint64_t)walker, kHmcAuxSlot, 0, seed, kHmcKey1);
    thr = det_log(uniform53(x.v[0]));
    r = 2.0 * uniform53(x.v[1]) - 1.0;
}

// What a block shares between its walkers (pointers into host or device memory, by where the code runs).
struct HmcShared {
    int32_t n_dim = 0, k = 0;                  // P, K
    const int32_t* col_source = nullptr;       // [K]  as mcd_stretch_desc
    const double* col_const = nullptr;         // [K]
    const double* col_factor = nullptr;        // [K]
    const double* lo = nullptr;                // [P]
    const double* hi = nullptr;                // [P]
    const double* chol = nullptr;              // [P][P] lower triangular L, M^-1 = L L^T
    int32_t fixed_ok = 1;
    int32_t diagonal = 1;                      // hmc_is_diagonal(chol): reflection; 0: leaving the box ends the trajectory
    int32_t n_leap = 1;
    double step_size = 0.0, jitter = 0.0;
    PriorTable prior;                          // structured priors of the free parameters, or none
};

inline bool hmc_is_diagonal(const double* chol, int P) {
    for (int r = 0; r < P; ++r)
        for (int c = 0; c < r; ++c)
            if (chol[r * P + c] != 0.0) return false;
    return true;
}

// The state of one walker's trajectory: P-vectors with unit stride.
struct HmcWalker {
    double* q = nullptr;          // [P] position on the trajectory
    double* p = nullptr;          // [P] momentum
    double* h0 = nullptr;         // H at the start
    double* eps = nullptr;        // this step's step size
    int32_t* alive = nullptr;     // 0: the proposal is already rejected
};

// resolved kernel row of a position: mcd_stretch.h's rule, column by column
MCD_HD void hmc_row(const HmcShared& s, const double* q, double* row) {
    for (int c = 0; c < s.k; ++c) {
        const int src = s.col_source[c];
        row[c] = src < 0 ? s.col_const[c] : (s.col_factor[c] == 1.0 ? q[src] : q[src] * s.col_factor[c]);
    }
}

// Chain rule: d lnlike / d free parameter c = sum over the kernel columns j it feeds (ascending j) of
// col_factor[j] grad[j]; columns fed by fixed parameters are dropped.  gcol[j * stride]: the K column derivatives.
// Returns whether every term is finite.
MCD_HD bool hmc_chain_rule(const HmcShared& s, const double* gcol, int64_t stride, double* g) {
    bool ok = true;
    for (int c = 0; c < s.n_dim; ++c) g[c] = 0.0;
    for (int j = 0; j < s.k; ++j) {
        const int src = s.col_source[j];
        if (src < 0) continue;
        const double t = gcol[j * stride] * s.col_factor[j];
        g[src] += t;
        ok = ok && hmc_finite(t);
    }
    return ok;
}

// y = L^T p
MCD_HD void hmc_lt_mul(const HmcShared& s, const double* p, double* y) {
    const int P = s.n_dim;
    for (int c = 0; c < P; ++c) {
        double a = 0.0;
        for (int r = c; r < P; ++r) a += s.chol[r * P + c] * p[r];
        y[c] = a;
    }
}

MCD_HD double hmc_kinetic(const HmcShared& s, const double* p) {
    double y[kHmcMaxDim], e = 0.0;
    hmc_lt_mul(s, p, y);
    for (int c = 0; c < s.n_dim; ++c) e += y[c] * y[c];
    return 0.5 * e;
}

// p = L^-T z by back substitution
MCD_HD void hmc_momentum(const HmcShared& s, const double* z, double* p) {
    const int P = s.n_dim;
    for (int c = P - 1; c >= 0; --c) {
        double a = z[c];
        for (int r = c + 1; r < P; ++r) a -= s.chol[r * P + c] * p[r];
        p[c] = a / s.chol[c * P + c];
    }
}

// q += eps L (L^T p), then the box (see the head of this file).  Returns false when the trajectory ends here.
MCD_HD bool hmc_drift(const HmcShared& s, double eps, double* q, double* p) {
    const int P = s.n_dim;
    double y[kHmcMaxDim];
    hmc_lt_mul(s, p, y);
    for (int r = 0; r < P; ++r) {
        double a = 0.0;
        for (int c = 0; c <= r; ++c) a += s.chol[r * P + c] * y[c];
        q[r] += eps * a;
    }
    bool inside = true;
    for (int c = 0; c < P; ++c) {
        if (s.diagonal) {
            for (int n = 0; n < kHmcMaxReflect; ++n) {
                if (q[c] < s.lo[c]) { q[c] = s.lo[c] + (s.lo[c] - q[c]); p[c] = -p[c]; }
                else if (q[c] > s.hi[c]) { q[c] = s.hi[c] - (q[c] - s.hi[c]); p[c] = -p[c]; }
                else break;
            }
        }
        inside = inside && (q[c] >= s.lo[c]) && (q[c] <= s.hi[c]);               // false for NaN as well
    }
    return inside;
}

MCD_HD void hmc_kick(const HmcShared& s, double eps, const double* g, double* p) {
    for (int c = 0; c < s.n_dim; ++c) p[c] += eps * g[c];
}

// Start of a step: momenta, H0, the step size, the first half kick and the first drift; row = the kernel row to evaluate
// next (the start point's when the trajectory has already ended).  pos / lnp / grad: the walker's current point, its
// log-probability (likelihood plus prior) and its free-parameter gradient (all finite: the block checked its starting point).
MCD_HD void hmc_begin(const HmcShared& s, uint64_t seed, int64_t step, int64_t walker, const double* pos, double lnp,
                      const double* grad, HmcWalker t, double* row) {
    const int P = s.n_dim;
    double z[kHmcMaxDim], thr, r;
    for (int c = 0; c < P; ++c) z[c] = hmc_normal(seed, step, walker, c);
    hmc_aux(seed, step, walker, thr, r);
    hmc_momentum(s, z, t.p);
    for (int c = 0; c < P; ++c) t.q[c] = pos[c];
    *t.h0 = -lnp + hmc_kinetic(s, t.p);
    *t.eps = s.step_size * (1.0 + s.jitter * r);
    int alive = s.fixed_ok != 0;
    if (alive) {
        hmc_kick(s, 0.5 * *t.eps, grad, t.p);
        alive = hmc_drift(s, *t.eps, t.q, t.p) ? 1 : 0;
    }
    *t.alive = alive;
    hmc_row(s, alive ? t.q : pos, row);
}

// What the last point of a trajectory leaves behind.
struct HmcOutcome { bool accepted; double energy_error; };

// Leapfrog point `leap` (1 .. n_leap) has been evaluated: l = lnlike at t.q, gcol the K column derivatives there (the
// prior's value and derivative at t.q are added here).
//   leap < n_leap : full kick, drift, row = the next point
//   leap == n_leap: half kick, H1, accept / reject: pos, *lnp, grad take the new point when accepted; row is not written.
// energy_error = |H1 - H0|, +inf for a trajectory that ended early.
MCD_HD HmcOutcome hmc_leap(const HmcShared& s, uint64_t seed, int64_t step, int64_t walker, int leap, double l,
                           const double* gcol, int64_t stride, HmcWalker t, double* pos, double* lnp, double* grad,
                           double* row) {
    HmcOutcome out{false, __builtin_huge_val()};
    double g[kHmcMaxDim];
    int alive = *t.alive;
    if (alive) {
        const bool ok = hmc_chain_rule(s, gcol, stride, g);
        if (!ok || !hmc_finite(l)) alive = 0;                      // a divergent trajectory is a rejection
        if (alive && s.prior.any()) {
            if (prior_row_inside(s.prior, s.n_dim, t.q)) l += prior_row_grad(s.prior, s.n_dim, t.q, g);
            else alive = 0;                                        // a log-normal coordinate <= 0: lnprior = -inf
        }
    }
    if (leap < s.n_leap) {
        if (alive) {
            hmc_kick(s, *t.eps, g, t.p);
            alive = hmc_drift(s, *t.eps, t.q, t.p) ? 1 : 0;
        }
        *t.alive = alive;
        hmc_row(s, alive ? t.q : pos, row);
        return out;
    }
    *t.alive = alive;
    if (!alive) return out;
    hmc_kick(s, 0.5 * *t.eps, g, t.p);
    const double h1 = -l + hmc_kinetic(s, t.p);
    const double dh = *t.h0 - h1;
    double thr, r;
    hmc_aux(seed, step, walker, thr, r);
    out.energy_error = dh < 0.0 ? -dh : dh;
    if (!hmc_finite(dh)) { out.energy_error = __builtin_huge_val(); return out; }
    if (thr < dh) {
        out.accepted = true;
        for (int c = 0; c < s.n_dim; ++c) { pos[c] = t.q[c]; grad[c] = g[c]; }
        *lnp = l;
    }
    return out;
}

// ---- host: one block of steps around a value-and-gradient callable ------------------------------------------------
enum HmcStatus : int { HMC_OK = 0, HMC_NONFINITE = 1, HMC_EVAL_FAILED = 2, HMC_BAD_ARGS = 3 };

inline bool hmc_args_ok(const HmcShared& s, int64_t W) {
    if (W < 1 || s.n_dim < 1 || s.n_dim > kHmcMaxDim || s.k < 1 || s.n_leap < 1) return false;
    if (!(s.step_size > 0.0) || !hmc_finite(s.step_size) || !(s.jitter >= 0.0) || !(s.jitter < 1.0)) return false;
    for (int c = 0; c < s.n_dim; ++c)
        if (!(s.chol[c * s.n_dim + c] > 0.0) || !hmc_finite(s.chol[c * s.n_dim + c])) return false;
    for (int r = 0; r < s.n_dim; ++r)
        for (int c = 0; c < s.n_dim; ++c)
            if (!hmc_finite(s.chol[r * s.n_dim + c]) || (c > r && s.chol[r * s.n_dim + c] != 0.0)) return false;
    return true;
}

// The block's starting point: table [W][K] of pos, and after the evaluation lnp [W] (likelihood plus prior) and the
// free-parameter gradients [W][P].  HMC_NONFINITE: a walker starts outside the box or on a log-normal coordinate <= 0, or
// with a non-finite value or gradient.  (With fixed_ok == 0
// nothing is ever accepted and nothing needs to be finite.)
inline int hmc_start(const HmcShared& s, int64_t W, const double* pos, const double* ll, const double* gcols, double* lnp,
                     double* grad) {
    const int P = s.n_dim, K = s.k;
    for (int64_t w = 0; w < W; ++w) {
        bool ok = hmc_chain_rule(s, gcols + w * K, 1, grad + w * P) && hmc_finite(ll[w]);
        for (int c = 0; c < P; ++c) ok = ok && pos[w * P + c] >= s.lo[c] && pos[w * P + c] <= s.hi[c];
        if (ok && s.prior.any()) ok = prior_row_inside(s.prior, P, pos + w * P);
        if (!ok && s.fixed_ok) return HMC_NONFINITE;
        lnp[w] = ll[w];
        if (ok && s.prior.any()) lnp[w] = ll[w] + prior_row_grad(s.prior, P, pos + w * P, grad + w * P);
    }
    return HMC_OK;
}

// eval(table [W][K], W, out [W], grad [W][K]) -> 0 on success: mcd_loglike_grad_batch, or a test's callable.
// pos [W][P] is updated in place, lnp [W] is written (the block evaluates its own starting point); chain [n_steps][W][P],
// lnprob_chain [n_steps][W], energy_error [n_steps][W] and accepted [W] (incremented) may be null.
template <class Eval>
int hmc_block(const HmcShared& s, int64_t W, int64_t n_steps, double* pos, double* lnp, uint64_t seed, int64_t step0,
              double* chain, double* lnprob_chain, int64_t* accepted, double* energy_error, Eval&& eval) {
    if (!hmc_args_ok(s, W) || n_steps < 0 || step0 < 0) return HMC_BAD_ARGS;
    const int P = s.n_dim, K = s.k;
    std::vector<double> table((size_t)W * K), ll((size_t)W), gcols((size_t)W * K), grad((size_t)W * P), cur((size_t)W * P),
        cur_lnp((size_t)W), q((size_t)W * P), p((size_t)W * P), h0((size_t)W), eps((size_t)W);
    std::vector<int32_t> alive((size_t)W);
    std::vector<int64_t> acc((size_t)W, 0);
    for (int64_t w = 0; w < W; ++w) hmc_row(s, pos + w * P, table.data() + w * K);
    if (eval(table.data(), W, ll.data(), gcols.data()) != 0) return HMC_EVAL_FAILED;
    if (hmc_start(s, W, pos, ll.data(), gcols.data(), cur_lnp.data(), grad.data()) != HMC_OK) return HMC_NONFINITE;
    for (size_t x = 0; x < (size_t)W * P; ++x) cur[x] = pos[x];
    auto walker = [&](int64_t w) {
        HmcWalker t;
        t.q = q.data() + w * P; t.p = p.data() + w * P; t.h0 = &h0[w]; t.eps = &eps[w]; t.alive = &alive[w];
        return t;
    };
    for (int64_t i = 0; i < n_steps; ++i) {
        for (int64_t w = 0; w < W; ++w)
            hmc_begin(s, seed, step0 + i, w, cur.data() + w * P, cur_lnp[w], grad.data() + w * P, walker(w), table.data() + w * K);
        for (int leap = 1; leap <= s.n_leap; ++leap) {
            if (eval(table.data(), W, ll.data(), gcols.data()) != 0) return HMC_EVAL_FAILED;
            for (int64_t w = 0; w < W; ++w) {
                const HmcOutcome o = hmc_leap(s, seed, step0 + i, w, leap, ll[w], gcols.data() + w * K, 1, walker(w),
                                              cur.data() + w * P, &cur_lnp[w], grad.data() + w * P, table.data() + w * K);
                if (leap == s.n_leap) {
                    if (o.accepted) acc[w] += 1;
                    if (energy_error) energy_error[i * W + w] = o.energy_error;
                }
            }
        }
        if (chain) for (int64_t x = 0; x < W * P; ++x) chain[i * W * P + x] = cur[x];
        if (lnprob_chain) for (int64_t w = 0; w < W; ++w) lnprob_chain[i * W + w] = cur_lnp[w];
    }
    // (the caller's state is written last, with final values only)
    for (size_t x = 0; x < (size_t)W * P; ++x) pos[x] = cur[x];
    for (int64_t w = 0; w < W; ++w) lnp[w] = cur_lnp[w];
    if (accepted) for (int64_t w = 0; w < W; ++w) accepted[w] += acc[w];
    return HMC_OK;
}

// ---- device: the resident block (mcd_hmc.hip) ------------------------------------------------------------------------
// Everything the two kernels need, by value in their argument block; every pointer is device memory.
struct HmcDevice {
    HmcShared s;
    int64_t n_walkers = 0;
    uint64_t seed = 0;
    double* pos = nullptr;            // [W][P] current point, its log-likelihood [W] and free-parameter gradient [W][P]
    double* lnp = nullptr;
    double* grad = nullptr;
    long long* accepted = nullptr;    // [W]
    double* q = nullptr;              // trajectory state (HmcWalker): [W][P], [W][P], [W], [W], [W]
    double* p = nullptr;
    double* h0 = nullptr;
    double* eps = nullptr;
    int32_t* alive = nullptr;
    double* chain = nullptr;          // [n_steps][W][P], [n_steps][W], [n_steps][W]; each may be null
    double* lnprob_chain = nullptr;
    double* energy_error = nullptr;
    double* table = nullptr;          // [W][K] the work set's parameter table (prepare_walkers reads it)
    const double* fields = nullptr;   // [1 + K][padded] reduced value and column derivatives (mcd_grad.h)
    int64_t padded = 0;               // mcd_launch.h: padded_walkers(W)
};

#if defined(__HIPCC__)
// step: absolute step index (the generator's counter); row: index of the step inside the block (the chain rows' place)
hipError_t launch_hmc_begin(hipStream_t s, const HmcDevice& d, int64_t step);
hipError_t launch_hmc_leap(hipStream_t s, const HmcDevice& d, int64_t step, int64_t row, int leap);
#endif

}  // namespace mcd

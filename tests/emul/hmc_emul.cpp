// CPU build of the Hamiltonian Monte Carlo algebra (csrc/mcd_hmc.h) for the tests: the same text the device kernels
// (csrc/mcd_hmc.hip) and the library's host-driven block compile, with the value-and-gradient evaluation supplied by the
// test as a callback.  Loaded by tests/hmc_helper.py.
#include <cstdint>
#include <vector>

#include "mcd_hmc.h"

using namespace mcd;

typedef int (*hmc_eval_fn)(const double* table, int64_t n, double* out, double* grad);

static HmcShared shared_of(int P, int K, const int32_t* col_source, const double* col_const, const double* col_factor,
                           const double* lo, const double* hi, int fixed_ok, const double* chol, double step_size,
                           double jitter, int n_leap) {
    HmcShared s;
    s.n_dim = P; s.k = K; s.col_source = col_source; s.col_const = col_const; s.col_factor = col_factor; s.lo = lo; s.hi = hi;
    s.chol = chol; s.fixed_ok = fixed_ok; s.n_leap = n_leap; s.step_size = step_size; s.jitter = jitter;
    s.diagonal = hmc_is_diagonal(chol, P) ? 1 : 0;
    return s;
}

extern "C" void emul_hmc_numbers(uint64_t seed, int64_t step0, int64_t n_steps, int64_t W, int P, double* z, double* thr,
                                 double* r) {
    for (int64_t i = 0; i < n_steps; ++i)
        for (int64_t w = 0; w < W; ++w) {
            for (int c = 0; c < P; ++c) z[(i * W + w) * P + c] = hmc_normal(seed, step0 + i, w, c);
            hmc_aux(seed, step0 + i, w, thr[i * W + w], r[i * W + w]);
        }
}

// one normal with the number of generator calls it may use; *pairs: candidate pairs drawn
extern "C" double emul_hmc_normal(uint64_t seed, int64_t step, int64_t walker, int comp, int max_calls, int* pairs) {
    return hmc_normal(seed, step, walker, comp, max_calls, pairs);
}

extern "C" uint64_t emul_hmc_key() { return kHmcKey1; }
extern "C" uint64_t emul_hmc_aux_slot() { return kHmcAuxSlot; }
extern "C" int emul_hmc_normal_calls() { return kHmcNormalCalls; }

// n_leap leapfrog points from (q, p) with a fixed eps and the identity column map (K = P): half kick, { drift, gradient,
// kick } with a half kick last -- hmc_begin / hmc_leap without the draws and the accept.  Returns 1 when the trajectory
// stayed alive (inside the box, finite gradients).
extern "C" int emul_hmc_leapfrog(int P, const double* chol, const double* lo, const double* hi, double eps, int n_leap,
                                 double* q, double* p, hmc_eval_fn eval) {
    std::vector<int32_t> src(P);
    std::vector<double> one(P, 1.0), zero(P, 0.0), g(P);
    for (int c = 0; c < P; ++c) src[c] = c;
    const HmcShared s = shared_of(P, P, src.data(), zero.data(), one.data(), lo, hi, 1, chol, eps, 0.0, n_leap);
    double l;
    if (eval(q, 1, &l, g.data()) != 0) return -1;
    hmc_kick(s, 0.5 * eps, g.data(), p);
    for (int leap = 1; leap <= n_leap; ++leap) {
        if (!hmc_drift(s, eps, q, p)) return 0;
        if (eval(q, 1, &l, g.data()) != 0) return -1;
        for (int c = 0; c < P; ++c)
            if (!hmc_finite(g[c])) return 0;
        hmc_kick(s, leap < n_leap ? eps : 0.5 * eps, g.data(), p);
    }
    return 1;
}

extern "C" double emul_hmc_kinetic(int P, const double* chol, const double* p) {
    HmcShared s;
    s.n_dim = P; s.chol = chol;
    return hmc_kinetic(s, p);
}

extern "C" void emul_hmc_momentum(int P, const double* chol, const double* z, double* p) {
    HmcShared s;
    s.n_dim = P; s.chol = chol;
    hmc_momentum(s, z, p);
}

// the library's host-driven block (csrc/mcd_hmc.h: hmc_block); returns its HmcStatus
extern "C" int emul_hmc_block(int64_t W, int P, int K, const int32_t* col_source, const double* col_const,
                              const double* col_factor, const double* lo, const double* hi, int fixed_ok, const double* chol,
                              double step_size, double jitter, int n_leap, int64_t n_steps, double* pos, double* lnp,
                              uint64_t seed, int64_t step0, double* chain, double* lnprob_chain, int64_t* accepted,
                              double* energy_error, hmc_eval_fn eval) {
    const HmcShared s = shared_of(P, K, col_source, col_const, col_factor, lo, hi, fixed_ok, chol, step_size, jitter, n_leap);
    return hmc_block(s, W, n_steps, pos, lnp, seed, step0, chain, lnprob_chain, accepted, energy_error,
                     [&](const double* t, int64_t n, double* out, double* grad) { return eval(t, n, out, grad); });
}

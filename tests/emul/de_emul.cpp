// CPU build of the differential-evolution move (csrc/mcd_de.h) for the tests: the same text the device kernels
// (csrc/mcd_de.hip) and the library's host-driven block compile, with the log-likelihood supplied by the test as a
// callback.  Loaded by tests/de_helper.py.
#include <cstdint>
#include <vector>

#include "mcd_de.h"

using namespace mcd;

typedef int (*de_eval_fn)(const double* table, int64_t n, double* out);

extern "C" uint64_t emul_de_key() { return kDeKey1; }
extern "C" int emul_de_normal_calls() { return kDeNormalCalls; }
extern "C" double emul_de_det_log(double x) { return det_log(x); }

// the four raw words of generator call `call` of (step, h, b, j)
extern "C" void emul_de_words(uint64_t seed, int64_t step, int h, int64_t b, int64_t j, int call, uint64_t* out) {
    const Philox4x64 r = de_words(seed, step, h, b, j, call);
    for (int i = 0; i < 4; ++i) out[i] = r.v[i];
}

extern "C" double emul_de_normal(uint64_t seed, int64_t step, int h, int64_t b, int64_t j, int max_calls, int* pairs_used) {
    return de_normal(seed, step, h, b, j, max_calls, pairs_used);
}

// order [n][B][W], pick_a / pick_b / gamma / thr [n][2][B][W/2]
extern "C" void emul_de_numbers(uint64_t seed, int64_t step0, int64_t n_steps, int64_t B, int64_t W, double gamma0, double sigma,
                                int32_t* order, int32_t* pick_a, int32_t* pick_b, double* gamma, double* thr) {
    std::vector<uint64_t> sorter;
    for (int64_t i = 0; i < n_steps; ++i) {
        const int64_t at = i * B * W;                                   // (2 B W/2 per step)
        de_numbers_of_step(seed, step0 + i, B, W, gamma0, sigma, order + at, pick_a + at, pick_b + at, gamma + at, thr + at, sorter);
    }
}

// the stretch move's numbers of the same layout family (csrc/mcd_rng.h), for the test that the two streams differ
extern "C" void emul_de_stretch_numbers(uint64_t seed, int64_t step0, int64_t n_steps, int64_t B, int64_t W, int n_dim,
                                        int32_t* order, double* zz, double* thr, int32_t* pick) {
    std::vector<uint64_t> sorter;
    for (int64_t i = 0; i < n_steps; ++i) {
        const int64_t at = i * B * W;
        chain_numbers_of_step(seed, step0 + i, B, W, n_dim, order + at, zz + at, thr + at, pick + at, sorter);
    }
}

// the library's host-driven block (csrc/mcd_de.h: de_block); returns its StretchStatus (3 also for a refused prior)
extern "C" int emul_de_block(int64_t B, int64_t W, int P, int K, const int32_t* col_source, const double* col_const,
                             const double* col_factor, const double* lo, const double* hi, int fixed_ok,
                             const int32_t* prior_kind, const double* prior_p0, const double* prior_p1, int64_t n_steps,
                             double* pos, double* lnp, const int32_t* order, const int32_t* pick_a, const int32_t* pick_b,
                             const double* gamma, const double* thr, double* chain, double* lnprob_chain, int64_t* accepted,
                             de_eval_fn eval) {
    std::vector<double> loc(P), scale(P), c0(P);
    StretchDesc d;
    d.n_bins = B; d.n_walkers = W; d.n_dim = P; d.k = K; d.col_source = col_source; d.col_const = col_const;
    d.col_factor = col_factor; d.lo = lo; d.hi = hi; d.fixed_ok = fixed_ok;
    if (prior_kind) {
        bool structured = false;
        if (!prior_derive(P, prior_kind, prior_p0, prior_p1, loc.data(), scale.data(), c0.data(), &structured)) return STRETCH_BAD_ARGS;
        if (structured) { d.prior.kind = prior_kind; d.prior.loc = loc.data(); d.prior.scale = scale.data(); d.prior.c0 = c0.data(); }
    }
    return de_block(d, n_steps, pos, lnp, order, pick_a, pick_b, gamma, thr, chain, lnprob_chain, accepted,
                    [&](const double* t, int64_t n, double* out) { return eval(t, n, out); });
}

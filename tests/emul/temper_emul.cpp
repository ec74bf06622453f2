// CPU build of the parallel-tempering algebra (csrc/mcd_temper.h) for the tests: the same text the device kernels
// (csrc/mcd_temper.hip) and the library's host-driven block compile, with the log-likelihood supplied by the test as a
// callback -- and the seeded stretch move of csrc/mcd_stretch.h on the same callback, which a ladder of one rung must
// reproduce.  Loaded by tests/temper_helper.py.
#include <cstdint>
#include <vector>

#include "mcd_stretch.h"
#include "mcd_temper.h"

using namespace mcd;

typedef int (*temper_eval_fn)(const double* table, int64_t n, double* out);

// the structured priors of a call: (kind, p0, p1) or a null kind
struct Priors {
    std::vector<double> loc, scale, c0;
    PriorTable table;
    bool ok = true;
    Priors(int P, const int32_t* kind, const double* p0, const double* p1) : loc(P), scale(P), c0(P) {
        if (!kind) return;
        bool structured = false;
        ok = prior_derive(P, kind, p0, p1, loc.data(), scale.data(), c0.data(), &structured);
        if (ok && structured) { table.kind = kind; table.loc = loc.data(); table.scale = scale.data(); table.c0 = c0.data(); }
    }
};

extern "C" uint64_t emul_temper_key() { return kTemperKey1; }

// swap_thr [n_steps][T - 1][W]
extern "C" void emul_temper_numbers(uint64_t seed, int64_t step0, int64_t n_steps, int32_t T, int64_t W, double* swap_thr) {
    for (int64_t i = 0; i < n_steps; ++i)
        for (int64_t t = 0; t + 1 < T; ++t)
            for (int64_t w = 0; w < W; ++w) swap_thr[(i * (T - 1) + t) * W + w] = temper_swap_thr(seed, step0 + i, t, w);
}

// the library's host-driven block (csrc/mcd_temper.h: temper_block); returns its TemperStatus
extern "C" int emul_temper_block(int32_t T, int64_t W, int P, int K, const int32_t* col_source, const double* col_const,
                                 const double* col_factor, const double* lo, const double* hi, int fixed_ok,
                                 const double* betas, const int32_t* prior_kind, const double* prior_p0, const double* prior_p1,
                                 int64_t n_steps, double* pos, double* ll, double* lp, uint64_t seed, int64_t step0,
                                 int32_t n_chain_temps, double* chain, double* lnlike_chain, int64_t* accepted,
                                 int64_t* swap_proposed, int64_t* swap_accepted, temper_eval_fn eval) {
    Priors pr(P, prior_kind, prior_p0, prior_p1);
    if (!pr.ok) return TEMPER_BAD_ARGS;
    TemperShared s;
    s.n_dim = P; s.k = K; s.col_source = col_source; s.col_const = col_const; s.col_factor = col_factor; s.lo = lo; s.hi = hi;
    s.fixed_ok = fixed_ok; s.n_temps = T; s.n_walkers = W; s.betas = betas; s.prior = pr.table;
    return temper_block(s, n_steps, pos, ll, lp, seed, step0, n_chain_temps, chain, lnlike_chain, accepted, swap_proposed,
                        swap_accepted, [&](const double* t, int64_t n, double* out) { return eval(t, n, out); });
}

// the seeded stretch move of ONE ensemble: stretch_block (csrc/mcd_stretch.h) fed chain_numbers_of_step, one step at a time
// as the library's host-driven seeded block does; returns its StretchStatus
extern "C" int emul_stretch_seeded(int64_t W, int P, int K, const int32_t* col_source, const double* col_const,
                                   const double* col_factor, const double* lo, const double* hi, int fixed_ok, int64_t n_steps,
                                   double* pos, double* lnp, uint64_t seed, int64_t step0, double* chain, double* lnprob_chain,
                                   int64_t* accepted, temper_eval_fn eval) {
    StretchDesc d;
    d.n_bins = 1; d.n_walkers = W; d.n_dim = P; d.k = K; d.col_source = col_source; d.col_const = col_const;
    d.col_factor = col_factor; d.lo = lo; d.hi = hi; d.fixed_ok = fixed_ok;
    const int64_t half = W / 2;
    std::vector<int32_t> order((size_t)W), pick((size_t)(2 * half));
    std::vector<double> zz((size_t)(2 * half)), thr((size_t)(2 * half));
    std::vector<uint64_t> sorter;
    int rc = STRETCH_OK;
    for (int64_t i = 0; i < n_steps && rc == STRETCH_OK; ++i) {
        chain_numbers_of_step(seed, step0 + i, 1, W, P, order.data(), zz.data(), thr.data(), pick.data(), sorter);
        rc = stretch_block(d, 1, pos, lnp, order.data(), zz.data(), thr.data(), pick.data(), chain ? chain + i * W * P : nullptr,
                           lnprob_chain ? lnprob_chain + i * W : nullptr, accepted,
                           [&](const double* t, int64_t n, double* out) { return eval(t, n, out); });
    }
    return rc;
}

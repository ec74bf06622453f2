// CPU build of the structured priors (csrc/mcd_prior.h) and of the two host-driven blocks that carry them
// (csrc/mcd_stretch.h: stretch_block, csrc/mcd_hmc.h: hmc_block) for the tests: the same text the device kernels and the
// library's host code compile, with the likelihood supplied by the test as a callback.  Loaded by tests/prior_helper.py.
#include <cstdint>
#include <vector>

#include "mcd_hmc.h"
#include "mcd_prior.h"
#include "mcd_stretch.h"

using namespace mcd;

namespace {
// (kind, p0, p1) -> the derived table; kind == nullptr: no prior.  false: invalid parameters.
struct Derived {
    std::vector<double> loc, scale, c0;
    PriorTable table;
    bool set(int P, const int32_t* kind, const double* p0, const double* p1) {
        table = PriorTable();
        if (!kind) return true;
        loc.resize(P); scale.resize(P); c0.resize(P);
        bool structured = false;
        if (!prior_derive(P, kind, p0, p1, loc.data(), scale.data(), c0.data(), &structured)) return false;
        if (structured) { table.kind = kind; table.loc = loc.data(); table.scale = scale.data(); table.c0 = c0.data(); }
        return true;
    }
};
}  // namespace

// value [n] (-inf where a log-normal coordinate is <= 0), grad [n][P] or null; -1: invalid prior parameters
extern "C" int emul_prior_eval(int P, const int32_t* kind, const double* p0, const double* p1, int64_t n, const double* x,
                               double* value, double* grad) {
    Derived d;
    if (!d.set(P, kind, p0, p1)) return -1;
    for (int64_t r = 0; r < n; ++r) {
        const double* row = x + r * P;
        double* g = grad ? grad + r * P : nullptr;
        if (g) for (int c = 0; c < P; ++c) g[c] = 0.0;
        if (!d.table.any()) { value[r] = 0.0; continue; }
        if (!prior_row_inside(d.table, P, row)) { value[r] = -__builtin_huge_val(); continue; }
        value[r] = g ? prior_row_grad(d.table, P, row, g) : prior_row(d.table, P, row);
    }
    return 0;
}

typedef int (*stretch_eval_fn)(const double* table, int64_t n, double* out);
extern "C" int emul_prior_stretch_block(int64_t B, int64_t W, int P, int K, const int32_t* col_source, const double* col_const,
                                        const double* col_factor, const double* lo, const double* hi, int fixed_ok,
                                        const int32_t* kind, const double* p0, const double* p1, int64_t n_steps, double* pos,
                                        double* lnp, const int32_t* order, const double* zz, const double* thr,
                                        const int32_t* pick, double* chain, double* lnprob_chain, int64_t* accepted,
                                        stretch_eval_fn eval) {
    Derived pr;
    if (!pr.set(P, kind, p0, p1)) return -1;
    StretchDesc d;
    d.n_bins = B; d.n_walkers = W; d.n_dim = P; d.k = K; d.col_source = col_source; d.col_const = col_const; d.col_factor = col_factor;
    d.lo = lo; d.hi = hi; d.fixed_ok = fixed_ok; d.prior = pr.table;
    return stretch_block(d, n_steps, pos, lnp, order, zz, thr, pick, chain, lnprob_chain, accepted,
                         [&](const double* t, int64_t n, double* out) { return eval(t, n, out); });
}

typedef int (*hmc_eval_fn)(const double* table, int64_t n, double* out, double* grad);
extern "C" int emul_prior_hmc_block(int64_t W, int P, int K, const int32_t* col_source, const double* col_const,
                                    const double* col_factor, const double* lo, const double* hi, int fixed_ok,
                                    const int32_t* kind, const double* p0, const double* p1, const double* chol,
                                    double step_size, double jitter, int n_leap, int64_t n_steps, double* pos, double* lnp,
                                    uint64_t seed, int64_t step0, double* chain, double* lnprob_chain, int64_t* accepted,
                                    double* energy_error, hmc_eval_fn eval) {
    Derived pr;
    if (!pr.set(P, kind, p0, p1)) return -1;
    HmcShared s;
    s.n_dim = P; s.k = K; s.col_source = col_source; s.col_const = col_const; s.col_factor = col_factor; s.lo = lo; s.hi = hi;
    s.chol = chol; s.fixed_ok = fixed_ok; s.n_leap = n_leap; s.step_size = step_size; s.jitter = jitter;
    s.diagonal = hmc_is_diagonal(chol, P) ? 1 : 0;
    s.prior = pr.table;
    return hmc_block(s, W, n_steps, pos, lnp, seed, step0, chain, lnprob_chain, accepted, energy_error,
                     [&](const double* t, int64_t n, double* out, double* grad) { return eval(t, n, out, grad); });
}

// element by element: n independent one-coordinate priors (kind [n], p0 [n], p1 [n]) at x [n] -> value [n], dx [n]
extern "C" int emul_prior_terms(int64_t n, const int32_t* kind, const double* p0, const double* p1, const double* x,
                                double* value, double* dx) {
    for (int64_t i = 0; i < n; ++i) {
        double loc, scale, c0;
        bool structured = false;
        if (!prior_derive(1, kind + i, p0 + i, p1 + i, &loc, &scale, &c0, &structured) || !structured) return -1;
        value[i] = prior_term_grad(kind[i], loc, scale, c0, x[i], dx[i]);
    }
    return 0;
}

// TEST INFRASTRUCTURE ONLY -- compiles the per-star posterior summaries of mcd_pointwise_posterior (csrc/mcd_posterior.h
// on top of csrc/mcd_math.h) for the CPU: the same (star, sample) term, the same running state and the same slice-ordered
// merge as posterior_slice_kernel / posterior_merge_kernel (csrc/mcd_posterior.hip).  Never loaded by the product package.
#include <cstdint>
#include <vector>

#include "mcd_dispatch.h"
#include "mcd_posterior.h"

using namespace mcd;

namespace {

// One star: `term(s, x, p)` gives the term of sample s; the S samples are cut into slices of slice_len (the last may be
// shorter), each folded from the empty state, and the slices merged in order -- the device plan of one pass.
template <bool MEM, class Term>
void one_star(int64_t S, int64_t slice_len, const std::vector<double>& inv, Term term, double* o4) {
    PostAcc acc;
    int64_t na = 0;
    for (int64_t j0 = 0; j0 < S; j0 += slice_len) {
        const int64_t count = (S - j0) < slice_len ? (S - j0) : slice_len;
        PostAcc b;
        b.init();
        for (int64_t j = 0; j < count; ++j) {
            double x, p;
            term(j0 + j, x, p);
            b.add<MEM>(x, p, inv[j]);
        }
        if (na == 0) acc = b;
        else acc.merge<MEM>(b, (double)na, (double)count);
        na += count;
    }
    acc.finish((double)S, o4[0], o4[1], o4[2], o4[3]);
}

int64_t plan(int64_t n, int64_t S, int64_t n_slices, int64_t* slice_len) {
    if (n_slices <= 0) return posterior_slices(n, S, slice_len);
    *slice_len = (S + n_slices - 1) / n_slices;
    return (S + *slice_len - 1) / *slice_len;
}

std::vector<double> reciprocals(int64_t len) {
    std::vector<double> inv((size_t)len);
    for (int64_t j = 0; j < len; ++j) inv[j] = 1.0 / (double)(j + 1);
    return inv;
}

template <int MODEL, bool FREE, bool MEM>
void run(int64_t n, const double* recs, const double* wrows, int64_t S, int64_t n_slices, double* out) {
    constexpr int ND = record_doubles(MODEL, FREE);
    int64_t slice_len = 0;
    plan(n, S, n_slices, &slice_len);
    const std::vector<double> inv = reciprocals(slice_len);
    std::vector<WalkerConsts<double>> w((size_t)S);
    for (int64_t s = 0; s < S; ++s) w[s].load(wrows + s * KD);
    for (int64_t i = 0; i < n; ++i) {
        double o4[4];
        one_star<MEM>(S, slice_len, inv,
                      [&](int64_t s, double& x, double& p) { posterior_term<MODEL, FREE, MEM, double>(recs + i * ND, w[s], x, p); },
                      o4);
        for (int f = 0; f < 4; ++f) out[f * n + i] = o4[f];
    }
}

}  // namespace

// out[4][n] = lppd, lnl_var, pmem_mean, pmem_std; n_slices <= 0: the library's slice plan
extern "C" int emul_posterior(int model, int free_centre, int mem, int64_t n, const double* recs, const double* wrows,
                              int64_t S, int64_t n_slices, double* out) {
    return dispatch_any_model(model, free_centre != 0, [&](auto M, auto FREE) {
        constexpr int MODEL = decltype(M)::value;
        constexpr bool kFree = decltype(FREE)::value;
        if constexpr (bg_kind(MODEL) != BG_NONE) {
            if (mem) { run<MODEL, kFree, true>(n, recs, wrows, S, n_slices, out); return 0; }
        }
        if (mem) return -1;
        run<MODEL, kFree, false>(n, recs, wrows, S, n_slices, out);
        return 0;
    }, -1);
}

// The same reduction over given terms: x, p [n][S] -> out[4][n]
extern "C" int emul_posterior_terms(int64_t n, int64_t S, const double* x, const double* p, int64_t n_slices, double* out) {
    int64_t slice_len = 0;
    plan(n, S, n_slices, &slice_len);
    const std::vector<double> inv = reciprocals(slice_len);
    for (int64_t i = 0; i < n; ++i) {
        double o4[4];
        one_star<true>(S, slice_len, inv, [&](int64_t s, double& xs, double& ps) { xs = x[i * S + s]; ps = p[i * S + s]; }, o4);
        for (int f = 0; f < 4; ++f) out[f * n + i] = o4[f];
    }
    return 0;
}

extern "C" int64_t emul_posterior_plan(int64_t n, int64_t S, int64_t* slice_len) { return posterior_slices(n, S, slice_len); }

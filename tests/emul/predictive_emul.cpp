// TEST INFRASTRUCTURE ONLY -- compiles the per-star posterior predictive checks of mcd_posterior_predictive
// (csrc/mcd_predictive.h on top of csrc/mcd_math.h) for the CPU: the same (star, sample) term, the same running state and
// the same slice-ordered merge as predictive_slice_kernel / predictive_merge_kernel (csrc/mcd_predictive.hip).  Never
// loaded by the product package.
#include <cstdint>
#include <vector>

#include "mcd_dispatch.h"
#include "mcd_posterior.h"
#include "mcd_predictive.h"

using namespace mcd;

namespace {

int64_t plan(int64_t n, int64_t S, int64_t n_slices, int64_t* slice_len) {
    if (n_slices <= 0) return posterior_slices(n, S, slice_len);
    *slice_len = (S + n_slices - 1) / n_slices;
    return (S + *slice_len - 1) / *slice_len;
}

// records and derived sample rows arrive as doubles; T = float rounds both once, as the float32 catalogues hold them
template <int MODEL, bool FREE, bool MIX, class T>
void run(int64_t n, const double* recs, const double* wrows, int64_t S, int64_t n_slices, double* out) {
    constexpr int ND = record_doubles(MODEL, FREE);
    int64_t slice_len = 0;
    plan(n, S, n_slices, &slice_len);
    std::vector<double> inv((size_t)slice_len);
    for (int64_t j = 0; j < slice_len; ++j) inv[j] = 1.0 / (double)(j + 1);
    std::vector<WalkerConsts<T>> w((size_t)S);
    std::vector<T> row(KD);
    for (int64_t s = 0; s < S; ++s) {
        for (int c = 0; c < KD; ++c) row[c] = (T)wrows[s * KD + c];
        w[s].load(row.data());
    }
    std::vector<T> rec(ND);
    for (int64_t i = 0; i < n; ++i) {
        for (int c = 0; c < ND; ++c) rec[c] = (T)recs[i * ND + c];
        PredAcc acc;
        int64_t na = 0;
        for (int64_t j0 = 0; j0 < S; j0 += slice_len) {
            const int64_t count = (S - j0) < slice_len ? (S - j0) : slice_len;
            PredAcc b;
            b.init();
            for (int64_t j = 0; j < count; ++j) {
                PredTerm x;
                predictive_term<MODEL, FREE, MIX, T>(rec.data(), w[j0 + j], x);
                b.add<MIX>(x, inv[j]);
            }
            if (na == 0) acc = b;
            else acc.merge<MIX>(b, (double)na, (double)count);
            na += count;
        }
        acc.finish<MIX>((double)S, out + i, n);
    }
}

template <int MODEL, bool FREE, bool MIX>
void run_precision(int f32, int64_t n, const double* recs, const double* wrows, int64_t S, int64_t n_slices, double* out) {
    if (f32) run<MODEL, FREE, MIX, float>(n, recs, wrows, S, n_slices, out);
    else run<MODEL, FREE, MIX, double>(n, recs, wrows, S, n_slices, out);
}

}  // namespace

// out[9][n] in PredOut order (the ninth field, pit_mix, is written with mix only); n_slices <= 0: the library's slice plan
extern "C" int emul_predictive(int model, int free_centre, int mix, int f32, int64_t n, const double* recs,
                               const double* wrows, int64_t S, int64_t n_slices, double* out) {
    return dispatch_any_model(model, free_centre != 0, [&](auto M, auto FREE) {
        constexpr int MODEL = decltype(M)::value;
        constexpr bool kFree = decltype(FREE)::value;
        if constexpr (bg_kind(MODEL) == BG_GAUSS) {
            if (mix) { run_precision<MODEL, kFree, true>(f32, n, recs, wrows, S, n_slices, out); return 0; }
        }
        if (mix) return -1;
        run_precision<MODEL, kFree, false>(f32, n, recs, wrows, S, n_slices, out);
        return 0;
    }, -1);
}

// the erfc the header uses, and the tail / CDF pair formed from it
extern "C" void emul_normal_tail_cdf(int64_t n, const double* z, double* t, double* cdf) {
    for (int64_t i = 0; i < n; ++i) normal_tail_cdf(z[i], t[i], cdf[i]);
}

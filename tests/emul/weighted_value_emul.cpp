// TEST INFRASTRUCTURE ONLY -- compiles the weighted value loop of mcd_weighted_loglike (csrc/mcd_weighted_value.h on top of
// csrc/mcd_holdout.h and csrc/mcd_weights.h) and, for comparison, the unweighted loop of mcd_holdout_loglike
// (csrc/mcd_holdout.h: chunk_holdout) for the CPU, so that the expressions the gfx950 kernel executes can be checked
// against the 80-bit truth without a GPU.  Never loaded by the product package.
#include <cstdint>

#include "mcd_dispatch.h"
#include "mcd_weighted_value.h"

using namespace mcd;

namespace {

// out[r] = sum of w l: chunks of chunk_len stars are summed on their own and then added in chunk order (the device adds
// the chunks' sums with a fixed tree instead)
template <int MODEL, bool FREE, int SCHEME>
void run(int64_t n, const double* recs, const double* wpar, int64_t R, const int64_t* row_replicate, uint64_t seed,
         const double* weights_t, int64_t n_replicates, int64_t chunk_len, double* out) {
    constexpr int ND = record_doubles(MODEL, FREE);
    for (int64_t r = 0; r < R; ++r) {
        WalkerConsts<double> c;
        c.load(wpar + r * KD);
        WeightRow src;
        src.seed = seed;
        src.replicate = (uint64_t)row_replicate[r];
        if (SCHEME == kWeightExplicit) { src.col = weights_t + row_replicate[r]; src.stride = n_replicates; }
        double total = 0.0;
        for (int64_t s = 0; s < n; s += chunk_len) {
            const int count = (int)((n - s) < chunk_len ? (n - s) : chunk_len);
            total += chunk_weighted_value<MODEL, FREE, SCHEME>(recs + s * ND, s, count, c, src);
        }
        out[r] = total;
    }
}

// the same sum of chunk sums over the unweighted loop
template <int MODEL, bool FREE>
void run_plain(int64_t n, const double* recs, const double* wpar, int64_t R, int64_t chunk_len, double* out) {
    constexpr int ND = record_doubles(MODEL, FREE);
    for (int64_t r = 0; r < R; ++r) {
        WalkerConsts<double> c;
        c.load(wpar + r * KD);
        double total = 0.0;
        for (int64_t s = 0; s < n; s += chunk_len) {
            const int count = (int)((n - s) < chunk_len ? (n - s) : chunk_len);
            total += chunk_holdout<MODEL, FREE, double>(recs + s * ND, count, c);
        }
        out[r] = total;
    }
}

}  // namespace

extern "C" {

// weights_t: [n][n_replicates] (the transposed array the device reads) for scheme 2, else unused
int emul_weighted_value(int model, int free_centre, int scheme, int64_t n, const double* recs, const double* wpar, int64_t R,
                        const int64_t* row_replicate, uint64_t seed, const double* weights_t, int64_t n_replicates,
                        int64_t chunk_len, double* out) {
    return dispatch_any_model(model, free_centre != 0, [&](auto M, auto FREE) {
        constexpr int MODEL = decltype(M)::value;
        constexpr bool kFree = decltype(FREE)::value;
        if (scheme == kWeightExponential)
            run<MODEL, kFree, kWeightExponential>(n, recs, wpar, R, row_replicate, seed, weights_t, n_replicates, chunk_len, out);
        else if (scheme == kWeightPoisson)
            run<MODEL, kFree, kWeightPoisson>(n, recs, wpar, R, row_replicate, seed, weights_t, n_replicates, chunk_len, out);
        else if (scheme == kWeightExplicit)
            run<MODEL, kFree, kWeightExplicit>(n, recs, wpar, R, row_replicate, seed, weights_t, n_replicates, chunk_len, out);
        else
            return -1;
        return 0;
    }, -1);
}

int emul_plain_value(int model, int free_centre, int64_t n, const double* recs, const double* wpar, int64_t R, int64_t chunk_len,
                     double* out) {
    return dispatch_any_model(model, free_centre != 0, [&](auto M, auto FREE) {
        run_plain<decltype(M)::value, decltype(FREE)::value>(n, recs, wpar, R, chunk_len, out);
        return 0;
    }, -1);
}

}  // extern "C"

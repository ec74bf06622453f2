// TEST INFRASTRUCTURE ONLY -- compiles the weighted gradient loop of mcd_weighted_loglike_grad (csrc/mcd_weighted.h on top
// of csrc/mcd_grad.h) and the weight generator (csrc/mcd_weights.h on top of csrc/mcd_rng.h) for the CPU, so that the
// expressions the gfx950 kernel executes can be checked against the 80-bit truth without a GPU.  Never loaded by the
// product package.
#include <cstdint>

#include "mcd_dispatch.h"
#include "mcd_weighted.h"

using namespace mcd;

namespace {

// out[r][0] = sum of w l, out[r][1 + k] = sum of w dl/dtheta_k: chunks of chunk_len stars are summed on their own and then
// added in chunk order (the device adds the chunks' sums with a fixed tree instead)
template <int MODEL, bool FREE, int SCHEME>
void run(int64_t n, const double* recs, const double* wpar, const double* params, int64_t R, const int64_t* row_replicate,
         uint64_t seed, const double* weights_t, int64_t n_replicates, int64_t chunk_len, double* out) {
    constexpr int ND = record_doubles(MODEL, FREE);
    constexpr int K = grad_columns(MODEL, FREE);
    for (int64_t r = 0; r < R; ++r) {
        WalkerConsts<double> c;
        c.load(wpar + r * KD);
        GradRaw<double> q;
        q.load<MODEL, FREE>(params + r * K);
        WeightRow src;
        src.seed = seed;
        src.replicate = (uint64_t)row_replicate[r];
        if (SCHEME == kWeightExplicit) { src.col = weights_t + row_replicate[r]; src.stride = n_replicates; }
        double total[1 + K] = {};
        for (int64_t s = 0; s < n; s += chunk_len) {
            const int count = (int)((n - s) < chunk_len ? (n - s) : chunk_len);
            double acc[1 + K] = {};
            chunk_weighted<MODEL, FREE, SCHEME>(recs + s * ND, s, count, c, q, src, acc);
            for (int f = 0; f <= K; ++f) total[f] += acc[f];
        }
        for (int f = 0; f <= K; ++f) out[r * (1 + K) + f] = total[f];
    }
}

}  // namespace

extern "C" {

// weights_t: [n][n_replicates] (the transposed array the device reads) for scheme 2, else unused
int emul_weighted(int model, int free_centre, int scheme, int64_t n, const double* recs, const double* wpar,
                  const double* params, int64_t R, const int64_t* row_replicate, uint64_t seed, const double* weights_t,
                  int64_t n_replicates, int64_t chunk_len, double* out) {
    return dispatch_any_model(model, free_centre != 0, [&](auto M, auto FREE) {
        constexpr int MODEL = decltype(M)::value;
        constexpr bool kFree = decltype(FREE)::value;
        if (scheme == kWeightExponential)
            run<MODEL, kFree, kWeightExponential>(n, recs, wpar, params, R, row_replicate, seed, weights_t, n_replicates, chunk_len, out);
        else if (scheme == kWeightPoisson)
            run<MODEL, kFree, kWeightPoisson>(n, recs, wpar, params, R, row_replicate, seed, weights_t, n_replicates, chunk_len, out);
        else if (scheme == kWeightExplicit)
            run<MODEL, kFree, kWeightExplicit>(n, recs, wpar, params, R, row_replicate, seed, weights_t, n_replicates, chunk_len, out);
        else
            return -1;
        return 0;
    }, -1);
}

void emul_bootstrap_weights(int scheme, uint64_t seed, int64_t rep0, int64_t n_reps, int64_t star0, int64_t n_stars, double* w) {
    for (int64_t b = 0; b < n_reps; ++b)
        for (int64_t i = 0; i < n_stars; ++i) w[b * n_stars + i] = bootstrap_weight(scheme, seed, rep0 + b, star0 + i);
}

// the four words of the weight stream's call for (replicate, block of four stars)
void emul_weight_words(uint64_t seed, int64_t replicate, int64_t block, uint64_t* out) {
    const Philox4x64 r = weight_block(seed, (uint64_t)replicate, (uint64_t)block);
    for (int k = 0; k < 4; ++k) out[k] = r.v[k];
}

uint64_t emul_weight_key() { return kWeightKey1; }

int emul_poisson_thresholds(double* out) {
    int n = 0;
#define MCD_PUT(C) out[n++] = C;
    MCD_POISSON_CUMULATIVE(MCD_PUT)
#undef MCD_PUT
    return n;
}

double emul_weight_uniform(uint64_t word) { return weight_uniform(word); }

void emul_poisson_count(int64_t n, const double* u, double* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = poisson_count(u[i]);
}

}  // extern "C"

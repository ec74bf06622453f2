// TEST INFRASTRUCTURE ONLY -- compiles the velocity rule and the value loop of the simulated catalogues
// (csrc/mcd_simulated.h on top of csrc/mcd_holdout.h and csrc/mcd_replicate.h) and, for comparison, the loop of
// mcd_holdout_loglike on the observed velocities (csrc/mcd_holdout.h: chunk_holdout) for the CPU, so that the expressions
// the gfx950 kernels execute can be checked against the 80-bit truth without a GPU.  Never loaded by the product package.
#include <cstdint>

#include "mcd_dispatch.h"
#include "mcd_simulated.h"

using namespace mcd;

namespace {

// out[e][star]: the stars in chunks of chunk_len, each chunk walked as simulate_kernel walks it
template <int MODEL, bool FREE>
void run_simulate(int64_t n, const double* recs, const double* wpar, int64_t E, uint64_t seed, int64_t sim0, double bg_mean,
                  double bg_sigma2, int64_t chunk_len, double* out) {
    constexpr int ND = record_doubles(MODEL, FREE);
    for (int64_t e = 0; e < E; ++e) {
        WalkerConsts<double> c;
        c.load(wpar + e * KD);
        for (int64_t s = 0; s < n; s += chunk_len) {
            const int count = (int)((n - s) < chunk_len ? (n - s) : chunk_len);
            const double* r = recs + s * ND;
            for (int j = 0; j < count; ++j, r += ND)
                out[e * n + s + j] = simulated_velocity<MODEL, FREE>(r, c, seed, sim0 + e, s + j, bg_mean, bg_sigma2);
        }
    }
}

// out[r] = sum of the terms: chunks of chunk_len stars are summed on their own and then added in chunk order (the device
// adds the chunks' sums with a fixed tree instead)
template <int MODEL, bool FREE>
void run_value(int64_t n, const double* recs, const double* wpar, int64_t R, const int64_t* row_sim, const double* table,
               int64_t n_sims, double bg_mean, double bg_sigma2, int64_t chunk_len, double* out) {
    constexpr int ND = record_doubles(MODEL, FREE);
    for (int64_t r = 0; r < R; ++r) {
        WalkerConsts<double> c;
        c.load(wpar + r * KD);
        double total = 0.0;
        for (int64_t s = 0; s < n; s += chunk_len) {
            const int count = (int)((n - s) < chunk_len ? (n - s) : chunk_len);
            total += chunk_simulated_value<MODEL, FREE>(recs + s * ND, s, count, c, table + row_sim[r], n_sims, bg_mean, bg_sigma2);
        }
        out[r] = total;
    }
}

// the same sum of chunk sums over the loop on the observed velocities
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

int emul_simulate(int model, int free_centre, int64_t n, const double* recs, const double* wpar, int64_t E, uint64_t seed,
                  int64_t sim0, double bg_mean, double bg_sigma2, int64_t chunk_len, double* out) {
    return dispatch_any_model(model, free_centre != 0, [&](auto M, auto FREE) {
        run_simulate<decltype(M)::value, decltype(FREE)::value>(n, recs, wpar, E, seed, sim0, bg_mean, bg_sigma2, chunk_len, out);
        return 0;
    }, -1);
}

// table: [n][n_sims] (the transposed array the device reads)
int emul_simulated_value(int model, int free_centre, int64_t n, const double* recs, const double* wpar, int64_t R,
                         const int64_t* row_sim, const double* table, int64_t n_sims, double bg_mean, double bg_sigma2,
                         int64_t chunk_len, double* out) {
    return dispatch_any_model(model, free_centre != 0, [&](auto M, auto FREE) {
        run_value<decltype(M)::value, decltype(FREE)::value>(n, recs, wpar, R, row_sim, table, n_sims, bg_mean, bg_sigma2,
                                                             chunk_len, out);
        return 0;
    }, -1);
}

int emul_simulated_plain(int model, int free_centre, int64_t n, const double* recs, const double* wpar, int64_t R,
                         int64_t chunk_len, double* out) {
    return dispatch_any_model(model, free_centre != 0, [&](auto M, auto FREE) {
        run_plain<decltype(M)::value, decltype(FREE)::value>(n, recs, wpar, R, chunk_len, out);
        return 0;
    }, -1);
}

void emul_simulated_numbers(uint64_t seed, int64_t s0, int64_t S, int64_t i0, int64_t N, double* g, double* u) {
    for (int64_t s = 0; s < S; ++s)
        for (int64_t i = 0; i < N; ++i) {
            g[s * N + i] = rep_normal(seed, s0 + s, i0 + i);
            u[s * N + i] = rep_uniform(seed, s0 + s, i0 + i);
        }
}

int emul_simulated_budget(int64_t n_sims, int64_t n_stars) { return simulated_fits_budget(n_sims, n_stars) ? 1 : 0; }

}  // extern "C"

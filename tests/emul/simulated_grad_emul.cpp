// TEST INFRASTRUCTURE ONLY -- compiles the value-and-gradient loop of mcd_simulated_loglike_grad (csrc/mcd_simulated_grad.h
// on top of csrc/mcd_grad.h and csrc/mcd_simulated.h) and, for comparison, the plain gradient loop on the observed
// velocities (csrc/mcd_grad.h: chunk_grad) for the CPU, so that the expressions the gfx950 kernel executes can be checked
// against the 80-bit truth without a GPU.  Never loaded by the product package.
#include <cstdint>

#include "mcd_dispatch.h"
#include "mcd_simulated_grad.h"

using namespace mcd;

namespace {

// out[r][0] = sum of l, out[r][1 + k] = sum of dl/dtheta_k: chunks of chunk_len stars are summed on their own and then
// added in chunk order (the device adds the chunks' sums with a fixed tree instead).  table == nullptr: chunk_grad on the
// records' own velocities.
template <int MODEL, bool FREE>
void run(int64_t n, const double* recs, const double* wpar, const double* params, int64_t R, const int64_t* row_sim,
         const double* table, int64_t n_sims, double bg_mean, double bg_sigma2, int64_t chunk_len, double* out) {
    constexpr int ND = record_doubles(MODEL, FREE);
    constexpr int K = grad_columns(MODEL, FREE);
    for (int64_t r = 0; r < R; ++r) {
        WalkerConsts<double> c;
        c.load(wpar + r * KD);
        GradRaw<double> q;
        q.load<MODEL, FREE>(params + r * K);
        double total[1 + K] = {};
        for (int64_t s = 0; s < n; s += chunk_len) {
            const int count = (int)((n - s) < chunk_len ? (n - s) : chunk_len);
            double acc[1 + K] = {};
            if (table)
                chunk_simulated_grad<MODEL, FREE>(recs + s * ND, s, count, c, q, table + row_sim[r], n_sims, bg_mean, bg_sigma2, acc);
            else
                chunk_grad<MODEL, FREE, double>(recs + s * ND, count, c, q, acc);
            for (int f = 0; f <= K; ++f) total[f] += acc[f];
        }
        for (int f = 0; f <= K; ++f) out[r * (1 + K) + f] = total[f];
    }
}

}  // namespace

extern "C" {

int emul_simulated_grad_columns(int model, int free_centre) { return grad_columns(model, free_centre != 0); }

// table: [n][n_sims] (the transposed array the device reads), or null for the plain loop; out: [R][1 + K]
int emul_simulated_grad(int model, int free_centre, int64_t n, const double* recs, const double* wpar, const double* params,
                        int64_t R, const int64_t* row_sim, const double* table, int64_t n_sims, double bg_mean, double bg_sigma2,
                        int64_t chunk_len, double* out) {
    return dispatch_any_model(model, free_centre != 0, [&](auto M, auto FREE) {
        run<decltype(M)::value, decltype(FREE)::value>(n, recs, wpar, params, R, row_sim, table, n_sims, bg_mean, bg_sigma2,
                                                       chunk_len, out);
        return 0;
    }, -1);
}

}  // extern "C"

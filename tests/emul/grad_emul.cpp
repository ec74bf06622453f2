// TEST INFRASTRUCTURE ONLY -- compiles the gradient's per-term arithmetic (csrc/mcd_grad.h) for the CPU, so that the
// expressions the gfx950 kernel executes can be checked against the 80-bit truth without a GPU.  Never loaded by the
// product package.
#include <cstdint>

#include "mcd_dispatch.h"
#include "mcd_grad.h"

using namespace mcd;

// out[w][0] = sum of l, out[w][1 + k] = sum of dl/dtheta_k: chunks of chunk_len stars are summed on their own and then
// added in chunk order (the device adds the chunks' sums with a fixed tree instead)
template <int MODEL, bool FREE>
static void run(int64_t n, const double* recs, const double* wpar, const double* params, int64_t W, int64_t chunk_len,
                double* out) {
    constexpr int ND = record_doubles(MODEL, FREE);
    constexpr int K = grad_columns(MODEL, FREE);
    for (int64_t w = 0; w < W; ++w) {
        WalkerConsts<double> c;
        c.load(wpar + w * KD);
        GradRaw<double> q;
        q.load<MODEL, FREE>(params + w * K);
        double total[1 + K] = {};
        for (int64_t s = 0; s < n; s += chunk_len) {
            const int count = (int)((n - s) < chunk_len ? (n - s) : chunk_len);
            double acc[1 + K] = {};
            chunk_grad<MODEL, FREE, double>(recs + s * ND, count, c, q, acc);
            for (int f = 0; f <= K; ++f) total[f] += acc[f];
        }
        for (int f = 0; f <= K; ++f) out[w * (1 + K) + f] = total[f];
    }
}

extern "C" int emul_grad_columns(int model, int free_centre) { return grad_columns(model, free_centre != 0); }

extern "C" int emul_grad(int model, int free_centre, int64_t n, const double* recs, const double* wpar, const double* params,
                         int64_t W, int64_t chunk_len, double* out) {
    return dispatch_model(model, free_centre != 0, [&](auto M, auto FREE) {
        run<decltype(M)::value, decltype(FREE)::value>(n, recs, wpar, params, W, chunk_len, out);
        return 0;
    }, -1);
}

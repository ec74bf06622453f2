// TEST INFRASTRUCTURE ONLY -- the host build of the double Lynden-Bell models' per-term arithmetic: star_d_n in its plain
// and fast general forms (through chunk_loglike, csrc/mcd_math.h), the per-star components and grad_term
// (csrc/mcd_grad.h), for models 7 and 8 with a fixed and a free centre.  Never loaded by the product package.
#include <cstdint>

#include "mcd_dispatch.h"
#include "mcd_grad.h"
#include "mcd_guard.h"
#include "mcd_math.h"

using namespace mcd;

static const double kExpTabHost[kExpTabSize] = {MCD_EXP_TABLE_VALUES};

extern "C" int double_emul_kd() { return KD; }
extern "C" int double_emul_num_all_models() { return kNumAllModels; }
// M * 2 + FREE of the pair the launchers' dispatcher calls the functor with, or `fallback`; *calls counts the calls
extern "C" int double_emul_dispatch(int model, int free_centre, int fallback, int* calls) {
    return dispatch_any_model(model, free_centre != 0, [&](auto M, auto FREE) {
        ++*calls;
        return decltype(M)::value * 2 + (decltype(FREE)::value ? 1 : 0);
    }, fallback);
}
extern "C" int double_emul_columns(int model, int free_centre) { return grad_columns(model, free_centre != 0); }
extern "C" int double_emul_record_doubles(int model, int free_centre) { return record_doubles(model, free_centre != 0); }

// out[w] = log-likelihood of walker row w; fast: 0 the plain form, 1 the fast general form.  Chunks of chunk_len stars are
// summed on their own and added in chunk order.  Returns 1 when a fast chunk asked for the plain kernels (denormal regime).
extern "C" int double_emul_loglike(int model, int free_centre, int fast, int64_t n, const double* recs, const double* wpar,
                                   int64_t W, int64_t chunk_len, double* out) {
    if (!is_double(model)) return -1;
    return dispatch_any_model(model, free_centre != 0, [&](auto M, auto FREE) {
        constexpr int MODEL = decltype(M)::value;
        constexpr bool kFree = decltype(FREE)::value;
        constexpr int ND = record_doubles(MODEL, kFree);
        int rerun = 0;
        for (int64_t w = 0; w < W; ++w) {
            WalkerConsts<double> c;
            c.load(wpar + w * KD);
            double total = 0.0;
            for (int64_t s = 0; s < n; s += chunk_len) {
                const int count = (int)((n - s) < chunk_len ? (n - s) : chunk_len);
                bool denormal = false;
                if (fast) total += chunk_loglike<MODEL, kFree, double, double, 1>(recs + s * ND, count, c, denormal, kExpTabHost);
                else total += chunk_loglike<MODEL, kFree, double, double, 0>(recs + s * ND, count, c, denormal, kExpTabHost);
                if (denormal) rerun = 1;
            }
            out[w] = total;
        }
        return rerun;
    }, -1);
}

// d[i], nn[i] of every star for ONE walker row, plain (fast = 0) or fast general form
extern "C" int double_emul_d_n(int model, int free_centre, int fast, int64_t n, const double* recs, const double* wrow,
                               double* d, double* nn) {
    if (!is_double(model)) return -1;
    return dispatch_any_model(model, free_centre != 0, [&](auto M, auto FREE) {
        constexpr int MODEL = decltype(M)::value;
        constexpr bool kFree = decltype(FREE)::value;
        constexpr int ND = record_doubles(MODEL, kFree);
        WalkerConsts<double> c;
        c.load(wrow);
        for (int64_t i = 0; i < n; ++i) {
            if (fast) star_d_n<MODEL, double, kFree, true>(recs + i * ND, c, d[i], nn[i]);
            else star_d_n<MODEL, double, kFree, false>(recs + i * ND, c, d[i], nn[i]);
        }
        return 0;
    }, -1);
}

// per-star mixture log-likelihood (mode 1) or membership probability (mode 0) of model 8 for ONE walker row
extern "C" int double_emul_per_star(int model, int free_centre, int mode, int64_t n, const double* recs, const double* wrow,
                                    double* out) {
    if (model != MODEL_DOUBLE_BGGAUSS) return -1;
    return dispatch_any_model(model, free_centre != 0, [&](auto M, auto FREE) {
        constexpr int MODEL = decltype(M)::value;
        constexpr bool kFree = decltype(FREE)::value;
        constexpr int ND = record_doubles(MODEL, kFree);
        WalkerConsts<double> c;
        c.load(wrow);
        for (int64_t i = 0; i < n; ++i) {
            double lc, lb, m;
            star_components<MODEL, kFree, double>(recs + i * ND, c, lc, lb, m);
            if (mode == 1) { out[i] = mixture_lnl(lc, lb, m); continue; }
            const double shift = max_(lc, lb);
            const double ec = m * std::exp(lc - shift), eb = (1.0 - m) * std::exp(lb - shift);
            out[i] = ec / (ec + eb);
        }
        return 0;
    }, -1);
}

// out[w][0] = sum of l, out[w][1 + k] = sum of dl/dtheta_k (grad_emul.cpp's loop)
extern "C" int double_emul_grad(int model, int free_centre, int64_t n, const double* recs, const double* wpar,
                                const double* params, int64_t W, int64_t chunk_len, double* out) {
    if (!is_double(model)) return -1;
    return dispatch_any_model(model, free_centre != 0, [&](auto M, auto FREE) {
        constexpr int MODEL = decltype(M)::value;
        constexpr bool kFree = decltype(FREE)::value;
        constexpr int ND = record_doubles(MODEL, kFree);
        constexpr int K = grad_columns(MODEL, kFree);
        for (int64_t w = 0; w < W; ++w) {
            WalkerConsts<double> c;
            c.load(wpar + w * KD);
            GradRaw<double> q;
            q.template load<MODEL, kFree>(params + w * K);
            double total[1 + K] = {};
            for (int64_t s = 0; s < n; s += chunk_len) {
                const int count = (int)((n - s) < chunk_len ? (n - s) : chunk_len);
                double acc[1 + K] = {};
                chunk_grad<MODEL, kFree, double>(recs + s * ND, count, c, q, acc);
                for (int f = 0; f <= K; ++f) total[f] += acc[f];
            }
            for (int f = 0; f <= K; ++f) out[w * (1 + K) + f] = total[f];
        }
        return 0;
    }, -1);
}

// the library's launch level for a parameter table (csrc/mcd_guard.h: fast_level) with the statistics gathered as
// mcd_catalog_create gathers them for a float64 profile catalogue
extern "C" int double_emul_level(int model, int free_centre, int64_t n, const double* ra, const double* dec, const double* v,
                                 const double* verr, const double* density, double ra_c, double dec_c, int k,
                                 const double* params, int64_t n_rows) {
    const CatalogStats st = compute_stats(n, v, verr, nullptr, nullptr, density, bg_kind(model), ra, dec, free_centre == 0,
                                          ra_c, dec_c);
    return fast_level(st, model, free_centre != 0, false, k, params, n_rows);
}

// TEST INFRASTRUCTURE ONLY -- the verr-sorted record array and the series reciprocal root of the level-2 BGFIXED
// fixed-centre loops (csrc/mcd_math.h: RootSeries, chunk_bgfixed_fast; csrc/mcd_chunks.h: verr_order, permuted_exceptions,
// series_thresholds) compiled for the CPU, so that the series, the wave's vote, the sort and the plan on a sorted shard
// can be checked without a GPU (tests/root_series_helper.py).  Never loaded by the product package.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "mcd_chunks.h"
#include "mcd_guard.h"
#include "mcd_math.h"

using namespace mcd;

static const double kExpTabSqrt2Host[kExpTabSize] = {MCD_EXP_TABLE_SQRT2_VALUES};

// verr-sorted records and the series reciprocal root of the level-2 BGFIXED fixed-centre loops (csrc/mcd_math.h:
// RootSeries, csrc/mcd_chunks.h: verr_order, permuted_exceptions, series_thresholds).
// g[i] from the series about centre eb[i] for sigma^2 = s2[i] at verr^2 = e[i]; ok[i] the lane's verdict for a band of
// half-width half[i]; newton[i] = the form it replaces as the rsq loops form it, rsqrt2_newton(8 e + 8 s2), with the
// relative error seed_err[i] on its seed (the host build's seed is 1 / sqrt; v_rsq_f64 is off by up to 2^-24.2)
extern "C" void emul_series_root(int64_t n, const double* eb, const double* half, const double* s2, const double* e,
                                 double* g, uint8_t* ok, double* newton, const double* seed_err) {
    for (int64_t i = 0; i < n; ++i) {
        RootSeries sr;
        ok[i] = sr.setup(eb[i], half[i], s2[i]) ? 1 : 0;
        g[i] = sr.g(e[i]);
        const double m = fma_(8.0, e[i], 8.0 * s2[i]);
        const double y = (1.0 / std::sqrt(m)) * (1.0 + seed_err[i]);
        newton[i] = seed_err[i] == 0.0 ? rsqrt2_newton(m) : y * fma_(-m, y * y, 3.0);      // (rsqrt2_newton's two lines)
    }
}

// the wave's vote on a chunk whose verr^2 runs from e_first to e_last, for the lanes' sigma^2
extern "C" int emul_series_vote(double e_first, double e_last, int64_t n_lanes, const double* s2) {
    bool all = true;
    for (int64_t l = 0; l < n_lanes; ++l) {
        RootSeries sr;
        all = sr.setup_chunk(e_first, e_last, s2[l]) && all;
    }
    return wave_all(all) ? 1 : 0;
}

extern "C" void emul_verr_order(int64_t n, int nd, const double* recs, int64_t* perm) {
    const std::vector<int64_t> p = verr_order(recs, n, nd);
    for (int64_t i = 0; i < n; ++i) perm[i] = p[(size_t)i];
}

extern "C" int64_t emul_permuted_exceptions(int64_t n_exc, const int64_t* exc, int64_t n, const int64_t* perm,
                                            int64_t star_begin, int64_t* out) {
    const std::vector<int64_t> r = permuted_exceptions(std::vector<int64_t>(exc, exc + n_exc),
                                                       std::vector<int64_t>(perm, perm + n), star_begin);
    for (size_t i = 0; i < r.size(); ++i) out[i] = r[i];
    return (int64_t)r.size();
}

// The library's plan for a sorted shard of one parameter set and who takes the series at the table's smallest sigma^2:
// info = {chunks, chunks counted by the planning-time thresholds (mcd_last_series_chunks), chunks the kernel's own vote
// admits, stars in those chunks}
extern "C" void emul_series_plan(int64_t n, const double* sorted_e2, int64_t n_walkers, int64_t target_waves, int tail_split,
                                 int64_t n_exc, const int64_t* exc, int balance, double s2_min, int64_t* info) {
    const ChunkPlan plan = plan_chunks({0, n}, 0, n, n_walkers, target_waves, tail_split, std::vector<int64_t>(exc, exc + n_exc),
                                       0, balance);
    const std::vector<double> need = series_thresholds(plan, sorted_e2);
    info[0] = (int64_t)plan.chunks.size();
    info[1] = (int64_t)(std::upper_bound(need.begin(), need.end(), s2_min) - need.begin());
    info[2] = info[3] = 0;
    for (size_t c = 0; c < plan.chunks.size(); ++c) {
        const Chunk& ch = plan.chunks[c];
        if (ch.count <= 0 || (!plan.general.empty() && plan.general[c])) continue;
        RootSeries sr;
        if (sr.setup_chunk(sorted_e2[ch.begin], sorted_e2[ch.begin + ch.count - 1], s2_min)) { ++info[2]; info[3] += ch.count; }
    }
}

// Level-2 BGFIXED fixed-centre evaluation of (sorted) records in chunks of chunk_len, lanes voting in tiles of 64
// walkers as the kernel's waves do; series = 0: the rsq loops.  n_series: (chunk, tile) pairs that took the series.
extern "C" void emul_series_loglike(int64_t n, const double* recs, int64_t W, const double* wpar, int64_t chunk_len,
                                    int series, double* out, int64_t* n_series) {
    constexpr int M = MODEL_BGFIXED;
    constexpr int ND = record_doubles(M, false);
    *n_series = 0;
    for (int64_t w = 0; w < W; ++w) out[w] = 0.0;
    for (int64_t s = 0; s < n; s += chunk_len) {
        const int count = (int)((n - s) < chunk_len ? (n - s) : chunk_len);
        const double* r = recs + s * ND;
        for (int64_t t0 = 0; t0 < W; t0 += 64) {
            const int64_t t1 = std::min(W, t0 + 64);
            bool vote = series != 0;
            for (int64_t w = t0; w < t1 && vote; ++w) {
                RootSeries sr;
                vote = sr.setup_chunk(r[1], r[(int64_t)(count - 1) * ND + 1], wpar[w * KD + W_S2]);
            }
            if (vote) ++*n_series;
            for (int64_t w = t0; w < t1; ++w) {
                WalkerConsts<double> c;
                c.load(wpar + w * KD);
                bool den;
                out[w] += chunk_loglike<M, false, double, double, 2>(r, count, c, den, kExpTabSqrt2Host, 1, vote);
            }
        }
    }
    for (int64_t w = 0; w < W; ++w) {
        double sb = 0.0;
        for (int64_t i = 0; i < n; ++i) sb += recs[i * ND + geometry_doubles(M, false)];
        out[w] += sb;
    }
}

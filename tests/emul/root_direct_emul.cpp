// TEST INFRASTRUCTURE ONLY -- the direct form of the series reciprocal root of the level-2 BGFIXED fixed-centre loops
// (csrc/mcd_math.h: RootDirect, chunk_bgfixed_fast; csrc/mcd_chunks.h: direct_thresholds) compiled for the CPU, so that
// its accuracy, the wave's second vote and the plan's count can be checked without a GPU (tests/root_direct_helper.py).
// Never loaded by the product package.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "mcd_chunks.h"
#include "mcd_guard.h"
#include "mcd_math.h"

using namespace mcd;

static const double kExpTabSqrt2Host[kExpTabSize] = {MCD_EXP_TABLE_SQRT2_VALUES};

extern "C" double emul_direct_rho_max() { return RootDirect::kRhoMax; }
extern "C" double emul_direct_error_bound() { return RootDirect::kErrorBound; }

// g[i] from the direct form about centre eb[i] for sigma^2 = s2[i] at verr^2 = e[i]; ok[i] the lane's verdict on the
// direct form; delta[i] = RootSeries::g on the same inputs
extern "C" void emul_direct_root(int64_t n, const double* eb, const double* s2, const double* e, double* g, uint8_t* ok,
                                 double* delta) {
    for (int64_t i = 0; i < n; ++i) {
        RootDirect sd;
        sd.setup(eb[i], s2[i]);
        g[i] = sd.g_direct(e[i]);
        ok[i] = RootDirect::direct_ok(eb[i], s2[i]) ? 1 : 0;
        RootSeries sr;
        sr.setup(eb[i], 0.0, s2[i]);
        delta[i] = sr.g(e[i]);
    }
}

// the wave's two votes on a chunk whose verr^2 runs from e_first to e_last, for the lanes' sigma^2: 0 the rsq loops, 1 the
// delta series, 2 the direct series
extern "C" int emul_direct_vote(double e_first, double e_last, int64_t n_lanes, const double* s2) {
    bool series = true, direct = true;
    for (int64_t l = 0; l < n_lanes; ++l) {
        RootSeries sr;
        series = sr.setup_chunk(e_first, e_last, s2[l]) && series;
        direct = RootDirect::direct_ok(sr.eb, s2[l]) && direct;
    }
    return wave_all(series) ? (wave_all(direct) ? 2 : 1) : 0;
}

// The library's plan for a sorted shard of one parameter set and who takes the direct form at the table's smallest
// sigma^2: info = {chunks, chunks counted by the planning-time thresholds (mcd_last_direct_chunks), chunks the kernel's own
// votes admit, stars in those chunks, chunks counted for the series (mcd_last_series_chunks)}
extern "C" void emul_direct_plan(int64_t n, const double* sorted_e2, int64_t n_walkers, int64_t target_waves, int tail_split,
                                 int64_t n_exc, const int64_t* exc, int balance, double s2_min, int64_t* info) {
    const ChunkPlan plan = plan_chunks({0, n}, 0, n, n_walkers, target_waves, tail_split, std::vector<int64_t>(exc, exc + n_exc),
                                       0, balance);
    const std::vector<double> need = direct_thresholds(plan, sorted_e2);
    const std::vector<double> need_series = series_thresholds(plan, sorted_e2);
    info[0] = (int64_t)plan.chunks.size();
    info[1] = (int64_t)(std::upper_bound(need.begin(), need.end(), s2_min) - need.begin());
    info[4] = (int64_t)(std::upper_bound(need_series.begin(), need_series.end(), s2_min) - need_series.begin());
    info[2] = info[3] = 0;
    for (size_t c = 0; c < plan.chunks.size(); ++c) {
        const Chunk& ch = plan.chunks[c];
        if (ch.count <= 0 || (!plan.general.empty() && plan.general[c])) continue;
        if (emul_direct_vote(sorted_e2[ch.begin], sorted_e2[ch.begin + ch.count - 1], 1, &s2_min) == 2) { ++info[2]; info[3] += ch.count; }
    }
}

// Level-2 BGFIXED fixed-centre evaluation of (sorted) records in chunks of chunk_len, lanes voting in tiles of 64
// walkers as the kernel's waves do.  mode 0: the rsq loops; 1: the series, delta form only (option root_direct = 0);
// 2: the direct form where the second vote passes.  counts = {(chunk, tile) pairs in the delta form, ... in the direct form}
extern "C" void emul_direct_loglike(int64_t n, const double* recs, int64_t W, const double* wpar, int64_t chunk_len,
                                    int mode, double* out, int64_t* counts) {
    constexpr int M = MODEL_BGFIXED;
    constexpr int ND = record_doubles(M, false);
    counts[0] = counts[1] = 0;
    for (int64_t w = 0; w < W; ++w) out[w] = 0.0;
    std::vector<double> s2;
    for (int64_t s = 0; s < n; s += chunk_len) {
        const int count = (int)((n - s) < chunk_len ? (n - s) : chunk_len);
        const double* r = recs + s * ND;
        for (int64_t t0 = 0; t0 < W; t0 += 64) {
            const int64_t t1 = std::min(W, t0 + 64);
            s2.clear();
            for (int64_t w = t0; w < t1; ++w) s2.push_back(wpar[w * KD + W_S2]);
            int form = mode ? emul_direct_vote(r[1], r[(int64_t)(count - 1) * ND + 1], (int64_t)s2.size(), s2.data()) : 0;
            if (mode == 1 && form == 2) form = 1;
            if (form) ++counts[form - 1];
            for (int64_t w = t0; w < t1; ++w) {
                WalkerConsts<double> c;
                c.load(wpar + w * KD);
                bool den;
                // (the host build's wave_all passes the lane's own verdict on: the tile's votes go in as the two flags)
                out[w] += chunk_loglike<M, false, double, double, 2>(r, count, c, den, kExpTabSqrt2Host, 1, form >= 1, form == 2);
            }
        }
    }
    for (int64_t w = 0; w < W; ++w) {
        double sb = 0.0;
        for (int64_t i = 0; i < n; ++i) sb += recs[i * ND + geometry_doubles(M, false)];
        out[w] += sb;
    }
}

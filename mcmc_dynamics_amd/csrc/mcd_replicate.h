// mcd_replicate.h -- replicated-data predictive checks per group of stars (mcd_replicate_check; Gelman, Meng & Stern 1996):
// for every posterior sample s a replicated catalogue is drawn from the model at that sample, and eight additive fields of
// the standardised residuals are accumulated per (sample, range of stars), once for the observed and once for the
// replicated velocities.  Host+device text with no HIP types, so that tests/emul compiles the same expressions
// (DESIGN.md section 3.18).  The reference has nothing of the kind.
//
// For star i (index in the caller's star order) and sample row s, with d, n from star_d_n (plain form) and everything
// after that in float64:
//   sd = sqrt(n)          z_obs = d / sd
//   g  = rep_normal(seed, s, i)                            standard normal, hmc_normal's construction on its own stream
//   u  = rep_uniform(seed, s, i)                           models with a background: the replicate is a cluster star when
//                                                          u < m, m the model's own membership prior (star_components)
//   z_rep = g                                              cluster star (exactly)
//         = ((mu_b - v_i) + d + sqrt(verr_i^2 + sigma_b^2) g) / sd      background star: the replicated velocity
//                                                          mu_b + sqrt(..) g as a residual against the CLUSTER component
//   (mu_b, sigma_b^2): the sample's (v_back, sigma_back^2) for the Gaussian-background models, two scalars of the call
//   for the fixed-background ones.
// Fields (RepField), each for z_obs and z_rep: sum z, z^2, z^3, z^4, sum z sin(theta), sum z cos(theta), max |z|, the
// count of |z| > 3 (a double).  No guard path: a non-finite term makes that sample's fields for that range non-finite and
// touches nothing else.
// The stream is a function of (seed, s, i) alone: ranges, chunk plan, passes and launch shape never change a replicate.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "mcd_chunks.h"
#include "mcd_predictive.h"
#include "mcd_rng.h"

namespace mcd {

constexpr uint64_t kRepKey1 = 0x6d63645f726570ull;           // "mcd_rep": never the chains' streams (kChainKey1, kHmcKey1)
// as mcd_hmc.h: kHmcNormalCalls -- after 16 calls (32 pairs, probability 4.1e-22 per normal) the draw returns 0.0
constexpr int kRepNormalCalls = 16;
constexpr int kRepFields = 8;                                 // include/mcd.h: MCD_REP_FIELDS
constexpr int kRepLaneDoubles = 2 * kRepFields;               // observed, then replicated
constexpr int64_t kRepMaxRows = 65536;                        // sample rows of one pass
constexpr int64_t kRepScratchBytes = (int64_t)256 << 20;      // the [slot][16][rows] partials of one pass (DESIGN 3.16's budget)
constexpr int64_t kRepTargetWaves = 8192;                     // 8 waves on each of 1024 SIMDs

enum RepField : int { RP_S1 = 0, RP_S2 = 1, RP_S3 = 2, RP_S4 = 3, RP_SIN = 4, RP_COS = 5, RP_MAX = 6, RP_TAIL3 = 7 };

// Standard normal of (seed, sample row, star): Marsaglia's polar method on uniform53 pairs, det_log, IEEE sqrt and
// division; counter (s, i, 0, call), pairs 2 c and 2 c + 1 of call c.  `max_calls` is kRepNormalCalls everywhere but in
// the test that walks into the fallback; *pairs_used (may be null): pairs drawn.
MCD_HD double rep_normal(uint64_t seed, int64_t s, int64_t i, int max_calls = kRepNormalCalls, int* pairs_used = nullptr) {
    int used = 0;
    for (int c = 0; c < max_calls; ++c) {
        const Philox4x64 r = philox4x64_10((uint64_t)s, (uint64_t)i, 0, (uint64_t)c, seed, kRepKey1);
        for (int h = 0; h < 2; ++h) {
            const double u = 2.0 * uniform53(r.v[2 * h]) - 1.0, v = 2.0 * uniform53(r.v[2 * h + 1]) - 1.0;
            const double q = u * u + v * v;
            ++used;
            if (q > 0.0 && q < 1.0) {
                if (pairs_used) *pairs_used = used;
                return u * sqrt_(-2.0 * det_log(q) / q);
            }
        }
    }
    if (pairs_used) *pairs_used = used;
    return 0.0;                                                // documented fallback, see kRepNormalCalls
}

// The membership uniform of (seed, sample row, star): word 0 of the call with counter (s, i, 1, 0)
MCD_HD double rep_uniform(uint64_t seed, int64_t s, int64_t i) {
    return uniform53(philox4x64_10((uint64_t)s, (uint64_t)i, 1, 0, seed, kRepKey1).v[0]);
}

struct RepTerm { double z_obs, z_rep, c, s; };

// bg_mean, bg_sigma2: (mu_b, sigma_b^2) of the fixed-background models (unused by the others)
template <int MODEL, bool FREE>
MCD_HD void replicate_term(RecPtr<double> r, const WalkerConsts<double>& w, uint64_t seed, int64_t s, int64_t i,
                           double bg_mean, double bg_sigma2, RepTerm& x) {
    constexpr int BG = bg_kind(MODEL);
    constexpr int XB = geometry_doubles(MODEL, FREE);
    // the draw is finished before the term is formed: the divergent rejection loop holds no record value
    const double g = rep_normal(seed, s, i);
    double u = 0.0;
    if constexpr (BG != BG_NONE) u = rep_uniform(seed, s, i);
    double d, n;
    star_d_n<MODEL, double, FREE>(r, w, d, n);
    const double sd = sqrt_(n);
    x.z_obs = d / sd;
    star_unit<MODEL, FREE, double>(r, w, x.c, x.s);
    if constexpr (BG == BG_NONE) {
        x.z_rep = g;
    } else {
        double m, mu, s2;
        if constexpr (BG == BG_FIXED) {
            m = r[XB + 1]; mu = bg_mean; s2 = bg_sigma2;
        } else if constexpr (BG == BG_FIXED_DENSITY) {
            const double rho = r[XB + 2];
            m = rho / (rho + w.fb); mu = bg_mean; s2 = bg_sigma2;
        } else {
            const double rho = r[XB];
            m = rho / (rho + w.fb); mu = w.vb; s2 = w.sb2;
        }
        const double zb = ((mu - r[0]) + d + sqrt_(r[1] + s2) * g) / sd;
        x.z_rep = u < m ? g : zb;
    }
}

// max that keeps a NaN once it has one
MCD_HD double rep_max(double m, double a) { return (a > m || a != a) ? a : m; }

// The eight fields of one of the two residuals, over a run of stars
struct RepSums {
    double f[kRepFields];
    MCD_HD void init() { for (int k = 0; k < kRepFields; ++k) f[k] = 0.0; }
    MCD_HD void add(double z, double c, double s) {
        const double z2 = z * z, a = fabs_(z);
        f[RP_S1] += z;
        f[RP_S2] += z2;
        f[RP_S3] += z2 * z;
        f[RP_S4] += z2 * z2;
        f[RP_SIN] += z * s;
        f[RP_COS] += z * c;
        f[RP_MAX] = rep_max(f[RP_MAX], a);
        f[RP_TAIL3] += (a > 3.0 ? 1.0 : 0.0) + (z - z);          // z - z: +0.0, NaN for a non-finite z
    }
    // this <- this followed by b (a later slot of the same range)
    MCD_HD void merge(const RepSums& b) {
        for (int k = 0; k < kRepFields; ++k) f[k] = k == RP_MAX ? rep_max(f[k], b.f[k]) : f[k] + b.f[k];
    }
};

struct RepAcc {
    RepSums obs, rep;
    MCD_HD void init() { obs.init(); rep.init(); }
};

// The address space of the index array on the device: wave-uniform reads of it are scalar loads, as the records'
typedef const int64_t MCD_CONST_AS* RepOrderPtr;

// One chunk of `order` for one sample row: the stars order[0 .. count) in that order
template <int MODEL, bool FREE>
MCD_HD void chunk_replicate(RecPtr<double> recs, RepOrderPtr order, int count, const WalkerConsts<double>& w, uint64_t seed,
                            int64_t s, double bg_mean, double bg_sigma2, RepAcc& acc) {
    constexpr int ND = record_doubles(MODEL, FREE);
    acc.init();
    for (int j = 0; j < count; ++j) {
        const int64_t i = order[j];
        RepTerm x;
        replicate_term<MODEL, FREE>(recs + i * ND, w, seed, s, i, bg_mean, bg_sigma2, x);
        acc.obs.add(x.z_obs, x.c, x.s);
        acc.rep.add(x.z_rep, x.c, x.s);
    }
}

// ---- host: validation and the plan ------------------------------------------------------------------------------------
// What is wrong with (range_offsets, order), or null.  `seen`: scratch of n_stars bytes.
inline const char* replicate_groups_error(int64_t n_ranges, const int64_t* range_offsets, const int64_t* order,
                                          int64_t n_stars, std::vector<uint8_t>& seen) {
    if (n_ranges < 1) return "n_ranges must be >= 1";
    if (!range_offsets) return "range_offsets must not be NULL";
    if (range_offsets[0] != 0) return "range_offsets[0] must be 0";
    for (int64_t r = 0; r < n_ranges; ++r)
        if (range_offsets[r + 1] < range_offsets[r]) return "range_offsets must be non-decreasing";
    const int64_t n_used = range_offsets[n_ranges];
    if (n_used > n_stars) return "range_offsets[n_ranges] exceeds the catalogue's stars";
    if (n_used > 0 && !order) return "order must not be NULL";
    seen.assign((size_t)n_stars, 0);
    for (int64_t j = 0; j < n_used; ++j) {
        const int64_t i = order[j];
        if (i < 0 || i >= n_stars) return "order holds an index outside the catalogue";
        if (seen[(size_t)i]) return "order holds an index twice";
        seen[(size_t)i] = 1;
    }
    return nullptr;
}

// whether the model takes its background's (mean, sigma) from the call
MCD_HD constexpr bool replicate_needs_background(int model) {
    return bg_kind(model) == BG_FIXED || bg_kind(model) == BG_FIXED_DENSITY;
}

inline const char* replicate_background_error(int model, double bg_mean, double bg_sigma) {
    if (!replicate_needs_background(model)) return nullptr;
    if (!(bg_mean - bg_mean == 0.0) || !(bg_sigma - bg_sigma == 0.0) || !(bg_sigma >= 0.0))
        return "a fixed-background model needs a finite bg_mean and a finite bg_sigma >= 0";
    return nullptr;
}

// The pass length and the chunk table of a call, from (n_used, R, S) alone [and a forced nominal chunk length]:
//   * rows of a pass: min(S, kRepMaxRows), halved (to whole 64-row tiles) while even one chunk per range and one more
//     would not fit the partials' budget
//   * nominal chunk length: n_used x row tiles / kRepTargetWaves stars (several waves per SIMD), at least what keeps
//     n_used / len + R chunks x 16 x rows doubles within the budget; plan_chunks rounds it to a multiple of 32, >= 64
//   * plan_chunks on the ranges with equal chunks (no guided tail): no chunk straddles a range
struct ReplicatePlan {
    int64_t pass_rows = 0;
    ChunkPlan chunks;
};

inline ReplicatePlan replicate_plan(int64_t n_ranges, const int64_t* range_offsets, int64_t n_samples, int64_t forced_len = 0,
                                    int64_t scratch_bytes = kRepScratchBytes) {
    ReplicatePlan p;
    const int64_t n_used = range_offsets[n_ranges];
    int64_t rows = std::max<int64_t>(1, std::min(n_samples, kRepMaxRows));
    const int64_t lane_bytes = (int64_t)kRepLaneDoubles * (int64_t)sizeof(double);
    auto max_chunks = [&](int64_t r) { return scratch_bytes / (lane_bytes * r); };
    while (rows > 64 && max_chunks(rows) < 2 * n_ranges + 2) rows = std::max<int64_t>(64, rows / 2 / 64 * 64);
    p.pass_rows = rows;
    const int64_t n_wtiles = (rows + 63) / 64;
    int64_t len = forced_len;
    if (len <= 0) {
        len = (n_used * n_wtiles + kRepTargetWaves - 1) / kRepTargetWaves;
        // chunks <= n_used / len + 2 R (a short last chunk per range; rounding to 32 only lengthens)
        const int64_t room = std::max<int64_t>(1, max_chunks(rows) - 2 * n_ranges);
        len = std::max(len, (n_used + room - 1) / room);
        len = std::max<int64_t>(len, 64);
    }
    const std::vector<int64_t> ranges(range_offsets, range_offsets + n_ranges + 1);
    p.chunks = plan_chunks(ranges, 0, n_used, rows, kRepTargetWaves, 0, {}, len);
    return p;
}

#if defined(__HIPCC__)
// mcd_replicate.hip.  partials: [n_chunks][16][n_rows]; out: [n_rows][n_ranges][8][2]; row0: the generator's index of
// the pass's first row
struct LaunchShape;
hipError_t launch_replicate(hipStream_t s, const LaunchShape& shape, const void* records, const int64_t* order,
                            const Chunk* chunks, int64_t n_chunks, const void* wpar, int64_t n_rows, int64_t row0,
                            uint64_t seed, double bg_mean, double bg_sigma2, double* partials);
hipError_t launch_replicate_reduce(hipStream_t s, const double* partials, const int64_t* range_slot_offsets,
                                   int64_t n_ranges, int64_t n_rows, double* out);
#endif

}  // namespace mcd

// TEST INFRASTRUCTURE ONLY -- compiles the replicated-data predictive checks of mcd_replicate_check
// (csrc/mcd_replicate.h on top of csrc/mcd_predictive.h, csrc/mcd_rng.h and csrc/mcd_math.h) for the CPU: the same term,
// the same generator, the same validation and chunk plan, and the slot-ordered combine of replicate_reduce_kernel
// (csrc/mcd_replicate.hip).  Never loaded by the product package.
#include <cstdint>
#include <cstring>
#include <vector>

#include "mcd_dispatch.h"
#include "mcd_replicate.h"

using namespace mcd;

namespace {

template <int MODEL, bool FREE>
void run(const double* recs, const double* wrows, int64_t S, uint64_t seed, int64_t row0, int64_t R, const int64_t* offs,
         const int64_t* order, double bg_mean, double bg_sigma, int64_t forced_len, double* out) {
    const ReplicatePlan plan = replicate_plan(R, offs, S, forced_len);
    const double bg_sigma2 = bg_sigma * bg_sigma;
    for (int64_t s = 0; s < S; ++s) {
        WalkerConsts<double> w;
        w.load(wrows + s * KD);
        for (int64_t r = 0; r < R; ++r) {
            RepAcc total;
            total.init();
            for (int64_t c = plan.chunks.offsets[r]; c < plan.chunks.offsets[r + 1]; ++c) {
                const Chunk& ch = plan.chunks.chunks[(size_t)c];
                RepAcc acc;
                chunk_replicate<MODEL, FREE>(recs, order + ch.begin, ch.count, w, seed, row0 + s, bg_mean, bg_sigma2, acc);
                total.obs.merge(acc.obs);
                total.rep.merge(acc.rep);
            }
            double* o = out + (s * R + r) * kRepLaneDoubles;
            for (int k = 0; k < kRepFields; ++k) { o[2 * k] = total.obs.f[k]; o[2 * k + 1] = total.rep.f[k]; }
        }
    }
}

void put(const char* why, char* msg, int cap) {
    if (msg && cap > 0) { std::strncpy(msg, why, (size_t)cap - 1); msg[cap - 1] = 0; }
}

}  // namespace

extern "C" {

// out[S][R][8][2]; forced_len <= 0: the library's chunk length.  No validation here (emul_replicate_validate).
int emul_replicate(int model, int free_centre, const double* recs, const double* wrows, int64_t S, uint64_t seed,
                   int64_t row0, int64_t R, const int64_t* offs, const int64_t* order, double bg_mean, double bg_sigma,
                   int64_t forced_len, double* out) {
    return dispatch_any_model(model, free_centre != 0, [&](auto M, auto FREE) {
        run<decltype(M)::value, decltype(FREE)::value>(recs, wrows, S, seed, row0, R, offs, order, bg_mean, bg_sigma,
                                                       forced_len, out);
        return 0;
    }, -1);
}

// the host checks of mcd_replicate_check on (ranges, order, background): 0, or 1 and the message
int emul_replicate_validate(int model, int64_t R, const int64_t* offs, const int64_t* order, int64_t n_stars, double bg_mean,
                            double bg_sigma, char* msg, int cap) {
    std::vector<uint8_t> seen;
    const char* why = replicate_groups_error(R, offs, order, n_stars, seen);
    if (!why) why = replicate_background_error(model, bg_mean, bg_sigma);
    if (!why) return 0;
    put(why, msg, cap);
    return 1;
}

// info: pass rows, chunks, nominal length, largest chunk; begin / count / range: the table (cap entries; null: skipped)
int64_t emul_replicate_plan(int64_t R, const int64_t* offs, int64_t S, int64_t forced_len, int64_t scratch_bytes, int64_t cap,
                            int64_t* begin, int32_t* count, int32_t* range, int64_t* info) {
    const ReplicatePlan p = replicate_plan(R, offs, S, forced_len, scratch_bytes > 0 ? scratch_bytes : kRepScratchBytes);
    const int64_t nc = (int64_t)p.chunks.chunks.size();
    int64_t longest = 0;
    for (int64_t i = 0; i < nc; ++i) {
        const Chunk& ch = p.chunks.chunks[(size_t)i];
        longest = ch.count > longest ? ch.count : longest;
        if (begin && i < cap) { begin[i] = ch.begin; count[i] = ch.count; range[i] = ch.pset; }
    }
    info[0] = p.pass_rows; info[1] = nc; info[2] = p.chunks.len; info[3] = longest;
    return nc;
}

void emul_replicate_numbers(uint64_t seed, int64_t s0, int64_t S, int64_t i0, int64_t N, double* g, double* u) {
    for (int64_t s = 0; s < S; ++s)
        for (int64_t i = 0; i < N; ++i) {
            g[s * N + i] = rep_normal(seed, s0 + s, i0 + i);
            u[s * N + i] = rep_uniform(seed, s0 + s, i0 + i);
        }
}

double emul_rep_normal(uint64_t seed, int64_t s, int64_t i, int max_calls, int* pairs_used) {
    return rep_normal(seed, s, i, max_calls, pairs_used);
}

// the four words of the replicate stream's call with counter (s, i, slot, call)
void emul_rep_words(uint64_t seed, int64_t s, int64_t i, int64_t slot, int64_t call, uint64_t* out) {
    const Philox4x64 r = philox4x64_10((uint64_t)s, (uint64_t)i, (uint64_t)slot, (uint64_t)call, seed, kRepKey1);
    for (int k = 0; k < 4; ++k) out[k] = r.v[k];
}

uint64_t emul_rep_key() { return kRepKey1; }
int emul_rep_normal_calls() { return kRepNormalCalls; }
int64_t emul_rep_max_rows() { return kRepMaxRows; }
int64_t emul_rep_scratch_bytes() { return kRepScratchBytes; }

// (cos, sin) of star_unit for n records and one walker row
int emul_star_unit(int model, int free_centre, int64_t n, const double* recs, const double* wrow, double* c, double* s) {
    return dispatch_any_model(model, free_centre != 0, [&](auto M, auto FREE) {
        constexpr int MODEL = decltype(M)::value;
        constexpr bool kFree = decltype(FREE)::value;
        constexpr int ND = record_doubles(MODEL, kFree);
        WalkerConsts<double> w;
        w.load(wrow);
        for (int64_t i = 0; i < n; ++i) star_unit<MODEL, kFree, double>(recs + i * ND, w, c[i], s[i]);
        return 0;
    }, -1);
}

}  // extern "C"

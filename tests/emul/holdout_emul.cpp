// Host build of the hold-out rules (csrc/mcd_holdout.h) and of the chunk plan the library makes for them
// (csrc/mcd_chunks.h: plan_chunks on the range offsets, with the catalogue's default options).  Test infrastructure only.
#include <cstdint>
#include <cstring>
#include <vector>

#include "mcd_chunks.h"
#include "mcd_holdout.h"

using namespace mcd;

extern "C" {

// 0 when the offsets are valid; else 1 and the message in msg (cap bytes)
int emul_holdout_offsets_error(int64_t n_sets, const int64_t* offs, int64_t n_stars, char* msg, int cap) {
    const char* why = holdout_offsets_error(n_sets, offs, n_stars);
    if (!why) return 0;
    if (msg && cap > 0) { std::strncpy(msg, why, (size_t)cap - 1); msg[cap - 1] = 0; }
    return 1;
}

// out: [n_sets + 2]; returns the number of ranges
int64_t emul_holdout_ranges(int64_t n_sets, const int64_t* offs, int64_t n_stars, int64_t* out) {
    const std::vector<int64_t> r = holdout_ranges(n_sets, offs, n_stars);
    for (size_t i = 0; i < r.size(); ++i) out[i] = r[i];
    return (int64_t)r.size() - 1;
}

// m [n_ranges][n_rows], rows e W + w -> train, test [n_rows]
void emul_holdout_combine(const double* m, int64_t n_ranges, int64_t n_rows, int64_t n_walkers, double* train, double* test) {
    for (int64_t row = 0; row < n_rows; ++row) holdout_combine(m, n_ranges, n_rows, row, row / n_walkers, train[row], test[row]);
}

// the plan of mcd_holdout_loglike for (offs, n_rows) with the library's default options; returns the number of chunks
// (or minus it when cap is too small); offsets: [n_ranges + 1]; info: max chunks per range, nominal length
int64_t emul_holdout_plan(int64_t n_sets, const int64_t* offs, int64_t n_stars, int64_t n_rows, int64_t cap, int64_t* begin,
                          int32_t* count, int32_t* range, int64_t* offsets, int64_t* info) {
    const std::vector<int64_t> r = holdout_ranges(n_sets, offs, n_stars);
    const ChunkPlan plan = plan_chunks(r, 0, n_stars, n_rows, 10240, 1, {}, 0);
    const int64_t nc = (int64_t)plan.chunks.size();
    if (nc > cap) return -nc;
    for (int64_t i = 0; i < nc; ++i) { begin[i] = plan.chunks[i].begin; count[i] = plan.chunks[i].count; range[i] = plan.chunks[i].pset; }
    for (size_t i = 0; i < plan.offsets.size(); ++i) offsets[i] = plan.offsets[i];
    info[0] = plan.max_chunks_per_pset;
    info[1] = plan.len;
    return nc;
}

int64_t emul_holdout_max_rows() { return kHoldoutMaxRows; }
int64_t emul_holdout_scratch_bytes() { return kHoldoutScratchBytes; }

}  // extern "C"

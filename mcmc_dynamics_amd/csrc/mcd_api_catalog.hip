// mcd_api_catalog.hip -- C-ABI of the MI355X log-likelihood library (see include/mcd.h; mcd_host.h lists the host units):
// one-off upload and packing of the star catalogue into HBM, star sharding across devices, the per-walker-count work
// sets with their chunk tables, the main kernel's launch shape, catalogue options and the queries about the last call.
#include "mcd_host.h"

using namespace mcd::host;

namespace {

int param_count(int model, bool free_centre) {
    int k = mcd::cluster_columns(model) + (free_centre ? 2 : 0);
    const int bg = mcd::bg_kind(model);
    if (bg == mcd::BG_GAUSS) k += 3;
    if (bg == mcd::BG_FIXED_DENSITY) k += 1;
    return k;
}

void free_workset(WorkSet& w) {
    if (w.d_chunks) (void)hipFree(w.d_chunks);
    if (w.d_offsets) (void)hipFree(w.d_offsets);
    if (w.d_chunk_general) (void)hipFree(w.d_chunk_general);
    if (w.d_split_const) (void)hipFree(w.d_split_const);
    if (w.d_params) (void)hipFree(w.d_params);
    if (w.d_wpar) (void)hipFree(w.d_wpar);
    if (w.d_partials) (void)hipFree(w.d_partials);
    if (w.d_out) (void)hipFree(w.d_out);
    if (w.d_out2) (void)hipFree(w.d_out2);
    if (w.d_partials2) (void)hipFree(w.d_partials2);
    if (w.d_grad_partials) (void)hipFree(w.d_grad_partials);
    if (w.d_grad_out) (void)hipFree(w.d_grad_out);
    if (w.h_grad_out) (void)hipHostFree(w.h_grad_out);
    if (w.ev_staged) (void)hipEventDestroy(w.ev_staged);
    for (int b = 0; b < 2; ++b) {
        if (w.ev_reduced[b]) (void)hipEventDestroy(w.ev_reduced[b]);
        if (w.ev_comm[b]) (void)hipEventDestroy(w.ev_comm[b]);
    }
    if (w.h_params) (void)hipHostFree(w.h_params);
    if (w.h_out) (void)hipHostFree(w.h_out);
    w = WorkSet();
}

// Which catalogues get ONE round of equal waves (mcd_chunks.h: balanced plans) and with how many workgroups per CU.
// Measured on MI355X (tools/balance_sweep.py, us per pipelined step = main kernel + reduction; multi-round schedule /
// best balanced plan): CONST x 256 walkers 1e4 stars 7.9 / 6.7, 3e4 9.7 / 8.8, 1e5 19.2 / 13.3, 2e5 27.4 / 20.3, 4e5
// 40.7 / 33.3, 8e5 67.0 / 63.3, 1.25e6 94.2 / 95.2;  BGFIXED x 256: 1e4 18.1 / 9.1, 1e5 38.1 / 28.5, 4e5 94.0 / 89.7,
// 6e5 129.5 / 130.7, 1e6 202 / 213;  BGGAUSS 1e5 x 256 58.1 / 46.4;  x 128 walkers: CONST 1e5 15.4 / 9.7, BGFIXED 27.5 /
// 18.0.  Small catalogues gain because every CU gets the same number of workgroups (1042 workgroups land as 4 or 5 per
// CU, and the launch waits for the CUs with 5) and because the workgroups add up their chunks' sums themselves; beyond
// ~0.9e6 (CONST) .. 1.3e6 (mixtures) CONST-equivalent stars per 256 walkers the dynamic balancing of 1.5 rounds with a
// guided tail wins.
// "work" = stars x (walker tiles / 4) x (instructions per term / those of CONST): the thresholds are in CONST stars.
double model_cost(int model, bool free_centre) {
    // fast f64 loops, DESIGN 3.3 (the double models: their profile counterparts plus the second component)
    // (the error-scale models: their base models' loops with one operand more)
    static const double kCost[mcd::kNumLaunchModels] = {8.5, 24.0, 45.0, 25.0, 60.0, 40.0, 42.0, 33.0, 68.0, 0.0 /* unassigned */, 8.5, 25.0};
    return (kCost[model] + (free_centre ? 7.0 : 0.0)) / 8.5;
}
int balance_auto_m(const mcd_catalog* cat, int64_t n, int64_t n_walkers) {
    const int64_t n_wtiles = (n_walkers + 63) / 64;
    const double tiles = n_wtiles <= 4 ? (double)n_wtiles : 4.0 * (double)((n_wtiles + 3) / 4);
    const double work = (double)n * tiles / 4.0 * model_cost(cat->model, cat->free_centre);
    // crossover to the multi-round schedules: CONST 1e6 x 256 is 76.4 us multi-round against 78.6 balanced (8e5: 67.0 / 63.3);
    // the mixtures keep winning a little longer per unit of work (BGFIXED 4e5 stars = 1.1e6 units: 94.0 / 89.7; 6e5: tie)
    const double limit = mcd::bg_kind(cat->model) == mcd::BG_NONE ? 9.0e5 : 1.3e6;
    if (cat->n_psets != 1 || work > limit) return 0;
    return work < 6.0e4 ? 2 : (work <= 3.4e5 ? 4 : 8);
}

// Which launches use the prefetching instantiation of the main kernel (mcd_math.h: RecordPrefetch; option "prefetch").
// Measured per shape with the prefetch compiled in and out (1x MI355X, us per step, in / out):
//   mixtures   C3 bgfixed 1e6 x 256: 201 / 217    x 128: 107 / 117    x 64: 62 / 90    bggauss 1e6 x 256: 370 / 381
//   CONST      1e6 x 256: 77.0 / 76.4   x 512: 148 / 144   x 128: 46.4 / 46.9   C5 (55 bins x 512): 173 / 164
//              C5 x 256: 94 / 90        C4 1e7 x 256: 694 / 711                  C2 1e5 x 256: 17.0 / 16.1
// The mixture loops wait for their records (4 stars per iteration, a third of the instructions are one dependent chain);
// the fraction tree of the no-background models reads 16 stars per iteration and hides the latency by itself, so the
// prefetch only pays there when the catalogue is far beyond every cache (C4).
bool wants_prefetch(const mcd_catalog* cat, const Shard& sh) {
    if (cat->prefetch >= 0) return cat->prefetch != 0;
    const size_t bytes = (size_t)sh.n * (size_t)mcd::record_bytes(cat->model, cat->free_centre, cat->precision);
    if (mcd::bg_kind(cat->model) == mcd::BG_NONE) return cat->n_psets == 1 && bytes >= ((size_t)128 << 20);
    return bytes >= ((size_t)8 << 20);
}

// Which shards the main kernel reads in verr order (option "verr_sorted").  By record volume alone -- the
// threshold from which the prefetching instantiation is chosen by default -- and not by the "prefetch" option, so that
// results do not depend on that option; smaller catalogues keep catalogue order and the bits they had.
bool wants_sorted(const mcd_catalog* cat, const Shard& sh) {
    if (cat->model != mcd::MODEL_BGFIXED || cat->free_centre || cat->precision != MCD_F64 || cat->n_psets != 1 || sh.n <= 0)
        return false;
    if (cat->verr_sorted >= 0) return cat->verr_sorted != 0;
    // an explicit "chunk_len" pins which catalogue stars form a chunk (and keeps a parameter set of a binned catalogue
    // bit for bit equal to a stand-alone catalogue of its stars): the order is then the caller's, unless forced
    if (cat->chunk_len > 0) return false;
    return (size_t)sh.n * (size_t)mcd::record_bytes(cat->model, cat->free_centre, cat->precision) >= ((size_t)8 << 20);
}

// The shard's records ordered by verr^2 ascending (ties in catalogue order: a fixed permutation), made once from the
// packed records: one round trip through host memory at the first plan that wants them.
int ensure_sorted_records(mcd_catalog* cat, Shard& sh) {
    if (sh.records_sorted) return MCD_OK;
    const DeviceSlot& slot = cat->ctx->slots[sh.slot];
    constexpr int ND = mcd::record_doubles(mcd::MODEL_BGFIXED, false);
    const size_t n = (size_t)sh.n, bytes = n * ND * sizeof(double);
    MCD_HIP(hipStreamSynchronize(slot.stream));
    std::vector<double> rec(n * ND), out(n * ND);
    MCD_HIP(hipMemcpy(rec.data(), sh.records, bytes, hipMemcpyDeviceToHost));
    const std::vector<int64_t> perm = mcd::verr_order(rec.data(), (int64_t)n, ND);
    sh.sorted_e2.resize(n);
    for (size_t i = 0; i < n; ++i) {
        std::memcpy(&out[i * ND], &rec[(size_t)perm[i] * ND], ND * sizeof(double));
        sh.sorted_e2[i] = out[i * ND + 1];
    }
    sh.sorted_exceptions = mcd::permuted_exceptions(cat->stats.narrow_exceptions, perm, sh.star_begin);
    // ... and the same stars with the split exponent offset (rec is free again: it takes them)
    sh.sorted_nbf.resize(n);
    mcd::exp_split_records(out.data(), (int64_t)n, rec.data(), sh.sorted_nbf.data());
    void* d[2] = {nullptr, nullptr};
    const double* src[2] = {out.data(), rec.data()};
    for (int a = 0; a < 2; ++a) {
        hipError_t e = hipMalloc(&d[a], bytes + 2048);          // (the slack of `records`)
        if (e == hipSuccess) e = hipMemset(d[a], 0, bytes + 2048);
        if (e == hipSuccess) e = hipMemcpy(d[a], src[a], bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            for (int b = 0; b <= a; ++b)
                if (d[b]) (void)hipFree(d[b]);
            MCD_HIP(e);
        }
    }
    sh.records_sorted = d[0];
    sh.records_split = d[1];
    return MCD_OK;
}

// The catalogue options other than the timing ones.  mcd_set_option refuses a value outside min .. max (or one that
// `accepts` turns down) with `message`, waits for whatever is in flight where `sync` is set, stores the value, and where
// `replan` is set (the chunk tables depend on the option) drops the work sets, which are rebuilt lazily.
struct Option {
    const char* key;
    int64_t min, max;
    const char* message;
    bool sync, replan;
    void (*set)(mcd_catalog* c, int64_t v);
    bool (*accepts)(int64_t v) = nullptr;
};
constexpr int64_t kMin = std::numeric_limits<int64_t>::min(), kMax = std::numeric_limits<int64_t>::max();   // no bound
#define MCD_SET(statement) [](mcd_catalog* c, int64_t v) { statement; }
const Option kOptions[] = {
    {"fast_path", 0, 2, "fast_path: 0 (plain), 1 (guarded, default) or 2 (guarded, no narrow variant)", false, false, MCD_SET(c->allow_fast = (int)v)},
    {"zero_copy", kMin, kMax, nullptr, false, false, MCD_SET(c->zero_copy = v != 0)},
    {"device_chain", 0, 2, "device_chain: 0 (host-driven blocks), 1 (default) or 2 (as 1 with the general step kernel, testing aid)", false, false,
     MCD_SET(c->device_chain = (int)v; c->chain_backoff = 0; c->chain_consecutive = 0; c->chain_hint = -1)},
    {"fused_reduce", kMin, kMax, nullptr, false, false, MCD_SET(c->fused_reduce = v != 0)},
    {"defer_guard", kMin, kMax, nullptr, false, false, MCD_SET(c->defer_guard = v != 0)},
    {"f32_domain", kMin, kMax, nullptr, false, false, MCD_SET(c->f32_domain = v != 0)},
    {"loo_scratch_mb", 1, kMax, "loo_scratch_mb must be >= 1", false, false, MCD_SET(c->loo_scratch_mb = v)},
    {"posterior_pass", 1, kMax, "posterior_pass must be >= 1", false, false, MCD_SET(c->posterior_pass = v)},
    {"replicate_row0", 0, kMax, "replicate_row0 must be >= 0", false, false, MCD_SET(c->replicate_row0 = v)},
    {"two_lanes", kMin, kMax, nullptr, true, false, MCD_SET(c->two_lanes = v != 0)},
    {"narrow_bounded", 0, 1, "narrow_bounded: 1 (where the guard admits it, default) or 0 (never)", false, false, MCD_SET(c->narrow_bounded = (int)v)},
    {"verr_sorted", -1, 1, "verr_sorted: -1 (by record volume, default), 0 (catalogue order) or 1 (sorted by verr)", true, true, MCD_SET(c->verr_sorted = (int)v)},
    {"root_series", 0, 1, "root_series: 1 (series root on the narrow chunks of verr-sorted records, default) or 0 (never)", false, false, MCD_SET(c->root_series = (int)v)},
    {"exp_split", 0, 1, "exp_split: 1 (split exponent offset in the direct chunks where the guard admits it, default) or 0 (never)", false, false, MCD_SET(c->exp_split = (int)v)},
    {"root_quad", 0, 1, "root_quad: 1 (quadratic series root on 32-star bands where a direct chunk admits it, default) or 0 (never)", false, false, MCD_SET(c->root_quad = (int)v)},
    {"block_step", 0, 1, "block_step: 1 (one block step per 32-star band in the bounded quadratic loop where the guard admits it, default) or 0 (never)", false, false, MCD_SET(c->block_step = (int)v)},
    {"root_direct", 0, 1, "root_direct: 1 (direct form of the series root where a chunk admits it, default) or 0 (delta form only)", false, false, MCD_SET(c->root_direct = (int)v)},
    {"prefetch", -1, 1, "prefetch: -1 (by record volume, default), 0 (off) or 1 (on)", false, false, MCD_SET(c->prefetch = (int)v)},
    {"spin_us", 0, kMax, "spin_us must be >= 0", false, false, MCD_SET(c->spin_us = v)},
    {"tail_split", kMin, kMax, nullptr, true, true, MCD_SET(c->tail_split = (int)v)},
    {"target_waves", 1, kMax, "target_waves must be positive", true, true, MCD_SET(c->target_waves = v)},
    {"chunk_len", 0, kMax, "chunk_len must be >= 0", true, true, MCD_SET(c->chunk_len = v)},
    {"balance", -1, 8, "balance: -1 (auto), 0 (off) or 1 .. 8 workgroups per CU", true, true, MCD_SET(c->balance = (int)v)},
    {"combine", 0, 16, "combine: 0 (never), 1 (largest workgroup the plan allows), 8 or 16 (waves per workgroup at most)", true, true,
     MCD_SET(c->combine = (int)v), [](int64_t v) { return v <= 1 || v == 8 || v == 16; }},
};
#undef MCD_SET
}  // namespace

MCD_HOST_BEGIN

// The main kernel's launch shape for work set `w` of shard `sh` with kernel family `level`; `coll`: the results go through
// an all-reduce.  The caller adds the launch tag (and, where it has a verdict, narrow_rescale).
LaunchShape main_launch_shape(mcd_catalog* cat, const Shard& sh, const WorkSet& w, int level, bool coll, double* out_buf,
                              int64_t n_out) {
    LaunchShape shape{cat->model, cat->free_centre, cat->precision, level, w.uniform_len, sh.n};
    shape.uniform_extra = w.uniform_extra;
    shape.waves = w.waves;
    shape.chunk_general = w.d_chunk_general;
    // records beyond what the caches hold between two passes: prefetch the next loop iteration's records (mcd_math.h)
    shape.prefetch = wants_prefetch(cat, sh);
    cat->last_prefetch = shape.prefetch && shape.fast != 0;
    // Re-run signal of the fast mixture kernels.  One device: a flag word behind the outputs receives a fresh tag per
    // launch (no reset needed).  Several ranks / devices: the kernels poison the affected partial sums with NaN
    // instead, which travels through the reduce kernel and the all-reduce to every rank.
    shape.rerun_flag = coll ? nullptr : out_buf + n_out;
    shape.root_series = w.sorted && cat->root_series != 0;
    shape.root_direct = shape.root_series && cat->root_direct != 0;
    shape.root_quad = shape.root_direct && cat->root_quad != 0;          // (acts only with the split exponent offset)
    return shape;
}

// the record array the main kernel reads for work set `w` (the one its chunk table was planned on)
const void* main_records(const Shard& sh, const WorkSet& w) { return w.sorted ? sh.records_sorted : sh.records; }

// Chunks of a launch of work set `w` at kernel family `level` for the parameter table `params` in which EVERY wave takes
// the series root: the vote passes in all lanes where it passes for the smallest sigma^2 of the table.  Counted from the
// thresholds gathered at planning time (a chunk within a rounding error of its threshold may be counted either way).
int64_t series_chunk_count(const mcd_catalog* cat, const WorkSet& w, int level, const double* params, int64_t n_rows) {
    if (!w.sorted || !cat->root_series || level != 2 || w.series_need.empty()) return 0;
    const mcd::ParamRanges pr = mcd::table_ranges(cat->model, cat->free_centre, cat->k, params, n_rows);
    if (!pr.finite) return 0;
    return (int64_t)(std::upper_bound(w.series_need.begin(), w.series_need.end(), pr.s2_min) - w.series_need.begin());
}

// ... of which in the direct form of the series (option "root_direct"): both votes pass in all lanes where they pass for the
// smallest sigma^2 of the table (either condition only loosens as sigma^2 grows, so the largest passes with it)
int64_t direct_chunk_count(const mcd_catalog* cat, const WorkSet& w, int level, const double* params, int64_t n_rows) {
    if (!w.sorted || !cat->root_series || !cat->root_direct || level != 2 || w.direct_need.empty()) return 0;
    const mcd::ParamRanges pr = mcd::table_ranges(cat->model, cat->free_centre, cat->k, params, n_rows);
    if (!pr.finite) return 0;
    return (int64_t)(std::upper_bound(w.direct_need.begin(), w.direct_need.end(), pr.s2_min) - w.direct_need.begin());
}

// ... of which in the quadratic form on 32-star bands (option "root_quad"; the caller knows whether the launch holds the
// third vote at all: mcd_internal.h: root_quad_launch)
int64_t quad_chunk_count(const mcd_catalog* cat, const WorkSet& w, int level, const double* params, int64_t n_rows) {
    if (!w.sorted || !cat->root_series || !cat->root_direct || !cat->root_quad || level != 2 || w.quad_need.empty()) return 0;
    const mcd::ParamRanges pr = mcd::table_ranges(cat->model, cat->free_centre, cat->k, params, n_rows);
    if (!pr.finite) return 0;
    return (int64_t)(std::upper_bound(w.quad_need.begin(), w.quad_need.end(), pr.s2_min) - w.quad_need.begin());
}

// the fast BGFIXED kernel leaves the walker-independent sum of lnL_bg to the reduction
const double* fast_pset_const(const mcd_catalog* cat, const Shard& sh, int level) {
    const int bgk = mcd::bg_kind(cat->model);
    return (level && (bgk == mcd::BG_FIXED || bgk == mcd::BG_FIXED_DENSITY)) ? sh.d_pset_const : nullptr;
}

// Work buffers of one shard for a given walker count; the chunk table itself is planned by mcd_chunks.h: plan_chunks
// (host-only, unit-tested on the CPU).
int build_workset(mcd_catalog* cat, Shard& sh, int64_t n_walkers, WorkSet** out) {
    auto it = sh.work.find(n_walkers);
    if (it != sh.work.end()) { *out = &it->second; return MCD_OK; }
    if (sh.work.size() >= 8) {                       // bound the cache (emcee uses W and W/2)
        for (auto& kv : sh.work) free_workset(kv.second);
        sh.work.clear();
        cat->cur_walkers = 0;                        // whatever was staged is gone; stage_params sets it again on success
    }
    const DeviceSlot& slot = cat->ctx->slots[sh.slot];
    MCD_HIP(hipSetDevice(slot.device));

    // balanced single-round plan where it pays (option "balance": -1 by the rule above, 0 never, m forced); a catalogue
    // too small for m workgroups per CU (fewer than 16 stars per chunk) takes half as many, down to the multi-round table
    // (the narrow-range exceptions and the series thresholds below belong to the array the kernel reads)
    const bool sorted = wants_sorted(cat, sh);
    if (sorted)
        if (int rc = ensure_sorted_records(cat, sh)) return rc;
    const std::vector<int64_t>& exceptions = sorted ? sh.sorted_exceptions : cat->stats.narrow_exceptions;
    mcd::ChunkPlan plan;
    for (int m = cat->balance < 0 ? balance_auto_m(cat, sh.n, n_walkers) : cat->balance;; m /= 2) {
        plan = mcd::plan_chunks(cat->bin_offsets, sh.star_begin, sh.n, n_walkers, cat->target_waves, cat->tail_split,
                                exceptions, cat->chunk_len, m);
        if (m == 0 || plan.balanced_m > 0) break;
    }
    const std::vector<mcd::Chunk>& chunks = plan.chunks;
    const std::vector<int64_t>& offs = plan.offsets;
    const std::vector<uint8_t>& general = plan.general;

    WorkSet w;
    w.n_walkers = n_walkers;
    w.n_chunks = (int64_t)chunks.size();
    w.max_chunks_per_pset = plan.max_chunks_per_pset;
    w.uniform_len = plan.uniform_len;
    w.uniform_extra = plan.uniform_extra;
    w.sorted = sorted;
    if (sorted) {
        w.series_need = mcd::series_thresholds(plan, sh.sorted_e2.data());
        w.direct_need = mcd::direct_thresholds(plan, sh.sorted_e2.data());
    }
    const std::vector<double> split_const =
        sorted ? mcd::exp_split_chunk_consts(plan, sh.sorted_nbf.data(), sh.sorted_e2.data(), sh.n) : std::vector<double>();
    if (sorted) w.quad_need = mcd::quad_thresholds(plan, sh.sorted_e2.data(), split_const.data() + 1, 2);
    {
        // balanced plans with an even number of workgroups per CU run as half as many 8-wave workgroups that add their
        // chunks' sums up themselves: half (to an eighth of) the partial sums per walker (mcd_kernels.hip: loglike_kernel)
        const int64_t n_wtiles = (n_walkers + 63) / 64;
        const bool shape_ok = plan.balanced_m > 0 && plan.balanced_m % 2 == 0 && (n_wtiles == 1 || n_wtiles == 2 || n_wtiles == 4) &&
                              cat->precision == MCD_F64;
        w.waves = 4;
        if (cat->combine != 0 && shape_ok) {
            // 4 workgroups per CU as one 16-wave workgroup: 256 partial sums per walker, which the resident chain's step
            // kernel adds up itself (mcd_stretch.hip) -- 3 - 6 % slower than two 8-wave workgroups, one kernel less per
            // half step; 8 per CU stay 8-wave workgroups (1e5 stars x 256 walkers: 14.5 us per step against 15.1)
            const bool can16 = mcd::bg_kind(cat->model) != mcd::BG_GAUSS;
            w.waves = 8;
            if (cat->combine == 16 && plan.balanced_m % 4 == 0 && can16) w.waves = 16;
            // (kernel traces of the C2 bench: 16-wave main kernel 10.7 us + one-wave-per-group reduction 4.6 against 12.0 + 4.0
            // with 8-wave workgroups and 512 partial sums per walker; wall-clock sweeps put the two within their noise)
            if (cat->combine == 1 && plan.balanced_m == 4 && can16) w.waves = 16;
        }
    }
    const int64_t n_out = cat->n_psets * n_walkers;
    const size_t term_bytes = cat->precision == MCD_F64 ? 8 : 4;
    auto allocate = [&]() -> hipError_t {
        hipError_t e;
        if (!general.empty()) {
            if ((e = hipMalloc(&w.d_chunk_general, general.size())) != hipSuccess) return e;
            if ((e = hipMemcpy(w.d_chunk_general, general.data(), general.size(), hipMemcpyHostToDevice)) != hipSuccess) return e;
        }
        if (!split_const.empty()) {
            if ((e = hipMalloc(&w.d_split_const, split_const.size() * sizeof(double))) != hipSuccess) return e;
            if ((e = hipMemcpy(w.d_split_const, split_const.data(), split_const.size() * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess) return e;
        }
        if ((e = hipMalloc(&w.d_chunks, std::max<size_t>(1, chunks.size()) * sizeof(mcd::Chunk))) != hipSuccess) return e;
        if ((e = hipMalloc(&w.d_offsets, offs.size() * sizeof(int64_t))) != hipSuccess) return e;
        if ((e = hipMalloc(&w.d_params, (size_t)n_out * cat->k * sizeof(double))) != hipSuccess) return e;
        if ((e = hipMalloc(&w.d_wpar, (size_t)n_out * mcd::KD * term_bytes)) != hipSuccess) return e;
        if ((e = hipMalloc(&w.d_partials, std::max<size_t>(1, (size_t)mcd::padded_walkers(n_walkers) * w.n_chunks) * sizeof(double))) != hipSuccess) return e;
        if ((e = hipMalloc(&w.d_out, (size_t)(n_out + 1) * sizeof(double))) != hipSuccess) return e;   // + re-run flag word
        if ((e = hipMemset(w.d_out, 0, (size_t)(n_out + 1) * sizeof(double))) != hipSuccess) return e;
        if ((e = hipMalloc(&w.d_out2, (size_t)(n_out + 1) * sizeof(double))) != hipSuccess) return e;
        if ((e = hipMemset(w.d_out2, 0, (size_t)(n_out + 1) * sizeof(double))) != hipSuccess) return e;
        if ((e = hipEventCreateWithFlags(&w.ev_staged, hipEventDisableTiming)) != hipSuccess) return e;
        for (int b = 0; b < 2; ++b) {
            if ((e = hipEventCreateWithFlags(&w.ev_reduced[b], hipEventDisableTiming)) != hipSuccess) return e;
            if ((e = hipEventCreateWithFlags(&w.ev_comm[b], hipEventDisableTiming)) != hipSuccess) return e;
        }
        if ((e = hipHostMalloc(&w.h_params, (size_t)n_out * cat->k * sizeof(double), hipHostMallocMapped)) != hipSuccess) return e;
        if ((e = hipHostMalloc(&w.h_out, (size_t)(n_out + 1) * sizeof(double), hipHostMallocMapped)) != hipSuccess) return e;
        std::memset(w.h_out, 0, (size_t)(n_out + 1) * sizeof(double));
        if ((e = hipHostGetDevicePointer((void**)&w.m_params, w.h_params, 0)) != hipSuccess) return e;
        if ((e = hipHostGetDevicePointer((void**)&w.m_out, w.h_out, 0)) != hipSuccess) return e;
        if (!chunks.empty() &&
            (e = hipMemcpy(w.d_chunks, chunks.data(), chunks.size() * sizeof(mcd::Chunk), hipMemcpyHostToDevice)) != hipSuccess)
            return e;
        return hipMemcpy(w.d_offsets, offs.data(), offs.size() * sizeof(int64_t), hipMemcpyHostToDevice);
    };
    const hipError_t err = allocate();
    if (err != hipSuccess) {
        free_workset(w);
        return fail(MCD_ERR_HIP, std::string("work buffers for this walker count: ") + hipGetErrorString(err));
    }
    auto ins = sh.work.emplace(n_walkers, w);
    *out = &ins.first->second;
    return MCD_OK;
}

MCD_HOST_END

extern "C" {

static int catalog_create_impl(mcd_ctx* ctx, const mcd_catalog_desc* d, std::unique_ptr<mcd_catalog>& cat);

int mcd_catalog_create(mcd_ctx* ctx, const mcd_catalog_desc* d, mcd_catalog** out) {
    try {
    if (!ctx || !d || !out) return fail(MCD_ERR_INVALID, "mcd_catalog_create: null argument");
    std::unique_ptr<mcd_catalog> cat;
    const int rc = catalog_create_impl(ctx, d, cat);
    if (rc != MCD_OK) {
        if (cat) {                                   // release whatever device memory was already allocated
            const std::string msg = g_last_error;
            mcd_catalog_destroy(cat.release());
            g_last_error = msg;
        }
        return rc;
    }
    *out = cat.release();
    return MCD_OK;
    } catch (...) { return on_exception("mcd_catalog_create"); }
}

static int catalog_create_impl(mcd_ctx* ctx, const mcd_catalog_desc* d, std::unique_ptr<mcd_catalog>& cat) {
    if (int urc = ctx_usable(ctx)) return urc;
    if (d->n_stars < 0) return fail(MCD_ERR_INVALID, "negative n_stars");
    if (!mcd::is_launch_model(d->model)) return fail(MCD_ERR_INVALID, "unknown model");
    const int bgk = mcd::bg_kind(d->model);
    if (d->centre != MCD_CENTRE_FIXED && d->centre != MCD_CENTRE_FREE) return fail(MCD_ERR_INVALID, "unknown centre mode");
    if (d->precision < MCD_F64 || d->precision > MCD_F32_ACC64) return fail(MCD_ERR_INVALID, "unknown precision");
    if (mcd::is_double(d->model) && d->precision != MCD_F64)
        return fail(MCD_ERR_INVALID, "the double Lynden-Bell models (MCD_MODEL_DOUBLE, MCD_MODEL_DOUBLE_BGGAUSS) are float64 only: "
                                     "float32 and f32acc64 catalogues are out of scope for them");
    if (mcd::is_escale(d->model) && d->precision != MCD_F64)
        return fail(MCD_ERR_INVALID, "the error-scale models (MCD_MODEL_CONST_ESCALE, MCD_MODEL_PROFILE_ESCALE) are float64 only: "
                                     "float32 and f32acc64 catalogues are out of scope for them");
    if (d->n_stars > 0 && (!d->ra || !d->dec || !d->v || !d->verr)) return fail(MCD_ERR_INVALID, "missing ra/dec/v/verr column");
    if (bgk == mcd::BG_FIXED && d->n_stars > 0 && (!d->lnlike_bg || !d->pmember))
        return fail(MCD_ERR_INVALID, "background model needs lnlike_bg and pmember columns");
    if (bgk == mcd::BG_GAUSS && d->n_stars > 0 && !d->density)
        return fail(MCD_ERR_INVALID, "Gaussian-background model needs the density column");
    if (bgk == mcd::BG_FIXED_DENSITY && d->n_stars > 0 && (!d->lnlike_bg || !d->density))
        return fail(MCD_ERR_INVALID, "constant-background model needs lnlike_bg and density columns");

    cat.reset(new (std::nothrow) mcd_catalog());
    if (!cat) return fail(MCD_ERR_INVALID, "out of memory");
    cat->ctx = ctx;
    cat->model = d->model;
    cat->free_centre = d->centre == MCD_CENTRE_FREE;
    cat->precision = d->precision;
    cat->k = param_count(d->model, cat->free_centre);
    cat->n_stars = d->n_stars;
    if (const char* tw = std::getenv("MCD_TARGET_WAVES")) {
        long v = std::atol(tw);
        if (v > 0) cat->target_waves = v;
    }
    if (d->n_bins > 1) {
        if (!d->bin_offsets) return fail(MCD_ERR_INVALID, "bin_offsets required when n_bins > 1");
        cat->n_psets = d->n_bins;
        cat->bin_offsets.assign(d->bin_offsets, d->bin_offsets + d->n_bins + 1);
        if (cat->bin_offsets.front() != 0 || cat->bin_offsets.back() != d->n_stars)
            return fail(MCD_ERR_INVALID, "bin_offsets must start at 0 and end at n_stars");
        for (int64_t b = 0; b < d->n_bins; ++b)
            if (cat->bin_offsets[b + 1] < cat->bin_offsets[b]) return fail(MCD_ERR_INVALID, "bin_offsets must be non-decreasing");
    } else {
        cat->n_psets = 1;
        cat->bin_offsets = {0, d->n_stars};
    }

    // range statistics for the fast-path guard
    cat->stats = mcd::compute_stats(d->n_stars, d->v, d->verr, d->lnlike_bg, d->pmember, d->density, bgk,
                                    cat->precision != MCD_F64 || mcd::is_profile(cat->model) ? d->ra : nullptr, d->dec,
                                    !cat->free_centre, d->ra_center, d->dec_center);

    // contiguous star shards, one per device of this process
    const int n_dev = (int)ctx->slots.size();
    cat->shards.resize(n_dev);
    const int rec_bytes = mcd::record_bytes(cat->model, cat->free_centre, cat->precision);
    for (int i = 0; i < n_dev; ++i) {
        Shard& sh = cat->shards[i];
        sh.slot = i;
        const mcd::ShardRange range = mcd::shard_range(d->n_stars, i, n_dev);
        sh.star_begin = range.begin;
        sh.n = range.n;
        const DeviceSlot& slot = ctx->slots[i];
        MCD_HIP(hipSetDevice(slot.device));
        MCD_HIP(hipEventCreate(&sh.ev_begin));
        MCD_HIP(hipEventCreate(&sh.ev_k0));
        MCD_HIP(hipEventCreate(&sh.ev_k1));
        MCD_HIP(hipEventCreate(&sh.ev_end));
        // slack: wide scalar loads and the software prefetch of the following loop iterations (mcd_math.h: RecordPrefetch)
        // read up to 1.5 KiB past a chunk's last record
        MCD_HIP(hipMalloc(&sh.records, (size_t)sh.n * rec_bytes + 2048));
        MCD_HIP(hipMemsetAsync(sh.records, 0, (size_t)sh.n * rec_bytes + 2048, slot.stream));
        if (bgk == mcd::BG_FIXED || bgk == mcd::BG_FIXED_DENSITY) {
            const std::vector<double> sums = mcd::pset_background_sums(d->lnlike_bg, cat->bin_offsets, sh.star_begin, sh.n);
            MCD_HIP(hipMalloc(&sh.d_pset_const, sums.size() * sizeof(double)));
            MCD_HIP(hipMemcpy(sh.d_pset_const, sums.data(), sums.size() * sizeof(double), hipMemcpyHostToDevice));
        }
        if (sh.n == 0) continue;
        // raw columns -> device scratch -> packed records (device-side trig), scratch freed afterwards
        const double* host_cols[7] = {d->ra, d->dec, d->v, d->verr, d->lnlike_bg, d->pmember, d->density};
        struct Scratch {                                    // freed on every exit path
            double* p[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
            ~Scratch() { for (double* q : p) if (q) (void)hipFree(q); }
        } dev;
        for (int c = 0; c < 7; ++c) {
            if (!host_cols[c]) continue;
            MCD_HIP(hipMalloc(&dev.p[c], (size_t)sh.n * sizeof(double)));
            MCD_HIP(hipMemcpyAsync(dev.p[c], host_cols[c] + sh.star_begin, (size_t)sh.n * sizeof(double),
                                   hipMemcpyHostToDevice, slot.stream));
        }
        mcd::RawColumns raw{dev.p[0], dev.p[1], dev.p[2], dev.p[3], dev.p[4], dev.p[5], dev.p[6]};
        MCD_HIP(mcd::launch_prepare_records(slot.stream, raw, sh.n, cat->model, cat->free_centre, cat->precision,
                                            d->ra_center, d->dec_center, sh.records));
        MCD_HIP(hipStreamSynchronize(slot.stream));
    }
    return MCD_OK;
}

int mcd_catalog_destroy(mcd_catalog* cat) {
    if (!cat) return MCD_OK;
    if (cat->ctx && cat->ctx->failed.load()) { delete cat; return MCD_OK; }      // (see mcd_ctx_destroy: nothing may be waited for)
    for (Shard& sh : cat->shards) {
        (void)hipSetDevice(cat->ctx->slots[sh.slot].device);
        (void)hipStreamSynchronize(cat->ctx->slots[sh.slot].stream);
        (void)hipStreamSynchronize(cat->ctx->slots[sh.slot].comm_stream);
        (void)hipStreamSynchronize(cat->ctx->slots[sh.slot].stream2);
        for (auto& kv : sh.work) free_workset(kv.second);
        if (sh.records) (void)hipFree(sh.records);
        if (sh.records_sorted) (void)hipFree(sh.records_sorted);
        if (sh.records_split) (void)hipFree(sh.records_split);
        if (sh.d_pset_const) (void)hipFree(sh.d_pset_const);
        if (sh.ev_begin) (void)hipEventDestroy(sh.ev_begin);
        if (sh.ev_k0) (void)hipEventDestroy(sh.ev_k0);
        if (sh.ev_k1) (void)hipEventDestroy(sh.ev_k1);
        if (sh.ev_end) (void)hipEventDestroy(sh.ev_end);
        for (auto& pr : sh.ring) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    }
    release_holdout(cat);
    release_weighted(cat);
    release_simulated(cat);
    for (hipEvent_t e : cat->chain_events) (void)hipEventDestroy(e);
    if (cat->chain.d) (void)hipFree(cat->chain.d);
    if (cat->chain.h) (void)hipHostFree(cat->chain.h);
    if (cat->hmc.d) (void)hipFree(cat->hmc.d);
    if (cat->hmc.h) (void)hipHostFree(cat->hmc.h);
    if (cat->temper.d) (void)hipFree(cat->temper.d);
    if (cat->temper.h) (void)hipHostFree(cat->temper.h);
    delete cat;
    return MCD_OK;
}

int mcd_catalog_param_count(const mcd_catalog* cat) { return cat ? cat->k : MCD_ERR_INVALID; }
int64_t mcd_catalog_n_stars(const mcd_catalog* cat) { return cat ? cat->n_stars : MCD_ERR_INVALID; }
int64_t mcd_catalog_n_outputs(const mcd_catalog* cat, int64_t n_walkers) {
    return cat ? cat->n_psets * n_walkers : MCD_ERR_INVALID;
}

int mcd_set_option(mcd_catalog* cat, const char* key, int64_t value) {
    try {
    if (!cat || !key) return fail(MCD_ERR_INVALID, "mcd_set_option: null argument");
    if (!std::strcmp(key, "timing")) {
        int rc = sync_all(cat);
        if (rc != MCD_OK) return rc;
        cat->timing = value != 0;
        cat->timing_all = value == 2;
        for (Shard& sh : cat->shards) sh.ring_used = 0;
        return MCD_OK;
    }
    if (!std::strcmp(key, "timing_discard")) {
        // forget the event pairs recorded so far without reading them (hipEventElapsedTime over hundreds of pairs takes
        // milliseconds, long enough for an idle GPU to leave its sustained clocks right before a measured region)
        int rc = sync_all(cat);
        if (rc != MCD_OK) return rc;
        for (Shard& sh : cat->shards) sh.ring_used = 0;
        cat->timing_launches = 0;
        return MCD_OK;
    }
    if (!std::strcmp(key, "timing_stride")) {
        if (value < 1) return fail(MCD_ERR_INVALID, "timing_stride must be >= 1");
        int rc = sync_all(cat);
        if (rc != MCD_OK) return rc;
        cat->timing_stride = value;
        cat->timing_launches = 0;
        return MCD_OK;
    }
    if (!std::strcmp(key, "timing_reserve")) {
        // create the per-launch event pairs of "timing" = 2 ahead of a measured loop (hipEventCreate costs microseconds)
        if (value < 0 || value > ((int64_t)1 << 16)) return fail(MCD_ERR_INVALID, "timing_reserve: 0 .. 65536 launches");
        for (Shard& sh : cat->shards) {
            MCD_HIP(hipSetDevice(cat->ctx->slots[sh.slot].device));
            while ((int64_t)sh.ring.size() < value) {
                hipEvent_t a, b;
                MCD_HIP(hipEventCreate(&a));
                if (hipEventCreate(&b) != hipSuccess) { (void)hipEventDestroy(a); return fail(MCD_ERR_HIP, "hipEventCreate"); }
                sh.ring.emplace_back(a, b);
            }
        }
        return MCD_OK;
    }
    for (const Option& o : kOptions) {
        if (std::strcmp(key, o.key)) continue;
        if (value < o.min || value > o.max || (o.accepts && !o.accepts(value))) return fail(MCD_ERR_INVALID, o.message);
        if (o.sync)
            if (int rc = sync_all(cat)) return rc;
        o.set(cat, value);
        if (o.replan) {
            for (Shard& sh : cat->shards) {            // chunk tables depend on it: rebuild lazily
                (void)hipSetDevice(cat->ctx->slots[sh.slot].device);
                for (auto& kv : sh.work) free_workset(kv.second);
                sh.work.clear();
            }
            release_holdout(cat);
            release_weighted(cat);
            release_simulated(cat, true);              // (the plans go, the resident set stays)
            cat->cur_walkers = 0;
        }
        return MCD_OK;
    }
    return fail(MCD_ERR_INVALID, std::string("unknown option: ") + key);
    } catch (...) { return on_exception("mcd_set_option"); }
}

int mcd_timing_collect(mcd_catalog* cat, double* total_kernel_ms, int64_t* n_launches) {
    try {
    if (!cat) return fail(MCD_ERR_INVALID, "null catalogue");
    int rc = sync_all(cat);
    if (rc != MCD_OK) return rc;
    Shard& sh = cat->shards[0];
    double total = 0.0;
    for (size_t i = 0; i < sh.ring_used; ++i) {
        float ms = 0.f;
        MCD_HIP(hipEventElapsedTime(&ms, sh.ring[i].first, sh.ring[i].second));
        total += ms;
    }
    if (total_kernel_ms) *total_kernel_ms = total;
    if (n_launches) *n_launches = (int64_t)sh.ring_used;
    for (Shard& s2 : cat->shards) s2.ring_used = 0;
    cat->timing_launches = 0;                  // the first launch after a collect is sampled
    return MCD_OK;
    } catch (...) { return on_exception("mcd_timing_collect"); }
}

int64_t mcd_rerun_count(const mcd_catalog* cat) { return cat ? cat->n_reruns : MCD_ERR_INVALID; }

int mcd_stretch_info(const mcd_catalog* cat, int64_t* device_blocks, int64_t* host_blocks, int64_t* discarded_blocks,
                     int32_t* last_discard_status) {
    if (!cat) return fail(MCD_ERR_INVALID, "null catalogue");
    if (device_blocks) *device_blocks = cat->chain_device_blocks;
    if (host_blocks) *host_blocks = cat->chain_host_blocks;
    if (discarded_blocks) *discarded_blocks = cat->chain_discarded;
    if (last_discard_status) *last_discard_status = cat->chain_last_status;
    return MCD_OK;
}

int mcd_last_prefetch(const mcd_catalog* cat) { return cat ? cat->last_prefetch : -1; }

int64_t mcd_last_series_chunks(const mcd_catalog* cat) { return cat ? cat->last_series_chunks : -1; }
int64_t mcd_last_direct_chunks(const mcd_catalog* cat) { return cat ? cat->last_direct_chunks : -1; }

int mcd_last_narrow_bounded(const mcd_catalog* cat) { return cat ? cat->last_narrow_bounded : -1; }
int mcd_last_exp_split(const mcd_catalog* cat) { return cat ? cat->last_exp_split : -1; }
int mcd_last_root_quad(const mcd_catalog* cat) { return cat ? cat->last_root_quad : -1; }
int mcd_last_block_step(const mcd_catalog* cat) { return cat ? cat->last_block_step : -1; }
int64_t mcd_last_quad_chunks(const mcd_catalog* cat) { return cat ? cat->last_quad_chunks : -1; }

int mcd_last_f32_domain(const mcd_catalog* cat, double* kappa_v, double* kappa_theta) {
    if (!cat) return -1;
    if (kappa_v) *kappa_v = cat->last_f32.kappa_v;
    if (kappa_theta) *kappa_theta = cat->last_f32.kappa_theta;
    if (cat->precision == MCD_F64) return 1;
    return cat->last_f32.inside ? 1 : 0;
}

int mcd_f32_outside(const mcd_catalog* cat, int64_t* calls, double* worst_kappa_v, double* worst_kappa_theta,
                    const char** reason) {
    if (!cat) return fail(MCD_ERR_INVALID, "null catalogue");
    if (calls) *calls = cat->f32_outside_calls;
    if (worst_kappa_v) *worst_kappa_v = cat->f32_worst_kappa_v;
    if (worst_kappa_theta) *worst_kappa_theta = cat->f32_worst_kappa_theta;
    if (reason) *reason = cat->f32_outside_reason;
    return MCD_OK;
}

int mcd_last_fast_level(const mcd_catalog* cat) {
    if (!cat || cat->cur_walkers <= 0 || cat->shards.empty()) return -1;
    const auto it = cat->shards.front().work.find(cat->cur_walkers);
    return it == cat->shards.front().work.end() ? -1 : it->second.fast;
}

double mcd_last_kernel_ms(const mcd_catalog* cat) { return cat ? cat->last_kernel_ms : -1.0; }
double mcd_last_device_ms(const mcd_catalog* cat) { return cat ? cat->last_device_ms : -1.0; }

int mcd_last_launch_info(const mcd_catalog* cat, int64_t* n_workgroups, int32_t* walker_tile, int64_t* n_chunks,
                         int32_t* record_bytes) {
    if (!cat) return fail(MCD_ERR_INVALID, "null catalogue");
    if (n_workgroups) *n_workgroups = cat->last_grid;
    if (walker_tile) *walker_tile = 64;
    if (n_chunks) *n_chunks = cat->last_chunks;
    if (record_bytes) *record_bytes = mcd::record_bytes(cat->model, cat->free_centre, cat->precision);
    return MCD_OK;
}

}  // extern "C"

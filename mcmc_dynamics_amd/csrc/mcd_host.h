// mcd_host.h -- private header of the host units behind the C-ABI of the MI355X log-likelihood library (include/mcd.h).
//
// Host-side responsibilities: device/stream/communicator set-up, one-off upload and packing of the
// star catalogue into HBM, star sharding across devices, chunk tables, per-call launch sequence
//   params H2D -> walker prep -> main kernel -> fixed-order reduce -> [RCCL all-reduce] -> D2H,
// and HIP-event timing for the measurement harness.  No C++ exception leaves a unit, and none defines a kernel:
//   mcd_api_ctx.hip        error state, RCCL loading, contexts, the failure / abort protocol, waits on a context's streams
//   mcd_api_catalog.hip    catalogues, work sets and chunk plans, the main kernel's launch shape, options, mcd_last_* queries
//   mcd_api_eval.hip       staging, enqueue, sync, fetch; the per-star outputs of one parameter row
//   mcd_api_chain.hip      the stretch-move block and the HMC block, each resident on the device or host-driven
//   mcd_api_de.hip         the differential-evolution block (mcd_de.h), resident on the device or host-driven
//   mcd_api_temper.hip     the parallel-tempering block in the same two forms
//   mcd_api_summaries.hip  mcd_pointwise_posterior, mcd_psis_loo, mcd_kde_background
//   mcd_api_holdout.hip    mcd_holdout_loglike, mcd_holdout_pointwise: the exact leave-out refits
//   mcd_api_mmatch.hip     mcd_moment_match: the decision loop of moment matching around the hold-out evaluation
//   mcd_api_replicate.hip  mcd_replicate_check, mcd_replicate_numbers: replicated-data predictive checks per range of stars
//   mcd_api_weighted.hip   mcd_weighted_loglike_grad, mcd_weighted_loglike, mcd_bootstrap_weights: value and gradient, or
//                          the value alone, under per-row star weights
//   mcd_api_simulated.hip  mcd_simulate, mcd_simulated_set, mcd_simulated_loglike, mcd_simulated_loglike_grad,
//                          mcd_simulated_info: simulated catalogues resident on the device, and every parameter row (value,
//                          or value and gradient) against the velocities of its own simulation
//   mcd_api_diag.hip       mcd_chain_diagnostics: on the host without a context, on the context's first device with one
// The kernel units they call share mcd_dispatch.h ((model, free_centre) and term precision -> template arguments, the one
// list of models) and mcd_launch.h (workgroup shape, padded_walkers, the main kernels' wave mapping and partial-sum address).
// What crosses units is in mcd::host (hidden: not among the library's exported symbols), the rest in each unit's
// anonymous namespace.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>   // types and prototypes only: librccl.so is dlopen'ed on first multi-GPU use

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mcd.h"
#include "mcd_exp_split.h"
#include "mcd_internal.h"
#include "mcd_guard.h"
#include "mcd_math.h"

struct mcd_ctx;
struct mcd_catalog;

// (the visibility holds for what one namespace block declares: the units open theirs with the same macro)
#define MCD_HOST_BEGIN namespace mcd { namespace host __attribute__((visibility("hidden"))) {
#define MCD_HOST_END }}
MCD_HOST_BEGIN

extern thread_local std::string g_last_error;          // what mcd_last_error returns (mcd_api_ctx.hip)
int fail(int code, const std::string& msg);
int on_exception(const char* where) noexcept;

#define MCD_HIP(call)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (call);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return ::mcd::host::fail(MCD_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));   \
    } while (0)

// RCCL entry points, resolved lazily so that single-GPU processes never load or initialise RCCL.
struct Rccl {
    void* handle = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
    decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
    decltype(&ncclCommCount) CommCount = nullptr;
    decltype(&ncclCommUserRank) CommUserRank = nullptr;
    decltype(&ncclGetVersion) GetVersion = nullptr;
};
extern Rccl g_rccl;                                     // one per process (mcd_api_ctx.hip)
int load_rccl();

#define MCD_NCCL(call)                                                                                  \
    do {                                                                                                \
        ncclResult_t r_ = (call);                                                                       \
        if (r_ != ncclSuccess)                                                                          \
            return ::mcd::host::fail(MCD_ERR_RCCL,                                                      \
                                   std::string(#call) + ": " + ::mcd::host::g_rccl.GetErrorString(r_)); \
    } while (0)

struct DeviceSlot {
    int device = 0;
    hipStream_t stream = nullptr;        // kernels, copies
    hipStream_t stream2 = nullptr;       // second compute lane of pipelined evaluations (WorkSet: two lanes)
    hipStream_t comm_stream = nullptr;   // the per-step all-reduce, so that it overlaps the next step's kernels
    ncclComm_t comm = nullptr;
};

// per-(shard, walker-count) work buffers
struct WorkSet {
    int64_t n_walkers = 0;
    int64_t n_chunks = 0;
    int64_t max_chunks_per_pset = 0;
    int uniform_len = 0;               // > 0 when the chunk table is arithmetic (single set; mcd_chunks.h: uniform_chunk)
    int uniform_extra = 0;
    int waves = 4;                     // 8: balanced plan whose workgroups combine their chunks' sums (f64 fast kernels only)
    mcd::Chunk* d_chunks = nullptr;
    int64_t* d_offsets = nullptr;      // [n_psets + 1] chunk offsets
    uint8_t* d_chunk_general = nullptr;   // [n_chunks] chunks excluded from the narrow-range variant; null when there are none
    double* d_split_const = nullptr;      // [n_chunks][2] sorted: what a direct chunk run with the split exponent offset adds
                                          // to its sum, and the largest half-width of a 32-star block it touches
                                          // (mcd_exp_split.h: exp_split_chunk_consts)
    double* d_params = nullptr;        // [n_psets][W][K]
    void* d_wpar = nullptr;            // [n_psets][W][KD]
    double* d_partials = nullptr;      // [roundup64(W) / 8][n_chunks][8]
    double* d_out = nullptr;           // [n_psets][W] (+ flag word)
    double* d_out2 = nullptr;          // second result buffer: collective mode alternates between the two, so that the
                                       // all-reduce of step i (comm stream) overlaps the kernels of step i + 1
    int buf = 0;                       // buffer the last enqueue wrote (0 for blocking calls without a collective)
    // Pipelined evaluations on ONE device without a collective alternate between two LANES: lane 0 = the compute stream
    // with (d_partials, d_out), lane 1 = the second stream with (d_partials2, d_out2).  Consecutive evaluations are
    // independent (each has its parameters staged), so the reduction and the launch ramp of one overlap the main kernel
    // of the next instead of sitting between two main kernels on one stream (enqueue(): two_lanes).
    double* d_partials2 = nullptr;
    // mcd_loglike_grad_batch (sized on first use): partial sums [1 + K][roundup64(W) / 8][n_chunks][8], results
    // [n_psets][1 + K][roundup64(W)] on the device and in pinned host memory
    double* d_grad_partials = nullptr;
    double* d_grad_out = nullptr;
    double* h_grad_out = nullptr;
    hipEvent_t ev_staged = nullptr;    // parameters staged (on the compute stream): lane 1 waits for it once per staging
    bool lane1_knows_staging = false;
    bool lane1_used = false;           // something may be in flight on the second stream
    hipEvent_t ev_reduced[2] = {nullptr, nullptr};   // reduce kernel done, buffer b ready for the all-reduce
    hipEvent_t ev_comm[2] = {nullptr, nullptr};      // all-reduce of buffer b done
    bool comm_pending[2] = {false, false};
    double* h_params = nullptr;        // pinned + mapped
    double* h_out = nullptr;           // pinned + mapped
    double* m_params = nullptr;        // device view of h_params (zero-copy path of the blocking call)
    double* m_out = nullptr;           // device view of h_out
    bool mapped = false;               // last staging used the zero-copy path: results land in h_out directly
    double launch_tag = 0.0;           // tag of the last fast-path launch (written to out[n_out] by a kernel that wants a re-run)
    int fast = 0;                      // mcd::LaunchShape::fast level of the staged batch
    int narrow_rescale = 0;            // its bounded narrow-range verdict (mcd_guard.h: bounded_rescale; R or 0)
    bool exp_split[2] = {false, false};   // mcd_guard.h: exp_split_admitted for the staged batch: [0] in the loops that keep the
                                          // clamp, [1] in the bounded loop with R = narrow_rescale
    bool block_step = false;           // mcd_guard.h: block_step_admitted for the staged batch (56 raw factors fit the bounded loop)
    bool staged = false;
    bool sorted = false;               // planned on, and launched with, the shard's verr-sorted records (Shard::records_sorted)
    std::vector<double> series_need;   // sorted: per chunk outside chunk_general, the smallest sigma^2 with which its verr^2
                                       // band passes the series vote (mcd_math.h: RootSeries), ascending
    int64_t series_chunks = 0;         // chunks of the staged batch every wave of which takes the series root
    std::vector<double> direct_need;   // sorted: ... and the smallest sigma^2 with which the chunk also passes the vote on the
                                       // direct form of the series (mcd_math.h: RootDirect)
    int64_t direct_chunks = 0;         // chunks of the staged batch every wave of which takes the direct form
    std::vector<double> quad_need;     // sorted: ... and the smallest sigma^2 with which the chunk passes the third vote too
                                       // (mcd_math.h: RootQuad; mcd_chunks.h: quad_thresholds)
    int64_t quad_chunks = 0;           // chunks of the staged batch every wave of which takes the quadratic form
};

// device arena of the resident stretch-move chain and its pinned host mirror (same layout, see stretch_block_device)
struct ChainArena {
    char* d = nullptr;
    char* h = nullptr;
    size_t bytes = 0;
};

struct Shard {
    int slot = 0;                      // index into ctx->slots
    int64_t star_begin = 0;            // global index of the first star held here
    int64_t n = 0;
    void* records = nullptr;
    // The same records ordered by verr ascending, read by the main kernel only (option "verr_sorted"; built on first use by
    // ensure_sorted_records): every kernel that reports per star keeps `records`, i.e. catalogue order.
    void* records_sorted = nullptr;
    std::vector<double> sorted_e2;            // verr^2 of records_sorted, in its order
    // records_sorted with the split exponent offset, [v, verr^2, cx, cy, M, omp', 0, 0] per star (mcd_exp_split.h; made with
    // records_sorted, read by the direct chunks of a launch with option "exp_split"), and the stars' nbf on the host
    void* records_split = nullptr;
    std::vector<double> sorted_nbf;
    std::vector<int64_t> sorted_exceptions;   // CatalogStats::narrow_exceptions of this shard as positions in records_sorted
                                              // (+ star_begin, ascending: what plan_chunks takes)
    double* d_pset_const = nullptr;    // BGFIXED: sum of lnlike_bg over this shard's stars of each parameter set
    std::map<int64_t, WorkSet> work;   // keyed by walker count
    hipEvent_t ev_begin = nullptr, ev_k0 = nullptr, ev_k1 = nullptr, ev_end = nullptr;
    // "timing" = 2: one (start, stop) event pair per main-kernel launch, summed by mcd_timing_collect
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ring;
    size_t ring_used = 0;
};

// mcd_holdout_loglike: the range plan of one (set_offsets, E W) and its buffers (mcd_api_holdout.hip), kept by the catalogue
struct HoldoutWork {
    int64_t n_rows = 0;                // E W
    int64_t n_ranges = 0;              // the sets [, the remainder] (mcd_holdout.h: holdout_ranges)
    int64_t n_chunks = 0;
    int64_t max_chunks_per_range = 0;
    mcd::Chunk* d_chunks = nullptr;
    int64_t* d_offsets = nullptr;      // [n_ranges + 1] chunk offsets
    double* d_params = nullptr;        // [E W][K]
    void* d_wpar = nullptr;            // [E W][KD]
    double* d_partials = nullptr;      // [roundup64(E W) / 8][n_chunks][8]
    double* d_sums = nullptr;          // [n_ranges][E W]
    double* d_out = nullptr;           // [2][E W] train, test
    double* h_params = nullptr;        // pinned
    double* h_out = nullptr;           // pinned
    hipEvent_t e0 = nullptr, e1 = nullptr;   // option "timing": around the main kernel
};

// mcd_weighted_loglike_grad, mcd_weighted_loglike, mcd_simulated_loglike: the chunk table over `records` for one row count
// and its buffers (mcd_api_weighted.hip), kept by the catalogue; the value calls' have one field where the gradient call's
// have 1 + K
struct WeightedWork {
    int64_t n_rows = 0;
    int64_t n_chunks = 0;
    mcd::Chunk* d_chunks = nullptr;
    int64_t* d_offsets = nullptr;      // [2] chunk offsets of the one range
    double* d_params = nullptr;        // [R][K]
    void* d_wpar = nullptr;            // [R][KD]
    int64_t* d_replicate = nullptr;    // [R]
    double* d_partials = nullptr;      // [1 + K][roundup64(R) / 8][n_chunks][8]
    double* d_out = nullptr;           // [1 + K][roundup64(R)]
    double* h_params = nullptr;        // pinned
    int64_t* h_replicate = nullptr;    // pinned
    double* h_out = nullptr;           // pinned
    hipEvent_t e0 = nullptr, e1 = nullptr;   // option "timing": around the main kernel
};

// Device scratch of one call: hipMalloc'ed blocks and an optional pair of timing events, released on every exit path.
struct DeviceScratch {
    std::vector<void*> blocks;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    DeviceScratch() = default;
    DeviceScratch(const DeviceScratch&) = delete;
    template <class T>
    hipError_t malloc(T** p, size_t bytes) {
        blocks.push_back(nullptr);                     // (first, so that a block is never without its entry)
        const hipError_t e = hipMalloc(&blocks.back(), bytes);
        *p = static_cast<T*>(blocks.back());
        return e;
    }
    hipError_t create_events() {
        const hipError_t e = hipEventCreate(&e0);
        return e != hipSuccess ? e : hipEventCreate(&e1);
    }
    ~DeviceScratch() {
        for (void* p : blocks) (void)hipFree(p);
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
    }
};

// The structured priors of a call, checked and derived by prior_of: `table` points into the vectors (or is empty)
struct PriorHost {
    std::vector<int32_t> kind;
    std::vector<double> loc, scale, c0;
    mcd::PriorTable table;
};

// ---- helpers that cross units (the comments are at the definitions) ----
// mcd_api_ctx.hip
int ctx_fail(mcd_ctx* ctx, const std::string& what);
int ctx_usable(mcd_ctx* ctx);
int wait_ctx_stream(mcd_ctx* ctx, hipStream_t s, int64_t spin_us, const char* stage);
// mcd_api_catalog.hip
int build_workset(mcd_catalog* cat, Shard& sh, int64_t n_walkers, WorkSet** out);
LaunchShape main_launch_shape(mcd_catalog* cat, const Shard& sh, const WorkSet& w, int level, bool coll, double* out_buf,
                              int64_t n_out);
const double* fast_pset_const(const mcd_catalog* cat, const Shard& sh, int level);
const void* main_records(const Shard& sh, const WorkSet& w);
int64_t series_chunk_count(const mcd_catalog* cat, const WorkSet& w, int level, const double* params, int64_t n_rows);
int64_t direct_chunk_count(const mcd_catalog* cat, const WorkSet& w, int level, const double* params, int64_t n_rows);
int64_t quad_chunk_count(const mcd_catalog* cat, const WorkSet& w, int level, const double* params, int64_t n_rows);
// mcd_api_chain.hip
int prior_of(const mcd_prior_desc* p, int32_t n_dim, const char* who, PriorHost& out);
void big_copy(void* dst, const void* src, size_t bytes);
// mcd_api_eval.hip
int fast_level(const mcd_catalog* cat, const double* params, int64_t n_rows);
int sync_all(mcd_catalog* cat);
// mcd_api_holdout.hip
void release_holdout(mcd_catalog* cat);
int holdout_device_plan(mcd_catalog* cat, const std::vector<int64_t>& ranges, int64_t n_rows, HoldoutWork** out);
int holdout_device_eval(mcd_catalog* cat, HoldoutWork& w, int64_t n_walkers, const int64_t* d_set_range);
// mcd_api_weighted.hip
void release_weighted(mcd_catalog* cat);
void free_weighted_work(WeightedWork& w);
int weighted_work(mcd_catalog* cat, std::map<int64_t, WeightedWork>& cache, size_t fields, const Shard& sh, int64_t n_rows,
                  WeightedWork** out);
int weighted_finish(mcd_catalog* cat, const std::string& name, WeightedWork& w, int64_t n_rows);
// mcd_api_simulated.hip
void release_simulated(mcd_catalog* cat, bool keep_set = false);

MCD_HOST_END

struct mcd_ctx {
    std::vector<mcd::host::DeviceSlot> slots;
    int rank = 0;
    int n_ranks = 1;
    bool multi_process = false;
    bool force_collective = false;     // MCD_FORCE_RCCL=1: run the all-reduce even on a 1-rank communicator (tests)
    // collective deadline (include/mcd.h): waits on streams that carry an all-reduce poll, bounded by the deadline and
    // by the abort flag another host thread may raise
    int64_t collective_timeout_ms = 120000;
    std::atomic<int> abort_flag{0};
    std::atomic<int> failed{0};
    std::mutex note_mutex;
    std::string abort_reason;          // (guarded by note_mutex)
    std::string failure;               // first failure: stage and cause
    bool has_comm() const { return n_ranks > 1 || slots.size() > 1 || force_collective; }
};

struct mcd_catalog {
    mcd_ctx* ctx = nullptr;
    int model = 0;
    bool free_centre = false;
    int precision = 0;
    int k = 4;
    int64_t n_stars = 0;               // stars held by this process
    int64_t n_psets = 1;
    std::vector<int64_t> bin_offsets;  // [n_psets + 1], indices into this process' stars
    std::vector<mcd::host::Shard> shards;
    mcd::CatalogStats stats;           // range statistics for the fast-path guard (mcd_guard.h)
    // options
    bool timing = false;
    bool timing_all = false;           // keep an event pair for every launch (measurement harness)
    int allow_fast = 1;                // option "fast_path": 0 plain kernels only, 1 guard decides, 2 guard decides but never the narrow variant
    bool zero_copy = true;             // blocking call reads params / writes results through mapped pinned memory
    int64_t timing_stride = 1;         // "timing" = 2: event pair on every n-th launch only (option "timing_stride")
    int64_t timing_launches = 0;
    int64_t spin_us = 20000;           // option "spin_us": poll a stream this long before blocking in hipStreamSynchronize
    int tail_split = 1;                // guided chunk schedule (shorter chunks at the end of a launch)
    int64_t target_waves = 10240;      // see mcd_chunks.h: plan_chunks
    int64_t chunk_len = 0;             // option "chunk_len": explicit nominal chunk length (0: from target_waves)
    int prefetch = -1;                 // option "prefetch": -1 by record volume (>= 8 MiB per device), 0 off, 1 on
    int narrow_bounded = 1;            // option "narrow_bounded": 1 the bounded narrow-range BGFIXED loop where the guard
                                       // admits it (mcd_guard.h: bounded_rescale), 0 never
    int verr_sorted = -1;              // option "verr_sorted": the main kernel reads a verr-sorted copy of the records (f64
                                       // MODEL_BGFIXED, fixed centre, one parameter set): -1 from 8 MiB of records per device, 0 never, 1 always
    int root_series = 1;               // option "root_series": 1 the series root on the sorted records' narrow chunks, 0 never
    int exp_split = 1;                 // option "exp_split": 1 the direct chunks run with the split exponent offset where the
                                       // guard admits it (mcd_guard.h: exp_split_admitted), 0 never
    int root_direct = 1;               // option "root_direct": 1 the direct form of the series where a chunk admits it, 0 the
                                       // delta form on every series chunk
    int root_quad = 1;                 // option "root_quad": 1 the quadratic form on 32-star bands where a direct chunk of a
                                       // launch with the split exponent offset admits it (mcd_math.h: RootQuad), 0 never
    int block_step = 1;                // option "block_step": 1 the bounded quadratic loop takes one block step per 32-star band
                                       // (fold, rescale and prefetch together) where the guard admits it, 0 never
    int balance = -1;                  // option "balance": one round of equal waves (mcd_chunks.h): -1 when the catalogue is
                                       // small enough, 0 never, m > 0 forced with m workgroups per CU
    int two_lanes = 1;                 // option "two_lanes": pipelined evaluations of one device alternate between two streams
    int f32_domain = 1;                // option "f32_domain": 1 calls outside the float32 accuracy domain (mcd_guard.h) are refused
                                       // with MCD_ERR_INVALID, 0 they are evaluated anyway (mcd_last_f32_domain tells)
    mcd::F32Domain last_f32;           // verdict on the last staged parameter table (float32 catalogues)
    // ... and over every table staged since creation (mcd_f32_outside): a library block stages many per call
    int64_t f32_outside_calls = 0;     // tables staged outside the domain (evaluated or refused)
    double f32_worst_kappa_v = 0.0, f32_worst_kappa_theta = 0.0;      // largest condition numbers of any staged table
    const char* f32_outside_reason = "";                              // reason of the last table outside
    int64_t posterior_pass = 65536;    // option "posterior_pass": samples per device pass of mcd_pointwise_posterior
    int64_t replicate_row0 = 0;        // option "replicate_row0": generator row index of the first sample row of mcd_replicate_check
    int64_t loo_scratch_mb = 2048;    // option "loo_scratch_mb": device scratch of mcd_psis_loo (sample table + term tile)
    int combine = 1;                   // option "combine": balanced plans may use 8- / 16-wave workgroups that combine their
                                       // chunks' sums: 0 never, 1 the largest the plan allows, 8 / 16 at most that many waves
    // state of the last evaluation
    int64_t cur_walkers = 0;
    double last_kernel_ms = -1.0, last_device_ms = -1.0;
    bool timing_pending = false;
    int64_t last_grid = 0, last_chunks = 0;
    uint64_t launch_seq = 0;           // source of launch tags
    int64_t n_reruns = 0;              // batches re-evaluated with the plain kernels (denormal regime of the reference)
    // resident stretch-move chain (mcd_stretch.hip)
    int device_chain = 1;              // option "device_chain": 0 host-driven blocks only
    int fused_reduce = 1;              // option "fused_reduce": the step kernel adds up small launches' partial sums itself
    int defer_guard = 1;               // option "defer_guard": one-ensemble resident blocks judge their tables at the end
    bool chain_last_fused = false;
    mcd::host::ChainArena chain;
    int chain_hint = -1;               // kernel family the device's guard asked for when it last disagreed (-1: none)
    int64_t chain_backoff = 0;         // blocks left to run host-driven after a discarded block
    int chain_consecutive = 0;         // discarded blocks in a row (the back-off doubles with each)
    int64_t chain_device_blocks = 0, chain_host_blocks = 0, chain_discarded = 0;
    int chain_last_status = 0;         // status word of the last discarded block (mcd::ChainStatus bits)
    std::vector<hipEvent_t> chain_events;   // large blocks: parts joined by events (stretch_block_device)
    // resident differential-evolution chain (mcd_de.hip, mcd_api_de.hip): counted apart from the stretch blocks; it shares
    // the arena `chain` (a block of either move fills it anew) and the options "device_chain" and "fast_path"
    int de_hint = -1;                  // kernel family the device's guard asked for when it last disagreed (-1: none)
    int64_t de_backoff = 0;            // blocks left to run host-driven after a discarded block
    int de_consecutive = 0;            // discarded blocks in a row (the back-off doubles with each)
    int64_t de_device_blocks = 0, de_host_blocks = 0, de_discarded = 0;
    int de_last_status = 0;            // status word of the last discarded block (mcd::ChainStatus bits)
    // Hamiltonian Monte Carlo blocks (mcd_hmc_block): trajectory state and chain rows of the resident block, its pinned mirror
    mcd::host::ChainArena hmc;
    int64_t hmc_device_blocks = 0, hmc_host_blocks = 0;
    // parallel-tempering blocks (mcd_temper_block): state, numbers, scratch and rows of the resident block, its pinned mirror
    mcd::host::ChainArena temper;
    int64_t temper_device_blocks = 0, temper_host_blocks = 0;
    // exact leave-out refits (mcd_holdout_loglike): plans and buffers per (set_offsets, E W), released with the catalogue
    std::map<std::pair<std::vector<int64_t>, int64_t>, mcd::host::HoldoutWork> holdout;
    // weighted evaluations (mcd_weighted_loglike_grad): plan and buffers per row count, and the transposed explicit weights
    // of the last call ([n_stars][n_replicates], grown as needed) with the fingerprint of their contents (-1 replicates:
    // none), released with the catalogue
    std::map<int64_t, mcd::host::WeightedWork> weighted;
    std::map<int64_t, mcd::host::WeightedWork> weighted_value;   // mcd_weighted_loglike's, a cache of its own
    double* d_weights = nullptr;
    size_t d_weights_bytes = 0;
    int64_t weights_replicates = -1;
    uint64_t weights_print[2] = {0, 0};
    // simulated catalogues (mcd_simulate, mcd_simulated_set): the resident velocity table [n_stars][n_sims] (grown as needed;
    // sim_count 0: no set is resident) with the fixed-background models' (mean, sigma^2), and mcd_simulated_loglike's plan
    // and buffers per row count (d_replicate holds row_sim), released with the catalogue
    double* d_sim = nullptr;
    size_t d_sim_bytes = 0;
    int64_t sim_count = 0;
    double sim_bg_mean = 0.0, sim_bg_sigma2 = 0.0;
    std::map<int64_t, mcd::host::WeightedWork> simulated;
    std::map<int64_t, mcd::host::WeightedWork> simulated_grad;   // mcd_simulated_loglike_grad's, 1 + K fields per row
    int last_prefetch = -1;            // the last main-kernel launch used the prefetching instantiation (-1: none yet)
    int64_t last_series_chunks = -1;   // chunks of the last main-kernel launch that took the series root (host count), -1: no launch yet
    int64_t last_direct_chunks = -1;   // ... of which in the direct form (host count), -1: no launch yet
    int last_exp_split = -1;           // 1: the direct chunks of the last main-kernel launch ran with the split exponent offset,
                                       // 0 not (-1: no launch yet)
    int last_root_quad = -1;           // 1: the last main-kernel launch held the third vote (option "root_quad" on a launch with
                                       // the split exponent offset), 0 not (-1: no launch yet)
    int last_block_step = -1;          // 1: the last main-kernel launch ran the block-step kernel (option "block_step" on a
                                       // bounded launch with R = 32 that holds the third vote), 0 not (-1: no launch yet)
    int64_t last_quad_chunks = -1;     // chunks of that launch in the quadratic form (host count), -1: no launch yet
    int last_narrow_bounded = -1;      // R of the bounded narrow-range loop the last main-kernel launch ran, 0 none (-1: no launch yet)
};

#define MCD_WAIT(ctx, stream, spin, stage)                                                              \
    do {                                                                                                \
        const int w_rc_ = ::mcd::host::wait_ctx_stream((ctx), (stream), (spin), (stage));               \
        if (w_rc_ != MCD_OK) return w_rc_;                                                              \
    } while (0)

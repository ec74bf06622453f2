// mcd_api_eval.hip -- C-ABI of the MI355X log-likelihood library (see include/mcd.h; mcd_host.h lists the host units):
// the per-call launch sequence
//   params H2D -> walker prep -> main kernel -> fixed-order reduce -> [RCCL all-reduce] -> D2H,
// blocking and pipelined, with its HIP-event timing, the per-star outputs of one parameter row, and the same sequence
// for the value-and-gradient kernel (mcd_loglike_grad_batch).
#include "mcd_host.h"
#include "mcd_grad.h"

using namespace mcd::host;

MCD_HOST_BEGIN

int fast_level(const mcd_catalog* cat, const double* params, int64_t n_rows) {
    if (!cat->allow_fast) return 0;
    const int level = mcd::fast_level(cat->stats, cat->model, cat->free_centre, cat->precision != MCD_F64, cat->k, params, n_rows);
    return cat->allow_fast == 2 && level > 1 ? 1 : level;
}

int sync_all(mcd_catalog* cat) {
    if (!cat) return fail(MCD_ERR_INVALID, "null catalogue");
    if (int rc = ctx_usable(cat->ctx)) return rc;
    for (Shard& sh : cat->shards) {
        const DeviceSlot& slot = cat->ctx->slots[sh.slot];
        MCD_HIP(hipSetDevice(slot.device));
        MCD_WAIT(cat->ctx, slot.stream, cat->spin_us, "mcd_sync / mcd_loglike_fetch (compute stream)");
        MCD_WAIT(cat->ctx, slot.stream2, cat->spin_us, "mcd_sync / mcd_loglike_fetch (second compute lane)");
        MCD_WAIT(cat->ctx, slot.comm_stream, cat->spin_us, "mcd_sync / mcd_loglike_fetch (communication stream)");
    }
    if (cat->timing && cat->timing_pending) {
        Shard& sh = cat->shards[0];
        float k_ms = 0.f, d_ms = 0.f;
        if (cat->timing_all) {
            if (sh.ring_used > 0)          // (none yet when only unsampled launches ran since the last collect)
                MCD_HIP(hipEventElapsedTime(&k_ms, sh.ring[sh.ring_used - 1].first, sh.ring[sh.ring_used - 1].second));
        } else {
            MCD_HIP(hipEventElapsedTime(&k_ms, sh.ev_k0, sh.ev_k1));
        }
        if (!cat->timing_all) MCD_HIP(hipEventElapsedTime(&d_ms, sh.ev_begin, sh.ev_end));
        cat->last_kernel_ms = k_ms;
        cat->last_device_ms = cat->timing_all ? -1.0 : d_ms;
        cat->timing_pending = false;
    }
    return MCD_OK;
}

MCD_HOST_END

namespace {

// Work buffers staged for walker count W (nullptr when the cache no longer holds them, e.g. after a failed upload)
WorkSet* find_work(Shard& sh, int64_t W) {
    const auto it = sh.work.find(W);
    return it == sh.work.end() ? nullptr : &it->second;
}

bool all_staged(mcd_catalog* cat) {
    if (cat->cur_walkers <= 0) return false;
    for (Shard& sh : cat->shards) {
        const WorkSet* w = find_work(sh, cat->cur_walkers);
        if (!w || !w->staged) return false;
    }
    return true;
}

int stage_params_impl(mcd_catalog* cat, int64_t n_walkers, int32_t k, const double* params, bool zero_copy) {
    if (!cat || !params) return fail(MCD_ERR_INVALID, "null catalogue or params");
    if (int rc = ctx_usable(cat->ctx)) return rc;
    if (n_walkers <= 0) return fail(MCD_ERR_INVALID, "n_walkers must be positive");
    if (k != cat->k) {
        char buf[128];
        snprintf(buf, sizeof buf, "parameter table has %d columns, catalogue expects %d", (int)k, cat->k);
        return fail(MCD_ERR_INVALID, buf);
    }
    const int64_t n_rows = cat->n_psets * n_walkers;
    if (cat->precision != MCD_F64) {
        // float32 catalogues: is this table inside the domain in which float32 keeps the stated tolerances?
        cat->last_f32 = mcd::f32_domain(cat->stats, cat->model, cat->free_centre, cat->k, params, n_rows);
        if (cat->last_f32.kappa_v > cat->f32_worst_kappa_v) cat->f32_worst_kappa_v = cat->last_f32.kappa_v;
        if (cat->last_f32.kappa_theta > cat->f32_worst_kappa_theta) cat->f32_worst_kappa_theta = cat->last_f32.kappa_theta;
        if (!cat->last_f32.inside) {
            ++cat->f32_outside_calls;
            cat->f32_outside_reason = cat->last_f32.reason;
        }
        if (!cat->last_f32.inside && cat->f32_domain)
            return fail(MCD_ERR_INVALID, std::string("outside the float32 accuracy domain (use an MCD_F64 catalogue, or option "
                                                     "f32_domain = 0 to evaluate regardless): ") + cat->last_f32.reason);
    }
    const int fast = fast_level(cat, params, n_rows);
    const int narrow_rescale = fast == 2 && cat->precision == MCD_F64
                                   ? mcd::bounded_rescale(cat->stats, cat->model, cat->free_centre, cat->k, params, n_rows) : 0;
    for (Shard& sh : cat->shards) {
        WorkSet* w = nullptr;
        int rc = build_workset(cat, sh, n_walkers, &w);
        if (rc != MCD_OK) return rc;
        const DeviceSlot& slot = cat->ctx->slots[sh.slot];
        MCD_HIP(hipSetDevice(slot.device));
        // the pinned staging buffer (and, on lane 1, the walker constants) may still be in flight from the previous call
        MCD_WAIT(cat->ctx, slot.stream, cat->spin_us, "mcd_params_upload (previous evaluation)");
        if (w->lane1_used) {
            MCD_WAIT(cat->ctx, slot.stream2, cat->spin_us, "mcd_params_upload (previous evaluation, second lane)");
            w->lane1_used = false;
        }
        std::memcpy(w->h_params, params, (size_t)n_rows * k * sizeof(double));
        // Blocking single-device call: the walker-prep kernel reads the pinned host table over PCIe and the reduce
        // kernel writes the results straight into pinned host memory -- no copy-engine operations on the critical
        // path.  The pipelined API and multi-device contexts keep device-resident tables.
        w->mapped = zero_copy;
        const double* src = w->m_params;
        if (!zero_copy) {
            MCD_HIP(hipMemcpyAsync(w->d_params, w->h_params, (size_t)n_rows * k * sizeof(double), hipMemcpyHostToDevice,
                                   slot.stream));
            src = w->d_params;
        }
        MCD_HIP(mcd::launch_prepare_walkers(slot.stream, src, n_rows, k, cat->model, cat->free_centre,
                                            cat->precision, w->d_wpar));
        MCD_HIP(hipEventRecord(w->ev_staged, slot.stream));
        w->lane1_knows_staging = false;
        w->fast = fast;
        w->narrow_rescale = narrow_rescale;
        for (int b = 0; b < 2; ++b)
            w->exp_split[b] = fast == 2 && cat->precision == MCD_F64 && (b == 0 || narrow_rescale != 0) &&
                              mcd::exp_split_admitted(cat->stats, cat->model, cat->free_centre, cat->k, params, n_rows,
                                                      b ? narrow_rescale : 0);
        w->block_step = w->exp_split[1] && narrow_rescale == 32 &&
                        mcd::block_step_admitted(cat->stats, cat->model, cat->free_centre, cat->k, params, n_rows);
        w->series_chunks = series_chunk_count(cat, *w, fast, params, n_rows);
        w->direct_chunks = direct_chunk_count(cat, *w, fast, params, n_rows);
        w->quad_chunks = quad_chunk_count(cat, *w, fast, params, n_rows);
        w->staged = true;
    }
    cat->cur_walkers = n_walkers;
    return MCD_OK;
}

// A failed upload leaves nothing staged: a later enqueue / fetch answers MCD_ERR_INVALID instead of working on buffers
// that may have been evicted.
int stage_params(mcd_catalog* cat, int64_t n_walkers, int32_t k, const double* params, bool zero_copy) {
    const int rc = stage_params_impl(cat, n_walkers, k, params, zero_copy);
    if (rc != MCD_OK && cat) cat->cur_walkers = 0;
    return rc;
}

// The event pair that brackets a shard's main kernel: the shard's own pair, or with per-launch timing ("timing" = 2) and a
// sampled launch the next pair of its ring (grown on demand).
int timing_pair(const mcd_catalog* cat, Shard& sh, bool sampled, hipEvent_t* k0, hipEvent_t* k1) {
    *k0 = sh.ev_k0;
    *k1 = sh.ev_k1;
    if (!(cat->timing_all && sampled)) return MCD_OK;
    if (sh.ring_used >= (size_t)1 << 16) sh.ring_used = 0;        // harness option left on: recycle, never grow without bound
    if (sh.ring_used == sh.ring.size()) {
        hipEvent_t a, b;
        MCD_HIP(hipEventCreate(&a));
        MCD_HIP(hipEventCreate(&b));
        sh.ring.emplace_back(a, b);
    }
    *k0 = sh.ring[sh.ring_used].first;
    *k1 = sh.ring[sh.ring_used].second;
    ++sh.ring_used;
    return MCD_OK;
}

// End of a timed launch sequence: the outer event of every shard, and the timing left for sync_all to collect
int timing_end(mcd_catalog* cat) {
    if (cat->timing_all) ++cat->timing_launches;
    if (!cat->timing) return MCD_OK;
    if (!cat->timing_all) {
        for (Shard& sh : cat->shards) {
            const DeviceSlot& slot = cat->ctx->slots[sh.slot];
            MCD_HIP(hipSetDevice(slot.device));
            MCD_HIP(hipEventRecord(sh.ev_end, slot.stream));
        }
    }
    cat->timing_pending = true;
    return MCD_OK;
}

// pipelined (mcd_loglike_enqueue): the all-reduce goes to the communication stream and overlaps the next step's kernels.
// A blocking call gains nothing from that hop: its all-reduce stays on the compute stream (after any collective still
// pending on the communication stream, so that operations on one communicator never run concurrently).
int enqueue(mcd_catalog* cat, bool pipelined) {
    if (!cat) return fail(MCD_ERR_INVALID, "null catalogue");
    if (int rc = ctx_usable(cat->ctx)) return rc;
    if (cat->cur_walkers <= 0) return fail(MCD_ERR_INVALID, "no parameters staged (call mcd_params_upload first)");
    if (!all_staged(cat)) return fail(MCD_ERR_INVALID, "no parameters staged for this walker count (the last upload failed?)");
    const int64_t W = cat->cur_walkers;
    const int64_t n_out = cat->n_psets * W;
    mcd_ctx* ctx = cat->ctx;
    for (Shard& sh : cat->shards) {
        WorkSet& w = (*find_work(sh, W));
        const DeviceSlot& slot = ctx->slots[sh.slot];
        MCD_HIP(hipSetDevice(slot.device));
        const bool coll = ctx->has_comm();
        double* out_buf = w.mapped ? w.m_out : w.d_out;
        // two lanes: see WorkSet.  (Not with per-launch timing of the harness' plain mode, whose begin / end events
        // bracket ONE stream; the sampled per-kernel events of "timing" = 2 are recorded on the lane's stream.)
        const bool two_lanes = pipelined && cat->two_lanes && !(cat->timing && !cat->timing_all);
        hipStream_t lane_stream = slot.stream;
        double* lane_partials = w.d_partials;
        if (coll || two_lanes) {
            // alternate result buffers (and, with two lanes, streams and partial-sum buffers).  With a collective this step
            // may only overwrite its buffer once the all-reduce that last used it (two steps ago, on the communication
            // stream) has finished; the all-reduces themselves stay in order on that one stream.
            w.buf ^= 1;
            out_buf = w.buf ? w.d_out2 : w.d_out;
            if (two_lanes && w.buf) {
                if (!w.d_partials2) {
                    MCD_HIP(hipMalloc(&w.d_partials2, std::max<size_t>(1, (size_t)mcd::padded_walkers(W) * w.n_chunks) * sizeof(double)));
                }
                if (!w.lane1_knows_staging) {
                    MCD_HIP(hipStreamWaitEvent(slot.stream2, w.ev_staged, 0));
                    w.lane1_knows_staging = true;
                }
                lane_stream = slot.stream2;
                lane_partials = w.d_partials2;
                w.lane1_used = true;
            }
        } else {
            w.buf = 0;
        }
        mcd::LaunchShape shape = main_launch_shape(cat, sh, w, w.fast, coll, out_buf, n_out);
        shape.narrow_rescale = cat->narrow_bounded ? w.narrow_rescale : 0;
        cat->last_narrow_bounded = mcd::narrow_bounded_launch(shape) ? shape.narrow_rescale : 0;
        // the direct chunks with the split exponent offset (option "exp_split"), where the guard admits it for the loop
        // this launch runs; refused: the direct form as it is
        if (cat->exp_split && w.sorted && w.d_split_const && w.exp_split[cat->last_narrow_bounded ? 1 : 0]) {
            shape.records_split = sh.records_split;
            shape.split_const = w.d_split_const;
        }
        cat->last_exp_split = mcd::exp_split_launch(shape) ? 1 : 0;
        cat->last_root_quad = mcd::root_quad_launch(shape) ? 1 : 0;
        shape.block_step = cat->block_step != 0 && w.block_step && mcd::block_step_fits_l2(w.n_chunks, W);
        cat->last_block_step = mcd::block_step_launch(shape) ? 1 : 0;
        if (&sh == &cat->shards.front()) cat->last_series_chunks = cat->last_direct_chunks = cat->last_quad_chunks = 0;
        cat->last_quad_chunks += cat->last_root_quad && shape.fast == 2 ? w.quad_chunks : 0;
        cat->last_series_chunks += shape.root_series && shape.fast == 2 ? w.series_chunks : 0;
        cat->last_direct_chunks += shape.root_direct && shape.fast == 2 ? w.direct_chunks : 0;
        w.launch_tag = coll ? 0.0 : (double)(++cat->launch_seq);
        shape.launch_tag = w.launch_tag;
        // per-launch events cost a signal packet each (~3 us per pair between back-to-back kernels): a harness may sample
        const bool sampled = !cat->timing_all || (cat->timing_launches % cat->timing_stride) == 0;
        hipEvent_t k0, k1;
        if (int rc = timing_pair(cat, sh, sampled, &k0, &k1)) return rc;
        if (cat->timing && !cat->timing_all) MCD_HIP(hipEventRecord(sh.ev_begin, slot.stream));
        if (cat->timing && sampled) MCD_HIP(hipEventRecord(k0, lane_stream));
        MCD_HIP(mcd::launch_loglike(lane_stream, shape, main_records(sh, w), w.d_chunks, w.n_chunks, w.d_wpar, lane_partials, W));
        if (cat->timing && sampled) MCD_HIP(hipEventRecord(k1, lane_stream));
        const double* pset_const = fast_pset_const(cat, sh, w.fast);
        // With a collective this step may only overwrite its result buffer once the all-reduce that last used it has
        // finished.  Only the REDUCTION writes that buffer (the main kernel's re-run signal travels in the partial sums
        // here), so the wait sits in front of it, not in front of the main kernel: with two lanes a lane reuses the buffer
        // of its own previous step, and the all-reduce of that step would otherwise be on the lane's critical path.
        if (coll && w.comm_pending[w.buf]) {
            MCD_HIP(hipStreamWaitEvent(lane_stream, w.ev_comm[w.buf], 0));
            w.comm_pending[w.buf] = false;
        }
        {
            const int64_t n_slots = mcd::partial_slots(shape, w.n_chunks, W);
            MCD_HIP(mcd::launch_reduce(lane_stream, lane_partials, w.d_offsets, cat->n_psets, n_slots,
                                       cat->n_psets == 1 ? n_slots : w.max_chunks_per_pset, W, pset_const, out_buf));
        }
        if (coll && pipelined) MCD_HIP(hipEventRecord(w.ev_reduced[w.buf], lane_stream));
    }
    // sum the per-device / per-rank partial log-likelihoods: one all-reduce of n_out doubles
    if (ctx->has_comm()) {
        if (!ctx->multi_process) MCD_NCCL(g_rccl.GroupStart());
        for (Shard& sh : cat->shards) {
            WorkSet& w = (*find_work(sh, W));
            const DeviceSlot& slot = ctx->slots[sh.slot];
            MCD_HIP(hipSetDevice(slot.device));
            double* buf = w.buf ? w.d_out2 : w.d_out;
            if (pipelined) {
                MCD_HIP(hipStreamWaitEvent(slot.comm_stream, w.ev_reduced[w.buf], 0));
                MCD_NCCL(g_rccl.AllReduce(buf, buf, (size_t)n_out, ncclDouble, ncclSum, slot.comm, slot.comm_stream));
            } else {
                if (w.comm_pending[w.buf ^ 1]) {           // the newest collective still on the communication stream
                    MCD_HIP(hipStreamWaitEvent(slot.stream, w.ev_comm[w.buf ^ 1], 0));
                    w.comm_pending[w.buf ^ 1] = false;
                }
                MCD_NCCL(g_rccl.AllReduce(buf, buf, (size_t)n_out, ncclDouble, ncclSum, slot.comm, slot.stream));
            }
        }
        if (!ctx->multi_process) MCD_NCCL(g_rccl.GroupEnd());
        if (pipelined) {
            for (Shard& sh : cat->shards) {
                WorkSet& w = (*find_work(sh, W));
                const DeviceSlot& slot = ctx->slots[sh.slot];
                MCD_HIP(hipSetDevice(slot.device));
                MCD_HIP(hipEventRecord(w.ev_comm[w.buf], slot.comm_stream));
                w.comm_pending[w.buf] = true;
            }
        }
    }
    if (int rc = timing_end(cat)) return rc;
    {
        WorkSet& w0 = (*find_work(cat->shards[0], W));
        cat->last_chunks = w0.n_chunks;
        mcd::LaunchShape sh0{cat->model, cat->free_centre, cat->precision, w0.fast};
        sh0.waves = w0.waves;
        const int64_t slots = mcd::partial_slots(sh0, w0.n_chunks, W);
        cat->last_grid = slots != w0.n_chunks ? slots : mcd::main_grid(w0.n_chunks, W);
    }
    return MCD_OK;
}

int fetch_once(mcd_catalog* cat, bool* rerun) {
    const int64_t W = cat->cur_walkers;
    const int64_t n_out = cat->n_psets * W;
    *rerun = false;
    const bool coll = cat->ctx->has_comm();
    bool any_fast = false;
    for (Shard& sh : cat->shards) {
        WorkSet& w = (*find_work(sh, W));
        any_fast = any_fast || w.fast != 0;
        const DeviceSlot& slot = cat->ctx->slots[sh.slot];
        MCD_HIP(hipSetDevice(slot.device));
        // after the all-reduce every device holds the same results: only the first shard's are copied
        if (!w.mapped && &sh == &cat->shards[0]) {
            const double* res = w.buf ? w.d_out2 : w.d_out;
            if (w.comm_pending[w.buf]) MCD_HIP(hipStreamWaitEvent(slot.stream, w.ev_comm[w.buf], 0));
            // (single device, two lanes: the newest results sit behind the work of the lane that produced them)
            hipStream_t copy_stream = (!coll && w.buf && w.lane1_used) ? slot.stream2 : slot.stream;
            MCD_HIP(hipMemcpyAsync(w.h_out, res, (size_t)(n_out + 1) * sizeof(double), hipMemcpyDeviceToHost, copy_stream));
        }
    }
    int rc = sync_all(cat);
    if (rc != MCD_OK) return rc;
    const WorkSet& w0 = (*find_work(cat->shards[0], W));
    if (coll) {
        // Every rank decides on the all-reduced values alone (identical everywhere), whatever kernel family it ran itself:
        // the re-evaluation is collective.  (A NaN that the plain kernels produce legitimately costs one extra pass.)
        for (int64_t i = 0; i < n_out && !*rerun; ++i) *rerun = w0.h_out[i] != w0.h_out[i];      // NaN-poisoned sums
    } else if (any_fast) {
        *rerun = w0.h_out[n_out] == w0.launch_tag;
    }
    return MCD_OK;
}

int fetch(mcd_catalog* cat, double* out) {
    if (!cat || !out) return fail(MCD_ERR_INVALID, "null catalogue or output");
    if (cat->cur_walkers <= 0 || !all_staged(cat)) return fail(MCD_ERR_INVALID, "nothing evaluated yet");
    const int64_t W = cat->cur_walkers;
    const int64_t n_out = cat->n_psets * W;
    bool rerun = false;
    int rc = fetch_once(cat, &rerun);
    if (rc != MCD_OK) return rc;
    if (rerun) {
        // A fast mixture kernel met the regime where the reference's log-sum-exp runs on denormal numbers (a star with
        // pmember == 1, f_back == 0 or density == 0 that is a > 37 sigma outlier of the remaining component).  Only the
        // plain kernels reproduce the reference's value there: evaluate the staged batch again with them.  In a
        // multi-rank job every rank takes the same decision (the all-reduce is collective): the affected partial sums
        // are NaN-poisoned by the kernel, so the all-reduced results carry the signal to every rank (fetch_once).
        ++cat->n_reruns;
        for (Shard& sh : cat->shards) (*find_work(sh, W)).fast = 0;
        rc = enqueue(cat, false);
        if (rc != MCD_OK) return rc;
        rc = fetch_once(cat, &rerun);
        if (rc != MCD_OK) return rc;
    }
    std::memcpy(out, (*find_work(cat->shards[0], W)).h_out, (size_t)n_out * sizeof(double));
    return MCD_OK;
}

int per_star(mcd_catalog* cat, int32_t k, const double* params, int mode, double* out) {
    if (!cat || !params || !out) return fail(MCD_ERR_INVALID, "per-star output: null argument");
    if (mcd::bg_kind(cat->model) == mcd::BG_NONE) return fail(MCD_ERR_INVALID, "per-star outputs need a background model");
    if (cat->n_psets != 1) return fail(MCD_ERR_INVALID, "per-star outputs are defined for un-binned catalogues");
    if (k != cat->k) return fail(MCD_ERR_INVALID, "parameter row has the wrong number of columns");
    const size_t term_bytes = cat->precision == MCD_F64 ? 8 : 4;
    for (Shard& sh : cat->shards) {
        if (sh.n == 0) continue;
        const DeviceSlot& slot = cat->ctx->slots[sh.slot];
        MCD_HIP(hipSetDevice(slot.device));
        double* d_p = nullptr; void* d_w = nullptr; double* d_o = nullptr;
        MCD_HIP(hipMalloc(&d_p, k * sizeof(double)));
        MCD_HIP(hipMalloc(&d_w, mcd::KD * term_bytes));
        MCD_HIP(hipMalloc(&d_o, (size_t)sh.n * sizeof(double)));
        MCD_HIP(hipMemcpyAsync(d_p, params, k * sizeof(double), hipMemcpyHostToDevice, slot.stream));
        MCD_HIP(mcd::launch_prepare_walkers(slot.stream, d_p, 1, k, cat->model, cat->free_centre, cat->precision, d_w));
        mcd::LaunchShape shape{cat->model, cat->free_centre, cat->precision, 0};
        MCD_HIP(mcd::launch_per_star(slot.stream, shape, sh.records, sh.n, d_w, mode, d_o));
        MCD_HIP(hipMemcpyAsync(out + sh.star_begin, d_o, (size_t)sh.n * sizeof(double), hipMemcpyDeviceToHost, slot.stream));
        MCD_HIP(hipStreamSynchronize(slot.stream));
        MCD_HIP(hipFree(d_p)); MCD_HIP(hipFree(d_w)); MCD_HIP(hipFree(d_o));
    }
    return MCD_OK;
}

// Value and gradient of one parameter table: the staging of the value path (params H2D, walker prep), the gradient kernel
// and the fixed-order reduction of its 1 + K fields on every shard, one all-reduce of the fields where the stars are
// spread over devices or ranks, D2H, and the transposition into the caller's [.][W] and [.][W][K] arrays.
int loglike_grad(mcd_catalog* cat, int64_t n_walkers, int32_t k, const double* params, double* out, double* grad) {
    if (!cat || !params || !grad) return fail(MCD_ERR_INVALID, "mcd_loglike_grad_batch: null catalogue, params or grad");
    if (int rc = ctx_usable(cat->ctx)) return rc;
    if (cat->precision != MCD_F64) return fail(MCD_ERR_INVALID, "gradients need an MCD_F64 catalogue");
    int rc = stage_params(cat, n_walkers, k, params, false);
    if (rc != MCD_OK) return rc;
    mcd_ctx* ctx = cat->ctx;
    const int64_t W = n_walkers;
    const int64_t fields = 1 + k;
    const int64_t padded = mcd::padded_walkers(W);
    const size_t n_res = (size_t)(cat->n_psets * fields * padded);       // doubles of a result buffer
    const bool coll = ctx->has_comm();
    for (Shard& sh : cat->shards) {
        WorkSet& w = (*find_work(sh, W));
        const DeviceSlot& slot = ctx->slots[sh.slot];
        MCD_HIP(hipSetDevice(slot.device));
        // (each buffer on its own: a call that failed half-way leaves what it got for the next one, nothing is allocated twice)
        if (!w.d_grad_partials)
            MCD_HIP(hipMalloc(&w.d_grad_partials, std::max<size_t>(1, (size_t)(fields * padded * w.n_chunks)) * sizeof(double)));
        if (!w.h_grad_out) MCD_HIP(hipHostMalloc(&w.h_grad_out, n_res * sizeof(double), hipHostMallocDefault));
        if (!w.d_grad_out) MCD_HIP(hipMalloc(&w.d_grad_out, n_res * sizeof(double)));
        mcd::LaunchShape shape{cat->model, cat->free_centre, cat->precision, 0};
        hipEvent_t k0, k1;
        if (int rc = timing_pair(cat, sh, true, &k0, &k1)) return rc;      // (a pair on every call, whatever the stride)
        // (timing: as for values, the inner event pair brackets the main kernel alone, the outer one the device sequence)
        if (cat->timing && !cat->timing_all) MCD_HIP(hipEventRecord(sh.ev_begin, slot.stream));
        if (cat->timing) MCD_HIP(hipEventRecord(k0, slot.stream));
        MCD_HIP(mcd::launch_loglike_grad(slot.stream, shape, main_records(sh, w), w.d_chunks, w.n_chunks, w.d_params, w.d_wpar,
                                         w.d_grad_partials, W));
        if (cat->timing) MCD_HIP(hipEventRecord(k1, slot.stream));
        MCD_HIP(mcd::launch_grad_reduce(slot.stream, shape, w.d_grad_partials, w.n_chunks, w.d_offsets, cat->n_psets,
                                        w.max_chunks_per_pset, W, w.d_grad_out));
    }
    if (coll) {
        // sum the shards' fields: one all-reduce of (1 + K) x outputs doubles (rows padded to whole walker tiles), on the
        // compute stream behind any collective still pending on the communication stream
        if (!ctx->multi_process) MCD_NCCL(g_rccl.GroupStart());
        for (Shard& sh : cat->shards) {
            WorkSet& w = (*find_work(sh, W));
            const DeviceSlot& slot = ctx->slots[sh.slot];
            MCD_HIP(hipSetDevice(slot.device));
            for (int b = 0; b < 2; ++b) {
                if (!w.comm_pending[b]) continue;
                MCD_HIP(hipStreamWaitEvent(slot.stream, w.ev_comm[b], 0));
                w.comm_pending[b] = false;
            }
            MCD_NCCL(g_rccl.AllReduce(w.d_grad_out, w.d_grad_out, n_res, ncclDouble, ncclSum, slot.comm, slot.stream));
        }
        if (!ctx->multi_process) MCD_NCCL(g_rccl.GroupEnd());
    }
    {
        // after the all-reduce every device holds the same results: only the first shard's are copied
        Shard& sh = cat->shards[0];
        WorkSet& w = (*find_work(sh, W));
        const DeviceSlot& slot = ctx->slots[sh.slot];
        MCD_HIP(hipSetDevice(slot.device));
        MCD_HIP(hipMemcpyAsync(w.h_grad_out, w.d_grad_out, n_res * sizeof(double), hipMemcpyDeviceToHost, slot.stream));
    }
    rc = timing_end(cat);
    if (rc != MCD_OK) return rc;
    rc = sync_all(cat);                       // (waits under the collective deadline, collects the timing)
    if (rc != MCD_OK) return rc;
    const double* res = (*find_work(cat->shards[0], W)).h_grad_out;
    for (int64_t b = 0; b < cat->n_psets; ++b) {
        const double* block = res + b * fields * padded;
        if (out) std::memcpy(out + b * W, block, (size_t)W * sizeof(double));
        for (int64_t j = 0; j < k; ++j) {
            const double* col = block + (1 + j) * padded;
            for (int64_t i = 0; i < W; ++i) grad[(b * W + i) * k + j] = col[i];
        }
    }
    return MCD_OK;
}

}  // namespace

extern "C" {

int mcd_loglike_grad_batch(mcd_catalog* cat, int64_t n_walkers, int32_t k, const double* params, double* out, double* grad) {
    try { return loglike_grad(cat, n_walkers, k, params, out, grad); } catch (...) { return on_exception("mcd_loglike_grad_batch"); }
}

int mcd_params_upload(mcd_catalog* cat, int64_t n_walkers, int32_t k, const double* params) {
    try { return stage_params(cat, n_walkers, k, params, false); } catch (...) { return on_exception("mcd_params_upload"); }
}

int mcd_loglike_enqueue(mcd_catalog* cat) {
    try { return enqueue(cat, true); } catch (...) { return on_exception("mcd_loglike_enqueue"); }
}
int mcd_loglike_fetch(mcd_catalog* cat, double* out) {
    try { return fetch(cat, out); } catch (...) { return on_exception("mcd_loglike_fetch"); }
}
int mcd_sync(mcd_catalog* cat) {
    try { return sync_all(cat); } catch (...) { return on_exception("mcd_sync"); }
}

int mcd_loglike_batch(mcd_catalog* cat, int64_t n_walkers, int32_t k, const double* params, double* out) {
    try {
    if (!out) return fail(MCD_ERR_INVALID, "null output");
    const bool collective = cat && cat->ctx->has_comm();
    int rc = stage_params(cat, n_walkers, k, params, !collective && cat && cat->zero_copy);
    if (rc != MCD_OK) return rc;
    rc = enqueue(cat, false);
    if (rc != MCD_OK) return rc;
    return fetch(cat, out);
    } catch (...) { return on_exception("mcd_loglike_batch"); }
}

int mcd_membership(mcd_catalog* cat, int32_t k, const double* params, double* out) {
    try {
    return per_star(cat, k, params, 0, out);
    } catch (...) { return on_exception("mcd_membership"); }
}

int mcd_loglike_per_star(mcd_catalog* cat, int32_t k, const double* params, double* out) {
    try {
    return per_star(cat, k, params, 1, out);
    } catch (...) { return on_exception("mcd_loglike_per_star"); }
}

}  // extern "C"

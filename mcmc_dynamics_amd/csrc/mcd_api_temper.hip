// mcd_api_temper.hip -- C-ABI of the MI355X log-likelihood library (see include/mcd.h; mcd_host.h lists the host units):
// mcd_temper_block / mcd_temper_block_prior as a block resident on the device (kernels: mcd_temper.hip) or driven from the
// host (mcd_temper.h: temper_block around mcd_loglike_batch), mcd_temper_numbers and mcd_temper_info.  Evaluations of a
// tempered block run the plain kernels (guard level 0) in both forms: the hot rungs roam the whole prior box, where the
// fast families' range guard (mcd_guard.h) would refuse often -- and without it the step kernel needs no guard, no re-run
// tag and no discard protocol.
#include "mcd_host.h"
#include "mcd_prior.h"
#include "mcd_rng.h"
#include "mcd_temper.h"

using namespace mcd::host;

namespace {

// What the resident form covers: one shard, no communicator, no timing, option "device_chain" on, an ensemble whose stretch
// numbers the device generates (W <= 8192), and a block whose numbers and rows fit the byte bound.
constexpr size_t kTemperResidentMaxBytes = (size_t)512 << 20;

size_t temper_block_bytes(int64_t T, int64_t W, int P, int64_t n_steps, int32_t n_chain_temps, bool chain, bool lnlike_chain) {
    return (size_t)n_steps * ((size_t)T * W * 24 + (chain ? (size_t)n_chain_temps * W * P * 8 : 0) + (lnlike_chain ? (size_t)T * W * 8 : 0));
}

bool temper_resident_covers(const mcd_catalog* cat, int64_t T, int64_t W, int P, int64_t n_steps, int32_t n_chain_temps,
                            bool chain, bool lnlike_chain) {
    if (!cat->device_chain || cat->shards.size() != 1 || cat->ctx->has_comm() || cat->timing || n_steps < 1) return false;
    if (!mcd::chain_numbers_on_device(W)) return false;
    return temper_block_bytes(T, W, P, n_steps, n_chain_temps, chain, lnlike_chain) <= kTemperResidentMaxBytes;
}

// The block as ONE chain of launches on the shard's stream; the host waits once under the context's deadline.  Per step:
//   step(propose h = 0), walker prep, main kernel, reduction, step(accept 0, propose 1), walker prep, main kernel, reduction,
//   step(accept 1), swap-and-record.
// *done = false (nothing written) when the arena cannot be had: the caller runs the block host-driven.
int temper_block_device(mcd_catalog* cat, const mcd::TemperShared& ts, int64_t n_steps, double* pos, double* ll, double* lp,
                        uint64_t seed, int64_t step0, int32_t n_chain_temps, double* chain, double* lnlike_chain,
                        int64_t* accepted, int64_t* swap_proposed, int64_t* swap_accepted, bool* done) {
    *done = false;
    mcd_ctx* ctx = cat->ctx;
    const int64_t T = ts.n_temps, W = ts.n_walkers, half = W / 2, rows = T * half;
    const int P = ts.n_dim, K = ts.k;
    const size_t TW = (size_t)T * W;
    std::vector<double> lp0(TW);
    if (mcd::temper_start(ts, pos, ll, lp0.data()) != mcd::TEMPER_OK)
        return fail(MCD_ERR_NONFINITE, "mcd_temper_block: a walker starts outside the prior or with a non-finite log-likelihood");
    Shard& sh = cat->shards[0];
    const DeviceSlot& slot = ctx->slots[sh.slot];
    MCD_HIP(hipSetDevice(slot.device));
    WorkSet* wp = nullptr;
    int rc = build_workset(cat, sh, rows, &wp);
    if (rc != MCD_OK) return rc;
    WorkSet& w = *wp;
    // nothing of an earlier call may still use the work buffers or the arena
    MCD_WAIT(cat->ctx, slot.stream, cat->spin_us, "mcd_temper_block (previous evaluation)");
    MCD_WAIT(cat->ctx, slot.stream2, cat->spin_us, "mcd_temper_block (previous evaluation, second lane)");
    MCD_WAIT(cat->ctx, slot.comm_stream, cat->spin_us, "mcd_temper_block (previous collective)");
    w.comm_pending[0] = w.comm_pending[1] = false;

    // ---- arena: [state and counts, both ways | column map, bounds, ladder, priors: in | numbers, scratch | rows: out]
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 63) / 64 * 64; return at; };
    const size_t o_pos = take(TW * P * 8), o_ll = take(TW * 8), o_lp = take(TW * 8), o_acc = take(TW * 8), o_swap = take(TW * 8);
    const size_t o_status = take(8);
    const size_t state_end = off;
    const size_t o_src = take((size_t)K * 4), o_const = take((size_t)K * 8), o_fac = take((size_t)K * 8);
    const size_t o_lo = take((size_t)P * 8), o_hi = take((size_t)P * 8), o_betas = take((size_t)T * 8);
    const bool with_prior = ts.prior.any();
    const size_t o_pkind = take(with_prior ? (size_t)P * 4 : 0), o_ploc = take(with_prior ? (size_t)P * 8 : 0);
    const size_t o_pscale = take(with_prior ? (size_t)P * 8 : 0), o_pc0 = take(with_prior ? (size_t)P * 8 : 0);
    const size_t input_end = off;
    const size_t n_in = (size_t)n_steps;
    const size_t o_order = take(n_in * TW * 4), o_zz = take(n_in * TW * 8), o_thr = take(n_in * TW * 8), o_pick = take(n_in * TW * 4);
    const size_t o_prop = take((size_t)rows * P * 8), o_ok = take((size_t)rows), o_lpn = take((size_t)rows * 8);
    const size_t o_rows = off;
    const size_t o_chain = take(chain ? n_in * (size_t)n_chain_temps * W * P * 8 : 0);
    const size_t o_llc = take(lnlike_chain ? n_in * TW * 8 : 0);
    const size_t total = off;
    ChainArena& a = cat->temper;
    if (a.bytes < total) {
        if (a.d) (void)hipFree(a.d);
        if (a.h) (void)hipHostFree(a.h);
        a = ChainArena();
        const size_t want = total + total / 2;
        // (one device, no collective: a block too large for the arena simply runs host-driven)
        if (hipMalloc((void**)&a.d, want) != hipSuccess) { (void)hipGetLastError(); a = ChainArena(); return MCD_OK; }
        if (hipHostMalloc((void**)&a.h, want, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(a.d);
            a = ChainArena();
            return MCD_OK;
        }
        a.bytes = want;
    }
    std::memcpy(a.h + o_pos, pos, TW * P * 8);
    std::memcpy(a.h + o_ll, ll, TW * 8);
    std::memcpy(a.h + o_lp, lp0.data(), TW * 8);
    std::memset(a.h + o_acc, 0, TW * 8);
    std::memset(a.h + o_swap, 0, TW * 8);
    std::memset(a.h + o_status, 0, 8);
    std::memcpy(a.h + o_src, ts.col_source, (size_t)K * 4);
    std::memcpy(a.h + o_const, ts.col_const, (size_t)K * 8);
    std::memcpy(a.h + o_fac, ts.col_factor, (size_t)K * 8);
    std::memcpy(a.h + o_lo, ts.lo, (size_t)P * 8);
    std::memcpy(a.h + o_hi, ts.hi, (size_t)P * 8);
    std::memcpy(a.h + o_betas, ts.betas, (size_t)T * 8);
    if (with_prior) {
        std::memcpy(a.h + o_pkind, ts.prior.kind, (size_t)P * 4);
        std::memcpy(a.h + o_ploc, ts.prior.loc, (size_t)P * 8);
        std::memcpy(a.h + o_pscale, ts.prior.scale, (size_t)P * 8);
        std::memcpy(a.h + o_pc0, ts.prior.c0, (size_t)P * 8);
    }

    mcd::TemperDevice td;
    td.s = ts;
    td.s.col_source = (const int32_t*)(a.d + o_src); td.s.col_const = (const double*)(a.d + o_const);
    td.s.col_factor = (const double*)(a.d + o_fac); td.s.lo = (const double*)(a.d + o_lo); td.s.hi = (const double*)(a.d + o_hi);
    td.s.betas = (const double*)(a.d + o_betas);
    if (with_prior) {
        td.s.prior.kind = (const int32_t*)(a.d + o_pkind); td.s.prior.loc = (const double*)(a.d + o_ploc);
        td.s.prior.scale = (const double*)(a.d + o_pscale); td.s.prior.c0 = (const double*)(a.d + o_pc0);
    }
    td.seed = seed;
    td.pos = (double*)(a.d + o_pos); td.ll = (double*)(a.d + o_ll); td.lp = (double*)(a.d + o_lp);
    td.accepted = (long long*)(a.d + o_acc); td.swap_accepted = (long long*)(a.d + o_swap); td.status = (int32_t*)(a.d + o_status);
    td.order = (const int32_t*)(a.d + o_order); td.zz = (const double*)(a.d + o_zz); td.thr = (const double*)(a.d + o_thr);
    td.pick = (const int32_t*)(a.d + o_pick);
    td.proposal = (double*)(a.d + o_prop); td.ok = (uint8_t*)(a.d + o_ok); td.lp_new = (double*)(a.d + o_lpn);
    td.table = w.d_params;
    td.out = w.d_out;
    td.chain = chain ? (double*)(a.d + o_chain) : nullptr;
    td.lnlike_chain = lnlike_chain ? (double*)(a.d + o_llc) : nullptr;
    td.n_chain_temps = n_chain_temps;

    // the launch of mcd_api_eval.hip's enqueue() at kernel family 0: the same shape, records, chunk table and reduction
    w.staged = false;                     // the parameter table and the walker constants are about to be overwritten
    mcd::LaunchShape shape = main_launch_shape(cat, sh, w, 0, false, w.d_out, rows);
    const int64_t n_slots = mcd::partial_slots(shape, w.n_chunks, rows);
    MCD_HIP(hipMemcpyAsync(a.d, a.h, input_end, hipMemcpyHostToDevice, slot.stream));
    MCD_HIP(mcd::launch_chain_numbers(slot.stream, seed, step0, 0, n_steps, T, W, P, (int32_t*)(a.d + o_order),
                                      (double*)(a.d + o_zz), (double*)(a.d + o_thr), (int32_t*)(a.d + o_pick)));
    auto evaluate = [&]() -> int {
        MCD_HIP(mcd::launch_prepare_walkers(slot.stream, w.d_params, rows, K, cat->model, cat->free_centre, cat->precision, w.d_wpar));
        MCD_HIP(mcd::launch_loglike(slot.stream, shape, main_records(sh, w), w.d_chunks, w.n_chunks, w.d_wpar, w.d_partials, rows));
        MCD_HIP(mcd::launch_reduce(slot.stream, w.d_partials, w.d_offsets, 1, n_slots, n_slots, rows, nullptr, w.d_out));
        return MCD_OK;
    };
    for (int64_t i = 0; i < n_steps; ++i) {
        MCD_HIP(mcd::launch_temper_step(slot.stream, td, -1, 0, i, 0));
        if ((rc = evaluate()) != MCD_OK) return rc;
        MCD_HIP(mcd::launch_temper_step(slot.stream, td, i, 0, i, 1));
        if ((rc = evaluate()) != MCD_OK) return rc;
        MCD_HIP(mcd::launch_temper_step(slot.stream, td, i, 1, -1, 0));
        MCD_HIP(mcd::launch_temper_swap(slot.stream, td, step0 + i, i));
    }
    MCD_HIP(hipMemcpyAsync(a.h, a.d, state_end, hipMemcpyDeviceToHost, slot.stream));
    if (total > o_rows) MCD_HIP(hipMemcpyAsync(a.h + o_rows, a.d + o_rows, total - o_rows, hipMemcpyDeviceToHost, slot.stream));
    MCD_WAIT(cat->ctx, slot.stream, cat->spin_us, "mcd_temper_block (resident block)");

    w.fast = 0;
    cat->cur_walkers = rows;
    cat->last_chunks = w.n_chunks;
    cat->last_grid = n_slots != w.n_chunks ? n_slots : mcd::main_grid(w.n_chunks, rows);
    cat->last_narrow_bounded = 0;
    cat->last_series_chunks = 0;
    cat->last_direct_chunks = 0;
    cat->last_exp_split = 0;
    cat->last_root_quad = 0;
    cat->last_block_step = 0;
    cat->last_quad_chunks = 0;
    if (*(const int32_t*)(a.h + o_status) != 0)
        return fail(MCD_ERR_NONFINITE, "mcd_temper_block: the log-likelihood returned NaN");
    ++cat->temper_device_blocks;                      // (successful blocks only, as the host-driven form counts)
    std::memcpy(pos, a.h + o_pos, TW * P * 8);
    std::memcpy(ll, a.h + o_ll, TW * 8);
    std::memcpy(lp, a.h + o_lp, TW * 8);
    const int64_t* acc = (const int64_t*)(a.h + o_acc);
    if (accepted) for (size_t x = 0; x < TW; ++x) accepted[x] += acc[x];
    const int64_t* sw = (const int64_t*)(a.h + o_swap);
    for (int64_t t = 0; t + 1 < T; ++t) {
        if (swap_proposed) swap_proposed[t] += mcd::temper_swaps_proposed(step0, n_steps, t, T, W);
        if (!swap_accepted) continue;
        for (int64_t x = 0; x < W; ++x) swap_accepted[t] += sw[t * W + x];
    }
    if (chain) big_copy(chain, a.h + o_chain, n_in * (size_t)n_chain_temps * W * P * 8);
    if (lnlike_chain) big_copy(lnlike_chain, a.h + o_llc, n_in * TW * 8);
    *done = true;
    return MCD_OK;
}

int run_temper(mcd_catalog* cat, const mcd_temper_desc* d, int64_t n_steps, double* pos, double* lnlike, double* lnprior,
               uint64_t seed, int64_t step0, double* chain, double* lnlike_chain, int64_t* accepted, int64_t* swap_proposed,
               int64_t* swap_accepted, const mcd_prior_desc* prior) {
    if (!cat || !d || !pos || !lnlike || !lnprior) return fail(MCD_ERR_INVALID, "mcd_temper_block: null argument");
    if (int urc = ctx_usable(cat->ctx)) return urc;
    const mcd_stretch_desc& m = d->map;
    if (m.n_bins > 1 || cat->n_psets != 1)
        return fail(MCD_ERR_INVALID, "mcd_temper_block: binned catalogues are not covered (the rungs take the ensemble index of the bins)");
    if (cat->precision != MCD_F64) return fail(MCD_ERR_INVALID, "mcd_temper_block: tempered blocks need an MCD_F64 catalogue");
    if (m.k != cat->k) return fail(MCD_ERR_INVALID, "mcd_temper_block: descriptor has the wrong number of kernel columns");
    if (n_steps < 0 || step0 < 0) return fail(MCD_ERR_INVALID, "mcd_temper_block: steps non-negative");
    if (!m.col_source || !m.col_const || !m.col_factor || !m.lo || !m.hi || !d->betas) return fail(MCD_ERR_INVALID, "mcd_temper_block: null descriptor array");
    for (int c = 0; c < m.k; ++c)
        if (m.col_source[c] >= m.n_dim) return fail(MCD_ERR_INVALID, "mcd_temper_block: col_source outside the free parameters");
    mcd::TemperShared ts;
    ts.n_dim = m.n_dim; ts.k = m.k; ts.col_source = m.col_source; ts.col_const = m.col_const; ts.col_factor = m.col_factor;
    ts.lo = m.lo; ts.hi = m.hi; ts.fixed_ok = m.fixed_ok; ts.n_temps = d->n_temps; ts.n_walkers = m.n_walkers; ts.betas = d->betas;
    PriorHost ph;
    if (int prc = prior_of(prior, m.n_dim, "mcd_temper_block", ph)) return prc;
    ts.prior = ph.table;
    if (!mcd::temper_args_ok(ts, d->n_chain_temps))
        return fail(MCD_ERR_INVALID, "mcd_temper_block: n_walkers even and >= 2, 1 <= n_dim <= 12, n_temps >= 1, betas[0] == 1 and "
                                     "strictly decreasing within [0, 1], 1 <= n_chain_temps <= n_temps");
    if (temper_resident_covers(cat, ts.n_temps, ts.n_walkers, ts.n_dim, n_steps, d->n_chain_temps, chain != nullptr, lnlike_chain != nullptr)) {
        bool done = false;
        const int rc = temper_block_device(cat, ts, n_steps, pos, lnlike, lnprior, seed, step0, d->n_chain_temps, chain, lnlike_chain,
                                           accepted, swap_proposed, swap_accepted, &done);
        if (rc != MCD_OK) return rc;
        if (done) return MCD_OK;
    }
    // host-driven block: the same loop (mcd_temper.h) around mcd_loglike_batch, whose all-reduce makes it work on several
    // devices and ranks -- with the plain kernels whatever option "fast_path" says, which is left as it was found
    struct PlainKernels {
        mcd_catalog* cat; int saved;
        explicit PlainKernels(mcd_catalog* c) : cat(c), saved(c->allow_fast) { c->allow_fast = 0; }
        ~PlainKernels() { cat->allow_fast = saved; }
    } plain(cat);
    int eval_rc = MCD_OK;
    const int rc = mcd::temper_block(ts, n_steps, pos, lnlike, lnprior, seed, step0, d->n_chain_temps, chain, lnlike_chain, accepted,
                                     swap_proposed, swap_accepted, [&](const double* table, int64_t n, double* out) {
                                         eval_rc = mcd_loglike_batch(cat, n, m.k, table, out);
                                         return eval_rc;
                                     });
    if (rc == mcd::TEMPER_EVAL_FAILED) return eval_rc;                   // message already set
    if (rc == mcd::TEMPER_OUTSIDE)
        return fail(MCD_ERR_NONFINITE, "mcd_temper_block: a walker starts outside the prior or with a non-finite log-likelihood");
    if (rc == mcd::TEMPER_NAN) return fail(MCD_ERR_NONFINITE, "mcd_temper_block: the log-likelihood returned NaN");
    if (rc != mcd::TEMPER_OK) return fail(MCD_ERR_INVALID, "mcd_temper_block: bad arguments");
    ++cat->temper_host_blocks;
    return MCD_OK;
}

}  // namespace

extern "C" {

int mcd_temper_block(mcd_catalog* cat, const mcd_temper_desc* d, int64_t n_steps, double* pos, double* lnlike, double* lnprior,
                     uint64_t seed, int64_t step0, double* chain, double* lnlike_chain, int64_t* accepted,
                     int64_t* swap_proposed, int64_t* swap_accepted) {
    try {
    return run_temper(cat, d, n_steps, pos, lnlike, lnprior, seed, step0, chain, lnlike_chain, accepted, swap_proposed,
                      swap_accepted, nullptr);
    } catch (...) { return on_exception("mcd_temper_block"); }
}

int mcd_temper_block_prior(mcd_catalog* cat, const mcd_temper_desc* d, int64_t n_steps, double* pos, double* lnlike,
                           double* lnprior, uint64_t seed, int64_t step0, double* chain, double* lnlike_chain,
                           int64_t* accepted, int64_t* swap_proposed, int64_t* swap_accepted, const mcd_prior_desc* prior) {
    try {
    return run_temper(cat, d, n_steps, pos, lnlike, lnprior, seed, step0, chain, lnlike_chain, accepted, swap_proposed,
                      swap_accepted, prior);
    } catch (...) { return on_exception("mcd_temper_block_prior"); }
}

int mcd_temper_numbers(uint64_t seed, int64_t step0, int64_t n_steps, int32_t n_temps, int64_t n_walkers, double* swap_thr) {
    try {
    if (n_steps < 0 || step0 < 0 || n_temps < 1 || n_walkers < 1 || (!swap_thr && n_steps > 0 && n_temps > 1))
        return fail(MCD_ERR_INVALID, "mcd_temper_numbers: bad arguments");
    const int64_t pairs = n_temps - 1;
    for (int64_t i = 0; i < n_steps; ++i)
        for (int64_t t = 0; t < pairs; ++t)
            for (int64_t w = 0; w < n_walkers; ++w)
                swap_thr[((size_t)i * pairs + t) * n_walkers + w] = mcd::temper_swap_thr(seed, step0 + i, t, w);
    return MCD_OK;
    } catch (...) { return on_exception("mcd_temper_numbers"); }
}

int mcd_temper_info(const mcd_catalog* cat, int64_t* device_blocks, int64_t* host_blocks) {
    if (!cat) return fail(MCD_ERR_INVALID, "null catalogue");
    if (device_blocks) *device_blocks = cat->temper_device_blocks;
    if (host_blocks) *host_blocks = cat->temper_host_blocks;
    return MCD_OK;
}

}  // extern "C"

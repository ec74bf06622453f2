// mcd_api_ctx.hip -- C-ABI of the MI355X log-likelihood library (see include/mcd.h; mcd_host.h lists the host units):
// the thread's error message, the dlopen'ed RCCL table, contexts (streams, communicators) and what a failed or aborted
// context does to the waits on its streams.
#include <dlfcn.h>

#include "mcd_host.h"

using namespace mcd::host;

namespace {

std::mutex g_rccl_mutex;

// Wait for a stream: poll it (hipStreamQuery) for up to `spin_us` microseconds before handing the thread to the blocking
// hipStreamSynchronize.  A blocking wait that lasts more than a fraction of a millisecond sleeps on an interrupt and
// wakes the host 50 - 500 us after the device is done (measured as jitter of a 4 ms timed region, tools/k20_probe.py); an
// MCMC driver has nothing else to do with its thread while an evaluation is in flight, so it polls (option "spin_us",
// default 20000; 0 = always block).
hipError_t wait_stream(hipStream_t s, int64_t spin_us) {
    if (spin_us > 0) {
        const auto t0 = std::chrono::steady_clock::now();
        for (;;) {
            const hipError_t q = hipStreamQuery(s);
            if (q == hipSuccess) return hipSuccess;
            if (q != hipErrorNotReady) return q;
            if (std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count() > spin_us) break;
        }
    }
    return hipStreamSynchronize(s);
}

int make_slot(int device, DeviceSlot* slot) {
    MCD_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    MCD_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(MCD_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    slot->device = device;
    MCD_HIP(hipStreamCreateWithFlags(&slot->stream, hipStreamNonBlocking));
    // the communication stream gets the highest priority: its one small all-reduce kernel per step should take the next
    // free CU slots while the following step's main kernel (thousands of queued workgroups) is being dispatched
    int prio_least = 0, prio_greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess) prio_greatest = 0;
    MCD_HIP(hipStreamCreateWithPriority(&slot->comm_stream, hipStreamNonBlocking, prio_greatest));
    MCD_HIP(hipStreamCreateWithFlags(&slot->stream2, hipStreamNonBlocking));
    return MCD_OK;
}

// What both context constructors read from the environment: MCD_COLLECTIVE_TIMEOUT_MS (the context's deadline) and
// MCD_FORCE_RCCL=1, returned: also a one-device context gets its communicator from ncclCommInitAll and all-reduces inside
// ncclGroupStart/End, so that a single-GPU box runs the call sequence of the multi-device mode
bool read_ctx_env(mcd_ctx* ctx) {
    if (const char* t = std::getenv("MCD_COLLECTIVE_TIMEOUT_MS")) ctx->collective_timeout_ms = std::max<long long>(0, std::atoll(t));
    const char* force = std::getenv("MCD_FORCE_RCCL");
    return force && force[0] == '1';
}

}  // namespace

MCD_HOST_BEGIN

thread_local std::string g_last_error;
Rccl g_rccl;

int fail(int code, const std::string& msg) {
    try { g_last_error = msg; } catch (...) { g_last_error.clear(); }       // (assigning can allocate)
    return code;
}

// Every entry point that can allocate host memory (std::vector / std::map / std::string) runs inside try / catch and
// lands here: no C++ exception crosses the C boundary, the caller gets a status code and a message instead.
int on_exception(const char* where) noexcept {
    try {
        throw;
    } catch (const std::bad_alloc&) {
        try { g_last_error = std::string(where) + ": out of host memory"; } catch (...) { g_last_error.clear(); }
        return MCD_ERR_NOMEM;
    } catch (const std::exception& e) {
        try { g_last_error = std::string(where) + ": internal error: " + e.what(); } catch (...) { g_last_error.clear(); }
        return MCD_ERR_INVALID;
    } catch (...) {
        g_last_error.clear();
        return MCD_ERR_INVALID;
    }
}

int load_rccl() {
    std::lock_guard<std::mutex> lock(g_rccl_mutex);          // contexts may be created from several host threads
    if (g_rccl.handle) return MCD_OK;
    // MCD_RCCL_LIBRARY: an explicit library path.  Used by the tests to substitute tests/fake_rccl (a host-staged
    // stand-in) so that one GPU can run the multi-rank / multi-device call sequences with real shards and kernels.
    void* h = nullptr;
    if (const char* forced = std::getenv("MCD_RCCL_LIBRARY")) {
        h = dlopen(forced, RTLD_NOW | RTLD_GLOBAL);
        if (!h) return fail(MCD_ERR_RCCL, std::string("cannot load MCD_RCCL_LIBRARY: ") + dlerror());
    }
    if (!h) h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return fail(MCD_ERR_RCCL, std::string("cannot load librccl.so: ") + dlerror());
#define MCD_SYM(field, name)                                                                            \
    g_rccl.field = reinterpret_cast<decltype(g_rccl.field)>(dlsym(h, name));                            \
    if (!g_rccl.field) return fail(MCD_ERR_RCCL, std::string("librccl.so lacks ") + name);
    MCD_SYM(GetUniqueId, "ncclGetUniqueId")
    MCD_SYM(CommInitRank, "ncclCommInitRank")
    MCD_SYM(CommInitAll, "ncclCommInitAll")
    MCD_SYM(CommDestroy, "ncclCommDestroy")
    MCD_SYM(AllReduce, "ncclAllReduce")
    MCD_SYM(GroupStart, "ncclGroupStart")
    MCD_SYM(GroupEnd, "ncclGroupEnd")
    MCD_SYM(GetErrorString, "ncclGetErrorString")
    MCD_SYM(CommCount, "ncclCommCount")
    MCD_SYM(CommUserRank, "ncclCommUserRank")
    MCD_SYM(GetVersion, "ncclGetVersion")
#undef MCD_SYM
    g_rccl.handle = h;
    return MCD_OK;
}

// The context failed (deadline, abort, an error in the middle of a block of launches other ranks are already committed
// to): remember the first cause; every later call answers MCD_ERR_RCCL at once (ctx_usable).
int ctx_fail(mcd_ctx* ctx, const std::string& what) {
    {
        std::lock_guard<std::mutex> lock(ctx->note_mutex);
        if (!ctx->failed.load()) ctx->failure = what;
        ctx->failed.store(1);
    }
    return fail(MCD_ERR_RCCL, what + " -- the context is unusable from here on: report and exit the process (no fallback "
                                     "inside it; mcd.h: collective deadline)");
}

int ctx_usable(mcd_ctx* ctx) {
    if (!ctx || !ctx->failed.load()) return MCD_OK;
    std::lock_guard<std::mutex> lock(ctx->note_mutex);
    return fail(MCD_ERR_RCCL, "this context failed earlier (" + ctx->failure + "): exit the process");
}

// Wait for a stream of a context.  Without a communicator: wait_stream.  With one, the stream may sit behind an
// all-reduce whose peers never arrive: poll (spin first, then sleep between polls), give up at the deadline or when
// another host thread raises the abort flag, and mark the context failed.  `stage` names the wait in the message.
int wait_ctx_stream(mcd_ctx* ctx, hipStream_t s, int64_t spin_us, const char* stage) {
    if (!ctx->has_comm() || ctx->collective_timeout_ms < 0) {
        const hipError_t e = wait_stream(s, spin_us);
        if (e != hipSuccess) return fail(MCD_ERR_HIP, std::string(stage) + ": " + hipGetErrorString(e));
        return MCD_OK;
    }
    const auto t0 = std::chrono::steady_clock::now();
    const int64_t limit_us = ctx->collective_timeout_ms * 1000;
    for (;;) {
        const hipError_t q = hipStreamQuery(s);
        if (q == hipSuccess) return MCD_OK;
        if (q != hipErrorNotReady) return fail(MCD_ERR_HIP, std::string(stage) + ": " + hipGetErrorString(q));
        if (ctx->abort_flag.load(std::memory_order_acquire)) {
            std::string why;
            { std::lock_guard<std::mutex> lock(ctx->note_mutex); why = ctx->abort_reason; }
            return ctx_fail(ctx, std::string(stage) + ": aborted by the host while waiting for a collective (" +
                                 (why.empty() ? "no reason given" : why) + ")");
        }
        const int64_t waited = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
        if (limit_us > 0 && waited > limit_us) {
            char buf[256];
            snprintf(buf, sizeof buf, "%s: no completion within collective_timeout_ms = %lld (rank %d of %d): a peer never "
                                      "reached the all-reduce, or the fabric is down",
                     stage, (long long)ctx->collective_timeout_ms, ctx->rank, ctx->n_ranks);
            return ctx_fail(ctx, buf);
        }
        if (waited > spin_us) std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
}

MCD_HOST_END

extern "C" {

const char* mcd_last_error(void) { return g_last_error.c_str(); }
int mcd_abi_version(void) { return MCD_ABI_VERSION; }

int mcd_ctx_create(int n_dev, const int* dev_ids, mcd_ctx** out) {
    try {
    if (!out || n_dev <= 0) return fail(MCD_ERR_INVALID, "mcd_ctx_create: bad arguments");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(MCD_ERR_NO_DEVICE, "no HIP device visible");
    // MCD_ALLOW_SHARED_DEVICE=1 (testing aid, with MCD_RCCL_LIBRARY): several shards may sit on the same device, each with
    // its own streams -- real RCCL refuses that, the stand-in of tests/fake_rccl does not
    const char* shared_dev = std::getenv("MCD_ALLOW_SHARED_DEVICE");
    const bool allow_shared = shared_dev && shared_dev[0] == '1' && dev_ids != nullptr;
    if (n_dev > count && !allow_shared) return fail(MCD_ERR_NO_DEVICE, "more devices requested than visible");
    if (dev_ids)
        for (int i = 0; i < n_dev; ++i)
            if (dev_ids[i] < 0 || dev_ids[i] >= count) return fail(MCD_ERR_NO_DEVICE, "device index out of range");
    std::unique_ptr<mcd_ctx, int (*)(mcd_ctx*)> ctx(new (std::nothrow) mcd_ctx(), &mcd_ctx_destroy);   // streams / communicators released on every error path
    if (!ctx) return fail(MCD_ERR_INVALID, "out of memory");
    ctx->slots.resize(n_dev);
    const bool force_rccl = read_ctx_env(ctx.get());
    std::vector<int> ids(n_dev);
    for (int i = 0; i < n_dev; ++i) {
        ids[i] = dev_ids ? dev_ids[i] : i;
        int rc = make_slot(ids[i], &ctx->slots[i]);
        if (rc != MCD_OK) return rc;
    }
    ctx->force_collective = n_dev == 1 && force_rccl;
    if (n_dev > 1 || ctx->force_collective) {
        int rc = load_rccl();
        if (rc != MCD_OK) return rc;
        std::vector<ncclComm_t> comms(n_dev);
        MCD_NCCL(g_rccl.CommInitAll(comms.data(), n_dev, ids.data()));
        for (int i = 0; i < n_dev; ++i) ctx->slots[i].comm = comms[i];
    }
    ctx->rank = 0;
    ctx->n_ranks = 1;
    ctx->multi_process = false;
    *out = ctx.release();
    return MCD_OK;
    } catch (...) { return on_exception("mcd_ctx_create"); }
}

int mcd_get_unique_id(void* out_id) {
    try {
    if (!out_id) return fail(MCD_ERR_INVALID, "null id buffer");
    static_assert(sizeof(ncclUniqueId) <= MCD_UNIQUE_ID_BYTES, "unique id does not fit");
    int rc = load_rccl();
    if (rc != MCD_OK) return rc;
    ncclUniqueId id;
    MCD_NCCL(g_rccl.GetUniqueId(&id));
    std::memset(out_id, 0, MCD_UNIQUE_ID_BYTES);
    std::memcpy(out_id, &id, sizeof id);
    return MCD_OK;
    } catch (...) { return on_exception("mcd_get_unique_id"); }
}

int mcd_ctx_create_rank(int device, int rank, int n_ranks, const void* unique_id, mcd_ctx** out) {
    try {
    if (!out || n_ranks <= 0 || rank < 0 || rank >= n_ranks) return fail(MCD_ERR_INVALID, "mcd_ctx_create_rank: bad arguments");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(MCD_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= count) return fail(MCD_ERR_NO_DEVICE, "device index out of range");
    std::unique_ptr<mcd_ctx, int (*)(mcd_ctx*)> ctx(new (std::nothrow) mcd_ctx(), &mcd_ctx_destroy);   // streams / communicators released on every error path
    if (!ctx) return fail(MCD_ERR_INVALID, "out of memory");
    ctx->slots.resize(1);
    const bool force_rccl = read_ctx_env(ctx.get());
    int rc = make_slot(device, &ctx->slots[0]);
    if (rc != MCD_OK) return rc;
    ctx->force_collective = force_rccl && unique_id;
    if (n_ranks > 1 || ctx->force_collective) {
        if (!unique_id) return fail(MCD_ERR_INVALID, "unique_id required when n_ranks > 1");
        rc = load_rccl();
        if (rc != MCD_OK) return rc;
        ncclUniqueId id;
        std::memcpy(&id, unique_id, sizeof id);
        MCD_NCCL(g_rccl.CommInitRank(&ctx->slots[0].comm, n_ranks, id, rank));
    }
    ctx->rank = rank;
    ctx->n_ranks = n_ranks;
    ctx->multi_process = true;
    *out = ctx.release();
    return MCD_OK;
    } catch (...) { return on_exception("mcd_ctx_create_rank"); }
}

int mcd_ctx_destroy(mcd_ctx* ctx) {
    if (!ctx) return MCD_OK;
    // a failed context has streams blocked behind a collective that will never finish: destroying them or the
    // communicator would block this thread as well.  The handles are abandoned; the process is about to exit.
    if (ctx->failed.load()) { delete ctx; return MCD_OK; }
    for (DeviceSlot& s : ctx->slots) {
        (void)hipSetDevice(s.device);
        if (s.comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(s.comm);
        if (s.stream) (void)hipStreamDestroy(s.stream);
        if (s.comm_stream) (void)hipStreamDestroy(s.comm_stream);
        if (s.stream2) (void)hipStreamDestroy(s.stream2);
    }
    delete ctx;
    return MCD_OK;
}

int mcd_ctx_n_devices(const mcd_ctx* ctx) { return ctx ? (int)ctx->slots.size() : 0; }

int mcd_ctx_set_option(mcd_ctx* ctx, const char* key, int64_t value) {
    try {
    if (!ctx || !key) return fail(MCD_ERR_INVALID, "mcd_ctx_set_option: null argument");
    if (!std::strcmp(key, "collective_timeout_ms")) {
        if (value < 0) return fail(MCD_ERR_INVALID, "collective_timeout_ms must be >= 0 (0: wait for ever)");
        ctx->collective_timeout_ms = value;
        return MCD_OK;
    }
    return fail(MCD_ERR_INVALID, std::string("unknown context option: ") + key);
    } catch (...) { return on_exception("mcd_ctx_set_option"); }
}

int mcd_ctx_abort(mcd_ctx* ctx, const char* reason) {
    try {
    if (!ctx) return fail(MCD_ERR_INVALID, "mcd_ctx_abort: null context");
    {
        std::lock_guard<std::mutex> lock(ctx->note_mutex);
        if (ctx->abort_reason.empty() && reason) ctx->abort_reason = reason;
    }
    ctx->abort_flag.store(1, std::memory_order_release);
    return MCD_OK;
    } catch (...) { return on_exception("mcd_ctx_abort"); }
}

int mcd_ctx_failed(const mcd_ctx* ctx) { return ctx && ctx->failed.load() ? 1 : 0; }

int mcd_ctx_comm_info(const mcd_ctx* ctx, int* comm_size, int* comm_rank, int* rccl_version) {
    try {
    if (!ctx || ctx->slots.empty()) return fail(MCD_ERR_INVALID, "mcd_ctx_comm_info: null context");
    if (comm_size) *comm_size = 0;
    if (comm_rank) *comm_rank = -1;
    if (rccl_version) *rccl_version = 0;
    const ncclComm_t comm = ctx->slots[0].comm;
    if (!comm) return MCD_OK;                       // single device, RCCL never loaded
    int n = 0, r = -1, v = 0;
    MCD_NCCL(g_rccl.CommCount(comm, &n));
    MCD_NCCL(g_rccl.CommUserRank(comm, &r));
    MCD_NCCL(g_rccl.GetVersion(&v));
    if (comm_size) *comm_size = n;
    if (comm_rank) *comm_rank = r;
    if (rccl_version) *rccl_version = v;
    return MCD_OK;
    } catch (...) { return on_exception("mcd_ctx_comm_info"); }
}

}  // extern "C"

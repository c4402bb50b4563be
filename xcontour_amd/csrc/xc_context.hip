// C ABI of libxcontour_hip.so (declared in include/xcontour_hip.h), part 1: the context and its error state, the grow-only device
// blocks it owns, device memory, residency, events and the timing of the dominant kernel.  No C++ type or exception crosses this boundary.
#include "xc_capi.h"
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#include <new>
#include <mutex>
#include <set>
#include <utility>

namespace xc {

static thread_local std::string g_err;   // errors without a context (xc_create)

int fail(xc_ctx* ctx, int code, const std::string& msg)
{
    if (ctx) {
        ctx->err = msg;
        // a call that fails delivers nothing: results still parked in the pinned output buffer must not reach arrays the caller may
        // free once it has seen the error
        ctx->pending_out.clear(); ctx->pending_in.clear(); ctx->pin_in_off = 0; ctx->pin_out_off = 0;
        // (an entry of the small-input cache filled during the failed call may never have been uploaded: forget what this call staged)
        for (auto& e : ctx->small_in) if (e.epoch == ctx->small_epoch) { e.host.clear(); e.epoch = ~0ull; }
        ++ctx->small_epoch;
    } else g_err = msg;
    return code;
}

int hipfail(xc_ctx* ctx, hipError_t e, const char* what)
{
    std::string m = std::string("HIP error: ") + hipGetErrorString(e) + " in " + what;
    (void)hipGetLastError();
    return fail(ctx, e == hipErrorOutOfMemory ? XC_ENOMEM : XC_EHIP, m);
}

int grow(xc_ctx* ctx, void** p, size_t* have, size_t need)
{
    if (need <= *have) return XC_OK;
    size_t want = *have ? *have : (size_t)1 << 20;
    while (want < need) want *= 2;
    if (*p) {
        XC_HIP(ctx, hipStreamSynchronize(ctx->stream));    // nothing in flight may still use the old block
        XC_HIP(ctx, hipFree(*p));
        *p = nullptr; *have = 0;
    }
    hipError_t e = hipMalloc(p, want);
    if (e != hipSuccess) { want = need; e = hipMalloc(p, want); }
    if (e != hipSuccess) return hipfail(ctx, e, "hipMalloc(scratch)");
    *have = want;
    return XC_OK;
}

int ensure_scratch(xc_ctx* ctx, size_t bytes) { return grow(ctx, &ctx->scratch, &ctx->scratch_bytes, bytes); }
int ensure_arena(xc_ctx* ctx, size_t bytes, void** base) { const int rc = grow(ctx, &ctx->arena, &ctx->arena_bytes, bytes); *base = ctx->arena; return rc; }
int ensure_big(xc_ctx* ctx, size_t bytes)     { return grow(ctx, &ctx->big, &ctx->big_bytes, bytes); }

int ensure_ones(xc_ctx* ctx, size_t n)
{
    if (n <= ctx->ones_n) return XC_OK;
    if (ctx->ones) { XC_HIP(ctx, hipStreamSynchronize(ctx->stream)); XC_HIP(ctx, hipFree(ctx->ones)); ctx->ones = nullptr; ctx->ones_n = 0; }
    size_t want = 4096; while (want < n) want *= 2;
    XC_HIP(ctx, hipMalloc((void**)&ctx->ones, want * sizeof(double)));
    std::vector<double> h(want, 1.0);
    XC_HIP(ctx, hipMemcpy(ctx->ones, h.data(), want * sizeof(double), hipMemcpyHostToDevice));
    ctx->ones_n = want;
    return XC_OK;
}

int ensure_big_lds(xc_ctx* ctx, const void* kernel, int bytes)
{
    static std::mutex mu;
    static std::set<std::pair<const void*, int>> done;
    std::lock_guard<std::mutex> lk(mu);
    const auto key = std::make_pair(kernel, ctx->device);
    if (done.count(key)) return XC_OK;
    XC_HIP(ctx, hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done.insert(key);
    return XC_OK;
}

// chained min/max partials (xc_keff_desc.q_next) describe the bytes [mm_q, mm_q + nslab*ny*nx*esize): any write into
// that range through the library, or freeing it, drops them
void mm_touch(xc_ctx* ctx, const void* p, size_t bytes)
{
    if (!ctx->mm_valid || !p) return;
    const char* a0 = (const char*)ctx->mm_q;
    const char* a1 = a0 + (size_t)ctx->mm_nslab * ctx->mm_ny * ctx->mm_nx * (ctx->mm_dtype == XC_F32 ? 4 : 8);
    const char* b0 = (const char*)p;
    if (b0 < a1 && b0 + (bytes ? bytes : 1) > a0) ctx->mm_valid = 0;
}

// device mirror of the host bytes [h, h + n), if the caller registered an array that contains them (xc_keep_resident)
const void* resident_lookup(const xc_ctx* ctx, const void* h, size_t n)
{
    const char* p = (const char*)h;
    for (const auto& e : ctx->resident)
        if (p >= e.host && p + n <= e.host + e.bytes) return (const char*)e.dev + (p - e.host);
    return nullptr;
}

int hist_ev_begin(xc_ctx* ctx)
{
    if (ctx->user_ev0) XC_HIP(ctx, hipEventRecord(ctx->user_ev0, ctx->stream));
    else if (ctx->timing) XC_HIP(ctx, hipEventRecord(ctx->ev_hist0, ctx->stream));
    return XC_OK;
}

int hist_ev_end(xc_ctx* ctx)
{
    if (ctx->user_ev0) {
        if (ctx->user_ev1) XC_HIP(ctx, hipEventRecord(ctx->user_ev1, ctx->stream));
        ctx->user_ev0 = ctx->user_ev1 = nullptr;
    } else if (ctx->timing) {
        XC_HIP(ctx, hipEventRecord(ctx->ev_hist1, ctx->stream)); ctx->ev_valid = 1;
    }
    return XC_OK;
}

}  // namespace xc

using namespace xc;

extern "C" {

const char* xc_version(void) { return "xcontour_hip 0.1.0 (gfx950)"; }

int xc_device_count(int* out_count)
{
    if (!out_count) return fail(nullptr, XC_EBADARG, "xc_device_count: out is NULL");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); n = 0; }
    *out_count = n;
    return XC_OK;
}

const char* xc_last_error(xc_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

int xc_create(int device_id, xc_ctx** out)
{
    if (!out) return fail(nullptr, XC_EBADARG, "xc_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1) {
        (void)hipGetLastError();
        return fail(nullptr, XC_ENODEV, "xc_create: no HIP device visible (this library has no CPU fallback)");
    }
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, XC_EBADARG, "xc_create: device_id out of range");
    xc_ctx* ctx = new (std::nothrow) xc_ctx();
    if (!ctx) return fail(nullptr, XC_ENOMEM, "xc_create: out of host memory");
    ctx->device = device_id;
    hipDeviceProp_t prop;
    if ((e = hipSetDevice(device_id)) != hipSuccess || (e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess) {
        int rc = hipfail(nullptr, e, "hipSetDevice/hipGetDeviceProperties"); delete ctx; return rc;
    }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        std::string m = std::string("xc_create: device is ") + prop.gcnArchName + ", this library is built for gfx950 only";
        delete ctx; return fail(nullptr, XC_ENODEV, m);
    }
    // (some boxes of the pool report an EMPTY marketing name: the field a reader checks first must still say what ran)
    snprintf(ctx->name, sizeof(ctx->name), "%s (%s, %d CUs, %.0f GB)", prop.name[0] ? prop.name : "AMD Instinct [name not reported by the driver]",
             prop.gcnArchName, prop.multiProcessorCount, (double)prop.totalGlobalMem / 1e9);
    {
        // the only place the library reads the environment: K3 geometry knobs for experiments (xc_internal.h, HistKnobs)
        auto env_int = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
        HistKnobs& k = ctx->knobs;
        k.xcd_map = env_int("XC_HIST_XCDMAP", 1); k.tile_map = env_int("XC_HIST_TILEMAP", 1); k.vec4 = env_int("XC_HIST_VEC4", -1); k.e32 = env_int("XC_HIST_E32", 1);
        k.threads = env_int("XC_HIST_THREADS", 0); k.ncopy = env_int("XC_HIST_NCOPY", 0); k.rows = env_int("XC_HIST_ROWS", 0);
        k.bps = env_int("XC_HIST_BPS", 0);
        k.cross_ncopy = env_int("XC_CROSS_NCOPY", 0); k.cross_blocks = env_int("XC_CROSS_BLOCKS", 0);
        k.copy_kernel = env_int("XC_COPY_KERNEL", 1); k.copy_out_kb = env_int("XC_COPY_OUT_KB", 256); if (k.copy_out_kb < 1 || k.copy_out_kb > 1024) k.copy_out_kb = 256; k.single = env_int("XC_KEFF_SINGLE", 1); k.single_timeout_us = env_int("XC_KEFF_SINGLE_TIMEOUT_US", 50000); k.single_map = env_int("XC_KEFF_SINGLE_MAP", 0);
        k.sort_range = env_int("XC_SORT_RANGE", 1); k.lwa_fast = env_int("XC_LWA_FAST", 1); k.k1_nt = env_int("XC_K1_NT", 0); k.lwa_strip = env_int("XC_LWA_STRIP", 1);
    }
    ctx->cus = prop.multiProcessorCount;
    if ((e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)) != hipSuccess) {
        int rc = hipfail(nullptr, e, "hipStreamCreate"); delete ctx; return rc;
    }
    if ((e = hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&ctx->ev_copy, hipEventDisableTiming)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&ctx->ev_compute, hipEventDisableTiming)) != hipSuccess) {
        int rc = hipfail(nullptr, e, "hipStreamCreate(copy)"); delete ctx; return rc;
    }
    if ((e = hipEventCreate(&ctx->ev_hist0)) != hipSuccess || (e = hipEventCreate(&ctx->ev_hist1)) != hipSuccess) {
        int rc = hipfail(nullptr, e, "hipEventCreate"); delete ctx; return rc;
    }
    *out = ctx;
    return XC_OK;
}

int xc_destroy(xc_ctx* ctx)
{
    if (!ctx) return XC_OK;
    (void)hipSetDevice(ctx->device);
    (void)xc_comm_finalize(ctx);
    if (ctx->copy_stream) (void)hipStreamSynchronize(ctx->copy_stream);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->comm_stream) { (void)hipStreamSynchronize(ctx->comm_stream); (void)hipStreamDestroy(ctx->comm_stream); }
    if (ctx->ev_comm_in) (void)hipEventDestroy(ctx->ev_comm_in);
    if (ctx->ev_comm_out) (void)hipEventDestroy(ctx->ev_comm_out);
    if (ctx->pinned_flag) (void)hipHostFree(ctx->pinned_flag);
    for (auto& e : ctx->small_in) if (e.dev) (void)hipFree(e.dev);
    if (ctx->pin_in) (void)hipHostFree(ctx->pin_in);
    if (ctx->pin_out) (void)hipHostFree(ctx->pin_out);
    if (ctx->lwa_flag) (void)hipFree(ctx->lwa_flag);
    if (ctx->single_ws) (void)hipFree(ctx->single_ws);
    if (ctx->single_stamps) (void)hipFree(ctx->single_stamps);
    for (auto& e : ctx->resident) (void)hipFree(e.dev);
    if (ctx->ev_copy) (void)hipEventDestroy(ctx->ev_copy);
    if (ctx->ev_compute) (void)hipEventDestroy(ctx->ev_compute);
    if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
    if (ctx->scratch) (void)hipFree(ctx->scratch);
    if (ctx->arena) (void)hipFree(ctx->arena);
    if (ctx->big) (void)hipFree(ctx->big);
    if (ctx->cpiece_ws) (void)hipFree(ctx->cpiece_ws);
    if (ctx->cpiece_acc) (void)hipFree(ctx->cpiece_acc);
    if (ctx->cscale_ws) (void)hipFree(ctx->cscale_ws);
    if (ctx->ones) (void)hipFree(ctx->ones);
    for (int i = 0; i < 2; ++i) if (ctx->mmnext[i]) (void)hipFree(ctx->mmnext[i]);
    if (ctx->ev_hist0) (void)hipEventDestroy(ctx->ev_hist0);
    if (ctx->ev_hist1) (void)hipEventDestroy(ctx->ev_hist1);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return XC_OK;
}

int xc_device_name(xc_ctx* ctx, char* buf, size_t buflen)
{
    if (!ctx || !buf || buflen == 0) return fail(ctx, XC_EBADARG, "xc_device_name: bad arguments");
    snprintf(buf, buflen, "%s", ctx->name);
    return XC_OK;
}

int xc_device_cus(xc_ctx* ctx, int* out_cus)
{
    if (!ctx || !out_cus) return fail(ctx, XC_EBADARG, "xc_device_cus: bad arguments");
    *out_cus = ctx->cus;
    return XC_OK;
}

void* xc_stream(xc_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int xc_malloc(xc_ctx* ctx, size_t bytes, void** out_dptr)
{
    XC_CTX(ctx);
    if (!out_dptr) return fail(ctx, XC_EBADARG, "xc_malloc: out is NULL");
    *out_dptr = nullptr;
    XC_HIP(ctx, hipMalloc(out_dptr, bytes ? bytes : 1));
    return XC_OK;
}

int xc_keep_resident(xc_ctx* ctx, const void* host_ptr, size_t bytes)
{
    XC_CTX(ctx);
    if (!host_ptr || bytes == 0) return fail(ctx, XC_EBADARG, "xc_keep_resident: bad arguments");
    XC_HIP(ctx, hipStreamSynchronize(ctx->copy_stream));
    XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < ctx->resident.size(); ++i)
        if (ctx->resident[i].host == (const char*)host_ptr) {       // registered before: refresh (the caller changed the array)
            auto& e = ctx->resident[i];
            hipError_t he = hipSuccess;
            if (bytes > e.bytes) {
                (void)hipFree(e.dev); e.dev = nullptr; e.bytes = 0;
                he = hipMalloc(&e.dev, bytes);
            }
            if (he == hipSuccess) he = hipMemcpy(e.dev, host_ptr, bytes, hipMemcpyHostToDevice);
            if (he != hipSuccess) {                                 // never leave a dead or half-refreshed mirror registered
                if (e.dev) (void)hipFree(e.dev);
                ctx->resident.erase(ctx->resident.begin() + (long)i);
                return hipfail(ctx, he, "xc_keep_resident: refresh");
            }
            e.bytes = bytes;                                        // (a shorter array now: the tail of the old mirror is no longer valid)
            // most recently refreshed first: an overlapping registration (an array and a sub-slab of it at another base
            // pointer) resolves to the mirror that was uploaded last
            if (i != 0) { auto me = e; ctx->resident.erase(ctx->resident.begin() + (long)i); ctx->resident.insert(ctx->resident.begin(), me); }
            return XC_OK;
        }
    void* dev = nullptr;
    XC_HIP(ctx, hipMalloc(&dev, bytes));
    hipError_t e = hipMemcpy(dev, host_ptr, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(dev); return hipfail(ctx, e, "xc_keep_resident: upload"); }
    ctx->resident.insert(ctx->resident.begin(), {(const char*)host_ptr, bytes, dev});       // newest first (see the refresh path)
    return XC_OK;
}

int xc_resident_lookup(xc_ctx* ctx, const void* host_ptr, size_t bytes, void** out_dev)
{
    if (!ctx || !out_dev) return fail(ctx, XC_EBADARG, "xc_resident_lookup: bad arguments");
    *out_dev = (host_ptr && bytes && !ctx->resident.empty()) ? const_cast<void*>(resident_lookup(ctx, host_ptr, bytes)) : nullptr;
    return XC_OK;
}

int xc_release_resident(xc_ctx* ctx, const void* host_ptr)
{
    XC_CTX(ctx);
    XC_HIP(ctx, hipStreamSynchronize(ctx->copy_stream));        // an asynchronous upload may still be reading a mirror
    XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < ctx->resident.size();) {
        if (!host_ptr || ctx->resident[i].host == (const char*)host_ptr) {
            (void)hipFree(ctx->resident[i].dev);
            ctx->resident.erase(ctx->resident.begin() + (long)i);
        } else ++i;
    }
    return XC_OK;
}

int xc_free(xc_ctx* ctx, void* dptr)
{
    XC_CTX(ctx);
    if (!dptr) return XC_OK;
    mm_touch(ctx, dptr, (size_t)1 << 62);         // an allocation that starts at or below the cached batch may contain it
    XC_HIP(ctx, hipStreamSynchronize(ctx->copy_stream));
    XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    XC_HIP(ctx, hipFree(dptr));
    return XC_OK;
}

int xc_memcpy_h2d(xc_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes)
{
    XC_CTX(ctx);
    if (bytes && (!dst_dev || !src_host)) return fail(ctx, XC_EBADARG, "xc_memcpy_h2d: NULL pointer");
    mm_touch(ctx, dst_dev, bytes);
    const void* m = ctx->resident.empty() ? nullptr : resident_lookup(ctx, src_host, bytes);   // a registered array: from its device mirror
    XC_HIP(ctx, hipMemcpyAsync(dst_dev, m ? m : src_host, bytes, m ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return XC_OK;
}

int xc_memcpy_h2d_async(xc_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes)
{
    XC_CTX(ctx);
    if (bytes && (!dst_dev || !src_host)) return fail(ctx, XC_EBADARG, "xc_memcpy_h2d_async: NULL pointer");
    mm_touch(ctx, dst_dev, bytes);
    const void* m = ctx->resident.empty() ? nullptr : resident_lookup(ctx, src_host, bytes);
    XC_HIP(ctx, hipMemcpyAsync(dst_dev, m ? m : src_host, bytes, m ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->copy_stream));
    return XC_OK;
}

int xc_stream_wait_copies(xc_ctx* ctx)
{
    XC_CTX(ctx);
    XC_HIP(ctx, hipEventRecord(ctx->ev_copy, ctx->copy_stream));
    XC_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_copy, 0));
    return XC_OK;
}

int xc_copies_wait_stream(xc_ctx* ctx)
{
    XC_CTX(ctx);
    XC_HIP(ctx, hipEventRecord(ctx->ev_compute, ctx->stream));
    XC_HIP(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_compute, 0));
    return XC_OK;
}

int xc_memcpy_d2h(xc_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes)
{
    XC_CTX(ctx);
    if (bytes && (!dst_host || !src_dev)) return fail(ctx, XC_EBADARG, "xc_memcpy_d2h: NULL pointer");
    XC_TRY(d2h(ctx, dst_host, src_dev, bytes));
    return xc_sync(ctx);
}

int xc_memset(xc_ctx* ctx, void* dptr, int value, size_t bytes)
{
    XC_CTX(ctx);
    if (bytes && !dptr) return fail(ctx, XC_EBADARG, "xc_memset: NULL pointer");
    mm_touch(ctx, dptr, bytes);
    XC_HIP(ctx, hipMemsetAsync(dptr, value, bytes, ctx->stream));
    return XC_OK;
}

int xc_event_create(xc_ctx* ctx, void** out_event)
{
    XC_CTX(ctx);
    if (!out_event) return fail(ctx, XC_EBADARG, "xc_event_create: out is NULL");
    hipEvent_t ev;
    XC_HIP(ctx, hipEventCreate(&ev));
    *out_event = (void*)ev;
    return XC_OK;
}

int xc_event_destroy(xc_ctx* ctx, void* event)
{
    XC_CTX(ctx);
    if (event) XC_HIP(ctx, hipEventDestroy((hipEvent_t)event));
    return XC_OK;
}

int xc_event_record(xc_ctx* ctx, void* event)
{
    XC_CTX(ctx);
    if (!event) return fail(ctx, XC_EBADARG, "xc_event_record: NULL event");
    XC_HIP(ctx, hipEventRecord((hipEvent_t)event, ctx->stream));
    return XC_OK;
}

int xc_event_record_copies(xc_ctx* ctx, void* event)      // on the COPY stream: completes when the uploads issued so far have landed
{
    XC_CTX(ctx);
    if (!event) return fail(ctx, XC_EBADARG, "xc_event_record_copies: NULL event");
    XC_HIP(ctx, hipEventRecord((hipEvent_t)event, ctx->copy_stream));
    return XC_OK;
}

int xc_event_query(xc_ctx* ctx, void* event, int* out_done)
{
    XC_CTX(ctx);
    if (!event || !out_done) return fail(ctx, XC_EBADARG, "xc_event_query: NULL argument");
    const hipError_t e = hipEventQuery((hipEvent_t)event);
    if (e == hipSuccess) { *out_done = 1; return XC_OK; }
    *out_done = 0;
    if (e == hipErrorNotReady) { (void)hipGetLastError(); return XC_OK; }
    return hipfail(ctx, e, "hipEventQuery");
}

int xc_event_elapsed_ms(xc_ctx* ctx, void* start, void* stop, float* out_ms)
{
    XC_CTX(ctx);
    if (!start || !stop || !out_ms) return fail(ctx, XC_EBADARG, "xc_event_elapsed_ms: NULL argument");
    XC_HIP(ctx, hipEventSynchronize((hipEvent_t)stop));
    XC_HIP(ctx, hipEventElapsedTime(out_ms, (hipEvent_t)start, (hipEvent_t)stop));
    return XC_OK;
}

int xc_set_kernel_timing(xc_ctx* ctx, int enable)
{
    if (!ctx) return fail(nullptr, XC_EBADARG, "null context");
    ctx->timing = enable ? 1 : 0; ctx->ev_valid = 0;
    return XC_OK;
}

int xc_set_hist_events(xc_ctx* ctx, void* start_event, void* stop_event)
{
    if (!ctx) return fail(nullptr, XC_EBADARG, "null context");
    ctx->user_ev0 = (hipEvent_t)start_event; ctx->user_ev1 = (hipEvent_t)stop_event;
    return XC_OK;
}

int xc_last_hist_ms(xc_ctx* ctx, float* out_ms)
{
    XC_CTX(ctx);
    if (!out_ms) return fail(ctx, XC_EBADARG, "xc_last_hist_ms: out is NULL");
    if (!ctx->ev_valid) return fail(ctx, XC_EBADARG, "xc_last_hist_ms: no timed histogram launch (call xc_set_kernel_timing(ctx,1) first)");
    XC_HIP(ctx, hipEventSynchronize(ctx->ev_hist1));
    XC_HIP(ctx, hipEventElapsedTime(out_ms, ctx->ev_hist0, ctx->ev_hist1));
    return XC_OK;
}

}  // extern "C"

// The transport of the host-form entry points: pinned bounce buffers for small arrays, one copy kernel per direction, results handed
// to the caller after the ONE stream synchronisation of a call (xc_sync).  See xc_ctx in xc_internal.h for the state.
#include "xc_capi.h"
#include <string.h>
#include <time.h>

namespace xc {

constexpr size_t kPinBytes = (size_t)4 << 20;        // each bounce buffer
constexpr size_t kPinSmall = (size_t)1 << 20;        // transfers up to this size take the bounce buffers
constexpr size_t kCopyKernelMax = (size_t)64 << 10;  // ... and INPUTS up to this size are moved by k_copy_small, up to eight arrays per launch, instead of one DMA copy each (results: knobs.copy_out_kb)

static inline double now_s()
{
    struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

static int ensure_pins(xc_ctx* ctx)
{
    if (ctx->pin_in) return XC_OK;
    // coherent (fine-grained) on request, not by the runtime's default: kernels read pin_in and write pin_out themselves (k_copy_small, the
    // direct results), and what the host sees after the stream wait must not depend on HIP_HOST_COHERENT
    XC_HIP(ctx, hipHostMalloc((void**)&ctx->pin_in, kPinBytes, hipHostMallocCoherent));
    hipError_t e = hipHostMalloc((void**)&ctx->pin_out, kPinBytes, hipHostMallocCoherent);
    if (e != hipSuccess) { (void)hipHostFree(ctx->pin_in); ctx->pin_in = nullptr; return hipfail(ctx, e, "hipHostMalloc"); }
    return XC_OK;
}

// host bytes -> device on the compute stream.  Small blocks: memcpy into the pinned input buffer + an asynchronous copy (the slot is
// free again after the call's xc_sync); larger ones: the runtime's own staged copy straight from the caller's memory.
static int h2d_raw(xc_ctx* ctx, void* d, const void* h, size_t n)
{
    if (n <= kPinSmall && ensure_pins(ctx) == XC_OK && ctx->pin_in_off + n <= kPinBytes) {
        char* p = ctx->pin_in + ctx->pin_in_off;
        ctx->pin_in_off += (n + 63) & ~(size_t)63;
        memcpy(p, h, n);
        if (ctx->knobs.copy_kernel && n <= kCopyKernelMax) { if (n) ctx->pending_in.push_back({d, p, n}); return XC_OK; }   // leaves with flush_in
        XC_HIP(ctx, hipMemcpyAsync(d, p, n, hipMemcpyHostToDevice, ctx->stream));
        return XC_OK;
    }
    XC_HIP(ctx, hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, ctx->stream));
    return XC_OK;
}

// the staged small inputs go to the device now: called by every host-form entry point between its staging and its first launch (and by
// xc_sync, so that nothing staged can outlive the call)
int flush_in(xc_ctx* ctx)
{
    int rc = XC_OK;
    for (size_t i = 0; i < ctx->pending_in.size() && rc == XC_OK; i += 8) {
        SmallCopies c; int m = 0;
        for (; m < 8 && i + m < ctx->pending_in.size(); ++m) {
            const auto& e = ctx->pending_in[i + m];
            c.src[m] = e.pinned; c.dst[m] = e.dev; c.bytes[m] = (unsigned)e.bytes;
        }
        for (int k = m; k < 8; ++k) { c.src[k] = nullptr; c.dst[k] = nullptr; c.bytes[k] = 0; }
        rc = launch_copy_small(ctx, c, m);
    }
    ctx->pending_in.clear();
    return rc;
}
// ... and the small results the call has asked for leave the device in one launch (xc_sync, before it waits for the stream)
static int flush_out(xc_ctx* ctx)
{
    SmallCopies c; int m = 0, rc = XC_OK;
    for (auto& po : ctx->pending_out) {
        if (!po.dev) continue;
        c.src[m] = po.dev; c.dst[m] = const_cast<void*>(po.pinned); c.bytes[m] = (unsigned)po.bytes; po.dev = nullptr;
        if (++m == 8) { if (rc == XC_OK) rc = launch_copy_small(ctx, c, m); m = 0; }
    }
    if (m) {
        for (int k = m; k < 8; ++k) { c.src[k] = nullptr; c.dst[k] = nullptr; c.bytes[k] = 0; }
        if (rc == XC_OK) rc = launch_copy_small(ctx, c, m);
    }
    return rc;
}

// every host-form entry point stages its inputs through here: bytes that have a device mirror are copied from the mirror
// (device to device, ~50 us for a cfg2 slab) instead of crossing PCIe again (~1 ms)
int h2d(xc_ctx* ctx, void* d, const void* h, size_t n)
{
    const double t0 = now_s();
    int rc = XC_OK;
    const void* m = ctx->resident.empty() ? nullptr : resident_lookup(ctx, h, n);
    if (m) { hipError_t e = hipMemcpyAsync(d, m, n, hipMemcpyDeviceToDevice, ctx->stream); if (e != hipSuccess) rc = hipfail(ctx, e, "hipMemcpyAsync(d2d)"); }
    else rc = h2d_raw(ctx, d, h, n);
    ctx->tr_h2d += now_s() - t0;
    return rc;
}
// the big read-only inputs of the Keff sequence skip even that copy: the kernel reads the mirror itself (`slot`: the arena bytes
// reserved for the upload, unused then)
int stage_in(xc_ctx* ctx, void* slot, const void* h, size_t n, const void** dev)
{
    if (!ctx->resident.empty())
        if (const void* m = resident_lookup(ctx, h, n)) { *dev = m; return XC_OK; }
    *dev = slot;
    const double t0 = now_s();
    const int rc = h2d_raw(ctx, slot, h, n);
    ctx->tr_h2d += now_s() - t0;
    return rc;
}
// a SMALL read-only input (see xc_ctx::SmallIn): the device copy of an earlier call when the bytes are the same, else an upload into a cache
// entry (through the pinned buffer and the copy kernel, like every small input) that later calls can hit
int stage_small(xc_ctx* ctx, void* slot, const void* h, size_t n, const void** dev)
{
    if (!ctx->resident.empty())
        if (const void* m = resident_lookup(ctx, h, n)) { *dev = m; return XC_OK; }
    if (ctx->knobs.copy_kernel && n > 0 && n <= kCopyKernelMax) {
        const double t0 = now_s();
        xc_ctx::SmallIn* lru = nullptr;
        for (auto& e : ctx->small_in) {
            if (e.dev && e.host.size() == n && memcmp(e.host.data(), h, n) == 0) {
                e.used = ++ctx->small_clock; e.epoch = ctx->small_epoch; ++ctx->small_hits;
                *dev = e.dev; ctx->tr_h2d += now_s() - t0;
                return XC_OK;
            }
            if (e.epoch != ctx->small_epoch && (!lru || e.used < lru->used)) lru = &e;
        }
        if (lru && ensure_pins(ctx) == XC_OK && ctx->pin_in_off + n <= kPinBytes) {
            if (!lru->dev) { hipError_t he = hipMalloc(&lru->dev, kCopyKernelMax); if (he != hipSuccess) { lru->dev = nullptr; (void)hipGetLastError(); } }
            if (lru->dev) {
                lru->host.assign((const char*)h, (const char*)h + n);
                lru->used = ++ctx->small_clock; lru->epoch = ctx->small_epoch; ++ctx->small_misses;
                char* p = ctx->pin_in + ctx->pin_in_off;
                ctx->pin_in_off += (n + 63) & ~(size_t)63;
                memcpy(p, h, n);
                ctx->pending_in.push_back({lru->dev, p, n});
                *dev = lru->dev; ctx->tr_h2d += now_s() - t0;
                return XC_OK;
            }
        }
    }
    *dev = slot;
    const double t0 = now_s();
    const int rc = h2d_raw(ctx, slot, h, n);
    ctx->tr_h2d += now_s() - t0;
    return rc;
}
// device -> the caller's host array.  Small results wait in the pinned output buffer and are handed over by xc_sync (EVERY host-form
// entry point ends in xc_sync): the copies of a call are asynchronous and its stream is waited for once.
int d2h(xc_ctx* ctx, void* h, const void* d, size_t n)
{
    const double t0 = now_s();
    int rc = XC_OK;
    if (n <= kPinSmall && ensure_pins(ctx) == XC_OK && ctx->pin_out_off + n <= kPinBytes) {
        char* p = ctx->pin_out + ctx->pin_out_off;
        ctx->pin_out_off += (n + 63) & ~(size_t)63;
        if (ctx->knobs.copy_kernel && n <= (size_t)ctx->knobs.copy_out_kb << 10) {
            if (n) ctx->pending_out.push_back({h, p, n, d});         // fetched by flush_out: every caller goes on to xc_sync without another launch on `d`
        } else {
            hipError_t e = hipMemcpyAsync(p, d, n, hipMemcpyDeviceToHost, ctx->stream);
            if (e != hipSuccess) rc = hipfail(ctx, e, "hipMemcpyAsync(d2h)");
            else ctx->pending_out.push_back({h, p, n, nullptr});
        }
    } else {
        hipError_t e = hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, ctx->stream);
        if (e != hipSuccess) rc = hipfail(ctx, e, "hipMemcpyAsync(d2h)");
    }
    ctx->tr_d2h += now_s() - t0;
    return rc;
}

// where the kernels of a host-form call write a SMALL result the caller wants in `h`: straight into the pinned output buffer -- the device
// writes host memory through the same pointer, xc_sync hands it over, and the stream carries no copy of any kind for it.  Only for outputs
// that are written once and never read back by a kernel.  nullptr: too large / buffer full / switched off -- arena bytes and d2h() then.
void* out_direct(xc_ctx* ctx, void* h, size_t n)
{
    if (!h || !ctx->knobs.copy_kernel || n == 0 || n > ((size_t)ctx->knobs.copy_out_kb << 10) || ensure_pins(ctx) != XC_OK || ctx->pin_out_off + n > kPinBytes) return nullptr;
    char* p = ctx->pin_out + ctx->pin_out_off;
    ctx->pin_out_off += (n + 63) & ~(size_t)63;
    ctx->pending_out.push_back({h, p, n, nullptr});
    return p;
}

}  // namespace xc

using namespace xc;

extern "C" {

int xc_sync(xc_ctx* ctx)
{
    XC_CTX(ctx);
    { const int rc = flush_in(ctx); if (rc != XC_OK) return rc; }
    { const int rc = flush_out(ctx); if (rc != XC_OK) return rc; }
    const double t0 = now_s();
    // (round 6: polling hipStreamQuery for the first 150 us instead of blocking at once changes nothing -- 369 against 374 us for the
    // reference's call sequence at its demo size: the runtime's own wait already spins)
    const hipError_t e = hipStreamSynchronize(ctx->stream);
    const double t1 = now_s();
    ctx->tr_sync += t1 - t0;
    // results parked in the pinned output buffer go to the caller's arrays now; both bounce buffers are free again
    if (e == hipSuccess) for (const auto& po : ctx->pending_out) memcpy(po.host, po.pinned, po.bytes);
    ctx->pending_out.clear(); ctx->pending_in.clear();
    ctx->pin_in_off = 0; ctx->pin_out_off = 0;
    ++ctx->small_epoch;
    ctx->tr_d2h += now_s() - t1;
    if (e != hipSuccess) return hipfail(ctx, e, "hipStreamSynchronize");
    return XC_OK;
}

int xc_trace(xc_ctx* ctx, int reset, double* out3)
{
    if (!ctx) return fail(nullptr, XC_EBADARG, "null context");
    if (out3) { out3[0] = ctx->tr_h2d; out3[1] = ctx->tr_d2h; out3[2] = ctx->tr_sync; }
    if (reset) ctx->tr_h2d = ctx->tr_d2h = ctx->tr_sync = 0.0;
    return XC_OK;
}

}  // extern "C"

// What the translation units behind the C ABI share: xc_context.hip (context, device memory, events), xc_transport.hip (pinned bounce
// buffers, xc_sync), xc_keff.hip (the Keff chain), xc_forms.hip (the host forms of the other kernels) and the launchers that lay out a
// device block.  A layout is stated once: lay_out for the kernel scratch and the piece workspaces, lay_stage (xc_stage.h) for the arena.
#pragma once
#include "xc_internal.h"
#include "xc_stage.h"
#include <utility>
#include <vector>

namespace xc {

inline size_t esize(int dtype) { return dtype == XC_F32 ? 4 : 8; }
inline bool is_float(int dtype) { return dtype == XC_F32 || dtype == XC_F64; }
// bytes of a weight array of the given rank (XC_DA_NONE: none)
inline size_t dA_bytes(int rank, int64_t nslab, int64_t ny, int64_t nx)
{
    return rank == XC_DA_ROW ? (size_t)ny * 8 : rank == XC_DA_PLANE ? (size_t)ny * nx * 8 : rank == XC_DA_SLAB ? (size_t)nslab * ny * nx * 8 : 0;
}

#define XC_TRY(expr) do { int _rc = (expr); if (_rc != XC_OK) return _rc; } while (0)
#define XC_CTX(ctx) do { if (!(ctx)) return xc::fail(nullptr, XC_EBADARG, "null context"); \
                         hipError_t _e = hipSetDevice((ctx)->device); \
                         if (_e != hipSuccess) return xc::hipfail((ctx), _e, "hipSetDevice"); } while (0)

// Where the time of one launcher call goes (xc_set_kernel_timing): an event between its stages, and after the call the time between two
// marks added to ms[kind of the later mark].  Nothing happens without ctx->timing; kind -1 opens an interval without booking it; an event
// call that fails is ignored.  The times are booked and the events destroyed when the timer goes out of scope, on whichever return: an
// interval whose events have not completed by then (a call that fails before its last wait) books nothing.
struct StageTimer {
    xc_ctx* ctx; float* ms;
    std::vector<std::pair<hipEvent_t, int>> marks;
    StageTimer(xc_ctx* c, float* m) : ctx(c), ms(m) {}
    StageTimer(const StageTimer&) = delete;
    StageTimer& operator=(const StageTimer&) = delete;
    void mark(int kind)
    {
        if (!ctx->timing) return;
        hipEvent_t ev;
        if (hipEventCreate(&ev) != hipSuccess) return;
        (void)hipEventRecord(ev, ctx->stream);
        marks.push_back({ev, kind});
    }
    ~StageTimer()
    {
        bool pending = false;
        for (size_t k = 1; k < marks.size(); ++k) {
            float t = 0.f;
            if (marks[k].second < 0) continue;
            if (hipEventElapsedTime(&t, marks[k - 1].first, marks[k].first) == hipSuccess) ms[marks[k].second] += t;
            else pending = true;
        }
        if (pending) (void)hipGetLastError();                           // "not ready" is no error of the next call
        for (auto& m : marks) (void)hipEventDestroy(m.first);
    }
};

// ---------------------------------------------------------------- xc_context.hip
int grow(xc_ctx* ctx, void** p, size_t* have, size_t need);          // the grow-only rule of ensure_* for any device block of the context
// a layout (xc_carve.h) over such a block: measured, the block grown to it, then placed
template <typename Lay> int lay_out(xc_ctx* ctx, void** p, size_t* have, Lay&& lay) { XC_TRY(grow(ctx, p, have, lay(Carve()))); lay(Carve(*p)); return XC_OK; }
void mm_touch(xc_ctx* ctx, const void* p, size_t bytes);             // a write into / the release of [p, p + bytes) drops chained min/max partials of it
const void* resident_lookup(const xc_ctx* ctx, const void* h, size_t n);   // device mirror of the host bytes [h, h + n) (xc_keep_resident), or null
int hist_ev_begin(xc_ctx* ctx);                                      // events around the dominant kernel (xc_set_kernel_timing, xc_set_hist_events)
int hist_ev_end(xc_ctx* ctx);

// ---------------------------------------------------------------- xc_transport.hip: how a host-form entry point moves its arrays
int h2d(xc_ctx* ctx, void* d, const void* h, size_t n);                                  // input copied to `d` (from its device mirror if it has one)
int stage_in(xc_ctx* ctx, void* slot, const void* h, size_t n, const void** dev);       // big read-only input: *dev = its mirror, else `slot` after an upload
int stage_small(xc_ctx* ctx, void* slot, const void* h, size_t n, const void** dev);    // small read-only input: mirror, content cache, else `slot`
int flush_in(xc_ctx* ctx);                                                               // between the staging and the first launch
// (d2h, out_direct and Stage, the arena blocks of one host-form call with lay_stage, its layout stated once: xc_stage.h)

}  // namespace xc

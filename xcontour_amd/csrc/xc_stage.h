// One host-form call on the staging arena, its layout stated once.  A form writes the blocks it stages through and the results it owes its
// caller as one function lay(Stage&) that only takes blocks and fills the form's device pointers; lay_stage runs it twice, as lay_out
// (xc_capi.h) runs a Carve layout: over a measuring Stage (null base), then -- the arena grown to what that measured, before the call's first
// copy is enqueued: the arena may not move inside a call -- over the arena.  Measuring has no side effects: it consumes no pinned bytes, queues
// no hand-over and leaves outs[] empty; a result that out_direct may place in the pinned buffer counts its arena bytes, so the measured total is
// never below what placing takes.  Plain C++17, no HIP header (tests/test_stage_host.py runs it sanitized over stand-ins of the three functions).
#pragma once
#include "xc_carve.h"
#include <assert.h>

struct xc_ctx;

namespace xc {

int ensure_arena(xc_ctx* ctx, size_t bytes, void** base);   // xc_context.hip: the grow-only arena of at least `bytes`; lay_stage is its only caller
int d2h(xc_ctx* ctx, void* h, const void* d, size_t n);     // xc_transport.hip: result for the caller's array, handed over by xc_sync
void* out_direct(xc_ctx* ctx, void* h, size_t n);           // xc_transport.hip: pinned bytes the kernels may write `h`'s result into, or null

struct Stage {                       // c.base == nullptr: measuring
    struct Out { void* host; const void* dev; size_t bytes; };
    xc_ctx* ctx; Carve c; Out outs[10]; int nout = 0;
    explicit Stage(xc_ctx* x, void* base = nullptr) : ctx(x), c(base) {}
    template <typename T = void> T* take(size_t bytes) { return (T*)c.take<char>(bytes); }
    // Where the kernels write a result the caller wants in `host`: for results written once and never read back by a kernel (`direct_ok`) a
    // slot of the pinned output buffer where out_direct grants one, else arena bytes that deliver() fetches.  Null when `host` is null ...
    template <typename T> T* out(T* host, size_t bytes, bool direct_ok = false) { return host ? keep(host, bytes, direct_ok) : nullptr; }
    // ... or, for a buffer the kernels write whether or not the caller wants it back, arena bytes nobody fetches
    template <typename T> T* keep(T* host, size_t bytes, bool direct_ok = false)
    {
        if (c.base && host && direct_ok) if (void* p = out_direct(ctx, host, bytes)) return (T*)p;
        T* d = take<T>(bytes);
        if (c.base && host) { assert(nout < 10); outs[nout++] = {host, d, bytes}; }
        return d;
    }
    // after the last launch: the copies of every arena-backed result, in the order they were asked for; the caller ends in xc_sync
    int deliver() { for (int i = 0; i < nout; ++i) if (int rc = d2h(ctx, outs[i].host, outs[i].dev, outs[i].bytes)) return rc; return 0; }
};

template <typename Lay> int lay_stage(Stage& st, Lay&& lay)
{
    Stage m(st.ctx); lay(m);
    void* base; if (int rc = ensure_arena(st.ctx, m.c.at, &base)) return rc;
    assert(base); st.c = Carve(base); lay(st);                 // (a null base would make the placing pass a measuring one)
    return 0;
}

}  // namespace xc

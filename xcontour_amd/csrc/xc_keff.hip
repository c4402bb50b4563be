// C ABI, part 3: the Keff chain -- K1 (min / max), the levels, the histogram pass (K3) with its reduction and the Keff epilogue (K5 / K6):
// xc_minmax, xc_levels, xc_contours, xc_hist, xc_keff_epilogue, xc_keff_dev and the records of what they launched.  The kernels are in
// xc_misc.hip, xc_hist.hip, xc_hist_det.hip and xc_keff1.hip.
#include "xc_capi.h"
#include <string.h>

using namespace xc;

// The 2-cells-per-lane kernels issue 16-byte (f64) / 8-byte (f32) loads from EVERY streamed array:
// OR the low address bits of all of them so that hist_geometry can fall back to 1 cell per lane
// when any base is not suitably aligned (e.g. a slab offset inside a caller's buffer).
static const void* vec_align_bits(const void* q, int q_dtype, const void* q_next, const double* dA, int dA_rank,
                                  const void* const* integ, const int32_t* integ_dtype, int nint)
{
    uintptr_t bits = reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(q_next);
    // f64 arrays need 16-byte alignment; express it in q's units: for f32 q (8-byte requirement) an
    // f64 array that is only 8-byte aligned must still force the fallback
    auto need16 = [&](const void* p) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        if (a % 16 != 0) bits |= (q_dtype == XC_F32) ? 4 : 8;   // make (bits % (2*esz)) != 0
    };
    if (dA && (dA_rank == XC_DA_PLANE || dA_rank == XC_DA_SLAB)) need16(dA);
    for (int i = 0; i < nint; ++i) {
        if (integ_dtype[i] == XC_F64) need16(integ[i]);
        else if (reinterpret_cast<uintptr_t>(integ[i]) % 8 != 0) bits |= (q_dtype == XC_F32) ? 4 : 8;
    }
    return reinterpret_cast<const void*>(bits);
}

static int check_hist_desc(xc_ctx* ctx, const xc_hist_desc* d)
{
    if (!d) return fail(ctx, XC_EBADARG, "xc_hist: desc is NULL");
    if (!d->q || !d->edges) return fail(ctx, XC_EBADARG, "xc_hist: q / edges is NULL");
    if (!is_float(d->q_dtype)) return fail(ctx, XC_EBADARG, "xc_hist: q_dtype must be XC_F32 or XC_F64");
    if (d->nslab < 1 || d->ny < 1 || d->nx < 1) return fail(ctx, XC_EBADARG, "xc_hist: nslab, ny, nx must be >= 1");
    if (d->nedge < 2) return fail(ctx, XC_EBADARG, "xc_hist: need at least 2 edges");
    if (d->dA_rank < XC_DA_NONE || d->dA_rank > XC_DA_SLAB) return fail(ctx, XC_EBADARG, "xc_hist: bad dA_rank");
    if (d->dA_rank != XC_DA_NONE && !d->dA) return fail(ctx, XC_EBADARG, "xc_hist: dA is NULL");
    if (d->nint < 0 || d->nint > XC_MAX_INTEGRANDS) return fail(ctx, XC_EBADARG, "xc_hist: nint must be 0..2");
    for (int i = 0; i < d->nint; ++i) {
        if (!d->integrand[i]) return fail(ctx, XC_EBADARG, "xc_hist: integrand is NULL");
        if (!is_float(d->integrand_dtype[i])) return fail(ctx, XC_EBADARG, "xc_hist: bad integrand dtype");
    }
    if (d->grad && (!d->rdx || !d->rdy)) return fail(ctx, XC_EBADARG, "xc_hist: grad needs rdx and rdy");
    if (d->grad && d->negate) return fail(ctx, XC_EBADARG, "xc_hist: negate is not available together with grad");
    if (!d->pdf && !d->counts && !d->cdf) return fail(ctx, XC_EBADARG, "xc_hist: no output requested");
    return XC_OK;
}

// K1's min / max partials of `nslab` slabs as a block of a layout -- and as the whole scratch of a call that runs K1 alone (xc_minmax_dev, xc_contours)
static double* k1_part(Carve& c, int64_t nslab) { return c.take<double>((size_t)nslab * kMinmaxBlocks * 2); }
static int k1_scratch(xc_ctx* ctx, int64_t nslab, double** part)
{
    return lay_out(ctx, &ctx->scratch, &ctx->scratch_bytes, [&](Carve c) { *part = k1_part(c, nslab); return c.at; });
}

// The scratch of one K3 call, one layout in this order: K1's min / max partials (the chain only; the base of the block either way), the blocks'
// partial sums and counts, the per-slab reduced sums and counts (adjacent: the few-slab path clears both as acc_words words from red_h), and
// for the deterministic sums the window constants and the bounds det_one_pass takes: K1 partials of one array at a time + (min, max) pairs
// of dA, the tracer, the integrands (det_pair 0, 1, 2..).  A block a mode does not use has no bytes.
struct K3Scratch {
    double *mmpart, *part_h, *red_h, *det_part, *det_pair[3 + XC_MAX_INTEGRANDS];
    unsigned* part_c; unsigned long long* red_c; int* c0; size_t part_c_bytes; int64_t acc_words;
    // own_part_h = false: the partial sums are the caller's own array (the stand-alone epilogue reduces ONE partial per slab, the pdf)
    int reserve(xc_ctx* ctx, int64_t nslab, int bps, int nch, int nbin, int det, bool minmax_partials, bool own_part_h = true)
    {
        const size_t S = (size_t)nslab;
        return lay_out(ctx, &ctx->scratch, &ctx->scratch_bytes, [&](Carve c) {
            mmpart = k1_part(c, minmax_partials ? nslab : 0);
            // (deterministic sums: a block's partial is the limbs of its superaccumulators instead of one double per channel)
            part_h = c.take<double>(own_part_h ? S * bps * (det ? det_limbs_total(nch) : nch) * nbin : 0);
            const size_t m0 = c.mark(); part_c = c.take<unsigned>(S * bps * nbin); const size_t m1 = c.mark();
            red_h = c.take<double>(S * nch * nbin); red_c = c.take<unsigned long long>(S * nbin);
            part_c_bytes = m1 - m0; acc_words = (int64_t)((c.mark() - m1) / 8);
            c0 = c.take<int>(det ? S * nch : 0); det_part = k1_part(c, det ? nslab : 0);
            for (double*& p : det_pair) p = c.take<double>(det ? S * 2 : 0);
            return c.at;
        });
    }
};

// the weights a kernel reads (HistArgs, SingleArgs): XC_DA_NONE becomes one 1.0 per row, finite and positive whatever the caller said
template <typename Desc, typename Args>
static int set_weights(xc_ctx* ctx, const Desc* d, Args& a)
{
    a.dA = d->dA; a.dA_rank = d->dA_rank; a.dA_pos_finite = d->dA_pos_finite;
    if (d->dA_rank != XC_DA_NONE) return XC_OK;
    XC_TRY(ensure_ones(ctx, (size_t)d->ny));
    a.dA = ctx->ones; a.dA_rank = XC_DA_ROW; a.dA_pos_finite = 1;
    return XC_OK;
}

// what xc_hist_desc and xc_keff_desc say alike about a histogram pass, and where its partials and its reduction go
template <typename Desc>
static int hist_common(xc_ctx* ctx, const Desc* d, int nch, int nbin, const HistGeom& g, const K3Scratch& L, HistArgs& a, FinalArgs& f)
{
    XC_TRY(set_weights(ctx, d, a));
    a.q = d->q; a.q_f32 = d->q_dtype == XC_F32; a.prod_f32 = d->prod_f32;
    a.rdx = d->rdx; a.rdy = d->rdy; a.periodic_x = d->periodic_x;
    a.ny = d->ny; a.nx = d->nx; a.nstrip = g.nstrip; a.ncopy = g.ncopy; a.nbin = nbin;
    // nobody asked for counts: the histogram pass skips their LDS adds (a third of its atomics)
    a.part_h = L.part_h; a.part_c = (d->counts || d->deterministic) ? L.part_c : nullptr;
    f.part_h = a.part_h; f.part_c = a.part_c; f.bps = g.bps; f.nch = nch; f.nbin = nbin;
    f.red_h = L.red_h; f.red_c = L.red_c;
    f.lt = d->lt; f.counts = d->counts;
    return XC_OK;
}

// The Keff epilogue of launch_finalize (channel 0 = area, channel 1 = intgrdS), for all three callers.  vstride: doubles between consecutive
// slabs in ctr and the vector outputs (0: N); ntbl: length of the table.
static void keff_final(FinalArgs& f, const xc_keff_desc* d, int vstride, int ntbl)
{
    f.lt = d->lt; f.reverse = !d->increase;       // decreasing levels -> flip to level order (core.py:454-455)
    f.keff = 1; f.ctr_f32 = d->ctr_dtype == XC_F32; f.ctr = d->ctr; f.vstride = vstride;
    f.tbl = d->tbl; f.tbl_coord = d->tbl_coord; f.ntbl = ntbl;
    f.preY = d->preY; f.npre = d->interp ? d->npre : 0;
    f.nkeff_mask = d->nkeff_mask; f.lmin_scale = d->lmin_scale;
    f.o_area = d->area; f.o_intS = d->intgrdS; f.o_latEq = d->latEq; f.o_dqdA = d->dqdA; f.o_dSdA = d->dintSdA;
    f.o_Leq2 = d->Leq2; f.o_Lmin = d->Lmin; f.o_nkeff = d->nkeff; f.o_interp = d->interp;
}

// Deterministic sums in ONE histogram pass (xc_binning.h, xc_hist_det.hip): the bounds that fix every channel's accumulator window
// come first -- max |dA| from the caller or from a min / max pass over the dA array, the extrema of every supplied integrand
// (and of the tracer, for the in-kernel gradient with explicit edges) from K1 passes of their own -- then the pass, then the exact
// reduction of the blocks' limbs into f.red_h / f.red_c; launch_finalize runs its second stage only.
static int det_one_pass(xc_ctx* ctx, int q_dtype, int nint, int grad, const HistGeom& g, int64_t nslab, int64_t ny, int64_t nx,
                        HistArgs& a, const K3Scratch& L, double dA_max_host, const void* const* integ, const int* integ_dtype, FinalArgs& f)
{
    double* part = L.det_part;
    auto extrema = [&](const void* p, int dtype, int64_t ns, int64_t ncell, double* out) -> int {
        // (the bounds of the accumulator windows: the largest FINITE magnitudes -- an infinite weight flags its own bin, it must not push
        // every finite one out of the window; the oracle takes its bounds the same way)
        XC_TRY(launch_minmax_partial(ctx, p, dtype, ns, ncell, part, nullptr, 0, true));
        return launch_minmax_final(ctx, part, ns, minmax_blocks(ncell, ns), out);
    };
    a.det_dA_max = -1.0; a.det_dA_max_dev = nullptr; a.det_dA_stride = 0;
    if (dA_max_host > 0.0 && dA_max_host < __builtin_inf()) a.det_dA_max = dA_max_host;
    else if (a.dA == ctx->ones) a.det_dA_max = 1.0;
    else {
        double* out = L.det_pair[0];
        const int64_t ns = a.dA_rank == XC_DA_SLAB ? nslab : 1, ncell = a.dA_rank == XC_DA_ROW ? ny : ny * nx;
        XC_TRY(extrema(a.dA, XC_F64, ns, ncell, out));
        a.det_dA_max_dev = out; a.det_dA_stride = a.dA_rank == XC_DA_SLAB ? 1 : 0;
    }
    a.det_q_mm = nullptr;
    if (grad && !a.levels_mode) {
        double* out = L.det_pair[1];
        XC_TRY(extrema(a.q, q_dtype, nslab, ny * nx, out));
        a.det_q_mm = out;
    }
    for (int i = 0; i < nint; ++i) {
        double* out = L.det_pair[2 + i];
        XC_TRY(extrema(integ[i], integ_dtype[i], nslab, ny * nx, out));
        a.det_int_mm[i] = out;
    }
    a.det_c0_out = L.c0;
    XC_TRY(launch_hist_det3(ctx, q_dtype, nint, grad, g, nslab, a));
    XC_TRY(launch_det3_reduce(ctx, nslab, g.bps, f.nch, f.nbin, a.part_h, a.part_c, L.c0, f.red_h, f.red_c));
    f.skip_reduce = 1;
    return XC_OK;
}

// xc_last_hist_variant: launch_three / launch_s4 write the record where they launch; a call that fails leaves it cleared
static int hist_recorded(xc_ctx* ctx, int rc)
{
    if (rc != XC_OK && ctx) ctx->last_hist = xc_hist_variant{};
    return rc;
}

static int hist_dev(xc_ctx* ctx, const xc_hist_desc* d)
{
    XC_TRY(check_hist_desc(ctx, d));
    const int nbin = (int)(d->nedge - 1), nch = 1 + d->nint + (d->grad ? 1 : 0);
    HistGeom g;
    const int det = d->deterministic ? 1 : 0;
    XC_TRY(hist_geometry(ctx, d->q_dtype, d->nslab, d->ny, d->nx, nbin, nch,
                         vec_align_bits(d->q, d->q_dtype, nullptr, d->dA, d->dA_rank, d->integrand, d->integrand_dtype, d->nint), &g, 0, det));
    K3Scratch L;
    XC_TRY(L.reserve(ctx, d->nslab, g.bps, nch, nbin, det, false));
    ctx->mm_valid = 0;                          // (the scratch may have moved)
    HistArgs a; memset(&a, 0, sizeof(a));
    FinalArgs f; memset(&f, 0, sizeof(f));
    XC_TRY(hist_common(ctx, d, nch, nbin, g, L, a, f));
    for (int i = 0; i < d->nint; ++i) { a.integ[i] = d->integrand[i]; a.integ_f32[i] = d->integrand_dtype[i] == XC_F32; }
    a.edges = d->edges; a.levels_mode = 0; a.edges_per_slab = d->edges_per_slab;
    a.last_closed = d->last_closed; a.negate = d->negate;
    f.reverse = d->reverse; f.pdf = d->pdf; f.cdf = d->cdf;
    XC_TRY(hist_ev_begin(ctx));
    if (det) {
        XC_TRY(det_one_pass(ctx, d->q_dtype, d->nint, d->grad, g, d->nslab, d->ny, d->nx, a, L, 0.0, d->integrand, d->integrand_dtype, f));
    } else {
        XC_TRY(launch_hist(ctx, d->q_dtype, d->nint, d->grad, g, d->nslab, a));
    }
    XC_TRY(hist_ev_end(ctx));
    return launch_finalize(ctx, d->nslab, f);
}

static int hist_host(xc_ctx* ctx, const xc_hist_desc* hd)
{
    XC_TRY(check_hist_desc(ctx, hd));
    const int64_t S = hd->nslab, ny = hd->ny, nx = hd->nx, ne = hd->nedge;
    const int nbin = (int)(ne - 1), nch = 1 + hd->nint + (hd->grad ? 1 : 0);
    const int64_t nes = hd->edges_per_slab ? S : 1;
    // reference: 'non monotonic bins' (core.py:1233-1251); np.digitize needs monotone edges.
    // NaN edges are let through (an all-NaN slab yields NaN levels and an empty histogram).
    for (int64_t s = 0; s < nes; ++s)
        for (int64_t k = 1; k < ne; ++k) {
            const double e0 = hd->edges[s * ne + k - 1], e1 = hd->edges[s * ne + k];
            if (e1 <= e0) return fail(ctx, XC_EEDGES, "non monotonic bins");
        }
    const size_t cells = (size_t)S * ny * nx;
    const size_t qb = cells * esize(hd->q_dtype), eb = (size_t)nes * ne * 8;
    const size_t dab = dA_bytes(hd->dA_rank, S, ny, nx);
    size_t ib[XC_MAX_INTEGRANDS] = {0, 0};
    for (int i = 0; i < hd->nint; ++i) ib[i] = cells * esize(hd->integrand_dtype[i]);
    const size_t rb = hd->grad ? (size_t)ny * 8 : 0;
    const size_t pb = (size_t)S * nch * nbin * 8, cb = (size_t)S * nbin * 8;
    Stage st(ctx); xc_hist_desc d = *hd; void *sq, *se, *sd = nullptr, *si[XC_MAX_INTEGRANDS], *sx = nullptr, *sy = nullptr; const void* p;
    XC_TRY(lay_stage(st, [&](Stage& s) {
        sq = s.take(qb); se = s.take(eb); if (dab) sd = s.take(dab);
        for (int i = 0; i < hd->nint; ++i) si[i] = s.take(ib[i]);
        if (hd->grad) { sx = s.take(rb); sy = s.take(rb); }
        // (the finalize kernel writes the three results once and reads none of them back: small ones go straight to the pinned buffer)
        d.pdf = s.out(hd->pdf, pb, true); d.cdf = s.out(hd->cdf, pb, true); d.counts = s.out(hd->counts, cb, true);
    }));
    XC_TRY(stage_in(ctx, sq, hd->q, qb, &d.q));
    XC_TRY(stage_small(ctx, se, hd->edges, eb, &p)); d.edges = (const double*)p;
    if (dab) { XC_TRY(stage_in(ctx, sd, hd->dA, dab, &p)); d.dA = (const double*)p; }
    for (int i = 0; i < hd->nint; ++i) XC_TRY(stage_in(ctx, si[i], hd->integrand[i], ib[i], &d.integrand[i]));
    if (hd->grad) {
        XC_TRY(stage_small(ctx, sx, hd->rdx, rb, &p)); d.rdx = (const double*)p;
        XC_TRY(stage_small(ctx, sy, hd->rdy, rb, &p)); d.rdy = (const double*)p;
    }
    XC_TRY(flush_in(ctx));
    XC_TRY(xc_hist_dev(ctx, &d));
    XC_TRY(st.deliver());
    return xc_sync(ctx);
}

// ------------------------------------------------------------------------------------ fused Keff pipeline
constexpr int XC_EAGAIN = -1000;      // internal: "not this path" (never leaves the library)

static int keff_single(xc_ctx* ctx, const xc_keff_desc* d)
{
    const int N = d->N;
    const int vstride = d->out_stride ? d->out_stride : N;
    SingleArgs a; memset(&a, 0, sizeof(a));
    XC_TRY(set_weights(ctx, d, a));
    SingleGeom g;
    if (!single_geometry(ctx, d->q_dtype, d->nslab, d->ny, d->nx, N, d->q, a.dA, a.dA_rank, &g)) return XC_EAGAIN;
    if (!ctx->single_ws) {
        XC_HIP(ctx, hipMalloc(&ctx->single_ws, 2 * sizeof(SingleSet)));
        XC_HIP(ctx, hipMemsetAsync(ctx->single_ws, 0, 2 * sizeof(SingleSet), ctx->stream));
        ctx->single_launches = 0; ctx->single_dirty_bins[0] = ctx->single_dirty_bins[1] = 0;
    }
    const unsigned cur = ctx->single_launches & 1u;
    SingleSet* sets = (SingleSet*)ctx->single_ws;
    a.q = d->q; a.rdx = d->rdx; a.rdy = d->rdy; a.periodic_x = d->periodic_x;
    a.ny = d->ny; a.nx = d->nx; a.nslab = (int)d->nslab;
    a.nbin = N; a.ncopy = g.ncopy; a.increase = d->increase; a.q_f32 = d->q_dtype == XC_F32; a.ctr_f32 = d->ctr_dtype == XC_F32;
    a.right_edge = d->right_edge; a.last_closed = d->right_edge == XC_EDGE_NUMPY; a.want_counts = d->counts ? 1 : 0;
    a.inv_nm1 = 1.0 / (double)(N - 1); a.inv_n = 1.0 / (double)N;
    a.G = g.G; a.nstrip = g.nstrip; a.cps = g.cps; a.rpc = g.rpc; a.strip_fast = ctx->knobs.single_map;
    a.cur = sets + cur; a.other = sets + (1u - cur); a.other_dirty_bins = ctx->single_dirty_bins[1u - cur];
    a.ctr_out = d->ctr; a.ctr_stride = vstride; a.status = d->status;
    a.timeout_ticks = (unsigned long long)(ctx->knobs.single_timeout_us > 0 ? ctx->knobs.single_timeout_us : 1) * 100ull;   // 100 MHz wall clock
    a.stamps = ctx->single_stamps;
    FinalArgs f; memset(&f, 0, sizeof(f));
    f.bps = 1; f.nch = 2; f.nbin = N; f.skip_reduce = 1;
    f.red_h = a.cur->acc_h; f.red_c = a.cur->acc_c;
    f.counts = d->counts;
    keff_final(f, d, vstride, (int)d->ny);
    f.abort_flag = &a.cur->abort; f.status_out = d->status;      // status may be NULL here
    f.dbg = ctx->single_stamps ? ctx->single_stamps + 8 : nullptr;            // (slots 8.. of workgroup 0, slab 0)
    ctx->mm_valid = 0;                                        // (no chained min/max comes out of this path)
    XC_TRY(hist_ev_begin(ctx));
    XC_TRY(launch_keff_single(ctx, d->q_dtype, a, g));
    XC_TRY(hist_ev_end(ctx));
    XC_TRY(launch_finalize(ctx, d->nslab, f));
    ctx->single_dirty_bins[cur] = N;                          // what the NEXT launch clears in this set (only once launch_finalize succeeded)
    ctx->single_dirty_bins[1u - cur] = 0;
    ++ctx->single_launches;
    ctx->last_keff_path = 1;
    return XC_OK;
}

static int keff_dev(xc_ctx* ctx, const xc_keff_desc* d)
{
    if (!d) return fail(ctx, XC_EBADARG, "xc_keff: desc is NULL");
    if (!d->q || !d->ctr || !d->area || !d->tbl || !d->tbl_coord) return fail(ctx, XC_EBADARG, "xc_keff: q/ctr/area/tbl/tbl_coord must be given");
    if (!is_float(d->q_dtype)) return fail(ctx, XC_EBADARG, "xc_keff: bad q_dtype");
    if (!is_float(d->ctr_dtype)) return fail(ctx, XC_EBADARG, "xc_keff: bad ctr_dtype");
    if (d->nslab < 1 || d->ny < 2 || d->nx < 1 || d->N < 2) return fail(ctx, XC_EBADARG, "xc_keff: need nslab>=1, ny>=2, nx>=1, N>=2");
    if (d->dA_rank < XC_DA_NONE || d->dA_rank > XC_DA_SLAB || (d->dA_rank != XC_DA_NONE && !d->dA)) return fail(ctx, XC_EBADARG, "xc_keff: bad dA");
    if (d->grad ? (!d->rdx || !d->rdy) : !d->grdS) return fail(ctx, XC_EBADARG, "xc_keff: need rdx/rdy (grad=1) or grdS (grad=0)");
    if (d->npre < 0 || (d->npre > 0 && d->interp && !d->preY)) return fail(ctx, XC_EBADARG, "xc_keff: preY is NULL");
    if (d->out_stride != 0 && d->out_stride < d->N) return fail(ctx, XC_EBADARG, "xc_keff: out_stride must be 0 (dense) or >= N");
    const int vstride = d->out_stride ? d->out_stride : d->N;
    const int N = d->N, nch = 2;
    const int det = d->deterministic ? 1 : 0;
    const void* q_next = d->q_next;                          // (deterministic sums: carried by the fixed-point pass)
    ctx->last_keff_path = 0;
    // ONE slab (the reference's callers hand planes over one at a time): the single-read kernel (xc_keff1.hip) where the slab fits the
    // register tiles of the chip -- min/max, levels and histogram in ONE launch, the tracer read ONCE.  (Two slabs: only when forced --
    // the kernel runs them one after the other, 64.7 us against the chain's 59.3.)
    if (d->single_read != XC_SINGLE_NEVER && ctx->knobs.single != 0 && !det && d->grad &&
        d->nslab <= (d->single_read == XC_SINGLE_FORCE ? kSingleMaxSlabs : 1)) {
        const int rc = keff_single(ctx, d);
        if (rc != XC_EAGAIN) return rc;                      // (XC_EAGAIN: the shape does not suit it; nothing was enqueued)
    }
    HistGeom g;
    {
        const void* gi[1] = {d->grdS}; const int32_t gt[1] = {d->grdS_dtype};
        const bool da2d = d->dA_rank == XC_DA_PLANE || d->dA_rank == XC_DA_SLAB;
        const bool fast_layout = d->grad && da2d && d->periodic_x && d->dA_pos_finite && d->right_edge != XC_EDGE_NUMPY;
        // float32 tracer with a supplied float32 squared gradient (the reference's own workflow): four cells per lane too
        const bool supplied_f32 = !d->grad && da2d && d->q_dtype == XC_F32 && d->grdS_dtype == XC_F32 &&
                                  reinterpret_cast<uintptr_t>(d->grdS) % 16 == 0;
        XC_TRY(hist_geometry(ctx, d->q_dtype, d->nslab, d->ny, d->nx, N, nch,
                             vec_align_bits(d->q, d->q_dtype, d->q_next, d->dA, d->dA_rank, gi, gt, d->grad ? 0 : 1), &g,
                             fast_layout ? 1 : (supplied_f32 ? 2 : 0), det));
    }
    K3Scratch L;
    XC_TRY(L.reserve(ctx, d->nslab, g.bps, nch, N, det, true));
    double* mmpart = L.mmpart;
    int mmP = minmax_blocks(d->ny * d->nx, d->nslab);
    bool accum = false;

    // min/max partials: either produced by the previous call's histogram pass (q_next) or by K1 now
    if (ctx->mm_valid && ctx->mm_q == d->q && ctx->mm_nslab == d->nslab && ctx->mm_ny == d->ny &&
        ctx->mm_nx == d->nx && ctx->mm_dtype == d->q_dtype && ctx->mm_gen == d->q_gen) {
        mmpart = ctx->mmnext[ctx->mm_cur]; mmP = ctx->mm_P;
    } else {
        // FEW slabs (more than 64 blocks per slab: a single cfg2 slab has ~200): the blocks add into per-slab accumulators, cleared by
        // this K1 launch, and the finalize kernel reads them directly -- three dependent launches instead of four
        accum = !det && g.bps > 64;
        XC_TRY(launch_minmax_partial(ctx, d->q, d->q_dtype, d->nslab, d->ny * d->nx, mmpart,
                                     accum ? L.red_h : nullptr, accum ? L.acc_words : 0));
    }
    ctx->mm_valid = 0;
    double* mm_next = nullptr;
    if (q_next) {
        const int nb = 1 - ctx->mm_cur;
        XC_TRY(grow(ctx, (void**)&ctx->mmnext[nb], &ctx->mmnext_bytes[nb], al((size_t)d->nslab * g.bps * 2 * sizeof(double))));
        mm_next = ctx->mmnext[nb];
    }

    HistArgs a; memset(&a, 0, sizeof(a));
    FinalArgs f; memset(&f, 0, sizeof(f));
    XC_TRY(hist_common(ctx, d, nch, N, g, L, a, f));
    if (!d->grad) { a.integ[0] = d->grdS; a.integ_f32[0] = d->grdS_dtype == XC_F32; }
    a.q_next = q_next; a.mm_next = mm_next;
    a.mmpart = mmpart; a.P = mmP; a.levels_mode = 1;
    a.last_closed = d->right_edge == XC_EDGE_NUMPY;
    a.increase = d->increase; a.ctr_f32 = d->ctr_dtype == XC_F32;
    a.right_edge = d->right_edge; a.inv_nm1 = 1.0 / (double)(N - 1);
    a.ctr_out = d->ctr; a.ctr_stride = vstride; a.status = d->status;
    if (accum) { a.acc_h = f.red_h; a.acc_c = d->counts ? f.red_c : nullptr; f.skip_reduce = 1; }
    XC_TRY(hist_ev_begin(ctx));
    if (det) {
        const void* gi[1] = {d->grdS}; const int gt[1] = {d->grdS_dtype};
        XC_TRY(det_one_pass(ctx, d->q_dtype, d->grad ? 0 : 1, d->grad, g, d->nslab, d->ny, d->nx, a, L, d->dA_max, gi, gt, f));
    } else {
        XC_TRY(launch_hist(ctx, d->q_dtype, d->grad ? 0 : 1, d->grad, g, d->nslab, a));
    }
    XC_TRY(hist_ev_end(ctx));
    if (q_next) {
        ctx->mm_cur = 1 - ctx->mm_cur; ctx->mm_valid = 1; ctx->mm_P = g.bps; ctx->mm_q = q_next;
        ctx->mm_nslab = d->nslab; ctx->mm_ny = d->ny; ctx->mm_nx = d->nx; ctx->mm_dtype = d->q_dtype;
        ctx->mm_gen = d->q_gen;
    }

    keff_final(f, d, vstride, (int)d->ny);
    return launch_finalize(ctx, d->nslab, f);
}

extern "C" {

// ------------------------------------------------------------------------------------ K1
int xc_minmax_dev(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ncell, double* out_minmax)
{
    XC_CTX(ctx);
    if (!q || !out_minmax || nslab < 1 || ncell < 1) return fail(ctx, XC_EBADARG, "xc_minmax: bad arguments");
    double* part;
    XC_TRY(k1_scratch(ctx, nslab, &part));
    XC_TRY(launch_minmax_partial(ctx, q, q_dtype, nslab, ncell, part));
    return launch_minmax_final(ctx, part, nslab, minmax_blocks(ncell, nslab), out_minmax);
}

int xc_minmax(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ncell, double* out_minmax)
{
    XC_CTX(ctx);
    if (!q || !out_minmax || nslab < 1 || ncell < 1) return fail(ctx, XC_EBADARG, "xc_minmax: bad arguments");
    if (!is_float(q_dtype)) return fail(ctx, XC_EBADARG, "xc_minmax: q_dtype must be XC_F32 or XC_F64");
    const size_t qb = (size_t)nslab * ncell * esize(q_dtype), ob = (size_t)nslab * 2 * sizeof(double);
    Stage st(ctx); void* sq; const void* dq; double* dout;
    XC_TRY(lay_stage(st, [&](Stage& s) { sq = s.take(qb); dout = s.out(out_minmax, ob); }));
    XC_TRY(stage_in(ctx, sq, q, qb, &dq));
    XC_TRY(flush_in(ctx));
    XC_TRY(xc_minmax_dev(ctx, dq, q_dtype, nslab, ncell, dout));
    XC_TRY(st.deliver());
    return xc_sync(ctx);
}

// ------------------------------------------------------------------------------------ levels
int xc_levels_dev(xc_ctx* ctx, const double* minmax, int q_dtype, int64_t nslab, int N, int increase,
                  int ctr_dtype, int right_edge, double* ctr, double* edges, int32_t* status)
{
    XC_CTX(ctx);
    return launch_levels(ctx, minmax, q_dtype, nslab, N, increase, ctr_dtype, right_edge, ctr, edges, status);
}

int xc_levels(xc_ctx* ctx, const double* minmax, int q_dtype, int64_t nslab, int N, int increase,
              int ctr_dtype, int right_edge, double* ctr, double* edges, int32_t* status)
{
    XC_CTX(ctx);
    if (!minmax || !ctr || !edges || !status || N < 2 || nslab < 1) return fail(ctx, XC_EBADARG, "xc_levels: bad arguments (need N >= 2)");
    const size_t mb = (size_t)nslab * 2 * 8, cb = (size_t)nslab * N * 8, eb = (size_t)nslab * (N + 1) * 8, sb = (size_t)nslab * 4;
    Stage st(ctx); double *dm, *dc, *de; int32_t* ds;
    XC_TRY(lay_stage(st, [&](Stage& s) { dm = s.take<double>(mb); dc = s.out(ctr, cb); de = s.out(edges, eb); ds = s.out(status, sb); }));
    XC_TRY(h2d(ctx, dm, minmax, mb));
    XC_TRY(flush_in(ctx));
    XC_TRY(launch_levels(ctx, dm, q_dtype, nslab, N, increase, ctr_dtype, right_edge, dc, de, ds));
    XC_TRY(st.deliver());
    return xc_sync(ctx);
}

// cal_contours(int levels) (core.py:205-249) in ONE call: min / max of every slab (K1), the levels (and edges) from them, ONE result
// hand-over and ONE stream synchronisation -- the facade used to make two host-form calls (xc_minmax, then xc_levels with the extrema
// sent back up) with a blocking transfer for each of their five small arrays.  Any output may be NULL except out_ctr.
int xc_contours(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ncell, int N, int increase, int ctr_dtype, int right_edge,
                double* out_minmax, double* out_ctr, double* out_edges, int32_t* out_status)
{
    XC_CTX(ctx);
    if (!q || !out_ctr || nslab < 1 || ncell < 1 || N < 2) return fail(ctx, XC_EBADARG, "xc_contours: bad arguments (need N >= 2)");
    if (!is_float(q_dtype)) return fail(ctx, XC_EBADARG, "xc_contours: q_dtype must be XC_F32 or XC_F64");
    const size_t qb = (size_t)nslab * ncell * esize(q_dtype);
    const size_t mb = (size_t)nslab * 2 * 8, cb = (size_t)nslab * N * 8, eb = (size_t)nslab * (N + 1) * 8, sb = (size_t)nslab * 4;
    Stage st(ctx); void* sq; const void* dq; double *dm, *dc, *de, *part; int32_t* ds;
    XC_TRY(lay_stage(st, [&](Stage& s) {
        sq = s.take(qb);
        dm = s.keep(out_minmax, mb);                         // (read by the level kernel: on the device whether it is wanted or not)
        dc = s.out(out_ctr, cb, true); de = s.keep(out_edges, eb, true); ds = s.keep(out_status, sb, true);
    }));
    XC_TRY(stage_in(ctx, sq, q, qb, &dq));
    XC_TRY(flush_in(ctx));
    // K1's partials are reduced by the level kernel itself: two launches for the whole call
    XC_TRY(k1_scratch(ctx, nslab, &part));
    XC_TRY(launch_minmax_partial(ctx, dq, q_dtype, nslab, ncell, part));
    XC_TRY(launch_levels(ctx, part, q_dtype, nslab, N, increase, ctr_dtype, right_edge, dc, de, ds, minmax_blocks(ncell, nslab), dm));
    XC_TRY(st.deliver());
    return xc_sync(ctx);
}

// ------------------------------------------------------------------------------------ K3 + K5
int xc_hist_dev(xc_ctx* ctx, const xc_hist_desc* d)
{
    XC_CTX(ctx);
    ctx->last_hist = xc_hist_variant{};
    return hist_recorded(ctx, hist_dev(ctx, d));
}

int xc_hist(xc_ctx* ctx, const xc_hist_desc* hd)
{
    XC_CTX(ctx);
    ctx->last_hist = xc_hist_variant{};
    return hist_recorded(ctx, hist_host(ctx, hd));
}

// ------------------------------------------------------------------------------------ K5 / K6 alone
int xc_keff_epilogue_dev(xc_ctx* ctx, const double* pdf, const double* ctr, int ctr_dtype, int64_t nslab, int N,
                         int increase, int lt, const double* tbl, const double* tbl_coord, int ntbl,
                         const double* preY, int npre, double nkeff_mask, double lmin_scale,
                         double* area, double* intgrdS, double* latEq, double* dqdA, double* dintSdA,
                         double* Leq2, double* Lmin, double* nkeff, double* interp)
{
    XC_CTX(ctx);
    if (!pdf || !ctr || !tbl || !tbl_coord) return fail(ctx, XC_EBADARG, "xc_keff_epilogue: pdf / ctr / tbl / tbl_coord must be given");
    if (nslab < 1 || N < 2 || ntbl < 2 || npre < 0) return fail(ctx, XC_EBADARG, "xc_keff_epilogue: need nslab >= 1, N >= 2, ntbl >= 2");
    if (!is_float(ctr_dtype)) return fail(ctx, XC_EBADARG, "xc_keff_epilogue: bad ctr_dtype");
    if (npre > 0 && interp && !preY) return fail(ctx, XC_EBADARG, "xc_keff_epilogue: preY is NULL");
    // the reduce stage sums ONE "partial" per slab (the pdf itself); its count channel reads zeros
    const int nch = 2;
    K3Scratch L;
    XC_TRY(L.reserve(ctx, nslab, 1, nch, N, 0, false, false));
    XC_HIP(ctx, hipMemsetAsync(L.part_c, 0, L.part_c_bytes, ctx->stream));
    ctx->mm_valid = 0;                          // the scratch may have moved
    FinalArgs f; memset(&f, 0, sizeof(f));
    f.part_h = pdf; f.part_c = L.part_c; f.bps = 1; f.nch = nch; f.nbin = N;
    f.red_h = L.red_h; f.red_c = L.red_c;
    xc_keff_desc d; memset(&d, 0, sizeof(d));       // the arguments in the form keff_final takes them
    d.lt = lt; d.increase = increase; d.ctr_dtype = ctr_dtype; d.ctr = const_cast<double*>(ctr);
    d.tbl = tbl; d.tbl_coord = tbl_coord; d.preY = preY; d.npre = npre; d.nkeff_mask = nkeff_mask; d.lmin_scale = lmin_scale;
    d.area = area; d.intgrdS = intgrdS; d.latEq = latEq; d.dqdA = dqdA; d.dintSdA = dintSdA;
    d.Leq2 = Leq2; d.Lmin = Lmin; d.nkeff = nkeff; d.interp = interp;
    keff_final(f, &d, 0, ntbl);
    return launch_finalize(ctx, nslab, f);
}

int xc_keff_epilogue(xc_ctx* ctx, const double* pdf, const double* ctr, int ctr_dtype, int64_t nslab, int N,
                     int increase, int lt, const double* tbl, const double* tbl_coord, int ntbl,
                     const double* preY, int npre, double nkeff_mask, double lmin_scale,
                     double* area, double* intgrdS, double* latEq, double* dqdA, double* dintSdA,
                     double* Leq2, double* Lmin, double* nkeff, double* interp)
{
    XC_CTX(ctx);
    if (!pdf || !ctr || !tbl || !tbl_coord || nslab < 1 || N < 2 || ntbl < 2 || npre < 0)
        return fail(ctx, XC_EBADARG, "xc_keff_epilogue: bad arguments");
    const size_t S = (size_t)nslab, vb = S * N * 8, pb = 2 * vb, tb = (size_t)ntbl * 8, yb = (size_t)npre * 8, ib = S * 9 * npre * 8;
    double* host[8] = {area, intgrdS, latEq, dqdA, dintSdA, Leq2, Lmin, nkeff};
    Stage st(ctx); double *dp, *dc, *dt, *dy, *dpre, *o[8], *di;
    XC_TRY(lay_stage(st, [&](Stage& s) {
        dp = s.take<double>(pb); dc = s.take<double>(vb); dt = s.take<double>(tb); dy = s.take<double>(tb);
        dpre = npre > 0 ? s.take<double>(yb) : nullptr;
        for (int i = 0; i < 8; ++i) o[i] = s.keep(host[i], vb);      // (the kernel gets all eight vectors, wanted or not)
        di = npre > 0 ? s.out(interp, ib) : nullptr;
    }));
    XC_TRY(h2d(ctx, dp, pdf, pb)); XC_TRY(h2d(ctx, dc, ctr, vb));
    XC_TRY(h2d(ctx, dt, tbl, tb)); XC_TRY(h2d(ctx, dy, tbl_coord, tb));
    if (npre > 0) { if (!preY) return fail(ctx, XC_EBADARG, "xc_keff_epilogue: preY is NULL"); XC_TRY(h2d(ctx, dpre, preY, yb)); }
    XC_TRY(flush_in(ctx));
    XC_TRY(xc_keff_epilogue_dev(ctx, dp, dc, ctr_dtype, nslab, N, increase, lt, dt, dy, ntbl, dpre, npre, nkeff_mask, lmin_scale,
                                o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7], di));
    XC_TRY(st.deliver());
    return xc_sync(ctx);
}

// ------------------------------------------------------------------------------------ fused Keff pipeline
int xc_keff_dev(xc_ctx* ctx, const xc_keff_desc* d)
{
    XC_CTX(ctx);
    ctx->last_hist = xc_hist_variant{};
    return hist_recorded(ctx, keff_dev(ctx, d));
}

int xc_last_keff_path(xc_ctx* ctx, int* out_path)
{
    if (!ctx || !out_path) return fail(ctx, XC_EBADARG, "xc_last_keff_path: bad arguments");
    *out_path = ctx->last_keff_path;
    return XC_OK;
}

// diagnostics: wall-clock stamps (100 MHz) of thread 0 of every workgroup of the single-read kernel at its phase boundaries;
// enable != 0 allocates [kSingleMaxSlabs][cus][12] uint64 and returns the device pointer, 0 frees it
int xc_dbg_single_stamps(xc_ctx* ctx, int enable, void** out_dev, int* out_slots)
{
    XC_CTX(ctx);
    if (ctx->single_stamps) { XC_HIP(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(ctx->single_stamps); ctx->single_stamps = nullptr; }
    if (enable) {
        const size_t bytes = (size_t)kSingleMaxSlabs * ctx->cus * kSingleStampSlots * sizeof(unsigned long long);
        XC_HIP(ctx, hipMalloc((void**)&ctx->single_stamps, bytes));
        XC_HIP(ctx, hipMemset(ctx->single_stamps, 0, bytes));
    }
    if (out_dev) *out_dev = ctx->single_stamps;
    if (out_slots) *out_slots = kSingleStampSlots;
    return XC_OK;
}

int xc_last_hist_variant(xc_ctx* ctx, xc_hist_variant* out)
{
    if (!ctx || !out) return fail(ctx, XC_EBADARG, "xc_last_hist_variant: bad arguments");
    *out = ctx->last_hist;
    return XC_OK;
}

}  // extern "C"

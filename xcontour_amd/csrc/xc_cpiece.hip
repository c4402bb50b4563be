// K13 -- the connected PIECES of the contours and their statistics (gfx950), from K12's segment records on the device.
//
// The reference's scripts work on pieces: tests/test_breaking.py keeps "the largest contour that encircles the pole", tests/test_clength.py
// sums contour_length(seg) piece by piece, utils.contour_area (utils.py:537-561) measures one.  Build-defined: a piece is a connected chain
// of segments under "next(i) is the segment of the same range whose e_from == e_to[i]" (xc_join.cpp): a ring, or an open polyline headed
// by a segment without a predecessor.  Only the per-piece table leaves the device.
//
// Input: count[nrange], e_from, e_to, pts as xc_contour_segments[_periodic]_dev wrote them (a range = one (slab, contour)); E = 2 ny nx
// bounds every edge id.  Labels, links and slots are 32-bit: E < 2^31 and every range has fewer than 2^31 segments (XC_EBADARG else).
//
// Phase A (scatter, link, round, unscatter and the groups live in xc_cpiece_link.h: K14, xc_cjoin.hip, shares them), per GROUP of
// consecutive ranges (as many as keep g E 4 bytes of table under the context's workspace cap, at least one; fewer
// than 2^31 segments per group; indices are group-local):
//   k_cp_scatter  tab[range][e_from[i]] = i (the table is -1 everywhere else), label0 = e_from, prev0 = -1, the segment's range
//   k_cp_link     next0[i] = tab[range][e_to[i]], and prev0[next0[i]] = i: prev is the inverse of next, no second table
//   k_cp_round    R = ceil(log2(largest count of the group)) + 1 rounds of synchronous pointer doubling on double buffers:
//                 label' = min(label, label[next], label[prev]), next' = next[next], prev' = prev[prev].  After k rounds a label is the
//                 smallest e_from within 2^k - 1 links either way: R rounds cover every piece, so a piece's label is the smallest e_from
//                 it contains -- the key xc_join_segments orders polylines by.  R is fixed on the host from the counts.  After R rounds
//                 prev is -1 on every member of an open piece (2^R links back fall off its head) and >= 0 on every member of a ring.
//   k_cp_root     root(i) = tab[range][label]; a segment that is its own root takes the next slot of its range (one atomic per wave on
//                 piece_count[range] where the wave lies in one range) and notes whether its piece is open
//   k_cp_bcast    every segment copies slot and open bit from its root into the one array that outlives the group (pslot[total])
//   k_cp_unscatter  tab[range][e_from[i]] = -1: the table is cleared once per call and handed on clean
// The host reads piece_count (the one round trip, as in K12), scans it, and stops with 1 when the pieces exceed `capacity`.
// Phase B, over all segments at once: k_cp_init, k_cp_reduce, k_cp_finish.  Every reduction is order-free:
//   nseg, winding   integer atomic adds;   first_edge, row_min, row_max   integer atomic min / max (rows are non-negative doubles: their
//                   bit patterns order like the values);   closed   the open bit, stored as 0 by any member of an open piece
//   winding  the sum over the links i -> next(i) of +1 where c2[i] == nx and c1[next] == 0, -1 for the opposite jump.  On a ring every
//            segment has a successor and a predecessor, an end point on the seam cell's right edge (column nx) is always followed by a
//            start point at column 0, and a start point at column nx always follows an end point at column 0: the sum is the number of
//            segments with c2 == nx minus the number with c1 == nx, which needs no link.  Open pieces and non-periodic planes get 0.
//   length   K10's segment length (interp_at on the node floor(r) / floor(c), column nx of a periodic plane at xcoord[0] + period,
//            seg_len<LATLON>; a segment whose end points coincide adds nothing), times radius once at the end
//   area     S = 1/2 sum (Ya' + Yb') (Xa - Xb), Y' = sin(Y) on the sphere (then S radius^2), NaN for an open piece
//   Sums: every term is added WHOLE (all 53 bits) to a fixed-point accumulator of CP_L 32-bit limbs kept in 64-bit words: a term is cut at
//   the limb boundaries into three chunks below 2^32, each added (negated for a negative term) with one 64-bit integer atomic; a word
//   takes 2^31 chunks before it could wrap.  The window's top sits 12 bits above a bound on one term fixed before the pass (K10's window
//   constant for the lengths; max |Y'| times the largest cell width for the areas); bits more than 32 CP_L below the top are dropped (a
//   function of the term alone).  k_cp_finish carries the words and rounds once, half to even: the result is the exact sum of the
//   terms, rounded once, whatever the order of arrival.
#include "xc_capi.h"
#include <cmath>
#include <vector>

namespace xc {
namespace {

#include "xc_binning.h"
#include "xc_clen_cell.h"

#include "xc_cpiece_link.h"
#include "xc_cpiece_slot.h"
#include "xc_cpiece_sum.h"

__global__ __launch_bounds__(CP_TPB)
void k_cp_bcast(int64_t n, long long s0, const int* __restrict__ root, const int* __restrict__ slot, int* __restrict__ pslot)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= n) return;
    pslot[s0 + i] = slot[root[i]];
}

// the window constant of the area terms: |1/2 (Ya' + Yb') (Xa - Xb)| <= max |Y'| x the largest cell width
__global__ __launch_bounds__(256)
void k_cp_area_window(const double* __restrict__ fy, int64_t ny, const double* __restrict__ fx, int64_t nx, int latlon, int wrap,
                      double period, int* __restrict__ c0)
{
    double my, mx;
    window_maxima<false>(fy, ny, fx, nx, wrap != 0, period, my, mx);
    if (latlon) my = 1.0;
    if (threadIdx.x == 0) c0[0] = det_c0_from_bound(1.0000001 * my * mx);
}

#define XC_CP_RECORDS long long* __restrict__ first_edge, long long* __restrict__ nseg, int* __restrict__ closed, int* __restrict__ winding, \
                      double* __restrict__ length, double* __restrict__ area, double* __restrict__ row_min, double* __restrict__ row_max

__global__ __launch_bounds__(CP_TPB)
void k_cp_init(int64_t np, XC_CP_RECORDS, unsigned long long* __restrict__ acc, int* __restrict__ flags)
{
    const int64_t p = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (p >= np) return;
    first_edge[p] = 0x7fffffffffffffffll; nseg[p] = 0; closed[p] = 1; winding[p] = 0;
    length[p] = 0.0; area[p] = 0.0;
    row_min[p] = __longlong_as_double(0x7ff0000000000000ll); row_max[p] = 0.0;
    flags[p] = 0;
#pragma unroll
    for (int j = 0; j < 2 * CP_L; ++j) acc[(size_t)p * 2 * CP_L + j] = 0ull;
}

template <bool LATLON>
__global__ __launch_bounds__(CP_TPB)
void k_cp_reduce(int64_t total, const long long* __restrict__ off, int64_t nrange, const long long* __restrict__ poff,
                 const unsigned long long* __restrict__ piece_count, const int* __restrict__ pslot,
                 const long long* __restrict__ e_from, const double* __restrict__ pts, int64_t ny, int64_t nx, int wrap,
                 const double* __restrict__ fy, const double* __restrict__ fx, double period, const int* __restrict__ c0,
                 XC_CP_RECORDS, unsigned long long* __restrict__ acc, int* __restrict__ flags, int* __restrict__ err)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= total) return;
    const int64_t r = cp_range_of(off, 0, nrange, i);
    const int ps = pslot[i];
    const unsigned long long sl = (unsigned)(ps & 0x7fffffff);
    if (sl >= piece_count[r]) { *err = CP_ERR_LINK; return; }             // records that are no K12 output: never past the table
    const int64_t p = poff[r] + (int64_t)sl;
    const bool open = ps < 0;
    const double2 a = *reinterpret_cast<const double2*>(pts + 4 * (size_t)i), b = *reinterpret_cast<const double2*>(pts + 4 * (size_t)i + 2);
    const double r1 = a.x, c1 = a.y, r2 = b.x, c2 = b.y;
    atomicAdd((unsigned long long*)nseg + p, 1ull);
    atomicMin((unsigned long long*)first_edge + p, (unsigned long long)e_from[i]);
    if (open) closed[p] = 0;
    atomicMin((unsigned long long*)row_min + p, (unsigned long long)__double_as_longlong(fmin(r1, r2)));
    atomicMax((unsigned long long*)row_max + p, (unsigned long long)__double_as_longlong(fmax(r1, r2)));
    if (wrap) {
        const double xn = (double)nx;
        const int w = (int)(c2 == xn) - (int)(c1 == xn);
        if (w != 0) atomicAdd(winding + p, w);
    }
    // index space -> coordinates: np.interp on the node floor(.)
    auto ycd = [&](double rr) {
        int64_t i0 = (int64_t)floor(rr);
        i0 = i0 < 0 ? 0 : (i0 > ny - 1 ? ny - 1 : i0);
        const int64_t i1 = i0 + 1 < ny ? i0 + 1 : ny - 1;
        return interp_at(rr, (double)i0, fy[i0], fy[i1]);
    };
    const int64_t cmax = wrap ? nx : nx - 1;                               // the last node column; column nx is column 0 one period on
    auto xat = [&](int64_t j) { return j < nx ? fx[j] : __dadd_rn(fx[0], period); };
    auto xcd = [&](double cc) {
        int64_t j0 = (int64_t)floor(cc);
        j0 = j0 < 0 ? 0 : (j0 > cmax ? cmax : j0);
        const int64_t j1 = j0 + 1 < cmax ? j0 + 1 : cmax;
        return interp_at(cc, (double)j0, xat(j0), xat(j1));
    };
    const double y1 = ycd(r1), y2 = ycd(r2), x1 = xcd(c1), x2 = xcd(c2);
    unsigned long long* pa = acc + (size_t)p * 2 * CP_L;
    if (!(r1 == r2 && c1 == c2)) cp_add(pa, flags + p, 1, seg_len<LATLON>(x1, y1, x2, y2), cp_top(c0[0]));
    if (!open) {
        const double ya = LATLON ? sin(y1) : y1, yb = LATLON ? sin(y2) : y2;
        cp_add(pa + CP_L, flags + p, 2, __dmul_rn(0.5, __dmul_rn(__dadd_rn(ya, yb), __dsub_rn(x1, x2))), cp_top(c0[1]));
    }
}

__global__ __launch_bounds__(CP_TPB)
void k_cp_finish(int64_t np, XC_CP_RECORDS, const unsigned long long* __restrict__ acc, const int* __restrict__ flags,
                 const int* __restrict__ c0, double radius)
{
    const int64_t p = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (p >= np) return;
    const int fl = flags[p], cl = closed[p];
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    double len = cp_to_double(acc + (size_t)p * 2 * CP_L, cp_top(c0[0]));
    if (radius > 0.0) len = __dmul_rn(len, radius);
    length[p] = (fl & 1) ? qnan : len;
    double s = qnan;
    if (cl && !(fl & 2)) {
        s = cp_to_double(acc + (size_t)p * 2 * CP_L + CP_L, cp_top(c0[1]));
        if (radius > 0.0) s = __dmul_rn(s, __dmul_rn(radius, radius));
    }
    area[p] = s;
    if (!cl) winding[p] = 0;
}
#undef XC_CP_RECORDS

}  // namespace

// One xc_contour_pieces_dev call.  Waits for the stream twice: for K12's counts (they size the groups and fix the rounds) and for the
// piece counts (they decide on the host whether the records fit).
int launch_contour_pieces(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to, const double* pts,
                          int64_t ny, int64_t nx, int periodic, const double* ycoord, const double* xcoord, double period, double radius,
                          int64_t capacity, uint64_t* piece_count, int64_t* first_edge, int64_t* nseg, int32_t* closed, int32_t* winding,
                          double* length, double* area, double* row_min, double* row_max)
{
    if (!count || !piece_count || !ycoord || !xcoord || nrange < 1 || ny < 1 || nx < 1 || capacity < 0)
        return fail(ctx, XC_EBADARG, "xc_contour_pieces: bad arguments");
    if (!(radius >= 0.0)) return fail(ctx, XC_EBADARG, "xc_contour_pieces: radius must be >= 0");
    if (periodic && (!std::isfinite(period) || period == 0.0 || nx < 2))
        return fail(ctx, XC_EBADARG, "xc_contour_pieces: a periodic plane needs a finite, non-zero period and nx >= 2");
    if (capacity > 0 && (!first_edge || !nseg || !closed || !winding || !length || !area || !row_min || !row_max))
        return fail(ctx, XC_EBADARG, "xc_contour_pieces: capacity > 0 needs the record arrays");
    if (ny > ((int64_t)1 << 30) / nx) return fail(ctx, XC_EBADARG, "xc_contour_pieces: plane too large for 32-bit labels (2 ny nx < 2^31)");
    const long long E = 2 * ny * nx;
    const int wrap = periodic ? 1 : 0, latlon = radius > 0.0;
    CpProfile& prof = ctx->prof_cpiece;
    profile_clear(prof);

    CpPlan pl;
    XC_TRY(cp_plan(ctx, "xc_contour_pieces", nrange, count, piece_count, e_from, e_to, pts, E, pl));
    const long long total = pl.total;
    if (total == 0) return XC_OK;

    // workspace: off | poff | c0[2], err | pslot[total] | the tail (xc_cpiece_link.h)
    long long *d_off, *d_poff; int *d_c0, *pslot; CpTail tail;
    auto lay = [&](Carve c) {
        d_off = c.take<long long>((size_t)nrange + 1); d_poff = c.take<long long>((size_t)nrange + 1);
        d_c0 = c.take<int>(CP_SMALL); pslot = c.take<int>((size_t)total);
        cp_carve_tail(c, pl, 6, tail);
        return c.at;
    };
    XC_TRY(lay_out(ctx, &ctx->cpiece_ws, &ctx->cpiece_ws_bytes, lay));
    int* d_err = d_c0 + 2;

    StageTimer tm(ctx, prof.ms);                                             // where the time goes (xc_set_kernel_timing)
    CpRun run(ctx, tm, pl, e_from, e_to, d_off, tail, d_err);

    tm.mark(-1);
    XC_TRY(run.upload_off());
    XC_HIP(ctx, hipMemsetAsync(d_c0, 0, CP_SMALL * 4, ctx->stream));
    XC_TRY(run.fill_table());
    tm.mark(0);
    for (const CpGroup& g : pl.groups) {
        run.begin(g);
        XC_TRY(run.rounds());
        const CpRoles& b = run.b;
        hipLaunchKernelGGL(k_cp_root, run.grid, dim3(CP_TPB), 0, ctx->stream, run.n, E, tail.tab, tail.rid, b.lab, b.prv, g.r0,
                           (unsigned long long*)piece_count, b.nxt2, b.lab2);
        hipLaunchKernelGGL(k_cp_bcast, run.grid, dim3(CP_TPB), 0, ctx->stream, run.n, run.s0, b.nxt2, b.lab2, pslot);
        XC_HIP(ctx, hipGetLastError());
        tm.mark(2);
        XC_TRY(run.end());
    }
    run.report(prof);
    // the second round trip: the piece counts (and whether the records were K12's)
    std::vector<uint64_t> hp((size_t)nrange);
    int herr = 0;
    XC_HIP(ctx, hipMemcpyAsync(hp.data(), piece_count, (size_t)nrange * 8, hipMemcpyDeviceToHost, ctx->stream));
    XC_TRY(cp_read_err(ctx, d_err, &herr));
    if (herr) return fail(ctx, XC_EBADARG, "xc_contour_pieces: an edge id outside [0, 2 ny nx)");
    std::vector<long long> poff((size_t)nrange + 1);
    poff[0] = 0;
    for (int64_t r = 0; r < nrange; ++r) poff[(size_t)r + 1] = poff[(size_t)r] + (long long)hp[(size_t)r];
    const long long np = poff[(size_t)nrange];
    if (np > capacity) return 1;
    unsigned long long* acc; int* flags;                                     // the limbs of both sums and the flags of every piece
    auto lay_acc = [&](Carve c) { acc = c.take<unsigned long long>((size_t)np * 2 * CP_L); flags = c.take<int>((size_t)np); return c.at; };
    XC_TRY(lay_out(ctx, &ctx->cpiece_acc, &ctx->cpiece_acc_bytes, lay_acc));
    tm.mark(-1);
    XC_HIP(ctx, hipMemcpyAsync(d_poff, poff.data(), (size_t)(nrange + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    XC_TRY(launch_clen_window(ctx, ycoord, ny, xcoord, nx, wrap ? period : 0.0, latlon, 1, d_c0));
    hipLaunchKernelGGL(k_cp_area_window, dim3(1), dim3(256), 0, ctx->stream, ycoord, ny, xcoord, nx, latlon, wrap, period, d_c0 + 1);
#define XC_CP_RECORDS (long long*)first_edge, (long long*)nseg, (int*)closed, (int*)winding, length, area, row_min, row_max
    hipLaunchKernelGGL(k_cp_init, dim3(cp_blocks(np)), dim3(CP_TPB), 0, ctx->stream, (int64_t)np, XC_CP_RECORDS, acc, flags);
    XC_HIP(ctx, hipGetLastError());
#define XC_CP_REDUCE(LL_) hipLaunchKernelGGL((k_cp_reduce<LL_>), dim3(cp_blocks(total)), dim3(CP_TPB), 0, ctx->stream, (int64_t)total, d_off, nrange, \
                          d_poff, (const unsigned long long*)piece_count, pslot, (const long long*)e_from, pts, ny, nx, wrap, ycoord, xcoord, \
                          period, d_c0, XC_CP_RECORDS, acc, flags, d_err)
    if (latlon) XC_CP_REDUCE(true); else XC_CP_REDUCE(false);
#undef XC_CP_REDUCE
    XC_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_cp_finish, dim3(cp_blocks(np)), dim3(CP_TPB), 0, ctx->stream, (int64_t)np, XC_CP_RECORDS, acc, flags, d_c0, radius);
#undef XC_CP_RECORDS
    XC_HIP(ctx, hipGetLastError());
    tm.mark(3);
    XC_TRY(cp_read_err(ctx, d_err, &herr));
    if (herr) return fail(ctx, XC_EBADARG, "xc_contour_pieces: the records are not those of one xc_contour_segments call (a repeated edge id)");
    return XC_OK;
}

}  // namespace xc

// ------------------------------------------------------------------------------------ C ABI
int xc_contour_pieces_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to, const double* pts,
                          int64_t ny, int64_t nx, int periodic, const double* ycoord, const double* xcoord, double period, double radius,
                          int64_t capacity, uint64_t* piece_count, int64_t* first_edge, int64_t* nseg, int32_t* closed, int32_t* winding,
                          double* length, double* area, double* row_min, double* row_max)
{
    XC_CTX(ctx);
    return xc::launch_contour_pieces(ctx, nrange, count, e_from, e_to, pts, ny, nx, periodic, ycoord, xcoord, period, radius, capacity,
                                     piece_count, first_edge, nseg, closed, winding, length, area, row_min, row_max);
}

int xc_set_cpiece_workspace(xc_ctx* ctx, uint64_t bytes)
{
    if (!ctx) return xc::fail(nullptr, XC_EBADARG, "null context");
    if (bytes < 1) return xc::fail(ctx, XC_EBADARG, "xc_set_cpiece_workspace: at least one byte (one range is always allowed)");
    ctx->cpiece_cap = (size_t)bytes;
    return XC_OK;
}

int xc_last_cpiece_profile(xc_ctx* ctx, double* ms, int* rounds, int* groups)
{
    return xc::profile_get(ctx, &xc_ctx::prof_cpiece, 4, ms, rounds, groups);
}

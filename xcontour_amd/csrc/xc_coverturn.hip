// K16 -- where a contour is OVERTURNED (gfx950): the crossings of every meridian with the selected pieces of K12's segment records,
// on the device.
//
// The reference's tests/test_breaking.py traces a PV contour and keeps "the largest contour fully encircling the pole" (Subroutines
// 4-5), and stops there.  The next step of a wave-breaking analysis asks where that contour folds over: where one meridian meets it
// three times or more, and how far in latitude the fold reaches.  Build-defined, in index space, integers and copies of K12's values only.
//
// Input: count[nrange], e_from, e_to, pts as xc_contour_segments[_periodic]_dev wrote them (xc_cpiece.hip states the record and the
// pieces); E = 2 ny nx bounds every edge id, labels and links are 32-bit (E < 2^31, fewer than 2^31 segments per range).
//
// Per GROUP of consecutive ranges (xc_cpiece_link.h: K13's groups under K13's cap, indices group-local):
//   phase A (K13's kernels)  k_cp_scatter, k_cp_link, R x k_cp_round: label = the piece's smallest e_from (its first_edge), prev >= 0 on
//                   every member of a ring and -1 on every member of an open piece
//   k_co_root, k_co_piece, k_co_pick  (xc_cpiece_select.h, shared with K17 and K24) the root of every piece, its nseg and winding, nsel, and
//                   the bid for the range's main ring under co_key
//   k_co_count      one thread per segment of a selected piece ('main': the piece whose key won): a start point on a vertical edge
//                   (e_from odd) is a crossing of column (e_from >> 1) % nx at row r1; the end point of a segment WITHOUT successor
//                   (tab[range][e_to] holds no segment: the tail of an open piece) with e_to odd is one at row r2.  Integer atomic add
//                   into ncross, atomic min / max on the row's bit pattern (rows are non-negative doubles: their bits order like
//                   the values).  The root of the main ring leaves its winding.
//   k_cp_unscatter  the table is handed on clean
// Around the groups: k_co_init (counts 0, row_lo +inf, row_hi 0, no main ring) and k_co_finish (NaN rows where nothing crossed; the
// winning key taken apart into main_first_edge and main_nseg; nsel of 'main').  The outputs are dense and fully written whatever the
// records hold; every index taken from a table is checked before it addresses anything; every launch has a fixed amount of work.
#include "xc_capi.h"
#include <vector>

namespace xc {
namespace {

#include "xc_cpiece_link.h"
#include "xc_cpiece_select.h"

__global__ __launch_bounds__(CP_TPB)
void k_co_init(int64_t ncol, int64_t nrange, int* __restrict__ ncross, double* __restrict__ row_lo, double* __restrict__ row_hi,
               int* __restrict__ nsel, long long* __restrict__ mfe, long long* __restrict__ mns, int* __restrict__ mw,
               unsigned long long* __restrict__ key)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i < ncol) { ncross[i] = 0; row_lo[i] = __longlong_as_double(0x7ff0000000000000ll); row_hi[i] = 0.0; }
    if (i < nrange) { nsel[i] = 0; mfe[i] = -1; mns[i] = 0; mw[i] = 0; key[i] = 0ull; }
}

__global__ __launch_bounds__(CP_TPB)
void k_co_count(int64_t n, long long s0, int64_t r0, long long E, int64_t nx, int select, const long long* __restrict__ e_from,
                const long long* __restrict__ e_to, const double* __restrict__ pts, const int* __restrict__ tab,
                const int* __restrict__ rid, const int* __restrict__ root, const int* __restrict__ prv, const int* __restrict__ lab,
                const unsigned* __restrict__ pn, const int* __restrict__ pw, const unsigned long long* __restrict__ key,
                int* __restrict__ ncross, double* __restrict__ row_lo, double* __restrict__ row_hi, int* __restrict__ mw)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= n) return;
    const int t = root[i], r = rid[i];                                // (k_co_root left 0 <= t < n)
    const bool ring = prv[i] >= 0;
    int w; bool ismain;
    const bool sel = co_selected(select, ring, t, lab[i], pn, pw, key[r0 + r], w, ismain);
    if (ismain && t == (int)i) mw[r0 + r] = w;
    if (!sel) return;
    const size_t out0 = (size_t)(r0 + r) * (size_t)nx;
    auto cross = [&](long long e, double row) {
        const size_t at = out0 + (size_t)((e >> 1) % nx);
        const unsigned long long b = (unsigned long long)__double_as_longlong(row);
        atomicAdd(ncross + at, 1);
        atomicMin((unsigned long long*)row_lo + at, b);
        atomicMax((unsigned long long*)row_hi + at, b);
    };
    const long long ef = e_from[s0 + i];
    if ((ef & 1) && ef >= 0 && ef < E) cross(ef, pts[4 * (size_t)(s0 + i)]);
    if (!ring) {
        const long long et = e_to[s0 + i];
        if ((et & 1) && et >= 0 && et < E) {
            const int j = tab[(size_t)r * E + et];
            if (j < 0 || j >= n) cross(et, pts[4 * (size_t)(s0 + i) + 2]);      // no successor: the tail of its piece
        }
    }
}

__global__ __launch_bounds__(CP_TPB)
void k_co_finish(int64_t ncol, int64_t nrange, int select, const int* __restrict__ ncross, double* __restrict__ row_lo,
                 double* __restrict__ row_hi, const unsigned long long* __restrict__ key, int* __restrict__ nsel,
                 long long* __restrict__ mfe, long long* __restrict__ mns)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i < ncol && ncross[i] == 0) {
        const double qnan = __longlong_as_double(0x7ff8000000000000ll);
        row_lo[i] = qnan; row_hi[i] = qnan;
    }
    if (i < nrange) {
        const unsigned long long k = key[i];
        if (k != 0ull) { mfe[i] = (long long)(CO_FE - (k & CO_FE)); mns[i] = (long long)(k >> 31); }
        if (select == 2) nsel[i] = k != 0ull ? 1 : 0;
    }
}

}  // namespace

// One xc_contour_overturning_dev call.  Waits for the stream twice: for K12's counts (they size the groups and fix the rounds) and
// for the word that says whether the records were K12's.
int launch_contour_overturning(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to, const double* pts,
                               int64_t ny, int64_t nx, int periodic, int select, int32_t* ncross, double* row_lo, double* row_hi, int32_t* nsel,
                               int64_t* main_first_edge, int64_t* main_nseg, int32_t* main_winding)
{
    if (!count || !ncross || !row_lo || !row_hi || !nsel || !main_first_edge || !main_nseg || !main_winding || nrange < 1 || ny < 1 || nx < 1)
        return fail(ctx, XC_EBADARG, "xc_contour_overturning: bad arguments");
    XC_TRY(co_check_select(ctx, "xc_contour_overturning", periodic, select));
    XC_TRY(co_check_plane(ctx, "xc_contour_overturning", periodic, ny, nx));
    if (nrange > ((int64_t)1 << 38) / nx) return fail(ctx, XC_EBADARG, "xc_contour_overturning: nrange nx must stay below 2^38");
    const long long E = 2 * ny * nx;
    const int wrap = periodic ? 1 : 0;
    CpProfile& prof = ctx->prof_coverturn;
    profile_clear(prof);

    CpPlan pl;                                                               // (no group without segments: the outputs are written all the same)
    XC_TRY(cp_plan(ctx, "xc_contour_overturning", nrange, count, nullptr, e_from, e_to, pts, E, pl));
    // workspace: off | key | err | the tail (xc_cpiece_link.h)
    long long* d_off; unsigned long long* key; int* d_err; CpTail tail;
    auto lay = [&](Carve c) {
        d_off = c.take<long long>((size_t)nrange + 1); key = c.take<unsigned long long>((size_t)nrange); d_err = c.take<int>(CP_SMALL);
        cp_carve_tail(c, pl, 6, tail);
        return c.at;
    };
    XC_TRY(lay_out(ctx, &ctx->cpiece_ws, &ctx->cpiece_ws_bytes, lay));

    StageTimer tm(ctx, prof.ms);                                             // where the time goes (xc_set_kernel_timing)
    CpRun run(ctx, tm, pl, e_from, e_to, d_off, tail, d_err);

    const int64_t ncol = nrange * nx;
    const dim3 ogrid(cp_blocks(ncol)), blk(CP_TPB);
    tm.mark(-1);
    hipLaunchKernelGGL(k_co_init, ogrid, blk, 0, ctx->stream, ncol, nrange, (int*)ncross, row_lo, row_hi, (int*)nsel, (long long*)main_first_edge,
                       (long long*)main_nseg, (int*)main_winding, key);
    XC_HIP(ctx, hipGetLastError());
    tm.mark(3);
    XC_HIP(ctx, hipMemsetAsync(d_err, 0, CP_SMALL * 4, ctx->stream));
    XC_TRY(run.upload_off());
    XC_TRY(run.fill_table());
    tm.mark(0);
    for (const CpGroup& g : pl.groups) {
        run.begin(g);
        XC_TRY(run.rounds());
        const CoRoles s = co_launch_select(run, wrap, nx, pts, select, (int*)nsel, key);
        XC_HIP(ctx, hipGetLastError());
        tm.mark(2);
        hipLaunchKernelGGL(k_co_count, run.grid, blk, 0, ctx->stream, run.n, run.s0, g.r0, E, nx, select, run.e_from, run.e_to, pts, tail.tab,
                           tail.rid, s.root, run.b.prv, run.b.lab, s.pn, s.pw, key, (int*)ncross, row_lo, row_hi, (int*)main_winding);
        XC_HIP(ctx, hipGetLastError());
        tm.mark(3);
        XC_TRY(run.end());
    }
    run.report(prof);
    hipLaunchKernelGGL(k_co_finish, ogrid, blk, 0, ctx->stream, ncol, nrange, select, (const int*)ncross, row_lo, row_hi, key, (int*)nsel,
                       (long long*)main_first_edge, (long long*)main_nseg);
    XC_HIP(ctx, hipGetLastError());
    tm.mark(3);
    int herr = 0;
    XC_TRY(cp_read_err(ctx, d_err, &herr));
    if (herr) return fail(ctx, XC_EBADARG, "xc_contour_overturning: an edge id outside [0, 2 ny nx)");
    return XC_OK;
}

}  // namespace xc

// ------------------------------------------------------------------------------------ C ABI
int xc_contour_overturning_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to, const double* pts,
                               int64_t ny, int64_t nx, int periodic, int select, int32_t* ncross, double* row_lo, double* row_hi, int32_t* nsel,
                               int64_t* main_first_edge, int64_t* main_nseg, int32_t* main_winding)
{
    XC_CTX(ctx);
    return xc::launch_contour_overturning(ctx, nrange, count, e_from, e_to, pts, ny, nx, periodic, select, ncross, row_lo, row_hi, nsel,
                                          main_first_edge, main_nseg, main_winding);
}

int xc_last_coverturn_profile(xc_ctx* ctx, double* ms, int* rounds, int* groups)
{
    return xc::profile_get(ctx, &xc_ctx::prof_coverturn, 4, ms, rounds, groups);
}

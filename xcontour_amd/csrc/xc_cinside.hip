// K17 -- what lies INSIDE the selected pieces of a contour (gfx950): node counts, weighted sums and a mask of the region they bound, from
// K12's segment records on the device.
//
// The package's other "integral within a contour" is the reference's threshold rule (every node with q > c), which puts cut-off blobs and
// filaments into the same bucket as the vortex they broke away from.  K16 selects "the largest contour fully encircling the pole"; this
// measures the region that one ring bounds.  Build-defined, in index space; the field is never read again.
//
// Input: count[nrange], e_from, e_to, pts as xc_contour_segments[_periodic]_dev wrote them; pieces, rings, winding, `select` and the main
// ring's tie rule are K16's (xc_cpiece_select.h).  E = 2 ny nx < 2^31 bounds every edge id.
//   X[r][c] = 1 iff the vertical edge V(r, c) carries a meridian crossing of a selected piece under K16's definition (the start point of a
//             segment with odd e_from, or the end point of a successor-less segment with odd e_to): column (id >> 1) % nx, row
//             (id >> 1) / nx.  Setting the flag is idempotent.
//   P[r][c] = XOR over r' < r of X[r'][c]: whether node (r, c) lies on the other side of the selected pieces from row 0 of its column.
//   inside  = P ^ flip.
//   per range: n_in = the inside nodes, sum_w = sum of w over them, sum_wf = sum of w f (one correctly rounded product per node), and the
//             mask itself.  The sums are K13's (xc_cpiece_sum.h): every term whole into CP_L limbs, rounded once.  The window's top sits
//             12 bits above max |w| (max |w f|) over the finite values of the range's slab, found by one pass before the scan.  A NaN
//             term is skipped; a +-inf term makes that sum of that range NaN.
//
// Per GROUP of consecutive ranges (xc_cpiece_link.h: K13's groups under K13's cap, indices group-local):
//   the group's bit planes are cleared: ny rows of wpr = ceil(nx / 32) 32-bit words per range, bit c & 31 of word c >> 5 of row r is
//                   X[r][c] -- the 64 lanes of a wave of the scan (consecutive columns) read two consecutive words per row
//   phase A (K13's kernels), k_co_root, k_co_piece, k_co_pick (K16's selection)
//   k_ci_mark       (xc_cinside_mark.h, shared with K24, like k_ci_chunk) one thread per segment of a selected piece: an atomic OR of its
//                   crossing bit(s); every id is checked first
//   k_cp_unscatter  the table is handed on clean
//   k_ci_chunk      (only where the rows are cut into more than one chunk) the XOR of every bit-plane word over the rows of each chunk
//   k_ci_scan       over the ranges from the end of the previous group to the end of this one (ranges without segments in front of the
//                   group have no crossing: their P is 0 everywhere): a block is 256 consecutive columns x one chunk of rows x one
//                   range.  A lane takes the XOR of the chunks above its own, then walks its rows with the parity in a register;
//                   w and f are read along x; n_in and the limbs of both sums stay in the lane's registers.  One wave reduction and
//                   one set of 64-bit integer atomics per wave close the pass.  The mask is written from the same walk.  Integer sums:
//                   the result depends neither on the chunks nor on the launch geometry.
// Around the groups: k_ci_bound (the maxima behind the windows), a last k_ci_scan for the ranges behind the last group, and k_ci_finish
// (the limbs rounded to double).  All outputs are dense and fully written whatever the records hold; every index taken from a record or a
// table is checked before it addresses anything; every launch has a fixed amount of work.
#include "xc_capi.h"
#include <algorithm>
#include <type_traits>
#include <vector>

namespace xc {
namespace {

#include "xc_binning.h"

#include "xc_cpiece_link.h"
#include "xc_cpiece_select.h"
#include "xc_cpiece_sum.h"
#include "xc_cinside_bound.h"
#include "xc_cinside_mark.h"

// Ranges [ra, ra + nr): block b is (column block, chunk, range).  Ranges of [g0, g1) have the bit plane bits[range - g0]; the others none.
template <typename FT, bool MASK>
__global__ __launch_bounds__(CI_TPB)
void k_ci_scan(int64_t ra, int64_t g0, int64_t g1, int64_t ny, int64_t nx, int64_t wpr, int64_t ncb, int64_t rc, int64_t nchunk, int ncont,
               unsigned flip, const unsigned* __restrict__ bits, const unsigned* __restrict__ cpar, const double* __restrict__ w,
               int w_per_slab, const FT* __restrict__ f, const unsigned long long* __restrict__ mx, unsigned long long* __restrict__ acc,
               unsigned long long* __restrict__ cnt, int* __restrict__ flg, unsigned char* __restrict__ mask)
{
    constexpr bool HASF = !std::is_void<FT>::value;
    const int64_t b = blockIdx.x;
    const int64_t cb = b % ncb, ch = (b / ncb) % nchunk, r = ra + b / (ncb * nchunk);
    const int64_t c = cb * CI_TPB + threadIdx.x;
    const bool active = c < nx;
    const int64_t s = r / ncont;
    const bool has = r >= g0 && r < g1;
    const size_t npl = (size_t)ny * (size_t)nx;
    const int64_t cw = c >> 5;
    const int cs = (int)(c & 31);
    const unsigned* bp = bits + (has ? (size_t)(r - g0) * (size_t)ny * (size_t)wpr : 0) + (size_t)cw;
    const double* wp = w ? w + (w_per_slab ? (size_t)s * npl : 0) + (size_t)c : nullptr;
    const int top_w = ci_top(mx[2 * s]);
    int top_f = 0;
    if constexpr (HASF) top_f = ci_top(mx[2 * s + 1]);

    unsigned p = flip;
    if (has && active)
        for (int64_t k = 0; k < ch; ++k) p ^= (cpar[(size_t)((r - g0) * nchunk + k) * (size_t)wpr + (size_t)cw] >> cs) & 1u;
    unsigned long long nin = 0ull, aw[CP_L], af[CP_L];
#pragma unroll
    for (int l = 0; l < CP_L; ++l) { aw[l] = 0ull; af[l] = 0ull; }
    int bad = 0;
    const int64_t row0 = ch * rc, row1 = row0 + rc < ny ? row0 + rc : ny;
    if (active) {
        for (int64_t row = row0; row < row1; ++row) {
            const size_t at = (size_t)row * (size_t)nx;
            if (p) {
                ++nin;
                const double a = wp ? wp[at] : 1.0;
                if (a == a && !cp_add_private(aw, a, top_w)) bad |= 1;
                if constexpr (HASF) {
                    const double t = __dmul_rn(a, (double)f[(size_t)s * npl + at + (size_t)c]);
                    if (t == t && !cp_add_private(af, t, top_f)) bad |= 2;
                }
            }
            if constexpr (MASK) mask[(size_t)r * npl + at + (size_t)c] = (unsigned char)p;
            if (has) p ^= (bp[(size_t)row * (size_t)wpr] >> cs) & 1u;
        }
    }
    // one wave, one set of atomics
    nin = ci_wave_sum(nin);
#pragma unroll
    for (int l = 0; l < CP_L; ++l) aw[l] = ci_wave_sum(aw[l]);
    if constexpr (HASF) {
#pragma unroll
        for (int l = 0; l < CP_L; ++l) af[l] = ci_wave_sum(af[l]);
    }
    const unsigned long long anybad1 = __ballot(bad & 1), anybad2 = __ballot(bad & 2);
    if ((threadIdx.x & 63) == 0) {
        if (nin) atomicAdd(cnt + r, nin);
        unsigned long long* pa = acc + (size_t)r * 2 * CP_L;
#pragma unroll
        for (int l = 0; l < CP_L; ++l) if (aw[l]) atomicAdd(pa + l, aw[l]);
        if constexpr (HASF) {
#pragma unroll
            for (int l = 0; l < CP_L; ++l) if (af[l]) atomicAdd(pa + CP_L + l, af[l]);
        }
        const int fl = (anybad1 ? 1 : 0) | (anybad2 ? 2 : 0);
        if (fl) atomicOr(flg + r, fl);
    }
}

__global__ __launch_bounds__(CP_TPB)
void k_ci_finish(int64_t nrange, int ncont, const unsigned long long* __restrict__ acc, const unsigned long long* __restrict__ cnt,
                 const int* __restrict__ flg, const unsigned long long* __restrict__ mx, long long* __restrict__ n_in,
                 double* __restrict__ sum_w, double* __restrict__ sum_wf)
{
    const int64_t r = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (r >= nrange) return;
    const int64_t s = r / ncont;
    const int fl = flg[r];
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    n_in[r] = (long long)cnt[r];
    sum_w[r] = (fl & 1) ? qnan : cp_to_double(acc + (size_t)r * 2 * CP_L, ci_top(mx[2 * s]));
    if (sum_wf) sum_wf[r] = (fl & 2) ? qnan : cp_to_double(acc + (size_t)r * 2 * CP_L + CP_L, ci_top(mx[2 * s + 1]));
}

}  // namespace

// One xc_contour_interior_dev call.  Waits for the stream twice: for K12's counts (they size the groups and fix the rounds) and for the
// word that says whether the records were K12's.
int launch_contour_interior(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to, const double* pts,
                            int64_t ny, int64_t nx, int periodic, int select, int flip, int ncont, const double* w, int w_per_slab,
                            const void* f, int f_dtype, int64_t* n_in, double* sum_w, double* sum_wf, uint8_t* mask)
{
    if (!count || !n_in || !sum_w || nrange < 1 || ny < 1 || nx < 1) return fail(ctx, XC_EBADARG, "xc_contour_interior: bad arguments");
    XC_TRY(co_check_select(ctx, "xc_contour_interior", periodic, select));
    if (flip != 0 && flip != 1) return fail(ctx, XC_EBADARG, "xc_contour_interior: flip is 0 or 1");
    if (ncont < 1 || nrange % ncont != 0) return fail(ctx, XC_EBADARG, "xc_contour_interior: nrange must be a multiple of ncont >= 1");
    if ((f == nullptr) != (sum_wf == nullptr)) return fail(ctx, XC_EBADARG, "xc_contour_interior: f and sum_wf go together");
    if (f && f_dtype != XC_F32 && f_dtype != XC_F64) return fail(ctx, XC_EBADARG, "xc_contour_interior: f_dtype is XC_F32 or XC_F64");
    XC_TRY(co_check_plane(ctx, "xc_contour_interior", periodic, ny, nx));
    const long long E = 2 * ny * nx;
    const int wrap = periodic ? 1 : 0;
    const int64_t nslab = nrange / ncont;
    if (nslab > 65535) return fail(ctx, XC_EBADARG, "xc_contour_interior: more than 65535 slabs");
    CpProfile& prof = ctx->prof_cinterior;
    profile_clear(prof);

    CpPlan pl;                                                               // (no group without segments: the outputs are written all the same)
    XC_TRY(cp_plan(ctx, "xc_contour_interior", nrange, count, nullptr, e_from, e_to, pts, E, pl));
    // the scan's geometry: 256 columns x rc rows x one range per block
    CiPlanes m(ny, nx, nrange);
    const int64_t wpr = m.geo.wpr, ncb = m.geo.ncb, nchunk = m.geo.nchunk, rc = m.geo.rc;
    // workspace: off | key, nsel, mx, acc, cnt, flg, err (cleared together) | bits[gmax][ny][wpr] | cpar[gmax][nchunk][wpr] | the tail
    //            (xc_cpiece_link.h)
    long long* d_off; unsigned long long *acc, *cnt; int *flg, *d_err; size_t b_zero = 0; CpTail tail;
    auto lay = [&](Carve c) {
        d_off = c.take<long long>((size_t)nrange + 1);
        b_zero = c.mark();
        m.carve_words(c, nrange, nslab);
        acc = c.take<unsigned long long>((size_t)nrange * 2 * CP_L); cnt = c.take<unsigned long long>((size_t)nrange); flg = c.take<int>((size_t)nrange);
        d_err = c.take<int>(CP_SMALL);
        b_zero = c.mark() - b_zero;
        m.carve_planes(c, pl.gmax);
        cp_carve_tail(c, pl, 6, tail);
        return c.at;
    };
    XC_TRY(lay_out(ctx, &ctx->cpiece_ws, &ctx->cpiece_ws_bytes, lay));

    StageTimer tm(ctx, prof.ms);                                             // where the time goes (xc_set_kernel_timing)
    CpRun run(ctx, tm, pl, e_from, e_to, d_off, tail, d_err);

    const dim3 blk(CP_TPB);
    const int64_t npl = ny * nx;
    // the scan of the ranges [a, b), those of [g0, g1) with their bit planes; as many launches as keep a grid below 2^31 blocks
    auto scan = [&](int64_t a, int64_t b, int64_t g0, int64_t g1) -> int {
        const int64_t per = ncb * nchunk, step = std::max<int64_t>(1, (((int64_t)1 << 31) - 1) / per);
        for (int64_t ra = a; ra < b; ra += step) {
            const int64_t nr = std::min<int64_t>(step, b - ra);
            const dim3 grid((unsigned)(nr * per));
#define XC_CI_SCAN(FT_, M_) hipLaunchKernelGGL((k_ci_scan<FT_, M_>), grid, dim3(CI_TPB), 0, ctx->stream, ra, g0, g1, ny, nx, wpr, ncb, rc, nchunk, ncont, \
                                               (unsigned)flip, m.bits, m.cpar, w, w_per_slab, (const FT_*)f, m.mx, acc, cnt, flg, (unsigned char*)mask)
            if (!f) { if (mask) XC_CI_SCAN(void, true); else XC_CI_SCAN(void, false); }
            else if (f_dtype == XC_F32) { if (mask) XC_CI_SCAN(float, true); else XC_CI_SCAN(float, false); }
            else { if (mask) XC_CI_SCAN(double, true); else XC_CI_SCAN(double, false); }
#undef XC_CI_SCAN
            XC_HIP(ctx, hipGetLastError());
        }
        return XC_OK;
    };

    tm.mark(-1);
    XC_HIP(ctx, hipMemsetAsync(m.key, 0, b_zero, ctx->stream));
    ci_launch_bound(ctx->stream, npl, nslab, w, w_per_slab, f, f_dtype, m.mx);
    XC_HIP(ctx, hipGetLastError());
    tm.mark(3);
    XC_TRY(run.upload_off());
    XC_TRY(run.fill_table());
    tm.mark(0);
    int64_t done = 0;                                                       // the ranges scanned so far
    for (const CpGroup& g : pl.groups) {
        const int64_t ng = g.r1 - g.r0;
        CoRoles s;
        XC_TRY(ci_mark_group(run, g, m, wrap, nx, pts, select, s));
        XC_HIP(ctx, hipGetLastError());
        tm.mark(3);
        XC_TRY(run.end());
        if (nchunk > 1) {
            const int64_t nwords = ng * nchunk * wpr;
            hipLaunchKernelGGL(k_ci_chunk, dim3(cp_blocks(nwords)), blk, 0, ctx->stream, nwords, ny, wpr, rc, nchunk, m.bits, m.cpar);
            XC_HIP(ctx, hipGetLastError());
        }
        XC_TRY(scan(done, g.r1, g.r0, g.r1));
        done = g.r1;
        tm.mark(3);
    }
    if (done < nrange) XC_TRY(scan(done, nrange, 0, 0));
    run.report(prof);
    hipLaunchKernelGGL(k_ci_finish, dim3(cp_blocks(nrange)), blk, 0, ctx->stream, nrange, ncont, acc, cnt, flg, m.mx, (long long*)n_in, sum_w, sum_wf);
    XC_HIP(ctx, hipGetLastError());
    tm.mark(3);
    int herr = 0;
    XC_TRY(cp_read_err(ctx, d_err, &herr));
    if (herr) return fail(ctx, XC_EBADARG, "xc_contour_interior: an edge id outside [0, 2 ny nx)");
    return XC_OK;
}

}  // namespace xc

// ------------------------------------------------------------------------------------ C ABI
int xc_contour_interior_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to, const double* pts,
                            int64_t ny, int64_t nx, int periodic, int select, int flip, int ncont, const double* w, int w_per_slab,
                            const void* f, int f_dtype, int64_t* n_in, double* sum_w, double* sum_wf, uint8_t* mask)
{
    XC_CTX(ctx);
    return xc::launch_contour_interior(ctx, nrange, count, e_from, e_to, pts, ny, nx, periodic, select, flip, ncont, w, w_per_slab, f, f_dtype,
                                       n_in, sum_w, sum_wf, mask);
}

int xc_last_cinterior_profile(xc_ctx* ctx, double* ms, int* rounds, int* groups)
{
    return xc::profile_get(ctx, &xc_ctx::prof_cinterior, 4, ms, rounds, groups);
}

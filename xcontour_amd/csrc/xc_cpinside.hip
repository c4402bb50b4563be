// K18 -- what lies INSIDE EVERY PIECE of a contour (gfx950): per ring the nodes it encloses and the sums of w and w f over them, from K12's
// segment records on the device.  K17 (xc_cinside.hip) answers for one selection per range and scans the whole plane for it; this answers
// for every piece of every range in one call, at a cost proportional to the nodes the rings enclose.
//
// The rule (include/xcontour_hip.h, K18 section) is K17's with the selection being one piece p:
//   X_p[r][c] = 1 iff V(r, c) carries a meridian crossing of a segment of p;  P_p[r][c] = XOR over r' < r of X_p[r'][c];
//   ring of winding 0: inside = P_p;  ring of winding != 0: inside = P_p ^ flip;  open piece: n_in = -1, both sums NaN.
// Pieces, closed, winding, nseg, first_edge and the slots are K13's; the sums are K17's (xc_cpiece_sum.h, the tops of xc_cinside_bound.h).
//
// The mapping rests on two facts about a ring of K12's records: it is a simple closed curve, so down one column its crossings alternate
// between entering and leaving; and the ids alone say which of the two a crossing is, up to one sign per ring:
//   a segment with e_from = V(r, c) lies in cell (r, c) when its e_to is H(r, c), H(r+1, c) or V(r, (c+1) % nx), else in cell (r, c-1)
//   (the seam cell for c = 0 of a periodic plane).  By K12's direction table (xc_cseg_cell.h) a segment that starts on a cell's left edge
//   has the node BELOW the crossing above the level, one that starts on a cell's right edge the node ABOVE it: s = +1 / -1.
//   The ring's sign S, from two integer sums over its crossings: winding 0 -- the crossings pair up into (entering at row a, leaving at
//   row b > a) with opposite s, so B = sum of s x row is -(the nodes enclosed) when the entering ones have s = +1 and +(...) otherwise:
//   S = +1 for B < 0, -1 for B > 0.  Winding != 0 -- every column has one crossing more with the parity-1 side below it than above it, so
//   A = sum of s is +-nx: S = the sign of A.  A crossing with s == S has the side of parity 1 below it.
// nx == 2 on a periodic plane makes V(r, c+1) and V(r, c-1) the same edge: nx < 3 with periodic is refused.
//
// Per GROUP of consecutive ranges (xc_cpiece_link.h: K13's groups under K13's cap, indices group-local):
//   phase A (K13's kernels), k_cp_root (K13's roots and slots, xc_cpiece_slot.h)
//   the host reads the group's piece counts (they place the group's pieces in the table; once the pieces no longer fit `capacity` the
//   rest of the call only counts)
//   k_pi_init       the staged records of the group's pieces are cleared
//   k_pi_piece      one thread per segment, integer atomics onto its piece: nseg, the winding by K13's seam count, A and B; the root
//                   writes first_edge and closed
//   k_pi_walk       one thread per segment with odd e_from of a ring and s == S.  Winding 0, or winding != 0 without flip: it walks DOWN
//                   its column from row r + 1, reading the group's edge table -- tab[V(r', c)] is the segment that starts there, root[] of
//                   it its piece -- and stops behind the next crossing of its own piece, or at row ny - 1.  Winding != 0 with flip: it
//                   walks UP from row r and stops before the previous crossing of its own piece, or at row 0.  n_in and the limbs of both
//                   sums stay in registers; one set of 64-bit integer atomics onto the piece's slot closes the walk.  At most ny steps.
//   k_cp_unscatter  the table is handed on clean
// Around the groups: k_ci_bound (K17's maxima behind the windows) and k_pi_finish (the limbs rounded to double, the records written to
// the caller's arrays -- only when all pieces fit).  The edge-table reads of a walk run along a column: one 4-byte read per step from a
// line of its own (DESIGN.md says what that costs).  Every index taken from a record or a table is checked before it addresses
// anything; no kernel waits for another block.
#include "xc_capi.h"
#include <algorithm>
#include <type_traits>
#include <vector>

namespace xc {
namespace {

#include "xc_binning.h"

#include "xc_cpiece_link.h"
#include "xc_cpiece_slot.h"
#include "xc_cpiece_sum.h"
#include "xc_cinside_bound.h"
#include "xc_cpiece_interior.h"                                             // PiStage and K18's kernels (K19 runs them too)

}  // namespace

// One xc_contour_piece_interiors_dev call.  Waits for the stream once for K12's counts, once per group for its piece counts, and once at the
// end.
int launch_contour_piece_interiors(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to,
                                   const double* pts, int64_t ny, int64_t nx, int periodic, int flip, int ncont, const double* w,
                                   int w_per_slab, const void* f, int f_dtype, int64_t capacity, uint64_t* piece_count, int64_t* first_edge,
                                   int64_t* nseg, int32_t* closed, int32_t* winding, int64_t* n_in, double* sum_w, double* sum_wf)
{
    const char* who = "xc_contour_piece_interiors";
    if (!count || !piece_count || nrange < 1 || ny < 1 || nx < 1 || capacity < 0) return fail(ctx, XC_EBADARG, std::string(who) + ": bad arguments");
    if (flip != 0 && flip != 1) return fail(ctx, XC_EBADARG, std::string(who) + ": flip is 0 or 1");
    if (ncont < 1 || nrange % ncont != 0) return fail(ctx, XC_EBADARG, std::string(who) + ": nrange must be a multiple of ncont >= 1");
    if (f && f_dtype != XC_F32 && f_dtype != XC_F64) return fail(ctx, XC_EBADARG, std::string(who) + ": f_dtype is XC_F32 or XC_F64");
    if (capacity > 0 && (!first_edge || !nseg || !closed || !winding || !n_in || !sum_w))
        return fail(ctx, XC_EBADARG, std::string(who) + ": capacity > 0 needs the record arrays");
    if (capacity > 0 && (f == nullptr) != (sum_wf == nullptr)) return fail(ctx, XC_EBADARG, std::string(who) + ": f and sum_wf go together");
    if (periodic && nx < 3) return fail(ctx, XC_EBADARG, std::string(who) + ": a periodic plane needs nx >= 3 (with two columns a cell's two vertical edges are one)");
    if (ny > (((int64_t)1 << 30) - 1) / nx) return fail(ctx, XC_EBADARG, std::string(who) + ": plane too large for 32-bit labels (2 ny nx < 2^31)");
    const long long E = 2 * ny * nx;
    const int wrap = periodic ? 1 : 0;
    const int64_t nslab = nrange / ncont;
    if (nslab > 65535) return fail(ctx, XC_EBADARG, std::string(who) + ": more than 65535 slabs");
    for (int k = 0; k < 4; ++k) ctx->cpinside_ms[k] = 0.f;
    ctx->cpinside_rounds = 0; ctx->cpinside_groups = 0;

    std::vector<uint64_t> hc((size_t)nrange);
    XC_HIP(ctx, hipMemcpyAsync(hc.data(), count, (size_t)nrange * 8, hipMemcpyDeviceToHost, ctx->stream));
    XC_HIP(ctx, hipMemsetAsync(piece_count, 0, (size_t)nrange * 8, ctx->stream));
    XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<long long> off((size_t)nrange + 1);
    off[0] = 0;
    for (int64_t r = 0; r < nrange; ++r) {
        if (hc[(size_t)r] >= (1ull << 31)) return fail(ctx, XC_EBADARG, std::string(who) + ": a range of 2^31 or more segments");
        off[(size_t)r + 1] = off[(size_t)r] + (long long)hc[(size_t)r];
    }
    const long long total = off[(size_t)nrange];
    if (total == 0) return XC_OK;
    if (!e_from || !e_to || !pts) return fail(ctx, XC_EBADARG, std::string(who) + ": segments without their records");
    const int64_t cap = std::min<int64_t>(capacity, total);               // a piece has a segment: no more pieces than segments

    int64_t gmax = 1; long long nmax = 0;
    const std::vector<CpGroup> groups = cp_plan_groups(ctx->cpiece_cap, E, nrange, hc, off, &gmax, &nmax);
    // workspace: off | poff | mx[nslab][2], err (cleared together) | tab[gmax][E] | rid[nmax] | label, next, prev x 2 [nmax]
    const size_t b_off = al((size_t)(nrange + 1) * 8), b_mx = al((size_t)nslab * 16), b_small = 256;
    const size_t b_tab = al((size_t)gmax * (size_t)E * 4), b_n = al((size_t)nmax * 4);
    XC_TRY(grow(ctx, &ctx->cpiece_ws, &ctx->cpiece_ws_bytes, 2 * b_off + b_mx + b_small + b_tab + 7 * b_n));
    char* ws = (char*)ctx->cpiece_ws;
    long long* d_off = (long long*)ws;
    long long* d_poff = (long long*)(ws + b_off);
    unsigned long long* mx = (unsigned long long*)(ws + 2 * b_off);
    int* d_err = (int*)((char*)mx + b_mx);
    int* tab = (int*)((char*)d_err + b_small);
    int* rid = (int*)((char*)tab + b_tab);
    int* buf[6];
    for (int k = 0; k < 6; ++k) buf[k] = (int*)((char*)rid + (size_t)(k + 1) * b_n);
    // the staged records: nothing reaches the caller's arrays before all pieces are known to fit
    PiStage st = {};
    if (cap > 0) {
        const size_t b8 = al((size_t)cap * 8), b4 = al((size_t)cap * 4), b_acc = al((size_t)cap * 2 * CP_L * 8);
        XC_TRY(grow(ctx, &ctx->cpiece_acc, &ctx->cpiece_acc_bytes, b_acc + 5 * b8 + 3 * b4));
        char* a = (char*)ctx->cpiece_acc;
        st.acc = (unsigned long long*)a; a += b_acc;
        st.cnt = (unsigned long long*)a; a += b8;
        st.sa = (unsigned long long*)a; a += b8;
        st.sb = (unsigned long long*)a; a += b8;
        st.ns = (unsigned long long*)a; a += b8;
        st.fe = (long long*)a; a += b8;
        st.wd = (int*)a; a += b4;
        st.cl = (int*)a; a += b4;
        st.flg = (int*)a;
    }

    // where the time goes (xc_set_kernel_timing): events between the stages, summed per kind after the call
    std::vector<std::pair<hipEvent_t, int>> marks;
    auto mark = [&](int kind) {
        if (!ctx->timing) return;
        hipEvent_t ev;
        if (hipEventCreate(&ev) != hipSuccess) return;
        (void)hipEventRecord(ev, ctx->stream);
        marks.push_back({ev, kind});
    };
    auto settle = [&]() {
        for (size_t k = 1; k < marks.size(); ++k) {
            float ms = 0.f;
            if (marks[k].second >= 0 && hipEventElapsedTime(&ms, marks[k - 1].first, marks[k].first) == hipSuccess) ctx->cpinside_ms[marks[k].second] += ms;
        }
        for (auto& m : marks) (void)hipEventDestroy(m.first);
        marks.clear();
    };

    const dim3 blk(CP_TPB);
    const int64_t npl = ny * nx;
    mark(-1);
    XC_HIP(ctx, hipMemsetAsync(mx, 0, b_mx + b_small, ctx->stream));
    if (cap > 0) {
        const dim3 bgrid((unsigned)std::min<int64_t>((npl + CI_TPB - 1) / CI_TPB, 1024), (unsigned)nslab);
        if (!f) hipLaunchKernelGGL((k_ci_bound<void>), bgrid, dim3(CI_TPB), 0, ctx->stream, npl, w, w_per_slab, (const void*)nullptr, mx);
        else if (f_dtype == XC_F32) hipLaunchKernelGGL((k_ci_bound<float>), bgrid, dim3(CI_TPB), 0, ctx->stream, npl, w, w_per_slab, (const float*)f, mx);
        else hipLaunchKernelGGL((k_ci_bound<double>), bgrid, dim3(CI_TPB), 0, ctx->stream, npl, w, w_per_slab, (const double*)f, mx);
        XC_HIP(ctx, hipGetLastError());
    }
    mark(3);
    XC_HIP(ctx, hipMemcpyAsync(d_off, off.data(), (size_t)(nrange + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    XC_HIP(ctx, hipMemsetAsync(tab, 0xff, (size_t)gmax * (size_t)E * 4, ctx->stream));
    mark(0);

    std::vector<uint64_t> hp((size_t)nrange, 0);
    std::vector<long long> poff((size_t)nrange + 1, 0);
    int64_t done = 0;                                                       // poff[0 .. done] stand
    bool over = cap == 0;                                                   // the pieces no longer fit: count only
    int rounds_total = 0;
    for (const CpGroup& g : groups) {
        const long long s0 = off[(size_t)g.r0];
        const int64_t n = off[(size_t)g.r1] - s0, ng = g.r1 - g.r0;
        const int R = cp_rounds(hc, g);                                    // ceil(log2(largest count)) + 1
        const dim3 grid(cp_blocks(n));
        int *lab = buf[0], *nxt = buf[1], *prv = buf[2], *lab2 = buf[3], *nxt2 = buf[4], *prv2 = buf[5];
        hipLaunchKernelGGL(k_cp_scatter, grid, blk, 0, ctx->stream, n, s0, d_off, g.r0, g.r1, E, (const long long*)e_from, tab, rid, lab, prv, d_err);
        hipLaunchKernelGGL(k_cp_link, grid, blk, 0, ctx->stream, n, s0, E, (const long long*)e_to, tab, rid, nxt, prv, d_err);
        XC_HIP(ctx, hipGetLastError());
        mark(0);
        for (int k = 0; k < R; ++k) {
            hipLaunchKernelGGL(k_cp_round, grid, blk, 0, ctx->stream, n, lab, nxt, prv, lab2, nxt2, prv2);
            std::swap(lab, lab2); std::swap(nxt, nxt2); std::swap(prv, prv2);
        }
        XC_HIP(ctx, hipGetLastError());
        rounds_total += R;
        mark(1);
        int *root = nxt2, *slot = lab2;
        hipLaunchKernelGGL(k_cp_root, grid, blk, 0, ctx->stream, n, E, tab, rid, lab, prv, g.r0, (unsigned long long*)piece_count, root, slot);
        XC_HIP(ctx, hipGetLastError());
        // the group's piece counts place its pieces in the table
        XC_HIP(ctx, hipMemcpyAsync(hp.data() + g.r0, piece_count + g.r0, (size_t)ng * 8, hipMemcpyDeviceToHost, ctx->stream));
        XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (; done < g.r1; ++done) poff[(size_t)done + 1] = poff[(size_t)done] + (long long)hp[(size_t)done];
        const long long p0 = poff[(size_t)g.r0], p1 = poff[(size_t)g.r1];
        if (p1 > cap) over = true;
        if (!over && p1 > p0) {
            XC_HIP(ctx, hipMemcpyAsync(d_poff + g.r0, poff.data() + g.r0, (size_t)(ng + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL(k_pi_init, dim3(cp_blocks(p1 - p0)), blk, 0, ctx->stream, (int64_t)p0, (int64_t)p1, st);
            hipLaunchKernelGGL(k_pi_piece, grid, blk, 0, ctx->stream, n, s0, g.r0, E, ny, nx, wrap, cap, (const long long*)e_from,
                               (const long long*)e_to, pts, rid, root, slot, (const unsigned long long*)piece_count, d_poff, st, d_err);
            XC_HIP(ctx, hipGetLastError());
            mark(2);
#define XC_PI_WALK(FT_) hipLaunchKernelGGL((k_pi_walk<FT_>), grid, blk, 0, ctx->stream, n, s0, g.r0, E, ny, nx, flip, ncont, cap, (const long long*)e_from, \
                                           (const long long*)e_to, tab, rid, root, slot, (const unsigned long long*)piece_count, d_poff, w, w_per_slab,      \
                                           (const FT_*)f, mx, st, d_err)
            if (!f) XC_PI_WALK(void); else if (f_dtype == XC_F32) XC_PI_WALK(float); else XC_PI_WALK(double);
#undef XC_PI_WALK
            XC_HIP(ctx, hipGetLastError());
            mark(3);
        } else {
            mark(2);
        }
        hipLaunchKernelGGL(k_cp_unscatter, grid, blk, 0, ctx->stream, n, s0, E, (const long long*)e_from, rid, tab);
        XC_HIP(ctx, hipGetLastError());
        mark(0);
    }
    for (; done < nrange; ++done) poff[(size_t)done + 1] = poff[(size_t)done] + (long long)hp[(size_t)done];
    ctx->cpinside_rounds = rounds_total; ctx->cpinside_groups = (int)groups.size();
    const long long np = poff[(size_t)nrange];
    int herr = 0;
    XC_HIP(ctx, hipMemcpyAsync(&herr, d_err, 4, hipMemcpyDeviceToHost, ctx->stream));
    XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (herr & CP_ERR_EDGE) { settle(); return fail(ctx, XC_EBADARG, std::string(who) + ": an edge id outside [0, 2 ny nx)"); }
    if (herr) { settle(); return fail(ctx, XC_EBADARG, std::string(who) + ": the records are not those of one xc_contour_segments call (a repeated edge id)"); }
    if (np > capacity) { settle(); return 1; }
    XC_HIP(ctx, hipMemcpyAsync(d_poff, poff.data(), (size_t)(nrange + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_pi_finish, dim3(cp_blocks(np)), blk, 0, ctx->stream, (int64_t)np, nrange, ncont, d_poff, st, mx, (long long*)first_edge,
                       (long long*)nseg, (int*)closed, (int*)winding, (long long*)n_in, sum_w, sum_wf);
    XC_HIP(ctx, hipGetLastError());
    mark(3);
    XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    settle();
    return XC_OK;
}

}  // namespace xc

// ------------------------------------------------------------------------------------ C ABI
int xc_contour_piece_interiors_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to,
                                   const double* pts, int64_t ny, int64_t nx, int periodic, int flip, int ncont, const double* w,
                                   int w_per_slab, const void* f, int f_dtype, int64_t capacity, uint64_t* piece_count, int64_t* first_edge,
                                   int64_t* nseg, int32_t* closed, int32_t* winding, int64_t* n_in, double* sum_w, double* sum_wf)
{
    XC_CTX(ctx);
    return xc::launch_contour_piece_interiors(ctx, nrange, count, e_from, e_to, pts, ny, nx, periodic, flip, ncont, w, w_per_slab, f, f_dtype,
                                              capacity, piece_count, first_edge, nseg, closed, winding, n_in, sum_w, sum_wf);
}

int xc_last_cpinside_profile(xc_ctx* ctx, double* ms, int* rounds, int* groups)
{
    if (!ctx) return xc::fail(nullptr, XC_EBADARG, "null context");
    if (ms) for (int k = 0; k < 4; ++k) ms[k] = (double)ctx->cpinside_ms[k];
    if (rounds) *rounds = ctx->cpinside_rounds;
    if (groups) *groups = ctx->cpinside_groups;
    return XC_OK;
}

// K19 -- which piece of a contour is NESTED in which (gfx950): per ring its parent (the innermost ring that encloses it), its depth, the
// number of its children and what it bounds NET of them, beside K18's records, from K12's segment records on the device.
//
// The rule (include/xcontour_hip.h, K19 section): with I_p K18's inside set of ring p, a encloses b iff I_b is a subset of I_a; parent[b] is
// the enclosing ring with the fewest inside nodes; open pieces are transparent; the net records are those of I_p minus its children's sets.
//
// The mapping rests on K18's facts (xc_cpinside.hip) and two more.  Rings of one range do not meet, so two of them are nested or disjoint,
// and a ring other than b holds ALL of I_b as soon as it holds the one node that lies across b's boundary from a node of I_b.  And down a
// column a ring's crossings alternate, so a walker that enters a ring it started outside of is outside again behind that ring's next
// crossing: whatever it meets in between is nested in that ring and cannot hold the start node.
//   OUTSIDE NODE   without flip row 0 lies outside EVERY ring (P = 0 there): the node ABOVE a ring's topmost crossing (the smallest odd
//                  e_from among its crossings) is outside it, and between that node and row 0 the column never meets the ring again.
//                  With flip row 0 lies INSIDE every ring that goes round, and it is row ny - 1 that lies outside every ring (a ring of
//                  winding 0 has an even number of crossings above it, one that goes round an odd number): the node BELOW a ring's
//                  bottommost crossing is outside it.  A walk that ends on the row that is outside everything has missed no ring.
//   PARENT WALK    from that node away from the ring, to row 0 (with flip: to row ny - 1).  A crossing of another ring x has x's inside BELOW it iff
//                  (s == S_x) != (winding_x != 0 && flip) (K18's s and S).  Inside on the walker's side: the walker is inside x, and x is
//                  the innermost such ring -- parent = x.  Inside on the far side: the walker enters x from outside and skips everything up
//                  to x's next crossing in this column.  Crossings of open pieces are ignored.  One `skip` register; at most ny steps.
//
// Per group, between K18's walks and k_cp_unscatter (the edge table, root[] and slot[] still stand):
//   k_pt_init    the staged tree records of the group's pieces are cleared
//   k_pt_top     one thread per segment: one 64-bit integer atomicMin of its crossing's key onto its ring (e_from, or ~e_from with
//                flip, when the walks go down, so that one minimum serves both)
//   k_pt_parent  one thread per ring: the parent walk; one integer atomic counts the child at its parent
//   k_pt_depth   one thread per ring chases its parents, at most the range's piece count of them; a chase that does not end there sets
//                PT_ERR_TREE in the err word (XC_EBADARG after the call)
//   k_pt_net     every ring with a parent adds its NEGATED n_in and limbs to the parent's net words, with 64-bit integer atomics.  K18's
//                limbs are signed sums of 32-bit chunks in two's-complement 64-bit words, so negation is exact, and the words of
//                (gross - children) are the words the net nodes alone would have given: cp_to_double rounds the exact net sum once.
// k_pt_finish adds the gross and the net words and writes the records, after k_pi_finish has written K18's.  Every index taken from a
// record or a table is checked before it addresses anything; no kernel waits for another block; no LDS, no scratch.
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
#include "xc_cpiece_interior.h"
#include "xc_cpiece_tree.h"                                                 // PtStage and K19's kernels (K20 runs them too)

}  // namespace

// One xc_contour_piece_tree_dev call: K18's (xc_cpinside.hip) with the tree stages per group.  Waits for the stream as K18 does.
int launch_contour_piece_tree(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to,
                              const double* pts, int64_t ny, int64_t nx, int periodic, int flip, int ncont, const double* w,
                              int w_per_slab, const void* f, int f_dtype, int64_t capacity, uint64_t* piece_count, int64_t* first_edge,
                              int64_t* nseg, int32_t* closed, int32_t* winding, int64_t* n_in, double* sum_w, double* sum_wf,
                              int64_t* parent, int32_t* depth, int32_t* nchild, int64_t* n_net, double* net_w, double* net_wf)
{
    const char* who = "xc_contour_piece_tree";
    if (!count || !piece_count || nrange < 1 || ny < 1 || nx < 1 || capacity < 0) return fail(ctx, XC_EBADARG, std::string(who) + ": bad arguments");
    if (flip != 0 && flip != 1) return fail(ctx, XC_EBADARG, std::string(who) + ": flip is 0 or 1");
    if (ncont < 1 || nrange % ncont != 0) return fail(ctx, XC_EBADARG, std::string(who) + ": nrange must be a multiple of ncont >= 1");
    if (f && f_dtype != XC_F32 && f_dtype != XC_F64) return fail(ctx, XC_EBADARG, std::string(who) + ": f_dtype is XC_F32 or XC_F64");
    if (capacity > 0 && (!first_edge || !nseg || !closed || !winding || !n_in || !sum_w || !parent || !depth || !nchild || !n_net || !net_w))
        return fail(ctx, XC_EBADARG, std::string(who) + ": capacity > 0 needs the record arrays");
    if (capacity > 0 && ((f == nullptr) != (sum_wf == nullptr) || (f == nullptr) != (net_wf == nullptr)))
        return fail(ctx, XC_EBADARG, std::string(who) + ": f, sum_wf and net_wf go together");
    if (periodic && nx < 3) return fail(ctx, XC_EBADARG, std::string(who) + ": a periodic plane needs nx >= 3 (with two columns a cell's two vertical edges are one)");
    if (ny > (((int64_t)1 << 30) - 1) / nx) return fail(ctx, XC_EBADARG, std::string(who) + ": plane too large for 32-bit labels (2 ny nx < 2^31)");
    const long long E = 2 * ny * nx;
    const int wrap = periodic ? 1 : 0;
    const int64_t nslab = nrange / ncont;
    if (nslab > 65535) return fail(ctx, XC_EBADARG, std::string(who) + ": more than 65535 slabs");
    for (int k = 0; k < 5; ++k) ctx->cptree_ms[k] = 0.f;
    ctx->cptree_rounds = 0; ctx->cptree_groups = 0;

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
    // workspace (K18's): off | poff | mx[nslab][2], err (cleared together) | tab[gmax][E] | rid[nmax] | label, next, prev x 2 [nmax]
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
    // the staged records, K18's and then the tree's: nothing reaches the caller's arrays before all pieces are known to fit
    PiStage st = {};
    PtStage pt = {};
    if (cap > 0) {
        const size_t b8 = al((size_t)cap * 8), b4 = al((size_t)cap * 4), b_acc = al((size_t)cap * 2 * CP_L * 8);
        XC_TRY(grow(ctx, &ctx->cpiece_acc, &ctx->cpiece_acc_bytes, 2 * b_acc + 8 * b8 + 5 * b4));
        char* a = (char*)ctx->cpiece_acc;
        st.acc = (unsigned long long*)a; a += b_acc;
        st.cnt = (unsigned long long*)a; a += b8;
        st.sa = (unsigned long long*)a; a += b8;
        st.sb = (unsigned long long*)a; a += b8;
        st.ns = (unsigned long long*)a; a += b8;
        st.fe = (long long*)a; a += b8;
        st.wd = (int*)a; a += b4;
        st.cl = (int*)a; a += b4;
        st.flg = (int*)a; a += b4;
        pt.net = (unsigned long long*)a; a += b_acc;
        pt.key = (unsigned long long*)a; a += b8;
        pt.nnet = (unsigned long long*)a; a += b8;
        pt.par = (long long*)a; a += b8;
        pt.nch = (int*)a; a += b4;
        pt.dep = (int*)a;
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
            if (marks[k].second >= 0 && hipEventElapsedTime(&ms, marks[k - 1].first, marks[k].first) == hipSuccess) ctx->cptree_ms[marks[k].second] += ms;
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
            const dim3 pgrid(cp_blocks(p1 - p0));
            const unsigned long long* pcnt = (const unsigned long long*)piece_count;
            XC_HIP(ctx, hipMemcpyAsync(d_poff + g.r0, poff.data() + g.r0, (size_t)(ng + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL(k_pi_init, pgrid, blk, 0, ctx->stream, (int64_t)p0, (int64_t)p1, st);
            hipLaunchKernelGGL(k_pi_piece, grid, blk, 0, ctx->stream, n, s0, g.r0, E, ny, nx, wrap, cap, (const long long*)e_from,
                               (const long long*)e_to, pts, rid, root, slot, pcnt, d_poff, st, d_err);
            XC_HIP(ctx, hipGetLastError());
            mark(2);
#define XC_PI_WALK(FT_) hipLaunchKernelGGL((k_pi_walk<FT_>), grid, blk, 0, ctx->stream, n, s0, g.r0, E, ny, nx, flip, ncont, cap, (const long long*)e_from, \
                                           (const long long*)e_to, tab, rid, root, slot, pcnt, d_poff, w, w_per_slab, (const FT_*)f, mx, st, d_err)
            if (!f) XC_PI_WALK(void); else if (f_dtype == XC_F32) XC_PI_WALK(float); else XC_PI_WALK(double);
#undef XC_PI_WALK
            XC_HIP(ctx, hipGetLastError());
            mark(3);
            hipLaunchKernelGGL(k_pt_init, pgrid, blk, 0, ctx->stream, (int64_t)p0, (int64_t)p1, pt);
            hipLaunchKernelGGL(k_pt_top, grid, blk, 0, ctx->stream, n, s0, g.r0, E, ny, nx, flip, cap, (const long long*)e_from,
                               (const long long*)e_to, rid, root, slot, pcnt, d_poff, st, pt, d_err);
            hipLaunchKernelGGL(k_pt_parent, pgrid, blk, 0, ctx->stream, (int64_t)p0, (int64_t)p1, n, s0, g.r0, g.r1, E, ny, nx, flip, cap,
                               (const long long*)e_from, (const long long*)e_to, tab, root, slot, pcnt, d_poff, st, pt, d_err);
            hipLaunchKernelGGL(k_pt_depth, pgrid, blk, 0, ctx->stream, (int64_t)p0, (int64_t)p1, g.r0, g.r1, d_poff, st, pt, d_err);
            hipLaunchKernelGGL(k_pt_net, pgrid, blk, 0, ctx->stream, (int64_t)p0, (int64_t)p1, st, pt);
            XC_HIP(ctx, hipGetLastError());
            mark(4);
        } else {
            mark(2);
        }
        hipLaunchKernelGGL(k_cp_unscatter, grid, blk, 0, ctx->stream, n, s0, E, (const long long*)e_from, rid, tab);
        XC_HIP(ctx, hipGetLastError());
        mark(0);
    }
    for (; done < nrange; ++done) poff[(size_t)done + 1] = poff[(size_t)done] + (long long)hp[(size_t)done];
    ctx->cptree_rounds = rounds_total; ctx->cptree_groups = (int)groups.size();
    const long long np = poff[(size_t)nrange];
    int herr = 0;
    XC_HIP(ctx, hipMemcpyAsync(&herr, d_err, 4, hipMemcpyDeviceToHost, ctx->stream));
    XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (herr & CP_ERR_EDGE) { settle(); return fail(ctx, XC_EBADARG, std::string(who) + ": an edge id outside [0, 2 ny nx)"); }
    if (herr & CP_ERR_LINK) { settle(); return fail(ctx, XC_EBADARG, std::string(who) + ": the records are not those of one xc_contour_segments call (a repeated edge id)"); }
    if (herr) { settle(); return fail(ctx, XC_EBADARG, std::string(who) + ": the records are not those of one xc_contour_segments call (rings that enclose each other)"); }
    if (np > capacity) { settle(); return 1; }
    XC_HIP(ctx, hipMemcpyAsync(d_poff, poff.data(), (size_t)(nrange + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_pi_finish, dim3(cp_blocks(np)), blk, 0, ctx->stream, (int64_t)np, nrange, ncont, d_poff, st, mx, (long long*)first_edge,
                       (long long*)nseg, (int*)closed, (int*)winding, (long long*)n_in, sum_w, sum_wf);
    XC_HIP(ctx, hipGetLastError());
    mark(3);
    hipLaunchKernelGGL(k_pt_finish, dim3(cp_blocks(np)), blk, 0, ctx->stream, (int64_t)np, nrange, ncont, d_poff, st, pt, mx, (long long*)parent,
                       (int*)depth, (int*)nchild, (long long*)n_net, net_w, net_wf);
    XC_HIP(ctx, hipGetLastError());
    mark(4);
    XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    settle();
    return XC_OK;
}

}  // namespace xc

// ------------------------------------------------------------------------------------ C ABI
int xc_contour_piece_tree_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to,
                              const double* pts, int64_t ny, int64_t nx, int periodic, int flip, int ncont, const double* w,
                              int w_per_slab, const void* f, int f_dtype, int64_t capacity, uint64_t* piece_count, int64_t* first_edge,
                              int64_t* nseg, int32_t* closed, int32_t* winding, int64_t* n_in, double* sum_w, double* sum_wf,
                              int64_t* parent, int32_t* depth, int32_t* nchild, int64_t* n_net, double* net_w, double* net_wf)
{
    XC_CTX(ctx);
    return xc::launch_contour_piece_tree(ctx, nrange, count, e_from, e_to, pts, ny, nx, periodic, flip, ncont, w, w_per_slab, f, f_dtype,
                                         capacity, piece_count, first_edge, nseg, closed, winding, n_in, sum_w, sum_wf, parent, depth,
                                         nchild, n_net, net_w, net_wf);
}

int xc_last_cptree_profile(xc_ctx* ctx, double* ms, int* rounds, int* groups)
{
    if (!ctx) return xc::fail(nullptr, XC_EBADARG, "null context");
    if (ms) for (int k = 0; k < 5; ++k) ms[k] = (double)ctx->cptree_ms[k];
    if (rounds) *rounds = ctx->cptree_rounds;
    if (groups) *groups = ctx->cptree_groups;
    return XC_OK;
}

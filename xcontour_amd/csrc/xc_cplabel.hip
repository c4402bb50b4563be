// K20 -- which ring HOLDS each node (gfx950): per range a dense int32 map [ny][nx] naming the innermost ring round every node, -1 for none,
// beside K19's records, from K12's segment records on the device.
//
// The rule (include/xcontour_hip.h, K20 section): with I_p K18's inside set of ring p, label[r][c] is the ring with (r, c) in I_p and the
// fewest inside nodes; open pieces are transparent.
//
// The mapping rests on K19's facts (xc_cptree.hip) and one more.  Without flip row 0 lies outside every ring, with flip row ny - 1 does:
// a column is scanned from that row, down without flip and up with it, and the scan starts in state -1 (no ring).
//   CROSSING   of a ring x (not open) at V(e, c): x's inside lies below it iff (s == S_x) != (winding_x != 0 && flip) (K18's s and S).
//              Inside on the far side of the walker: it enters x and the state becomes x.  Inside on the near side: it leaves x and
//              the state becomes par[x] (K19's parent) -- a vertical edge carries at most one vertex of a level, so the node across
//              that edge lies in every ring round x and in no sibling of x: in par[x] and no deeper.  One register, no stack.
//   ROW CHUNKS a node's label is the state behind the nearest crossing of a ring behind it in its column, wherever the scan began.  So a
//              column is cut into chunks of rows (pl_geometry: at least PL_ROWS rows each, at most PL_CHUNKS chunks; ny alone decides).
//              With more than one chunk k_pl_carry first leaves, per (range, chunk, column), the state behind the chunk's last crossing
//              of a ring, or PL_NONE; a chunk then starts from the nearest carry behind it that is not PL_NONE, else from -1.
//
// Per group, after K19's stages and before k_cp_unscatter (the edge table, root[], slot[], the signs and par[] still stand):
//   k_pl_carry   one thread per (range of the group, chunk but the last, column): the carry of the chunk
//   k_pl_scan    one thread per (range of the group, chunk, column): at most PL_CHUNKS carries looked back at, then the chunk's rows: the
//                label of a node is stored, then the edge behind it is crossed
// Lanes of a wave take consecutive columns: the table reads tab[V(e, c)] sit 8 bytes apart and the label stores are contiguous.  root[],
// slot[], e_from, e_to and the staged records are read at crossings only.  Ranges of the call that no group holds (no segments) are set
// to -1 with a memset.  Every index taken from a record or a table is checked before it addresses anything; every loop ends within ny
// steps; no kernel waits for another block; no LDS, no scratch.
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
#include "xc_cpiece_tree.h"
#include "xc_cpiece_label.h"                                                // the chunks, pl_cross and k_pl_carry (K21 runs them too)

__global__ __launch_bounds__(CP_TPB)
void k_pl_scan(int64_t ng, int64_t rows, int64_t nchunk, PlGroup g, PiStage st, PtStage pt, const int* __restrict__ carry,
               int* __restrict__ label, int* __restrict__ err)
{
    int64_t rl, k, c;
    if (!pl_thread(ng, nchunk, g.nx, rl, k, c)) return;
    const int64_t r = g.r0 + rl;
    const long long lo = g.poff[r], hi = g.poff[r + 1];
    const int* tp = g.tab + (size_t)rl * (size_t)g.E + 2 * (size_t)c + 1;
    int state = -1;
    for (int64_t kk = k - 1; kk >= 0; --kk) {                                // at most PL_CHUNKS - 1 steps
        const int v = carry[(size_t)(rl * nchunk + kk) * (size_t)g.nx + (size_t)c];
        if (v != PL_NONE) { state = v; break; }
    }
    int* out = label + (size_t)r * (size_t)g.ny * (size_t)g.nx + (size_t)c;
    const int64_t t1 = (k + 1) * rows < g.ny ? (k + 1) * rows : g.ny;
    for (int64_t t = k * rows; t < t1; ++t) {
        const int64_t at = g.flip ? g.ny - 1 - t : t;                        // 0 <= at < ny
        out[(size_t)at * (size_t)g.nx] = state;
        if (t == g.ny - 1) break;
        const int64_t e = g.flip ? at - 1 : at;                              // the edge to the next node: 0 <= e < ny - 1
        const int v = pl_cross(tp[2 * (size_t)g.nx * (size_t)e], r, lo, hi, g, st, pt, err);
        if (v != PL_NONE) state = v;
    }
}

}  // namespace

// One xc_contour_piece_labels_dev call: K19's (xc_cptree.hip) with the label scan per group.  Waits for the stream as K18 does.
int launch_contour_piece_labels(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to,
                                const double* pts, int64_t ny, int64_t nx, int periodic, int flip, int ncont, const double* w,
                                int w_per_slab, const void* f, int f_dtype, int64_t capacity, uint64_t* piece_count, int64_t* first_edge,
                                int64_t* nseg, int32_t* closed, int32_t* winding, int64_t* n_in, double* sum_w, double* sum_wf,
                                int64_t* parent, int32_t* depth, int32_t* nchild, int64_t* n_net, double* net_w, double* net_wf,
                                int32_t* label)
{
    const char* who = "xc_contour_piece_labels";
    if (!count || !piece_count || nrange < 1 || ny < 1 || nx < 1 || capacity < 0) return fail(ctx, XC_EBADARG, std::string(who) + ": bad arguments");
    if (flip != 0 && flip != 1) return fail(ctx, XC_EBADARG, std::string(who) + ": flip is 0 or 1");
    if (ncont < 1 || nrange % ncont != 0) return fail(ctx, XC_EBADARG, std::string(who) + ": nrange must be a multiple of ncont >= 1");
    if (f && f_dtype != XC_F32 && f_dtype != XC_F64) return fail(ctx, XC_EBADARG, std::string(who) + ": f_dtype is XC_F32 or XC_F64");
    if (capacity > 0 && (!first_edge || !nseg || !closed || !winding || !n_in || !sum_w || !parent || !depth || !nchild || !n_net || !net_w))
        return fail(ctx, XC_EBADARG, std::string(who) + ": capacity > 0 needs the record arrays");
    if (capacity > 0 && !label) return fail(ctx, XC_EBADARG, std::string(who) + ": capacity > 0 needs the label map");
    if (capacity > 0 && ((f == nullptr) != (sum_wf == nullptr) || (f == nullptr) != (net_wf == nullptr)))
        return fail(ctx, XC_EBADARG, std::string(who) + ": f, sum_wf and net_wf go together");
    if (periodic && nx < 3) return fail(ctx, XC_EBADARG, std::string(who) + ": a periodic plane needs nx >= 3 (with two columns a cell's two vertical edges are one)");
    if (ny > (((int64_t)1 << 30) - 1) / nx) return fail(ctx, XC_EBADARG, std::string(who) + ": plane too large for 32-bit labels (2 ny nx < 2^31)");
    const long long E = 2 * ny * nx;
    const int wrap = periodic ? 1 : 0;
    const int64_t nslab = nrange / ncont;
    if (nslab > 65535) return fail(ctx, XC_EBADARG, std::string(who) + ": more than 65535 slabs");
    for (int k = 0; k < 6; ++k) ctx->cplabel_ms[k] = 0.f;
    ctx->cplabel_rounds = 0; ctx->cplabel_groups = 0;

    const int64_t npl = ny * nx;
    // the ranges [ra, rb) of the map hold no ring: -1 everywhere
    auto blank = [&](int64_t ra, int64_t rb) -> hipError_t {
        if (!label || rb <= ra) return hipSuccess;
        return hipMemsetAsync(label + (size_t)ra * (size_t)npl, 0xff, (size_t)(rb - ra) * (size_t)npl * 4, ctx->stream);
    };

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
    if (total == 0) {
        XC_HIP(ctx, blank(0, nrange));
        XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return XC_OK;
    }
    if (!e_from || !e_to || !pts) return fail(ctx, XC_EBADARG, std::string(who) + ": segments without their records");
    const int64_t cap = std::min<int64_t>(capacity, total);               // a piece has a segment: no more pieces than segments

    int64_t gmax = 1; long long nmax = 0;
    const std::vector<CpGroup> groups = cp_plan_groups(ctx->cpiece_cap, E, nrange, hc, off, &gmax, &nmax);
    int64_t rows = 0, nchunk = 0;
    pl_geometry(ny, &rows, &nchunk);
    // workspace (K18's, then the carries): off | poff | mx[nslab][2], err (cleared together) | tab[gmax][E] | rid[nmax] | label, next, prev
    // x 2 [nmax] | carry[gmax][nchunk][nx]
    const size_t b_off = al((size_t)(nrange + 1) * 8), b_mx = al((size_t)nslab * 16), b_small = 256;
    const size_t b_tab = al((size_t)gmax * (size_t)E * 4), b_n = al((size_t)nmax * 4);
    const size_t b_carry = nchunk > 1 ? al((size_t)gmax * (size_t)nchunk * (size_t)nx * 4) : 0;
    XC_TRY(grow(ctx, &ctx->cpiece_ws, &ctx->cpiece_ws_bytes, 2 * b_off + b_mx + b_small + b_tab + 7 * b_n + b_carry));
    char* ws = (char*)ctx->cpiece_ws;
    long long* d_off = (long long*)ws;
    long long* d_poff = (long long*)(ws + b_off);
    unsigned long long* mx = (unsigned long long*)(ws + 2 * b_off);
    int* d_err = (int*)((char*)mx + b_mx);
    int* tab = (int*)((char*)d_err + b_small);
    int* rid = (int*)((char*)tab + b_tab);
    int* buf[6];
    for (int k = 0; k < 6; ++k) buf[k] = (int*)((char*)rid + (size_t)(k + 1) * b_n);
    int* carry = (int*)((char*)rid + 7 * b_n);
    // the staged records, K18's and then the tree's: nothing reaches the caller's record arrays before all pieces are known to fit
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
            if (marks[k].second >= 0 && hipEventElapsedTime(&ms, marks[k - 1].first, marks[k].first) == hipSuccess) ctx->cplabel_ms[marks[k].second] += ms;
        }
        for (auto& m : marks) (void)hipEventDestroy(m.first);
        marks.clear();
    };

    const dim3 blk(CP_TPB);
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
    int64_t mapped = 0;                                                     // the map of ranges [0, mapped) is written
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
            // the map of the group's ranges, and -1 for the ranges without segments in front of it
            XC_HIP(ctx, blank(mapped, g.r0));
            const PlGroup pg = {n, s0, g.r0, E, ny, nx, flip, cap, (const long long*)e_from, (const long long*)e_to, tab, root, slot, pcnt, d_poff};
            const dim3 lgrid(cp_blocks(ng * nchunk * nx));                 // no more threads than the group's table has nodes
            if (nchunk > 1) hipLaunchKernelGGL(k_pl_carry, lgrid, blk, 0, ctx->stream, ng, rows, nchunk, pg, st, pt, carry, d_err);
            hipLaunchKernelGGL(k_pl_scan, lgrid, blk, 0, ctx->stream, ng, rows, nchunk, pg, st, pt, (const int*)carry, (int*)label, d_err);
            XC_HIP(ctx, hipGetLastError());
            mapped = g.r1;
            mark(5);
        } else {
            mark(2);
        }
        hipLaunchKernelGGL(k_cp_unscatter, grid, blk, 0, ctx->stream, n, s0, E, (const long long*)e_from, rid, tab);
        XC_HIP(ctx, hipGetLastError());
        mark(0);
    }
    for (; done < nrange; ++done) poff[(size_t)done + 1] = poff[(size_t)done] + (long long)hp[(size_t)done];
    ctx->cplabel_rounds = rounds_total; ctx->cplabel_groups = (int)groups.size();
    const long long np = poff[(size_t)nrange];
    int herr = 0;
    XC_HIP(ctx, hipMemcpyAsync(&herr, d_err, 4, hipMemcpyDeviceToHost, ctx->stream));
    XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (herr & CP_ERR_EDGE) { settle(); return fail(ctx, XC_EBADARG, std::string(who) + ": an edge id outside [0, 2 ny nx)"); }
    if (herr & CP_ERR_LINK) { settle(); return fail(ctx, XC_EBADARG, std::string(who) + ": the records are not those of one xc_contour_segments call (a repeated edge id)"); }
    if (herr) { settle(); return fail(ctx, XC_EBADARG, std::string(who) + ": the records are not those of one xc_contour_segments call (rings that enclose each other)"); }
    if (np > capacity) { settle(); return 1; }
    if (!over) XC_HIP(ctx, blank(mapped, nrange));                          // the ranges without segments behind the last group
    mark(5);
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
int xc_contour_piece_labels_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to,
                                const double* pts, int64_t ny, int64_t nx, int periodic, int flip, int ncont, const double* w,
                                int w_per_slab, const void* f, int f_dtype, int64_t capacity, uint64_t* piece_count, int64_t* first_edge,
                                int64_t* nseg, int32_t* closed, int32_t* winding, int64_t* n_in, double* sum_w, double* sum_wf,
                                int64_t* parent, int32_t* depth, int32_t* nchild, int64_t* n_net, double* net_w, double* net_wf,
                                int32_t* label)
{
    XC_CTX(ctx);
    return xc::launch_contour_piece_labels(ctx, nrange, count, e_from, e_to, pts, ny, nx, periodic, flip, ncont, w, w_per_slab, f, f_dtype,
                                           capacity, piece_count, first_edge, nseg, closed, winding, n_in, sum_w, sum_wf, parent, depth,
                                           nchild, n_net, net_w, net_wf, label);
}

int xc_last_cplabel_profile(xc_ctx* ctx, double* ms, int* rounds, int* groups)
{
    if (!ctx) return xc::fail(nullptr, XC_EBADARG, "null context");
    if (ms) for (int k = 0; k < 6; ++k) ms[k] = (double)ctx->cplabel_ms[k];
    if (rounds) *rounds = ctx->cplabel_rounds;
    if (groups) *groups = ctx->cplabel_groups;
    return XC_OK;
}

// K18-K21 -- the ring records (gfx950): one launcher behind xc_contour_piece_interiors_dev (K18: what every piece bounds),
// xc_contour_piece_tree_dev (K19: which piece is nested in which), xc_contour_piece_labels_dev (K20: which ring holds each node) and
// xc_contour_piece_props_dev (K21: what every ring holds of further fields).  Each builds on the one before it: K19 is K18 with the tree
// stages per group, K20 and K21 are K19 with a column scan per group.  The rules, the mappings and the kernels are in the headers that
// own them: xc_cpiece_interior.h (K18), xc_cpiece_tree.h (K19), xc_cpiece_label.h (K20), xc_cpiece_props.h (K21); phase A is K13's
// (xc_cpiece_link.h, xc_cpiece_slot.h).
//
// One call, per GROUP of consecutive ranges (K13's groups under K13's cap, indices group-local):
//   phase A, k_cp_root; the host reads the group's piece counts (they place the group's pieces in the table; once the pieces no longer
//   fit `capacity` the rest of the call only counts); K18's stages; with `tree` K19's; with `label` or `props` the carries and the scan;
//   k_cp_unscatter hands the table on clean.
// Around the groups: k_ci_bound (and k_pp_bound) in front, the finish passes behind -- only when all pieces fit: nothing reaches the
// caller's record arrays before that is known.  A call waits for the stream once for K12's counts, once per group for its piece counts,
// once for the error word and once at the end.
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
#include "xc_cpiece_label.h"
#include "xc_cpiece_props.h"

// One call of one of the four entries: the caller's pointers and scalars in the order of the C ABI.  The parts that are set decide which
// stages run: K18 none, K19 `tree`, K20 `tree` and `label`, K21 `tree` and `props`.
struct PieceCall {
    const char* who;                                                       // the entry, for the error texts
    CpProfile* prof;                                                       // the entry's own profile record of the context
    int64_t nrange; const uint64_t* count; const int64_t *e_from, *e_to; const double* pts; int64_t ny, nx; int periodic, flip, ncont;
    const double* w; int w_per_slab; const void* f; int f_dtype; int64_t capacity; uint64_t* piece_count;
    int64_t *first_edge, *nseg; int32_t *closed, *winding; int64_t* n_in; double *sum_w, *sum_wf;
    bool tree; int64_t* parent; int32_t *depth, *nchild; int64_t* n_net; double *net_w, *net_wf;
    bool label; int32_t* map;
    bool props; int nf; const void* const* g; const int *g_dtype, *g_per_slab; const void* x; int x_dtype;
    double *net_g, *sum_g, *x_min, *x_max; int64_t *at_min, *at_max;
};

// The workspace of a call (ctx->cpiece_ws): off | poff | mx[nslab][2], err (cleared together: b_zero bytes) | the tail (xc_cpiece_link.h)
// | K20, K21: carry[gmax][nchunk][nx] | K21: mxg[nslab][nf] (b_mxg bytes) | fld[XC_PROPS_MAXF + 1]
struct PieceWs {
    long long *off, *poff; unsigned long long* mx; int* err; CpTail t; int* carry; unsigned long long* mxg; PpField* fld;
    size_t b_zero, b_mxg;
};
size_t piece_ws_carve(Carve c, const PieceCall& pc, int64_t nslab, const CpPlan& pl, int64_t nchunk, PieceWs& ws)
{
    ws.off = c.take<long long>((size_t)pc.nrange + 1); ws.poff = c.take<long long>((size_t)pc.nrange + 1);
    ws.b_zero = c.mark();
    ws.mx = c.take<unsigned long long>((size_t)nslab * 2); ws.err = c.take<int>(CP_SMALL);
    ws.b_zero = c.mark() - ws.b_zero;
    cp_carve_tail(c, pl, 6, ws.t);
    ws.carry = c.take<int>(nchunk > 1 ? (size_t)pl.gmax * (size_t)nchunk * (size_t)pc.nx : 0);
    ws.b_mxg = c.mark();
    ws.mxg = c.take<unsigned long long>(pc.props ? (size_t)nslab * (size_t)std::max(pc.nf, 1) : 0);
    ws.b_mxg = c.mark() - ws.b_mxg;
    ws.fld = c.take<PpField>(pc.props ? XC_PROPS_MAXF + 1 : 0);
    return c.at;
}

int launch_piece_records(xc_ctx* ctx, const PieceCall& c)
{
    auto refuse = [&](const char* what) { return fail(ctx, XC_EBADARG, std::string(c.who) + what); };
    if (!c.count || !c.piece_count || c.nrange < 1 || c.ny < 1 || c.nx < 1 || c.capacity < 0) return refuse(": bad arguments");
    if (c.flip != 0 && c.flip != 1) return refuse(": flip is 0 or 1");
    if (c.ncont < 1 || c.nrange % c.ncont != 0) return refuse(": nrange must be a multiple of ncont >= 1");
    if (c.f && c.f_dtype != XC_F32 && c.f_dtype != XC_F64) return refuse(": f_dtype is XC_F32 or XC_F64");
    if (c.props) {
        if (c.nf < 0 || c.nf > XC_PROPS_MAXF) return refuse(": nf lies in [0, XC_PROPS_MAXF]");
        if (c.nf > 0 && (!c.g || !c.g_dtype || !c.g_per_slab)) return refuse(": nf > 0 needs g, g_dtype and g_per_slab");
        for (int m = 0; m < c.nf; ++m) {
            if (!c.g[m]) return refuse(": a field plane is NULL");
            if (c.g_dtype[m] != XC_F32 && c.g_dtype[m] != XC_F64) return refuse(": g_dtype is XC_F32 or XC_F64");
        }
        if (c.x && c.x_dtype != XC_F32 && c.x_dtype != XC_F64) return refuse(": x_dtype is XC_F32 or XC_F64");
    }
    if (c.capacity > 0 && (!c.first_edge || !c.nseg || !c.closed || !c.winding || !c.n_in || !c.sum_w ||
                           (c.tree && (!c.parent || !c.depth || !c.nchild || !c.n_net || !c.net_w))))
        return refuse(": capacity > 0 needs the record arrays");
    if (c.label && c.capacity > 0 && !c.map) return refuse(": capacity > 0 needs the label map");
    if (!c.tree && c.capacity > 0 && (c.f == nullptr) != (c.sum_wf == nullptr)) return refuse(": f and sum_wf go together");
    if (c.tree && c.capacity > 0 && ((c.f == nullptr) != (c.sum_wf == nullptr) || (c.f == nullptr) != (c.net_wf == nullptr)))
        return refuse(": f, sum_wf and net_wf go together");
    if (c.props && c.capacity > 0 && ((c.nf == 0) != (c.net_g == nullptr) || (c.nf == 0) != (c.sum_g == nullptr)))
        return refuse(": net_g and sum_g are NULL exactly when nf is 0");
    if (c.props && c.capacity > 0 && ((c.x == nullptr) != (c.x_min == nullptr) || (c.x == nullptr) != (c.x_max == nullptr) ||
                                      (c.x == nullptr) != (c.at_min == nullptr) || (c.x == nullptr) != (c.at_max == nullptr)))
        return refuse(": x, x_min, x_max, at_min and at_max go together");
    if (c.periodic && c.nx < 3) return refuse(": a periodic plane needs nx >= 3 (with two columns a cell's two vertical edges are one)");
    if (c.ny > (((int64_t)1 << 30) - 1) / c.nx) return refuse(": plane too large for 32-bit labels (2 ny nx < 2^31)");
    const int64_t ny = c.ny, nx = c.nx, nrange = c.nrange, npl = ny * nx, nslab = nrange / c.ncont;
    const long long E = 2 * ny * nx;
    const int wrap = c.periodic ? 1 : 0, nf = c.nf, hasx = c.x ? 1 : 0;
    if (nslab > 65535) return refuse(": more than 65535 slabs");
    profile_clear(*c.prof);
    hipStream_t stream = ctx->stream;

    CpPlan pl;
    XC_TRY(cp_plan(ctx, c.who, nrange, c.count, c.piece_count, c.e_from, c.e_to, c.pts, E, pl));
    const long long total = pl.total;
    if (total == 0) {
        if (c.label) {                                                       // no ring anywhere: -1 everywhere
            XC_HIP(ctx, pl_blank(stream, c.map, npl, 0, nrange));
            XC_HIP(ctx, hipStreamSynchronize(stream));
        }
        return XC_OK;
    }
    const int64_t cap = std::min<int64_t>(c.capacity, total);             // a piece has a segment: no more pieces than segments

    int64_t rows = 0, nchunk = 0;                                           // the row chunks of the scans (K20, K21)
    if (c.label || c.props) pl_geometry(ny, &rows, &nchunk);
    PieceWs ws;
    XC_TRY(lay_out(ctx, &ctx->cpiece_ws, &ctx->cpiece_ws_bytes, [&](Carve a) { return piece_ws_carve(a, c, nslab, pl, nchunk, ws); }));
    // the staged records, K18's, then the tree's, then K21's: nothing reaches the caller's record arrays before all pieces are known to fit
    PiStage st = {};
    PtStage pt = {};
    PpStage pp = {};
    if (cap > 0) {
        auto lay = [&](Carve a) {
            pi_carve(a, cap, st);
            if (c.tree) pt_carve(a, cap, pt);
            if (c.props) pp_carve(a, cap, nf, pp);
            return a.at;
        };
        XC_TRY(lay_out(ctx, &ctx->cpiece_acc, &ctx->cpiece_acc_bytes, lay));
    }
    // K21: the call's fields as the kernels read them; entry nf is the extremum field
    PpField hfld[XC_PROPS_MAXF + 1] = {};
    for (int m = 0; m < nf; ++m) hfld[m] = {c.g[m], c.g_per_slab[m] ? (unsigned long long)npl : 0ull, c.g_dtype[m] == XC_F32 ? 1 : 0, 0};
    if (c.x) hfld[nf] = {c.x, (unsigned long long)npl, c.x_dtype == XC_F32 ? 1 : 0, 0};
    const bool pscan = c.props && (nf > 0 || hasx);                        // K21 without fields and without x is K19

    // the stages of the profiles: 0 table, 1 rounds, 2 roots, 3 walk, 4 tree, 5 label or props scan, 6 fold and finish
    StageTimer tm(ctx, c.prof->ms);
    CpRun run(ctx, tm, pl, c.e_from, c.e_to, ws.off, ws.t, ws.err);
    const dim3 blk(CP_TPB);
    tm.mark(-1);
    XC_HIP(ctx, hipMemsetAsync(ws.mx, 0, ws.b_zero, stream));
    if (cap > 0) {
        ci_launch_bound(stream, npl, nslab, c.w, c.w_per_slab, c.f, c.f_dtype, ws.mx);
        XC_HIP(ctx, hipGetLastError());
    }
    tm.mark(3);
    if (c.props) {
        if (cap > 0) {
            XC_HIP(ctx, hipMemsetAsync(ws.mxg, 0, ws.b_mxg, stream));
            XC_HIP(ctx, hipMemcpyAsync(ws.fld, hfld, sizeof(hfld), hipMemcpyHostToDevice, stream));
            if (nf > 0) {
                pp_launch_bound(stream, npl, nslab, nf, c.w, c.w_per_slab, ws.fld, ws.mxg);
                XC_HIP(ctx, hipGetLastError());
            }
        }
        tm.mark(5);
    }
    XC_TRY(run.upload_off());
    XC_TRY(run.fill_table());
    tm.mark(0);

    std::vector<uint64_t> hp((size_t)nrange, 0);
    std::vector<long long> poff((size_t)nrange + 1, 0);
    int64_t done = 0;                                                       // poff[0 .. done] stand
    int64_t mapped = 0;                                                     // K20: the map of ranges [0, mapped) is written
    bool over = cap == 0;                                                   // the pieces no longer fit: count only
    int* const tab = ws.t.tab; int* const rid = ws.t.rid;
    for (const CpGroup& g : pl.groups) {
        run.begin(g);
        XC_TRY(run.rounds());
        const long long s0 = run.s0;
        const int64_t n = run.n, ng = g.r1 - g.r0;
        int *root = run.b.nxt2, *slot = run.b.lab2;
        hipLaunchKernelGGL(k_cp_root, run.grid, blk, 0, stream, n, E, tab, rid, run.b.lab, run.b.prv, g.r0, (unsigned long long*)c.piece_count, root, slot);
        XC_HIP(ctx, hipGetLastError());
        // the group's piece counts place its pieces in the table
        XC_HIP(ctx, hipMemcpyAsync(hp.data() + g.r0, c.piece_count + g.r0, (size_t)ng * 8, hipMemcpyDeviceToHost, stream));
        XC_HIP(ctx, hipStreamSynchronize(stream));
        for (; done < g.r1; ++done) poff[(size_t)done + 1] = poff[(size_t)done] + (long long)hp[(size_t)done];
        const int64_t p0 = poff[(size_t)g.r0], p1 = poff[(size_t)g.r1];
        if (p1 > cap) over = true;
        if (!over && p1 > p0) {
            const PlGroup pg = {n, s0, g.r0, E, ny, nx, c.flip, cap, (const long long*)c.e_from, (const long long*)c.e_to, tab, root, slot,
                                (const unsigned long long*)c.piece_count, ws.poff};
            XC_HIP(ctx, hipMemcpyAsync(ws.poff + g.r0, poff.data() + g.r0, (size_t)(ng + 1) * 8, hipMemcpyHostToDevice, stream));
            pi_launch_piece(stream, pg, p0, p1, wrap, c.pts, rid, st, ws.err);
            XC_HIP(ctx, hipGetLastError());
            tm.mark(2);
            pi_launch_walk(stream, pg, c.ncont, rid, c.w, c.w_per_slab, c.f, c.f_dtype, ws.mx, st, ws.err);
            XC_HIP(ctx, hipGetLastError());
            tm.mark(3);
            if (c.tree) {
                pt_launch_group(stream, pg, g.r1, p0, p1, rid, st, pt, ws.err);
                XC_HIP(ctx, hipGetLastError());
                tm.mark(4);
            }
            if (c.label || pscan) {
                // K20: the map of the group's ranges, and -1 for the ranges without segments in front of it; K21: the staged words cleared
                if (c.label) XC_HIP(ctx, pl_blank(stream, c.map, npl, mapped, g.r0));
                if (pscan) hipLaunchKernelGGL(k_pp_init, dim3(cp_blocks(p1 - p0)), blk, 0, stream, p0, p1, nf, pp);
                pl_launch_carry(stream, ng, rows, nchunk, pg, st, pt, ws.carry, ws.err);
                if (c.label) pl_launch_scan(stream, ng, rows, nchunk, pg, st, pt, ws.carry, c.map, ws.err);
                else pp_launch_scan(stream, ng, rows, nchunk, c.ncont, pg, st, pt, ws.carry, c.w, c.w_per_slab, ws.fld, nf, hasx, ws.mxg, pp, ws.err);
                XC_HIP(ctx, hipGetLastError());
                mapped = g.r1;
                tm.mark(5);
            }
            if (pscan) {
                if (nf > 0) {
                    hipLaunchKernelGGL(k_pp_fold, dim3(cp_blocks(p1 - p0)), blk, 0, stream, p0, p1, g.r0, g.r1, ws.poff, nf, st, pt, pp, ws.err);
                    XC_HIP(ctx, hipGetLastError());
                }
                tm.mark(6);
            }
        } else {
            tm.mark(2);
        }
        XC_TRY(run.end());
    }
    for (; done < nrange; ++done) poff[(size_t)done + 1] = poff[(size_t)done] + (long long)hp[(size_t)done];
    run.report(*c.prof);
    const long long np = poff[(size_t)nrange];
    int herr = 0;
    XC_TRY(cp_read_err(ctx, ws.err, &herr));
    // (a K18 call sets the first two bits only)
    if (herr & CP_ERR_EDGE) return refuse(": an edge id outside [0, 2 ny nx)");
    if (herr & CP_ERR_LINK) return refuse(": the records are not those of one xc_contour_segments call (a repeated edge id)");
    if (herr) return refuse(": the records are not those of one xc_contour_segments call (rings that enclose each other)");
    if (np > c.capacity) return 1;
    if (c.label) {
        if (!over) XC_HIP(ctx, pl_blank(stream, c.map, npl, mapped, nrange));   // the ranges without segments behind the last group
        tm.mark(5);
    }
    XC_HIP(ctx, hipMemcpyAsync(ws.poff, poff.data(), (size_t)(nrange + 1) * 8, hipMemcpyHostToDevice, stream));
    hipLaunchKernelGGL(k_pi_finish, dim3(cp_blocks(np)), blk, 0, stream, (int64_t)np, nrange, c.ncont, ws.poff, st, ws.mx, (long long*)c.first_edge,
                       (long long*)c.nseg, (int*)c.closed, (int*)c.winding, (long long*)c.n_in, c.sum_w, c.sum_wf);
    XC_HIP(ctx, hipGetLastError());
    tm.mark(3);
    if (c.tree) {
        hipLaunchKernelGGL(k_pt_finish, dim3(cp_blocks(np)), blk, 0, stream, (int64_t)np, nrange, c.ncont, ws.poff, st, pt, ws.mx,
                           (long long*)c.parent, (int*)c.depth, (int*)c.nchild, (long long*)c.n_net, c.net_w, c.net_wf);
        XC_HIP(ctx, hipGetLastError());
        tm.mark(4);
    }
    if (c.props) {
        if (pscan) {
            hipLaunchKernelGGL(k_pp_finish, dim3(cp_blocks(np * (nf + hasx))), blk, 0, stream, (int64_t)np, nrange, c.ncont, nf, hasx, c.capacity,
                               ws.poff, st, pp, ws.mxg, c.net_g, c.sum_g, c.x_min, c.x_max, (long long*)c.at_min, (long long*)c.at_max);
            XC_HIP(ctx, hipGetLastError());
        }
        tm.mark(6);
    }
    XC_HIP(ctx, hipStreamSynchronize(stream));
    return XC_OK;
}

}  // namespace
}  // namespace xc

// ------------------------------------------------------------------------------------ C ABI
int xc_contour_piece_interiors_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to,
                                   const double* pts, int64_t ny, int64_t nx, int periodic, int flip, int ncont, const double* w,
                                   int w_per_slab, const void* f, int f_dtype, int64_t capacity, uint64_t* piece_count, int64_t* first_edge,
                                   int64_t* nseg, int32_t* closed, int32_t* winding, int64_t* n_in, double* sum_w, double* sum_wf)
{
    XC_CTX(ctx);
    const xc::PieceCall c = {"xc_contour_piece_interiors", &ctx->prof_cpinside, nrange, count,
                             e_from, e_to, pts, ny, nx, periodic, flip, ncont, w, w_per_slab, f, f_dtype, capacity, piece_count, first_edge,
                             nseg, closed, winding, n_in, sum_w, sum_wf};
    return xc::launch_piece_records(ctx, c);
}

int xc_contour_piece_tree_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to,
                              const double* pts, int64_t ny, int64_t nx, int periodic, int flip, int ncont, const double* w,
                              int w_per_slab, const void* f, int f_dtype, int64_t capacity, uint64_t* piece_count, int64_t* first_edge,
                              int64_t* nseg, int32_t* closed, int32_t* winding, int64_t* n_in, double* sum_w, double* sum_wf,
                              int64_t* parent, int32_t* depth, int32_t* nchild, int64_t* n_net, double* net_w, double* net_wf)
{
    XC_CTX(ctx);
    const xc::PieceCall c = {"xc_contour_piece_tree", &ctx->prof_cptree, nrange, count, e_from, e_to,
                             pts, ny, nx, periodic, flip, ncont, w, w_per_slab, f, f_dtype, capacity, piece_count, first_edge, nseg, closed,
                             winding, n_in, sum_w, sum_wf, true, parent, depth, nchild, n_net, net_w, net_wf};
    return xc::launch_piece_records(ctx, c);
}

int xc_contour_piece_labels_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to,
                                const double* pts, int64_t ny, int64_t nx, int periodic, int flip, int ncont, const double* w,
                                int w_per_slab, const void* f, int f_dtype, int64_t capacity, uint64_t* piece_count, int64_t* first_edge,
                                int64_t* nseg, int32_t* closed, int32_t* winding, int64_t* n_in, double* sum_w, double* sum_wf,
                                int64_t* parent, int32_t* depth, int32_t* nchild, int64_t* n_net, double* net_w, double* net_wf,
                                int32_t* label)
{
    XC_CTX(ctx);
    const xc::PieceCall c = {"xc_contour_piece_labels", &ctx->prof_cplabel, nrange, count, e_from,
                             e_to, pts, ny, nx, periodic, flip, ncont, w, w_per_slab, f, f_dtype, capacity, piece_count, first_edge, nseg,
                             closed, winding, n_in, sum_w, sum_wf, true, parent, depth, nchild, n_net, net_w, net_wf, true, label};
    return xc::launch_piece_records(ctx, c);
}

int xc_contour_piece_props_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to,
                               const double* pts, int64_t ny, int64_t nx, int periodic, int flip, int ncont, const double* w,
                               int w_per_slab, const void* f, int f_dtype, int64_t capacity, uint64_t* piece_count, int64_t* first_edge,
                               int64_t* nseg, int32_t* closed, int32_t* winding, int64_t* n_in, double* sum_w, double* sum_wf,
                               int64_t* parent, int32_t* depth, int32_t* nchild, int64_t* n_net, double* net_w, double* net_wf,
                               int nf, const void* const* g, const int* g_dtype, const int* g_per_slab, const void* x, int x_dtype,
                               double* net_g, double* sum_g, double* x_min, double* x_max, int64_t* at_min, int64_t* at_max)
{
    XC_CTX(ctx);
    const xc::PieceCall c = {"xc_contour_piece_props", &ctx->prof_cpprops, nrange, count, e_from,
                             e_to, pts, ny, nx, periodic, flip, ncont, w, w_per_slab, f, f_dtype, capacity, piece_count, first_edge, nseg,
                             closed, winding, n_in, sum_w, sum_wf, true, parent, depth, nchild, n_net, net_w, net_wf, false, nullptr,
                             true, nf, g, g_dtype, g_per_slab, x, x_dtype, net_g, sum_g, x_min, x_max, at_min, at_max};
    return xc::launch_piece_records(ctx, c);
}

int xc_last_cpinside_profile(xc_ctx* ctx, double* ms, int* rounds, int* groups)
{
    return xc::profile_get(ctx, &xc_ctx::prof_cpinside, 4, ms, rounds, groups);
}

int xc_last_cptree_profile(xc_ctx* ctx, double* ms, int* rounds, int* groups)
{
    return xc::profile_get(ctx, &xc_ctx::prof_cptree, 5, ms, rounds, groups);
}

int xc_last_cplabel_profile(xc_ctx* ctx, double* ms, int* rounds, int* groups)
{
    return xc::profile_get(ctx, &xc_ctx::prof_cplabel, 6, ms, rounds, groups);
}

int xc_last_cpprops_profile(xc_ctx* ctx, double* ms, int* rounds, int* groups)
{
    return xc::profile_get(ctx, &xc_ctx::prof_cpprops, 7, ms, rounds, groups);
}

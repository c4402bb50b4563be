// K27 -- how far every node lies from a contour, and which part of it is nearest (gfx950): the distance from each node of the plane to
// the selected pieces of K12's segment records, on the device.
//
// K25 brought contour VECTORS back onto the plane; this brings the contour's geometry back: the cross-contour coordinate of every
// front-relative composite (distance from the vortex edge, from a jet axis, from an SSH front).  The reference's scripts get it by
// tracing a level and querying a KD-tree on the host (tests/test_breaking.py uses scipy.spatial).  Build-defined.
//
// Input: count[nrange], e_from, e_to, pts as xc_contour_segments[_periodic]_dev wrote them; pieces, rings, winding, `select` and the main
// ring's tie rule are K16's (xc_cpiece_select.h); ycoord, xcoord, period, radius with K13's meaning: a record end point (rho, gamma) maps
// to coordinates as K13 maps it (np.interp on the node floor(.), column nx of a periodic plane at xcoord[0] + period); node (r, c) is
// (ycoord[r], xcoord[c]).  xc_cdist_metric.h states the two metrics, operation by operation.
//   plane  (radius == 0): d2 of xc_cdist_metric.h; with `periodic` the minimum over px, px + period, px - period; dist = sqrt(min d2)
//   sphere (radius > 0, radians): c2 of xc_cdist_metric.h; dist = radius * 2 asin(min(1, sqrt(min c2) / 2)), one asin per node
//   edge   the e_from of the segment with the smallest d2 / c2, the smallest id among equal bit patterns;  piece  its piece's first_edge
//   dist = +inf, edge = piece = -1 where the range has no selected segment, or the distance exceeds max_dist (> 0 and finite);
//   negate_mask flips the sign of every finite dist where it is 1.
// min is order-free: no output depends on the order of the segments, of arrival, on the launch geometry or on the workspace cap.
//
// Per GROUP of consecutive ranges (xc_cpiece_link.h: K13's groups under K13's cap, indices group-local): phase A (K13's kernels), K16's
// selection (k_co_root, k_co_piece, k_co_pick), the segment table binned by coarse block (xc_cdist_table.h), k_cp_unscatter (the table is
// handed on clean), the tile pass k_cd_dist (xc_cdist_search.h).  K28 -- composites by distance (xc_contour_distance_profile_dev): the same
// launcher and phases with k_cd_profile as the tile pass (xc_cdist_profile.h); what else it adds to a call is CdK28's, below.
// This file: the call, the workspace, the launcher and the C ABI.
#include "xc_capi.h"
#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

namespace xc {
namespace {

#include "xc_binning.h"
#include "xc_clen_cell.h"

#include "xc_cpiece_link.h"
#include "xc_cpiece_select.h"
#include "xc_cpiece_sum.h"
#include "xc_cinside_bound.h"
#include "xc_cpiece_field.h"
#include "xc_cdist_metric.h"
#include "xc_cdist_table.h"
#include "xc_cdist_search.h"
#include "xc_cdist_profile.h"

// the period of a longitude ring in radians as the facade hands it over: float64(deg2rad(float32(360)))
const double CD_RING = (double)6.2831855f;

// K28's words of the workspace, in two runs (CdWs::lay); K27 leaves every size zero and they take no byte
struct CdpWs {
    size_t nslab = 0, n_mxg = 0, n_bin = 0, n_ch = 0, n_edge = 0, n_fld = 0;
    unsigned long long *mxw, *mxg, *acc, *cnt; int* bflag; double* edges; PpField* fld;
    PpField h_fld[XC_PROPS_MAXF] = {};                                      // the field table on the host, as uploaded
    void lay_cleared(Carve& a)
    {
        mxw = a.take<unsigned long long>(nslab * 2); mxg = a.take<unsigned long long>(n_mxg);
        acc = a.take<unsigned long long>(n_bin * n_ch * CP_L); cnt = a.take<unsigned long long>(n_bin); bflag = a.take<int>(n_bin * n_ch);
    }
    void lay_tables(Carve& a) { edges = a.take<double>(n_edge); fld = a.take<PpField>(n_fld); }
};

// ctx->cpiece_ws for one call: off | key, nsel, err, pairs and tiles; K28: mxw, mxg, acc, cnt, bflag (cleared together, b_zero bytes
// from key) | K28: edges, fld | trig | per group: bcnt, lcount, lstart, lcnt, box | the segment table (tseg, tid, tpiece) | the tail
// (xc_cpiece_link.h)
struct CdWs {
    long long* off; unsigned long long* key; int *nsel, *err; unsigned long long* pairs; CdpWs p; double* trig;
    int *bcnt, *lcount, *lstart, *lcnt; double *box, *tseg; int *tid, *tpiece; CpTail tail; size_t b_zero = 0;
    size_t lay(Carve a, int64_t nrange, size_t ntrig, int64_t nb, bool sphere, const CpPlan& pl)
    {
        off = a.take<long long>((size_t)nrange + 1);
        b_zero = a.mark();
        key = a.take<unsigned long long>((size_t)nrange); nsel = a.take<int>((size_t)nrange); err = a.take<int>(CP_SMALL);
        pairs = a.take<unsigned long long>(4);
        p.lay_cleared(a);
        b_zero = a.mark() - b_zero;
        p.lay_tables(a);
        trig = a.take<double>(ntrig);
        const size_t gb = (size_t)pl.gmax * (size_t)nb;
        bcnt = a.take<int>(gb); lcount = a.take<int>((size_t)pl.gmax); lstart = a.take<int>(gb); lcnt = a.take<int>(gb);
        box = a.take<double>(gb * (size_t)(sphere ? CD_NBOX_SPHERE : CD_NBOX_PLANE));
        tseg = a.take<double>((size_t)pl.nmax * (size_t)(sphere ? CD_ND_SPHERE : CD_ND_PLANE));
        tid = a.take<int>((size_t)pl.nmax); tpiece = a.take<int>((size_t)pl.nmax);
        cp_carve_tail(a, pl, 6, tail);
        return a.at;
    }
};

// What K28 adds to a call, in one place: its arguments in the order of the C ABI, their refusals, the sizes of its words, the prepare
// step in front of the groups and the finish step behind them.  The tile pass itself is k_cd_profile's.
struct CdK28 {
    int nedge; const double* edges; int ncont; const double* w; int w_per_slab; int nf; const void* const* f;
    const int *f_dtype, *f_per_slab; int64_t* nodes; double *area, *sums; int32_t* flags;
    static constexpr int NSTAT = 2;             // its statistic words behind the two pair counts: the tiles of the LDS window, of the global path

    template <typename Refuse> int validate(Refuse&& refuse, int64_t nrange) const
    {
        bool ok = edges && nedge >= 2 && nedge <= CDP_MAX_EDGES;
        for (int i = 0; ok && i < nedge; ++i) ok = std::isfinite(edges[i]) && (i == 0 || edges[i] > edges[i - 1]);
        if (!ok) return refuse(": edges must be 2 to 4097 finite, strictly ascending float64 values");
        if (nf < 0 || nf > XC_PROPS_MAXF) return refuse(": at most 8 fields (XC_PROPS_MAXF)");
        if (nf > 0 && (!f || !f_dtype || !f_per_slab || !sums)) return refuse(": the fields, their dtypes and sums go together");
        for (int m = 0; m < nf; ++m)
            if (!f[m] || (f_dtype[m] != XC_F32 && f_dtype[m] != XC_F64)) return refuse(": a field is a device plane of XC_F32 or XC_F64");
        if (ncont < 1 || nrange % ncont != 0) return refuse(": nrange must be a multiple of ncont >= 1");
        if (nrange / ncont > 65535) return refuse(": more than 65535 slabs");
        return XC_OK;
    }
    void size(CdpWs& p, int64_t nrange) const
    {
        p.nslab = (size_t)(nrange / ncont); p.n_mxg = p.nslab * (size_t)std::max(nf, 1);
        p.n_bin = (size_t)nrange * (size_t)(nedge - 1); p.n_ch = (size_t)(1 + nf); p.n_edge = (size_t)nedge; p.n_fld = XC_PROPS_MAXF;
    }
    // the edges and the fields as the kernels read them; the windows' tops; stage 5.  P: what k_cd_profile takes.
    int prepare(xc_ctx* ctx, StageTimer& tm, CdpWs& p, size_t npl, unsigned long long* tiles, CdProf& P) const
    {
        for (int m = 0; m < nf; ++m) p.h_fld[m] = {f[m], f_per_slab[m] ? (unsigned long long)npl : 0ull, f_dtype[m] == XC_F32 ? 1 : 0, 0};
        XC_HIP(ctx, hipMemcpyAsync(p.edges, edges, (size_t)nedge * 8, hipMemcpyHostToDevice, ctx->stream));
        XC_HIP(ctx, hipMemcpyAsync(p.fld, p.h_fld, sizeof(p.h_fld), hipMemcpyHostToDevice, ctx->stream));
        ci_launch_bound(ctx->stream, (int64_t)npl, (int64_t)p.nslab, w, w_per_slab, nullptr, 0, p.mxw);
        if (nf > 0) pp_launch_bound(ctx->stream, (int64_t)npl, (int64_t)p.nslab, nf, w, w_per_slab, p.fld, p.mxg);
        XC_HIP(ctx, hipGetLastError());
        tm.mark(5);
        P.nedge = nedge; P.nf = nf; P.ncont = ncont; P.global = ctx->cdprofile_global; P.edges = p.edges; P.w = w; P.w_per_slab = w_per_slab;
        P.fld = p.fld; P.mxw = p.mxw; P.mxg = p.mxg; P.acc = p.acc; P.cnt = p.cnt; P.bflag = p.bflag; P.tiles = tiles;
        return XC_OK;
    }
    // the words rounded once into the caller's tables; stage 6
    int finish(xc_ctx* ctx, StageTimer& tm, const CdpWs& p, int64_t nrange) const
    {
        const int M = nedge - 1, nch = 1 + nf;
        XC_HIP(ctx, hipMemsetAsync(flags, 0, (size_t)nrange * (size_t)nch * 4, ctx->stream));
        hipLaunchKernelGGL(k_cd_profile_finish, dim3(cp_blocks(nrange * M * nch)), dim3(CP_TPB), 0, ctx->stream, nrange, M, nf, ncont, p.acc, p.cnt,
                           p.bflag, p.mxw, p.mxg, (long long*)nodes, area, sums, (int*)flags);
        XC_HIP(ctx, hipGetLastError());
        tm.mark(6);
        return XC_OK;
    }
};

// One call of xc_contour_distance_dev or xc_contour_distance_profile_dev: what the two share in the order of the C ABI, K27's planes,
// K28's part (null for K27: it writes planes, K28 bins them where they are made).
struct CdCall {
    const char* who; xc_ctx::CdLast* last; int nstat;                      // the entry, its record of the context, the statistic words it reports
    int64_t nrange; const uint64_t* count; const int64_t *e_from, *e_to; const double* pts; int64_t ny, nx; int periodic, select;
    const double *ycoord, *xcoord; double period, radius, max_dist; const uint8_t* negate_mask;
    bool outs;                                                             // the outputs the entry cannot do without are all there
    double* dist; int64_t *edge, *piece;
    const CdK28* k28;
};

// One group on the plane or on the sphere: its binning (count, scan, fill, box; stage 3), the edge table handed on, and the tiles of its
// ranges in as many launches as keep a grid below 2^31 blocks -- k_cd_profile with K28's operands P, k_cd_dist without.
template <bool SPHERE>
int cd_group(xc_ctx* ctx, StageTimer& tm, CpRun& run, const CdWs& ws, const CdSel& S, const double* pts, CdArgs A, const CdProf* P)
{
    const dim3 blk(CP_TPB);
    const int64_t r0 = run.g.r0, r1 = run.g.r1, ng = r1 - r0, nb = A.nb, nbc = (A.nx + CD_B - 1) / CD_B;
    hipLaunchKernelGGL(k_cd_count, run.grid, blk, 0, ctx->stream, run.n, run.s0, r0, run.pl.E, A.nx, nbc, nb, S, ws.bcnt);
    hipLaunchKernelGGL(k_cd_scan, dim3((unsigned)ng), blk, 0, ctx->stream, nb, ws.bcnt, ws.lcount, ws.lstart, ws.lcnt);
    hipLaunchKernelGGL((k_cd_fill<SPHERE>), run.grid, blk, 0, ctx->stream, run.n, run.s0, r0, run.pl.E, A.ny, A.nx, nbc, nb, A.wrap, A.period, S,
                       ws.off, pts, A.fy, A.fx, ws.bcnt, ws.tseg, ws.tid, ws.tpiece);
    hipLaunchKernelGGL((k_cd_box<SPHERE>), dim3(cp_blocks(ng * nb)), blk, 0, ctx->stream, ng, nb, run.s0, r0, ws.off, ws.lcount, ws.lstart,
                       ws.lcnt, ws.tseg, ws.box);
    XC_HIP(ctx, hipGetLastError());
    tm.mark(3);
    XC_TRY(run.end());
    const int64_t ntile = A.nty * A.ntx, step = std::max<int64_t>(1, (((int64_t)1 << 31) - 1) / ntile);
    A.g0 = r0; A.s0 = run.s0;
    for (int64_t ra = r0; ra < r1; ra += step) {
        A.ra = ra;
        const dim3 grid((unsigned)(std::min<int64_t>(step, r1 - ra) * ntile));
        if (P) hipLaunchKernelGGL((k_cd_profile<SPHERE>), grid, dim3(CD_TPB), 0, ctx->stream, A, *P);
        else hipLaunchKernelGGL((k_cd_dist<SPHERE>), grid, dim3(CD_TPB), 0, ctx->stream, A);
        XC_HIP(ctx, hipGetLastError());
    }
    return XC_OK;
}

}  // namespace

// One call.  Waits for the stream three times: for K12's counts (they size the groups and fix the rounds), for the word that says whether
// the ids were in range (before anything is written), and for the pair counts of the profile.
static int launch_cdist(xc_ctx* ctx, const CdCall& c)
{
    const std::string who_s(c.who);
    auto refuse = [&](const char* what) { return fail(ctx, XC_EBADARG, who_s + what); };
    const char* who = c.who;
    const CdK28* k28 = c.k28;
    const int64_t nrange = c.nrange, ny = c.ny, nx = c.nx;
    const int periodic = c.periodic;
    const double period = c.period, radius = c.radius, max_dist = c.max_dist;
    if (!c.count || !c.ycoord || !c.xcoord || nrange < 1 || ny < 1 || nx < 1 || !c.outs) return refuse(": bad arguments");
    XC_TRY(co_check_select(ctx, who, periodic, c.select));
    if (!(radius >= 0.0) || !std::isfinite(radius)) return refuse(": radius must be finite and >= 0");
    if (periodic && (!std::isfinite(period) || period == 0.0 || nx < 2)) return refuse(": a periodic plane needs a finite, non-zero period and nx >= 2");
    if (radius > 0.0 && periodic && period != CD_RING && period != -CD_RING)
        return refuse(": on the sphere the period is float64(deg2rad(float32(+-360))): the plane is a sphere or none");
    if (max_dist != max_dist) return refuse(": max_dist is NaN");
    XC_TRY(co_check_plane(ctx, who, periodic, ny, nx));
    if (nrange > ((int64_t)1 << 40) / (ny * nx)) return refuse(": nrange ny nx must stay below 2^40");
    if (k28) XC_TRY(k28->validate(refuse, nrange));
    const long long E = 2 * ny * nx;
    const int wrap = periodic ? 1 : 0;
    const bool sphere = radius > 0.0;
    CpProfile& prof = c.last->prof;
    profile_clear(prof);
    unsigned long long* hstat = c.last->stat;
    for (int i = 0; i < c.nstat; ++i) hstat[i] = 0;

    CpPlan pl;                                                               // (no group without segments: the outputs are written all the same)
    XC_TRY(cp_plan(ctx, who, nrange, c.count, nullptr, c.e_from, c.e_to, c.pts, E, pl));
    const int64_t nb = ((ny + CD_B - 1) / CD_B) * ((nx + CD_B - 1) / CD_B);
    CdWs ws;
    if (k28) k28->size(ws.p, nrange);
    XC_TRY(lay_out(ctx, &ctx->cpiece_ws, &ctx->cpiece_ws_bytes,
                   [&](Carve a) { return ws.lay(a, nrange, sphere ? (size_t)(2 * ny + 2 * nx) : 0, nb, sphere, pl); }));

    // the stages of the profiles: 0 table, 1 rounds, 2 select, 3 binning, 4 distance; K28: 5 bound, 6 finish
    StageTimer tm(ctx, prof.ms);                                             // where the time goes (xc_set_kernel_timing)
    CpRun run(ctx, tm, pl, c.e_from, c.e_to, ws.off, ws.tail, ws.err);
    const dim3 blk(CP_TPB);
    const size_t npl = (size_t)ny * (size_t)nx;

    tm.mark(-1);
    XC_HIP(ctx, hipMemsetAsync(ws.key, 0, ws.b_zero, ctx->stream));
    if (pl.total > 0) {                                                      // the ids first: a refusal writes nothing
        hipLaunchKernelGGL(k_cd_check, dim3(cp_blocks(pl.total)), blk, 0, ctx->stream, (int64_t)pl.total, E, (const long long*)c.e_from,
                           (const long long*)c.e_to, ws.err);
        XC_HIP(ctx, hipGetLastError());
        int herr = 0;
        XC_TRY(cp_read_err(ctx, ws.err, &herr));
        if (herr) return refuse(": an edge id outside [0, 2 ny nx)");
    }
    if (sphere) {
        hipLaunchKernelGGL(k_cd_trig, dim3(cp_blocks(std::max(ny, nx))), blk, 0, ctx->stream, ny, nx, c.ycoord, c.xcoord, ws.trig);
        XC_HIP(ctx, hipGetLastError());
    }
    tm.mark(3);
    CdProf P = {};
    if (k28) XC_TRY(k28->prepare(ctx, tm, ws.p, npl, ws.pairs + 2, P));
    XC_TRY(run.upload_off());
    XC_TRY(run.fill_table());
    tm.mark(0);

    // K27: the planes of the ranges [a, b) without any segment (K28's words of such a range stay zero)
    auto none = [&](int64_t a, int64_t b) -> int {
        if (k28) return XC_OK;
        for (int64_t r = a; r < b; ++r) {
            hipLaunchKernelGGL(k_cd_none, dim3((unsigned)((npl + CP_TPB - 1) / CP_TPB)), blk, 0, ctx->stream, (size_t)r * npl, npl, c.dist,
                               (long long*)c.edge, (long long*)c.piece);
        }
        XC_HIP(ctx, hipGetLastError());
        return XC_OK;
    };
    CdArgs A;
    A.ny = ny; A.nx = nx; A.nty = (ny + CD_T - 1) / CD_T; A.ntx = (nx + CD_T - 1) / CD_T; A.nb = nb; A.wrap = wrap; A.prune = ctx->cdist_prune;
    A.period = wrap ? period : 0.0; A.radius = radius; A.cap = (max_dist > 0.0 && std::isfinite(max_dist)) ? max_dist : 0.0;
    A.fy = c.ycoord; A.fx = c.xcoord; A.trig = ws.trig; A.off = ws.off; A.lcount = ws.lcount; A.lstart = ws.lstart; A.lcnt = ws.lcnt; A.box = ws.box;
    A.tseg = ws.tseg; A.tid = ws.tid; A.tpiece = ws.tpiece; A.mask = c.negate_mask; A.dist = c.dist; A.edge = (long long*)c.edge;
    A.piece = (long long*)c.piece; A.pairs = ws.pairs;
    const auto group = sphere ? cd_group<true> : cd_group<false>;            // the plane or the sphere, chosen once
    const CdProf* tile = k28 ? &P : nullptr;                                 // k_cd_profile's operands, or k_cd_dist

    int64_t done = 0;                                                       // the ranges written so far
    for (const CpGroup& g : pl.groups) {
        XC_TRY(none(done, g.r0));
        XC_HIP(ctx, hipMemsetAsync(ws.bcnt, 0, (size_t)(g.r1 - g.r0) * (size_t)nb * 4, ctx->stream));
        tm.mark(3);
        run.begin(g);
        XC_TRY(run.rounds());
        const CoRoles s = co_launch_select(run, wrap, nx, c.pts, c.select, ws.nsel, ws.key);
        XC_HIP(ctx, hipGetLastError());
        tm.mark(2);
        const CdSel S = {c.select, run.e_from, ws.tail.rid, s.root, run.b.prv, run.b.lab, s.pn, s.pw, ws.key};
        XC_TRY(group(ctx, tm, run, ws, S, c.pts, A, tile));
        done = g.r1;
        tm.mark(4);
    }
    XC_TRY(none(done, nrange));
    tm.mark(4);
    if (k28) XC_TRY(k28->finish(ctx, tm, ws.p, nrange));
    run.report(prof);
    XC_HIP(ctx, hipMemcpyAsync(hstat, ws.pairs, (size_t)c.nstat * 8, hipMemcpyDeviceToHost, ctx->stream));
    XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return XC_OK;
}

// the sixteen arguments the two entries share, into the call of the entry `who` with its record and the number of its statistic words
static CdCall cd_call(const char* who, xc_ctx::CdLast* last, int nstat, int64_t nrange, const uint64_t* count, const int64_t* e_from,
                      const int64_t* e_to, const double* pts, int64_t ny, int64_t nx, int periodic, int select, const double* ycoord,
                      const double* xcoord, double period, double radius, double max_dist, const uint8_t* negate_mask)
{
    CdCall c = {};
    c.who = who; c.last = last; c.nstat = nstat;
    c.nrange = nrange; c.count = count; c.e_from = e_from; c.e_to = e_to; c.pts = pts; c.ny = ny; c.nx = nx; c.periodic = periodic;
    c.select = select; c.ycoord = ycoord; c.xcoord = xcoord; c.period = period; c.radius = radius; c.max_dist = max_dist;
    c.negate_mask = negate_mask;
    return c;
}

// behind the two xc_last_*_profile: table = stages 0 + 1 + 2, binning = 3, distance = 4, then `more` further stages as they are; the
// pair counts; the groups
static int cd_last(xc_ctx* ctx, xc_ctx::CdLast xc_ctx::* rec, int more, double* ms, int64_t* pairs_visited, int64_t* pairs_total, int* groups)
{
    if (!ctx) return fail(nullptr, XC_EBADARG, "null context");
    const xc_ctx::CdLast& l = ctx->*rec;
    const CpProfile& p = l.prof;
    if (ms) {
        ms[0] = (double)p.ms[0] + (double)p.ms[1] + (double)p.ms[2]; ms[1] = (double)p.ms[3]; ms[2] = (double)p.ms[4];
        for (int k = 0; k < more; ++k) ms[3 + k] = (double)p.ms[5 + k];
    }
    if (pairs_visited) *pairs_visited = (int64_t)l.stat[0];
    if (pairs_total) *pairs_total = (int64_t)l.stat[1];
    if (groups) *groups = p.groups;
    return XC_OK;
}

}  // namespace xc

// ------------------------------------------------------------------------------------ C ABI
int xc_contour_distance_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to, const double* pts,
                            int64_t ny, int64_t nx, int periodic, int select, const double* ycoord, const double* xcoord, double period,
                            double radius, double max_dist, const uint8_t* negate_mask, double* dist, int64_t* edge, int64_t* piece)
{
    XC_CTX(ctx);
    xc::CdCall c = xc::cd_call("xc_contour_distance", &ctx->last_cdist, 2, nrange, count, e_from, e_to, pts, ny, nx, periodic, select, ycoord,
                               xcoord, period, radius, max_dist, negate_mask);
    c.outs = dist != nullptr; c.dist = dist; c.edge = edge; c.piece = piece;
    return xc::launch_cdist(ctx, c);
}

int xc_contour_distance_profile_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to,
                                    const double* pts, int64_t ny, int64_t nx, int periodic, int select, const double* ycoord,
                                    const double* xcoord, double period, double radius, double max_dist, const uint8_t* negate_mask,
                                    int nedge, const double* edges, int ncont, const double* w, int w_per_slab, int nf, const void* const* f,
                                    const int* f_dtype, const int* f_per_slab, int64_t* nodes, double* area, double* sums, int32_t* flags)
{
    XC_CTX(ctx);
    const xc::CdK28 k28 = {nedge, edges, ncont, w, w_per_slab, nf, f, f_dtype, f_per_slab, nodes, area, sums, flags};
    xc::CdCall c = xc::cd_call("xc_contour_distance_profile", &ctx->last_cdprofile, 2 + xc::CdK28::NSTAT, nrange, count, e_from, e_to, pts, ny, nx,
                               periodic, select, ycoord, xcoord, period, radius, max_dist, negate_mask);
    c.outs = nodes && area && flags; c.k28 = &k28;
    return xc::launch_cdist(ctx, c);
}

int xc_set_cdist_prune(xc_ctx* ctx, int on)
{
    if (!ctx) return xc::fail(nullptr, XC_EBADARG, "null context");
    ctx->cdist_prune = on ? 1 : 0;
    return XC_OK;
}

int xc_set_cdprofile_global(xc_ctx* ctx, int on)
{
    if (!ctx) return xc::fail(nullptr, XC_EBADARG, "null context");
    ctx->cdprofile_global = on ? 1 : 0;
    return XC_OK;
}

int xc_last_cdist_profile(xc_ctx* ctx, double* ms, int64_t* pairs_visited, int64_t* pairs_total, int* groups)
{
    return xc::cd_last(ctx, &xc_ctx::last_cdist, 0, ms, pairs_visited, pairs_total, groups);
}

int xc_last_cdprofile_profile(xc_ctx* ctx, double* ms, int64_t* pairs_visited, int64_t* pairs_total, int64_t* tiles_window,
                              int64_t* tiles_global, int* groups)
{
    XC_TRY(xc::cd_last(ctx, &xc_ctx::last_cdprofile, 2, ms, pairs_visited, pairs_total, groups));
    if (tiles_window) *tiles_window = (int64_t)ctx->last_cdprofile.stat[2];
    if (tiles_global) *tiles_global = (int64_t)ctx->last_cdprofile.stat[3];
    return XC_OK;
}

// C ABI, part 4: the host forms of the kernels outside the Keff chain -- row sums (K2), the squared gradient (K4), the local wave
// activity (K7, xc_lwa.hip), the sorted profile (K8, xc_sort.hip), crossings (K9, xc_cross.hip), contour lengths (K10, xc_clen.hip; K11, xc_lclen.hip), line integrals along contours (K15, xc_cline.hip), contour segments (K12, xc_cseg.hip),
// the contour map (K25, xc_cmap.hip), synthetic slabs -- and the records of what they launched.
#include "xc_capi.h"
#include <cmath>

using namespace xc;

// the levels of K9 / K10, [nc][ncont]: ascending (ties allowed), no NaN
static bool check_ascending(const double* contours, int64_t nc, int ncont)
{
    for (int64_t s = 0; s < nc; ++s)
        for (int k = 0; k < ncont; ++k) {
            const double c = contours[s * ncont + k];
            if (c != c || (k > 0 && c < contours[s * ncont + k - 1])) return false;
        }
    return true;
}

// what several forms refuse alike, each under its own name: a coordinate that is not finite ...
static int check_coords(xc_ctx* ctx, const char* who, const double* ycoord, int64_t ny, const double* xcoord, int64_t nx)
{
    for (int64_t i = 0; i < ny + nx; ++i)
        if (!std::isfinite(i < ny ? ycoord[i] : xcoord[i - ny])) return fail(ctx, XC_EBADARG, std::string(who) + ": coordinates must be finite");
    return XC_OK;
}
// ... and levels, one set (*nc = 1) or one per slab, that do not ascend
static int check_levels(xc_ctx* ctx, const char* who, const double* contours, int contours_per_slab, int64_t nslab, int ncont, int64_t* nc)
{
    *nc = contours_per_slab ? nslab : 1;
    return check_ascending(contours, *nc, ncont) ? XC_OK : fail(ctx, XC_EEDGES, std::string(who) + ": contours must be ascending without NaN");
}

// the levels of K25, [nc][N]: finite and strictly monotonic in the direction of their ends, slab by slab; a slab with a NaN end is the
// all-NaN tracer's and is let through.  Two adjacent equal levels anywhere come first, under the reference's own text
static int check_map_levels(xc_ctx* ctx, const double* xp, int64_t nc, int N)
{
    for (int64_t s = 0; s < nc; ++s) {
        const double* x = xp + s * N;
        if (x[0] != x[0] || x[N - 1] != x[N - 1]) continue;
        for (int k = 1; k < N; ++k) if (x[k] == x[k - 1]) return fail(ctx, XC_EEDGES, "non monotonic bins");
    }
    for (int64_t s = 0; s < nc; ++s) {
        const double* x = xp + s * N;
        if (x[0] != x[0] || x[N - 1] != x[N - 1]) continue;
        const bool up = x[0] < x[N - 1];
        for (int k = 0; k < N; ++k)
            if (!std::isfinite(x[k]) || (k > 0 && (up ? !(x[k] > x[k - 1]) : !(x[k] < x[k - 1]))))
                return fail(ctx, XC_EBADARG, "xc_contour_map: the levels of every slab must be finite and strictly monotonic");
    }
    return XC_OK;
}

// xc_last_clen_geometry: launch_contour_lengths writes the record where it picks the geometry; a call that fails leaves it cleared
static int clen_recorded(xc_ctx* ctx, int rc)
{
    if (rc != XC_OK) ctx->last_clen = xc_clen_geometry{};
    return rc;
}

// the period of a periodic X direction (K10, K11) against the host coordinates: finite, non-zero, of the sign of
// xcoord[nx-1] - xcoord[0] and longer than that span; the ring needs nx >= 2
static bool check_period(const double* xcoord, int64_t nx, double period)
{
    if (nx < 2 || !std::isfinite(period) || period == 0.0) return false;
    const double span = xcoord[nx - 1] - xcoord[0];
    if ((span > 0.0 && period < 0.0) || (span < 0.0 && period > 0.0)) return false;
    return std::fabs(period) > std::fabs(span);
}

// The frame the host forms of K10, K11, K15 and K26 share: the refusals they have in common, the byte sizes, and the tracer, the coordinates
// and the levels staged.  A form names itself, calls the steps in the order its refusals are tested in, with its own refusals between them, and
// states its further inputs, its outputs and its launch.
struct Frame {
    xc_ctx* ctx; const char* who; const void* q; int q_dtype; int64_t nslab, ny, nx; const double *ycoord, *xcoord;
    const double* levels;                                    // null: none are staged (K11 at the window means)
    Stage st; const void *pq = nullptr, *pf = nullptr; double *dy = nullptr, *dx = nullptr, *dc = nullptr;
    Frame(xc_ctx* c, const char* w, const void* q_, int dt, int64_t ns, int64_t ny_, int64_t nx_, const double* y, const double* x, const double* lv)
        : ctx(c), who(w), q(q_), q_dtype(dt), nslab(ns), ny(ny_), nx(nx_), ycoord(y), xcoord(x), levels(lv), st(c) {}
    int refuse(const char* what) const { return fail(ctx, XC_EBADARG, std::string(who) + what); }
    size_t cells() const { return (size_t)nslab * ny * nx; }
    // the first two refusals.  more: the form's further pointers and counts are there; dtypes: its further dtypes are floats
    int arguments(bool more, bool dtypes = true)
    {
        if (!more || !q || !ycoord || !xcoord || nslab < 1 || ny < 1 || nx < 1) return refuse(": bad arguments");
        return dtypes && is_float(q_dtype) ? XC_OK : refuse(": bad dtype");
    }
    // finite coordinates, then the period of a ring under the form's own text
    int coordinates(bool ring, double period, const char* text)
    {
        XC_TRY(check_coords(ctx, who, ycoord, ny, xcoord, nx));
        return ring && !check_period(xcoord, nx, period) ? fail(ctx, XC_EBADARG, text) : XC_OK;
    }
    // the levels, one set or one per slab, ascend without NaN
    int ascending(int ncont, int per_slab) { int64_t nc; return check_levels(ctx, who, levels, per_slab, nslab, ncont, &nc); }
    // The arena laid out -- the tracer, a second plane `f` of `fb` bytes (K15's integrand; null: none), the coordinates, the levels of `lb`
    // bytes, then what `outs` takes -- and the inputs staged and flushed: pq / pf, dy, dx, dc are what the launch reads
    template <typename Lay> int stage(const void* f, size_t fb, size_t lb, Lay&& outs)
    {
        const size_t qb = cells() * esize(q_dtype), yb = (size_t)ny * 8, xb = (size_t)nx * 8;
        void *dq, *df = nullptr;
        XC_TRY(lay_stage(st, [&](Stage& s) {
            dq = s.take(qb); if (f) df = s.take(fb); dy = s.take<double>(yb); dx = s.take<double>(xb); dc = levels ? s.take<double>(lb) : nullptr;
            outs(s);
        }));
        XC_TRY(stage_in(ctx, dq, q, qb, &pq));              // (a tracer / integrand with a device mirror is read where it is)
        if (f) XC_TRY(stage_in(ctx, df, f, fb, &pf));
        XC_TRY(h2d(ctx, dy, ycoord, yb)); XC_TRY(h2d(ctx, dx, xcoord, xb));
        if (levels) XC_TRY(h2d(ctx, dc, levels, lb));
        return flush_in(ctx);
    }
    // behind the launch: the results handed over
    int finish(int launched) { XC_TRY(launched); XC_TRY(st.deliver()); return xc_sync(ctx); }
};
static size_t level_bytes(int contours_per_slab, int64_t nslab, int ncont) { return (size_t)(contours_per_slab ? nslab : 1) * ncont * 8; }

// `periodic` == 0: `period` is not read and X does not wrap
static int local_contour_lengths_host(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                                      const double* ycoord, const double* xcoord, int periodic, double period, double radius,
                                      int64_t wy, int64_t wx, int64_t sy, int64_t sx, int64_t min_periods,
                                      const double* levels, double* out_len, double* out_level, uint64_t* out_nseg)
{
    Frame fr(ctx, "xc_local_contour_lengths", q, q_dtype, nslab, ny, nx, ycoord, xcoord, levels);
    XC_TRY(fr.arguments(out_len));
    if (wy < 2 || wx < 2) return fail(ctx, XC_EBADARG, "xc_local_contour_lengths: the window must be at least 2 x 2 nodes");
    if (sy < 1 || sx < 1) return fail(ctx, XC_EBADARG, "xc_local_contour_lengths: strides must be >= 1");
    XC_TRY(fr.coordinates(periodic, period, "xc_local_contour_lengths_periodic: period must be finite, non-zero, of the sign of "
                                            "xcoord[nx-1] - xcoord[0] and longer than that span, and nx >= 2"));
    if (periodic && wx > nx)
        return fail(ctx, XC_EBADARG, "xc_local_contour_lengths_periodic: the window must not be wider than the ring (wx <= nx)");
    const size_t ob = (size_t)nslab * (size_t)((ny + sy - 1) / sy) * (size_t)((nx + sx - 1) / sx) * 8;        // (results and levels: one per window)
    double *dl, *de; uint64_t* dn;
    XC_TRY(fr.stage(nullptr, 0, ob, [&](Stage& s) { dl = s.out(out_len, ob); de = s.out(out_level, ob); dn = s.out(out_nseg, ob); }));
    return fr.finish(launch_local_contour_lengths(ctx, fr.pq, q_dtype, nslab, ny, nx, fr.dy, fr.dx, periodic ? period : 0.0, radius, wy, wx, sy, sx,
                                                  min_periods, fr.dc, dl, de, dn));
}

static int contour_lengths_host(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                                const double* ycoord, const double* xcoord, int periodic, double period, double radius,
                                const double* contours, int ncont, int contours_per_slab,
                                double* out_len, uint64_t* out_nseg)
{
    Frame fr(ctx, "xc_contour_lengths", q, q_dtype, nslab, ny, nx, ycoord, xcoord, contours);
    XC_TRY(fr.arguments(contours && out_len && ncont >= 1));
    if (!(radius >= 0.0)) return fail(ctx, XC_EBADARG, "xc_contour_lengths: radius must be >= 0");
    XC_TRY(fr.coordinates(periodic, period, "xc_contour_lengths_periodic: period must be finite, non-zero, of the sign of xcoord[nx-1] - xcoord[0] "
                                            "and longer than that span, and nx >= 2"));
    XC_TRY(fr.ascending(ncont, contours_per_slab));
    const size_t ob = (size_t)nslab * ncont * 8; double* dl; uint64_t* dn;
    XC_TRY(fr.stage(nullptr, 0, level_bytes(contours_per_slab, nslab, ncont), [&](Stage& s) { dl = s.out(out_len, ob); dn = s.out(out_nseg, ob); }));
    return fr.finish(launch_contour_lengths(ctx, fr.pq, q_dtype, nslab, ny, nx, fr.dy, fr.dx, periodic ? period : 0.0, radius, fr.dc, ncont,
                                            contours_per_slab, dl, dn));
}

// period == 0.0: X has two free edges
static int contour_line_integrals_host(xc_ctx* ctx, const void* q, int q_dtype, const void* f, int f_dtype, int64_t nslab, int64_t ny,
                                       int64_t nx, const double* ycoord, const double* xcoord, double period, double radius,
                                       const double* contours, int ncont, int contours_per_slab,
                                       double* out_integral, double* out_length, uint64_t* out_nseg)
{
    Frame fr(ctx, "xc_contour_line_integrals", q, q_dtype, nslab, ny, nx, ycoord, xcoord, contours);
    XC_TRY(fr.arguments(f && contours && out_integral && out_length && ncont >= 1, is_float(f_dtype)));
    if (!(radius >= 0.0)) return fail(ctx, XC_EBADARG, "xc_contour_line_integrals: radius must be >= 0");
    XC_TRY(fr.coordinates(period != 0.0, period, "xc_contour_line_integrals: period must be 0, or finite, of the sign of xcoord[nx-1] - xcoord[0] "
                                                 "and longer than that span, and nx >= 2"));
    XC_TRY(fr.ascending(ncont, contours_per_slab));
    const size_t ob = (size_t)nslab * ncont * 8; double *di, *dl; uint64_t* dn;
    XC_TRY(fr.stage(f, fr.cells() * esize(f_dtype), level_bytes(contours_per_slab, nslab, ncont), [&](Stage& s) {
        di = s.out(out_integral, ob); dl = s.out(out_length, ob); dn = s.out(out_nseg, ob); }));
    return fr.finish(launch_contour_line_integrals(ctx, fr.pq, q_dtype, fr.pf, f_dtype, nslab, ny, nx, fr.dy, fr.dx, period, radius, fr.dc, ncont,
                                                   contours_per_slab, di, dl, dn));
}

extern "C" {

// ------------------------------------------------------------------------------------ K2
int xc_rowsum_dev(xc_ctx* ctx, const void* mask, int mask_dtype, const double* dA, int dA_rank,
                  int64_t ny, int64_t nx, int multiply, double* out_rows)
{
    XC_CTX(ctx);
    return launch_rowsum(ctx, mask, mask_dtype, dA, dA_rank, ny, nx, multiply, out_rows);
}

int xc_rowsum(xc_ctx* ctx, const void* mask, int mask_dtype, const double* dA, int dA_rank,
              int64_t ny, int64_t nx, int multiply, double* out_rows)
{
    XC_CTX(ctx);
    if (!out_rows || ny < 1 || nx < 1) return fail(ctx, XC_EBADARG, "xc_rowsum: bad arguments");
    if (mask && !is_float(mask_dtype)) return fail(ctx, XC_EBADARG, "xc_rowsum: bad mask dtype");
    const size_t mb = mask ? (size_t)ny * nx * esize(mask_dtype) : 0;
    const size_t dab = dA_rank == XC_DA_SLAB ? 0 : dA_bytes(dA_rank, 1, ny, nx);     // (per-slab weights: left to the launcher to reject)
    if (dab && !dA) return fail(ctx, XC_EBADARG, "xc_rowsum: dA is NULL");
    Stage st(ctx); void *sm = nullptr, *sd = nullptr; double* dout;
    XC_TRY(lay_stage(st, [&](Stage& s) { if (mb) sm = s.take(mb); if (dab) sd = s.take(dab); dout = s.out(out_rows, (size_t)ny * 8, true); }));
    const void *dm = nullptr, *dd = nullptr;                 // (resident inputs are read where they are: no device-to-device copy into the arena)
    if (mb) XC_TRY(stage_in(ctx, sm, mask, mb, &dm));
    if (dab) XC_TRY(stage_in(ctx, sd, dA, dab, &dd));
    XC_TRY(flush_in(ctx));
    XC_TRY(launch_rowsum(ctx, dm, mask_dtype, (const double*)dd, dA_rank, ny, nx, multiply, dout));
    XC_TRY(st.deliver());
    return xc_sync(ctx);
}

// ------------------------------------------------------------------------------------ K4
int xc_grad2_dev(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                 const double* rdx, const double* rdy, int periodic_x, double* out)
{
    XC_CTX(ctx);
    return launch_grad2(ctx, q, q_dtype, nslab, ny, nx, rdx, rdy, periodic_x, out);
}

int xc_grad2(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
             const double* rdx, const double* rdy, int periodic_x, double* out)
{
    XC_CTX(ctx);
    if (!q || !rdx || !rdy || !out || nslab < 1 || ny < 1 || nx < 1) return fail(ctx, XC_EBADARG, "xc_grad2: bad arguments");
    if (!is_float(q_dtype)) return fail(ctx, XC_EBADARG, "xc_grad2: bad dtype");
    const size_t cells = (size_t)nslab * ny * nx, qb = cells * esize(q_dtype), ob = cells * 8, rb = (size_t)ny * 8;
    Stage st(ctx); void* dq; double *dx, *dy, *dout;
    XC_TRY(lay_stage(st, [&](Stage& s) { dq = s.take(qb); dx = s.take<double>(rb); dy = s.take<double>(rb); dout = s.out(out, ob); }));
    const void* pq;                                          // (a tracer with a device mirror is read where it is)
    XC_TRY(stage_in(ctx, dq, q, qb, &pq)); XC_TRY(h2d(ctx, dx, rdx, rb)); XC_TRY(h2d(ctx, dy, rdy, rb));
    XC_TRY(flush_in(ctx));
    XC_TRY(launch_grad2(ctx, pq, q_dtype, nslab, ny, nx, dx, dy, periodic_x, dout));
    XC_TRY(st.deliver());
    return xc_sync(ctx);
}

// ------------------------------------------------------------------------------------ K25
int xc_contour_map_dev(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                       const double* xp, int N, int xp_per_slab,
                       int nv, const double* const* fp, const int* fp_per_slab, void* const* out, int out_dtype)
{
    XC_CTX(ctx);
    return launch_contour_map(ctx, q, q_dtype, nslab, ny, nx, xp, N, xp_per_slab, nv, fp, fp_per_slab, out, out_dtype);
}

int xc_contour_map(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                   const double* xp, int N, int xp_per_slab,
                   int nv, const double* const* fp, const int* fp_per_slab, void* const* out, int out_dtype)
{
    XC_CTX(ctx);
    if (!q || !xp || !fp || !fp_per_slab || !out || nslab < 1 || ny < 1 || nx < 1 || N < 2 || nv < 1 || nv > XC_CMAP_MAXV)
        return fail(ctx, XC_EBADARG, "xc_contour_map: bad arguments");
    for (int v = 0; v < nv; ++v)
        if (!fp[v] || !out[v]) return fail(ctx, XC_EBADARG, "xc_contour_map: bad arguments");
    if (!is_float(q_dtype) || !is_float(out_dtype)) return fail(ctx, XC_EBADARG, "xc_contour_map: bad dtype");
    if (nslab > 65535 || (int64_t)(nv + 1) * N > XC_CMAP_MAX_LDS_DOUBLES)          // (the launcher's limits, before anything is staged)
        return fail(ctx, XC_EBADARG, "xc_contour_map: at most 65535 slabs, and (nv + 1) * N <= XC_CMAP_MAX_LDS_DOUBLES");
    XC_TRY(check_map_levels(ctx, xp, xp_per_slab ? nslab : 1, N));
    const size_t cells = (size_t)nslab * ny * nx, qb = cells * esize(q_dtype), ob = cells * esize(out_dtype);
    const size_t xb = (size_t)(xp_per_slab ? nslab : 1) * N * 8;
    Stage st(ctx); void* dq; double* dx; const double* df[XC_CMAP_MAXV]; void* dout[XC_CMAP_MAXV];
    XC_TRY(lay_stage(st, [&](Stage& s) {
        dq = s.take(qb); dx = s.take<double>(xb);
        for (int v = 0; v < nv; ++v) df[v] = s.take<double>((size_t)(fp_per_slab[v] ? nslab : 1) * N * 8);
        for (int v = 0; v < nv; ++v) dout[v] = s.out((char*)out[v], ob);
    }));
    const void* pq;                                          // (a tracer with a device mirror is read where it is)
    XC_TRY(stage_in(ctx, dq, q, qb, &pq)); XC_TRY(h2d(ctx, dx, xp, xb));
    for (int v = 0; v < nv; ++v) XC_TRY(h2d(ctx, (void*)df[v], fp[v], (size_t)(fp_per_slab[v] ? nslab : 1) * N * 8));
    XC_TRY(flush_in(ctx));
    XC_TRY(launch_contour_map(ctx, pq, q_dtype, nslab, ny, nx, dx, N, xp_per_slab, nv, df, fp_per_slab, dout, out_dtype));
    XC_TRY(st.deliver());
    return xc_sync(ctx);
}

// ------------------------------------------------------------------------------------ K9
int xc_crossing_dev(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                    int pad_x, int pad_mode, const double* contours, int ncont, int contours_per_slab,
                    const void* area, int area_dtype, int area_per_slab, int stride, int full_width,
                    double* out_len, uint64_t* out_cnt)
{
    XC_CTX(ctx);
    return launch_crossing(ctx, q, q_dtype, nslab, ny, nx, pad_x, pad_mode, contours, ncont, contours_per_slab,
                           area, area_dtype, area_per_slab, stride, full_width, out_len, out_cnt);
}

int xc_crossing(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                int pad_x, int pad_mode, const double* contours, int ncont, int contours_per_slab,
                const void* area, int area_dtype, int area_per_slab, int stride, int full_width,
                double* out_len, uint64_t* out_cnt)
{
    XC_CTX(ctx);
    if (!q || !contours || !area || (!out_len && !out_cnt) || nslab < 1 || ny < 1 || nx < 1 || ncont < 1)
        return fail(ctx, XC_EBADARG, "xc_crossing: bad arguments");
    if (!is_float(q_dtype) || !is_float(area_dtype)) return fail(ctx, XC_EBADARG, "xc_crossing: bad dtype");
    int64_t nc; XC_TRY(check_levels(ctx, "xc_crossing", contours, contours_per_slab, nslab, ncont, &nc));
    const size_t cells = (size_t)nslab * ny * nx, qb = cells * esize(q_dtype);
    const size_t ab = (area_per_slab ? cells : (size_t)ny * nx) * esize(area_dtype);
    const size_t cb = (size_t)nc * ncont * 8, ob = (size_t)nslab * ncont * 8;
    Stage st(ctx); void *dq, *da; double *dc, *dl; uint64_t* dn;
    XC_TRY(lay_stage(st, [&](Stage& s) { dq = s.take(qb); da = s.take(ab); dc = s.take<double>(cb); dl = s.out(out_len, ob); dn = s.out(out_cnt, ob); }));
    const void* pq; const void* pa;                          // (tracer / areas with a device mirror are read where they are)
    XC_TRY(stage_in(ctx, dq, q, qb, &pq)); XC_TRY(stage_in(ctx, da, area, ab, &pa)); XC_TRY(h2d(ctx, dc, contours, cb));
    XC_TRY(flush_in(ctx));
    XC_TRY(launch_crossing(ctx, pq, q_dtype, nslab, ny, nx, pad_x, pad_mode, dc, ncont, contours_per_slab,
                           pa, area_dtype, area_per_slab, stride, full_width, dl, dn));
    XC_TRY(st.deliver());
    return xc_sync(ctx);
}

// ------------------------------------------------------------------------------------ K10
int xc_contour_lengths_dev(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                           const double* ycoord, const double* xcoord, double radius,
                           const double* contours, int ncont, int contours_per_slab,
                           double* out_len, uint64_t* out_nseg)
{
    XC_CTX(ctx);
    ctx->last_clen = xc_clen_geometry{};
    return clen_recorded(ctx, launch_contour_lengths(ctx, q, q_dtype, nslab, ny, nx, ycoord, xcoord, 0.0, radius, contours, ncont,
                                                     contours_per_slab, out_len, out_nseg));
}

int xc_contour_lengths(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                       const double* ycoord, const double* xcoord, double radius,
                       const double* contours, int ncont, int contours_per_slab,
                       double* out_len, uint64_t* out_nseg)
{
    XC_CTX(ctx);
    ctx->last_clen = xc_clen_geometry{};
    return clen_recorded(ctx, contour_lengths_host(ctx, q, q_dtype, nslab, ny, nx, ycoord, xcoord, 0, 0.0, radius, contours, ncont,
                                                   contours_per_slab, out_len, out_nseg));
}

// (the device form cannot read the coordinates: its caller vouches for the period's sign and length)
int xc_contour_lengths_periodic_dev(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                                    const double* ycoord, const double* xcoord, double period, double radius,
                                    const double* contours, int ncont, int contours_per_slab,
                                    double* out_len, uint64_t* out_nseg)
{
    XC_CTX(ctx);
    ctx->last_clen = xc_clen_geometry{};
    if (!std::isfinite(period) || period == 0.0 || nx < 2)
        return fail(ctx, XC_EBADARG, "xc_contour_lengths_periodic: period must be finite and non-zero, and nx >= 2");
    return clen_recorded(ctx, launch_contour_lengths(ctx, q, q_dtype, nslab, ny, nx, ycoord, xcoord, period, radius, contours, ncont,
                                                     contours_per_slab, out_len, out_nseg));
}

int xc_contour_lengths_periodic(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                                const double* ycoord, const double* xcoord, double period, double radius,
                                const double* contours, int ncont, int contours_per_slab,
                                double* out_len, uint64_t* out_nseg)
{
    XC_CTX(ctx);
    ctx->last_clen = xc_clen_geometry{};
    return clen_recorded(ctx, contour_lengths_host(ctx, q, q_dtype, nslab, ny, nx, ycoord, xcoord, 1, period, radius, contours, ncont,
                                                   contours_per_slab, out_len, out_nseg));
}

int xc_last_clen_geometry(xc_ctx* ctx, xc_clen_geometry* out)
{
    if (!ctx || !out) return fail(ctx, XC_EBADARG, "xc_last_clen_geometry: bad arguments");
    *out = ctx->last_clen;
    return XC_OK;
}

// ------------------------------------------------------------------------------------ K26
int xc_coarsen_dev(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx, int ratio, int skipna, double* out)
{
    XC_CTX(ctx);
    return launch_coarsen(ctx, q, q_dtype, nslab, ny, nx, ratio, skipna, out);
}

int xc_coarsen(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx, int ratio, int skipna, double* out)
{
    XC_CTX(ctx);
    ctx->last_cscale = xc_cscale_geometry{};
    if (!q || !out || nslab < 1 || ny < 1 || nx < 1 || !is_float(q_dtype) || ratio < 1 || ratio > XC_CSCALE_MAXRATIO || ny / ratio < 1 || nx / ratio < 1)
        return launch_coarsen(ctx, q, q_dtype, nslab, ny, nx, ratio, skipna, out);       // (refused there, under its texts, before anything is staged)
    const size_t qb = (size_t)nslab * ny * nx * esize(q_dtype), ob = (size_t)nslab * (ny / ratio) * (nx / ratio) * 8;
    Stage st(ctx); void* dq; double* dout;
    XC_TRY(lay_stage(st, [&](Stage& s) { dq = s.take(qb); dout = s.out(out, ob); }));
    const void* pq;                                          // (a tracer with a device mirror is read where it is)
    XC_TRY(stage_in(ctx, dq, q, qb, &pq));
    XC_TRY(flush_in(ctx));
    XC_TRY(launch_coarsen(ctx, pq, q_dtype, nslab, ny, nx, ratio, skipna, dout));
    XC_TRY(st.deliver());
    return xc_sync(ctx);
}

// (the device form cannot read the coordinates or the levels: its caller vouches for them, as for K10's device forms)
int xc_contour_lengths_scales_dev(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                                  const double* ycoord, const double* xcoord, double period, double radius,
                                  const int* ratios, int nratio, int skipna,
                                  const double* contours, int ncont, int contours_per_slab, double* out_len, uint64_t* out_nseg)
{
    XC_CTX(ctx);
    ctx->last_clen = xc_clen_geometry{};
    return clen_recorded(ctx, launch_contour_lengths_scales(ctx, q, q_dtype, nslab, ny, nx, ycoord, xcoord, period, radius, ratios, nratio,
                                                            skipna, contours, ncont, contours_per_slab, out_len, out_nseg));
}

int xc_contour_lengths_scales(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                              const double* ycoord, const double* xcoord, double period, double radius,
                              const int* ratios, int nratio, int skipna,
                              const double* contours, int ncont, int contours_per_slab, double* out_len, uint64_t* out_nseg)
{
    XC_CTX(ctx);
    ctx->last_clen = xc_clen_geometry{};
    ctx->last_cscale = xc_cscale_geometry{};
    const char* who = "xc_contour_lengths_scales";
    Frame fr(ctx, who, q, q_dtype, nslab, ny, nx, ycoord, xcoord, contours);
    XC_TRY(fr.arguments(ratios && contours && out_len && ncont >= 1));
    if (!(radius >= 0.0)) return fr.refuse(": radius must be >= 0");
    if (nslab > 65535) return fr.refuse(": at most 65535 slabs per call");
    XC_TRY(cscale_check_ratios(ctx, ny, nx, ratios, nratio, period != 0.0));
    XC_TRY(fr.coordinates(period != 0.0, period, "xc_contour_lengths_scales: period must be finite, of the sign of xcoord[nx-1] - xcoord[0] and "
                                                 "longer than that span, and nx >= 2 (0: X has two free edges)"));
    XC_TRY(fr.ascending(ncont, contours_per_slab));
    const size_t ob = (size_t)nratio * nslab * ncont * 8; double* dl; uint64_t* dn;
    XC_TRY(fr.stage(nullptr, 0, level_bytes(contours_per_slab, nslab, ncont), [&](Stage& s) { dl = s.out(out_len, ob); dn = s.out(out_nseg, ob); }));
    return fr.finish(clen_recorded(ctx, launch_contour_lengths_scales(ctx, fr.pq, q_dtype, nslab, ny, nx, fr.dy, fr.dx, period, radius, ratios, nratio,
                                                                      skipna, fr.dc, ncont, contours_per_slab, dl, dn)));
}

int xc_last_cscale_geometry(xc_ctx* ctx, xc_cscale_geometry* out)
{
    if (!ctx || !out) return fail(ctx, XC_EBADARG, "xc_last_cscale_geometry: bad arguments");
    *out = ctx->last_cscale;
    return XC_OK;
}

// ------------------------------------------------------------------------------------ K15
// (the device form cannot read the coordinates: its caller vouches for a period's sign and length)
int xc_contour_line_integrals_dev(xc_ctx* ctx, const void* q, int q_dtype, const void* f, int f_dtype, int64_t nslab, int64_t ny, int64_t nx,
                                  const double* ycoord, const double* xcoord, double period, double radius,
                                  const double* contours, int ncont, int contours_per_slab,
                                  double* out_integral, double* out_length, uint64_t* out_nseg)
{
    XC_CTX(ctx);
    ctx->last_clen = xc_clen_geometry{};
    return clen_recorded(ctx, launch_contour_line_integrals(ctx, q, q_dtype, f, f_dtype, nslab, ny, nx, ycoord, xcoord, period, radius,
                                                            contours, ncont, contours_per_slab, out_integral, out_length, out_nseg));
}

int xc_contour_line_integrals(xc_ctx* ctx, const void* q, int q_dtype, const void* f, int f_dtype, int64_t nslab, int64_t ny, int64_t nx,
                              const double* ycoord, const double* xcoord, double period, double radius,
                              const double* contours, int ncont, int contours_per_slab,
                              double* out_integral, double* out_length, uint64_t* out_nseg)
{
    XC_CTX(ctx);
    ctx->last_clen = xc_clen_geometry{};
    return clen_recorded(ctx, contour_line_integrals_host(ctx, q, q_dtype, f, f_dtype, nslab, ny, nx, ycoord, xcoord, period, radius,
                                                          contours, ncont, contours_per_slab, out_integral, out_length, out_nseg));
}

// ------------------------------------------------------------------------------------ K11
int xc_local_contour_lengths_dev(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                                 const double* ycoord, const double* xcoord, double radius,
                                 int64_t wy, int64_t wx, int64_t sy, int64_t sx, int64_t min_periods,
                                 const double* levels, double* out_len, double* out_level, uint64_t* out_nseg)
{
    XC_CTX(ctx);
    return launch_local_contour_lengths(ctx, q, q_dtype, nslab, ny, nx, ycoord, xcoord, 0.0, radius, wy, wx, sy, sx, min_periods,
                                        levels, out_len, out_level, out_nseg);
}

int xc_local_contour_lengths(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                             const double* ycoord, const double* xcoord, double radius,
                             int64_t wy, int64_t wx, int64_t sy, int64_t sx, int64_t min_periods,
                             const double* levels, double* out_len, double* out_level, uint64_t* out_nseg)
{
    XC_CTX(ctx);
    return local_contour_lengths_host(ctx, q, q_dtype, nslab, ny, nx, ycoord, xcoord, 0, 0.0, radius, wy, wx, sy, sx, min_periods,
                                      levels, out_len, out_level, out_nseg);
}

// (the device form cannot read the coordinates: its caller vouches for the period's sign and length)
int xc_local_contour_lengths_periodic_dev(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                                          const double* ycoord, const double* xcoord, double period, double radius,
                                          int64_t wy, int64_t wx, int64_t sy, int64_t sx, int64_t min_periods,
                                          const double* levels, double* out_len, double* out_level, uint64_t* out_nseg)
{
    XC_CTX(ctx);
    if (!std::isfinite(period) || period == 0.0 || nx < 2)
        return fail(ctx, XC_EBADARG, "xc_local_contour_lengths_periodic: period must be finite and non-zero, and nx >= 2");
    return launch_local_contour_lengths(ctx, q, q_dtype, nslab, ny, nx, ycoord, xcoord, period, radius, wy, wx, sy, sx, min_periods,
                                        levels, out_len, out_level, out_nseg);
}

int xc_local_contour_lengths_periodic(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                                      const double* ycoord, const double* xcoord, double period, double radius,
                                      int64_t wy, int64_t wx, int64_t sy, int64_t sx, int64_t min_periods,
                                      const double* levels, double* out_len, double* out_level, uint64_t* out_nseg)
{
    XC_CTX(ctx);
    return local_contour_lengths_host(ctx, q, q_dtype, nslab, ny, nx, ycoord, xcoord, 1, period, radius, wy, wx, sy, sx, min_periods,
                                      levels, out_len, out_level, out_nseg);
}

// ------------------------------------------------------------------------------------ K12
int xc_contour_segments_dev(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                            const double* contours, int ncont, int contours_per_slab, int64_t capacity,
                            uint64_t* out_count, int64_t* e_from, int64_t* e_to, double* pts)
{
    XC_CTX(ctx);
    return launch_contour_segments(ctx, q, q_dtype, nslab, ny, nx, 0, contours, ncont, contours_per_slab, capacity, out_count, e_from, e_to,
                                   pts, nullptr);
}

int xc_contour_segments_periodic_dev(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                                     const double* contours, int ncont, int contours_per_slab, int64_t capacity,
                                     uint64_t* out_count, int64_t* e_from, int64_t* e_to, double* pts)
{
    XC_CTX(ctx);
    return launch_contour_segments(ctx, q, q_dtype, nslab, ny, nx, 1, contours, ncont, contours_per_slab, capacity, out_count, e_from, e_to,
                                   pts, nullptr);
}

// The records are as many as the field has segments, known only after the count pass: they land in a device block of their own,
// taken and released inside the call, and are copied out from there.  wrap: the _periodic form.
static int contour_segments_host(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx, int wrap,
                                 const double* contours, int ncont, int contours_per_slab, int64_t capacity,
                                 uint64_t* out_count, int64_t* e_from, int64_t* e_to, double* pts)
{
    if (!q || !contours || !out_count || nslab < 1 || ny < 1 || nx < 1 || ncont < 1 || capacity < 0)
        return fail(ctx, XC_EBADARG, "xc_contour_segments: bad arguments");
    if (wrap && nx < 2) return fail(ctx, XC_EBADARG, "xc_contour_segments_periodic: nx >= 2");
    if (!is_float(q_dtype)) return fail(ctx, XC_EBADARG, "xc_contour_segments: bad dtype");
    if (capacity > 0 && (!e_from || !e_to || !pts)) return fail(ctx, XC_EBADARG, "xc_contour_segments: capacity > 0 needs the record arrays");
    int64_t nc; XC_TRY(check_levels(ctx, "xc_contour_segments", contours, contours_per_slab, nslab, ncont, &nc));
    const size_t qb = (size_t)nslab * ny * nx * esize(q_dtype), cb = (size_t)nc * ncont * 8, ob = (size_t)nslab * ncont * 8;
    Stage st(ctx); void* dq; double* dc; uint64_t* dn;
    XC_TRY(lay_stage(st, [&](Stage& s) { dq = s.take(qb); dc = s.take<double>(cb); dn = s.out(out_count, ob); }));
    const void* pq;                                          // (a tracer with a device mirror is read where it is)
    XC_TRY(stage_in(ctx, dq, q, qb, &pq)); XC_TRY(h2d(ctx, dc, contours, cb));
    XC_TRY(flush_in(ctx));
    int64_t total = 0;
    int rc = launch_contour_segments(ctx, pq, q_dtype, nslab, ny, nx, wrap, dc, ncont, contours_per_slab, 0, dn, nullptr, nullptr, nullptr,
                                     &total);
    if (rc < 0) return rc;
    XC_TRY(st.deliver());
    XC_TRY(xc_sync(ctx));
    if (total > capacity) return 1;
    if (total == 0) return XC_OK;
    char* rec = nullptr;                                      // e_from | e_to | pts
    const size_t n8 = (size_t)total * 8;
    if (hipMalloc((void**)&rec, 6 * n8) != hipSuccess) { (void)hipGetLastError(); return fail(ctx, XC_ENOMEM, "xc_contour_segments: no device memory for the records"); }
    rc = launch_contour_segments(ctx, pq, q_dtype, nslab, ny, nx, wrap, dc, ncont, contours_per_slab, total, dn, (int64_t*)rec,
                                 (int64_t*)(rec + n8), (double*)(rec + 2 * n8), nullptr);
    hipError_t e = hipSuccess;
    if (rc == XC_OK) {
        e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess) e = hipMemcpy(e_from, rec, n8, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(e_to, rec + n8, n8, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(pts, rec + 2 * n8, 4 * n8, hipMemcpyDeviceToHost);
    }
    (void)hipFree(rec);
    if (e != hipSuccess) return hipfail(ctx, e, "xc_contour_segments: copying the records");
    return rc;
}

int xc_contour_segments(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                        const double* contours, int ncont, int contours_per_slab, int64_t capacity,
                        uint64_t* out_count, int64_t* e_from, int64_t* e_to, double* pts)
{
    XC_CTX(ctx);
    return contour_segments_host(ctx, q, q_dtype, nslab, ny, nx, 0, contours, ncont, contours_per_slab, capacity, out_count, e_from, e_to, pts);
}

int xc_contour_segments_periodic(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                                 const double* contours, int ncont, int contours_per_slab, int64_t capacity,
                                 uint64_t* out_count, int64_t* e_from, int64_t* e_to, double* pts)
{
    XC_CTX(ctx);
    return contour_segments_host(ctx, q, q_dtype, nslab, ny, nx, 1, contours, ncont, contours_per_slab, capacity, out_count, e_from, e_to, pts);
}

// ------------------------------------------------------------------------------------ K7
int xc_lwa_dev(xc_ctx* ctx, const void* q, int q_dtype, const double* Q, const double* coord,
               const double* dA, int dA_rank, double dA_max, const double* M, int M_rank,
               int64_t nslab, int64_t ny, int64_t nx, int increase, int part, int variant,
               const int32_t* mask_idx, int nmask, double* out_lwa, int8_t* out_masks)
{
    XC_CTX(ctx);
    const LwaArgs a = {q, q_dtype, Q, coord, dA, dA_rank, dA_max, M, M_rank, nslab, ny, nx, increase, part, variant, mask_idx, nmask, out_lwa, out_masks};
    return launch_lwa(ctx, a);
}

int xc_lwa(xc_ctx* ctx, const void* q, int q_dtype, const double* Q, const double* coord,
           const double* dA, int dA_rank, double dA_max, const double* M, int M_rank,
           int64_t nslab, int64_t ny, int64_t nx, int increase, int part, int variant,
           const int32_t* mask_idx, int nmask, double* out_lwa, int8_t* out_masks)
{
    XC_CTX(ctx);
    if (!q || !Q || !coord || !dA || !out_lwa || nslab < 1 || ny < 2 || nx < 1) return fail(ctx, XC_EBADARG, "xc_lwa: bad arguments");
    if (!is_float(q_dtype)) return fail(ctx, XC_EBADARG, "xc_lwa: bad dtype");
    if (nmask < 0 || (nmask > 0 && (!mask_idx || !out_masks))) return fail(ctx, XC_EBADARG, "xc_lwa: mask arguments");
    for (int i = 0; i < nmask; ++i)
        if (mask_idx[i] < 0 || mask_idx[i] >= ny) return fail(ctx, XC_EBADARG, "indices in mask_idx out of boundary");
    const size_t cells = (size_t)nslab * ny * nx;
    const size_t qb = cells * esize(q_dtype), Qb = (size_t)nslab * ny * 8, cb = (size_t)ny * 8;
    const size_t dab = dA_bytes(dA_rank, 1, ny, nx), Mb = dA_bytes(M_rank, 1, ny, nx);      // (ROW or PLANE, checked by the launcher; M: or none)
    const size_t ob = cells * 8, mib = (size_t)nmask * 4, mob = (size_t)nmask * cells;
    Stage st(ctx); void* dq; double *dQ, *dc, *dd, *dM, *dout; int32_t* dmi; int8_t* dmo;
    XC_TRY(lay_stage(st, [&](Stage& s) {
        dq = s.take(qb); dQ = s.take<double>(Qb); dc = s.take<double>(cb); dd = s.take<double>(dab); dM = Mb ? s.take<double>(Mb) : nullptr;
        dout = s.out(out_lwa, ob); dmi = nmask ? s.take<int32_t>(mib) : nullptr; dmo = nmask ? s.out(out_masks, mob) : nullptr;
    }));
    // the read-only planes are used where they are when they have a device mirror (the weights of a resident object: no device-to-device
    // copy per call); Q and the coordinate are small (pinned buffer + copy kernel)
    const void* pq; const void* pd; const void* pM = nullptr;
    XC_TRY(stage_in(ctx, dq, q, qb, &pq)); XC_TRY(h2d(ctx, dQ, Q, Qb)); XC_TRY(h2d(ctx, dc, coord, cb)); XC_TRY(stage_in(ctx, dd, dA, dab, &pd));
    if (Mb) XC_TRY(stage_in(ctx, dM, M, Mb, &pM));
    if (nmask) XC_TRY(h2d(ctx, dmi, mask_idx, mib));
    XC_TRY(flush_in(ctx));
    const LwaArgs a = {pq, q_dtype, dQ, dc, (const double*)pd, dA_rank, dA_max, (const double*)pM, M_rank, nslab, ny, nx, increase, part, variant,
                       dmi, nmask, dout, dmo};
    XC_TRY(launch_lwa(ctx, a));
    XC_TRY(st.deliver());
    return xc_sync(ctx);
}

// ------------------------------------------------------------------------------------ K8
int xc_sort_profile_batch_dev(xc_ctx* ctx, const void* q, int q_dtype, const void* mask, int mask_dtype, int mask_per_slab,
                              const double* dA, int dA_rank, int64_t nslab, int64_t ny, int64_t nx, int negate,
                              const double* targets, int J, const double* tbl, const double* coord, int ntbl,
                              double* out_Q, double* out_qsorted, double* out_acum, uint32_t* out_nvalid, double* out_bpe)
{
    XC_CTX(ctx);
    if (ny < 1 || nx < 1 || nslab < 1) return fail(ctx, XC_EBADARG, "xc_sort_profile: bad shape");
    XC_TRY(ensure_scratch(ctx, sort_workspace_bytes(ny * nx, nslab)));
    const SortArgs a = {q, q_dtype, mask, mask_dtype, mask_per_slab, dA, dA_rank, nslab, ny, nx, negate, targets, J, tbl, coord, ntbl,
                        ctx->scratch, out_Q, out_qsorted, out_acum, out_nvalid, out_bpe};
    return launch_sort_profile(ctx, a);
}

int xc_sort_profile_batch(xc_ctx* ctx, const void* q, int q_dtype, const void* mask, int mask_dtype, int mask_per_slab,
                          const double* dA, int dA_rank, int64_t nslab, int64_t ny, int64_t nx, int negate,
                          const double* targets, int J, const double* tbl, const double* coord, int ntbl,
                          double* out_Q, double* out_qsorted, double* out_acum, uint32_t* out_nvalid, double* out_bpe)
{
    XC_CTX(ctx);
    if (!q || ny < 1 || nx < 1 || nslab < 1 || J < 0) return fail(ctx, XC_EBADARG, "xc_sort_profile: bad arguments");
    if (!is_float(q_dtype)) return fail(ctx, XC_EBADARG, "xc_sort_profile: bad dtype");
    if (mask && !is_float(mask_dtype)) return fail(ctx, XC_EBADARG, "xc_sort_profile: bad mask dtype");
    const size_t S = (size_t)nslab, n = (size_t)ny * nx;
    const size_t qb = S * n * esize(q_dtype), mb = mask ? (mask_per_slab ? S : 1) * n * esize(mask_dtype) : 0;
    const size_t dab = dA_bytes(dA_rank, nslab, ny, nx);
    if (dab && !dA) return fail(ctx, XC_EBADARG, "xc_sort_profile: dA is NULL");
    const size_t tb = (size_t)J * 8, Qb = S * tb, tbb = (out_bpe ? (size_t)ntbl * 8 : 0);
    Stage st(ctx); void *dq, *dm = nullptr; double *dd = nullptr, *dt = nullptr, *dQ = nullptr, *dtbl = nullptr, *dcrd = nullptr, *dqs, *dac, *dbpe; uint32_t* dnv;
    XC_TRY(lay_stage(st, [&](Stage& s) {
        dq = s.take(qb); if (mb) dm = s.take(mb); if (dab) dd = s.take<double>(dab);
        if (J > 0 && out_Q) { dt = s.take<double>(tb); dQ = s.out(out_Q, Qb); }
        if (out_bpe) { dtbl = s.take<double>(tbb); dcrd = s.take<double>(tbb); }
        dqs = s.out(out_qsorted, S * n * 8); dac = s.out(out_acum, S * n * 8);
        dnv = s.keep(out_nvalid, S * 4);                     // (the kernel counts whether the caller asks or not)
        dbpe = s.out(out_bpe, S * 8);
    }));
    XC_TRY(h2d(ctx, dq, q, qb));
    if (mb) XC_TRY(h2d(ctx, dm, mask, mb));
    if (dab) XC_TRY(h2d(ctx, dd, dA, dab));
    if (J > 0 && out_Q) XC_TRY(h2d(ctx, dt, targets, tb));
    if (out_bpe) {
        if (!tbl || !coord || ntbl < 2) return fail(ctx, XC_EBADARG, "xc_sort_profile: BPE needs tbl/coord");
        XC_TRY(h2d(ctx, dtbl, tbl, tbb)); XC_TRY(h2d(ctx, dcrd, coord, tbb));
    }
    XC_TRY(flush_in(ctx));
    XC_TRY(xc_sort_profile_batch_dev(ctx, dq, q_dtype, dm, mask_dtype, mask_per_slab, dd, dA_rank, nslab, ny, nx, negate,
                                     dt, dQ ? J : 0, dtbl, dcrd, ntbl, dQ, dqs, dac, dnv, dbpe));
    XC_TRY(st.deliver());
    return xc_sync(ctx);
}

int xc_sort_profile_dev(xc_ctx* ctx, const void* q, int q_dtype, const void* mask, int mask_dtype,
                        const double* dA, int dA_rank, int64_t ny, int64_t nx, int negate,
                        const double* targets, int J, const double* tbl, const double* coord, int ntbl,
                        double* out_Q, double* out_qsorted, double* out_acum, uint32_t* out_nvalid, double* out_bpe)
{
    if (dA_rank == XC_DA_SLAB) return fail(ctx, XC_EBADARG, "xc_sort_profile: dA_rank must be NONE, ROW or PLANE");
    return xc_sort_profile_batch_dev(ctx, q, q_dtype, mask, mask_dtype, 0, dA, dA_rank, 1, ny, nx, negate, targets, J, tbl, coord, ntbl,
                                     out_Q, out_qsorted, out_acum, out_nvalid, out_bpe);
}

int xc_sort_profile(xc_ctx* ctx, const void* q, int q_dtype, const void* mask, int mask_dtype,
                    const double* dA, int dA_rank, int64_t ny, int64_t nx, int negate,
                    const double* targets, int J, const double* tbl, const double* coord, int ntbl,
                    double* out_Q, double* out_qsorted, double* out_acum, uint32_t* out_nvalid, double* out_bpe)
{
    if (dA_rank == XC_DA_SLAB) return fail(ctx, XC_EBADARG, "xc_sort_profile: dA_rank must be NONE, ROW or PLANE");
    return xc_sort_profile_batch(ctx, q, q_dtype, mask, mask_dtype, 0, dA, dA_rank, 1, ny, nx, negate, targets, J, tbl, coord, ntbl,
                                 out_Q, out_qsorted, out_acum, out_nvalid, out_bpe);
}

int xc_set_lwa_exact(xc_ctx* ctx, int exact)
{
    if (!ctx) return fail(nullptr, XC_EBADARG, "null context");
    if (exact < 0 || exact > 3) return fail(ctx, XC_EBADARG, "xc_set_lwa_exact: mode must be 0 (automatic), 1 (band walk), 2 (interval kernel, checked) or 3 (interval kernel, premises vouched for)");
    ctx->lwa_exact = exact;
    return XC_OK;
}

int xc_last_lwa_path(xc_ctx* ctx, int* out_path)
{
    if (!ctx || !out_path) return fail(ctx, XC_EBADARG, "xc_last_lwa_path: bad arguments");
    if (ctx->last_lwa_path < 0) {                                      // decided by the device-side check of the last call: read its flag
        unsigned f = 0;
        XC_HIP(ctx, hipSetDevice(ctx->device));
        XC_HIP(ctx, hipMemcpyAsync(&f, ctx->lwa_flag, sizeof(f), hipMemcpyDeviceToHost, ctx->stream));
        XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ctx->last_lwa_path = (f == ctx->lwa_epoch) ? 2 : 1;
    }
    *out_path = ctx->last_lwa_path;
    return XC_OK;
}

int xc_last_sort_path(xc_ctx* ctx, int* out_path)
{
    if (!ctx || !out_path) return fail(ctx, XC_EBADARG, "xc_last_sort_path: bad arguments");
    *out_path = ctx->last_sort_path;
    return XC_OK;
}

// ------------------------------------------------------------------------------------ synthetic slabs
int xc_synth_dev(xc_ctx* ctx, void* out, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                 const double* lat_deg, const double* lon_deg, uint64_t seed, int variant)
{
    XC_CTX(ctx);
    if (out && nslab > 0 && ny > 0 && nx > 0) mm_touch(ctx, out, (size_t)nslab * ny * nx * esize(q_dtype));
    return launch_synth(ctx, out, q_dtype, nslab, ny, nx, lat_deg, lon_deg, seed, variant);
}

}  // extern "C"

// K26  contour lengths at coarsened resolutions (xc_coarsen, xc_contour_lengths_scales).  gfx950 only.
//
// The reference's fractal-dimension workflow hands cal_contour_lengths a block-averaged tracer once per ruler.  Here the tracer is
// uploaded once, coarsened on the GPU for every ratio and traced by K10 (xc_clen.hip), which is not changed.  Rule (build-defined, in
// include/xcontour_hip.h, K26 section): coarse node (I, J) of ratio r is the mean of the fine block [I r, I r + r) x [J r, J r + r),
// trailing rows and columns that fill no block dropped; every value is promoted to float64; a block row is summed left to right
// starting FROM its first element, the row sums top to bottom starting FROM the first; the mean is that sum divided once by
// double(r r).  skipna: NaN nodes are left out of the same order, a row without a node adds nothing, the divisor is the number of
// nodes used, a block without a node is NaN.  Additions and one division only: nothing for contraction to change.
//
// Mapping: k_coarsen<T>, 256 threads = four waves, grid (tiles in x, tiles in y, slabs).  A tile is kCscaleRows = 4 coarse rows (one per
// wave) of tx coarse columns, tx = 64, 32 or 16 so that a wave's fine row segment, tx r values, stays within kCscaleSeg = 1024.  One
// LANE owns one coarse node and walks its block in the order above, so the result cannot depend on the launch geometry; no atomics, no
// cross-lane sums.  The fine plane is never read with a stride: for each of the r fine rows the wave loads its segment in passes of 64
// consecutive values (lane l reads base + 64 p + l), parks them in LDS and, after the barrier, every lane reads its own r values back in
// order.  In LDS a lane's run starts at lane * (r | 1): the odd stride keeps the 32 lanes of a read group on different banks for every
// r (at stride r = 32 they would all share one).
// The coordinates take the same rule in one dimension (k_coarsen_coords, one lane per coarse coordinate; a few thousand values).
//
// Launcher: for each ratio in the caller's order -- coarsen into the workspace (ratio 1: nothing, K10 reads the caller's plane and
// coordinates), then launch_contour_lengths on the workspace, periodic when a period is given.  All on the context's stream; the
// workspace, one Carve layout sized by the largest coarse plane, is reused ratio after ratio, which the stream order makes safe.  It is a
// block of its own (ctx->cscale_ws): K10 lays its partial sums out over ctx->scratch and may move that block.
#include "xc_capi.h"
#include <cmath>

namespace xc {

namespace {

constexpr int kCscaleThreads = 256;
constexpr int kCscaleRows    = 4;           // coarse rows of a tile: one per wave
constexpr int kCscaleSeg     = 1024;        // fine values of one wave's row segment at most
constexpr int kCscalePasses  = kCscaleSeg / 64;
static_assert(kCscaleThreads == 64 * kCscaleRows, "one wave per coarse row of the tile");
static_assert(XC_CSCALE_MAXRATIO * 16 <= kCscaleSeg, "the narrowest tile (16 columns) of the largest ratio fits the segment");

__host__ __device__ inline int cscale_tile_x(int r) { return r <= kCscaleSeg / 64 ? 64 : (r <= kCscaleSeg / 32 ? 32 : 16); }

__device__ __forceinline__ double cs_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// the running sum of one order: `add` takes the next value; the first one taken starts the sum
struct SeqSum {
    double s = 0.0; bool any = false;
    __device__ __forceinline__ void add(double x) { s = any ? __dadd_rn(s, x) : x; any = true; }
};

template <typename T>
__global__ __launch_bounds__(kCscaleThreads)
void k_coarsen(const T* __restrict__ q, int64_t ny, int64_t nx, int r, int skipna, int tx, int64_t cny, int64_t cnx,
               double* __restrict__ out)
{
    extern __shared__ __align__(16) unsigned char s_raw[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int stride = r | 1;                                              // LDS values between the runs of two lanes
    T* sw = reinterpret_cast<T*>(s_raw) + (size_t)wave * tx * stride;     // this wave's segment
    const int64_t J0 = (int64_t)blockIdx.x * tx, I = (int64_t)blockIdx.y * kCscaleRows + wave, slab = blockIdx.z;
    const int ncol = (int)(cnx - J0 < tx ? cnx - J0 : tx);                 // coarse columns of this tile (>= 1)
    const bool row_in = I < cny;
    const int seg = row_in ? ncol * r : 0;                                 // fine values of the wave's segment
    const T* row0 = q + ((size_t)slab * ny + (size_t)(row_in ? I : 0) * r) * nx + (size_t)J0 * r;
    // where value e = 64 p + lane of the segment lies in LDS: e + pad (e / r), the quotient kept by steps instead of a division per value
    const int pad = stride - r, dq = 64 / r, dm = 64 % r, npass = (tx * r + 63) / 64;
    SeqSum total; int n = 0;
    for (int dr = 0; dr < r; ++dr) {
        const T* src = row0 + (size_t)dr * nx;
        T v[kCscalePasses];
#pragma unroll
        for (int p = 0; p < kCscalePasses; ++p) {
            const int e = p * 64 + lane;
            if (p < npass && e < seg) v[p] = src[e];
        }
        int qe = lane / r, me = lane % r;
#pragma unroll
        for (int p = 0; p < kCscalePasses; ++p) {
            const int e = p * 64 + lane;
            if (p < npass && e < seg) sw[e + pad * qe] = v[p];
            qe += dq; me += dm;
            if (me >= r) { me -= r; ++qe; }
        }
        __syncthreads();
        if (row_in && lane < ncol) {
            const T* mine = sw + (size_t)lane * stride;
            SeqSum rs;
            for (int k = 0; k < r; ++k) {
                const double x = (double)mine[k];
                if (skipna && x != x) continue;
                rs.add(x); ++n;
            }
            if (rs.any) total.add(rs.s);
        }
        __syncthreads();
    }
    if (row_in && lane < ncol)
        out[((size_t)slab * cny + I) * cnx + J0 + lane] = n > 0 ? __ddiv_rn(total.s, (double)n) : cs_nan();
}

// Yc[I] = (y[I r] + ... + y[I r + r - 1]) / double(r), summed in that order from the first; Xc the same.  One lane per coordinate
__global__ __launch_bounds__(256)
void k_coarsen_coords(const double* __restrict__ y, int64_t cny, const double* __restrict__ x, int64_t cnx, int r,
                      double* __restrict__ yc, double* __restrict__ xc)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= cny + cnx) return;
    const double* src = i < cny ? y + i * r : x + (i - cny) * r;
    double s = src[0];
    for (int k = 1; k < r; ++k) s = __dadd_rn(s, src[k]);
    (i < cny ? yc[i] : xc[i - cny]) = __ddiv_rn(s, (double)r);
}

// one coarsen launch and its line `slot` of the record
int coarsen_into(xc_ctx* ctx, xc_cscale_geometry& g, int slot, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx, int r,
                 int skipna, double* out)
{
    const int64_t cny = ny / r, cnx = nx / r;
    const int tx = cscale_tile_x(r);
    const dim3 grid((unsigned)((cnx + tx - 1) / tx), (unsigned)((cny + kCscaleRows - 1) / kCscaleRows), (unsigned)nslab);
    const size_t lds = (size_t)kCscaleRows * tx * (r | 1) * esize(q_dtype);
    if (q_dtype == XC_F64)
        hipLaunchKernelGGL(k_coarsen<double>, grid, dim3(kCscaleThreads), lds, ctx->stream, (const double*)q, ny, nx, r, skipna, tx, cny, cnx, out);
    else
        hipLaunchKernelGGL(k_coarsen<float>, grid, dim3(kCscaleThreads), lds, ctx->stream, (const float*)q, ny, nx, r, skipna, tx, cny, cnx, out);
    XC_HIP(ctx, hipGetLastError());
    g.grid_x[slot] = (int32_t)grid.x; g.grid_y[slot] = (int32_t)grid.y; g.grid_z[slot] = (int32_t)grid.z;
    g.tile_x[slot] = tx; g.tile_y[slot] = kCscaleRows;
    return XC_OK;
}

}  // namespace

// what xc_contour_lengths_scales refuses of its ratios on a plane (`wrap`: periodic X), each message naming the ratio; the host form asks
// before it stages anything, the launcher before it launches anything
int cscale_check_ratios(xc_ctx* ctx, int64_t ny, int64_t nx, const int* ratios, int nratio, bool wrap)
{
    if (nratio < 1 || nratio > XC_CSCALE_MAXR) return fail(ctx, XC_EBADARG, "xc_contour_lengths_scales: 1 <= nratio <= XC_CSCALE_MAXR ratios");
    for (int k = 0; k < nratio; ++k) {
        const int r = ratios[k];
        const std::string w = "xc_contour_lengths_scales: ratio " + std::to_string(r);
        if (r < 1 || r > XC_CSCALE_MAXRATIO) return fail(ctx, XC_EBADARG, w + " is outside 1 .. XC_CSCALE_MAXRATIO");
        if (ny / r < 2) return fail(ctx, XC_EBADARG, w + " leaves fewer than 2 coarse rows");
        if (wrap && nx % r != 0)
            return fail(ctx, XC_EBADARG, w + " does not divide nx: the seam cell of a periodic plane would swallow the trimmed columns");
        if (!wrap && nx / r < 2) return fail(ctx, XC_EBADARG, w + " leaves fewer than 2 coarse columns");
    }
    return XC_OK;
}

int launch_coarsen(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx, int ratio, int skipna, double* out)
{
    ctx->last_cscale = xc_cscale_geometry{};
    if (!q || !out || nslab < 1 || ny < 1 || nx < 1) return fail(ctx, XC_EBADARG, "xc_coarsen: bad arguments");
    if (q_dtype != XC_F32 && q_dtype != XC_F64) return fail(ctx, XC_EBADARG, "xc_coarsen: q_dtype must be XC_F32 or XC_F64");
    if (nslab > 65535) return fail(ctx, XC_EBADARG, "xc_coarsen: at most 65535 slabs per call");
    if (ratio < 1 || ratio > XC_CSCALE_MAXRATIO || ny / ratio < 1 || nx / ratio < 1)
        return fail(ctx, XC_EBADARG, "xc_coarsen: ratio " + std::to_string(ratio) + " is outside 1 .. XC_CSCALE_MAXRATIO or leaves no coarse node");
    if ((ny / ratio + kCscaleRows - 1) / kCscaleRows > 65535) return fail(ctx, XC_EBADARG, "xc_coarsen: more than 262140 coarse rows");
    xc_cscale_geometry g = {};
    g.q_dtype = q_dtype; g.nratio = 1; g.block = kCscaleThreads; g.ratio[0] = ratio;
    XC_TRY(coarsen_into(ctx, g, 0, q, q_dtype, nslab, ny, nx, ratio, skipna ? 1 : 0, out));           // (ratio 1: the plane promoted)
    ctx->last_cscale = g;
    return XC_OK;
}

int launch_contour_lengths_scales(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                                  const double* ycoord, const double* xcoord, double period, double radius,
                                  const int* ratios, int nratio, int skipna, const double* contours, int N, int contours_per_slab,
                                  double* out_len, uint64_t* out_nseg)
{
    ctx->last_cscale = xc_cscale_geometry{};
    if (!q || !ycoord || !xcoord || !ratios || !contours || !out_len || nslab < 1 || ny < 1 || nx < 1 || N < 1)
        return fail(ctx, XC_EBADARG, "xc_contour_lengths_scales: bad arguments");
    if (q_dtype != XC_F32 && q_dtype != XC_F64) return fail(ctx, XC_EBADARG, "xc_contour_lengths_scales: q_dtype must be XC_F32 or XC_F64");
    if (!(radius >= 0.0)) return fail(ctx, XC_EBADARG, "xc_contour_lengths_scales: radius must be >= 0");
    if (nslab > 65535) return fail(ctx, XC_EBADARG, "xc_contour_lengths_scales: at most 65535 slabs per call");
    const bool wrap = period != 0.0;
    if (wrap && (!std::isfinite(period) || nx < 2))
        return fail(ctx, XC_EBADARG, "xc_contour_lengths_scales: period must be finite, and nx >= 2");
    XC_TRY(cscale_check_ratios(ctx, ny, nx, ratios, nratio, wrap));
    int rmin = 0;                                           // the smallest ratio above 1: the largest coarse plane
    for (int k = 0; k < nratio; ++k)
        if (ratios[k] > 1 && (rmin == 0 || ratios[k] < rmin)) rmin = ratios[k];
    if ((ny / 2 + kCscaleRows - 1) / kCscaleRows > 65535) return fail(ctx, XC_EBADARG, "xc_contour_lengths_scales: too many rows");
    double *plane = nullptr, *yc = nullptr, *xc = nullptr;
    if (rmin)
        XC_TRY(lay_out(ctx, &ctx->cscale_ws, &ctx->cscale_ws_bytes, [&](Carve c) {
            plane = c.take<double>((size_t)nslab * (ny / rmin) * (nx / rmin));
            yc = c.take<double>((size_t)(ny / rmin)); xc = c.take<double>((size_t)(nx / rmin));
            return c.at;
        }));
    xc_cscale_geometry g = {};                              // (handed to the context after the last launch: a call that fails leaves zeros)
    g.q_dtype = q_dtype; g.nratio = nratio; g.block = kCscaleThreads;
    const size_t per = (size_t)nslab * N;
    for (int k = 0; k < nratio; ++k) {
        const int r = ratios[k];
        double* len = out_len + k * per;
        uint64_t* nseg = out_nseg ? out_nseg + k * per : nullptr;
        g.ratio[k] = r;
        if (r == 1) {                                       // the plane and the coordinates themselves: nothing is copied
            XC_TRY(launch_contour_lengths(ctx, q, q_dtype, nslab, ny, nx, ycoord, xcoord, period, radius, contours, N, contours_per_slab, len, nseg));
            continue;
        }
        const int64_t cny = ny / r, cnx = nx / r;
        XC_TRY(coarsen_into(ctx, g, k, q, q_dtype, nslab, ny, nx, r, skipna ? 1 : 0, plane));
        hipLaunchKernelGGL(k_coarsen_coords, dim3((unsigned)((cny + cnx + 255) / 256)), dim3(256), 0, ctx->stream, ycoord, cny, xcoord, cnx, r, yc, xc);
        XC_HIP(ctx, hipGetLastError());
        XC_TRY(launch_contour_lengths(ctx, plane, XC_F64, nslab, cny, cnx, yc, xc, period, radius, contours, N, contours_per_slab, len, nseg));
    }
    ctx->last_cscale = g;
    return XC_OK;
}

}  // namespace xc

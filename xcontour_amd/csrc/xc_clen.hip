// K10 -- marching-squares contour lengths (gfx950).
//
// Replaces Contour2D.cal_contour_lengths (reference core.py:969-1014), its per-slab loop _contour_lengths (1437-1487) and
// utils.contour_length / __segment_length_* / __geodist (utils.py:565-761), which trace every contour with skimage's
// find_contours and walk the polylines.  What the method returns is the TOTAL length of each contour, and that total does not
// depend on how segments are joined into polylines: it is a sum over grid cells of a function of the cell's four corners and
// the level.  The rule (skimage find_contours(image, level) with its defaults, restated; build-defined, float64 throughout):
//   cell (r0, c0): corners ul = q[r0][c0], ur = q[r0][c0+1], ll = q[r0+1][c0], lr = q[r0+1][c0+1]; a NaN corner: no segment;
//   case = (ul > c) + 2 (ur > c) + 4 (ll > c) + 8 (lr > c); 0 and 15: no segment;
//   frac(a, b) = a == b ? 0 : (c - a) / (b - a);  edge points (row, column):
//     top (r0, c0 + frac(ul, ur))   bottom (r0+1, c0 + frac(ll, lr))   left (r0 + frac(ul, ll), c0)   right (r0 + frac(ur, lr), c0+1)
//   one segment joining the two crossed edges, except the saddles (fully_connected='low'): 6 -> (right, top), (left, bottom);
//   9 -> (top, left), (bottom, right).  A segment whose two points are equal is dropped (find_contours' assembly).
//   A point maps to coordinates like np.interp(x, arange(n), fdef); the segment length is the haversine of __geodist
//   (radius > 0, radian coordinates) or hypot (radius == 0); total == 0 -> NaN (utils.py:603-604), else total * radius.
//
// Mapping: the tile walk of xc_cell_walk.h (tiles of 32 x 252 cells, lanes along X, the right neighbour by DPP, the crossed levels
// from xc_levels.h).  Each crossed (cell, level) adds its 0..2 segment lengths (xc_clen_cell.h).
//
// Sums are deterministic (independent of arrival order, block geometry and slabs per launch): every length is cut once to
// 49 bits and added as two integer chunks to the limbs of a fixed-point accumulator per level (xc_binning.h det_split), on a
// window fixed before the pass by a bound on one segment (pi on the unit sphere, else the largest cell diagonal, k_clen_window);
// the blocks' limbs are carried and summed exactly and converted once (k_det3_reduce of xc_hist_det.hip).
// Capacity: a limb word takes at most one chunk (< 2^48) per segment; a block gives each of its `ncopy` LDS copies at most
// 32767 cells (launcher), i.e. at most 65534 chunks (< 2^64), and carries before it writes.  Levels that do not fit the LDS
// budget are split over gridDim.z (each group a full pass: any N is accepted).
//
// Periodic X (WRAP, xc_contour_lengths_periodic): the plane gains one cell column, index nx-1, whose left corners are node column
// nx-1 and whose right corners are node column 0: cL = nx-1, xL = fx[nx-1], xR = fx[0] + period (one float64 addition); everything
// else is the rule above, and the window constant takes that cell's width into its largest cell diagonal.  The result is, bit for
// bit, what the plain kernel returns for the plane with column 0 appended as column nx and fx[0] + period appended to the
// coordinates.  period: finite, non-zero, of the sign of fx[nx-1] - fx[0], |period| > |fx[nx-1] - fx[0]|; nx >= 2.  Y never wraps.
// Kernel k_ring_len; k_clen is the same code with the wrap compiled out.  k_clen_window takes the period at run time.
// Mapping: the seam rule of xc_cell_walk.h; what K10 adds is the coordinate of the lane whose column is nx: fx[0] + period, which the
// seam cell receives as its xR by the same DPP shift as its right corners.
#include "xc_capi.h"
#include <cmath>

namespace xc {
namespace {

#include "xc_binning.h"
#include "xc_levels.h"
#include "xc_cell_walk.h"
#include "xc_clen_cell.h"

constexpr size_t CLEN_LDS = 48 * 1024;      // LDS per block (several blocks per CU)

// The window constant of every slab from a bound on one segment: pi on the unit sphere, else the largest cell diagonal (period != 0:
// the seam cell, fx[nx-1] to fx[0] + period, among them).
__global__ __launch_bounds__(256)
void k_clen_window(const double* __restrict__ fy, int64_t ny, const double* __restrict__ fx, int64_t nx, int latlon,
                   int64_t nslab, int* __restrict__ c0, double period)
{
    const int w = det_c0_from_bound(clen_segment_bound(fy, ny, fx, nx, latlon, period));
    for (int64_t s = threadIdx.x; s < nslab; s += 256) c0[s] = w;
}

// The pass of k_clen (WRAP = false: the plane as it is) and k_ring_len (WRAP = true: periodic X); WRAP is a compile-time variant: the
// plain kernel pays nothing for it.  grid (bps, nslab, level groups of G).  LDS: levels [G + 2] (-inf, the group's levels, +inf), then per
// (level, copy) CLEN_WORDS limb words and one count word.
template <typename TQ, bool LATLON, bool WRAP>
__device__ __forceinline__
void clen_pass(const TQ* __restrict__ q, int64_t ny, int64_t nx, const double* __restrict__ fy, const double* __restrict__ fx,
            const double* __restrict__ contours, int N, int contours_per_slab, int G, const int* __restrict__ c0s,
            int64_t ntj, int64_t nti, int bps, int ncopy, unsigned long long* __restrict__ part_l, unsigned* __restrict__ part_c,
            double period)
{
    extern __shared__ double sm[];
    const int tid = threadIdx.x;
    const int64_t slab = blockIdx.y;
    const int g0 = blockIdx.z * G, ng = (N - g0 < G) ? N - g0 : G;
    double* s_cx = sm;                                                                    // [ng + 2]
    unsigned long long* s_acc = (unsigned long long*)(sm + ng + 2);                       // [ng][ncopy][CLEN_WORDS]
    unsigned* s_cnt = (unsigned*)(s_acc + (size_t)ng * ncopy * CLEN_WORDS);              // [ng][ncopy]
    const double* cs = contours + (contours_per_slab ? (size_t)slab * N : 0) + g0;
    for (int k = tid; k < ng * ncopy * CLEN_WORDS; k += WALK_TPB) s_acc[k] = 0ull;
    for (int k = tid; k < ng * ncopy; k += WALK_TPB) s_cnt[k] = 0u;
    const LevelSearch ls = load_levels<WALK_TPB>(cs, ng, s_cx);                            // (its barrier covers the sums cleared above)
    const int c0w = c0s[slab];
    const int cshift = __builtin_ctz((unsigned)ncopy), copy = tid & (ncopy - 1);
    double xL, xR;                                                                        // the coordinates of this lane's cell columns
    cell_walk<TQ, WRAP>(q + (size_t)slab * ny * nx, ny, nx, ntj, nti, bps, s_cx, ng, ls,
        [&](int64_t i, int64_t c) {                                                       // the lane of column nx: column 0, one period on
            if constexpr (WRAP) xL = i == nx ? __dadd_rn(fx[0], period) : fx[c]; else xL = fx[c];
            xR = lane_shift_keep<DPP_WAVE_SHL1>(xL, xL);
        },
        [&](int k, int64_t r, int64_t c, double ul, double ur, double ll, double lr) {
            cell_level<LATLON>(ul, ur, ll, lr, s_cx[k + 1], (double)r, (double)c, fy[r], fy[r + 1], xL, xR,
                               s_acc + ((size_t)((k << cshift) + copy)) * CLEN_WORDS, s_cnt + (k << cshift) + copy, c0w);
        });
    __syncthreads();
    // per level: the copies carried into canonical limbs and summed (clen_carry of xc_clen_cell.h), written as this block's partial
    const size_t pb = ((size_t)slab * bps + blockIdx.x);
    for (int k = tid; k < ng; k += WALK_TPB) {
        unsigned long long acc[kDetLimbsX] = {0ull, 0ull, 0ull, 0ull}, n = 0ull;
        unsigned flag = 0u;
        for (int cp = 0; cp < ncopy; ++cp)
            clen_carry(acc, n, flag, s_acc + ((size_t)((k << cshift) + cp)) * CLEN_WORDS, s_cnt[(k << cshift) + cp]);
        clen_carry_top(acc);
        const int kg = g0 + k;
#pragma unroll
        for (int l = 0; l < kDetLimbsX; ++l) part_l[(pb * kDetLimbsX + l) * N + kg] = acc[l];
        part_c[pb * N + kg] = ((unsigned)n & 0x0fffffffu) | flag;
    }
}

#define XC_CLEN_PARAMS const TQ* __restrict__ q, int64_t ny, int64_t nx, const double* __restrict__ fy, const double* __restrict__ fx, \
                        const double* __restrict__ contours, int N, int contours_per_slab, int G, const int* __restrict__ c0s,            \
                        int64_t ntj, int64_t nti, int bps, int ncopy, unsigned long long* __restrict__ part_l, unsigned* __restrict__ part_c
#define XC_CLEN_ARGS q, ny, nx, fy, fx, contours, N, contours_per_slab, G, c0s, ntj, nti, bps, ncopy, part_l, part_c

template <typename TQ, bool LATLON>
__global__ __launch_bounds__(WALK_TPB)
void k_clen(XC_CLEN_PARAMS)
{
    clen_pass<TQ, LATLON, false>(XC_CLEN_ARGS, 0.0);
}

// periodic X: the ring of nx cell columns
template <typename TQ, bool LATLON>
__global__ __launch_bounds__(WALK_TPB)
void k_ring_len(XC_CLEN_PARAMS, double period)
{
    clen_pass<TQ, LATLON, true>(XC_CLEN_ARGS, period);
}
#undef XC_CLEN_ARGS
#undef XC_CLEN_PARAMS

// total == 0 -> NaN (utils.py:603-604); else times the radius once (utils.py:606-607)
__global__ __launch_bounds__(256)
void k_clen_finish(double* __restrict__ out, int64_t n, double radius)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double t = out[i];
    out[i] = t == 0.0 ? dnan() : (radius > 0.0 ? __dmul_rn(t, radius) : t);
}

}  // namespace

int launch_clen_window(xc_ctx* ctx, const double* ycoord, int64_t ny, const double* xcoord, int64_t nx, double period, int latlon,
                       int64_t nslab, int* c0)
{
    hipLaunchKernelGGL(k_clen_window, dim3(1), dim3(256), 0, ctx->stream, ycoord, ny, xcoord, nx, latlon, nslab, c0, period);
    XC_HIP(ctx, hipGetLastError());
    return XC_OK;
}

int launch_contour_lengths(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                           const double* ycoord, const double* xcoord, double period, double radius,
                           const double* contours, int N, int contours_per_slab, double* out_len, uint64_t* out_nseg)
{
    if (!q || !ycoord || !xcoord || !contours || !out_len || nslab < 1 || ny < 1 || nx < 1 || N < 1)
        return fail(ctx, XC_EBADARG, "xc_contour_lengths: bad arguments");
    if (q_dtype != XC_F32 && q_dtype != XC_F64) return fail(ctx, XC_EBADARG, "xc_contour_lengths: q_dtype must be XC_F32 or XC_F64");
    if (!(radius >= 0.0)) return fail(ctx, XC_EBADARG, "xc_contour_lengths: radius must be >= 0");
    if (nslab > 65535) return fail(ctx, XC_EBADARG, "xc_contour_lengths: nslab too large");
    // period != 0: periodic X (the entry points have checked the period); the ring has nx cell columns
    const bool wrap = period != 0.0;
    if (wrap && (!std::isfinite(period) || nx < 2))
        return fail(ctx, XC_EBADARG, "xc_contour_lengths_periodic: period must be finite and non-zero, and nx >= 2");
    // LDS: level values 8 B + per copy CLEN_WORDS x 8 + 4 B.  As many copies (up to 8) as the budget takes for all levels;
    // one copy and groups of G levels past it
    auto lds_of = [](int g, int nc) { return (size_t)(g + 2) * 8 + (size_t)g * nc * (CLEN_WORDS * 8 + 4) + 16; };
    int ncopy = 8;
    while (ncopy > 1 && lds_of(N, ncopy) > CLEN_LDS) ncopy >>= 1;
    int G = N;
    if (lds_of(N, ncopy) > CLEN_LDS) G = (int)((CLEN_LDS - 32) / (8 + CLEN_WORDS * 8 + 4));
    const int ngroup = (N + G - 1) / G;
    const size_t lds = lds_of(G, ncopy);
    // blocks per slab: at most CLEN_COPY_CELLS cells per copy: a tile gives a copy WALK_RB * WALK_TPB / ncopy of them
    const WalkGeometry wg = walk_geometry(ny, nx, wrap, nslab, (int64_t)CLEN_COPY_CELLS * ncopy / (WALK_RB * WALK_TPB));
    const int64_t ntj = wg.ntj, nti = wg.nti, bps = wg.bps;
    {   // (xc_last_clen_geometry; the C entry points clear it when the call fails)
        xc_clen_geometry& g = ctx->last_clen;
        g = xc_clen_geometry{};
        g.q_dtype = q_dtype; g.latlon = radius > 0.0; g.N = N; g.ncopy = ncopy; g.G = G; g.ngroup = ngroup;
        g.ntile = wg.ntile; g.bps = (int32_t)bps; g.bps_rule = wg.bps_rule; g.nslab = nslab;
    }
    unsigned long long *part_l, *nseg; unsigned* part_c; int* c0;
    XC_TRY(lay_out(ctx, &ctx->scratch, &ctx->scratch_bytes, [&](Carve c) {
        part_l = c.take<unsigned long long>((size_t)nslab * bps * kDetLimbsX * N); part_c = c.take<unsigned>((size_t)nslab * bps * N);
        c0 = c.take<int>((size_t)nslab);
        nseg = out_nseg ? (unsigned long long*)out_nseg : c.take<unsigned long long>((size_t)nslab * N);
        return c.at;
    }));
    const int latlon = radius > 0.0;
    {
        const int rc = launch_clen_window(ctx, ycoord, ny, xcoord, nx, period, latlon, nslab, c0);
        if (rc != XC_OK) return rc;
    }
    if (bps > 0) {
        const dim3 grid((unsigned)bps, (unsigned)nslab, (unsigned)ngroup);
#define XC_CLEN_ARGS(TQ_) (const TQ_*)q, ny, nx, ycoord, xcoord, contours, N, contours_per_slab, G, c0, ntj, nti, (int)bps, ncopy, part_l, part_c
#define XC_CLEN(TQ_, LL_) do {                                                                                                        \
            if (wrap) hipLaunchKernelGGL((k_ring_len<TQ_, LL_>), grid, dim3(WALK_TPB), lds, ctx->stream, XC_CLEN_ARGS(TQ_), period);      \
            else hipLaunchKernelGGL((k_clen<TQ_, LL_>), grid, dim3(WALK_TPB), lds, ctx->stream, XC_CLEN_ARGS(TQ_));                       \
        } while (0)
        if (q_dtype == XC_F64) { if (latlon) XC_CLEN(double, true); else XC_CLEN(double, false); }
        else { if (latlon) XC_CLEN(float, true); else XC_CLEN(float, false); }
#undef XC_CLEN
#undef XC_CLEN_ARGS
        XC_HIP(ctx, hipGetLastError());
    }
    const int rc = launch_det3_reduce(ctx, nslab, (int)bps, 1, N, reinterpret_cast<const double*>(part_l), part_c, c0, out_len, nseg);
    if (rc != XC_OK) return rc;
    const int64_t n = nslab * (int64_t)N;
    hipLaunchKernelGGL(k_clen_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, out_len, n, latlon ? radius : 0.0);
    XC_HIP(ctx, hipGetLastError());
    return XC_OK;
}

}  // namespace xc

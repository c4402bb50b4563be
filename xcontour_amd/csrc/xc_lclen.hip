// K11 -- local (sliding-window) contour lengths (gfx950).
//
// Replaces the loop of the reference's tests/test_localLength.py: q.rolling(center=True).construct(stride=) and one
// find_contours call per window through apply_ufunc(vectorize=True).  Every window is a little plane of its own; its level is
// given, or the window's mean; its length is K10's total (xc_clen.hip) of that level on the window.  Build-defined:
//   windows: centres are the nodes (j, i), j = 0, sy, 2 sy, ... < ny, i = 0, sx, ... < nx; window (j, i) owns the node rows
//     [j - wy/2, j - wy/2 + wy - 1] (integer division) and likewise the columns, clipped to the plane; no wrap across the X seam;
//   level: levels[slab][wj][wi] when given; else the NaN-skipping mean in float64 in a fixed order: in every window row the
//     valid nodes left to right from 0.0 (a NaN node adds nothing and does not count), the row sums top to bottom, one IEEE
//     division by the valid count; fewer than min_periods valid nodes: NaN;
//   length: the rule of K10 on the window -- cell indices count from the window's first row and column, coordinates are the
//     window's slice of the plane's --, a total of 0 -> NaN; a NaN level: NaN length, 0 segments.
//
// Mapping: one workgroup per (window, slab), 256 threads (64 for windows of up to 2048 cells); all windows of all slabs in one
// launch.  Phase one, the level: one lane per window row walks its row left to right (the rows of neighbouring windows overlap:
// cache hits), thread 0 adds the row sums top to bottom.  Phase two, the length: the window's cells in strips of 16 cell rows
// x 64 cell columns, a wave per strip, lanes along X carrying the previous row; a NaN-free cell with mn <= c < mx calls the
// per-cell routine K10 uses (xc_clen_cell.h) into its wave's LDS accumulator (4 limbs, trash word, count word).
//
// Sums are K10's fixed-point sums on K10's window constant (k_clen_window over the whole plane's coordinates): a window's bits
// do not depend on the threads per block, the stride, the slabs per call or who else shares the launch.  Capacity: a wave's
// copy takes at most 31 strips = 31744 cells (<= 32767) before thread 0 carries the copies into its registers; it converts once.
//
// Periodic X (WRAP, xc_local_contour_lengths_periodic): windows are not clipped in X.  Window i owns the node columns
// [i - wx/2, i - wx/2 + wx - 1] taken modulo nx, in that (unwrapped) order; the coordinate of a column c outside [0, nx) is
// fx[c mod nx] + period or fx[c mod nx] - period (one float64 addition or subtraction; wx <= nx, so only one lap either way can
// occur).  The mean keeps its order, per row left to right in window order; length, NaN rules and the window constant are those
// of periodic K10 (xc_clen.hip).  The result is, bit for bit, the plain kernel's on the plane with h >= wx columns of the ring
// copied to either side, at the matching centres.  Y is clipped as before; nwx = ceil(nx / sx).  Column indices wrap per lane.
#include "xc_internal.h"
#include <cmath>

namespace xc {
namespace {

#include "xc_binning.h"
#include "xc_clen_cell.h"

constexpr int LCLEN_TPB = 256;              // threads per block of a large window
constexpr int LCLEN_WAVES = LCLEN_TPB / 64;
constexpr int LCLEN_SMALL = 2048;           // windows of up to this many cells take one wave
constexpr int LCLEN_RB = 16;                // cell rows per strip
constexpr int LCLEN_STRIPS = CLEN_COPY_CELLS / (64 * LCLEN_RB);   // strips of a wave between two carries

static_assert(LCLEN_STRIPS >= 1 && LCLEN_STRIPS * 64 * LCLEN_RB <= CLEN_COPY_CELLS, "a copy takes at most CLEN_COPY_CELLS cells before a carry");

// The body of k_lclen (WRAP = false: windows clipped in X) and k_ring_lclen (WRAP = true: periodic X); WRAP is a compile-time variant:
// the plain kernel pays nothing for it.  grid (windows per slab, nslab); blockDim.x 64 or LCLEN_TPB
template <typename TQ, bool LATLON, bool WRAP>
__device__ __forceinline__
void lclen_window(const TQ* __restrict__ q, int64_t ny, int64_t nx, const double* __restrict__ fy, const double* __restrict__ fx,
             int64_t wy, int64_t wx, int64_t sy, int64_t sx, int64_t nwx, int64_t nwin, int64_t min_periods,
             const double* __restrict__ levels, const int* __restrict__ c0s, double radius,
             double* __restrict__ out_len, double* __restrict__ out_level, unsigned long long* __restrict__ out_nseg, double period)
{
    __shared__ double s_row[LCLEN_TPB];
    __shared__ unsigned long long s_acc[LCLEN_WAVES][CLEN_WORDS];
    __shared__ unsigned s_cnt[LCLEN_WAVES];
    __shared__ unsigned long long s_valid;
    __shared__ double s_level;
    const int tid = threadIdx.x, ntd = blockDim.x, lane = tid & 63, wave = tid >> 6, nwave = ntd >> 6;
    const int64_t win = blockIdx.x, slab = blockIdx.y;
    const int64_t wj = win / nwx, wi = win - wj * nwx;
    const int64_t jr = wj * sy - wy / 2, ic = wi * sx - wx / 2;
    // the window's nodes: rows [r0, r1], columns [c0, c1] (WRAP: unwrapped columns, c0 in (-nx, nx) and c1 < 2 nx, not clipped)
    const int64_t r0 = jr > 0 ? jr : 0, r1 = jr + wy - 1 < ny - 1 ? jr + wy - 1 : ny - 1;
    const int64_t c0 = WRAP ? ic : (ic > 0 ? ic : 0), c1 = WRAP ? ic + wx - 1 : (ic + wx - 1 < nx - 1 ? ic + wx - 1 : nx - 1);
    const int64_t wh = r1 - r0 + 1, ww = c1 - c0 + 1;
    const TQ* qs = q + (size_t)slab * ny * nx;
    const size_t o = (size_t)slab * nwin + win;

    for (int k = tid; k < nwave * CLEN_WORDS; k += ntd) (&s_acc[0][0])[k] = 0ull;
    if (tid < nwave) s_cnt[tid] = 0u;
    if (tid == 0) s_valid = 0ull;
    double c;
    if (levels) {
        c = levels[o];
        __syncthreads();
    } else {
        double tot = 0.0;                                                                 // (thread 0)
        for (int64_t b = 0; b < wh; b += ntd) {
            __syncthreads();                                                              // s_row is free (and s_valid cleared)
            if (b + tid < wh) {
                const TQ* p = qs + (size_t)(r0 + b + tid) * nx + (WRAP ? 0 : c0);
                double s = 0.0;
                unsigned long long n = 0ull;
#pragma unroll 8
                for (int64_t k = 0; k < ww; ++k) {
                    double v;
                    if constexpr (WRAP) {                                                 // the node column on the ring
                        int64_t kc = c0 + k;
                        kc += kc < 0 ? nx : 0; kc -= kc >= nx ? nx : 0;
                        v = (double)p[kc];
                    } else {
                        v = (double)p[k];
                    }
                    const bool ok = v == v;
                    s = __dadd_rn(s, ok ? v : 0.0);                                       // (s is never -0.0: adding 0.0 adds nothing)
                    n += ok;
                }
                s_row[tid] = s;
                if (n) lds_add(&s_valid, n);
            }
            __syncthreads();
            if (tid == 0) {
                const int m = wh - b < ntd ? (int)(wh - b) : ntd;
                for (int i = 0; i < m; ++i) tot = __dadd_rn(tot, s_row[i]);
            }
        }
        if (tid == 0) {
            const unsigned long long n = s_valid;
            s_level = (long long)n < min_periods ? dnan() : __ddiv_rn(tot, (double)n);    // (0 / 0: NaN)
        }
        __syncthreads();
        c = s_level;
    }

    unsigned long long m[kDetLimbsX] = {0ull, 0ull, 0ull, 0ull}, nseg = 0ull;            // (thread 0) the window's carried limbs
    unsigned flag = 0u;
    const int c0w = c0s[0];
    const int64_t ch = wh - 1, cw = ww - 1;                                               // cell rows / columns
    if (c == c && ch > 0 && cw > 0) {                                                     // block-uniform
        const int64_t ncp = (cw + 63) / 64, nstrip = ((ch + LCLEN_RB - 1) / LCLEN_RB) * ncp;
        for (int64_t s0 = 0; s0 < nstrip; s0 += (int64_t)nwave * LCLEN_STRIPS) {
            for (int t = 0; t < LCLEN_STRIPS; ++t) {
                const int64_t s = s0 + (int64_t)t * nwave + wave;
                if (s >= nstrip) break;                                                   // wave-uniform
                const int64_t bj = s / ncp, cp = s - bj * ncp;
                const int64_t i = cp * 64 + lane;                                         // this lane's cell column in the window
                const bool cell = i < cw;                                                 // lanes without a cell load the last one's corners
                const int64_t ci = cell ? i : cw - 1;
                const int64_t j0 = bj * LCLEN_RB, j1 = j0 + LCLEN_RB < ch ? j0 + LCLEN_RB : ch;
                const double cL = (double)ci;
                double xL, xR;
                int64_t nL = c0 + ci, dR = 1;                                             // the left corner's column, the right one's offset
                if constexpr (WRAP) {
                    const int64_t uL = c0 + ci, uR = uL + 1;                              // unwrapped, in (-nx, 2 nx)
                    nL = uL < 0 ? uL + nx : (uL >= nx ? uL - nx : uL);
                    const int64_t nR = uR < 0 ? uR + nx : (uR >= nx ? uR - nx : uR);
                    xL = uL < 0 ? __dsub_rn(fx[nL], period) : (uL >= nx ? __dadd_rn(fx[nL], period) : fx[nL]);
                    xR = uR < 0 ? __dsub_rn(fx[nR], period) : (uR >= nx ? __dadd_rn(fx[nR], period) : fx[nR]);
                    dR = nR - nL;                                                         // 1, or 1 - nx across the seam
                } else {
                    xL = fx[nL]; xR = fx[nL + 1];
                }
                const TQ* p = qs + (size_t)(r0 + j0) * nx + nL;
                double ul = (double)p[0], ur = (double)p[dR];
                constexpr int B = 4;
                for (int64_t jb = j0; jb < j1; jb += B) {
                    TQ v[B][2];
#pragma unroll
                    for (int b = 0; b < B; ++b) {                                         // all loads of the batch in flight together
                        const int64_t jj = (jb + b < j1) ? jb + b : j1 - 1;
                        const TQ* pr = p + (size_t)(jj + 1 - j0) * nx;
                        v[b][0] = pr[0]; v[b][1] = pr[dR];
                    }
#pragma unroll
                    for (int b = 0; b < B; ++b) {
                        const int64_t r = jb + b;
                        if (r >= j1) break;                                               // wave-uniform
                        const double ll = (double)v[b][0], lr = (double)v[b][1];
                        const bool hasnan = (ul != ul) | (ur != ur) | (ll != ll) | (lr != lr);
                        if (cell && !hasnan) {
                            const double mn = fmin(fmin(ul, ur), fmin(ll, lr)), mx = fmax(fmax(ul, ur), fmax(ll, lr));
                            if (mn <= c && c < mx)
                                cell_level<LATLON>(ul, ur, ll, lr, c, (double)r, cL, fy[r0 + r], fy[r0 + r + 1], xL, xR,
                                                   s_acc[wave], &s_cnt[wave], c0w);
                        }
                        ul = ll; ur = lr;
                    }
                }
            }
            __syncthreads();
            // the waves' copies carried into thread 0's limbs (clen_carry of xc_clen_cell.h) and cleared for the next strips
            if (tid == 0) {
                for (int w = 0; w < nwave; ++w) {
                    clen_carry(m, nseg, flag, s_acc[w], s_cnt[w]);
#pragma unroll
                    for (int l = 0; l < CLEN_WORDS; ++l) s_acc[w][l] = 0ull;
                    s_cnt[w] = 0u;
                }
                clen_carry_top(m);
            }
            __syncthreads();
        }
    }
    if (tid == 0) {
        long long a[kDetLimbsX];
#pragma unroll
        for (int l = 0; l < kDetLimbsX; ++l) a[l] = (long long)m[l];
        const double t = flag ? dnan() : det_limbs_to_double(a, c0w);                     // (a non-finite length: NaN, as K10)
        // total == 0 -> NaN (utils.py:603-604); else times the radius once (utils.py:606-607)
        out_len[o] = t == 0.0 ? dnan() : (radius > 0.0 ? __dmul_rn(t, radius) : t);
        if (out_level) out_level[o] = c;
        if (out_nseg) out_nseg[o] = nseg;
    }
}

#define XC_LCLEN_PARAMS const TQ* __restrict__ q, int64_t ny, int64_t nx, const double* __restrict__ fy, const double* __restrict__ fx,       \
                        int64_t wy, int64_t wx, int64_t sy, int64_t sx, int64_t nwx, int64_t nwin, int64_t min_periods,                       \
                        const double* __restrict__ levels, const int* __restrict__ c0s, double radius, double* __restrict__ out_len,           \
                        double* __restrict__ out_level, unsigned long long* __restrict__ out_nseg
#define XC_LCLEN_ARGS q, ny, nx, fy, fx, wy, wx, sy, sx, nwx, nwin, min_periods, levels, c0s, radius, out_len, out_level, out_nseg

template <typename TQ, bool LATLON>
__global__ __launch_bounds__(LCLEN_TPB)
void k_lclen(XC_LCLEN_PARAMS)
{
    lclen_window<TQ, LATLON, false>(XC_LCLEN_ARGS, 0.0);
}

// periodic X: windows run on round the ring
template <typename TQ, bool LATLON>
__global__ __launch_bounds__(LCLEN_TPB)
void k_ring_lclen(XC_LCLEN_PARAMS, double period)
{
    lclen_window<TQ, LATLON, true>(XC_LCLEN_ARGS, period);
}
#undef XC_LCLEN_ARGS
#undef XC_LCLEN_PARAMS

}  // namespace

int launch_local_contour_lengths(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                                 const double* ycoord, const double* xcoord, double period, double radius,
                                 int64_t wy, int64_t wx, int64_t sy, int64_t sx, int64_t min_periods,
                                 const double* levels, double* out_len, double* out_level, uint64_t* out_nseg)
{
    if (!q || !ycoord || !xcoord || !out_len || nslab < 1 || ny < 1 || nx < 1)
        return fail(ctx, XC_EBADARG, "xc_local_contour_lengths: bad arguments");
    if (q_dtype != XC_F32 && q_dtype != XC_F64) return fail(ctx, XC_EBADARG, "xc_local_contour_lengths: q_dtype must be XC_F32 or XC_F64");
    if (!(radius >= 0.0)) return fail(ctx, XC_EBADARG, "xc_local_contour_lengths: radius must be >= 0");
    if (wy < 2 || wx < 2) return fail(ctx, XC_EBADARG, "xc_local_contour_lengths: the window must be at least 2 x 2 nodes");
    if (sy < 1 || sx < 1) return fail(ctx, XC_EBADARG, "xc_local_contour_lengths: strides must be >= 1");
    if (min_periods < 0) return fail(ctx, XC_EBADARG, "xc_local_contour_lengths: min_periods must be >= 0");
    if (nslab > 65535) return fail(ctx, XC_EBADARG, "xc_local_contour_lengths: nslab too large");
    // period != 0: periodic X (the entry points have checked the period)
    const bool wrap = period != 0.0;
    if (wrap && (!std::isfinite(period) || nx < 2))
        return fail(ctx, XC_EBADARG, "xc_local_contour_lengths_periodic: period must be finite and non-zero, and nx >= 2");
    if (wrap && wx > nx) return fail(ctx, XC_EBADARG, "xc_local_contour_lengths_periodic: the window must not be wider than the ring (wx <= nx)");
    const int64_t nwy = (ny + sy - 1) / sy, nwx = (nx + sx - 1) / sx;
    if (nwy > 0x7fffffff / nwx) return fail(ctx, XC_EBADARG, "xc_local_contour_lengths: too many windows per slab");
    const int64_t nwin = nwy * nwx;
    {
        const int rc = ensure_scratch(ctx, 256);
        if (rc != XC_OK) return rc;
    }
    int* c0 = (int*)ctx->scratch;
    const int latlon = radius > 0.0;
    {
        const int rc = launch_clen_window(ctx, ycoord, ny, xcoord, nx, period, latlon, 1, c0);
        if (rc != XC_OK) return rc;
    }
    // the cells of an unclipped window decide the threads per block (the sums do not depend on it)
    const int64_t hy = (wy < ny ? wy : ny) - 1, hx = (wx < nx ? wx : nx) - 1;                        // (periodic: wx <= nx, wx - 1 cells)
    const int tpb = hy * hx <= LCLEN_SMALL ? 64 : LCLEN_TPB;
    const dim3 grid((unsigned)nwin, (unsigned)nslab);
#define XC_LCLEN_ARGS(TQ_) (const TQ_*)q, ny, nx, ycoord, xcoord, wy, wx, sy, sx, nwx, nwin, min_periods, levels, c0, latlon ? radius : 0.0, \
                      out_len, out_level, (unsigned long long*)out_nseg
#define XC_LCLEN(TQ_, LL_) do {                                                                                              \
        if (wrap) hipLaunchKernelGGL((k_ring_lclen<TQ_, LL_>), grid, dim3(tpb), 0, ctx->stream, XC_LCLEN_ARGS(TQ_), period);     \
        else hipLaunchKernelGGL((k_lclen<TQ_, LL_>), grid, dim3(tpb), 0, ctx->stream, XC_LCLEN_ARGS(TQ_));                       \
    } while (0)
    if (q_dtype == XC_F64) { if (latlon) XC_LCLEN(double, true); else XC_LCLEN(double, false); }
    else { if (latlon) XC_LCLEN(float, true); else XC_LCLEN(float, false); }
#undef XC_LCLEN
#undef XC_LCLEN_ARGS
    XC_HIP(ctx, hipGetLastError());
    return XC_OK;
}

}  // namespace xc

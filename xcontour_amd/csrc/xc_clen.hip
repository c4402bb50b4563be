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
// Mapping (like K9 at stride 1): tiles of 32 cell rows x 252 cell columns, 4 waves of 63 cells; lanes along X; every lane
// loads ONE corner per row and takes its right neighbour from the next lane (DPP), carrying the previous row, so every tracer
// row is read from HBM once per tile.  A NaN-free cell crosses exactly the levels with mn <= c < mx: the index range between
// the two lower bounds (xc_levels.h).  Each crossed (cell, level) adds its 0..2 segment lengths.
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
// Kernels k_ring_len / k_ring_window; k_clen and k_clen_window are the same code with the wrap compiled out.
// Mapping: tiles cover nx cell columns, and the lane whose column is nx -- the right neighbour of the seam cell's lane, a cell lane
// or the wave's halo lane 63 -- loads node column 0 and carries fx[0] + period, so the seam cell takes its right corner by the
// same DPP shift as every other cell.
#include "xc_internal.h"
#include <cmath>

namespace xc {
namespace {

#include "xc_binning.h"
#include "xc_levels.h"
#include "xc_clen_cell.h"

constexpr int CLEN_RB = 32;                 // cell rows per tile
constexpr int CLEN_TPB = 256;               // threads per block
constexpr int CLEN_W = 252;                 // cell columns per tile: 4 waves x 63 cells
constexpr size_t CLEN_LDS = 48 * 1024;      // LDS per block (several blocks per CU)

// The window constant of every slab from a bound on one segment: pi on the unit sphere, else the largest cell diagonal (WRAP: the
// seam cell, fx[nx-1] to fx[0] + period, among them).
template <bool WRAP>
__device__ __forceinline__ void clen_window(const double* __restrict__ fy, int64_t ny, const double* __restrict__ fx, int64_t nx, int latlon,
                                            int64_t nslab, int* __restrict__ c0, double period)
{
    const int tid = threadIdx.x;
    double my = 0.0, mx = 0.0;
    for (int64_t i = tid; i + 1 < ny; i += 256) my = fmax(my, fabs(fy[i + 1] - fy[i]));
    for (int64_t i = tid; i + 1 < nx; i += 256) mx = fmax(mx, fabs(fx[i + 1] - fx[i]));
    if constexpr (WRAP) { if (tid == 0) mx = fmax(mx, fabs(__dadd_rn(fx[0], period) - fx[nx - 1])); }
    for (int o = 32; o > 0; o >>= 1) { my = fmax(my, __shfl_xor(my, o)); mx = fmax(mx, __shfl_xor(mx, o)); }
    __shared__ double s_m[2][4];
    if ((tid & 63) == 0) { s_m[0][tid >> 6] = my; s_m[1][tid >> 6] = mx; }
    __syncthreads();
    my = fmax(fmax(s_m[0][0], s_m[0][1]), fmax(s_m[0][2], s_m[0][3]));
    mx = fmax(fmax(s_m[1][0], s_m[1][1]), fmax(s_m[1][2], s_m[1][3]));
    const double bound = latlon ? 3.2 : 1.0000001 * hypot(mx, my);
    const int w = det_c0_from_bound(bound);
    for (int64_t s = tid; s < nslab; s += 256) c0[s] = w;
}

__global__ __launch_bounds__(256)
void k_clen_window(const double* __restrict__ fy, int64_t ny, const double* __restrict__ fx, int64_t nx, int latlon,
                   int64_t nslab, int* __restrict__ c0)
{
    clen_window<false>(fy, ny, fx, nx, latlon, nslab, c0, 0.0);
}

__global__ __launch_bounds__(256)
void k_ring_window(const double* __restrict__ fy, int64_t ny, const double* __restrict__ fx, int64_t nx, int latlon,
                   int64_t nslab, int* __restrict__ c0, double period)
{
    clen_window<true>(fy, ny, fx, nx, latlon, nslab, c0, period);
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
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    for (int k = tid; k < ng; k += CLEN_TPB) s_cx[k + 1] = cs[k];
    if (tid == 0) { s_cx[0] = -inf; s_cx[ng + 1] = inf; }
    for (int k = tid; k < ng * ncopy * CLEN_WORDS; k += CLEN_TPB) s_acc[k] = 0ull;
    for (int k = tid; k < ng * ncopy; k += CLEN_TPB) s_cnt[k] = 0u;
    __syncthreads();
    const int c0w = c0s[slab];
    const double c_first = s_cx[1];
    double inv_step = (ng > 1) ? (double)(ng - 1) / (s_cx[ng] - c_first) : 0.0;
    if (!(inv_step > 0.0 && inv_step < inf)) inv_step = 0.0;
    double zlo = 0.5;
    {   // equally spaced levels?  (block-uniform answer, as in K9) -- and how far the levels sit from their ideal positions
        int ok = inv_step > 0.0;
        double dev = 0.0;
        for (int k = tid; k < ng && ok; k += CLEN_TPB) {
            const double d = fabs((s_cx[k + 1] - c_first) * inv_step - (double)k);
            ok = d < 0.01; dev = fmax(dev, d);
        }
        if (!__syncthreads_and(ok)) inv_step = 0.0;
        for (int o = 32; o > 0; o >>= 1) dev = fmax(dev, __shfl_xor(dev, o));
        __shared__ double s_dev[CLEN_TPB / 64];
        if ((tid & 63) == 0) s_dev[tid >> 6] = dev;
        __syncthreads();
        dev = s_dev[0];
        for (int w = 1; w < CLEN_TPB / 64; ++w) dev = fmax(dev, s_dev[w]);
        zlo = 2.0 * dev + 1e-9;
    }
    const int cshift = __builtin_ctz((unsigned)ncopy), copy = tid & (ncopy - 1);
    const TQ* qs = q + (size_t)slab * ny * nx;
    const int64_t ncx = WRAP ? nx : nx - 1, ncy = ny - 1;
    const int lane = tid & 63, wave = tid >> 6;

    for (int64_t tile = blockIdx.x; tile < ntj * nti; tile += bps) {
        const int64_t tj = tile / nti, ti = tile - tj * nti;
        const int64_t i = ti * CLEN_W + wave * 63 + lane;                                // this lane's cell column
        const int64_t j0 = tj * CLEN_RB, j1 = (j0 + CLEN_RB < ncy) ? j0 + CLEN_RB : ncy;
        const bool cell = lane < 63 && i < ncx;                                          // lanes without a cell still load and shift
        int64_t c = i < nx - 1 ? i : nx - 1;                                             // corner column loaded by this lane
        double xL;
        if constexpr (WRAP) {                                                            // column nx is column 0, one period on
            if (i == nx) c = 0;
            xL = i == nx ? __dadd_rn(fx[0], period) : fx[c];
        } else {
            xL = fx[c];
        }
        const double xR = lane_shift_keep<DPP_WAVE_SHL1>(xL, xL);
        const double cL = (double)c;
        double ul = (double)qs[(size_t)j0 * nx + c];
        double ur = lane_shift_keep<DPP_WAVE_SHL1>(ul, ul);
        constexpr int B = 4;
        for (int64_t jb = j0; jb < j1; jb += B) {
            TQ v[B];
#pragma unroll
            for (int b = 0; b < B; ++b) {                                                // all loads of the batch in flight together
                const int64_t jj = (jb + b < j1) ? jb + b : j1 - 1;
                v[b] = qs[(size_t)(jj + 1) * nx + c];
            }
#pragma unroll
            for (int b = 0; b < B; ++b) {
                const int64_t r = jb + b;
                if (r >= j1) break;                                                      // wave-uniform
                const double ll = (double)v[b], lr = lane_shift_keep<DPP_WAVE_SHL1>(ll, ll);
                const bool hasnan = (ul != ul) | (ur != ur) | (ll != ll) | (lr != lr);
                if (cell && !hasnan) {
                    const double mn = fmin(fmin(ul, ur), fmin(ll, lr)), mx = fmax(fmax(ul, ur), fmax(ll, lr));
                    int klo, khi;
                    if (inv_step > 0.0) {
                        klo = count_below_uniform(s_cx, ng, mn, c_first, inv_step, zlo);
                        khi = count_below_uniform(s_cx, ng, mx, c_first, inv_step, zlo);
                    } else {
                        klo = count_below(s_cx, ng, mn);
                        khi = count_below(s_cx, ng, mx);
                    }
                    if (khi > klo) {
                        const double yT = fy[r], yB = fy[r + 1];
                        for (int k = klo; k < khi; ++k)
                            cell_level<LATLON>(ul, ur, ll, lr, s_cx[k + 1], (double)r, cL, yT, yB, xL, xR,
                                               s_acc + ((size_t)((k << cshift) + copy)) * CLEN_WORDS, s_cnt + (k << cshift) + copy, c0w);
                    }
                }
                ul = ll; ur = lr;
            }
        }
    }
    __syncthreads();
    // per level: the copies carried into canonical limbs (words 1..3 < 2^48 plus carries, word 0 the rest) and summed, carried
    // once more, written as this block's partial; the trash word is dropped
    const size_t pb = ((size_t)slab * bps + blockIdx.x);
    for (int k = tid; k < ng; k += CLEN_TPB) {
        unsigned long long acc[kDetLimbsX] = {0ull, 0ull, 0ull, 0ull};
        unsigned n = 0u;
        for (int cp = 0; cp < ncopy; ++cp) {
            const unsigned long long* w = s_acc + ((size_t)((k << cshift) + cp)) * CLEN_WORDS;
#pragma unroll
            for (int l = 0; l < kDetLimbsX; ++l) {
                const unsigned long long x = w[l];
                acc[l] += x & 0xffffffffffffull;
                if (l > 0) acc[l - 1] += x >> kDetLimbBits; else acc[0] += x & ~0xffffffffffffull;
            }
            const unsigned m = s_cnt[(k << cshift) + cp];
            n = ((n & 0x0fffffffu) + (m & 0x0fffffffu)) | ((n | m) & CLEN_FLAG);
        }
#pragma unroll
        for (int l = kDetLimbsX - 1; l > 0; --l) { acc[l - 1] += acc[l] >> kDetLimbBits; acc[l] &= 0xffffffffffffull; }
        const int kg = g0 + k;
#pragma unroll
        for (int l = 0; l < kDetLimbsX; ++l) part_l[(pb * kDetLimbsX + l) * N + kg] = acc[l];
        part_c[pb * N + kg] = n;
    }
}

#define XC_CLEN_PARAMS const TQ* __restrict__ q, int64_t ny, int64_t nx, const double* __restrict__ fy, const double* __restrict__ fx, \
                        const double* __restrict__ contours, int N, int contours_per_slab, int G, const int* __restrict__ c0s,            \
                        int64_t ntj, int64_t nti, int bps, int ncopy, unsigned long long* __restrict__ part_l, unsigned* __restrict__ part_c
#define XC_CLEN_ARGS q, ny, nx, fy, fx, contours, N, contours_per_slab, G, c0s, ntj, nti, bps, ncopy, part_l, part_c

template <typename TQ, bool LATLON>
__global__ __launch_bounds__(CLEN_TPB)
void k_clen(XC_CLEN_PARAMS)
{
    clen_pass<TQ, LATLON, false>(XC_CLEN_ARGS, 0.0);
}

// periodic X: the ring of nx cell columns
template <typename TQ, bool LATLON>
__global__ __launch_bounds__(CLEN_TPB)
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
    out[i] = t == 0.0 ? __longlong_as_double(0x7ff8000000000000LL) : (radius > 0.0 ? __dmul_rn(t, radius) : t);
}

}  // namespace

int launch_clen_window(xc_ctx* ctx, const double* ycoord, int64_t ny, const double* xcoord, int64_t nx, double period, int latlon,
                       int64_t nslab, int* c0)
{
    if (period != 0.0)
        hipLaunchKernelGGL(k_ring_window, dim3(1), dim3(256), 0, ctx->stream, ycoord, ny, xcoord, nx, latlon, nslab, c0, period);
    else
        hipLaunchKernelGGL(k_clen_window, dim3(1), dim3(256), 0, ctx->stream, ycoord, ny, xcoord, nx, latlon, nslab, c0);
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
    const int64_t ncx = wrap ? nx : nx - 1, ncy = ny - 1;
    const int64_t ntj = ncy > 0 ? (ncy + CLEN_RB - 1) / CLEN_RB : 0, nti = ncx > 0 ? (ncx + CLEN_W - 1) / CLEN_W : 0;
    const int64_t ntile = ntj * nti;
    // blocks per slab: ~2048 blocks per launch, and at most CLEN_COPY_CELLS cells per copy: a tile gives a copy
    // CLEN_RB * CLEN_TPB / ncopy of them
    const int64_t max_tiles = (int64_t)CLEN_COPY_CELLS * ncopy / (CLEN_RB * CLEN_TPB);
    int64_t bps = 0;
    int bps_rule = 0;
    if (ntile > 0) {
        bps = 2048 / nslab; bps_rule = XC_CLEN_BPS_SHARE;
        if (bps < 8) { bps = 8; bps_rule = XC_CLEN_BPS_FLOOR; }
        const int64_t need = (ntile + max_tiles - 1) / max_tiles;
        if (bps < need) { bps = need; bps_rule = XC_CLEN_BPS_CAPACITY; }
        if (bps > ntile) { bps = ntile; bps_rule = XC_CLEN_BPS_NTILE; }
    }
    {   // (xc_last_clen_geometry; the C entry points clear it when the call fails)
        xc_clen_geometry& g = ctx->last_clen;
        g = xc_clen_geometry{};
        g.q_dtype = q_dtype; g.latlon = radius > 0.0; g.N = N; g.ncopy = ncopy; g.G = G; g.ngroup = ngroup;
        g.ntile = ntile; g.bps = (int32_t)bps; g.bps_rule = bps_rule; g.nslab = nslab;
    }
    const size_t al = 256;
    auto up = [&](size_t b) { return (b + al - 1) & ~(al - 1); };
    const size_t pl = up((size_t)nslab * bps * kDetLimbsX * N * 8), pc = up((size_t)nslab * bps * N * 4);
    const size_t pw = up((size_t)nslab * 4), pn = out_nseg ? 0 : up((size_t)nslab * N * 8);
    {
        const int rc = ensure_scratch(ctx, pl + pc + pw + pn + al);
        if (rc != XC_OK) return rc;
    }
    char* sc = (char*)ctx->scratch;
    unsigned long long* part_l = (unsigned long long*)sc;
    unsigned* part_c = (unsigned*)(sc + pl);
    int* c0 = (int*)(sc + pl + pc);
    unsigned long long* nseg = out_nseg ? (unsigned long long*)out_nseg : (unsigned long long*)(sc + pl + pc + pw);
    const int latlon = radius > 0.0;
    {
        const int rc = launch_clen_window(ctx, ycoord, ny, xcoord, nx, period, latlon, nslab, c0);
        if (rc != XC_OK) return rc;
    }
    if (bps > 0) {
        const dim3 grid((unsigned)bps, (unsigned)nslab, (unsigned)ngroup);
#define XC_CLEN_ARGS(TQ_) (const TQ_*)q, ny, nx, ycoord, xcoord, contours, N, contours_per_slab, G, c0, ntj, nti, (int)bps, ncopy, part_l, part_c
#define XC_CLEN(TQ_, LL_) do {                                                                                                        \
            if (wrap) hipLaunchKernelGGL((k_ring_len<TQ_, LL_>), grid, dim3(CLEN_TPB), lds, ctx->stream, XC_CLEN_ARGS(TQ_), period);      \
            else hipLaunchKernelGGL((k_clen<TQ_, LL_>), grid, dim3(CLEN_TPB), lds, ctx->stream, XC_CLEN_ARGS(TQ_));                       \
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

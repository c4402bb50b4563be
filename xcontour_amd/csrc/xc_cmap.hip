// K25  contour vectors back on the plane (xc_contour_map): out_v[s][r][c] = np.interp(q[s][r][c], X, F_v), the reference's
// _interp1d (core.py:1405-1434) with x = the tracer of every node, xf = the contour levels, yf = a per-contour vector.  gfx950 only.
//
// One bandwidth-bound pass: 8 (4) bytes read and 8 nv (4 nv) bytes written per cell, nothing else.  A workgroup stages the slab's
// levels and its nv value vectors into LDS once -- in ASCENDING order whatever the direction of the levels, so that the look-ups below
// run interp_locate / interp_eval (xc_finalize.h) with rev = 0 -- and then walks tiles of XC_CMAP_TILE cells of that slab, bps tiles apart.
// A thread takes four consecutive cells of a tile: one (float32) or two (float64) 16-byte non-temporal loads, one bracket search
// per cell for all nv vectors, 16-byte stores.  The first cell of a slab need not lie on the 16-byte grid (an odd ny * nx): the
// `head` cells in front of the first 16-byte boundary of the tracer and the last ncell mod 4 cells take a scalar path, and an output
// whose address is off the grid where the tracer's is on it is stored cell by cell.
#include "xc_internal.h"

namespace xc {

namespace {

#include "xc_binning.h"
#include "xc_finalize.h"

constexpr int kCmapThreads = 256;
constexpr int kCmapCells   = 4;          // cells per thread and tile
constexpr int kCmapMinTiles = 4;         // tiles a workgroup walks at least (where the slab has them): the staging is paid once for them
constexpr int kCmapBlocks  = 2048;       // workgroups of a launch, about: eight per CU
static_assert(kCmapThreads * kCmapCells == XC_CMAP_TILE, "XC_CMAP_TILE is the cells one workgroup takes per step");

struct CmapArgs {
    const void* q; int64_t ncell;
    const double* xp; int64_t xp_stride;              // 0: one set of levels for all slabs
    int N, nv;
    const double* fp[XC_CMAP_MAXV]; int64_t fp_stride[XC_CMAP_MAXV];
    void* out[XC_CMAP_MAXV];
};

// interp_locate's bracket for ascending, strictly monotonic, finite levels sx[0 .. n-1] (x0 = sx[0], xn = sx[n-1]), found from the
// uniform guess (x - x0) (n - 1) / (xn - x0): the guess is tested against the explicit levels, then its two neighbours, and what is
// further off goes to interp_locate itself.  A hit sx[k] <= x < sx[k+1] IS the largest index with sx[j] <= x; the guess only saves time.
__device__ __forceinline__ int cmap_locate(double x, const double* __restrict__ sx, int n, double x0, double xn, double inv)
{
    if (x != x) return -3;
    if (x > xn) return -2;
    if (x < x0) return -1;
    const double t = __dmul_rn(__dsub_rn(x, x0), inv);                  // (inv = 0 or NaN for a span that overflows: k = 0)
    const int k = t >= (double)(n - 2) ? n - 2 : (t > 0.0 ? (int)t : 0);
    const double lo = sx[k], hi = sx[k + 1];
    if ((x >= lo) & (x < hi)) return k;
    if (x < lo) { if (k > 0 && x >= sx[k - 1]) return k - 1; }
    else if (k + 2 <= n - 1 && x < sx[k + 2]) return k + 1;
    return interp_locate(x, sx, n, 0);
}

template <typename TO> __device__ __forceinline__ void cmap_store4(TO* o, const double (&r)[4]);
template <> __device__ __forceinline__ void cmap_store4<double>(double* o, const double (&r)[4])
{
    if (((uintptr_t)o & 15) == 0) {
        *reinterpret_cast<double2*>(o) = make_double2(r[0], r[1]);
        *reinterpret_cast<double2*>(o + 2) = make_double2(r[2], r[3]);
    } else { o[0] = r[0]; o[1] = r[1]; o[2] = r[2]; o[3] = r[3]; }
}
template <> __device__ __forceinline__ void cmap_store4<float>(float* o, const double (&r)[4])
{
    if (((uintptr_t)o & 15) == 0) *reinterpret_cast<float4*>(o) = make_float4((float)r[0], (float)r[1], (float)r[2], (float)r[3]);
    else { o[0] = (float)r[0]; o[1] = (float)r[1]; o[2] = (float)r[2]; o[3] = (float)r[3]; }
}

template <typename TQ, typename TO>
__global__ __launch_bounds__(kCmapThreads)
void k_cmap(const CmapArgs a)
{
    extern __shared__ double s_cmap[];
    const int tid = threadIdx.x, N = a.N, nv = a.nv;
    const int64_t slab = blockIdx.y, ncell = a.ncell;
    double* sx = s_cmap;                 // [N] ascending
    double* sf = s_cmap + N;             // [nv][N] in the order of sx
    const double* xs = a.xp + slab * a.xp_stride;
    const double xfirst = xs[0], xlast = xs[N - 1];
    const int rev = !(xfirst < xlast);                                   // core.py:1426-1430
    const bool allnan = xfirst != xfirst || xlast != xlast;              // an all-NaN tracer's levels: NaN everywhere
    for (int i = tid; i < N; i += kCmapThreads) sx[i] = xs[rev ? N - 1 - i : i];
    for (int v = 0; v < nv; ++v) {
        const double* fs = a.fp[v] + slab * a.fp_stride[v];
        for (int i = tid; i < N; i += kCmapThreads) sf[(size_t)v * N + i] = fs[rev ? N - 1 - i : i];
    }
    __syncthreads();
    const double x0 = rev ? xlast : xfirst, xn = rev ? xfirst : xlast;
    const double inv = __ddiv_rn((double)(N - 1), __dsub_rn(xn, x0));

    const TQ* qs = reinterpret_cast<const TQ*>(a.q) + slab * ncell;
    // cells in front of the tracer's first 16-byte boundary
    int64_t head = (int64_t)(((16 - ((uintptr_t)qs & 15)) & 15) / sizeof(TQ));
    if (head > ncell) head = ncell;
    const int64_t ntile = (ncell - head + XC_CMAP_TILE - 1) / XC_CMAP_TILE;

    auto eval = [&](double x, int j, int v) { return allnan ? dnan() : interp_eval(x, j, sx, sf + (size_t)v * N, N, 0); };
    auto one = [&](int64_t c) {
        const double x = (double)qs[c];
        const int j = cmap_locate(x, sx, N, x0, xn, inv);
        for (int v = 0; v < nv; ++v) reinterpret_cast<TO*>(a.out[v])[slab * ncell + c] = (TO)eval(x, j, v);
    };
    if (blockIdx.x == 0 && tid < head) one(tid);

    const int64_t bps = gridDim.x;
    auto group = [&](int64_t t) { return head + t * XC_CMAP_TILE + (int64_t)kCmapCells * tid; };
    int64_t t = blockIdx.x;
    double x[kCmapCells] = {0.0, 0.0, 0.0, 0.0};
    if (t < ntile && group(t) + kCmapCells <= ncell) RowLoadNT<TQ, kCmapCells>::ld(qs + group(t), x);
    for (; t < ntile; t += bps) {
        const int64_t c0 = group(t), cn = group(t + bps);
        const bool full = c0 + kCmapCells <= ncell, fulln = t + bps < ntile && cn + kCmapCells <= ncell;
        double xnext[kCmapCells] = {0.0, 0.0, 0.0, 0.0};
        if (fulln) RowLoadNT<TQ, kCmapCells>::ld(qs + cn, xnext);      // the next tile's cells are in flight under this one's look-ups
        if (full) {
            int j[kCmapCells];
#pragma unroll
            for (int e = 0; e < kCmapCells; ++e) j[e] = cmap_locate(x[e], sx, N, x0, xn, inv);
            for (int v = 0; v < nv; ++v) {
                double r[kCmapCells];
#pragma unroll
                for (int e = 0; e < kCmapCells; ++e) r[e] = eval(x[e], j[e], v);
                cmap_store4<TO>(reinterpret_cast<TO*>(a.out[v]) + slab * ncell + c0, r);
            }
        } else {
            for (int64_t c = c0; c < ncell; ++c) one(c);                // the last ncell mod 4 cells of the slab
        }
#pragma unroll
        for (int e = 0; e < kCmapCells; ++e) x[e] = xnext[e];
    }
}

}  // namespace

// ------------------------------------------------------------------------------------ launcher
int launch_contour_map(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx,
                       const double* xp, int N, int xp_per_slab, int nv, const double* const* fp, const int* fp_per_slab,
                       void* const* out, int out_dtype)
{
    if (!q || !xp || !fp || !fp_per_slab || !out || nslab < 1 || ny < 1 || nx < 1)
        return fail(ctx, XC_EBADARG, "xc_contour_map: bad arguments");
    if (N < 2) return fail(ctx, XC_EBADARG, "xc_contour_map: need at least two levels");
    if (nv < 1 || nv > XC_CMAP_MAXV) return fail(ctx, XC_EBADARG, "xc_contour_map: 1 <= nv <= XC_CMAP_MAXV value vectors");
    for (int v = 0; v < nv; ++v)
        if (!fp[v] || !out[v]) return fail(ctx, XC_EBADARG, "xc_contour_map: bad arguments");
    if ((q_dtype != XC_F32 && q_dtype != XC_F64) || (out_dtype != XC_F32 && out_dtype != XC_F64))
        return fail(ctx, XC_EBADARG, "xc_contour_map: q_dtype and out_dtype must be XC_F32 or XC_F64");
    if (nslab > 65535) return fail(ctx, XC_EBADARG, "xc_contour_map: at most 65535 slabs per call");
    if ((int64_t)(nv + 1) * N > XC_CMAP_MAX_LDS_DOUBLES)
        return fail(ctx, XC_EBADARG, "xc_contour_map: (nv + 1) * N must not exceed XC_CMAP_MAX_LDS_DOUBLES (the levels and the vectors live in LDS)");
    CmapArgs a = {};
    a.q = q; a.ncell = ny * nx; a.xp = xp; a.xp_stride = xp_per_slab ? N : 0; a.N = N; a.nv = nv;
    for (int v = 0; v < nv; ++v) { a.fp[v] = fp[v]; a.fp_stride[v] = fp_per_slab[v] ? N : 0; a.out[v] = out[v]; }
    // workgroups per slab: each walks kCmapMinTiles tiles or more, and the launch has about kCmapBlocks of them
    const int64_t ntile = (a.ncell + XC_CMAP_TILE - 1) / XC_CMAP_TILE + 1;           // (+ 1: the head may push a tile over)
    int64_t bps = (ntile + kCmapMinTiles - 1) / kCmapMinTiles;
    const int64_t cap = kCmapBlocks / nslab > 1 ? kCmapBlocks / nslab : 1;
    if (bps > cap) bps = cap;
    const dim3 grid((unsigned)bps, (unsigned)nslab), block(kCmapThreads);
    const size_t lds = (size_t)(nv + 1) * N * sizeof(double);
    if (q_dtype == XC_F64 && out_dtype == XC_F64) hipLaunchKernelGGL((k_cmap<double, double>), grid, block, lds, ctx->stream, a);
    else if (q_dtype == XC_F64) hipLaunchKernelGGL((k_cmap<double, float>), grid, block, lds, ctx->stream, a);
    else if (out_dtype == XC_F64) hipLaunchKernelGGL((k_cmap<float, double>), grid, block, lds, ctx->stream, a);
    else hipLaunchKernelGGL((k_cmap<float, float>), grid, block, lds, ctx->stream, a);
    XC_HIP(ctx, hipGetLastError());
    return XC_OK;
}

}  // namespace xc

// K15 -- integrals of a field along contours (gfx950).
//
// What a user of a contour trace wants after its length (K10): a field F integrated along the contour, I = sum over the contour's segments
// of the trapezoid rule, and its mean I / L.  (The reference's cal_contour_mean is the area-derivative estimate, smeared over a bin; it does
// not touch the traced contour.)  Like the length, the integral does not depend on how segments are joined: it is a sum over grid cells of
// a function of the cell's four corners, the integrand's four corners and the level.  The rule (build-defined, float64 throughout):
//   segments: exactly K10's (the header of xc_clen.hip): the same cells -- the seam cell under a period among them --, crossed levels, cases,
//     saddle pairing, end points in index space, their mapping to coordinates, the same length len (seg_len); coincident end points: dropped;
//   F(u), u an end point on the grid edge between two nodes: the integrand mapped as the coordinates are, interp_at(point index, first node
//     index, F[first node], F[second node]): the node's value on a node (the other node does not enter), else (F1 - F0) (x - i0) + F0, every
//     operation correctly rounded.  The seam cell: the second node of its top and bottom edges is column 0 of the same row, its left point
//     uses column nx-1, its right point column 0;
//   term = (0.5 (F(u) + F(v))) len: one add, one multiply by 0.5, one multiply by len;
//   a segment with a NaN F(u) or F(v) is skipped: it adds to no output and is not counted;
//   per (slab, level) two fixed-point channels -- 0: len, 1: term, over the counted segments -- and the count;
//   length = channel 0, integral = channel 1, each times the radius once on the sphere; nseg = the count; both NaN where channel 0 is 0
//     (K10's rule: a level that crosses nothing, a NaN level among them); an infinite term: that level's integral alone is NaN.
//
// Mapping: K10's -- the tile walk of xc_cell_walk.h unchanged, the segments of xc_clen_cell.h, the level groups over gridDim.z --; what K15 adds
// is in xc_cline_cell.h.  The integrand's four corner nodes are loaded inside the per-level callback: crossed cells are sparse and the four
// loads sit next to the tracer's lines.  This first version re-reads them for every crossed level of a cell (cache hits after the first).
//
// Sums: the order-free fixed-point sums of K10 (xc_binning.h det_split, k_det3_reduce with two channels).  Windows, fixed before the pass,
// c0 laid out [slab][channel]: channel 0 K10's bound on one segment (clen_segment_bound); channel 1 that bound x max(|min F|, |max F|) over the
// slab's finite integrand values (K1's finite-only pass) x 1.0000001, 0 for a slab without a finite value.  Terms are signed: their chunks
// are two's complement and their limbs fold signed (cline_carry_signed); the lengths fold through clen_carry as in K10, so with a NaN-free
// integrand length and count are K10's bit for bit.  Capacity: a word takes at most one chunk (|chunk| < 2^48) per segment; a block gives
// each LDS copy at most CLINE_COPY_CELLS = 16383 cells, i.e. at most 32766 chunks (< 2^63, signed), and carries before it writes.
#include "xc_capi.h"
#include <cmath>

namespace xc {
namespace {

#include "xc_binning.h"
#include "xc_levels.h"
#include "xc_cell_walk.h"
#include "xc_clen_cell.h"
#include "xc_cline_cell.h"

constexpr size_t CLINE_LDS = 48 * 1024;     // LDS per block (several blocks per CU)

// The window constants c0[slab][channel]: channel 0 from K10's bound on one segment, channel 1 from that bound times the largest finite
// |F| of the slab (mm[slab] = K1's finite-only (min, max), NaN without a finite value: bound 0)
__global__ __launch_bounds__(256)
void k_cline_window(const double* __restrict__ fy, int64_t ny, const double* __restrict__ fx, int64_t nx, int latlon,
                    int64_t nslab, const double* __restrict__ mm, int* __restrict__ c0, double period)
{
    const double bound = clen_segment_bound(fy, ny, fx, nx, latlon, period);
    const int w = det_c0_from_bound(bound);
    for (int64_t s = threadIdx.x; s < nslab; s += 256) {
        const double m = fmax(fabs(mm[2 * s]), fabs(mm[2 * s + 1]));                      // (fmax skips NaN; both NaN: NaN)
        c0[CLINE_NCH * s] = w;
        c0[CLINE_NCH * s + 1] = det_c0_from_bound(m == m ? __dmul_rn(__dmul_rn(bound, m), 1.0000001) : 0.0);
    }
}

// The pass of k_cline (WRAP = false) and k_ring_cline (WRAP = true: periodic X), K10's clen_pass with two channels.  grid (bps, nslab, level
// groups of G).  LDS: levels [G + 2] (-inf, the group's levels, +inf), then per (level, copy) CLINE_WORDS limb words and one count word.
template <typename TQ, typename TF, bool LATLON, bool WRAP>
__device__ __forceinline__
void cline_pass(const TQ* __restrict__ q, const TF* __restrict__ f, int64_t ny, int64_t nx, const double* __restrict__ fy,
                const double* __restrict__ fx, const double* __restrict__ contours, int N, int contours_per_slab, int G,
                const int* __restrict__ c0s, int64_t ntj, int64_t nti, int bps, int ncopy, unsigned long long* __restrict__ part_l,
                unsigned* __restrict__ part_c, double period)
{
    extern __shared__ double sm[];
    const int tid = threadIdx.x;
    const int64_t slab = blockIdx.y;
    const int g0 = blockIdx.z * G, ng = (N - g0 < G) ? N - g0 : G;
    double* s_cx = sm;                                                                    // [ng + 2]
    unsigned long long* s_acc = (unsigned long long*)(sm + ng + 2);                       // [ng][ncopy][CLINE_WORDS]
    unsigned* s_cnt = (unsigned*)(s_acc + (size_t)ng * ncopy * CLINE_WORDS);             // [ng][ncopy]
    const double* cs = contours + (contours_per_slab ? (size_t)slab * N : 0) + g0;
    for (int k = tid; k < ng * ncopy * CLINE_WORDS; k += WALK_TPB) s_acc[k] = 0ull;
    for (int k = tid; k < ng * ncopy; k += WALK_TPB) s_cnt[k] = 0u;
    const LevelSearch ls = load_levels<WALK_TPB>(cs, ng, s_cx);                            // (its barrier covers the sums cleared above)
    const int c0len = c0s[CLINE_NCH * slab], c0term = c0s[CLINE_NCH * slab + 1];
    const int cshift = __builtin_ctz((unsigned)ncopy), copy = tid & (ncopy - 1);
    const TF* fs = f + (size_t)slab * ny * nx;
    double xL, xR;                                                                        // the coordinates of this lane's cell columns
    cell_walk<TQ, WRAP>(q + (size_t)slab * ny * nx, ny, nx, ntj, nti, bps, s_cx, ng, ls,
        [&](int64_t i, int64_t c) {                                                       // the lane of column nx: column 0, one period on
            if constexpr (WRAP) xL = i == nx ? __dadd_rn(fx[0], period) : fx[c]; else xL = fx[c];
            xR = lane_shift_keep<DPP_WAVE_SHL1>(xL, xL);
        },
        [&](int k, int64_t r, int64_t c, double ul, double ur, double ll, double lr) {
            int64_t cr = c + 1;                                                           // the right corners' node column: the seam cell's is 0
            if constexpr (WRAP) { if (c == nx - 1) cr = 0; }
            const TF* f0 = fs + (size_t)r * nx;
            const TF* f1 = f0 + nx;
            const double Ful = (double)f0[c], Fur = (double)f0[cr], Fll = (double)f1[c], Flr = (double)f1[cr];
            cline_cell_level<LATLON>(ul, ur, ll, lr, Ful, Fur, Fll, Flr, s_cx[k + 1], (double)r, (double)c, fy[r], fy[r + 1], xL, xR,
                                     s_acc + ((size_t)((k << cshift) + copy)) * CLINE_WORDS, s_cnt + (k << cshift) + copy, c0len, c0term);
        });
    __syncthreads();
    // per level: the copies carried into canonical limbs and summed -- lengths unsigned (clen_carry of xc_clen_cell.h), terms signed
    // (cline_carry_signed) --, written as this block's partial: limbs [channel][limb][level], as k_det3_reduce reads them
    const size_t pb = ((size_t)slab * bps + blockIdx.x);
    constexpr int NL = CLINE_NCH * kDetLimbsX;
    for (int k = tid; k < ng; k += WALK_TPB) {
        unsigned long long acc[kDetLimbsX] = {0ull, 0ull, 0ull, 0ull}, n = 0ull;
        long long tacc[kDetLimbsX] = {0, 0, 0, 0};
        unsigned flag = 0u;
        for (int cp = 0; cp < ncopy; ++cp) {
            const unsigned long long* w = s_acc + ((size_t)((k << cshift) + cp)) * CLINE_WORDS;
            const unsigned cw = s_cnt[(k << cshift) + cp];
            clen_carry(acc, n, flag, w, cw);
            cline_carry_signed(tacc, w + CLEN_WORDS);
            flag |= cw & CLINE_FLAG;
        }
        clen_carry_top(acc);
        const int kg = g0 + k;
#pragma unroll
        for (int l = 0; l < kDetLimbsX; ++l) {
            part_l[(pb * NL + l) * N + kg] = acc[l];
            part_l[(pb * NL + kDetLimbsX + l) * N + kg] = (unsigned long long)tacc[l];
        }
        part_c[pb * N + kg] = ((unsigned)n & 0x0fffffffu) | flag;
    }
}

#define XC_CLINE_PARAMS const TQ* __restrict__ q, const TF* __restrict__ f, int64_t ny, int64_t nx, const double* __restrict__ fy,               \
                        const double* __restrict__ fx, const double* __restrict__ contours, int N, int contours_per_slab, int G,               \
                        const int* __restrict__ c0s, int64_t ntj, int64_t nti, int bps, int ncopy, unsigned long long* __restrict__ part_l,     \
                        unsigned* __restrict__ part_c
#define XC_CLINE_ARGS q, f, ny, nx, fy, fx, contours, N, contours_per_slab, G, c0s, ntj, nti, bps, ncopy, part_l, part_c

template <typename TQ, typename TF, bool LATLON>
__global__ __launch_bounds__(WALK_TPB)
void k_cline(XC_CLINE_PARAMS)
{
    cline_pass<TQ, TF, LATLON, false>(XC_CLINE_ARGS, 0.0);
}

// periodic X: the ring of nx cell columns
template <typename TQ, typename TF, bool LATLON>
__global__ __launch_bounds__(WALK_TPB)
void k_ring_cline(XC_CLINE_PARAMS, double period)
{
    cline_pass<TQ, TF, LATLON, true>(XC_CLINE_ARGS, period);
}
#undef XC_CLINE_ARGS
#undef XC_CLINE_PARAMS

// red[slab][channel][level] -> length and integral: both NaN where the length sum is 0 (K10's rule; a NaN level crosses nothing), else times
// the radius once
__global__ __launch_bounds__(256)
void k_cline_finish(const double* __restrict__ red, int64_t nslab, int N, double radius, double* __restrict__ out_integral,
                    double* __restrict__ out_length)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nslab * N) return;
    const int64_t s = i / N, k = i - s * N;
    const double t = red[(s * CLINE_NCH) * N + k], g = red[(s * CLINE_NCH + 1) * N + k];
    const bool none = t == 0.0;
    out_length[i] = none ? dnan() : (radius > 0.0 ? __dmul_rn(t, radius) : t);
    out_integral[i] = none ? dnan() : (radius > 0.0 ? __dmul_rn(g, radius) : g);
}

template <typename TQ, typename TF>
void cline_launch(xc_ctx* ctx, bool latlon, bool wrap, dim3 grid, size_t lds, const void* q, const void* f, int64_t ny, int64_t nx,
                  const double* fy, const double* fx, const double* contours, int N, int contours_per_slab, int G, const int* c0,
                  int64_t ntj, int64_t nti, int bps, int ncopy, unsigned long long* part_l, unsigned* part_c, double period)
{
#define XC_CLINE_ARGS (const TQ*)q, (const TF*)f, ny, nx, fy, fx, contours, N, contours_per_slab, G, c0, ntj, nti, bps, ncopy, part_l, part_c
#define XC_CLINE(LL_) do {                                                                                                          \
        if (wrap) hipLaunchKernelGGL((k_ring_cline<TQ, TF, LL_>), grid, dim3(WALK_TPB), lds, ctx->stream, XC_CLINE_ARGS, period);      \
        else hipLaunchKernelGGL((k_cline<TQ, TF, LL_>), grid, dim3(WALK_TPB), lds, ctx->stream, XC_CLINE_ARGS);                        \
    } while (0)
    if (latlon) XC_CLINE(true); else XC_CLINE(false);
#undef XC_CLINE
#undef XC_CLINE_ARGS
}

}  // namespace

int launch_contour_line_integrals(xc_ctx* ctx, const void* q, int q_dtype, const void* f, int f_dtype, int64_t nslab, int64_t ny,
                                  int64_t nx, const double* ycoord, const double* xcoord, double period, double radius,
                                  const double* contours, int N, int contours_per_slab, double* out_integral, double* out_length,
                                  uint64_t* out_nseg)
{
    if (!q || !f || !ycoord || !xcoord || !contours || !out_integral || !out_length || nslab < 1 || ny < 1 || nx < 1 || N < 1)
        return fail(ctx, XC_EBADARG, "xc_contour_line_integrals: bad arguments");
    if (q_dtype != XC_F32 && q_dtype != XC_F64) return fail(ctx, XC_EBADARG, "xc_contour_line_integrals: q_dtype must be XC_F32 or XC_F64");
    if (f_dtype != XC_F32 && f_dtype != XC_F64) return fail(ctx, XC_EBADARG, "xc_contour_line_integrals: f_dtype must be XC_F32 or XC_F64");
    if (!(radius >= 0.0)) return fail(ctx, XC_EBADARG, "xc_contour_line_integrals: radius must be >= 0");
    if (nslab > 65535) return fail(ctx, XC_EBADARG, "xc_contour_line_integrals: nslab too large");
    // period != 0: periodic X (the entry points have checked the period); the ring has nx cell columns
    const bool wrap = period != 0.0;
    if (wrap && (!std::isfinite(period) || nx < 2))
        return fail(ctx, XC_EBADARG, "xc_contour_line_integrals: period must be finite, and nx >= 2 on a ring");
    // LDS: K10's budget rule with two channels: level values 8 B + per copy CLINE_WORDS x 8 + 4 B.  As many copies (up to 8) as the budget
    // takes for all levels; one copy and groups of G levels past it
    auto lds_of = [](int g, int nc) { return (size_t)(g + 2) * 8 + (size_t)g * nc * (CLINE_WORDS * 8 + 4) + 16; };
    int ncopy = 8;
    while (ncopy > 1 && lds_of(N, ncopy) > CLINE_LDS) ncopy >>= 1;
    int G = N;
    if (lds_of(N, ncopy) > CLINE_LDS) G = (int)((CLINE_LDS - 32) / (8 + CLINE_WORDS * 8 + 4));
    const int ngroup = (N + G - 1) / G;
    const size_t lds = lds_of(G, ncopy);
    // blocks per slab: at most CLINE_COPY_CELLS cells per copy: a tile gives a copy WALK_RB * WALK_TPB / ncopy of them
    const WalkGeometry wg = walk_geometry(ny, nx, wrap, nslab, (int64_t)CLINE_COPY_CELLS * ncopy / (WALK_RB * WALK_TPB));
    const int64_t ntj = wg.ntj, nti = wg.nti, bps = wg.bps;
    {   // (xc_last_clen_geometry; the C entry points clear it when the call fails)
        xc_clen_geometry& g = ctx->last_clen;
        g = xc_clen_geometry{};
        g.q_dtype = q_dtype; g.latlon = radius > 0.0; g.N = N; g.ncopy = ncopy; g.G = G; g.ngroup = ngroup;
        g.ntile = wg.ntile; g.bps = (int32_t)bps; g.bps_rule = wg.bps_rule; g.nslab = nslab;
    }
    constexpr int NL = CLINE_NCH * kDetLimbsX;
    const int64_t ncell = ny * nx;
    const int P = minmax_blocks(ncell, nslab);
    unsigned long long *part_l, *nseg; unsigned* part_c; int* c0; double *red, *mmpart, *mm;
    XC_TRY(lay_out(ctx, &ctx->scratch, &ctx->scratch_bytes, [&](Carve c) {
        part_l = c.take<unsigned long long>((size_t)nslab * bps * NL * N); part_c = c.take<unsigned>((size_t)nslab * bps * N);
        c0 = c.take<int>((size_t)nslab * CLINE_NCH); red = c.take<double>((size_t)nslab * CLINE_NCH * N);
        nseg = out_nseg ? (unsigned long long*)out_nseg : c.take<unsigned long long>((size_t)nslab * N);
        mmpart = c.take<double>((size_t)nslab * P * 2); mm = c.take<double>((size_t)nslab * 2);
        return c.at;
    }));
    const int latlon = radius > 0.0;
    // the integrand's finite extrema (K1), then both window constants of every slab
    XC_TRY(launch_minmax_partial(ctx, f, f_dtype, nslab, ncell, mmpart, nullptr, 0, true));
    XC_TRY(launch_minmax_final(ctx, mmpart, nslab, P, mm));
    hipLaunchKernelGGL(k_cline_window, dim3(1), dim3(256), 0, ctx->stream, ycoord, ny, xcoord, nx, latlon, nslab, mm, c0, period);
    XC_HIP(ctx, hipGetLastError());
    if (bps > 0) {
        const dim3 grid((unsigned)bps, (unsigned)nslab, (unsigned)ngroup);
#define XC_CLINE_GO(TQ_, TF_) cline_launch<TQ_, TF_>(ctx, latlon, wrap, grid, lds, q, f, ny, nx, ycoord, xcoord, contours, N, contours_per_slab, G, \
                                                     c0, ntj, nti, (int)bps, ncopy, part_l, part_c, period)
        if (q_dtype == XC_F64) { if (f_dtype == XC_F64) XC_CLINE_GO(double, double); else XC_CLINE_GO(double, float); }
        else { if (f_dtype == XC_F64) XC_CLINE_GO(float, double); else XC_CLINE_GO(float, float); }
#undef XC_CLINE_GO
        XC_HIP(ctx, hipGetLastError());
    }
    XC_TRY(launch_det3_reduce(ctx, nslab, (int)bps, CLINE_NCH, N, reinterpret_cast<const double*>(part_l), part_c, c0, red, nseg));
    const int64_t n = nslab * (int64_t)N;
    hipLaunchKernelGGL(k_cline_finish, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, red, nslab, N, latlon ? radius : 0.0,
                       out_integral, out_length);
    XC_HIP(ctx, hipGetLastError());
    return XC_OK;
}

}  // namespace xc

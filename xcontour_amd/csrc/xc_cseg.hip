// K12 -- marching-squares contour SEGMENTS (gfx950): what K10 (xc_clen.hip) sums, written out.
//
// No reference call site inside the snapshot's package (its find_contour helper is not in it); the reference's scripts trace contours
// with skimage's find_contours and go on from the polylines (tests/test_clength.py:615-630, tests/test_breaking.py,
// tests/test_localLength.py).  Build-defined.  The rule is K10's, stated in the header of xc_clen.hip (case table, frac, saddles as
// fully_connected='low', a NaN corner emits nothing), with the two differences of xc_cseg_cell.h: segments are DIRECTED (start -> end
// as in skimage's _get_contour_segments) and a segment whose two end points coincide is kept.
//
// Record, one per segment, as a structure of arrays: e_from / e_to (int64) the ids of the grid edges its start / end point lie on --
// horizontal edge (r, c)-(r, c+1): 2 (r nx + c); vertical edge (r, c)-(r+1, c): 2 (r nx + c) + 1 -- and pts[4] (float64) = (r1, c1, r2,
// c2) in index space, each coordinate one correctly rounded sub / div / add.  Within one (slab, level) every grid edge is the start of
// at most one segment and the end of at most one: e_from identifies the segment, and joining (xc_join.cpp) is integer matching.
//
// Layout: segments packed by (slab, level): range (s, k) = [off[s N + k], off[s N + k + 1]), off the exclusive scan of the counts.  The
// order INSIDE a range is unspecified (it depends on the order in which a block's lanes take their slots).
//
// Two passes over K10's tile walk and launch geometry (xc_cell_walk.h; level groups of XC_CSEG_GROUP_LEVELS over gridDim.z):
//   count  every block counts its segments per level in LDS (ds_add_u32) and writes them: part[slab][block][level];
//   k_cseg_sum   per (slab, level): the blocks' counts -> each block's offset inside the range, and the range's count;
//   k_cseg_scan  the exclusive scan of the range counts -> off[nslab N + 1];
//   emit   the same walk; every block keeps one LDS cursor per level (ds_add_rtn_u32) and writes the record at
//          off[range] + the block's offset + slot with plain stores.
// No global atomics, no float atomics; counts and records are the same on every run, up to the order inside a range.
// Capacity: a block's count of one level is a 32-bit word: the launcher gives a block at most 2^17 tiles (< 2^32 segments).
//
// Periodic X (WRAP, xc_contour_segments_periodic): as in K10 the plane gains one cell column, index nx-1 -- the seam cell --, whose
// left corners are node column nx-1 and whose right corners are node column 0: cL = nx-1, cR = nx exactly (a point on its right edge
// has column (double)nx).  Edge ids: the seam cell's top and bottom edges are H(r, nx-1) and H(r+1, nx-1), ids the plain kernel never
// uses, and its right edge is column 0's, V(r, 0) = 2 r nx + 1 (the plain hT + 3 would be V(r+1, 0)); every other id is unchanged, so
// per (slab, level) every edge still starts at most one segment and ends at most one.  The result is what the plain kernel returns
// for the plane with column 0 appended as column nx -- pts bit for bit -- with every edge id folded from that plane's numbering to
// the ring's: (kind, r, c) over nx + 1 columns -> 2 (r nx + (c mod nx)) + kind.  nx >= 2; Y never wraps.
// Kernels k_ring_seg<TQ, EMIT>; k_cseg is the same code with the wrap compiled out.  Mapping: the seam rule of xc_cell_walk.h; what
// K12 adds is above: the seam cell's edge ids (rwrap) and cR = nx, which is cL + 1 as for every other cell.
#include "xc_capi.h"
#include <cmath>

namespace xc {
namespace {

#include "xc_binning.h"
#include "xc_levels.h"
#include "xc_cell_walk.h"
#include "xc_clen_cell.h"
#include "xc_cseg_cell.h"

constexpr int64_t CSEG_MAX_TILES = 1 << 17; // tiles per block at most: 2^17 x 32 x 252 cells x 2 segments < 2^32

// LDS of a block (dynamic, 16-byte aligned carve): s_cx[G + 2] (-inf, the group's levels, +inf) | s_base[G] | s_cur[G]; load_levels
// adds 32 static bytes
constexpr size_t cseg_lds(int G) { return (size_t)(G + 2) * 8 + (size_t)G * 8 + (size_t)G * 4 + 16; }
static_assert(cseg_lds(XC_CSEG_GROUP_LEVELS) + 32 <= 48 * 1024, "a level group must fit 48 KB of LDS");

#define XC_CSEG_PARAMS const TQ* __restrict__ q, int64_t ny, int64_t nx, const double* __restrict__ contours, int N, int contours_per_slab, \
                        int G, int64_t ntj, int64_t nti, int bps, unsigned* __restrict__ part,                                            \
                        const unsigned long long* __restrict__ part_off, const long long* __restrict__ off, long long capacity,           \
                        long long* __restrict__ e_from, long long* __restrict__ e_to, double* __restrict__ pts
#define XC_CSEG_ARGS q, ny, nx, contours, N, contours_per_slab, G, ntj, nti, bps, part, part_off, off, capacity, e_from, e_to, pts

// The pass of k_cseg (WRAP = false: the plane as it is) and k_ring_seg (WRAP = true: periodic X); WRAP is a compile-time variant: the
// plain kernel pays nothing for it.
// EMIT = false: part[slab][block][level] = the block's segment count.  EMIT = true: the records, at off[slab N + level] +
// part_off[slab][block][level] + slot; nothing is written at or past `capacity`.
template <typename TQ, bool EMIT, bool WRAP>
__device__ __forceinline__
void cseg_pass(XC_CSEG_PARAMS)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const int tid = threadIdx.x;
    const int64_t slab = blockIdx.y;
    const int g0 = blockIdx.z * G, ng = (N - g0 < G) ? N - g0 : G;
    double* s_cx = sm;                                                                    // [ng + 2]
    unsigned long long* s_base = (unsigned long long*)(s_cx + ng + 2);                    // [ng]
    unsigned* s_cur = (unsigned*)(s_base + ng);                                           // [ng]
    const double* cs = contours + (contours_per_slab ? (size_t)slab * N : 0) + g0;
    const size_t pb = ((size_t)slab * bps + blockIdx.x) * N + g0;                         // this block's row of part / part_off
    for (int k = tid; k < ng; k += WALK_TPB) {
        s_cur[k] = 0u;
        if constexpr (EMIT) s_base[k] = (unsigned long long)off[(size_t)slab * N + g0 + k] + part_off[pb + k];
    }
    const LevelSearch ls = load_levels<WALK_TPB>(cs, ng, s_cx);                            // (its barrier covers the cursors set above)
    const int64_t nx2 = 2 * nx;
    int64_t rwrap;                                                                        // the seam cell's right edge: V(r, 0)
    cell_walk<TQ, WRAP>(q + (size_t)slab * ny * nx, ny, nx, ntj, nti, bps, s_cx, ng, ls,
        [&](int64_t i, int64_t) { rwrap = (WRAP && i == nx - 1) ? nx2 : 0; },
        [&](int k, int64_t r, int64_t c, double ul, double ur, double ll, double lr) {
            const double lv = s_cx[k + 1];
            if constexpr (EMIT) {
                const unsigned long long base = s_base[k];
                cseg_cell(ul, ur, ll, lr, lv, (double)r, (double)c, 2 * (r * nx + c), nx2, rwrap,
                          [&](int64_t ef, int64_t et, double r1, double c1, double r2, double c2) {
                              const unsigned slot = __hip_atomic_fetch_add(s_cur + k, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                              const long long at = (long long)(base + slot);
                              if (at < capacity) {
                                  e_from[at] = ef; e_to[at] = et;
                                  double* p = pts + 4 * (size_t)at;
                                  p[0] = r1; p[1] = c1; p[2] = r2; p[3] = c2;
                              }
                          });
            } else {
                lds_add(s_cur + k, (unsigned)cseg_count(cell_case(ul, ur, ll, lr, lv)));
            }
        });
    if constexpr (!EMIT) {
        __syncthreads();
        for (int k = tid; k < ng; k += WALK_TPB) part[pb + k] = s_cur[k];
    }
}

template <typename TQ, bool EMIT>
__global__ __launch_bounds__(WALK_TPB)
void k_cseg(XC_CSEG_PARAMS)
{
    cseg_pass<TQ, EMIT, false>(XC_CSEG_ARGS);
}

// periodic X: the ring of nx cell columns
template <typename TQ, bool EMIT>
__global__ __launch_bounds__(WALK_TPB)
void k_ring_seg(XC_CSEG_PARAMS)
{
    cseg_pass<TQ, EMIT, true>(XC_CSEG_ARGS);
}
#undef XC_CSEG_ARGS
#undef XC_CSEG_PARAMS

// per (slab, level): part[slab][b][level], b = 0 .. bps-1, -> part_off[slab][b][level] = the sum over the blocks before b, and
// count[slab][level] = the sum over all.  bps = 0 (no cells): counts of 0.
__global__ __launch_bounds__(256)
void k_cseg_sum(const unsigned* __restrict__ part, int64_t nslab, int bps, int N, unsigned long long* __restrict__ part_off,
                unsigned long long* __restrict__ count)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nslab * N) return;
    const int64_t s = i / N, k = i - s * N;
    unsigned long long t = 0ull;
    for (int b = 0; b < bps; ++b) {
        const size_t at = ((size_t)s * bps + b) * N + k;
        part_off[at] = t;
        t += part[at];
    }
    count[i] = t;
}

// off[0 .. M] = the exclusive scan of count[0 .. M-1] (off[M] the total).  One block: every thread sums a contiguous chunk, the
// chunk sums are scanned in LDS, every thread writes its chunk.
__global__ __launch_bounds__(1024)
void k_cseg_scan(const unsigned long long* __restrict__ count, int64_t M, long long* __restrict__ off)
{
    __shared__ unsigned long long s_sum[1024];
    const int tid = threadIdx.x;
    const int64_t per = (M + 1023) / 1024, i0 = tid * per, i1 = (i0 + per < M) ? i0 + per : M;
    unsigned long long t = 0ull;
    for (int64_t i = i0; i < i1; ++i) t += count[i];
    s_sum[tid] = t;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                                                  // inclusive scan of the chunk sums
        const unsigned long long a = tid >= o ? s_sum[tid - o] : 0ull;
        __syncthreads();
        s_sum[tid] += a;
        __syncthreads();
    }
    unsigned long long run = s_sum[tid] - t;
    for (int64_t i = i0; i < i1; ++i) { off[i] = (long long)run; run += count[i]; }
    if (tid == 1023) off[M] = (long long)s_sum[1023];
}

}  // namespace

// One xc_contour_segments_dev call (device pointers; wrap != 0: xc_contour_segments_periodic_dev, the ring of nx cell columns).  Waits
// for the stream once, between the passes: the total decides on the host whether the records fit.  -> XC_OK, 1 (capacity < total:
// only out_count was written) or an error.
int launch_contour_segments(xc_ctx* ctx, const void* q, int q_dtype, int64_t nslab, int64_t ny, int64_t nx, int wrap,
                            const double* contours, int N, int contours_per_slab, int64_t capacity,
                            uint64_t* out_count, int64_t* e_from, int64_t* e_to, double* pts, int64_t* out_total)
{
    if (out_total) *out_total = 0;
    if (!q || !contours || !out_count || nslab < 1 || ny < 1 || nx < 1 || N < 1 || capacity < 0)
        return fail(ctx, XC_EBADARG, "xc_contour_segments: bad arguments");
    if (q_dtype != XC_F32 && q_dtype != XC_F64) return fail(ctx, XC_EBADARG, "xc_contour_segments: q_dtype must be XC_F32 or XC_F64");
    if (wrap && nx < 2) return fail(ctx, XC_EBADARG, "xc_contour_segments_periodic: nx >= 2");
    if (nslab > 65535) return fail(ctx, XC_EBADARG, "xc_contour_segments: nslab too large");
    if (capacity > 0 && (!e_from || !e_to || !pts)) return fail(ctx, XC_EBADARG, "xc_contour_segments: capacity > 0 needs the record arrays");
    if (ny > (int64_t)1 << 30 || nx > (int64_t)1 << 30) return fail(ctx, XC_EBADARG, "xc_contour_segments: plane too large for the edge ids");
    const int G = N < XC_CSEG_GROUP_LEVELS ? N : XC_CSEG_GROUP_LEVELS;
    const int ngroup = (N + G - 1) / G;
    if (ngroup > 65535) return fail(ctx, XC_EBADARG, "xc_contour_segments: too many contours");
    const size_t lds = cseg_lds(G);
    // blocks per slab: at most CSEG_MAX_TILES tiles each
    const WalkGeometry wg = walk_geometry(ny, nx, wrap != 0, nslab, CSEG_MAX_TILES);
    const int64_t ntj = wg.ntj, nti = wg.nti, bps = wg.bps;
    if (bps > 0x7fffffff) return fail(ctx, XC_EBADARG, "xc_contour_segments: plane too large");
    const int64_t M = nslab * (int64_t)N;
    unsigned* part; unsigned long long* part_off; long long* off;
    XC_TRY(lay_out(ctx, &ctx->scratch, &ctx->scratch_bytes, [&](Carve c) {
        part = c.take<unsigned>((size_t)nslab * bps * N); part_off = c.take<unsigned long long>((size_t)nslab * bps * N);
        off = c.take<long long>((size_t)(M + 1));
        return c.at;
    }));
    const dim3 grid((unsigned)bps, (unsigned)nslab, (unsigned)ngroup);
#define XC_CSEG_ARGS(TQ_) (const TQ_*)q, ny, nx, contours, N, contours_per_slab, G, ntj, nti, (int)bps, part, part_off, off, (long long)capacity, \
                          (long long*)e_from, (long long*)e_to, pts
#define XC_CSEG(TQ_, EMIT_) do {                                                                                                      \
        if (wrap) hipLaunchKernelGGL((k_ring_seg<TQ_, EMIT_>), grid, dim3(WALK_TPB), lds, ctx->stream, XC_CSEG_ARGS(TQ_));                \
        else hipLaunchKernelGGL((k_cseg<TQ_, EMIT_>), grid, dim3(WALK_TPB), lds, ctx->stream, XC_CSEG_ARGS(TQ_));                         \
    } while (0)
    if (bps > 0) {
        if (q_dtype == XC_F64) XC_CSEG(double, false); else XC_CSEG(float, false);
        XC_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_cseg_sum, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, ctx->stream, part, nslab, (int)bps, N, part_off,
                       (unsigned long long*)out_count);
    XC_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_cseg_scan, dim3(1), dim3(1024), 0, ctx->stream, (const unsigned long long*)out_count, M, off);
    XC_HIP(ctx, hipGetLastError());
    // the one round trip: the total
    if (!ctx->pinned_flag) XC_HIP(ctx, hipHostMalloc((void**)&ctx->pinned_flag, 64, hipHostMallocDefault));
    long long* h_total = (long long*)ctx->pinned_flag;
    XC_HIP(ctx, hipMemcpyAsync(h_total, off + M, 8, hipMemcpyDeviceToHost, ctx->stream));
    XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const int64_t total = (int64_t)*h_total;
    if (out_total) *out_total = total;
    if (total > capacity) return 1;
    if (total > 0) {
        if (q_dtype == XC_F64) XC_CSEG(double, true); else XC_CSEG(float, true);
        XC_HIP(ctx, hipGetLastError());
    }
#undef XC_CSEG
#undef XC_CSEG_ARGS
    return XC_OK;
}

}  // namespace xc

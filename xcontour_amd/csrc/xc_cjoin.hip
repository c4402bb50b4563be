// K14 -- K12's segment records joined into polylines ON THE DEVICE (gfx950): the content of xc_join_segments (xc_join.cpp), with the
// records already gathered into walk order.  K13 (xc_cpiece.hip) labels the pieces; what it does not know is where a segment sits
// inside its piece.  K14 adds that -- the RANK of a segment along its polyline -- and the place of every polyline in its range.
//
// Input: count[nrange], e_from, e_to, pts as xc_contour_segments[_periodic]_dev wrote them; E = 2 ny nx bounds every edge id.  Labels,
// links, ranks and slots are 32-bit: E < 2^31 and every range has fewer than 2^31 segments (XC_EBADARG else).
//
// Per GROUP of consecutive ranges (xc_cpiece_link.h: K13's groups under K13's cap, indices group-local):
//   phase A (K13's kernels)
//     k_cp_scatter, k_cp_link   the dense edge table, next0 and prev0
//     k_cj_check      the records are a join's input: tab[e_from[i]] == i (no repeated e_from), prev0[next0[i]] == i (no repeated e_to
//                     among segments that have a successor); a segment WITHOUT successor claims its e_to's free table slot (-1 -> -2,
//                     one compare-and-swap) and a second claimant of that slot is a repeated e_to too.  Keeps prev0.
//     k_cj_unmark     the claimed slots back to -1
//     k_cp_round      R = ceil(log2(largest count of the group)) + 1 rounds: label = the smallest e_from of the piece, prev >= 0 on
//                     every member of a ring and -1 on every member of an open piece
//     k_cj_root       root(i) = tab[range][label], the segment with the piece's smallest e_from; size[i] = 0
//   phase B
//     k_cj_rank_init  p = prev0, but -1 at the root of every ring (the ring is cut at its smallest e_from: xc_join.cpp's start);
//                     rank = 1 where p >= 0; the piece's size by one integer atomic add onto the root
//     k_cj_rank_round R rounds of list ranking on double buffers: rank' = rank + rank[p], p' = p[p].  After k rounds rank counts the
//                     predecessors within 2^k links; R rounds cover every piece: rank = the segment's position in its polyline's walk
//   placement: the polylines of a range are ordered by first_edge, and the range's row of the edge table is sorted by edge id.  An
//   exclusive scan along the row over the ROOT entries of (size, 1) gives every root the start of its polyline inside the range and
//   its index among the range's polylines.  Three bounded launches, no look-back, no waiting between blocks:
//     k_cj_chunk_sums one block per chunk of CJ_CHUNK table entries of one row: the chunk's sum (chunks never span rows)
//     k_cj_scan_sums  one block per row: the exclusive scan of its chunk sums; the row's total is poly_count[range]
//     k_cj_apply      one block per chunk: rescans the chunk (registers and LDS) from the chunk's prefix, writes start and index at
//                     root entries only
//     k_cj_place      inv[off[range] + start[root] + rank] = the segment (every dest checked against its range), and at the roots the
//                     polyline's index, size and ring flag into arrays that outlive the group
//     k_cp_unscatter  the table is cleared once per call and handed on clean
// The host reads poly_count (the second round trip, as in K13) and stops with 1 when the polylines exceed `capacity`.  Then
//     k_cj_emit       one pass: thread d writes walk position d -- pts, e_from and the source index of segment inv[d]: the STORES are
//                     coalesced (32 B per lane for pts), the gather is on the load side -- and, where segment d is a root, its polyline's
//                     record at poff[range] + index.
// Records that are no join's input (an id outside [0, E), a repeated id) are XC_EBADARG; every index taken from a table is checked
// against its bounds before it addresses anything, every loop has a fixed trip count.
#include "xc_capi.h"
#include <vector>

namespace xc {
namespace {

#include "xc_cpiece_link.h"

constexpr int CJ_ITEMS = 8;                          // table entries per thread of a scan block
constexpr int CJ_CHUNK = CP_TPB * CJ_ITEMS;          // 2048 entries per chunk
constexpr int CJ_RING = (int)0x80000000u;            // gsz: the polyline is a ring
constexpr int CJ_ERR_DUP = 4;
constexpr int CJ_STAGES = 5;

__global__ __launch_bounds__(CP_TPB)
void k_cj_check(int64_t n, long long s0, long long E, const long long* __restrict__ e_from, const long long* __restrict__ e_to,
                int* __restrict__ tab, const int* __restrict__ rid, const int* __restrict__ nxt, const int* __restrict__ prv,
                int* __restrict__ p0, int* __restrict__ err)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= n) return;
    const size_t row = (size_t)rid[i] * E;
    const long long ef = e_from[s0 + i];
    bool bad = false;
    if (ef >= 0 && ef < E) bad = tab[row + ef] != (int)i;
    const int j = nxt[i];
    if (j >= 0) bad = bad || prv[j] != (int)i;
    else {
        const long long et = e_to[s0 + i];
        if (et >= 0 && et < E) bad = bad || atomicCAS(tab + row + et, -1, -2) != -1;
    }
    p0[i] = prv[i];
    if (bad) atomicOr(err, CJ_ERR_DUP);
}

__global__ __launch_bounds__(CP_TPB)
void k_cj_unmark(int64_t n, long long s0, long long E, const long long* __restrict__ e_to, int* __restrict__ tab,
                 const int* __restrict__ rid, const int* __restrict__ nxt)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= n || nxt[i] >= 0) return;
    const long long et = e_to[s0 + i];
    if (et < 0 || et >= E) return;
    int* slot = tab + (size_t)rid[i] * E + et;
    if (*slot == -2) *slot = -1;
}

__global__ __launch_bounds__(CP_TPB)
void k_cj_root(int64_t n, long long E, const int* __restrict__ tab, const int* __restrict__ rid, const int* __restrict__ lab,
               int* __restrict__ root, unsigned* __restrict__ size)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= n) return;
    const int l = lab[i];
    int t = (l >= 0 && l < E) ? tab[(size_t)rid[i] * E + l] : (int)i;
    if (t < 0 || t >= n) t = (int)i;
    root[i] = t;
    size[i] = 0u;
}

__global__ __launch_bounds__(CP_TPB)
void k_cj_rank_init(int64_t n, const int* __restrict__ root, const int* __restrict__ prv, int* __restrict__ p, unsigned* __restrict__ rank,
                    unsigned* __restrict__ size)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= n) return;
    const int t = root[i];
    int a = p[i];
    if (t == (int)i && prv[i] >= 0) a = -1;                               // the root of a ring: the walk starts here
    if (a >= n) a = -1;
    p[i] = a;
    rank[i] = a >= 0 ? 1u : 0u;
    atomicAdd(size + t, 1u);
}

__global__ __launch_bounds__(CP_TPB)
void k_cj_rank_round(int64_t n, const int* __restrict__ p, const unsigned* __restrict__ rank, int* __restrict__ p2,
                     unsigned* __restrict__ rank2)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= n) return;
    const int a = p[i];
    unsigned r = rank[i];
    int a2 = -1;
    if (a >= 0) { r += rank[a]; a2 = p[a]; }
    rank2[i] = r; p2[i] = a2;
}

// what a table entry adds to the scan: (size << 32) | 1 at a root's entry, nothing elsewhere
__device__ __forceinline__ unsigned long long cj_entry(int v, int64_t n, const int* __restrict__ root, const unsigned* __restrict__ size)
{
    if (v < 0 || v >= n || root[v] != v) return 0ull;
    return ((unsigned long long)size[v] << 32) | 1ull;
}

// the CJ_ITEMS entries of this thread (E is even and the thread's first index is even: an in-range pair is whole)
__device__ __forceinline__ void cj_load(const int* __restrict__ rowp, long long E, long long at, int (&v)[CJ_ITEMS])
{
#pragma unroll
    for (int k = 0; k < CJ_ITEMS; k += 2) {
        int2 w = make_int2(-1, -1);
        if (at + k < E) w = *reinterpret_cast<const int2*>(rowp + at + k);
        v[k] = w.x; v[k + 1] = w.y;
    }
}

// inclusive scan of one value per thread over the block, through the waves' shuffles and LDS; returns the block's total in `total`
__device__ __forceinline__ unsigned long long cj_block_scan(unsigned long long x, unsigned long long* lds, unsigned long long& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    __syncthreads();                                                       // (the previous use of lds is over)
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    unsigned long long before = 0ull, all = 0ull;
#pragma unroll
    for (int w = 0; w < CP_TPB / 64; ++w) {
        const unsigned long long t = lds[w];
        if (w < wave) before += t;
        all += t;
    }
    total = all;
    return x + before;
}

__global__ __launch_bounds__(CP_TPB)
void k_cj_chunk_sums(long long E, int64_t nchunk, int64_t n, const int* __restrict__ tab, const int* __restrict__ root,
                     const unsigned* __restrict__ size, unsigned long long* __restrict__ sums)
{
    __shared__ unsigned long long lds[CP_TPB / 64];
    const int64_t row = (int64_t)blockIdx.x / nchunk, chunk = (int64_t)blockIdx.x % nchunk;
    int v[CJ_ITEMS];
    cj_load(tab + (size_t)row * E, E, chunk * CJ_CHUNK + (long long)threadIdx.x * CJ_ITEMS, v);
    unsigned long long x = 0ull, total;
#pragma unroll
    for (int k = 0; k < CJ_ITEMS; ++k) x += cj_entry(v[k], n, root, size);
    (void)cj_block_scan(x, lds, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(CP_TPB)
void k_cj_scan_sums(int64_t nchunk, unsigned long long* __restrict__ sums, int64_t r0, unsigned long long* __restrict__ poly_count)
{
    __shared__ unsigned long long lds[CP_TPB / 64];
    unsigned long long* s = sums + (size_t)blockIdx.x * nchunk;
    unsigned long long carry = 0ull;
    for (int64_t base = 0; base < nchunk; base += CP_TPB) {
        const int64_t c = base + threadIdx.x;
        const unsigned long long x = c < nchunk ? s[c] : 0ull;
        unsigned long long total;
        const unsigned long long incl = cj_block_scan(x, lds, total);
        if (c < nchunk) s[c] = incl - x + carry;
        carry += total;
    }
    if (threadIdx.x == 0) poly_count[r0 + blockIdx.x] = carry & 0xffffffffull;
}

__global__ __launch_bounds__(CP_TPB)
void k_cj_apply(long long E, int64_t nchunk, int64_t n, const int* __restrict__ tab, const int* __restrict__ root,
                const unsigned* __restrict__ size, const unsigned long long* __restrict__ sums, unsigned* __restrict__ start,
                int* __restrict__ pidx)
{
    __shared__ unsigned long long lds[CP_TPB / 64];
    const int64_t row = (int64_t)blockIdx.x / nchunk, chunk = (int64_t)blockIdx.x % nchunk;
    int v[CJ_ITEMS];
    cj_load(tab + (size_t)row * E, E, chunk * CJ_CHUNK + (long long)threadIdx.x * CJ_ITEMS, v);
    unsigned long long e[CJ_ITEMS], x = 0ull, total;
#pragma unroll
    for (int k = 0; k < CJ_ITEMS; ++k) { e[k] = cj_entry(v[k], n, root, size); x += e[k]; }
    unsigned long long at = cj_block_scan(x, lds, total) - x + sums[blockIdx.x];
#pragma unroll
    for (int k = 0; k < CJ_ITEMS; ++k) {
        if (e[k] != 0ull) { start[v[k]] = (unsigned)(at >> 32); pidx[v[k]] = (int)(at & 0x7fffffffull); }
        at += e[k];
    }
}

__global__ __launch_bounds__(CP_TPB)
void k_cj_place(int64_t n, long long s0, const long long* __restrict__ off, int64_t r0, const int* __restrict__ rid,
                const int* __restrict__ root, const unsigned* __restrict__ rank, const unsigned* __restrict__ start,
                const int* __restrict__ pidx, const unsigned* __restrict__ size, const int* __restrict__ prv, int* __restrict__ inv,
                int* __restrict__ gidx, int* __restrict__ gsz, int* __restrict__ err)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= n) return;
    const int64_t r = r0 + rid[i];
    const long long base = off[r], cnt = off[r + 1] - base;
    const int t = root[i];
    const unsigned long long dest = (unsigned long long)start[t] + rank[i];
    if (dest < (unsigned long long)cnt) inv[base + (long long)dest] = (int)(s0 + i - base);
    else atomicOr(err, CP_ERR_LINK);
    const bool isroot = t == (int)i;
    gidx[s0 + i] = isroot ? pidx[i] : -1;
    gsz[s0 + i] = isroot ? (int)((size[i] & 0x7fffffffu) | (prv[i] >= 0 ? (unsigned)CJ_RING : 0u)) : 0;
}

__global__ __launch_bounds__(CP_TPB)
void k_cj_emit(int64_t total, const long long* __restrict__ off, int64_t nrange, const long long* __restrict__ poff,
               const unsigned long long* __restrict__ poly_count, const int* __restrict__ inv, const int* __restrict__ gidx,
               const int* __restrict__ gsz, const long long* __restrict__ e_from, const double* __restrict__ pts,
               long long* __restrict__ poly_nseg, int* __restrict__ poly_closed, long long* __restrict__ poly_first_edge,
               double* __restrict__ pts_walk, long long* __restrict__ e_from_walk, long long* __restrict__ order, int* __restrict__ err)
{
    const int64_t d = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (d >= total) return;
    const int64_t r = cp_range_of(off, 0, nrange, d);
    const long long base = off[r], cnt = off[r + 1] - base;
    // segment d as a root: its polyline's record
    const int g = gidx[d];
    if (g >= 0) {
        if ((unsigned long long)g < poly_count[r]) {
            const long long p = poff[r] + g;
            const int sz = gsz[d];
            poly_nseg[p] = (long long)(sz & 0x7fffffff);
            poly_closed[p] = sz < 0 ? 1 : 0;
            poly_first_edge[p] = e_from[d];
        } else atomicOr(err, CP_ERR_LINK);
    }
    // walk position d: the segment that belongs here
    const int s = inv[d];
    if (s < 0 || s >= cnt) { atomicOr(err, CP_ERR_LINK); return; }
    const long long src = base + s;
    if (pts_walk) {
        const double2 a = *reinterpret_cast<const double2*>(pts + 4 * (size_t)src), b = *reinterpret_cast<const double2*>(pts + 4 * (size_t)src + 2);
        *reinterpret_cast<double2*>(pts_walk + 4 * (size_t)d) = a;
        *reinterpret_cast<double2*>(pts_walk + 4 * (size_t)d + 2) = b;
    }
    if (e_from_walk) e_from_walk[d] = e_from[src];
    if (order) order[d] = src;
}

}  // namespace

// One xc_contour_polylines_dev call.  Waits for the stream twice: for K12's counts (they size the groups and fix the rounds) and for the
// polyline counts (they decide on the host whether the records fit).
int launch_contour_polylines(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to, const double* pts,
                             int64_t ny, int64_t nx, int64_t capacity, uint64_t* poly_count, int64_t* poly_nseg, int32_t* poly_closed,
                             int64_t* poly_first_edge, double* pts_walk, int64_t* e_from_walk, int64_t* order)
{
    if (!count || !poly_count || nrange < 1 || ny < 1 || nx < 1 || capacity < 0)
        return fail(ctx, XC_EBADARG, "xc_contour_polylines: bad arguments");
    if (capacity > 0 && (!poly_nseg || !poly_closed || !poly_first_edge))
        return fail(ctx, XC_EBADARG, "xc_contour_polylines: capacity > 0 needs the polyline arrays");
    if (ny > ((int64_t)1 << 30) / nx) return fail(ctx, XC_EBADARG, "xc_contour_polylines: plane too large for 32-bit labels (2 ny nx < 2^31)");
    const long long E = 2 * ny * nx;
    CpProfile& prof = ctx->prof_cjoin;
    profile_clear(prof);

    CpPlan pl;
    XC_TRY(cp_plan(ctx, "xc_contour_polylines", nrange, count, poly_count, e_from, e_to, pts, E, pl));
    const long long total = pl.total;
    if (total == 0) return XC_OK;

    const int64_t nchunk = (E + CJ_CHUNK - 1) / CJ_CHUNK;
    if (pl.gmax > (((int64_t)1 << 31) - 1) / nchunk)
        return fail(ctx, XC_EBADARG, "xc_contour_polylines: too many ranges in one group (lower xc_set_cpiece_workspace)");
    // workspace: off | poff | err | inv, gidx, gsz [total] | sums[gmax][nchunk] | the tail with ten buffers (xc_cpiece_link.h)
    constexpr int NBUF = 10;
    long long *d_off, *d_poff; int *d_err, *inv, *gidx, *gsz; unsigned long long* sums; CpTail tail;
    auto lay = [&](Carve c) {
        d_off = c.take<long long>((size_t)nrange + 1); d_poff = c.take<long long>((size_t)nrange + 1);
        d_err = c.take<int>(CP_SMALL);
        inv = c.take<int>((size_t)total); gidx = c.take<int>((size_t)total); gsz = c.take<int>((size_t)total);
        sums = c.take<unsigned long long>((size_t)pl.gmax * (size_t)nchunk);
        cp_carve_tail(c, pl, NBUF, tail);
        return c.at;
    };
    XC_TRY(lay_out(ctx, &ctx->cpiece_ws, &ctx->cpiece_ws_bytes, lay));
    int *const tab = tail.tab, *const rid = tail.rid;

    StageTimer tm(ctx, prof.ms);                                             // where the time goes (xc_set_kernel_timing)
    CpRun run(ctx, tm, pl, e_from, e_to, d_off, tail, d_err);

    tm.mark(-1);
    XC_TRY(run.upload_off());
    XC_HIP(ctx, hipMemsetAsync(d_err, 0, CP_SMALL * 4, ctx->stream));
    XC_HIP(ctx, hipMemsetAsync(inv, 0xff, (size_t)total * 4, ctx->stream));
    XC_TRY(run.fill_table());
    tm.mark(0);
    for (const CpGroup& g : pl.groups) {
        run.begin(g);
        const long long s0 = run.s0;
        const int64_t n = run.n, rows = g.r1 - g.r0;
        const dim3 grid = run.grid, blk(CP_TPB), sgrid((unsigned)(rows * nchunk));
        int *p = tail.buf[6], *root = tail.buf[7];
        unsigned* size = (unsigned*)tail.buf[8];
        int* pidx = tail.buf[9];
        // behind the table, in its stage: the records are a join's input
        hipLaunchKernelGGL(k_cj_check, grid, blk, 0, ctx->stream, n, s0, E, run.e_from, run.e_to, tab, rid, run.b.nxt, run.b.prv, p, d_err);
        hipLaunchKernelGGL(k_cj_unmark, grid, blk, 0, ctx->stream, n, s0, E, run.e_to, tab, rid, run.b.nxt);
        XC_TRY(run.rounds());
        const CpRoles& b = run.b;
        // lab, prv: the labels and the ring marks; nxt, lab2, nxt2, prv2 are free from here on
        hipLaunchKernelGGL(k_cj_root, grid, blk, 0, ctx->stream, n, E, tab, rid, b.lab, root, size);
        unsigned *rank = (unsigned*)b.nxt, *rank2 = (unsigned*)b.nxt2;
        int* p2 = b.lab2;
        hipLaunchKernelGGL(k_cj_rank_init, grid, blk, 0, ctx->stream, n, root, b.prv, p, rank, size);
        for (int k = 0; k < run.R; ++k) {
            hipLaunchKernelGGL(k_cj_rank_round, grid, blk, 0, ctx->stream, n, p, rank, p2, rank2);
            std::swap(p, p2); std::swap(rank, rank2);
        }
        XC_HIP(ctx, hipGetLastError());
        run.rounds_total += run.R;                                           // the rank rounds: as many again
        tm.mark(2);
        unsigned* start = (unsigned*)b.prv2;
        hipLaunchKernelGGL(k_cj_chunk_sums, sgrid, blk, 0, ctx->stream, E, nchunk, n, tab, root, size, sums);
        hipLaunchKernelGGL(k_cj_scan_sums, dim3((unsigned)rows), blk, 0, ctx->stream, nchunk, sums, g.r0, (unsigned long long*)poly_count);
        hipLaunchKernelGGL(k_cj_apply, sgrid, blk, 0, ctx->stream, E, nchunk, n, tab, root, size, sums, start, pidx);
        hipLaunchKernelGGL(k_cj_place, grid, blk, 0, ctx->stream, n, s0, d_off, g.r0, rid, root, rank, start, pidx, size, b.prv, inv, gidx, gsz, d_err);
        XC_HIP(ctx, hipGetLastError());
        tm.mark(3);
        XC_TRY(run.end());
    }
    run.report(prof);
    // the second round trip: the polyline counts (and whether the records were a join's input)
    std::vector<uint64_t> hp((size_t)nrange);
    int herr = 0;
    XC_HIP(ctx, hipMemcpyAsync(hp.data(), poly_count, (size_t)nrange * 8, hipMemcpyDeviceToHost, ctx->stream));
    XC_TRY(cp_read_err(ctx, d_err, &herr));
    if (herr & CP_ERR_EDGE) return fail(ctx, XC_EBADARG, "xc_contour_polylines: an edge id outside [0, 2 ny nx)");
    if (herr) return fail(ctx, XC_EBADARG, "xc_contour_polylines: an edge id repeats among the e_from or the e_to of a range");
    std::vector<long long> poff((size_t)nrange + 1);
    poff[0] = 0;
    for (int64_t r = 0; r < nrange; ++r) poff[(size_t)r + 1] = poff[(size_t)r] + (long long)hp[(size_t)r];
    if (poff[(size_t)nrange] > capacity) return 1;
    tm.mark(-1);
    XC_HIP(ctx, hipMemcpyAsync(d_poff, poff.data(), (size_t)(nrange + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_cj_emit, dim3(cp_blocks(total)), dim3(CP_TPB), 0, ctx->stream, (int64_t)total, d_off, nrange, d_poff,
                       (const unsigned long long*)poly_count, inv, gidx, gsz, (const long long*)e_from, pts, (long long*)poly_nseg,
                       (int*)poly_closed, (long long*)poly_first_edge, pts_walk, (long long*)e_from_walk, (long long*)order, d_err);
    XC_HIP(ctx, hipGetLastError());
    tm.mark(4);
    XC_TRY(cp_read_err(ctx, d_err, &herr));
    if (herr) return fail(ctx, XC_EBADARG, "xc_contour_polylines: the records are not those of one xc_contour_segments call");
    return XC_OK;
}

}  // namespace xc

// ------------------------------------------------------------------------------------ C ABI
int xc_contour_polylines_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to, const double* pts,
                             int64_t ny, int64_t nx, int64_t capacity, uint64_t* poly_count, int64_t* poly_nseg, int32_t* poly_closed,
                             int64_t* poly_first_edge, double* pts_walk, int64_t* e_from_walk, int64_t* order)
{
    XC_CTX(ctx);
    return xc::launch_contour_polylines(ctx, nrange, count, e_from, e_to, pts, ny, nx, capacity, poly_count, poly_nseg, poly_closed,
                                        poly_first_edge, pts_walk, e_from_walk, order);
}

int xc_last_cjoin_profile(xc_ctx* ctx, double* ms, int* rounds, int* groups)
{
    return xc::profile_get(ctx, &xc_ctx::prof_cjoin, xc::CJ_STAGES, ms, rounds, groups);
}

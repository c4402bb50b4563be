// K23 -- the TRACKS of a ring graph (gfx950): rings are vertices, the accepted links between the rings of consecutive steps are edges; a
// track is a connected component.  Per ring its component's smallest ring (root), the dense rank of that root (track) and its accepted
// in- and out-degree; per link whether it was accepted; per track one row.  The graph is generic: nothing here knows of planes.
//
// The rule (include/xcontour_hip.h, K23 section).  The mapping:
//   ACCEPT     one thread per link, grid-stride: the indices are checked (an index >= nring sets the error word and the call fails before
//              anything is written), the accept rule is applied -- n >= min_overlap * min(size[a], size[b]) with the product rounded once
//              (__dmul_rn) --, link_ok is written and the two degrees are counted with 32-bit integer atomics.
//   ROUNDS     parent[g] <= g at all times, parent[g] = g at the start.  A round is two kernels: HOOK, one thread per accepted link,
//              grid-stride, finds both roots and, if they differ, takes atomicMin(&parent[larger], smaller) and sets the `changed` word;
//              COMPRESS, one thread per ring, stores parent[g] = find(g).  The host repeats the round until it reads `changed` as zero.
//              find() follows strictly decreasing indices, so it ends after at most g steps; no thread waits for another thread or
//              workgroup.  Every link between two different trees unhooks the larger of their roots, so every round but the last merges
//              at least two trees of every unfinished component: at most nring rounds and the empty one; the host fails with XC_EHIP beyond
//              nring + 1.  The fixed point -- parent[g] = the smallest ring of g's component -- is unique: link order, grid size and the
//              order of arrival do not show.  (A round may walk a long chain once: the first compress of a chain of L rings given in
//              ascending order is one walk of L steps for its last ring; profiles/contour_piece_tracks.md has the rounds.)
//   RANK       the dense rank of the roots in ascending order: k_rt_count counts the roots of every block of 256 rings, the host scans the
//              block counts, k_rt_rank gives every root the block's offset plus its rank inside the block (ballots and four LDS words).
//              No look-back: no block waits for a neighbour.
//   ROWS       only when all rows fit the capacity: every ring adds itself to the row of its track with integer atomics (min, max, add),
//              so any order leaves the same words.
// Everything is built in the context's workspaces; the caller's arrays are written by copies at the very end, or not at all.
// Every index is checked before it addresses anything; every loop is bounded (grid-stride over n, a walk of at most g steps).  16 bytes of LDS.
#include "xc_capi.h"
#include <algorithm>
#include <cmath>
#include <vector>

namespace xc {
namespace {

using u64 = unsigned long long;
constexpr int RT_TPB = 256;
constexpr int64_t RT_MAX_BLOCKS = 1 << 16;      // of a grid-stride launch
constexpr int RT_ERR_INDEX = 1;                 // a link names a ring >= nring

inline unsigned rt_grid(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + RT_TPB - 1) / RT_TPB, RT_MAX_BLOCKS)); }

// the root of g's tree: parent[x] <= x, so the walk strictly descends and ends after at most g steps
__device__ __forceinline__ u64 rt_find(const u64* parent, u64 g)
{
    for (;;) {
        const u64 p = __hip_atomic_load(parent + g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p >= g) return g;
        g = p;
    }
}

__global__ __launch_bounds__(RT_TPB)
void k_rt_init(int64_t nring, u64* __restrict__ parent)
{
    const int64_t stride = (int64_t)gridDim.x * RT_TPB;
    for (int64_t g = (int64_t)blockIdx.x * RT_TPB + threadIdx.x; g < nring; g += stride) parent[g] = (u64)g;
}

// link_ok and the degrees; size may be null when mo == 0
__global__ __launch_bounds__(RT_TPB)
void k_rt_accept(int64_t nring, int64_t nlink, const long long* __restrict__ size, const long long* __restrict__ la,
                 const long long* __restrict__ lb, const long long* __restrict__ ln, double mo, unsigned char* __restrict__ ok,
                 int* __restrict__ nprev, int* __restrict__ nnext, int* __restrict__ err)
{
    const int64_t stride = (int64_t)gridDim.x * RT_TPB;
    for (int64_t i = (int64_t)blockIdx.x * RT_TPB + threadIdx.x; i < nlink; i += stride) {
        const long long a = la[i], b = lb[i], n = ln[i];
        if (a >= nring || b >= nring) { atomicOr(err, RT_ERR_INDEX); ok[i] = 0; continue; }
        bool acc = a >= 0 && b >= 0 && n >= 1;
        if (acc && mo != 0.0) {
            const long long sa = size[a], sb = size[b];
            acc = (double)n >= __dmul_rn(mo, (double)(sa < sb ? sa : sb));
        }
        ok[i] = acc ? 1 : 0;
        if (acc) { atomicAdd(nnext + a, 1); atomicAdd(nprev + b, 1); }
    }
}

__global__ __launch_bounds__(RT_TPB)
void k_rt_hook(int64_t nlink, const long long* __restrict__ la, const long long* __restrict__ lb, const unsigned char* __restrict__ ok,
               u64* parent, int* __restrict__ changed)
{
    const int64_t stride = (int64_t)gridDim.x * RT_TPB;
    bool any = false;
    for (int64_t i = (int64_t)blockIdx.x * RT_TPB + threadIdx.x; i < nlink; i += stride) {
        if (!ok[i]) continue;                                              // (an accepted link has both indices in [0, nring))
        const u64 ra = rt_find(parent, (u64)la[i]), rb = rt_find(parent, (u64)lb[i]);
        if (ra == rb) continue;
        atomicMin(parent + (ra > rb ? ra : rb), ra > rb ? rb : ra);
        any = true;
    }
    if (any) atomicOr(changed, 1);
}

__global__ __launch_bounds__(RT_TPB)
void k_rt_compress(int64_t nring, u64* parent)
{
    const int64_t stride = (int64_t)gridDim.x * RT_TPB;
    for (int64_t g = (int64_t)blockIdx.x * RT_TPB + threadIdx.x; g < nring; g += stride) {
        const u64 r = rt_find(parent, (u64)g);                             // (roots do not move in this kernel: every walk ends at the same one)
        __hip_atomic_store(parent + g, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// the roots among the 256 rings of this block: the lane's rank among them, and their number
__device__ __forceinline__ int rt_block_rank(bool is_root, int& total)
{
    __shared__ int wave_n[RT_TPB / 64];
    const u64 m = __ballot(is_root);
    const int lane = (int)(threadIdx.x & 63), wv = (int)(threadIdx.x >> 6);
    if (lane == 0) wave_n[wv] = __popcll(m);
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int k = 0; k < RT_TPB / 64; ++k) { before += k < wv ? wave_n[k] : 0; total += wave_n[k]; }
    return before + __popcll(m & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(RT_TPB)
void k_rt_count(int64_t nring, const u64* __restrict__ parent, u64* __restrict__ bcount)
{
    const int64_t g = (int64_t)blockIdx.x * RT_TPB + threadIdx.x;
    int total;
    (void)rt_block_rank(g < nring && parent[g] == (u64)g, total);
    if (threadIdx.x == 0) bcount[blockIdx.x] = (u64)total;
}

// trk[root] = its dense rank; with rows, first_ring[rank] = root
__global__ __launch_bounds__(RT_TPB)
void k_rt_rank(int64_t nring, const u64* __restrict__ parent, const u64* __restrict__ boff, int64_t ntrack, u64* __restrict__ trk,
               long long* __restrict__ first_ring)
{
    const int64_t g = (int64_t)blockIdx.x * RT_TPB + threadIdx.x;
    const bool is_root = g < nring && parent[g] == (u64)g;
    int total;
    const u64 rank = boff[blockIdx.x] + (u64)rt_block_rank(is_root, total);
    if (!is_root) return;
    trk[g] = rank;
    if (first_ring && rank < (u64)ntrack) first_ring[rank] = (long long)g;
}

// every ring takes the track of its root and, with rows, adds itself to that track's row
__global__ __launch_bounds__(RT_TPB)
void k_rt_rows(int64_t nring, const u64* __restrict__ parent, u64* trk, const int* __restrict__ step, const int* __restrict__ nprev,
               const int* __restrict__ nnext, int64_t ntrack, int* __restrict__ first_step, int* __restrict__ last_step,
               u64* __restrict__ nrings, u64* __restrict__ nsplit, u64* __restrict__ nmerge)
{
    const int64_t stride = (int64_t)gridDim.x * RT_TPB;
    for (int64_t g = (int64_t)blockIdx.x * RT_TPB + threadIdx.x; g < nring; g += stride) {
        const u64 r = parent[g];                                           // <= g
        const u64 t = trk[r];                                              // (written by k_rt_rank: only roots' words are read here)
        if (r != (u64)g) trk[g] = t;
        if (!first_step || t >= (u64)ntrack) continue;
        atomicMin(first_step + t, step[g]);
        atomicMax(last_step + t, step[g]);
        atomicAdd(nrings + t, 1ull);
        if (nnext[g] >= 2) atomicAdd(nsplit + t, 1ull);
        if (nprev[g] >= 2) atomicAdd(nmerge + t, 1ull);
    }
}

}  // namespace

// One xc_ring_tracks_dev call.  Waits for the stream as K22 does.
int launch_ring_tracks(xc_ctx* ctx, int64_t nring, int64_t nlink, const int32_t* ring_step, const int64_t* ring_size, const int64_t* link_a,
                       const int64_t* link_b, const int64_t* link_n, double min_overlap, int64_t* root, int64_t* track, int32_t* nprev,
                       int32_t* nnext, uint8_t* link_ok, int64_t capacity, uint64_t* ntrack, int64_t* first_ring, int32_t* first_step,
                       int32_t* last_step, int64_t* nrings, int64_t* nsplit, int64_t* nmerge)
{
    const char* who = "xc_ring_tracks";
    if (nring < 1 || nlink < 0 || capacity < 0 || !ring_step || !ntrack) return fail(ctx, XC_EBADARG, std::string(who) + ": bad arguments");
    if (nring >= ((int64_t)1 << 38) || nlink >= ((int64_t)1 << 38)) return fail(ctx, XC_EBADARG, std::string(who) + ": more than 2^38 rings or links");
    if (nlink > 0 && (!link_a || !link_b || !link_n)) return fail(ctx, XC_EBADARG, std::string(who) + ": nlink > 0 needs the link arrays");
    if (!(min_overlap >= 0.0 && min_overlap <= 1.0)) return fail(ctx, XC_EBADARG, std::string(who) + ": min_overlap must lie in [0, 1]");
    if (min_overlap != 0.0 && !ring_size) return fail(ctx, XC_EBADARG, std::string(who) + ": min_overlap > 0 needs ring_size");
    if (capacity > 0 && (!root || !track || !nprev || !nnext || (nlink > 0 && !link_ok) || !first_ring || !first_step || !last_step || !nrings
                         || !nsplit || !nmerge))
        return fail(ctx, XC_EBADARG, std::string(who) + ": capacity > 0 needs every output array");
    CpProfile& prof = ctx->prof_cptrack;
    profile_clear(prof);

    // workspace: err, changed | parent[nring] | trk[nring] | nprev[nring], nnext[nring] | bcount[nb], boff[nb] | ok[nlink]
    const int64_t nb = (nring + RT_TPB - 1) / RT_TPB;
    const size_t b_small = 256;
    int *d_err, *d_prev, *d_next; u64 *parent, *trk, *d_bcount, *d_boff; unsigned char* d_ok; size_t b_degrees = 0;
    auto lay = [&](Carve c) {
        d_err = c.take<int>(b_small / 4); parent = c.take<u64>((size_t)nring); trk = c.take<u64>((size_t)nring);
        b_degrees = c.mark();
        d_prev = c.take<int>((size_t)nring); d_next = c.take<int>((size_t)nring);
        b_degrees = c.mark() - b_degrees;
        d_bcount = c.take<u64>((size_t)nb); d_boff = c.take<u64>((size_t)nb); d_ok = c.take<unsigned char>((size_t)nlink + 1);
        return c.at;
    };
    XC_TRY(lay_out(ctx, &ctx->cpiece_ws, &ctx->cpiece_ws_bytes, lay));
    int* d_changed = d_err + 1;

    StageTimer tm(ctx, prof.ms);                                               // where the time goes (xc_set_kernel_timing)
    auto bail = [&](int rc) { (void)hipStreamSynchronize(ctx->stream); return rc; };
    const dim3 blk(RT_TPB);
    const long long* la = (const long long*)link_a;
    const long long* lb = (const long long*)link_b;

    tm.mark(-1);
    XC_HIP(ctx, hipMemsetAsync(d_err, 0, b_small, ctx->stream));
    XC_HIP(ctx, hipMemsetAsync(d_prev, 0, b_degrees, ctx->stream));
    hipLaunchKernelGGL(k_rt_init, dim3(rt_grid(nring)), blk, 0, ctx->stream, nring, parent);
    if (nlink > 0)
        hipLaunchKernelGGL(k_rt_accept, dim3(rt_grid(nlink)), blk, 0, ctx->stream, nring, nlink, (const long long*)ring_size, la, lb,
                           (const long long*)link_n, min_overlap, d_ok, d_prev, d_next, d_err);
    XC_HIP(ctx, hipGetLastError());
    tm.mark(0);
    int herr = 0;
    XC_HIP(ctx, hipMemcpyAsync(&herr, d_err, 4, hipMemcpyDeviceToHost, ctx->stream));
    XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (herr) return fail(ctx, XC_EBADARG, std::string(who) + ": a link names a ring >= nring");

    // the rounds: hook, compress, until nothing changed
    int rounds = 0;
    for (int changed = nlink > 0 ? 1 : 0; changed;) {
        if ((int64_t)rounds > nring) return fail(ctx, XC_EHIP, std::string(who) + ": the rounds did not end within nring + 1");
        XC_HIP(ctx, hipMemsetAsync(d_changed, 0, 4, ctx->stream));
        hipLaunchKernelGGL(k_rt_hook, dim3(rt_grid(nlink)), blk, 0, ctx->stream, nlink, la, lb, d_ok, parent, d_changed);
        hipLaunchKernelGGL(k_rt_compress, dim3(rt_grid(nring)), blk, 0, ctx->stream, nring, parent);
        XC_HIP(ctx, hipGetLastError());
        XC_HIP(ctx, hipMemcpyAsync(&changed, d_changed, 4, hipMemcpyDeviceToHost, ctx->stream));
        XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ++rounds;
    }
    prof.rounds = rounds;
    tm.mark(1);

    // the dense rank of the roots: per-block counts, the host's scan, per-block ranks
    hipLaunchKernelGGL(k_rt_count, dim3((unsigned)nb), blk, 0, ctx->stream, nring, parent, d_bcount);
    XC_HIP(ctx, hipGetLastError());
    std::vector<u64> bc((size_t)nb), bo((size_t)nb);
    XC_HIP(ctx, hipMemcpyAsync(bc.data(), d_bcount, (size_t)nb * 8, hipMemcpyDeviceToHost, ctx->stream));
    XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    u64 nt = 0;
    for (int64_t k = 0; k < nb; ++k) { bo[(size_t)k] = nt; nt += bc[(size_t)k]; }
    const uint64_t nt_out = (uint64_t)nt;
    XC_HIP(ctx, hipMemcpyAsync(ntrack, &nt_out, 8, hipMemcpyHostToDevice, ctx->stream));
    if ((int64_t)nt > capacity) { tm.mark(2); return bail(1); }

    // the staged rows: first_ring, nrings, nsplit, nmerge (8 bytes), first_step, last_step (4 bytes)
    long long* s_first; u64 *s_nrings, *s_nsplit, *s_nmerge; int *s_fstep, *s_lstep; size_t b_counts = 0;
    auto lay_acc = [&](Carve c) {
        s_first = c.take<long long>((size_t)nt);
        b_counts = c.mark();
        s_nrings = c.take<u64>((size_t)nt); s_nsplit = c.take<u64>((size_t)nt); s_nmerge = c.take<u64>((size_t)nt);
        b_counts = c.mark() - b_counts;
        s_fstep = c.take<int>((size_t)nt); s_lstep = c.take<int>((size_t)nt);
        return c.at;
    };
    if (lay_out(ctx, &ctx->cpiece_acc, &ctx->cpiece_acc_bytes, lay_acc) != XC_OK)
        return bail(fail(ctx, XC_ENOMEM, std::string(who) + ": no memory for the track rows"));
    XC_HIP(ctx, hipMemcpyAsync(d_boff, bo.data(), (size_t)nb * 8, hipMemcpyHostToDevice, ctx->stream));
    XC_HIP(ctx, hipMemsetAsync(s_nrings, 0, b_counts, ctx->stream));
    XC_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)s_fstep, 0x7fffffff, (size_t)nt, ctx->stream));
    XC_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)s_lstep, (int)0x80000000u, (size_t)nt, ctx->stream));
    hipLaunchKernelGGL(k_rt_rank, dim3((unsigned)nb), blk, 0, ctx->stream, nring, parent, d_boff, (int64_t)nt, trk, s_first);
    hipLaunchKernelGGL(k_rt_rows, dim3(rt_grid(nring)), blk, 0, ctx->stream, nring, parent, trk, (const int*)ring_step, d_prev, d_next, (int64_t)nt,
                       s_fstep, s_lstep, s_nrings, s_nsplit, s_nmerge);
    XC_HIP(ctx, hipGetLastError());
    const hipMemcpyKind dd = hipMemcpyDeviceToDevice;
    XC_HIP(ctx, hipMemcpyAsync(root, parent, (size_t)nring * 8, dd, ctx->stream));
    XC_HIP(ctx, hipMemcpyAsync(track, trk, (size_t)nring * 8, dd, ctx->stream));
    XC_HIP(ctx, hipMemcpyAsync(nprev, d_prev, (size_t)nring * 4, dd, ctx->stream));
    XC_HIP(ctx, hipMemcpyAsync(nnext, d_next, (size_t)nring * 4, dd, ctx->stream));
    if (nlink > 0) XC_HIP(ctx, hipMemcpyAsync(link_ok, d_ok, (size_t)nlink, dd, ctx->stream));
    XC_HIP(ctx, hipMemcpyAsync(first_ring, s_first, (size_t)nt * 8, dd, ctx->stream));
    XC_HIP(ctx, hipMemcpyAsync(nrings, s_nrings, (size_t)nt * 8, dd, ctx->stream));
    XC_HIP(ctx, hipMemcpyAsync(nsplit, s_nsplit, (size_t)nt * 8, dd, ctx->stream));
    XC_HIP(ctx, hipMemcpyAsync(nmerge, s_nmerge, (size_t)nt * 8, dd, ctx->stream));
    XC_HIP(ctx, hipMemcpyAsync(first_step, s_fstep, (size_t)nt * 4, dd, ctx->stream));
    XC_HIP(ctx, hipMemcpyAsync(last_step, s_lstep, (size_t)nt * 4, dd, ctx->stream));
    tm.mark(2);
    return bail(XC_OK);
}

}  // namespace xc

// ------------------------------------------------------------------------------------ C ABI
int xc_ring_tracks_dev(xc_ctx* ctx, int64_t nring, int64_t nlink, const int32_t* ring_step, const int64_t* ring_size, const int64_t* link_a,
                       const int64_t* link_b, const int64_t* link_n, double min_overlap, int64_t* root, int64_t* track, int32_t* nprev,
                       int32_t* nnext, uint8_t* link_ok, int64_t capacity, uint64_t* ntrack, int64_t* first_ring, int32_t* first_step,
                       int32_t* last_step, int64_t* nrings, int64_t* nsplit, int64_t* nmerge)
{
    XC_CTX(ctx);
    return xc::launch_ring_tracks(ctx, nring, nlink, ring_step, ring_size, link_a, link_b, link_n, min_overlap, root, track, nprev, nnext,
                                  link_ok, capacity, ntrack, first_ring, first_step, last_step, nrings, nsplit, nmerge);
}

int xc_last_cptrack_profile(xc_ctx* ctx, double* ms, int* rounds)
{
    return xc::profile_get(ctx, &xc_ctx::prof_cptrack, 3, ms, rounds, nullptr);
}

// K8 -- exact adiabatic rearrangement: device radix sort of (tracer, dA) pairs, cumulative
// area of the sorted state, sorted profile Q(A) and background-potential-energy integral.
//
// No reference call site (the reference realises "sorting" as histogram CDF + table lookup,
// SURVEY F6); this is SURVEY 8-a9, build-defined and pinned by oracle.sorted_profile:
//   drop NaN / masked cells; stable ascending sort of (q, dA); Acum = cumsum(dA_sorted);
//   Q_exact(A_j) = q_sorted[min(searchsorted(Acum, A_j, 'right'), n-1)].
//
// Every kernel takes the slab from blockIdx.y (or blockIdx.x for the one-block-per-slab kernels): a stack of
// planes is sorted by ONE set of launches (segmented sort: per-slab tile histograms, bases and scans).
//
// float64 tracers (round 3): THREE passes instead of eight.  The sort key of the passes is not the 64-bit pattern but
// the 24-bit RANGE key  d = floor((v - min) * (2^24 - 1) / (max - min))  (min / max from K1; subtract, multiply by a positive
// constant and floor are each monotone, so d never orders two values the wrong way; equal values share a d).  Three
// stable LSD passes over the bytes of d leave the pairs sorted by d with the cells of one d in their original order; a
// RUN of equal d holds 0.4 cells on average for 6.5 M pairs, so `k_fix_runs` finishes the job with a stable odd-even
// transposition sort of every run that is out of order (in LDS, runs of <= 128) and proves the result: one flag is
// read back, and only if some run was longer and out of order (a spike of distinct values narrower than 2^-24 of the
// range) the stack is sorted again by the full eight-pass path.  Ties of any length are already in order.
//
// Hand-written LSD radix sort, 8-bit digits, 64-bit order-preserving keys, f64 payload:
// one block owns one tile of 4096 consecutive elements (4 waves x 1024); stable ranks come from wave
// ballots (8 ballots give the peer mask of a lane's digit) + per-wave digit counters in LDS; the tile is
// reordered by digit in LDS before it is stored; the (digit-major) tile histogram is scanned by two
// small kernels.  The key type is a template parameter: float32 tracers sort 32-bit keys in 4 passes
// (4 B/elem histogram + 24 B/elem scatter), float64 tracers 64-bit keys in 8 passes (8 + 32 B/elem).
//
// This file: the workspace, the launchers and the two paths.  The kernels are in xc_sort_key.h (keys, range key), xc_sort_radix.h
// (the passes, the repair) and xc_sort_tail.h (scans, profile, BPE).
#include "xc_capi.h"
#include <type_traits>
#include <utility>

namespace xc {
namespace {

#ifndef XC_TILE_ROUNDS
#define XC_TILE_ROUNDS 16
#endif
// Tile of the radix passes: 4 waves x 64 lanes x TILE_ROUNDS pairs.  Sixteen rounds per lane keep a large sort's per-tile costs
// (digit scans, the histogram row per tile) small; a stack with few tiles -- the cfg5 stand-in: 3 planes x 110 tiles on 256 CUs --
// fills the chip only with the half tile (measured, r05: cfg5 0.192 -> 0.171 ms, one such plane 0.131 -> 0.108 ms with 8 rounds; 16 planes of
// 256 x 512 -- 512 tiles -- 0.178 -> 0.198 ms, 64 planes 25 % slower: the choice is by the number of tiles, not a constant).
constexpr int TILE_ROUNDS = XC_TILE_ROUNDS, BTILE = 4 * 64 * TILE_ROUNDS;
constexpr int TILE_ROUNDS_SMALL = 8, BTILE_SMALL = 4 * 64 * TILE_ROUNDS_SMALL;
#ifndef XC_SMALL_TILES_MAX
#define XC_SMALL_TILES_MAX 400
#endif
inline bool small_tiles(int64_t n, int64_t nslab) { return nslab * ((n + BTILE - 1) / BTILE) <= XC_SMALL_TILES_MAX; }
#ifndef XC_BPE_BLOCKS
#define XC_BPE_BLOCKS 256
#endif
constexpr int BPE_BLOCKS = XC_BPE_BLOCKS;
// the repair kernel (k_fix_runs, xc_sort_radix.h): owned positions per block, longest run repaired, window = 1 + FIX_C + 255 cells
constexpr int FIX_C = 1024, FIX_RUN = 128, FIX_NL = 5, FIX_W = FIX_NL * 256;
typedef unsigned long long u64;
typedef unsigned int u32;

// inclusive scan over the 64 lanes of a wave
template <typename T>
__device__ __forceinline__ T wave_incl_scan(T x, int lane)
{
    for (int o = 1; o < 64; o <<= 1) { const T y = __shfl_up(x, o); if (lane >= o) x += y; }
    return x;
}

#include "xc_sort_key.h"
#include "xc_sort_radix.h"
#include "xc_sort_tail.h"

// Workspace (device), every array with a leading slab dim.  ONE walk of the layout: with a null base it only adds up `bytes`.
struct SortWs {
    void *kA, *kB;               // keys, ping / pong (sized for 64-bit keys either way)
    double *vA, *vB;             // payload, ping / pong
    unsigned *hist, *totals;     // [256][ntiles] tile histogram of a pass (ntiles of the half tiling: the larger one), its row sums
    unsigned* nvalid;
    double *bsum, *parts;        // block sums of the f64 scan, BPE partials
    double *mmpart, *mm;         // K1 partials, [4] min / max / robust range
    unsigned* tick;              // arrival tickets of the kernels that finish in their last block (zeroed by k_range_bounds / a memset)
    unsigned *rhist, *rtab;      // coarse histogram and table of the range key
    size_t bytes;
};
SortWs sort_ws(void* base, int64_t n, int64_t nslab)
{
    const size_t S = (size_t)nslab, ntiles = (size_t)((n + BTILE_SMALL - 1) / BTILE_SMALL), nb = (size_t)((n + 2047) / 2048);
    SortWs w;
    w.bytes = 0;
    auto take = [&](auto*& p, size_t bytes) {
        p = base ? (std::remove_reference_t<decltype(p)>)((char*)base + w.bytes) : nullptr;
        w.bytes += al(bytes);
    };
    take(w.kA, S * n * 8); take(w.kB, S * n * 8); take(w.vA, S * n * 8); take(w.vB, S * n * 8);
    take(w.hist, S * 256 * ntiles * 4); take(w.totals, S * 256 * 4); take(w.nvalid, S * 4);
    take(w.bsum, S * nb * 8); take(w.parts, S * BPE_BLOCKS * 8);
    take(w.mmpart, S * kMinmaxBlocks * 2 * 8); take(w.mm, S * 4 * 8); take(w.tick, S * 4 * 4);
    take(w.rhist, S * RANGE_NB * 4); take(w.rtab, S * 2 * RANGE_NB * 4);
    return w;
}

// what the passes of one sort share: the ping-pong buffers (swapped by every pass) and the launch constants
template <typename K>
struct SortRun {
    K *kin, *kout; double *vin, *vout;
    int64_t n; unsigned ns; unsigned *hist, *totals; PairSrc src;
    bool tsmall, mf32;           // half tiles; the mask is float32
};

// one LSD pass (histogram, row scan, scatter); MODE 0: byte `shift / 8` of the key, MODE 1: of the 24-bit range key
template <typename K, bool FIRST, typename TQ, typename TM, int MODE, int TR>
int launch_pass(xc_ctx* ctx, SortRun<K>& s, int shift)
{
    constexpr int BT = 4 * 64 * TR;
    constexpr size_t lds = (size_t)BT * 8 + (4 * 256 + 256 + 8) * sizeof(unsigned) + BT;
    const int ntiles = (int)((s.n + BT - 1) / BT);
    const int inline_scan = ntiles <= 32 ? 1 : 0;       // measured: the O(ntiles) walk per block costs ~0.14 us per tile, the scan launch ~5 us
    const dim3 grid((unsigned)ntiles, s.ns);
    const auto scatter = k_radix_scatter<K, FIRST, TQ, TM, MODE, TR>;
    XC_TRY(ensure_big_lds(ctx, (const void*)scatter, (int)lds));
    hipLaunchKernelGGL((k_radix_hist<K, FIRST, TQ, TM, MODE, TR>), grid, dim3(256), 0, ctx->stream, s.kin, s.n, shift, ntiles, s.hist, s.src);
    if (!inline_scan) hipLaunchKernelGGL((k_block_exscan<unsigned, true>), dim3(256, s.ns), dim3(1024), 0, ctx->stream, s.hist, ntiles, s.totals);
    hipLaunchKernelGGL(scatter, grid, dim3(256), lds, ctx->stream, s.kin, s.vin, s.kout, s.vout, s.n, shift, ntiles, s.hist, s.totals, inline_scan, s.src);
    XC_HIP(ctx, hipGetLastError());
    std::swap(s.kin, s.kout);
    std::swap(s.vin, s.vout);
    return XC_OK;
}

// the kernels that read the mask itself (pass 0, k_range_hist) take its type as a template argument
template <typename T> struct Tag { typedef T type; };
template <typename F> int with_mask_type(bool mf32, F&& f) { return mf32 ? f(Tag<float>()) : f(Tag<double>()); }

// pass 0 reads the tracer itself (the unsorted pairs never touch memory), the later passes the pairs of the pass before
template <typename K, typename TQ, int MODE>
int pass(xc_ctx* ctx, SortRun<K>& s, bool first, int shift)
{
    auto go = [&](auto tr) -> int {
        constexpr int TR = decltype(tr)::value;
        if (!first) return launch_pass<K, false, double, double, MODE, TR>(ctx, s, shift);
        return with_mask_type(s.mf32, [&](auto tm) { return launch_pass<K, true, TQ, typename decltype(tm)::type, MODE, TR>(ctx, s, shift); });
    };
    return s.tsmall ? go(std::integral_constant<int, TILE_ROUNDS_SMALL>()) : go(std::integral_constant<int, TILE_ROUNDS>());
}

template <typename TQ, typename K>
int sort_profile_typed(xc_ctx* ctx, const SortArgs& a)
{
    const int64_t n = a.ny * a.nx;
    const int nb = (int)((n + 2047) / 2048);
    const size_t S = (size_t)a.nslab;
    const SortWs w = sort_ws(a.workspace, n, a.nslab);
    unsigned* nvalid = a.out_nvalid ? a.out_nvalid : w.nvalid;      // the caller's own buffer: no copy at the end
    const unsigned ns = (unsigned)a.nslab, gb = (unsigned)((n + 255) / 256);
    // a per-slab dA plane is the PLANE case with a slab stride
    const int krank = a.dA_rank == XC_DA_SLAB ? XC_DA_PLANE : a.dA_rank;
    const int64_t dstride = a.dA_rank == XC_DA_SLAB ? n : 0, mstride = (a.mask && a.mask_per_slab) ? n : 0;
    const PairSrc src = {a.q, a.mask, a.dA, krank, a.negate, a.nx, mstride, dstride, w.mm, w.rtab};
    SortRun<K> s = {(K*)w.kA, (K*)w.kB, w.vA, w.vB, n, ns, w.hist, w.totals, src, small_tiles(n, a.nslab), a.mask && a.mask_dtype == XC_F32};
    const SortRun<K> start = s;

    // everything after the sort: cumulative area, profile, BPE, copies of the requested arrays
    auto tail = [&](bool count_valid) -> int {
        if (count_valid) hipLaunchKernelGGL(k_count_valid<K>, dim3(ns), dim3(64), 0, ctx->stream, s.kin, n, nvalid);
        double* acum = s.vout;                                 // reuse the idle payload buffer
        hipLaunchKernelGGL(k_scan_local<false>, dim3(nb, ns), dim3(256), 0, ctx->stream, s.vin, acum, n, w.bsum);
        hipLaunchKernelGGL((k_block_exscan<double, false>), dim3(ns), dim3(1024), 0, ctx->stream, w.bsum, nb, (double*)nullptr);
        hipLaunchKernelGGL(k_scan_local<true>, dim3(nb, ns), dim3(256), 0, ctx->stream, s.vin, acum, n, w.bsum);
        XC_HIP(ctx, hipGetLastError());
        const int nprof = a.out_Q && a.J > 0 ? (a.J + 255) / 256 : 0;
        if (a.out_bpe)          // (the profile rides in the same launch: see k_bpe)
            hipLaunchKernelGGL(k_bpe<K>, dim3(BPE_BLOCKS + nprof, ns), dim3(256), 0, ctx->stream, s.kin, s.vin, acum, nvalid, a.tbl, a.coord, a.ntbl, w.parts, n,
                               w.tick, a.out_bpe, a.targets, a.J, a.out_Q, nprof);
        else if (nprof) hipLaunchKernelGGL(k_profile<K>, dim3(nprof, ns), dim3(256), 0, ctx->stream, s.kin, acum, nvalid, a.targets, a.J, a.out_Q, n);
        if (a.out_qsorted) hipLaunchKernelGGL(k_unkey<K>, dim3(gb, ns), dim3(256), 0, ctx->stream, s.kin, n, a.out_qsorted);
        if (a.out_acum) XC_HIP(ctx, hipMemcpyAsync(a.out_acum, acum, S * n * 8, hipMemcpyDeviceToDevice, ctx->stream));
        XC_HIP(ctx, hipGetLastError());
        return XC_OK;
    };

    if constexpr (sizeof(K) == 8) {
        if (ctx->knobs.sort_range) {
            // ---- three passes over the 24-bit range key, then the short runs (see the head of this file)
            XC_TRY(launch_minmax_partial(ctx, a.q, a.q_dtype, a.nslab, n, w.mmpart));
            // the "not sorted" word lives in pinned host memory and the repair kernel writes it THERE (a system-scope atomic, only when a
            // run fails): no device word to clear before and to copy back after (two of the chain's ~20 dependent launches)
            if (!ctx->pinned_flag) XC_HIP(ctx, hipHostMalloc((void**)&ctx->pinned_flag, 64, hipHostMallocDefault));
            volatile unsigned& h_flag = *ctx->pinned_flag;
            h_flag = 0;
            hipLaunchKernelGGL(k_range_bounds, dim3(ns), dim3(512), 0, ctx->stream, w.mmpart, minmax_blocks(n, a.nslab), w.mm, w.rhist, w.tick);
            int64_t hb = (range_sample(n).nseg + 7) / 8;                 // eight 256-cell segments per block and round
            hb = hb > 1024 ? 1024 : (hb < 1 ? 1 : hb);
            with_mask_type(s.mf32, [&](auto tm) {
                hipLaunchKernelGGL((k_range_hist<TQ, typename decltype(tm)::type>), dim3((unsigned)hb, ns), dim3(256), 0, ctx->stream, n, src, w.rhist);
                return XC_OK;
            });
            hipLaunchKernelGGL(k_range_table, dim3(ns), dim3(RANGE_NB), 0, ctx->stream, w.rhist, w.rtab);
            XC_HIP(ctx, hipGetLastError());
            for (int p = 0; p < 3; ++p) XC_TRY((pass<K, TQ, 1>(ctx, s, p == 0, 8 * p)));
            hipLaunchKernelGGL(k_fix_runs<K>, dim3((unsigned)((n + FIX_C - 1) / FIX_C), ns), dim3(256), 0, ctx->stream, s.kin, s.vin, n, ctx->pinned_flag, nvalid, src);
            XC_HIP(ctx, hipGetLastError());
            // the rest is enqueued as if the repair had sufficed -- it nearly always has -- so that the GPU does not idle through
            // the one host round trip of the sort; a stack that failed the check is sorted again below and the rest redone
            XC_TRY(tail(false));
            XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
            ctx->last_sort_path = h_flag == 0 ? 1 : 2;
            if (h_flag == 0) return XC_OK;
            s = start;
        } else ctx->last_sort_path = 0;
    } else ctx->last_sort_path = 0;
    if (ctx->last_sort_path == 0) XC_HIP(ctx, hipMemsetAsync(w.tick, 0, S * 4 * 4, ctx->stream));     // (the range path's first kernel clears the tickets itself)
    for (int p = 0; p < KeyTraits<K>::passes; ++p) XC_TRY((pass<K, TQ, 0>(ctx, s, p == 0, 8 * p)));
    return tail(true);
}

}  // namespace

size_t sort_workspace_bytes(int64_t n, int64_t nslab) { return sort_ws(nullptr, n, nslab).bytes; }

int launch_sort_profile(xc_ctx* ctx, const SortArgs& a)
{
    const int64_t n = a.ny * a.nx;
    if (!a.q || !a.workspace || n < 1 || n > 0x7fffffff || a.nslab < 1 || a.nslab > 65535) return fail(ctx, XC_EBADARG, "xc_sort_profile: bad arguments");
    if (a.dA_rank < XC_DA_NONE || a.dA_rank > XC_DA_SLAB) return fail(ctx, XC_EBADARG, "xc_sort_profile: bad dA_rank");
    if (a.dA_rank != XC_DA_NONE && !a.dA) return fail(ctx, XC_EBADARG, "xc_sort_profile: dA is NULL");
    if (a.q_dtype != XC_F32 && a.q_dtype != XC_F64) return fail(ctx, XC_EBADARG, "xc_sort_profile: q_dtype must be XC_F32 or XC_F64");
    if (a.out_Q && a.J > 0 && !a.targets) return fail(ctx, XC_EBADARG, "xc_sort_profile: targets is NULL");
    if (a.out_bpe && (!a.tbl || !a.coord || a.ntbl < 2)) return fail(ctx, XC_EBADARG, "xc_sort_profile: BPE needs tbl/coord");
    if (a.q_dtype == XC_F64) return sort_profile_typed<double, u64>(ctx, a);
    return sort_profile_typed<float, u32>(ctx, a);      // the order of floats is the order of their 32-bit keys: 4 passes of 4-byte keys
}

}  // namespace xc

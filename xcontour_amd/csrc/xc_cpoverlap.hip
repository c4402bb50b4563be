// K22 -- the OVERLAP of two label maps (gfx950): per range the contingency table of two dense int32 maps [ny][nx] -- for every pair of
// labels (a, b) that share a node the number of shared nodes, the sum of w and the sum of w f over them -- built on the device; only the
// sparse table crosses to the host.  The maps are K20's (xc_cpiece_label.h) of two fields: today's rings against yesterday's.
//
// The rule (include/xcontour_hip.h, K22 section).  The mapping is K20's layout without its carries (the maps are dense):
//   THREADS    one thread per (range of the group, chunk of rows, column), columns fastest (pl_geometry, pl_thread): the two label loads
//              and the loads of w and f of a wave are contiguous.
//   RUNS       a thread walks down its chunk and keeps the current pair with a private node count and CP_L private words per sum
//              (cp_add_private, xc_cpiece_sum.h); when the pair changes, and at the chunk's end, it hands the run over to the pair's
//              slot.  At the chunk's end a wave whose lanes all hold the same pair of the same range adds its lanes' words with shuffles
//              first and issues one atomic per word (inside a large ring or the background every lane ends in the same pair; K21
//              measured that case, profiles/contour_piece_props.md).
//   SLOTS      per range an open-addressing table in global memory.  The key is (uint32)a << 32 | (uint32)b with negative labels folded
//              to -1; the all-ones key is EMPTY and is exactly the omitted pair (-1, -1).  A slot is claimed with one 64-bit atomicCAS
//              and found by linear probing, at most `slots` steps; an insertion that finds no slot sets PO_ERR_FULL and the call fails.
//              No thread spins, no kernel waits for another block.  A slot is PO_W 64-bit words: key | nodes | not-finite flags |
//              CP_L words of sum_w [| CP_L words of sum_wf]: 64 bytes without f, 104 bytes with it.  k_po_init clears them; every
//              update is a 64-bit integer atomic, so any order of arrival leaves the same words and cp_to_double rounds each sum once.
//   NO WRAP    a chunk of a term is below 2^32; a private word holds the terms of one chunk's rows, times 64 after the wave's sum; a
//              slot's word holds one term per node of the pair, at most ny nx < 2^31 of them: below 2^63 in magnitude.
//   SIZING     k_po_runs counts, per range, the runs of constant pair (other than EMPTY) down the chunks: an upper bound on the range's
//              distinct pairs.  The range's table has the next power of two >= twice that count: it is never more than half full.
//              Ranges are taken in groups of consecutive ranges whose tables fit the xc_set_cpiece_workspace cap (one range always
//              does).  On pure noise every node starts a run: 2 ny nx slots rounded up, up to 4 ny nx x 104 bytes for one range.
//   FINISH     per group k_po_count counts the occupied slots of every range into pair_count; the host takes the scan; k_po_emit
//              gives every occupied slot a row of its range (an atomic cursor: the order inside a range is the call's own) and converts
//              the words once per value into STAGED rows.  In both, a wave whose 64 consecutive slots lie in one range issues one atomic for
//              all its occupied slots (one per pair on the range's one counter took most of the call).  Nothing reaches the caller's row arrays before all rows are known to fit.
// Every index is checked before it addresses anything and every loop is bounded (a chunk's rows, a table's slots, 64 steps of a search).
// No LDS, no scratch.
#include "xc_capi.h"
#include <algorithm>
#include <type_traits>
#include <vector>

namespace xc {
namespace {

#include "xc_binning.h"

#include "xc_cpiece_link.h"
#include "xc_cpiece_slot.h"
#include "xc_cpiece_sum.h"
#include "xc_cinside_bound.h"

constexpr unsigned long long PO_EMPTY = ~0ull;   // no pair yet: the key of (-1, -1)
constexpr int PO_ERR_FULL = 1;                   // an insertion found no slot within the table
constexpr int PO_ERR_ROW = 2;                    // an occupied slot found no row within its range's count

__device__ __forceinline__ unsigned long long po_key(int a, int b)
{
    const unsigned ua = a < 0 ? 0xffffffffu : (unsigned)a, ub = b < 0 ? 0xffffffffu : (unsigned)b;
    return ((unsigned long long)ua << 32) | (unsigned long long)ub;
}

// where a key starts to probe (the 64-bit finaliser of MurmurHash3)
__device__ __forceinline__ unsigned long long po_mix(unsigned long long k)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return k;
}

// the slot of `key` in a table of `nslot` slots (a power of two) of W words each, claimed if the key is new; -1: none within nslot steps
__device__ __forceinline__ long long po_find(unsigned long long* __restrict__ tab, unsigned long long nslot, int W, unsigned long long key)
{
    const unsigned long long mask = nslot - 1ull;
    unsigned long long at = po_mix(key) & mask;
    for (unsigned long long step = 0; step < nslot; ++step, at = (at + 1ull) & mask) {
        unsigned long long* s = tab + (size_t)at * (size_t)W;
        const unsigned long long cur = __hip_atomic_load(s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == key) return (long long)at;
        if (cur != PO_EMPTY) continue;                                     // a key, once written, stays
        const unsigned long long prev = atomicCAS(s, PO_EMPTY, key);
        if (prev == PO_EMPTY || prev == key) return (long long)at;
    }
    return -1ll;
}

// the range of slot `i` of the call's tables: soff[r] <= i < soff[r + 1], r0 <= r < r1 (soff ascends; empty tables are skipped)
__device__ __forceinline__ int64_t po_range_of(const unsigned long long* __restrict__ soff, int64_t r0, int64_t r1, unsigned long long i)
{
    int64_t lo = r0, hi = r1;                                              // soff[lo] <= i < soff[hi]
    for (int step = 0; step < 64 && hi - lo > 1; ++step) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (soff[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// Do the slots of this thread's wave -- consecutive ones, lane 0's first; i: this thread's, ns: the group's -- lie in ONE range?  Then r
// is that range.  Every lane of the wave must call it, and lane 0's slot must lie inside the group's tables.
__device__ __forceinline__ bool po_wave_range(const unsigned long long* __restrict__ soff, int64_t r0, int64_t r1, unsigned long long i,
                                              unsigned long long ns, int64_t& r)
{
    const unsigned long long first = i - (unsigned long long)(threadIdx.x & 63);
    const unsigned long long last = first + 63ull < ns ? first + 63ull : ns - 1ull;
    r = po_range_of(soff, r0, r1, soff[r0] + first);
    return first < ns && r == po_range_of(soff, r0, r1, soff[r0] + last);
}

// runs[r] += the runs of constant pair, other than (-1, -1), down the chunks of range r0 + rl
__global__ __launch_bounds__(CP_TPB)
void k_po_runs(int64_t ng, int64_t r0, int64_t rows, int64_t nchunk, int64_t ny, int64_t nx, const int* __restrict__ la,
               const int* __restrict__ lb, unsigned long long* __restrict__ runs)
{
    int64_t rl, k, c;
    if (!pl_thread(ng, nchunk, nx, rl, k, c)) return;
    const size_t base = (size_t)(r0 + rl) * (size_t)ny * (size_t)nx + (size_t)c;
    const int64_t t1 = (k + 1) * rows < ny ? (k + 1) * rows : ny;
    unsigned long long cur = PO_EMPTY, cnt = 0ull;
    for (int64_t t = k * rows; t < t1; ++t) {
        const size_t node = base + (size_t)t * (size_t)nx;
        const unsigned long long key = po_key(la[node], lb[node]);
        if (key != cur) { cur = key; cnt += key != PO_EMPTY ? 1ull : 0ull; }
    }
    if (__ballot(1) == ~0ull && __all(rl == __shfl(rl, 0))) {               // one range: one atomic for the wave
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d);
        if ((threadIdx.x & 63) != 0) cnt = 0ull;
    }
    if (cnt) atomicAdd(runs + r0 + rl, cnt);
}

// `nslot` slots of a group's tables: EMPTY, all other words zero
__global__ __launch_bounds__(CP_TPB)
void k_po_init(unsigned long long nslot, int W, unsigned long long* __restrict__ tab)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= nslot * (unsigned long long)W) return;
    tab[i] = (i % (unsigned long long)W) == 0ull ? PO_EMPTY : 0ull;
}

// what a thread gathered for `key` goes to the key's slot and is cleared; tab: the range's table
template <bool HASF>
__device__ __forceinline__ void po_hand_over(unsigned long long* __restrict__ tab, unsigned long long nslot, int W, unsigned long long key,
                                             unsigned long long& n, unsigned long long (&aw)[CP_L], unsigned long long (&af)[CP_L], int& bad,
                                             int* __restrict__ err)
{
    if (n == 0ull) return;                                                 // (nothing is gathered for EMPTY)
    const long long at = nslot ? po_find(tab, nslot, W, key) : -1ll;
    if (at < 0) atomicOr(err, PO_ERR_FULL);
    else {
        unsigned long long* s = tab + (size_t)at * (size_t)W;
        atomicAdd(s + 1, n);
        if (bad) atomicOr(s + 2, (unsigned long long)bad);
#pragma unroll
        for (int l = 0; l < CP_L; ++l) if (aw[l]) atomicAdd(s + 3 + l, aw[l]);
        if constexpr (HASF) {
#pragma unroll
            for (int l = 0; l < CP_L; ++l) if (af[l]) atomicAdd(s + 3 + CP_L + l, af[l]);
        }
    }
    n = 0ull; bad = 0;
#pragma unroll
    for (int l = 0; l < CP_L; ++l) { aw[l] = 0ull; af[l] = 0ull; }
}

// The accumulate pass over the ranges [r0, r0 + ng) of a group.  soff: the exclusive scan of the slots of every range of the call; the
// group's tables start at tab.  FT: the type of f (void: none).
template <typename FT>
__global__ __launch_bounds__(CP_TPB)
void k_po_scan(int64_t ng, int64_t r0, int64_t rows, int64_t nchunk, int64_t ny, int64_t nx, int ncont, const int* __restrict__ la,
               const int* __restrict__ lb, const double* __restrict__ w, int w_per_slab, const FT* __restrict__ f,
               const unsigned long long* __restrict__ mx, const unsigned long long* __restrict__ soff, int W,
               unsigned long long* __restrict__ tab, int* __restrict__ err)
{
    constexpr bool HASF = !std::is_void<FT>::value;
    int64_t rl, k, c;
    if (!pl_thread(ng, nchunk, nx, rl, k, c)) return;
    const int64_t r = r0 + rl;
    const unsigned long long nslot = soff[r + 1] - soff[r];
    unsigned long long* rt = tab + (size_t)(soff[r] - soff[r0]) * (size_t)W;
    const size_t sl = (size_t)(r / ncont), npl = (size_t)ny * (size_t)nx;
    const double* wp = w ? w + (w_per_slab ? sl * npl : 0) : nullptr;
    const int top_w = ci_top(mx[2 * sl]);
    int top_f = 0;
    if constexpr (HASF) top_f = ci_top(mx[2 * sl + 1]);
    unsigned long long cur = PO_EMPTY, n = 0ull, aw[CP_L], af[CP_L];
#pragma unroll
    for (int l = 0; l < CP_L; ++l) { aw[l] = 0ull; af[l] = 0ull; }
    int bad = 0;
    const int64_t t1 = (k + 1) * rows < ny ? (k + 1) * rows : ny;
    for (int64_t t = k * rows; t < t1; ++t) {
        const size_t node = (size_t)t * (size_t)nx + (size_t)c;            // < ny nx
        const unsigned long long key = po_key(la[(size_t)r * npl + node], lb[(size_t)r * npl + node]);
        if (key != cur) {
            po_hand_over<HASF>(rt, nslot, W, cur, n, aw, af, bad, err);    // the run of `cur` ends
            cur = key;
        }
        if (key == PO_EMPTY) continue;
        ++n;
        const double v = wp ? wp[node] : 1.0;
        if (v == v && !cp_add_private(aw, v, top_w)) bad |= 1;
        if constexpr (HASF) {
            const double tv = __dmul_rn(v, (double)f[sl * npl + node]);
            if (tv == tv && !cp_add_private(af, tv, top_f)) bad |= 2;
        }
    }
    // The chunk's end.  Inside a large ring, or the background of one map, every lane of a wave ends its chunk in the SAME pair of the same
    // range: the wave then adds its lanes' counts and words with shuffles and lane 0 alone hands them over.  Integer sums: the slot's words
    // are the same either way.
    if (__ballot(1) == ~0ull) {                                            // (a wave with idle lanes hands over lane by lane)
        const unsigned long long k0 = __shfl(cur, 0);
        const int64_t rl0 = __shfl(rl, 0);
        if (k0 != PO_EMPTY && __all(cur == k0 && rl == rl0)) {
            const bool lead = (threadIdx.x & 63) == 0;
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) { n += __shfl_xor(n, d); bad |= __shfl_xor(bad, d); }
#pragma unroll
            for (int l = 0; l < CP_L; ++l) {
                unsigned long long v = aw[l];
                if (__any(v != 0ull)) {
#pragma unroll
                    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
                }
                aw[l] = lead ? v : 0ull;
            }
            if constexpr (HASF) {
#pragma unroll
                for (int l = 0; l < CP_L; ++l) {
                    unsigned long long v = af[l];
                    if (__any(v != 0ull)) {
#pragma unroll
                        for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
                    }
                    af[l] = lead ? v : 0ull;
                }
            }
            if (!lead) { n = 0ull; bad = 0; }
        }
    }
    po_hand_over<HASF>(rt, nslot, W, cur, n, aw, af, bad, err);
}

// pair_count[r] += the occupied slots of range r; one thread per slot of the group's tables (slots [soff[r0], soff[r1]) of the call)
__global__ __launch_bounds__(CP_TPB)
void k_po_count(int64_t r0, int64_t r1, const unsigned long long* __restrict__ soff, int W, const unsigned long long* __restrict__ tab,
                unsigned long long* __restrict__ pair_count)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * CP_TPB + threadIdx.x, ns = soff[r1] - soff[r0];
    const bool occ = i < ns && tab[(size_t)i * (size_t)W] != PO_EMPTY;
    const unsigned long long m = __ballot(occ);
    if (m == 0ull) return;                                                 // (the whole wave: lane 0's slot lies inside the tables)
    int64_t r;
    if (po_wave_range(soff, r0, r1, i, ns, r)) {                           // one range: one atomic for the wave, not one per pair
        if ((threadIdx.x & 63) == 0) atomicAdd(pair_count + r, (unsigned long long)__popcll(m));
    } else if (occ) atomicAdd(pair_count + po_range_of(soff, r0, r1, soff[r0] + i), 1ull);
}

// every occupied slot of the group -> a staged row of its range (rows [poff[r], poff[r + 1]) of `cap` staged rows)
__global__ __launch_bounds__(CP_TPB)
void k_po_emit(int64_t r0, int64_t r1, int ncont, int hasf, const unsigned long long* __restrict__ soff, int W,
               const unsigned long long* __restrict__ tab, const long long* __restrict__ poff, unsigned long long* __restrict__ cursor,
               const unsigned long long* __restrict__ mx, int64_t cap, int* __restrict__ sa, int* __restrict__ sb, long long* __restrict__ sn,
               double* __restrict__ sw, double* __restrict__ swf, int* __restrict__ err)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * CP_TPB + threadIdx.x, ns = soff[r1] - soff[r0];
    const unsigned long long* s = tab + (size_t)(i < ns ? i : 0ull) * (size_t)W;
    const unsigned long long key = i < ns ? s[0] : PO_EMPTY;
    const bool occ = key != PO_EMPTY;
    const unsigned long long m = __ballot(occ);
    if (m == 0ull) return;                                                 // (the whole wave)
    int64_t r;
    unsigned long long pos = 0ull;
    if (po_wave_range(soff, r0, r1, i, ns, r)) {                           // one range: lane 0 takes the wave's rows, a lane its rank in them
        const int lane = (int)(threadIdx.x & 63);
        if (lane == 0) pos = atomicAdd(cursor + r, (unsigned long long)__popcll(m));
        pos = __shfl(pos, 0) + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
        if (!occ) return;
    } else {
        if (!occ) return;
        r = po_range_of(soff, r0, r1, soff[r0] + i);
        pos = atomicAdd(cursor + r, 1ull);
    }
    const long long row = poff[r] + (long long)pos;
    if (row < poff[r] || row >= poff[r + 1] || row >= cap) { atomicOr(err, PO_ERR_ROW); return; }
    const int64_t sl = r / ncont;
    const int fl = (int)s[2];
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    sa[row] = (int)(unsigned)(key >> 32); sb[row] = (int)(unsigned)(key & 0xffffffffull);
    sn[row] = (long long)s[1];
    sw[row] = (fl & 1) ? qnan : cp_to_double(s + 3, ci_top(mx[2 * sl]));
    if (hasf) swf[row] = (fl & 2) ? qnan : cp_to_double(s + 3 + CP_L, ci_top(mx[2 * sl + 1]));
}

}  // namespace

// One xc_label_overlap_dev call.  Waits for the stream as K18 does.
int launch_label_overlap(xc_ctx* ctx, int64_t nrange, int64_t ny, int64_t nx, int ncont, const int32_t* lab_a, const int32_t* lab_b,
                         const double* w, int w_per_slab, const void* f, int f_dtype, int64_t capacity, uint64_t* pair_count, int32_t* a,
                         int32_t* b, int64_t* n, double* sum_w, double* sum_wf)
{
    const char* who = "xc_label_overlap";
    if (!lab_a || !lab_b || !pair_count || nrange < 1 || ny < 1 || nx < 1 || capacity < 0) return fail(ctx, XC_EBADARG, std::string(who) + ": bad arguments");
    if (ncont < 1 || nrange % ncont != 0) return fail(ctx, XC_EBADARG, std::string(who) + ": nrange must be a multiple of ncont >= 1");
    if (f && f_dtype != XC_F32 && f_dtype != XC_F64) return fail(ctx, XC_EBADARG, std::string(who) + ": f_dtype is XC_F32 or XC_F64");
    if (capacity > 0 && (!a || !b || !n || !sum_w)) return fail(ctx, XC_EBADARG, std::string(who) + ": capacity > 0 needs the row arrays");
    if (capacity > 0 && (f == nullptr) != (sum_wf == nullptr)) return fail(ctx, XC_EBADARG, std::string(who) + ": f and sum_wf go together");
    if (ny > (((int64_t)1 << 31) - 1) / nx) return fail(ctx, XC_EBADARG, std::string(who) + ": plane too large (ny nx < 2^31)");
    const int64_t nslab = nrange / ncont;
    if (nslab > 65535) return fail(ctx, XC_EBADARG, std::string(who) + ": more than 65535 slabs");
    CpProfile& prof = ctx->prof_cpoverlap;
    profile_clear(prof);
    const int64_t npl = ny * nx;
    const int hasf = f ? 1 : 0;
    const int W = 3 + CP_L * (1 + hasf);
    int64_t rows = 0, nchunk = 0;
    pl_geometry(ny, &rows, &nchunk);
    // the ranges one launch of a scan takes: 2^30 threads (one range, PL_CHUNKS nx < 2^36 threads at most, is always taken)
    const int64_t rmax = std::max<int64_t>(1, ((int64_t)1 << 30) / (nchunk * nx));

    // workspace: mx[nslab][2], err (cleared together) | runs, soff, poff, cursor: nrange + 1 words each (runs and cursor use nrange)
    unsigned long long *mx, *d_runs, *d_soff, *d_cur; long long* d_poff; int* d_err; size_t b_zero = 0;
    auto lay = [&](Carve c) {
        mx = c.take<unsigned long long>((size_t)nslab * 2); d_err = c.take<int>(CP_SMALL);
        b_zero = c.mark();                                                  // (from the first block on)
        d_runs = c.take<unsigned long long>((size_t)nrange + 1); d_soff = c.take<unsigned long long>((size_t)nrange + 1);
        d_poff = c.take<long long>((size_t)nrange + 1); d_cur = c.take<unsigned long long>((size_t)nrange + 1);
        return c.at;
    };
    XC_TRY(lay_out(ctx, &ctx->cpiece_ws, &ctx->cpiece_ws_bytes, lay));

    StageTimer tm(ctx, prof.ms);                                                // where the time goes (xc_set_kernel_timing)

    const dim3 blk(CP_TPB);
    const int* la = (const int*)lab_a;
    const int* lb = (const int*)lab_b;
    tm.mark(-1);
    XC_HIP(ctx, hipMemsetAsync(mx, 0, b_zero, ctx->stream));
    XC_HIP(ctx, hipMemsetAsync(d_runs, 0, (size_t)nrange * 8, ctx->stream));
    XC_HIP(ctx, hipMemsetAsync(d_cur, 0, (size_t)nrange * 8, ctx->stream));
    XC_HIP(ctx, hipMemsetAsync(pair_count, 0, (size_t)nrange * 8, ctx->stream));
    for (int64_t r0 = 0; r0 < nrange; r0 += rmax) {
        const int64_t ng = std::min(rmax, nrange - r0);
        hipLaunchKernelGGL(k_po_runs, dim3(cp_blocks(ng * nchunk * nx)), blk, 0, ctx->stream, ng, r0, rows, nchunk, ny, nx, la, lb, d_runs);
    }
    XC_HIP(ctx, hipGetLastError());
    tm.mark(0);
    std::vector<uint64_t> runs((size_t)nrange);
    XC_HIP(ctx, hipMemcpyAsync(runs.data(), d_runs, (size_t)nrange * 8, hipMemcpyDeviceToHost, ctx->stream));
    XC_HIP(ctx, hipStreamSynchronize(ctx->stream));

    // the tables: the next power of two >= twice the runs of the range (none without runs)
    std::vector<unsigned long long> soff((size_t)nrange + 1);
    soff[0] = 0ull;
    uint64_t total_runs = 0;
    for (int64_t r = 0; r < nrange; ++r) {
        unsigned long long s = 0ull;
        if (runs[(size_t)r]) { s = 2ull; while (s < 2ull * runs[(size_t)r]) s *= 2ull; }
        soff[(size_t)r + 1] = soff[(size_t)r] + s;
        total_runs += runs[(size_t)r];
    }
    if (total_runs == 0) return XC_OK;                     // both maps hold no ring: no rows (pair_count is cleared)
    XC_HIP(ctx, hipMemcpyAsync(d_soff, soff.data(), (size_t)(nrange + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    // groups of consecutive ranges whose tables fit the cap (one range always does), no more than rmax ranges; ranges without runs in
    // front of a group cost nothing
    struct Group { int64_t r0, r1; };
    std::vector<Group> groups;
    const unsigned long long slot_cap = std::min<unsigned long long>(                                    // (one thread per slot: 2^38 a launch)
        std::max<unsigned long long>(1ull, (unsigned long long)ctx->cpiece_cap / ((unsigned long long)W * 8ull)), 1ull << 38);
    unsigned long long smax = 0ull;
    for (int64_t r = 0; r < nrange;) {
        while (r < nrange && runs[(size_t)r] == 0) ++r;
        if (r >= nrange) break;
        int64_t r1 = r + 1;
        while (r1 < nrange && r1 - r < rmax && soff[(size_t)r1 + 1] - soff[(size_t)r] <= slot_cap) ++r1;
        while (r1 - 1 > r && runs[(size_t)r1 - 1] == 0) --r1;
        groups.push_back({r, r1});
        smax = std::max(smax, soff[(size_t)r1] - soff[(size_t)r]);
        r = r1;
    }
    if (smax > ((1ull << 62) / ((unsigned long long)W * 8ull))) return fail(ctx, XC_ENOMEM, std::string(who) + ": the table of one group is too large");
    // the tables of one group, then the staged rows (a, b: 4 bytes; n, sum_w, sum_wf: 8 bytes) of min(capacity, all runs)
    const int64_t cap = (int64_t)std::min<uint64_t>((uint64_t)capacity, total_runs);
    unsigned long long* tab; int *sa, *sb; long long* sn; double *sw, *swf;
    auto lay_acc = [&](Carve c) {
        tab = c.take<unsigned long long>((size_t)smax * (size_t)W);
        sa = c.take<int>((size_t)cap); sb = c.take<int>((size_t)cap);
        sn = c.take<long long>((size_t)cap); sw = c.take<double>((size_t)cap); swf = c.take<double>((size_t)cap);
        return c.at;
    };
    if (lay_out(ctx, &ctx->cpiece_acc, &ctx->cpiece_acc_bytes, lay_acc) != XC_OK)
        return fail(ctx, XC_ENOMEM, std::string(who) + ": no memory for the pair tables");

    ci_launch_bound(ctx->stream, npl, nslab, w, w_per_slab, f, f_dtype, mx);
    XC_HIP(ctx, hipGetLastError());
    tm.mark(1);

    std::vector<uint64_t> hp((size_t)nrange, 0);
    std::vector<long long> poff((size_t)nrange + 1, 0);
    int64_t done = 0;                                                       // poff[0 .. done] stand
    bool over = cap == 0;                                                   // the rows no longer fit: count only
    for (const Group& gr : groups) {
        const int64_t ng = gr.r1 - gr.r0;
        const unsigned long long ns = soff[(size_t)gr.r1] - soff[(size_t)gr.r0];
        const dim3 sgrid((unsigned)((ns + CP_TPB - 1) / CP_TPB)), lgrid(cp_blocks(ng * nchunk * nx));
        for (unsigned long long s0 = 0; s0 < ns; s0 += 1ull << 34) {        // (2^34 slots, fewer than 2^30 blocks, a launch)
            const unsigned long long n1 = std::min<unsigned long long>(ns - s0, 1ull << 34);
            hipLaunchKernelGGL(k_po_init, dim3((unsigned)((n1 * (unsigned long long)W + CP_TPB - 1) / CP_TPB)), blk, 0, ctx->stream, n1, W,
                               tab + (size_t)s0 * (size_t)W);
        }
#define XC_PO_SCAN(FT_) hipLaunchKernelGGL((k_po_scan<FT_>), lgrid, blk, 0, ctx->stream, ng, gr.r0, rows, nchunk, ny, nx, ncont, la, lb, w, w_per_slab, \
                                           (const FT_*)f, mx, d_soff, W, tab, d_err)
        if (!f) XC_PO_SCAN(void); else if (f_dtype == XC_F32) XC_PO_SCAN(float); else XC_PO_SCAN(double);
#undef XC_PO_SCAN
        XC_HIP(ctx, hipGetLastError());
        tm.mark(1);
        hipLaunchKernelGGL(k_po_count, sgrid, blk, 0, ctx->stream, gr.r0, gr.r1, d_soff, W, tab, (unsigned long long*)pair_count);
        XC_HIP(ctx, hipGetLastError());
        XC_HIP(ctx, hipMemcpyAsync(hp.data() + gr.r0, pair_count + gr.r0, (size_t)ng * 8, hipMemcpyDeviceToHost, ctx->stream));
        XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (; done < gr.r1; ++done) poff[(size_t)done + 1] = poff[(size_t)done] + (long long)hp[(size_t)done];
        if (poff[(size_t)gr.r1] > cap) over = true;
        if (!over) {
            XC_HIP(ctx, hipMemcpyAsync(d_poff + gr.r0, poff.data() + gr.r0, (size_t)(ng + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL(k_po_emit, sgrid, blk, 0, ctx->stream, gr.r0, gr.r1, ncont, hasf, d_soff, W, tab, d_poff, d_cur, mx, cap, sa, sb, sn,
                               sw, swf, d_err);
            XC_HIP(ctx, hipGetLastError());
        }
        tm.mark(2);
    }
    for (; done < nrange; ++done) poff[(size_t)done + 1] = poff[(size_t)done] + (long long)hp[(size_t)done];
    prof.groups = (int)groups.size();
    const long long np = poff[(size_t)nrange];
    int herr = 0;
    XC_HIP(ctx, hipMemcpyAsync(&herr, d_err, 4, hipMemcpyDeviceToHost, ctx->stream));
    XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (herr) return fail(ctx, XC_EHIP, std::string(who) + (herr & PO_ERR_FULL ? ": a pair found no slot in its range's table" : ": a pair found no row in its range"));
    if (np > capacity) return 1;
    if (np > 0) {
        XC_HIP(ctx, hipMemcpyAsync(a, sa, (size_t)np * 4, hipMemcpyDeviceToDevice, ctx->stream));
        XC_HIP(ctx, hipMemcpyAsync(b, sb, (size_t)np * 4, hipMemcpyDeviceToDevice, ctx->stream));
        XC_HIP(ctx, hipMemcpyAsync(n, sn, (size_t)np * 8, hipMemcpyDeviceToDevice, ctx->stream));
        XC_HIP(ctx, hipMemcpyAsync(sum_w, sw, (size_t)np * 8, hipMemcpyDeviceToDevice, ctx->stream));
        if (hasf) XC_HIP(ctx, hipMemcpyAsync(sum_wf, swf, (size_t)np * 8, hipMemcpyDeviceToDevice, ctx->stream));
    }
    tm.mark(2);
    (void)hipStreamSynchronize(ctx->stream);
    return XC_OK;
}

}  // namespace xc

// ------------------------------------------------------------------------------------ C ABI
int xc_label_overlap_dev(xc_ctx* ctx, int64_t nrange, int64_t ny, int64_t nx, int ncont, const int32_t* lab_a, const int32_t* lab_b,
                         const double* w, int w_per_slab, const void* f, int f_dtype, int64_t capacity, uint64_t* pair_count, int32_t* a,
                         int32_t* b, int64_t* n, double* sum_w, double* sum_wf)
{
    XC_CTX(ctx);
    return xc::launch_label_overlap(ctx, nrange, ny, nx, ncont, lab_a, lab_b, w, w_per_slab, f, f_dtype, capacity, pair_count, a, b, n,
                                    sum_w, sum_wf);
}

int xc_last_cpoverlap_profile(xc_ctx* ctx, double* ms, int* rounds, int* groups)
{
    return xc::profile_get(ctx, &xc_ctx::prof_cpoverlap, 3, ms, rounds, groups);
}

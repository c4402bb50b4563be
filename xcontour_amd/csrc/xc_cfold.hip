// K24 -- the FOLDS of a contour (gfx950): which runs of overturned meridians form one wave-breaking event, how many nodes and how much
// weight each event has folded over, and which way it leans -- from K12's segment records on the device.
//
// K16 counts how often each meridian meets the selected pieces and says "a column with ncross >= 3 is overturned"; K17 says what the
// pieces bound.  This is the step after both (the Barnes and Hartmann 2012 kind of analysis): the events.  Build-defined, in index space;
// the field is never read again.  include/xcontour_hip.h (K24) states the rule; in short, with X and P of K17 under the same select:
//   n[c] = sum_r X[r][c], lo[c] / hi[c] the smallest / largest r with X[r][c] = 1; a column with n[c] >= 3 is FOLDED; its fold nodes
//   are (r, c), lo[c] < r <= hi[c], and node (r, c) belongs to tongue t = P[r][c] ^ P[lo[c] + 1][c] (0 under, 1 over).  An EVENT is a
//   maximal set of folded columns with at most `gap` unfolded columns between consecutive ones, round the seam on a periodic plane.
// P[lo + 1] is 1 (X[lo] is the first flag of its column), so t is the XOR of X over the rows lo < r' < r: a lane that starts under the
// lowest crossing starts with t = 0, one that starts at a cut of the rows with !P.
//
// Per GROUP of consecutive ranges (xc_cpiece_link.h: K13's groups under K13's cap, indices group-local):
//   the bit planes cleared, phase A (K13's kernels), k_co_root, k_co_piece, k_co_pick (K16's selection: xc_cpiece_select.h, shared with
//   K16 and K17) and k_ci_mark -- one step, ci_mark_group, shared with K17 like the planes' blocks and k_ci_chunk (xc_cinside_mark.h)
//   k_cf_rows       one thread per segment of a selected piece: K16's atomic min / max of the crossing's row (its bit pattern) per column
//   k_cf_cols       the column pass: a block is 256 consecutive columns x one chunk of rows x one range; a lane walks its rows of the bit
//                   plane and adds its flags to ncross, their first and last row to lo / hi (integer atomics)
//   k_cf_runs       the run pass, over the ranges from the end of the previous group to the end of this one: one workgroup per range
//                   walks the nx columns in tiles of its width, twice.  The column of the previous folded column comes from a max-scan
//                   (wave shuffles, LDS across the waves, a carry across the tiles); a folded column further than gap + 1 from it is a
//                   head; the event index is the prefix sum of the heads.  The first walk counts the heads and finds the first and the
//                   last folded column, which decide the seam rule; the second labels the columns (col_event), fills the rows without
//                   crossing with NaN and reduces the columns of every event (integer atomics: ncol, ncross_max, the rows' bit patterns,
//                   c_east; the head writes c_west).
//   k_cf_scan       the fold scan (not on a count-only call): blocks of 256 columns x chunks of rows x the ranges of the group; a wave
//                   without folded column leaves at once.  A lane walks the rows lo + 1 .. hi of its chunk with t in a register, w and f
//                   read along x.  It keeps the limbs of every sum twice -- over both tongues, and over tongue 1 alone: the words are
//                   sums modulo 2^64, so tongue 0 is their difference, exactly -- and no limb is indexed by a run-time value.  For every
//                   event of the wave one masked wave reduction and one set of 64-bit integer atomics.
//   k_cf_finish     the limbs of the group's events rounded to double into the staging slot (range, event)
// Around the groups: k_cf_init, k_ci_bound (the maxima behind the windows), a last k_cf_runs for the ranges behind the last group,
// k_cf_offsets (the exclusive scan of event_count) and, when the events fit the capacity, k_cf_compact (the staging slots packed under
// the scan).  The dense outputs and event_count are fully written whatever the records hold; every index taken from a record or a table
// is checked before it addresses anything; every launch has a fixed amount of work.
#include "xc_capi.h"
#include <algorithm>
#include <type_traits>
#include <vector>

namespace xc {
namespace {

#include "xc_binning.h"

#include "xc_cpiece_link.h"
#include "xc_cpiece_select.h"
#include "xc_cpiece_sum.h"
#include "xc_cinside_bound.h"
#include "xc_cinside_mark.h"

constexpr int CF_WAVES = CI_TPB / 64;
constexpr int CF_NSUM = 4;                    // area, mx, my, integral
constexpr int CF_ACC = 2 * CF_NSUM * CP_L;    // the words of one event: every sum over both tongues, then over tongue 1
constexpr unsigned long long CF_QNAN = 0x7ff8000000000000ull;

// the staging slot (range, event), event < emax = ceil(nx / 2): what k_cf_runs and k_cf_finish leave for k_cf_compact
struct CfSlots {
    int *c_west, *c_east, *ncol, *nmax;
    unsigned long long *row_lo, *row_hi;      // bit patterns
    long long* nodes;                         // [slot][2]
    double* sums;                             // [slot][CF_NSUM][2]
};

// the tops of the four windows of slab s: max |w|, max |w| nx, max |w| ny (a product that overflows counts as the largest double), max |w f|
__device__ __forceinline__ void cf_tops(const unsigned long long* __restrict__ mx, int64_t s, int64_t ny, int64_t nx, int (&top)[CF_NSUM])
{
    const double mw = __longlong_as_double((long long)mx[2 * s]), big = __longlong_as_double(0x7fefffffffffffffll);
    top[0] = ci_top(mx[2 * s]);
    top[1] = ci_top((unsigned long long)__double_as_longlong(fmin(__dmul_rn(mw, (double)nx), big)));
    top[2] = ci_top((unsigned long long)__double_as_longlong(fmin(__dmul_rn(mw, (double)ny), big)));
    top[3] = ci_top(mx[2 * s + 1]);
}

__global__ __launch_bounds__(CP_TPB)
void k_cf_init(int64_t ncol, int* __restrict__ ncross, double* __restrict__ row_lo, double* __restrict__ row_hi, int* __restrict__ lo,
               int* __restrict__ hi)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= ncol) return;
    ncross[i] = 0; row_lo[i] = __longlong_as_double((long long)CI_INF); row_hi[i] = 0.0;
    lo[i] = 0x7fffffff; hi[i] = -1;
}

// K16's rows: the smallest / largest stored row over the crossings of a column (rows are non-negative doubles: their bits order like them)
__global__ __launch_bounds__(CP_TPB)
void k_cf_rows(int64_t n, long long s0, int64_t r0, long long E, int64_t nx, int select, const long long* __restrict__ e_from,
               const long long* __restrict__ e_to, const double* __restrict__ pts, const int* __restrict__ tab,
               const int* __restrict__ rid, const int* __restrict__ root, const int* __restrict__ prv, const int* __restrict__ lab,
               const unsigned* __restrict__ pn, const int* __restrict__ pw, const unsigned long long* __restrict__ key,
               double* __restrict__ row_lo, double* __restrict__ row_hi)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= n) return;
    const int t = root[i], r = rid[i];                                // (k_co_root left 0 <= t < n)
    const bool ring = prv[i] >= 0;
    int w; bool ismain;
    if (!co_selected(select, ring, t, lab[i], pn, pw, key[r0 + r], w, ismain)) return;
    const size_t out0 = (size_t)(r0 + r) * (size_t)nx;
    auto cross = [&](long long e, double row) {
        const size_t at = out0 + (size_t)((e >> 1) % nx);
        const unsigned long long b = (unsigned long long)__double_as_longlong(row);
        atomicMin((unsigned long long*)row_lo + at, b);
        atomicMax((unsigned long long*)row_hi + at, b);
    };
    const long long ef = e_from[s0 + i];
    if ((ef & 1) && ef >= 0 && ef < E) cross(ef, pts[4 * (size_t)(s0 + i)]);
    if (!ring) {
        const long long et = e_to[s0 + i];
        if ((et & 1) && et >= 0 && et < E) {
            const int j = tab[(size_t)r * E + et];
            if (j < 0 || j >= n) cross(et, pts[4 * (size_t)(s0 + i) + 2]);      // no successor: the tail of its piece
        }
    }
}

// The column pass over the ranges [g0, g0 + ng): block b is (column block, chunk, range); X has the rows r < ny - 1.
__global__ __launch_bounds__(CI_TPB)
void k_cf_cols(int64_t g0, int64_t ny, int64_t nx, int64_t wpr, int64_t ncb, int64_t rc, int64_t nchunk, const unsigned* __restrict__ bits,
               int* __restrict__ ncross, int* __restrict__ lo, int* __restrict__ hi)
{
    const int64_t b = blockIdx.x;
    const int64_t cb = b % ncb, ch = (b / ncb) % nchunk, rl = b / (ncb * nchunk);
    const int64_t c = cb * CI_TPB + threadIdx.x;
    if (c >= nx) return;
    const int cs = (int)(c & 31);
    const unsigned* bp = bits + (size_t)rl * (size_t)ny * (size_t)wpr + (size_t)(c >> 5);
    const int64_t row0 = ch * rc, row1 = std::min<int64_t>(row0 + rc, ny - 1);
    int n = 0, first = 0x7fffffff, last = -1;
    for (int64_t row = row0; row < row1; ++row) {
        if ((bp[(size_t)row * (size_t)wpr] >> cs) & 1u) {
            ++n;
            if (first > (int)row) first = (int)row;
            last = (int)row;
        }
    }
    if (n) {
        const size_t at = (size_t)(g0 + rl) * (size_t)nx + (size_t)c;
        atomicAdd(ncross + at, n); atomicMin(lo + at, first); atomicMax(hi + at, last);
    }
}

// One tile of the run pass: column base + threadIdx.x.  last / heads: the last folded column and the heads in front of the tile, brought
// up to its end on return (the same in every thread).  -> n, fold, whether the column is a head, lin: the index of its event in the order
// of the heads, prev: the folded column in front of it (-1: none).  sh: 2 CF_WAVES ints.
__device__ __forceinline__ void cf_tile(int64_t base, int64_t nx, int gap, const int* __restrict__ ncr, int* sh, int& last, int& heads,
                                        int& n, bool& fold, bool& head, int& lin, int& prev)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t c = base + threadIdx.x;
    n = c < nx ? ncr[c] : 0;
    fold = n >= 3;
    int m = fold ? (int)c : -1;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(m, d); if (lane >= d && o > m) m = o; }
    prev = __shfl_up(m, 1);
    if (lane == 0) prev = -1;
    if (lane == 63) sh[wv] = m;
    __syncthreads();
    int before = last;
    for (int k = 0; k < wv; ++k) before = sh[k] > before ? sh[k] : before;
    prev = before > prev ? before : prev;
    head = fold && (prev < 0 || (int)c - prev - 1 > gap);
    const unsigned long long hb = __ballot(head);
    if (lane == 0) sh[CF_WAVES + wv] = (int)__popcll(hb);
    __syncthreads();
    int hbefore = heads;
    for (int k = 0; k < wv; ++k) hbefore += sh[CF_WAVES + k];
    lin = hbefore + (int)__popcll(hb & ((2ull << lane) - 1ull)) - 1;
    int nl = last, nh = heads;
    for (int k = 0; k < CF_WAVES; ++k) { nl = sh[k] > nl ? sh[k] : nl; nh += sh[CF_WAVES + k]; }
    __syncthreads();                                                  // sh is the next tile's
    last = nl; heads = nh;
}

// The run pass: one workgroup per range of [ra, ra + gridDim.x).
__global__ __launch_bounds__(CI_TPB)
void k_cf_runs(int64_t ra, int64_t nx, int gap, int wrap, int64_t emax, const int* __restrict__ ncross, double* __restrict__ row_lo,
               double* __restrict__ row_hi, int* __restrict__ col_event, unsigned long long* __restrict__ event_count, CfSlots S)
{
    __shared__ int sh[2 * CF_WAVES];
    __shared__ int sfirst;
    const int64_t r = ra + blockIdx.x;
    const int* ncr = ncross + (size_t)r * (size_t)nx;
    if (threadIdx.x == 0) sfirst = -1;
    __syncthreads();
    int last = -1, heads = 0, n, lin, prev; bool fold, head;
    for (int64_t base = 0; base < nx; base += CI_TPB) {
        cf_tile(base, nx, gap, ncr, sh, last, heads, n, fold, head, lin, prev);
        if (fold && prev < 0) sfirst = (int)(base + threadIdx.x);     // the first folded column: one thread of one tile
    }
    __syncthreads();
    const int K = heads, L = last, F = sfirst;
    const bool join = wrap && K >= 2 && (int64_t)F + nx - (int64_t)L - 1 <= (int64_t)gap;      // the first run is the end of the last
    const int nev = join ? K - 1 : K;
    if (threadIdx.x == 0) event_count[r] = (unsigned long long)nev;
    const size_t slot0 = (size_t)r * (size_t)emax;
    for (int j = threadIdx.x; j < nev; j += CI_TPB) {
        S.ncol[slot0 + j] = 0; S.nmax[slot0 + j] = 0; S.c_east[slot0 + j] = -1; S.c_west[slot0 + j] = -1;
        S.row_lo[slot0 + j] = CI_INF; S.row_hi[slot0 + j] = 0ull;
    }
    __threadfence();
    __syncthreads();
    last = -1; heads = 0;
    for (int64_t base = 0; base < nx; base += CI_TPB) {
        cf_tile(base, nx, gap, ncr, sh, last, heads, n, fold, head, lin, prev);
        const int64_t c = base + threadIdx.x;
        if (c >= nx) continue;
        const size_t at = (size_t)r * (size_t)nx + (size_t)c;
        if (n == 0) { row_lo[at] = __longlong_as_double((long long)CF_QNAN); row_hi[at] = __longlong_as_double((long long)CF_QNAN); }
        const int ev = !fold ? -1 : !join ? lin : lin == 0 ? K - 2 : lin - 1;
        col_event[at] = ev;
        if (!fold) continue;
        const size_t slot = slot0 + (size_t)ev;
        atomicAdd(S.ncol + slot, 1);
        atomicMax(S.nmax + slot, n);
        atomicMin(S.row_lo + slot, (unsigned long long)__double_as_longlong(row_lo[at]));
        atomicMax(S.row_hi + slot, (unsigned long long)__double_as_longlong(row_hi[at]));
        if (head && !(join && lin == 0)) S.c_west[slot] = (int)c;
        if (!(join && lin == K - 1)) atomicMax(S.c_east + slot, (int)c);
    }
}

// both accumulators of one sum: `tot` over both tongues, `ov` over tongue 1; false where cp_add would flag the term
__device__ __forceinline__ bool cf_add(unsigned long long (&tot)[CP_L], unsigned long long (&ov)[CP_L], double v, unsigned t, int top)
{
    const bool ok = cp_add_private(tot, v, top);
    cp_add_private(ov, t ? v : 0.0, top);
    return ok;
}

// The fold scan over the ranges [g0, g0 + ng) of a group: block b is (column block, chunk, range).  acc[(rl emax + event) CF_ACC],
// cnt[.. 2] (fold nodes of both tongues, of tongue 1), flg[..]: bit 2 k + t says that sum k of tongue t met a term outside its window.
template <typename FT>
__global__ __launch_bounds__(CI_TPB)
void k_cf_scan(int64_t g0, int64_t ny, int64_t nx, int64_t wpr, int64_t ncb, int64_t rc, int64_t nchunk, int ncont, int64_t emax,
               const unsigned* __restrict__ bits, const unsigned* __restrict__ cpar, const int* __restrict__ col_event,
               const int* __restrict__ lo, const int* __restrict__ hi, const int* __restrict__ c_west, const double* __restrict__ w,
               int w_per_slab, const FT* __restrict__ f, const unsigned long long* __restrict__ mx, unsigned long long* __restrict__ acc,
               unsigned long long* __restrict__ cnt, int* __restrict__ flg)
{
    constexpr bool HASF = !std::is_void<FT>::value;
    const int64_t b = blockIdx.x;
    const int64_t cb = b % ncb, ch = (b / ncb) % nchunk, rl = b / (ncb * nchunk), r = g0 + rl;
    const int64_t c = cb * CI_TPB + threadIdx.x;
    const size_t col = (size_t)r * (size_t)nx + (size_t)c;
    const int ev = c < nx ? col_event[col] : -1;
    if (!__any(ev >= 0)) return;                                      // no folded column in this wave
    const int64_t s = r / ncont;
    const size_t npl = (size_t)ny * (size_t)nx;
    const int64_t cw = c >> 5;
    const int cs = (int)(c & 31);
    int top[CF_NSUM];
    cf_tops(mx, s, ny, nx, top);

    unsigned long long ntot = 0ull, nov = 0ull, at_[CP_L], ao[CP_L], xt[CP_L], xo[CP_L], yt[CP_L], yo[CP_L], ft[CP_L], fo[CP_L];
#pragma unroll
    for (int l = 0; l < CP_L; ++l) { at_[l] = ao[l] = xt[l] = xo[l] = yt[l] = yo[l] = ft[l] = fo[l] = 0ull; }
    int bad = 0;
    if (ev >= 0) {
        const int64_t l0 = lo[col], h0 = hi[col];                    // (folded: 0 <= l0 < h0 <= ny - 2)
        const int64_t row0 = ch * rc, a0 = std::max<int64_t>(row0, l0 + 1), a1 = std::min<int64_t>(std::min<int64_t>(row0 + rc, ny) - 1, h0);
        if (a0 <= a1) {
            const unsigned* bp = bits + (size_t)rl * (size_t)ny * (size_t)wpr + (size_t)cw;
            const double* wp = w ? w + (w_per_slab ? (size_t)s * npl : 0) + (size_t)c : nullptr;
            unsigned t = 0u;
            if (row0 > l0 + 1) {                                      // a cut of the rows inside the fold: t = !P[row0]
                t = 1u;
                for (int64_t k = 0; k < ch; ++k) t ^= (cpar[(size_t)(rl * nchunk + k) * (size_t)wpr + (size_t)cw] >> cs) & 1u;
            }
            const int64_t west = c_west[(size_t)r * (size_t)emax + (size_t)ev];
            const double dx = (double)(c >= west ? c - west : c - west + nx);
            for (int64_t row = a0; row <= a1; ++row) {
                const size_t at = (size_t)row * (size_t)nx;
                const double a = wp ? wp[at] : 1.0;
                ++ntot; nov += t;
                if (a == a && !cf_add(at_, ao, a, t, top[0])) bad |= 1 << t;
                const double tx = __dmul_rn(a, dx);
                if (tx == tx && !cf_add(xt, xo, tx, t, top[1])) bad |= 4 << t;
                const double ty = __dmul_rn(a, (double)row);
                if (ty == ty && !cf_add(yt, yo, ty, t, top[2])) bad |= 16 << t;
                if constexpr (HASF) {
                    const double tf = __dmul_rn(a, (double)f[(size_t)s * npl + at + (size_t)c]);
                    if (tf == tf && !cf_add(ft, fo, tf, t, top[3])) bad |= 64 << t;
                }
                t ^= (bp[(size_t)row * (size_t)wpr] >> cs) & 1u;
            }
        }
    }
    // every event of the wave: one masked reduction, one set of atomics
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(ev >= 0);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        const int k = __shfl(ev, src);
        const bool mine = ev == k;
        todo &= ~__ballot(mine);
        const bool lead = lane == src;
        const size_t slot = (size_t)rl * (size_t)emax + (size_t)k;
        unsigned long long* pa = acc + slot * CF_ACC;
        auto put = [&](unsigned long long* p, unsigned long long v) {
            v = ci_wave_sum(mine ? v : 0ull);
            if (lead && v) atomicAdd(p, v);
        };
        put(cnt + 2 * slot, ntot); put(cnt + 2 * slot + 1, nov);
#pragma unroll
        for (int l = 0; l < CP_L; ++l) {
            put(pa + 0 * CP_L + l, at_[l]); put(pa + 1 * CP_L + l, ao[l]);
            put(pa + 2 * CP_L + l, xt[l]); put(pa + 3 * CP_L + l, xo[l]);
            put(pa + 4 * CP_L + l, yt[l]); put(pa + 5 * CP_L + l, yo[l]);
            if constexpr (HASF) { put(pa + 6 * CP_L + l, ft[l]); put(pa + 7 * CP_L + l, fo[l]); }
        }
        int fl = 0;
#pragma unroll
        for (int q = 0; q < 2 * CF_NSUM; ++q) if (__ballot(mine && ((bad >> q) & 1))) fl |= 1 << q;
        if (lead && fl) atomicOr(flg + slot, fl);
    }
}

// the events of the ranges [g0, g0 + ng): limbs to doubles, into the staging slots
__global__ __launch_bounds__(CP_TPB)
void k_cf_finish(int64_t g0, int64_t ng, int64_t ny, int64_t nx, int ncont, int64_t emax, int hasf,
                 const unsigned long long* __restrict__ event_count, const unsigned long long* __restrict__ acc,
                 const unsigned long long* __restrict__ cnt, const int* __restrict__ flg, const unsigned long long* __restrict__ mx, CfSlots S)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= ng * emax) return;
    const int64_t rl = i / emax, j = i - rl * emax, r = g0 + rl;
    if ((unsigned long long)j >= event_count[r]) return;
    const size_t slot = (size_t)r * (size_t)emax + (size_t)j;
    int top[CF_NSUM];
    cf_tops(mx, r / ncont, ny, nx, top);
    const int fl = flg[i];
    const unsigned long long* pa = acc + (size_t)i * CF_ACC;
    const double qnan = __longlong_as_double((long long)CF_QNAN);
    S.nodes[2 * slot] = (long long)(cnt[2 * i] - cnt[2 * i + 1]);
    S.nodes[2 * slot + 1] = (long long)cnt[2 * i + 1];
#pragma unroll
    for (int k = 0; k < CF_NSUM; ++k) {
        if (k == CF_NSUM - 1 && !hasf) continue;
        unsigned long long un[CP_L];
#pragma unroll
        for (int l = 0; l < CP_L; ++l) un[l] = pa[(2 * k) * CP_L + l] - pa[(2 * k + 1) * CP_L + l];
        S.sums[(slot * CF_NSUM + k) * 2] = ((fl >> (2 * k)) & 1) ? qnan : cp_to_double(un, top[k]);
        S.sums[(slot * CF_NSUM + k) * 2 + 1] = ((fl >> (2 * k + 1)) & 1) ? qnan : cp_to_double(pa + (2 * k + 1) * CP_L, top[k]);
    }
}

// eoff[nrange + 1] = the exclusive scan of event_count: one workgroup, a run of ranges per thread
__global__ __launch_bounds__(CP_TPB)
void k_cf_offsets(int64_t nrange, const unsigned long long* __restrict__ event_count, long long* __restrict__ eoff)
{
    __shared__ long long part[CP_TPB];
    const int64_t per = (nrange + CP_TPB - 1) / CP_TPB, a = std::min<int64_t>(threadIdx.x * per, nrange), b = std::min<int64_t>(a + per, nrange);
    long long sum = 0;
    for (int64_t r = a; r < b; ++r) sum += (long long)event_count[r];
    part[threadIdx.x] = sum;
    __syncthreads();
    long long at = 0;
    for (int k = 0; k < (int)threadIdx.x; ++k) at += part[k];
    for (int64_t r = a; r < b; ++r) { eoff[r] = at; at += (long long)event_count[r]; }
    if (threadIdx.x == CP_TPB - 1) eoff[nrange] = at;
}

// the staging slots packed under eoff into the caller's arrays
__global__ __launch_bounds__(CP_TPB)
void k_cf_compact(int64_t total, int64_t nrange, int64_t emax, const long long* __restrict__ eoff, CfSlots S, int* __restrict__ c_west,
                  int* __restrict__ c_east, int* __restrict__ ncol, int* __restrict__ nmax, double* __restrict__ row_lo,
                  double* __restrict__ row_hi, long long* __restrict__ nodes, double* __restrict__ area, double* __restrict__ mx,
                  double* __restrict__ my, double* __restrict__ integral)
{
    const int64_t e = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (e >= total) return;
    const int64_t r = cp_range_of(eoff, 0, nrange, e);
    const size_t slot = (size_t)r * (size_t)emax + (size_t)(e - eoff[r]);
    c_west[e] = S.c_west[slot]; c_east[e] = S.c_east[slot]; ncol[e] = S.ncol[slot]; nmax[e] = S.nmax[slot];
    row_lo[e] = __longlong_as_double((long long)S.row_lo[slot]); row_hi[e] = __longlong_as_double((long long)S.row_hi[slot]);
    for (int t = 0; t < 2; ++t) {
        nodes[2 * e + t] = S.nodes[2 * slot + t];
        area[2 * e + t] = S.sums[(slot * CF_NSUM + 0) * 2 + t];
        mx[2 * e + t] = S.sums[(slot * CF_NSUM + 1) * 2 + t];
        my[2 * e + t] = S.sums[(slot * CF_NSUM + 2) * 2 + t];
        if (integral) integral[2 * e + t] = S.sums[(slot * CF_NSUM + 3) * 2 + t];
    }
}

}  // namespace

// One xc_contour_folds_dev call.  Waits for the stream twice: for K12's counts (they size the groups and fix the rounds) and for the event
// counts, with the word that says whether the records were K12's.
int launch_contour_folds(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to, const double* pts,
                         int64_t ny, int64_t nx, int periodic, int select, int ncont, const double* w, int w_per_slab, const void* f,
                         int f_dtype, int64_t gap, int32_t* ncross, double* row_lo, double* row_hi, int32_t* col_event, int64_t capacity,
                         uint64_t* event_count, int32_t* c_west, int32_t* c_east, int32_t* ncol, int32_t* ncross_max, double* ev_row_lo,
                         double* ev_row_hi, int64_t* nodes, double* area, double* mx_, double* my_, double* integral)
{
    if (!count || !ncross || !row_lo || !row_hi || !col_event || !event_count || nrange < 1 || ny < 1 || nx < 1 || capacity < 0)
        return fail(ctx, XC_EBADARG, "xc_contour_folds: bad arguments");
    XC_TRY(co_check_select(ctx, "xc_contour_folds", periodic, select));
    if (ncont < 1 || nrange % ncont != 0) return fail(ctx, XC_EBADARG, "xc_contour_folds: nrange must be a multiple of ncont >= 1");
    if (gap < 0 || gap >= nx) return fail(ctx, XC_EBADARG, "xc_contour_folds: gap must lie in [0, nx)");
    if (capacity > 0 && (!c_west || !c_east || !ncol || !ncross_max || !ev_row_lo || !ev_row_hi || !nodes || !area || !mx_ || !my_))
        return fail(ctx, XC_EBADARG, "xc_contour_folds: capacity > 0 needs the event arrays");
    if (capacity > 0 && (f == nullptr) != (integral == nullptr)) return fail(ctx, XC_EBADARG, "xc_contour_folds: f and integral go together");
    if (f && f_dtype != XC_F32 && f_dtype != XC_F64) return fail(ctx, XC_EBADARG, "xc_contour_folds: f_dtype is XC_F32 or XC_F64");
    XC_TRY(co_check_plane(ctx, "xc_contour_folds", periodic, ny, nx));
    if (nrange > ((int64_t)1 << 38) / nx) return fail(ctx, XC_EBADARG, "xc_contour_folds: nrange nx must stay below 2^38");
    const long long E = 2 * ny * nx;
    const int wrap = periodic ? 1 : 0;
    const int64_t nslab = nrange / ncont;
    if (nslab > 65535) return fail(ctx, XC_EBADARG, "xc_contour_folds: more than 65535 slabs");
    const bool sums = capacity > 0;                                          // a count-only call needs neither the fold scan nor w and f
    CpProfile& prof = ctx->prof_cfold;
    profile_clear(prof);

    CpPlan pl;                                                               // (no group without segments: the outputs are written all the same)
    XC_TRY(cp_plan(ctx, "xc_contour_folds", nrange, count, nullptr, e_from, e_to, pts, E, pl));
    CiPlanes m(ny, nx, nrange);
    const int64_t wpr = m.geo.wpr, ncb = m.geo.ncb, nchunk = m.geo.nchunk, rc = m.geo.rc;
    const int64_t emax = (nx + 1) / 2, ncol_all = nrange * nx;
    const size_t nslot = (size_t)nrange * (size_t)emax, gslot = (size_t)pl.gmax * (size_t)emax;
    // workspace: off | key, nsel, mx, err (cleared together) | eoff | lo, hi [nrange][nx] | the staging slots [nrange][emax] |
    //            acc, cnt, flg [gmax][emax] (cleared per group) | bits[gmax][ny][wpr] | cpar[gmax][nchunk][wpr] | the tail (xc_cpiece_link.h)
    long long *d_off, *eoff; int *d_err, *lo, *hi, *flg; unsigned long long *acc, *cnt; size_t b_zero = 0, b_gzero = 0; CfSlots S; CpTail tail;
    auto lay = [&](Carve c) {
        d_off = c.take<long long>((size_t)nrange + 1);
        b_zero = c.mark();
        m.carve_words(c, nrange, nslab);
        d_err = c.take<int>(CP_SMALL);
        b_zero = c.mark() - b_zero;
        eoff = c.take<long long>((size_t)nrange + 1);
        lo = c.take<int>((size_t)ncol_all); hi = c.take<int>((size_t)ncol_all);
        S.c_west = c.take<int>(nslot); S.c_east = c.take<int>(nslot); S.ncol = c.take<int>(nslot); S.nmax = c.take<int>(nslot);
        S.row_lo = c.take<unsigned long long>(nslot); S.row_hi = c.take<unsigned long long>(nslot);
        S.nodes = c.take<long long>(nslot * 2); S.sums = c.take<double>(nslot * CF_NSUM * 2);
        b_gzero = c.mark();
        acc = c.take<unsigned long long>(gslot * CF_ACC); cnt = c.take<unsigned long long>(gslot * 2); flg = c.take<int>(gslot);
        b_gzero = c.mark() - b_gzero;
        m.carve_planes(c, pl.gmax);
        cp_carve_tail(c, pl, 6, tail);
        return c.at;
    };
    XC_TRY(lay_out(ctx, &ctx->cpiece_ws, &ctx->cpiece_ws_bytes, lay));

    StageTimer tm(ctx, prof.ms);                                             // where the time goes (xc_set_kernel_timing)
    CpRun run(ctx, tm, pl, e_from, e_to, d_off, tail, d_err);

    const dim3 blk(CP_TPB);
    const int64_t npl = ny * nx;
    // the run pass of the ranges [a, b)
    auto runs = [&](int64_t a, int64_t b) -> int {
        for (int64_t ra = a; ra < b; ra += 65535 * 1024) {
            const int64_t nr = std::min<int64_t>(65535 * 1024, b - ra);
            hipLaunchKernelGGL(k_cf_runs, dim3((unsigned)nr), dim3(CI_TPB), 0, ctx->stream, ra, nx, (int)gap, wrap, emax, (const int*)ncross, row_lo,
                               row_hi, (int*)col_event, (unsigned long long*)event_count, S);
            XC_HIP(ctx, hipGetLastError());
        }
        return XC_OK;
    };

    tm.mark(-1);
    XC_HIP(ctx, hipMemsetAsync(m.key, 0, b_zero, ctx->stream));
    hipLaunchKernelGGL(k_cf_init, dim3(cp_blocks(ncol_all)), blk, 0, ctx->stream, ncol_all, (int*)ncross, row_lo, row_hi, lo, hi);
    XC_HIP(ctx, hipGetLastError());
    tm.mark(3);
    if (sums) {
        ci_launch_bound(ctx->stream, npl, nslab, w, w_per_slab, f, f_dtype, m.mx);
        XC_HIP(ctx, hipGetLastError());
        tm.mark(5);
    }
    XC_TRY(run.upload_off());
    XC_TRY(run.fill_table());
    tm.mark(0);
    int64_t done = 0;                                                       // the ranges whose runs stand
    for (const CpGroup& g : pl.groups) {
        const int64_t ng = g.r1 - g.r0;
        if (ng * ncb * nchunk >= ((int64_t)1 << 31)) return fail(ctx, XC_EBADARG, "xc_contour_folds: a group of too many ranges (lower xc_set_cpiece_workspace)");
        CoRoles s;
        XC_TRY(ci_mark_group(run, g, m, wrap, nx, pts, select, s));
        hipLaunchKernelGGL(k_cf_rows, run.grid, blk, 0, ctx->stream, run.n, run.s0, g.r0, E, nx, select, run.e_from, run.e_to, pts, tail.tab,
                           tail.rid, s.root, run.b.prv, run.b.lab, s.pn, s.pw, m.key, row_lo, row_hi);
        XC_HIP(ctx, hipGetLastError());
        tm.mark(3);
        XC_TRY(run.end());
        const dim3 sgrid((unsigned)(ng * ncb * nchunk));
        hipLaunchKernelGGL(k_cf_cols, sgrid, dim3(CI_TPB), 0, ctx->stream, g.r0, ny, nx, wpr, ncb, rc, nchunk, m.bits, (int*)ncross, lo, hi);
        XC_HIP(ctx, hipGetLastError());
        tm.mark(3);
        XC_TRY(runs(done, g.r1));
        done = g.r1;
        tm.mark(4);
        if (!sums) continue;
        XC_HIP(ctx, hipMemsetAsync(acc, 0, b_gzero, ctx->stream));
        if (nchunk > 1) {
            const int64_t nwords = ng * nchunk * wpr;
            hipLaunchKernelGGL(k_ci_chunk, dim3(cp_blocks(nwords)), blk, 0, ctx->stream, nwords, ny, wpr, rc, nchunk, m.bits, m.cpar);
            XC_HIP(ctx, hipGetLastError());
        }
#define XC_CF_SCAN(FT_) hipLaunchKernelGGL((k_cf_scan<FT_>), sgrid, dim3(CI_TPB), 0, ctx->stream, g.r0, ny, nx, wpr, ncb, rc, nchunk, ncont, emax, m.bits, \
                                           m.cpar, (const int*)col_event, lo, hi, S.c_west, w, w_per_slab, (const FT_*)f, m.mx, acc, cnt, flg)
        if (!f) XC_CF_SCAN(void); else if (f_dtype == XC_F32) XC_CF_SCAN(float); else XC_CF_SCAN(double);
#undef XC_CF_SCAN
        XC_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_cf_finish, dim3(cp_blocks(ng * emax)), blk, 0, ctx->stream, g.r0, ng, ny, nx, ncont, emax, f ? 1 : 0,
                           (const unsigned long long*)event_count, acc, cnt, flg, m.mx, S);
        XC_HIP(ctx, hipGetLastError());
        tm.mark(5);
    }
    if (done < nrange) XC_TRY(runs(done, nrange));
    run.report(prof);
    hipLaunchKernelGGL(k_cf_offsets, dim3(1), blk, 0, ctx->stream, nrange, (const unsigned long long*)event_count, eoff);
    XC_HIP(ctx, hipGetLastError());
    tm.mark(4);
    // the second round trip: the event counts (and whether the records were K12's)
    std::vector<uint64_t> hec((size_t)nrange);
    int herr = 0;
    XC_HIP(ctx, hipMemcpyAsync(hec.data(), event_count, (size_t)nrange * 8, hipMemcpyDeviceToHost, ctx->stream));
    XC_TRY(cp_read_err(ctx, d_err, &herr));
    if (herr) return fail(ctx, XC_EBADARG, "xc_contour_folds: an edge id outside [0, 2 ny nx)");
    long long total = 0;
    for (int64_t r = 0; r < nrange; ++r) total += (long long)hec[(size_t)r];
    if (total > capacity) return 1;
    if (total == 0) return XC_OK;
    tm.mark(-1);
    hipLaunchKernelGGL(k_cf_compact, dim3(cp_blocks(total)), blk, 0, ctx->stream, (int64_t)total, nrange, emax, eoff, S, (int*)c_west, (int*)c_east,
                       (int*)ncol, (int*)ncross_max, ev_row_lo, ev_row_hi, (long long*)nodes, area, mx_, my_, integral);
    XC_HIP(ctx, hipGetLastError());
    tm.mark(5);
    return XC_OK;
}

}  // namespace xc

// ------------------------------------------------------------------------------------ C ABI
int xc_contour_folds_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to, const double* pts,
                         int64_t ny, int64_t nx, int periodic, int select, int ncont, const double* w, int w_per_slab, const void* f,
                         int f_dtype, int64_t gap, int32_t* ncross, double* row_lo, double* row_hi, int32_t* col_event, int64_t capacity,
                         uint64_t* event_count, int32_t* c_west, int32_t* c_east, int32_t* ncol, int32_t* ncross_max, double* ev_row_lo,
                         double* ev_row_hi, int64_t* nodes, double* area, double* mx, double* my, double* integral)
{
    XC_CTX(ctx);
    return xc::launch_contour_folds(ctx, nrange, count, e_from, e_to, pts, ny, nx, periodic, select, ncont, w, w_per_slab, f, f_dtype, gap,
                                    ncross, row_lo, row_hi, col_event, capacity, event_count, c_west, c_east, ncol, ncross_max, ev_row_lo,
                                    ev_row_hi, nodes, area, mx, my, integral);
}

int xc_last_cfold_profile(xc_ctx* ctx, double* ms, int* rounds, int* groups)
{
    return xc::profile_get(ctx, &xc_ctx::prof_cfold, 6, ms, rounds, groups);
}

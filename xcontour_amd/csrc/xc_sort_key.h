// K8, the keys: order-preserving key of a tracer value, the pairs of pass 0, the 24-bit range key of the float64 passes and the
// three kernels that prepare it.  Included INSIDE `namespace xc { namespace {` of xc_sort.hip, which defines u32 / u64 and
// wave_incl_scan ahead of it.
#pragma once

template <typename K> struct KeyTraits;
template <> struct KeyTraits<u64> {
    static constexpr int passes = 8;
    __device__ static __forceinline__ u64 invalid() { return ~0ull; }
    __device__ static __forceinline__ u64 encode(double v)
    {
        // order-preserving map of IEEE doubles to unsigned integers; -0.0 is folded onto +0.0 so that
        // equal values keep their original order exactly like numpy's stable sort
        const u64 u = (u64)__double_as_longlong(v == 0.0 ? 0.0 : v);
        return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    }
    __device__ static __forceinline__ double decode(u64 k)
    {
        const u64 u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
        return __longlong_as_double((long long)u);
    }
};
template <> struct KeyTraits<u32> {            // float32 tracers: the key of the float IS the order of its double
    static constexpr int passes = 4;
    __device__ static __forceinline__ u32 invalid() { return ~0u; }
    __device__ static __forceinline__ u32 encode(double v)
    {
        const float f = (float)v;              // exact: v came from a float (possibly negated)
        const u32 u = (u32)__float_as_int(f == 0.0f ? 0.0f : f);
        return (u >> 31) ? ~u : (u | 0x80000000u);
    }
    __device__ static __forceinline__ double decode(u32 k)
    {
        const u32 u = (k >> 31) ? (k & 0x7fffffffu) : ~k;
        return (double)__int_as_float((int)u);
    }
};

// the (key, payload) pairs of TILE_ROUNDS cells per lane, straight from the tracer / mask / dA: pass 0 of the sort builds its
// pairs with this, so the unsorted pairs are never written and read back (24-32 B per cell).  Phases, not a per-cell
// function: every load of a stream is issued before the first use (clamped addresses, wave-uniform branches only), and a
// per-row dA divides in 32 bits (n < 2^31).
template <typename TQ, typename TM, typename K, int R, bool VALS>
__device__ __forceinline__ void load_pairs(const TQ* __restrict__ q, const TM* __restrict__ mask, const double* __restrict__ dA,
                                           int dA_rank, int64_t nx, int negate, int64_t base, int lane, int64_t n,
                                           K (&key)[R], double (&val)[R])
{
    TQ qv[R];
    TM mv[R];
    unsigned idx[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { const int64_t i = base + r * 64 + lane; idx[r] = (unsigned)(i < n ? i : n - 1); qv[r] = q[idx[r]]; }
    if (mask) {
#pragma unroll
        for (int r = 0; r < R; ++r) mv[r] = mask[idx[r]];
    }
    if (VALS) {
        if (dA_rank == XC_DA_PLANE) {
#pragma unroll
            for (int r = 0; r < R; ++r) val[r] = dA[idx[r]];
        } else if (dA_rank == XC_DA_ROW) {
            const unsigned unx = (unsigned)nx;
#pragma unroll
            for (int r = 0; r < R; ++r) val[r] = dA[idx[r] / unx];
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) val[r] = 1.0;
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const double v = negate ? -(double)qv[r] : (double)qv[r];
        const bool ok = (v == v) && (!mask || mv[r] == (TM)1) && (base + r * 64 + lane < n);
        key[r] = ok ? KeyTraits<K>::encode(v) : KeyTraits<K>::invalid();       // dropped cells sort to the end
        if (VALS) val[r] = ok ? val[r] : 0.0;
    }
}
struct PairSrc {                 // where pass 0 finds its input (per-slab strides applied by the kernels)
    const void* q; const void* mask; const double* dA;
    int dA_rank, negate; int64_t nx, mask_stride, dA_stride;
    const double* mm;            // [nslab][4] min, max, robust low, robust high of the tracer (K1 + k_range_bounds): the range-key passes only
    const unsigned* rtab;        // [nslab][2 * RANGE_NB] first range key and number of range keys of every coarse bin
};

// ---- the 24-bit range key (MODE 1 of the passes).  Valid values map to [0, 2^24 - 2] monotonically, dropped cells
// (key == invalid) to 2^24 - 1, so that they gather behind every valid value without sharing a run with the maximum.
// The map is piecewise linear: the value range is cut into RANGE_NB equal coarse bins and every bin gets a share of the 2^24
// range keys proportional to its POPULATION (histogram equalisation: k_range_hist counts, k_range_table divides), so a
// plateau that holds a third of the cells inside a thousandth of the range -- a well-mixed layer, a saturating tanh profile --
// is still resolved to ~2^-30 of the range and its runs of equal range key stay short.  Monotone: x = (v - lo) * S is
// monotone in v, so are b = floor(x) and, inside a bin, x - b (exact) and floor((x - b) * width); bins do not overlap.
constexpr unsigned RANGE_INVALID = 0xFFFFFFu;
constexpr int RANGE_NB = 256;
constexpr int RANGE_SAMPLE = 16;       // k_range_hist looks at one 2048-cell chunk in 16: any positive widths give a monotone map, the
                                        // populations only have to be roughly right for the runs to come out short
// Three zones (round 4).  The 256 equalised coarse bins cover the ROBUST range [rlo, rhi] of the plane -- the 9th smallest of
// the K1 block minima to the 9th largest of the block maxima (k_range_bounds) -- and the cells outside it (a handful: the block
// extrema are extreme order statistics of the plane) get 2^16 keys each, linear over [min, rlo) and (rhi, max].  With the exact
// min / max as the ends of the equalised range (round 3) ONE stray cell -- an unmasked fill value, a spike -- stretched the range,
// the whole field fell into one coarse bin and the sort fell back to eight passes (0.95 ms against 0.38).  Monotone as before:
// the zones are ordered, each map is monotone inside its zone.
constexpr unsigned RANGE_WOUT = 65536u;                                   // keys of each outer zone
constexpr unsigned RANGE_WIN = 16777215u - 2u * RANGE_WOUT;               // keys of the equalised inner zone: [WOUT, WOUT + WIN)
struct RangeMap { double lo, scale, mn, s_lo, hi, s_hi; const unsigned* tab; };      // tab: the slab's table, staged in LDS by the kernel
__device__ __forceinline__ void range_params(const double* __restrict__ mm, int slab, int negate, RangeMap& r)
{
    const double a = mm[4 * slab], b = mm[4 * slab + 1], c = mm[4 * slab + 2], d = mm[4 * slab + 3];    // min, max, robust low, robust high
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    r.mn = negate ? -b : a;
    const double mx = negate ? -a : b;
    r.lo = negate ? -d : c;
    r.hi = negate ? -c : d;
    const double w = r.hi - r.lo, wl = r.lo - r.mn, wh = mx - r.hi;
    r.scale = (w > 0.0 && w < inf) ? (double)RANGE_NB / w : (w == 0.0 ? 1e300 : 0.0);   // constant robust range: strays still leave it (x = +-huge); empty / infinite range: one bin
    r.s_lo = (wl > 0.0 && wl < inf) ? (double)RANGE_WOUT / wl : 0.0;
    r.s_hi = (wh > 0.0 && wh < inf) ? (double)RANGE_WOUT / wh : 0.0;
}
// coarse bin of the equalised zone: x = (v - rlo) * scale, xc = x clamped to [0, RANGE_NB] (the last bin takes x = 256)
__device__ __forceinline__ int range_bin(double v, double lo, double scale, double& x, double& xc)
{
    x = (v - lo) * scale;                                               // NaN (inf - inf, 0 * inf) -> inner bin 0 below
    xc = fmin(fmax(x, 0.0), (double)RANGE_NB);
    return (int)fmin(xc, (double)(RANGE_NB - 1));
}
// stage the slab's table in LDS (2 * RANGE_NB words); the caller synchronises before the first range_key
__device__ __forceinline__ RangeMap range_map(const PairSrc& src, int slab, unsigned* s_tab)
{
    RangeMap r;
    range_params(src.mm, slab, src.negate, r);
    const unsigned* g = src.rtab + (size_t)slab * 2 * RANGE_NB;
    for (int i = threadIdx.x; i < 2 * RANGE_NB; i += blockDim.x) s_tab[i] = g[i];
    r.tab = s_tab;
    return r;
}
template <typename K>
__device__ __forceinline__ unsigned range_key(K key, const RangeMap& m)
{
    if (key == KeyTraits<K>::invalid()) return RANGE_INVALID;
    const double v = KeyTraits<K>::decode(key);
    // the zone follows from x = (v - rlo) * scale itself: x < 0 below the robust range, x > 256 above it (a value a rounding
    // away from an end may stay inside: it then shares the end key, which keeps the map monotone); one compare on the hot path.
    // A degenerate robust range (a constant field with strays) has scale = 1e300 (range_params): x is 0 or +-huge.
    double x, xc;
    const int b = range_bin(v, m.lo, m.scale, x, xc);
    const unsigned first = m.tab[2 * b], width = m.tab[2 * b + 1];
    const double f = fmin(xc - (double)b, 1.0) * (double)width;          // (x - b in [0, 1]; the last bin takes x = 256)
    const unsigned off = (unsigned)f;
    unsigned k = first + (off < width ? off : width - 1u);
    // a cell outside the robust range (x NaN: stays in bin 0).  The test is made WAVE-uniform so that it stays a branch: written
    // per lane, the compiler predicates the two outer-zone maps into every key evaluation (+14 instructions per key and pass:
    // measured +30 us on the 6.48 M-pair sort); a handful of waves per plane ever take it.
    if (__ballot(xc != x) != 0ull) {
        if (x < 0.0) k = (unsigned)fmin(fmax((v - m.mn) * m.s_lo, 0.0), (double)(RANGE_WOUT - 1u));
        else if (x > (double)RANGE_NB) k = RANGE_WOUT + RANGE_WIN + (unsigned)fmin(fmax((v - m.hi) * m.s_hi, 0.0), (double)(RANGE_WOUT - 1u));
    }
    return k;
}
template <typename K, int MODE>
__device__ __forceinline__ unsigned digit_of(K key, int shift, const RangeMap& m)
{
    if (MODE == 0) return (unsigned)((key >> shift) & (K)255);
    return (range_key<K>(key, m) >> shift) & 255u;
}

// min, max and the ROBUST range of every plane from the per-block partials of K1 ([nslab][P][2]; a block = a contiguous piece
// of the plane): consecutive blocks are folded into at most 512 groups, dealt round-robin to the eight waves of the workgroup;
// every wave names its TWO smallest group minima and two largest group maxima (two rounds of a shuffle tree with retirement), and
// the T-th smallest / largest of those 16 candidates (T = 9; fewer than 72 groups: an eighth of them, at least 1 = the exact
// extrema) bounds the robust range: up to eight stray-holding groups are trimmed wherever they sit, and a candidate is never
// below the true T-th smallest group minimum, so the handful of cells outside [rlo, rhi] only grows by a few groups' worth when
// the extremes cluster in one wave's share.  (Exact selection by rank counting over all groups: 11-24 us per call; this: ~3.)
// out: [nslab][4] = min, max, rlo, rhi (all-NaN plane: NaN).
__global__ __launch_bounds__(512)
void k_range_bounds(const double* __restrict__ part, int P, double* __restrict__ out, unsigned* __restrict__ rhist, unsigned* __restrict__ tick)
{
    __shared__ double s_c[2][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // (round 5) this kernel runs before the sampled population is counted: it clears the slab's coarse histogram and the arrival
    // tickets of the later kernels itself -- one hipMemsetAsync less in a chain of ~20 dependent launches
    if (tid < RANGE_NB) rhist[(size_t)blockIdx.x * RANGE_NB + tid] = 0u;
    if (tid < 4) tick[(size_t)blockIdx.x * 4 + tid] = 0u;
    const double* mp = part + (size_t)blockIdx.x * P * 2;
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    const int per = (P + 511) / 512, ng = (P + per - 1) / per;           // groups of `per` consecutive blocks
    const int g = lane * 8 + wave;                                       // group of this thread: round-robin over the waves
    double a = inf, b = -inf;
    if (g < ng)
        for (int i = g * per; i < (g + 1) * per && i < P; ++i) { a = fmin(a, mp[2 * i]); b = fmax(b, mp[2 * i + 1]); }
    for (int r = 0; r < 2; ++r) {
        double lo = a, hi = b;
        for (int o = 32; o > 0; o >>= 1) { lo = fmin(lo, __shfl_xor(lo, o)); hi = fmax(hi, __shfl_xor(hi, o)); }
        if (lane == 0) { s_c[0][wave * 2 + r] = lo; s_c[1][wave * 2 + r] = hi; }
        const unsigned long long wa = __ballot(a == lo), wb = __ballot(b == hi);          // retire ONE holder of each extreme
        if (wa && lane == __builtin_ctzll(wa)) a = inf;
        if (wb && lane == __builtin_ctzll(wb)) b = -inf;
    }
    __syncthreads();
    if (tid < 16) {
        const double ca = s_c[0][tid], cb = s_c[1][tid];
        int below = 0, above = 0;                                         // strict rank among the 16 candidates, index as the tie-break
        for (int i = 0; i < 16; ++i) {
            const double x = s_c[0][i], y = s_c[1][i];
            below += (x < ca) || (x == ca && i < tid);
            above += (y > cb) || (y == cb && i < tid);
        }
        const int T = ng >= 72 ? 9 : (ng / 8 > 0 ? ng / 8 : 1);
        double* o = out + (size_t)blockIdx.x * 4;
        if (below == 0) o[0] = ca;
        if (above == 0) o[1] = cb;
        if (below == T - 1) o[2] = ca;
        if (above == T - 1) o[3] = cb;
    }
    __syncthreads();                                                      // (same workgroup: the stores above are visible to thread 0 below)
    if (tid == 0) {
        double* o = out + (size_t)blockIdx.x * 4;
        double lo0 = o[0], hi0 = o[1], c = o[2], d = o[3];
        if (lo0 == inf && hi0 == -inf) { lo0 = hi0 = c = d = __longlong_as_double(0x7ff8000000000000LL); }     // no valid cell
        else {
            if (!(c >= lo0) || c == inf || c == -inf) c = lo0;           // candidates without a valid cell carry +inf / -inf: fall back to the extrema
            if (!(d <= hi0) || d == inf || d == -inf) d = hi0;
            if (!(c <= d)) { c = lo0; d = hi0; }
        }
        o[0] = lo0; o[1] = hi0; o[2] = c; o[3] = d;
    }
}

// what k_range_hist samples: the first 256 cells of every 256 * samp (small planes: every cell), nseg such segments
struct RangeSample { int64_t samp, nseg; };
__host__ __device__ inline RangeSample range_sample(int64_t n)
{
    const int64_t samp = n > (int64_t)256 * RANGE_SAMPLE * 64 ? RANGE_SAMPLE : 1;
    return {samp, (n + 256 * samp - 1) / (256 * samp)};
}
// population of the RANGE_NB coarse bins (valid cells only, the validity rule of load_pairs); hist was cleared by k_range_bounds
template <typename TQ, typename TM>
__global__ __launch_bounds__(256)
void k_range_hist(int64_t n, const PairSrc src, unsigned* __restrict__ hist)
{
    __shared__ unsigned s_h[RANGE_NB];
    for (int i = threadIdx.x; i < RANGE_NB; i += 256) s_h[i] = 0;
    RangeMap rp;
    range_params(src.mm, blockIdx.y, src.negate, rp);
    const double lo = rp.lo, hi = rp.hi, scale = rp.scale;
    const TQ* q = (const TQ*)src.q + (size_t)blockIdx.y * n;
    const TM* mask = src.mask ? (const TM*)src.mask + (size_t)blockIdx.y * src.mask_stride : nullptr;
    __syncthreads();
    constexpr int U = 8;
    const RangeSample rs = range_sample(n);
    const int64_t samp = rs.samp, nseg = rs.nseg;
    for (int64_t s0 = (int64_t)blockIdx.x * U; s0 < nseg; s0 += (int64_t)gridDim.x * U) {
        TQ qv[U]; TM mv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { const int64_t i = (s0 + u) * 256 * samp + threadIdx.x; qv[u] = q[i < n ? i : n - 1]; }
        if (mask) {
#pragma unroll
            for (int u = 0; u < U; ++u) { const int64_t i = (s0 + u) * 256 * samp + threadIdx.x; mv[u] = mask[i < n ? i : n - 1]; }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = (s0 + u) * 256 * samp + threadIdx.x;
            const double v = src.negate ? -(double)qv[u] : (double)qv[u];
            if (s0 + u < nseg && i < n && v >= lo && v <= hi && (!mask || mv[u] == (TM)1)) { double x, xc; atomicAdd(&s_h[range_bin(v, lo, scale, x, xc)], 1u); }   // (the robust range only; NaN fails both compares)
        }
    }
    __syncthreads();
    unsigned* h = hist + (size_t)blockIdx.y * RANGE_NB;
    for (int i = threadIdx.x; i < RANGE_NB; i += 256) if (s_h[i]) atomicAdd(&h[i], s_h[i]);
}

// counts -> (first range key, number of range keys) per coarse bin: HALF of the 2^24 - 1 keys are dealt out evenly (a bin the
// sample missed still resolves 2^-23 of the range), the other half in proportion to the sampled counts (rounded down: the
// last key used is at most 2^24 - 2)
__global__ __launch_bounds__(RANGE_NB)
void k_range_table(const unsigned* __restrict__ hist, unsigned* __restrict__ rtab)
{
    __shared__ unsigned s_w[(RANGE_NB + 63) / 64];
    __shared__ unsigned long long s_tot;
    const int b = threadIdx.x, lane = b & 63, wave = b >> 6;
    const unsigned c = hist[(size_t)blockIdx.x * RANGE_NB + b];
    unsigned long long t = c;
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
    if (b == 0) s_tot = 0ull;
    __syncthreads();
    if (lane == 0) atomicAdd(&s_tot, t);
    __syncthreads();
    const unsigned long long tot = s_tot, even = (RANGE_WIN / 2u) / RANGE_NB, budget = (unsigned long long)RANGE_WIN - even * RANGE_NB;
    const unsigned width = (unsigned)even + (tot ? (unsigned)((unsigned long long)c * budget / tot) : 0u);
    const unsigned x = wave_incl_scan(width, lane);                           // exclusive scan of the widths
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    unsigned first = RANGE_WOUT + x - width;                            // behind the lower outer zone
    for (int w = 0; w < wave; ++w) first += s_w[w];
    rtab[((size_t)blockIdx.x * RANGE_NB + b) * 2] = first;
    rtab[((size_t)blockIdx.x * RANGE_NB + b) * 2 + 1] = width;
}

// The level table and level search of K9 (xc_cross.hip), K10 (xc_clen.hip) and K12 (xc_cseg.hip): a block's ascending levels in
// LDS between two sentinels, and how many of them lie below a value.
// Included inside namespace xc { namespace { ... } } of each translation unit, after xc_binning.h.
#pragma once

// number of contours < v, i.e. the klo with cx[klo] < v <= cx[klo+1]; cx = [-inf, c_0 .. c_{N-1}, +inf]
__device__ __forceinline__ int count_below(const double* __restrict__ cx, int N, double v)
{
    int lo = 0, hi = N;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (cx[mid + 1] < v) lo = mid + 1; else hi = mid; }
    return lo;
}

// Equally spaced levels: number of contours < v from arithmetic.  The block measured how far the levels sit from their ideal
// positions (zlo = twice that, in units of the spacing, plus the rounding of t): when the fractional position of v lies
// outside that zone of either neighbouring level the arithmetic answer IS the count and no LDS read is needed; otherwise
// (v within a hair of a level, NaN, infinities) one adjacent-pair read verifies, bisection is the fallback.
__device__ __forceinline__ int count_below_uniform(const double* __restrict__ cx, int N, double v, double c_first,
                                                   double inv_step, double zlo)
{
    const double t = (v - c_first) * inv_step;
    int k = (int)fmin(fmax(t + 1.0, 0.0), (double)N);          // floor(t) + 1 clamped to [0, N]; NaN -> 0
    const double fr = __builtin_amdgcn_fract(t);
    if (!((fr > zlo) & (fr < 1.0 - zlo))) {
        const double c_lo = cx[k], c_hi = cx[k + 1];
        if (!((c_lo < v) & (v <= c_hi))) k = count_below(cx, N, v);
    }
    return k;
}

// How a block searches its level table: inv_step > 0: equally spaced levels, by arithmetic (count_below_uniform); 0: bisection.
struct LevelSearch {
    double c_first, inv_step, zlo;
    // the crossed range of [mn, mx): the levels k with mn <= c_k < mx are klo .. khi - 1
    __device__ __forceinline__ void crossed(const double* __restrict__ cx, int N, double mn, double mx, int& klo, int& khi) const
    {
        if (inv_step > 0.0) {
            klo = count_below_uniform(cx, N, mn, c_first, inv_step, zlo);
            khi = count_below_uniform(cx, N, mx, c_first, inv_step, zlo);
        } else {
            klo = count_below(cx, N, mn);
            khi = count_below(cx, N, mx);
        }
    }
};

// A block of TPB threads loads its ng levels: s_cx[0 .. ng + 1] = -inf, cs[0 .. ng - 1], +inf.  Every thread of the block calls it;
// its first barrier also publishes what the caller wrote to LDS before the call.  Equally spaced?  is a block-uniform answer; zlo is
// twice the largest distance of a level from its ideal position, in units of the spacing, plus the rounding of t itself
// (|t| <= ~N: 1e-13 at most).
template <int TPB>
__device__ __forceinline__ LevelSearch load_levels(const double* __restrict__ cs, int ng, double* __restrict__ s_cx)
{
    __shared__ double s_dev[TPB / 64];
    const int tid = threadIdx.x;
    const double inf = dinf();
    for (int k = tid; k < ng; k += TPB) s_cx[k + 1] = cs[k];
    if (tid == 0) { s_cx[0] = -inf; s_cx[ng + 1] = inf; }
    __syncthreads();
    LevelSearch ls;
    ls.c_first = s_cx[1];
    ls.inv_step = (ng > 1) ? (double)(ng - 1) / (s_cx[ng] - ls.c_first) : 0.0;
    if (!(ls.inv_step > 0.0 && ls.inv_step < inf)) ls.inv_step = 0.0;
    int ok = ls.inv_step > 0.0;
    double dev = 0.0;
    for (int k = tid; k < ng && ok; k += TPB) {
        const double d = fabs((s_cx[k + 1] - ls.c_first) * ls.inv_step - (double)k);
        ok = d < 0.01; dev = fmax(dev, d);
    }
    if (!__syncthreads_and(ok)) ls.inv_step = 0.0;
    for (int o = 32; o > 0; o >>= 1) dev = fmax(dev, __shfl_xor(dev, o));
    if ((tid & 63) == 0) s_dev[tid >> 6] = dev;
    __syncthreads();
    dev = s_dev[0];
    for (int w = 1; w < TPB / 64; ++w) dev = fmax(dev, s_dev[w]);
    ls.zlo = 2.0 * dev + 1e-9;
    return ls;
}

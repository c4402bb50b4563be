// Level search shared by K9 (xc_cross.hip) and K10 (xc_clen.hip): how many of N ascending levels lie below a value.
// Included inside namespace xc { namespace { ... } } of each translation unit.
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

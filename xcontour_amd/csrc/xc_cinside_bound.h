// The bounds behind the windows of K17's sums, shared by K17 (xc_cinside.hip), K18-K21 (xc_cprecords.hip) and K22 (xc_cpoverlap.hip);
// xc_cinside.hip's header states the rule: the window's top sits 12 bits above max |w| (max |w f|) over the finite values of the slab.
// Included inside namespace xc { namespace { ... } } after xc_binning.h and xc_cpiece_sum.h; the including file includes <type_traits>.
#pragma once

constexpr int CI_TPB = 256;                   // the columns of one block of K17's scan; the block of k_ci_bound
constexpr unsigned long long CI_INF = 0x7ff0000000000000ull;

__device__ __forceinline__ unsigned long long ci_wave_max(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const unsigned long long o = __shfl_xor(v, d); v = o > v ? o : v; }
    return v;
}

// the bit patterns of max |w| and max |w f| over the finite values of every slab: mx[2 s], mx[2 s + 1] (0 at the start).  FT: the type of f
// (void: none)
template <typename FT>
__global__ __launch_bounds__(CI_TPB)
void k_ci_bound(int64_t npl, const double* __restrict__ w, int w_per_slab, const FT* __restrict__ f, unsigned long long* __restrict__ mx)
{
    constexpr bool HASF = !std::is_void<FT>::value;
    const int64_t s = blockIdx.y;
    const double* wp = w ? w + (w_per_slab ? (size_t)s * (size_t)npl : 0) : nullptr;
    unsigned long long mw = 0ull, mf = 0ull;
    for (int64_t i = (int64_t)blockIdx.x * CI_TPB + threadIdx.x; i < npl; i += (int64_t)gridDim.x * CI_TPB) {
        const double a = wp ? wp[i] : 1.0;
        const unsigned long long ba = (unsigned long long)__double_as_longlong(fabs(a));
        if (ba < CI_INF && ba > mw) mw = ba;
        if constexpr (HASF) {
            const double t = __dmul_rn(a, (double)f[(size_t)s * (size_t)npl + i]);
            const unsigned long long bt = (unsigned long long)__double_as_longlong(fabs(t));
            if (bt < CI_INF && bt > mf) mf = bt;
        }
    }
    mw = ci_wave_max(mw);
    if constexpr (HASF) mf = ci_wave_max(mf);
    if ((threadIdx.x & 63) == 0) {
        if (mw) atomicMax(mx + 2 * s, mw);
        if constexpr (HASF) if (mf) atomicMax(mx + 2 * s + 1, mf);
    }
}

// k_ci_bound for an integrand of f_dtype (f null: none): at most 1024 blocks a slab
inline void ci_launch_bound(hipStream_t stream, int64_t npl, int64_t nslab, const double* w, int w_per_slab, const void* f, int f_dtype,
                            unsigned long long* mx)
{
    const dim3 bgrid((unsigned)std::min<int64_t>((npl + CI_TPB - 1) / CI_TPB, 1024), (unsigned)nslab);
    if (!f) hipLaunchKernelGGL((k_ci_bound<void>), bgrid, dim3(CI_TPB), 0, stream, npl, w, w_per_slab, (const void*)nullptr, mx);
    else if (f_dtype == XC_F32) hipLaunchKernelGGL((k_ci_bound<float>), bgrid, dim3(CI_TPB), 0, stream, npl, w, w_per_slab, (const float*)f, mx);
    else hipLaunchKernelGGL((k_ci_bound<double>), bgrid, dim3(CI_TPB), 0, stream, npl, w, w_per_slab, (const double*)f, mx);
}

// the top of a window from the bit pattern of the bound on one term
__device__ __forceinline__ int ci_top(unsigned long long bound_bits) { return cp_top(det_c0_from_bound(__longlong_as_double((long long)bound_bits))); }

// The field table of K21, shared by K21 (xc_cpiece_props.h, xc_cprecords.hip) and K28 (xc_cdist_profile.h): how a call's fields reach the
// kernels, how a kernel reads one, and the pass that leaves max |w g_m| over the finite values of every (slab, field) -- the tops of the
// windows of the fields' sums.  Included inside namespace xc { namespace { ... } } after xc_cpiece_sum.h and xc_cinside_bound.h.
#pragma once

// one field plane as the kernels read it (a table of the call's fields on the device; the extremum field is entry nf)
struct PpField {
    const void* p;
    unsigned long long stride;    // elements between two slabs: ny nx, or 0 for a plane all slabs share
    int f32, pad;
};

__device__ __forceinline__ double pp_load(const PpField& f, size_t slab, size_t node)
{
    const size_t i = (size_t)f.stride * slab + node;
    return f.f32 ? (double)((const float*)f.p)[i] : ((const double*)f.p)[i];
}

// mxg[s][m]: the bit pattern of max |w g_m| over the finite values of slab s (0 at the start); grid (blocks, nslab, nf)
__global__ __launch_bounds__(CI_TPB)
void k_pp_bound(int64_t npl, int nf, const double* __restrict__ w, int w_per_slab, const PpField* __restrict__ fld,
                unsigned long long* __restrict__ mxg)
{
    const int64_t s = blockIdx.y;
    const int m = blockIdx.z;
    const PpField f = fld[m];
    const double* wp = w ? w + (w_per_slab ? (size_t)s * (size_t)npl : 0) : nullptr;
    unsigned long long mf = 0ull;
    for (int64_t i = (int64_t)blockIdx.x * CI_TPB + threadIdx.x; i < npl; i += (int64_t)gridDim.x * CI_TPB) {
        const double t = __dmul_rn(wp ? wp[i] : 1.0, pp_load(f, (size_t)s, (size_t)i));
        const unsigned long long bt = (unsigned long long)__double_as_longlong(fabs(t));
        if (bt < CI_INF && bt > mf) mf = bt;
    }
    mf = ci_wave_max(mf);
    if ((threadIdx.x & 63) == 0 && mf) atomicMax(mxg + (size_t)s * nf + m, mf);
}

// the tops of the windows of the nf fields; at most 1024 blocks a slab and field
inline void pp_launch_bound(hipStream_t stream, int64_t npl, int64_t nslab, int nf, const double* w, int w_per_slab, const PpField* fld,
                            unsigned long long* mxg)
{
    const dim3 ggrid((unsigned)std::min<int64_t>((npl + CI_TPB - 1) / CI_TPB, 1024), (unsigned)nslab, (unsigned)nf);
    hipLaunchKernelGGL(k_pp_bound, ggrid, dim3(CI_TPB), 0, stream, npl, nf, w, w_per_slab, fld, mxg);
}

// K7 -- local finite-amplitude wave activity / local APE (gfx950).
//
// Replaces the J-iteration python loop of Contour2D.cal_local_wave_activity
// (reference core.py:752-791): for every target row j and column x
//     lwa[j,x] = - sum_{y'} (q[y',x] - Q[j]) * mask3(j,y',x) * (dA[y',x]/dAmax) * M[y',x]
// with mask3 in {-1,0,1} from the sign of qe and the side of row j (core.py:757-766)
// and the part selection of core.py:773-784 (masked-out cells are NaN there and are
// skipped by the sum, i.e. contribute nothing).
//
// Mapping: lanes run along X (coalesced row reads), each thread keeps JT target rows in
// registers and streams the column once per JT targets; the y' loop is sequential, the
// same order numpy's axis-0 nansum uses, so results are reproducible bit for bit.
//
// This file: k_lwa_masks, the plan (which kernels a call takes, with what geometry) and the launcher.  The kernels are in xc_lwa_walk.h
// (the bit-exact band walk: k_lwa_prep + k_lwa, k_lwa_strip) and xc_lwa_fast.h (the interval kernel: k_lwa_check + k_lwa_fast).
#include "xc_capi.h"
#include <type_traits>

namespace xc {
namespace {

#include "xc_binning.h"
#include "xc_lwa_walk.h"
#include "xc_lwa_fast.h"

__device__ __forceinline__ int mask3(double qe, bool m, int increase)
{
    // core.py:759-766
    const bool neg = increase ? (qe > 0.0) : (qe < 0.0);   // -> -1 on the far side
    const bool pos = increase ? (qe < 0.0) : (qe > 0.0);   // -> +1 on the near side
    return (pos && m) ? 1 : (m ? 0 : (neg ? -1 : 0));
}

template <typename T>
__global__ __launch_bounds__(256)
void k_lwa_masks(const T* __restrict__ q, const double* __restrict__ Q, const double* __restrict__ coord,
                 int64_t ny, int64_t nx, int increase, int v2,
                 const int32_t* __restrict__ mask_idx, int nmask, int8_t* __restrict__ out)
{
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t y = blockIdx.y;
    const int slab = blockIdx.z / nmask, im = blockIdx.z % nmask;
    if (x >= nx) return;
    const int coord_incre = lwa_coord_incre(coord, ny);
    const int64_t j = mask_idx[im];
    const double qe = v2 ? __dsub_rn((double)q[(size_t)slab * ny * nx + j * nx + x], Q[(size_t)slab * ny + y])
                         : __dsub_rn((double)q[(size_t)slab * ny * nx + y * nx + x], Q[(size_t)slab * ny + j]);
    const bool m = coord_incre ? (coord[y] >= coord[j]) : (coord[y] <= coord[j]);      // lwa_near, with the loads inside the arms
    out[(((size_t)slab * nmask + im) * ny + y) * nx + x] = (int8_t)mask3(qe, m, v2 ? !increase : increase);
}

// ---------------------------------------------------------------- the plan
// What one call launches, from its shapes alone (no HIP call in here).  mode (xc_set_lwa_exact): 0 automatic (planes of more than
// kLwaFastMinRows rows take the interval kernel behind its device-side check), 1 the band walk everywhere, 2 the interval kernel for every
// plane (checked), 3 the same with the premises vouched for by the caller (it looked at Q and the coordinate on the host): ONE launch, no
// check, no gated band walk behind it.  Otherwise exactly one band walk is enqueued: the strip kernel or prep + streaming kernel.
struct LwaPlan {
    bool fast;  bool gated;  int CG;  int64_t nvb;  dim3 fast_grid;  size_t fast_lds;      // k_lwa_fast; gated: behind k_lwa_check, the band walk behind both
    bool strip;  int wchunk;  dim3 strip_grid;  size_t strip_lds;                          // k_lwa_strip
    bool stream;  int JT;  dim3 prep_grid, walk_grid;  size_t scratch_bytes;               // k_lwa_prep + k_lwa<.., JT>
    const char* refuse;                                                                    // non-null: the call cannot run
};
LwaPlan lwa_plan(int64_t nslab, int64_t ny, int64_t nx, size_t tsize, int dA_rank, int M_rank, int variant, int mode, int knob_fast,
                 int knob_strip, int cus)
{
    LwaPlan p = {};
    if (cus <= 0) cus = 256;
    const bool want_fast = mode >= 2 || (mode == 0 && knob_fast && (ny > kLwaFastMinRows || knob_fast > 1));
    if (variant == 0 && want_fast && ny * nx < ((int64_t)1 << 29)) {           // (32-bit byte offsets inside a plane: k_lwa_fast)
        for (int c : {4, 2, 1})
            if (!p.CG && lwa_fast_lds(nullptr, (int)ny, c).bytes <= kLdsBudget) p.CG = c;
    }
    if (p.CG) {
        p.fast = true;
        p.gated = mode != 3;
        p.fast_lds = lwa_fast_lds(nullptr, (int)ny, p.CG).bytes;
        const int64_t ngrp = (nx + p.CG - 1) / p.CG, gq = 8 * (16 / p.CG);        // (XCD-aware group order: k_lwa_fast)
        p.nvb = ((ngrp + gq - 1) / gq) * gq;                                        // virtual blocks: the groups, padded to whole lines per XCD
        // persistent: one workgroup per CU and slab at most (the LDS holds one), a multiple of 8 so that a workgroup keeps its XCD; a stack
        // of slabs fills the chip with its first slabs and the rest queue behind them
        int64_t pw = (cus / 8) * 8;
        if (pw < 8) pw = 8;
        p.fast_grid = dim3((unsigned)(p.nvb < pw ? p.nvb : pw), (unsigned)nslab);
        if (!p.gated) return p;                                                     // vouched for: nothing else to enqueue
    }
    // ---- one launch with the 64-column strip of the tracer in LDS when it fits
    const bool wpl = dA_rank == XC_DA_PLANE, mpl = (M_rank == XC_DA_NONE ? dA_rank : M_rank) == XC_DA_PLANE;
    for (int c : {64, 32, 16})
        if (!p.wchunk && lwa_strip_lds(nullptr, ny, tsize, wpl, mpl, c).bytes <= kLdsBudget) p.wchunk = c;
    const int64_t nstrip = (nx + 63) / 64;
    const int64_t jgroups = (ny + LWA_SW - 1) / LWA_SW;                       // workgroups per strip, LWA_SW target rows each
    // measured on MI355X: the strip kernel wins while its grid does not fill the chip twice (cfg3 alone: 13 us against 5 + 19 for
    // prologue + streaming kernel); stacks that do are VALU-bound either way and the streaming kernel's four targets per
    // thread win (64 slabs: 226 against 272 us)
    const bool few = nstrip * nslab * jgroups <= 2 * cus || knob_strip > 1;
    if (p.wchunk && knob_strip && ny <= 0x7fff && nx <= 0x7fffffff / ny && few && nstrip <= 0x7fffffff && jgroups <= 65535 && nslab <= 65535) {
        p.strip = true;
        p.strip_lds = lwa_strip_lds(nullptr, ny, tsize, wpl, mpl, p.wchunk).bytes;
        p.strip_grid = dim3((unsigned)nstrip, (unsigned)jgroups, (unsigned)nslab);
        return p;
    }
    p.wchunk = 0;
    // ---- prep + streaming kernel.  Small problems: one target row per thread so that the whole chip is busy
    p.stream = true;
    p.scratch_bytes = lwa_scratch(nullptr, nslab, ny, nx, dA_rank).bytes;
    if ((nstrip + 63) / 64 > 65535) { p.refuse = "xc_lwa: nx too large"; return p; }
    p.JT = (double)ny * (double)ny * (double)nx * (double)nslab < 2.0e8 ? 1 : 4;
    p.prep_grid = dim3((unsigned)(ny + LWA_RB), (unsigned)nslab, (unsigned)((nstrip + 63) / 64));
    p.walk_grid = dim3((unsigned)nstrip, (unsigned)((ny + 4 * p.JT - 1) / (4 * p.JT)), (unsigned)nslab);
    return p;
}

// ---------------------------------------------------------------- the launcher
// the (q_dtype, variant, JT) instance of a kernel: f(Tag<T>, bool_constant<V2>, integral_constant<int, JT>); a kernel with fewer template
// parameters ignores the tags it does not have
template <typename T> struct Tag { typedef T type; };
template <typename F>
int lwa_dispatch(int q_dtype, int variant, int jt, F&& f)
{
    auto by_jt = [&](auto t, auto v) { return jt == 4 ? f(t, v, std::integral_constant<int, 4>()) : f(t, v, std::integral_constant<int, 1>()); };
    auto by_variant = [&](auto t) { return variant ? by_jt(t, std::true_type()) : by_jt(t, std::false_type()); };
    return q_dtype == XC_F64 ? by_variant(Tag<double>()) : by_variant(Tag<float>());
}

// the band walk behind a checked interval kernel runs only if the device word holds this call's epoch (a premise failed); flag null: always
struct LwaGate { unsigned* flag; unsigned epoch; };

// k_lwa_check (unless the caller vouches) + k_lwa_fast
int enqueue_interval(xc_ctx* ctx, const LwaArgs& a, const LwaPlan& p, LwaGate* g)
{
    if (p.gated) {
        if (!ctx->lwa_flag) { XC_HIP(ctx, hipMalloc((void**)&ctx->lwa_flag, 256)); XC_HIP(ctx, hipMemset(ctx->lwa_flag, 0, 256)); ctx->lwa_epoch = 0; }
        g->flag = ctx->lwa_flag;
        g->epoch = ++ctx->lwa_epoch;        // a failed check stamps the word with its call's epoch: no memset per call
        hipLaunchKernelGGL(k_lwa_check, dim3((unsigned)a.nslab), dim3(256), 0, ctx->stream, a.Q, a.coord, (int)a.ny, a.increase, g->flag, g->epoch);
        XC_HIP(ctx, hipGetLastError());
    }
    const int keep = lwa_keep(a.part, a.increase), side = keep < 0 ? 2 : keep;      // k_lwa_fast: 0 both sides, 1 near, 2 far
    XC_TRY(lwa_dispatch(a.q_dtype, 0, 1, [&](auto t, auto, auto) -> int {
        typedef typename decltype(t)::type T;
        XC_TRY(ensure_big_lds(ctx, reinterpret_cast<const void*>(k_lwa_fast<T>), (int)kLdsBudget + 4096));
        hipLaunchKernelGGL((k_lwa_fast<T>), p.fast_grid, dim3(1024), p.fast_lds, ctx->stream, (const T*)a.q, a.Q, a.dA, a.dA_rank, a.dA_max,
                           a.M, a.M_rank, (int)a.ny, a.nx, a.increase, side, p.CG, p.nvb, a.out_lwa, g->flag, g->epoch);
        return XC_OK;
    }));
    XC_HIP(ctx, hipGetLastError());
    return XC_OK;
}

// M defaults to dA itself (core.py:789 as written)
inline const double* lwa_metric(const LwaArgs& a) { return a.M_rank == XC_DA_NONE ? a.dA : a.M; }
inline int lwa_metric_rank(const LwaArgs& a) { return a.M_rank == XC_DA_NONE ? a.dA_rank : a.M_rank; }

int enqueue_strip(xc_ctx* ctx, const LwaArgs& a, const LwaPlan& p, const LwaGate& g)
{
    XC_TRY(lwa_dispatch(a.q_dtype, a.variant, 1, [&](auto t, auto v, auto) -> int {
        typedef typename decltype(t)::type T;
        constexpr bool V2 = decltype(v)::value;
        XC_TRY(ensure_big_lds(ctx, reinterpret_cast<const void*>(k_lwa_strip<T, V2>), (int)kLdsBudget + 4096));
        hipLaunchKernelGGL((k_lwa_strip<T, V2>), p.strip_grid, dim3(64 * LWA_SW), p.strip_lds, ctx->stream, (const T*)a.q, a.Q, a.coord, a.dA, a.dA_rank,
                           a.dA_max, lwa_metric(a), lwa_metric_rank(a), a.ny, a.nx, a.increase, a.part, p.wchunk, a.out_lwa, g.flag, g.epoch);
        return XC_OK;
    }));
    XC_HIP(ctx, hipGetLastError());
    return XC_OK;
}

int enqueue_stream(xc_ctx* ctx, const LwaArgs& a, const LwaPlan& p, const LwaGate& g)
{
    XC_TRY(ensure_scratch(ctx, p.scratch_bytes));
    const LwaScratch w = lwa_scratch(ctx->scratch, a.nslab, a.ny, a.nx, a.dA_rank);
    XC_TRY(lwa_dispatch(a.q_dtype, a.variant, p.JT, [&](auto t, auto v, auto jt) -> int {
        typedef typename decltype(t)::type T;
        hipLaunchKernelGGL(k_lwa_prep<T>, p.prep_grid, dim3(256), 0, ctx->stream, (const T*)a.q, a.Q, a.coord, a.dA, a.dA_rank, a.dA_max, a.ny, a.nx,
                           w.nstrip, w.wei, w.rowinfo, w.stripmm, g.flag, g.epoch);
        hipLaunchKernelGGL((k_lwa<T, decltype(v)::value, decltype(jt)::value>), p.walk_grid, dim3(256), 0, ctx->stream, (const T*)a.q, a.Q, a.coord,
                           w.wei, a.dA_rank, lwa_metric(a), lwa_metric_rank(a), w.rowinfo, w.stripmm, a.ny, a.nx, a.increase, a.part, a.out_lwa,
                           g.flag, g.epoch);
        return XC_OK;
    }));
    XC_HIP(ctx, hipGetLastError());
    return XC_OK;
}

int enqueue_masks(xc_ctx* ctx, const LwaArgs& a)
{
    const dim3 grid((unsigned)((a.nx + 255) / 256), (unsigned)a.ny, (unsigned)(a.nslab * a.nmask));
    lwa_dispatch(a.q_dtype, 0, 1, [&](auto t, auto, auto) -> int {
        typedef typename decltype(t)::type T;
        hipLaunchKernelGGL(k_lwa_masks<T>, grid, dim3(256), 0, ctx->stream, (const T*)a.q, a.Q, a.coord, a.ny, a.nx, a.increase, a.variant,
                           a.mask_idx, a.nmask, a.out_masks);
        return XC_OK;
    });
    XC_HIP(ctx, hipGetLastError());
    return XC_OK;
}

int lwa_validate(xc_ctx* ctx, const LwaArgs& a)
{
    if (!a.q || !a.Q || !a.coord || !a.dA || !a.out_lwa || a.nslab < 1 || a.ny < 2 || a.nx < 1)
        return fail(ctx, XC_EBADARG, "xc_lwa: bad arguments");
    if (a.dA_rank != XC_DA_ROW && a.dA_rank != XC_DA_PLANE) return fail(ctx, XC_EBADARG, "xc_lwa: dA_rank must be ROW or PLANE");
    if (a.M_rank != XC_DA_NONE && a.M_rank != XC_DA_ROW && a.M_rank != XC_DA_PLANE) return fail(ctx, XC_EBADARG, "xc_lwa: bad M_rank");
    if (a.M_rank != XC_DA_NONE && !a.M) return fail(ctx, XC_EBADARG, "xc_lwa: M is NULL");
    if (a.part < 0 || a.part > 2) return fail(ctx, XC_EBADARG, "xc_lwa: part must be 0 (all), 1 (upper) or 2 (lower)");
    if (a.nmask < 0 || (a.nmask > 0 && (!a.mask_idx || !a.out_masks))) return fail(ctx, XC_EBADARG, "xc_lwa: mask arguments");
    if (a.ny > 65535 || a.nslab * (a.nmask > 0 ? a.nmask : 1) > 65535) return fail(ctx, XC_EBADARG, "xc_lwa: ny / nslab too large");
    if (a.variant != 0 && a.variant != 1) return fail(ctx, XC_EBADARG, "xc_lwa: variant must be 0 or 1");
    if (a.q_dtype != XC_F32 && a.q_dtype != XC_F64) return fail(ctx, XC_EBADARG, "xc_lwa: q_dtype must be XC_F32 or XC_F64");
    return XC_OK;
}

}  // namespace

int launch_lwa(xc_ctx* ctx, const LwaArgs& a)
{
    XC_TRY(lwa_validate(ctx, a));
    const LwaPlan p = lwa_plan(a.nslab, a.ny, a.nx, esize(a.q_dtype), a.dA_rank, a.M_rank, a.variant, ctx->lwa_exact, ctx->knobs.lwa_fast,
                               ctx->knobs.lwa_strip, ctx->cus);
    if (p.refuse) return fail(ctx, XC_EBADARG, p.refuse);
    LwaGate g = {nullptr, 0};
    if (p.fast) XC_TRY(enqueue_interval(ctx, a, p, &g));
    if (p.strip) XC_TRY(enqueue_strip(ctx, a, p, g));
    if (p.stream) XC_TRY(enqueue_stream(ctx, a, p, g));
    ctx->last_lwa_path = !p.fast ? 0 : (p.gated ? -1 : 1);      // -1: decided on the device, xc_last_lwa_path reads the flag
    return a.nmask > 0 ? enqueue_masks(ctx, a) : XC_OK;
}

}  // namespace xc

// K21 -- what every ring HOLDS of further fields (gfx950): per ring the exact sums of up to XC_PROPS_MAXF fields over its NET nodes (the
// nodes K20 would label with the ring) and over its whole inside set, and the minimum and maximum of one field over its net nodes with the
// flat node each sits on, beside K19's records, from K12's segment records on the device.  No label map is allocated.
//
// The rule (include/xcontour_hip.h, K21 section).  The mapping is K20's scan (xc_cplabel.hip, xc_cpiece_label.h): a column is scanned from
// the row that lies outside every ring, in one register of state; instead of storing the state of a node the scan ADDS the node's terms to
// the ring the state names.
//   SUMS       a term w g_m (the product rounded once) is cut into 32-bit chunks and added whole to CP_L words (xc_cpiece_sum.h): integer
//              additions, so every order of arrival gives the same words, and cp_to_double rounds the exact sum once.  A thread keeps
//              CP_L PRIVATE words per field while its state stays the same ring and hands them to the ring's staged words with 64-bit
//              integer atomics when the state changes and at the chunk's end; at the chunk's end a wave whose lanes all stand in one ring
//              adds their words with shuffles first and issues one atomic per word (a large ring would otherwise take 64 on one address).
//   NO WRAP    a chunk of a term is below 2^32 and a term gives a word at most one chunk.  A private word holds the terms of one chunk's
//              rows at most, fewer than 2^25 + 16 of them (ny < 2^30 in at most PL_CHUNKS chunks): below 2^58 in magnitude.  A staged net
//              word holds one term per net node of the ring, a staged gross word one per inside node: at most ny nx < 2^30 terms, below
//              2^62 in magnitude.  Signed 64-bit words hold both.
//   GROSS      I_p is the net set of p and of all its descendants (K20): every ring adds its net words, and its not-finite flags, to its
//              own gross words and to those of every ancestor along par[] (k_pp_fold) -- integer atomics again: exact in any order.
//   EXTREMUM   values are compared by the monotone 64-bit key of a double (-0.0 below +0.0), NaN is skipped.  Pass 1 leaves the ring's
//              smallest and largest key (private keys, one atomicMin / atomicMax per run of a state).  PASS 2 over the same chunks, once
//              the keys are final, takes per ring the smallest flat node whose key EQUALS the ring's key with an integer atomicMin: the
//              two-pass scheme, the same result for every order of arrival.
//   FIELDS     k_pp_scan<NF, XM> is templated on the number of fields of a PASS, NF <= PP_PASS = 4; a call of more fields runs two
//              passes.  The second pass of the extremum rides on the second pass of the fields where there is one.  The compiler's
//              resource report decided: see profiles/contour_piece_props.md.
//
// Per group, after K19's stages and before k_cp_unscatter (the edge table, root[], slot[], the signs and par[] still stand):
//   k_pp_init    the staged words, keys, places and flags of the group's pieces are cleared
//   k_pl_carry   K20's: the carry of every chunk but the last (xc_cpiece_label.h)
//   k_pp_scan    one thread per (range of the group, chunk, column), columns fastest; nodes in state -1 load nothing.  Lanes of a wave take
//                consecutive columns: the reads of w, g_m, x and of tab[V(e, c)] are contiguous across a wave
//   k_pp_fold    one thread per ring: net -> gross up the tree; a chase that does not end within the range's piece count sets PT_ERR_TREE
// Before the groups k_pp_bound leaves max |w g_m| over the finite values of every (slab, field): the tops of the windows.  k_pp_finish
// converts the words once per value, after k_pi_finish and k_pt_finish have written K19's columns and only when all pieces fit.  Every
// index taken from a record or a table is checked before it addresses anything; every scan ends within ny steps; no kernel waits for
// another block; no LDS, no scratch.
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
#include "xc_cpiece_interior.h"
#include "xc_cpiece_tree.h"
#include "xc_cpiece_label.h"

constexpr int PP_PASS = 4;                    // fields of one pass of the scan
constexpr unsigned long long PP_NOKEY = ~0ull;  // no key yet (minimum), no place yet; the key of no value: a NaN's
constexpr unsigned long long PP_SIGN = 1ull << 63;

// one field plane as the kernels read it (a table of the call's fields on the device; the extremum field is entry nf)
struct PpField {
    const void* p;
    unsigned long long stride;    // elements between two slabs: ny nx, or 0 for a plane all slabs share
    int f32, pad;
};

// the staged records of K21 (behind K19's in ctx->cpiece_acc), `cap` of each
struct PpStage {
    unsigned long long* net;      // [cap][nf][CP_L] the limbs of the net sums
    unsigned long long* gro;      // [cap][nf][CP_L] the limbs of the gross sums
    unsigned long long* kmin;     // the smallest key of x over the net nodes (PP_NOKEY: none)
    unsigned long long* kmax;     // the largest (0: none)
    unsigned long long* amin;     // the smallest flat node that carries kmin
    unsigned long long* amax;
    int* flg;                     // bit m: a net term of field m is not finite
    int* gflg;                    // the same of the gross sum
};

__device__ __forceinline__ double pp_load(const PpField& f, size_t slab, size_t node)
{
    const size_t i = (size_t)f.stride * slab + node;
    return f.f32 ? (double)((const float*)f.p)[i] : ((const double*)f.p)[i];
}

// the usual monotone key of a double: unsigned order of the keys = order of the values, -0.0 below +0.0
__device__ __forceinline__ unsigned long long pp_key(double v)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b & PP_SIGN) ? ~b : (b | PP_SIGN);
}
__device__ __forceinline__ double pp_unkey(unsigned long long k)
{
    return __longlong_as_double((long long)((k & PP_SIGN) ? (k & ~PP_SIGN) : ~k));
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

__global__ __launch_bounds__(CP_TPB)
void k_pp_init(int64_t p0, int64_t p1, int nf, PpStage pp)
{
    const int64_t p = p0 + (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (p >= p1) return;
    const size_t nw = (size_t)nf * CP_L;
    for (size_t j = 0; j < nw; ++j) { pp.net[(size_t)p * nw + j] = 0ull; pp.gro[(size_t)p * nw + j] = 0ull; }
    pp.kmin[p] = PP_NOKEY; pp.kmax[p] = 0ull; pp.amin[p] = PP_NOKEY; pp.amax[p] = PP_NOKEY; pp.flg[p] = 0; pp.gflg[p] = 0;
}

__device__ __forceinline__ unsigned long long pp_wave_min(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { const unsigned long long o = __shfl_xor(v, d); v = o < v ? o : v; }
    return v;
}

// what a thread gathered for ring p goes to the ring's staged words, keys (XM 1) or places (XM 2), and is cleared; 0 <= p < cap
template <int NF, int XM>
__device__ __forceinline__ void pp_hand_over(const PpStage& pp, size_t p, int nf, int m0, unsigned long long (&acc)[NF ? NF : 1][CP_L], int& bad,
                                             unsigned long long& kmn, unsigned long long& kmx, unsigned long long& amn, unsigned long long& amx)
{
    if constexpr (NF > 0) {
        unsigned long long* d = pp.net + (p * (size_t)nf + (size_t)m0) * CP_L;
#pragma unroll
        for (int m = 0; m < NF; ++m)
#pragma unroll
            for (int l = 0; l < CP_L; ++l) {
                if (acc[m][l]) atomicAdd(d + m * CP_L + l, acc[m][l]);
                acc[m][l] = 0ull;
            }
        if (bad) { atomicOr(pp.flg + p, bad); bad = 0; }
    }
    if constexpr (XM == 1) {
        if (kmn != PP_NOKEY) { atomicMin(pp.kmin + p, kmn); atomicMax(pp.kmax + p, kmx); }
        kmn = PP_NOKEY; kmx = 0ull;
    }
    if constexpr (XM == 2) {
        if (amn != PP_NOKEY) atomicMin(pp.amin + p, amn);
        if (amx != PP_NOKEY) atomicMin(pp.amax + p, amx);
        amn = PP_NOKEY; amx = PP_NOKEY;
    }
}

// One pass of the scan over NF fields, fld[m0 .. m0 + NF), of the call's nf.  XM 0: no extremum; 1: the keys of x = fld[nf]; 2: the places
// of the final keys.
template <int NF, int XM>
__global__ __launch_bounds__(CP_TPB)
void k_pp_scan(int64_t ng, int64_t rows, int64_t nchunk, int ncont, PlGroup g, PiStage st, PtStage pt, const int* __restrict__ carry,
               const double* __restrict__ w, int w_per_slab, const PpField* __restrict__ fld, int m0, int nf,
               const unsigned long long* __restrict__ mxg, PpStage pp, int* __restrict__ err)
{
    int64_t rl, k, c;
    if (!pl_thread(ng, nchunk, g.nx, rl, k, c)) return;
    const int64_t r = g.r0 + rl;
    const long long lo = g.poff[r], hi = g.poff[r + 1];
    const int* tp = g.tab + (size_t)rl * (size_t)g.E + 2 * (size_t)c + 1;   // tp[2 nx e] = tab[V(e, c)]
    int state = -1;
    for (int64_t kk = k - 1; kk >= 0; --kk) {                                // at most PL_CHUNKS - 1 steps
        const int v = carry[(size_t)(rl * nchunk + kk) * (size_t)g.nx + (size_t)c];
        if (v != PL_NONE) { state = v; break; }
    }
    const size_t sl = (size_t)(r / ncont), npl = (size_t)g.ny * (size_t)g.nx;
    const double* wp = w ? w + (w_per_slab ? sl * npl : 0) : nullptr;
    constexpr int NA = NF ? NF : 1;
    PpField f[NA];
    int top[NA];
    unsigned long long acc[NA][CP_L];
#pragma unroll
    for (int m = 0; m < NF; ++m) {
        f[m] = fld[m0 + m];
        top[m] = ci_top(mxg[sl * (size_t)nf + (size_t)(m0 + m)]);
#pragma unroll
        for (int l = 0; l < CP_L; ++l) acc[m][l] = 0ull;
    }
    PpField fx = {};
    if constexpr (XM != 0) fx = fld[nf];
    int bad = 0;
    unsigned long long kmn = PP_NOKEY, kmx = 0ull;                           // XM 1: the keys of this run
    unsigned long long rmn = PP_NOKEY, rmx = 0ull, amn = PP_NOKEY, amx = PP_NOKEY;   // XM 2: the ring's keys, the places of this run
    if constexpr (XM == 2) if (state >= 0) { rmn = pp.kmin[lo + state]; rmx = pp.kmax[lo + state]; }
    // the chunk's nodes are steps [k rows, t1) of the scan
    const int64_t t1 = (k + 1) * rows < g.ny ? (k + 1) * rows : g.ny;
    for (int64_t t = k * rows; t < t1; ++t) {
        const int64_t at = g.flip ? g.ny - 1 - t : t;                        // 0 <= at < ny
        if (state >= 0) {
            const size_t node = (size_t)at * (size_t)g.nx + (size_t)c;
            if constexpr (NF > 0) {
                const double wv = wp ? wp[node] : 1.0;
#pragma unroll
                for (int m = 0; m < NF; ++m) {
                    const double tv = __dmul_rn(wv, pp_load(f[m], sl, node));
                    if (tv == tv && !cp_add_private(acc[m], tv, top[m])) bad |= 1 << (m0 + m);
                }
            }
            if constexpr (XM != 0) {
                const double xv = pp_load(fx, sl, node);
                if (xv == xv) {
                    const unsigned long long key = pp_key(xv);
                    if constexpr (XM == 1) { kmn = key < kmn ? key : kmn; kmx = key > kmx ? key : kmx; }
                    else {
                        if (key == rmn && node < amn) amn = node;
                        if (key == rmx && node < amx) amx = node;
                    }
                }
            }
        }
        if (t == g.ny - 1) break;
        const int64_t e = g.flip ? at - 1 : at;                              // the edge to the next node: 0 <= e < ny - 1
        const int v = pl_cross(tp[2 * (size_t)g.nx * (size_t)e], r, lo, hi, g, st, pt, err);
        if (v == PL_NONE || v == state) continue;
        if (state >= 0) pp_hand_over<NF, XM>(pp, (size_t)(lo + state), nf, m0, acc, bad, kmn, kmx, amn, amx);   // the run of `state` ends
        state = v;
        if constexpr (XM == 2) if (state >= 0) { rmn = pp.kmin[lo + state]; rmx = pp.kmax[lo + state]; }
    }
    // The chunk's end.  Inside a large ring every lane of a wave ends its chunk in the SAME ring: the wave then adds its lanes' words (and
    // takes the minimum / maximum of their keys and places) with shuffles and lane 0 alone hands them over -- one atomic per word and
    // wave, not 64 on one address.  Integer sums again: the ring's words are the same either way.
    const long long pk = state >= 0 ? lo + state : -1ll;
    if (__ballot(1) == ~0ull) {                                              // (a wave with idle lanes hands over lane by lane)
        const long long pf = __shfl(pk, 0);
        if (pf >= 0 && __all(pk == pf)) {
            const bool lead = (threadIdx.x & 63) == 0;
            if constexpr (NF > 0) {
#pragma unroll
                for (int m = 0; m < NF; ++m)
#pragma unroll
                    for (int l = 0; l < CP_L; ++l) {
                        unsigned long long v = acc[m][l];
                        if (__any(v != 0ull)) {
#pragma unroll
                            for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
                        }
                        acc[m][l] = lead ? v : 0ull;
                    }
#pragma unroll
                for (int d = 32; d > 0; d >>= 1) bad |= __shfl_xor(bad, d);
                if (!lead) bad = 0;
            }
            if constexpr (XM == 1) {
                kmn = pp_wave_min(kmn); kmx = ci_wave_max(kmx);
                if (!lead) { kmn = PP_NOKEY; kmx = 0ull; }
            }
            if constexpr (XM == 2) {
                amn = pp_wave_min(amn); amx = pp_wave_min(amx);
                if (!lead) { amn = PP_NOKEY; amx = PP_NOKEY; }
            }
        }
    }
    if (pk >= 0) pp_hand_over<NF, XM>(pp, (size_t)pk, nf, m0, acc, bad, kmn, kmx, amn, amx);
}

__global__ __launch_bounds__(CP_TPB)
void k_pp_fold(int64_t p0, int64_t p1, int64_t r0, int64_t r1, const long long* __restrict__ poff, int nf, PiStage st, PtStage pt,
               PpStage pp, int* __restrict__ err)
{
    const int64_t p = p0 + (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (p >= p1 || !st.cl[p]) return;
    const int64_t r = cp_range_of(poff, r0, r1, p);
    const long long lo = poff[r], hi = poff[r + 1];                        // an ancestor is a piece of the same range
    const size_t nw = (size_t)nf * CP_L;
    const unsigned long long* src = pp.net + (size_t)p * nw;
    const int fl = pp.flg[p];
    long long q = p;                                                        // the ring itself, then its ancestors
    for (long long step = 0; q >= 0; ++step) {
        if (q < lo || q >= hi || q >= p1 || step >= hi - lo) { *err = PT_ERR_TREE; break; }
        unsigned long long* d = pp.gro + (size_t)q * nw;
        for (size_t j = 0; j < nw; ++j) { const unsigned long long v = src[j]; if (v) atomicAdd(d + j, v); }
        if (fl) atomicOr(pp.gflg + q, fl);
        q = pt.par[q];
    }
}

// one thread per (column, piece): columns 0 .. nf - 1 the sums of a field, column nf (with x) the extremum
__global__ __launch_bounds__(CP_TPB)
void k_pp_finish(int64_t np, int64_t nrange, int ncont, int nf, int hasx, int64_t capacity, const long long* __restrict__ poff, PiStage st,
                 PpStage pp, const unsigned long long* __restrict__ mxg, double* __restrict__ net_g, double* __restrict__ sum_g,
                 double* __restrict__ x_min, double* __restrict__ x_max, long long* __restrict__ at_min, long long* __restrict__ at_max)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= np * (nf + hasx)) return;
    const int m = (int)(i / np);
    const int64_t p = i - (int64_t)m * np;
    const int cl = st.cl[p];
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    if (m < nf) {
        const int64_t s = cp_range_of(poff, 0, nrange, p) / ncont;
        const int top = ci_top(mxg[(size_t)s * nf + m]);
        const size_t at = ((size_t)p * nf + m) * CP_L, out = (size_t)m * (size_t)capacity + (size_t)p;
        net_g[out] = (!cl || ((pp.flg[p] >> m) & 1)) ? qnan : cp_to_double(pp.net + at, top);
        sum_g[out] = (!cl || ((pp.gflg[p] >> m) & 1)) ? qnan : cp_to_double(pp.gro + at, top);
        return;
    }
    const unsigned long long kmn = pp.kmin[p], kmx = pp.kmax[p];
    const bool has = cl && kmn != PP_NOKEY;
    x_min[p] = has ? pp_unkey(kmn) : qnan; x_max[p] = has ? pp_unkey(kmx) : qnan;
    at_min[p] = has ? (long long)pp.amin[p] : -1ll; at_max[p] = has ? (long long)pp.amax[p] : -1ll;
}

// the passes of one group's scan: fields in runs of PP_PASS; the keys of x in the first pass, their places in the second (one of its own
// where the fields need none)
template <int XM>
void pp_launch_pass(int n_pass, dim3 grid, hipStream_t stream, int64_t ng, int64_t rows, int64_t nchunk, int ncont, const PlGroup& pg,
                    const PiStage& st, const PtStage& pt, const int* carry, const double* w, int w_per_slab, const PpField* fld, int m0,
                    int nf, const unsigned long long* mxg, const PpStage& pp, int* err)
{
#define XC_PP_SCAN(NF_) hipLaunchKernelGGL((k_pp_scan<NF_, XM>), grid, dim3(CP_TPB), 0, stream, ng, rows, nchunk, ncont, pg, st, pt, carry, w, \
                                           w_per_slab, fld, m0, nf, mxg, pp, err)
    switch (n_pass) {
    case 0: if constexpr (XM != 0) XC_PP_SCAN(0); break;
    case 1: XC_PP_SCAN(1); break;
    case 2: XC_PP_SCAN(2); break;
    case 3: XC_PP_SCAN(3); break;
    default: XC_PP_SCAN(4); break;
    }
#undef XC_PP_SCAN
}

}  // namespace

// One xc_contour_piece_props_dev call: K19's (xc_cptree.hip) with the props scan per group.  Waits for the stream as K18 does.
int launch_contour_piece_props(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to,
                               const double* pts, int64_t ny, int64_t nx, int periodic, int flip, int ncont, const double* w,
                               int w_per_slab, const void* f, int f_dtype, int64_t capacity, uint64_t* piece_count, int64_t* first_edge,
                               int64_t* nseg, int32_t* closed, int32_t* winding, int64_t* n_in, double* sum_w, double* sum_wf,
                               int64_t* parent, int32_t* depth, int32_t* nchild, int64_t* n_net, double* net_w, double* net_wf,
                               int nf, const void* const* g, const int* g_dtype, const int* g_per_slab, const void* x, int x_dtype,
                               double* net_g, double* sum_g, double* x_min, double* x_max, int64_t* at_min, int64_t* at_max)
{
    const char* who = "xc_contour_piece_props";
    if (!count || !piece_count || nrange < 1 || ny < 1 || nx < 1 || capacity < 0) return fail(ctx, XC_EBADARG, std::string(who) + ": bad arguments");
    if (flip != 0 && flip != 1) return fail(ctx, XC_EBADARG, std::string(who) + ": flip is 0 or 1");
    if (ncont < 1 || nrange % ncont != 0) return fail(ctx, XC_EBADARG, std::string(who) + ": nrange must be a multiple of ncont >= 1");
    if (f && f_dtype != XC_F32 && f_dtype != XC_F64) return fail(ctx, XC_EBADARG, std::string(who) + ": f_dtype is XC_F32 or XC_F64");
    if (nf < 0 || nf > XC_PROPS_MAXF) return fail(ctx, XC_EBADARG, std::string(who) + ": nf lies in [0, XC_PROPS_MAXF]");
    if (nf > 0 && (!g || !g_dtype || !g_per_slab)) return fail(ctx, XC_EBADARG, std::string(who) + ": nf > 0 needs g, g_dtype and g_per_slab");
    for (int m = 0; m < nf; ++m) {
        if (!g[m]) return fail(ctx, XC_EBADARG, std::string(who) + ": a field plane is NULL");
        if (g_dtype[m] != XC_F32 && g_dtype[m] != XC_F64) return fail(ctx, XC_EBADARG, std::string(who) + ": g_dtype is XC_F32 or XC_F64");
    }
    if (x && x_dtype != XC_F32 && x_dtype != XC_F64) return fail(ctx, XC_EBADARG, std::string(who) + ": x_dtype is XC_F32 or XC_F64");
    if (capacity > 0 && (!first_edge || !nseg || !closed || !winding || !n_in || !sum_w || !parent || !depth || !nchild || !n_net || !net_w))
        return fail(ctx, XC_EBADARG, std::string(who) + ": capacity > 0 needs the record arrays");
    if (capacity > 0 && ((f == nullptr) != (sum_wf == nullptr) || (f == nullptr) != (net_wf == nullptr)))
        return fail(ctx, XC_EBADARG, std::string(who) + ": f, sum_wf and net_wf go together");
    if (capacity > 0 && ((nf == 0) != (net_g == nullptr) || (nf == 0) != (sum_g == nullptr)))
        return fail(ctx, XC_EBADARG, std::string(who) + ": net_g and sum_g are NULL exactly when nf is 0");
    if (capacity > 0 && ((x == nullptr) != (x_min == nullptr) || (x == nullptr) != (x_max == nullptr) || (x == nullptr) != (at_min == nullptr) ||
                         (x == nullptr) != (at_max == nullptr)))
        return fail(ctx, XC_EBADARG, std::string(who) + ": x, x_min, x_max, at_min and at_max go together");
    if (periodic && nx < 3) return fail(ctx, XC_EBADARG, std::string(who) + ": a periodic plane needs nx >= 3 (with two columns a cell's two vertical edges are one)");
    if (ny > (((int64_t)1 << 30) - 1) / nx) return fail(ctx, XC_EBADARG, std::string(who) + ": plane too large for 32-bit labels (2 ny nx < 2^31)");
    const long long E = 2 * ny * nx;
    const int wrap = periodic ? 1 : 0;
    const int64_t nslab = nrange / ncont;
    if (nslab > 65535) return fail(ctx, XC_EBADARG, std::string(who) + ": more than 65535 slabs");
    for (int k = 0; k < 7; ++k) ctx->cpprops_ms[k] = 0.f;
    ctx->cpprops_rounds = 0; ctx->cpprops_groups = 0;
    const int hasx = x ? 1 : 0;
    const int64_t npl = ny * nx;

    std::vector<uint64_t> hc((size_t)nrange);
    XC_HIP(ctx, hipMemcpyAsync(hc.data(), count, (size_t)nrange * 8, hipMemcpyDeviceToHost, ctx->stream));
    XC_HIP(ctx, hipMemsetAsync(piece_count, 0, (size_t)nrange * 8, ctx->stream));
    XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<long long> off((size_t)nrange + 1);
    off[0] = 0;
    for (int64_t r = 0; r < nrange; ++r) {
        if (hc[(size_t)r] >= (1ull << 31)) return fail(ctx, XC_EBADARG, std::string(who) + ": a range of 2^31 or more segments");
        off[(size_t)r + 1] = off[(size_t)r] + (long long)hc[(size_t)r];
    }
    const long long total = off[(size_t)nrange];
    if (total == 0) return XC_OK;
    if (!e_from || !e_to || !pts) return fail(ctx, XC_EBADARG, std::string(who) + ": segments without their records");
    const int64_t cap = std::min<int64_t>(capacity, total);               // a piece has a segment: no more pieces than segments

    int64_t gmax = 1; long long nmax = 0;
    const std::vector<CpGroup> groups = cp_plan_groups(ctx->cpiece_cap, E, nrange, hc, off, &gmax, &nmax);
    int64_t rows = 0, nchunk = 0;
    pl_geometry(ny, &rows, &nchunk);
    // workspace (K20's, then the bounds and the table of fields): off | poff | mx[nslab][2], err (cleared together) | tab[gmax][E] |
    // rid[nmax] | label, next, prev x 2 [nmax] | carry[gmax][nchunk][nx] | mxg[nslab][nf] | fld[nf + 1]
    const size_t b_off = al((size_t)(nrange + 1) * 8), b_mx = al((size_t)nslab * 16), b_small = 256;
    const size_t b_tab = al((size_t)gmax * (size_t)E * 4), b_n = al((size_t)nmax * 4);
    const size_t b_carry = nchunk > 1 ? al((size_t)gmax * (size_t)nchunk * (size_t)nx * 4) : 0;
    const size_t b_mxg = al((size_t)nslab * (size_t)std::max(nf, 1) * 8), b_fld = al((size_t)(XC_PROPS_MAXF + 1) * sizeof(PpField));
    XC_TRY(grow(ctx, &ctx->cpiece_ws, &ctx->cpiece_ws_bytes, 2 * b_off + b_mx + b_small + b_tab + 7 * b_n + b_carry + b_mxg + b_fld));
    char* ws = (char*)ctx->cpiece_ws;
    long long* d_off = (long long*)ws;
    long long* d_poff = (long long*)(ws + b_off);
    unsigned long long* mx = (unsigned long long*)(ws + 2 * b_off);
    int* d_err = (int*)((char*)mx + b_mx);
    int* tab = (int*)((char*)d_err + b_small);
    int* rid = (int*)((char*)tab + b_tab);
    int* buf[6];
    for (int k = 0; k < 6; ++k) buf[k] = (int*)((char*)rid + (size_t)(k + 1) * b_n);
    int* carry = (int*)((char*)rid + 7 * b_n);
    unsigned long long* mxg = (unsigned long long*)((char*)carry + b_carry);
    PpField* d_fld = (PpField*)((char*)mxg + b_mxg);
    // the staged records, K18's, the tree's and then K21's: nothing reaches the caller's record arrays before all pieces are known to fit
    PiStage st = {};
    PtStage pt = {};
    PpStage pp = {};
    if (cap > 0) {
        const size_t b8 = al((size_t)cap * 8), b4 = al((size_t)cap * 4), b_acc = al((size_t)cap * 2 * CP_L * 8);
        const size_t b_g = al((size_t)cap * (size_t)nf * CP_L * 8);
        XC_TRY(grow(ctx, &ctx->cpiece_acc, &ctx->cpiece_acc_bytes, 2 * b_acc + 8 * b8 + 5 * b4 + 2 * b_g + 4 * b8 + 2 * b4));
        char* a = (char*)ctx->cpiece_acc;
        st.acc = (unsigned long long*)a; a += b_acc;
        st.cnt = (unsigned long long*)a; a += b8;
        st.sa = (unsigned long long*)a; a += b8;
        st.sb = (unsigned long long*)a; a += b8;
        st.ns = (unsigned long long*)a; a += b8;
        st.fe = (long long*)a; a += b8;
        st.wd = (int*)a; a += b4;
        st.cl = (int*)a; a += b4;
        st.flg = (int*)a; a += b4;
        pt.net = (unsigned long long*)a; a += b_acc;
        pt.key = (unsigned long long*)a; a += b8;
        pt.nnet = (unsigned long long*)a; a += b8;
        pt.par = (long long*)a; a += b8;
        pt.nch = (int*)a; a += b4;
        pt.dep = (int*)a; a += b4;
        pp.net = (unsigned long long*)a; a += b_g;
        pp.gro = (unsigned long long*)a; a += b_g;
        pp.kmin = (unsigned long long*)a; a += b8;
        pp.kmax = (unsigned long long*)a; a += b8;
        pp.amin = (unsigned long long*)a; a += b8;
        pp.amax = (unsigned long long*)a; a += b8;
        pp.flg = (int*)a; a += b4;
        pp.gflg = (int*)a;
    }
    // the call's fields as the kernels read them; entry nf is the extremum field
    PpField hfld[XC_PROPS_MAXF + 1] = {};
    for (int m = 0; m < nf; ++m) hfld[m] = {g[m], g_per_slab[m] ? (unsigned long long)npl : 0ull, g_dtype[m] == XC_F32 ? 1 : 0, 0};
    if (x) hfld[nf] = {x, (unsigned long long)npl, x_dtype == XC_F32 ? 1 : 0, 0};

    // where the time goes (xc_set_kernel_timing): events between the stages, summed per kind after the call
    std::vector<std::pair<hipEvent_t, int>> marks;
    auto mark = [&](int kind) {
        if (!ctx->timing) return;
        hipEvent_t ev;
        if (hipEventCreate(&ev) != hipSuccess) return;
        (void)hipEventRecord(ev, ctx->stream);
        marks.push_back({ev, kind});
    };
    auto settle = [&]() {
        for (size_t k = 1; k < marks.size(); ++k) {
            float ms = 0.f;
            if (marks[k].second >= 0 && hipEventElapsedTime(&ms, marks[k - 1].first, marks[k].first) == hipSuccess) ctx->cpprops_ms[marks[k].second] += ms;
        }
        for (auto& m : marks) (void)hipEventDestroy(m.first);
        marks.clear();
    };

    const dim3 blk(CP_TPB);
    mark(-1);
    XC_HIP(ctx, hipMemsetAsync(mx, 0, b_mx + b_small, ctx->stream));
    if (cap > 0) {
        const dim3 bgrid((unsigned)std::min<int64_t>((npl + CI_TPB - 1) / CI_TPB, 1024), (unsigned)nslab);
        if (!f) hipLaunchKernelGGL((k_ci_bound<void>), bgrid, dim3(CI_TPB), 0, ctx->stream, npl, w, w_per_slab, (const void*)nullptr, mx);
        else if (f_dtype == XC_F32) hipLaunchKernelGGL((k_ci_bound<float>), bgrid, dim3(CI_TPB), 0, ctx->stream, npl, w, w_per_slab, (const float*)f, mx);
        else hipLaunchKernelGGL((k_ci_bound<double>), bgrid, dim3(CI_TPB), 0, ctx->stream, npl, w, w_per_slab, (const double*)f, mx);
        XC_HIP(ctx, hipGetLastError());
    }
    mark(3);
    if (cap > 0) {
        XC_HIP(ctx, hipMemsetAsync(mxg, 0, b_mxg, ctx->stream));
        XC_HIP(ctx, hipMemcpyAsync(d_fld, hfld, sizeof(hfld), hipMemcpyHostToDevice, ctx->stream));
        if (nf > 0) {
            const dim3 ggrid((unsigned)std::min<int64_t>((npl + CI_TPB - 1) / CI_TPB, 1024), (unsigned)nslab, (unsigned)nf);
            hipLaunchKernelGGL(k_pp_bound, ggrid, dim3(CI_TPB), 0, ctx->stream, npl, nf, w, w_per_slab, (const PpField*)d_fld, mxg);
            XC_HIP(ctx, hipGetLastError());
        }
    }
    mark(5);
    XC_HIP(ctx, hipMemcpyAsync(d_off, off.data(), (size_t)(nrange + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    XC_HIP(ctx, hipMemsetAsync(tab, 0xff, (size_t)gmax * (size_t)E * 4, ctx->stream));
    mark(0);

    std::vector<uint64_t> hp((size_t)nrange, 0);
    std::vector<long long> poff((size_t)nrange + 1, 0);
    int64_t done = 0;                                                       // poff[0 .. done] stand
    bool over = cap == 0;                                                   // the pieces no longer fit: count only
    int rounds_total = 0;
    for (const CpGroup& gr : groups) {
        const long long s0 = off[(size_t)gr.r0];
        const int64_t n = off[(size_t)gr.r1] - s0, ng = gr.r1 - gr.r0;
        const int R = cp_rounds(hc, gr);                                   // ceil(log2(largest count)) + 1
        const dim3 grid(cp_blocks(n));
        int *lab = buf[0], *nxt = buf[1], *prv = buf[2], *lab2 = buf[3], *nxt2 = buf[4], *prv2 = buf[5];
        hipLaunchKernelGGL(k_cp_scatter, grid, blk, 0, ctx->stream, n, s0, d_off, gr.r0, gr.r1, E, (const long long*)e_from, tab, rid, lab, prv, d_err);
        hipLaunchKernelGGL(k_cp_link, grid, blk, 0, ctx->stream, n, s0, E, (const long long*)e_to, tab, rid, nxt, prv, d_err);
        XC_HIP(ctx, hipGetLastError());
        mark(0);
        for (int k = 0; k < R; ++k) {
            hipLaunchKernelGGL(k_cp_round, grid, blk, 0, ctx->stream, n, lab, nxt, prv, lab2, nxt2, prv2);
            std::swap(lab, lab2); std::swap(nxt, nxt2); std::swap(prv, prv2);
        }
        XC_HIP(ctx, hipGetLastError());
        rounds_total += R;
        mark(1);
        int *root = nxt2, *slot = lab2;
        hipLaunchKernelGGL(k_cp_root, grid, blk, 0, ctx->stream, n, E, tab, rid, lab, prv, gr.r0, (unsigned long long*)piece_count, root, slot);
        XC_HIP(ctx, hipGetLastError());
        // the group's piece counts place its pieces in the table
        XC_HIP(ctx, hipMemcpyAsync(hp.data() + gr.r0, piece_count + gr.r0, (size_t)ng * 8, hipMemcpyDeviceToHost, ctx->stream));
        XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (; done < gr.r1; ++done) poff[(size_t)done + 1] = poff[(size_t)done] + (long long)hp[(size_t)done];
        const long long p0 = poff[(size_t)gr.r0], p1 = poff[(size_t)gr.r1];
        if (p1 > cap) over = true;
        if (!over && p1 > p0) {
            const dim3 pgrid(cp_blocks(p1 - p0));
            const unsigned long long* pcnt = (const unsigned long long*)piece_count;
            XC_HIP(ctx, hipMemcpyAsync(d_poff + gr.r0, poff.data() + gr.r0, (size_t)(ng + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL(k_pi_init, pgrid, blk, 0, ctx->stream, (int64_t)p0, (int64_t)p1, st);
            hipLaunchKernelGGL(k_pi_piece, grid, blk, 0, ctx->stream, n, s0, gr.r0, E, ny, nx, wrap, cap, (const long long*)e_from,
                               (const long long*)e_to, pts, rid, root, slot, pcnt, d_poff, st, d_err);
            XC_HIP(ctx, hipGetLastError());
            mark(2);
#define XC_PI_WALK(FT_) hipLaunchKernelGGL((k_pi_walk<FT_>), grid, blk, 0, ctx->stream, n, s0, gr.r0, E, ny, nx, flip, ncont, cap, (const long long*)e_from, \
                                           (const long long*)e_to, tab, rid, root, slot, pcnt, d_poff, w, w_per_slab, (const FT_*)f, mx, st, d_err)
            if (!f) XC_PI_WALK(void); else if (f_dtype == XC_F32) XC_PI_WALK(float); else XC_PI_WALK(double);
#undef XC_PI_WALK
            XC_HIP(ctx, hipGetLastError());
            mark(3);
            hipLaunchKernelGGL(k_pt_init, pgrid, blk, 0, ctx->stream, (int64_t)p0, (int64_t)p1, pt);
            hipLaunchKernelGGL(k_pt_top, grid, blk, 0, ctx->stream, n, s0, gr.r0, E, ny, nx, flip, cap, (const long long*)e_from,
                               (const long long*)e_to, rid, root, slot, pcnt, d_poff, st, pt, d_err);
            hipLaunchKernelGGL(k_pt_parent, pgrid, blk, 0, ctx->stream, (int64_t)p0, (int64_t)p1, n, s0, gr.r0, gr.r1, E, ny, nx, flip, cap,
                               (const long long*)e_from, (const long long*)e_to, tab, root, slot, pcnt, d_poff, st, pt, d_err);
            hipLaunchKernelGGL(k_pt_depth, pgrid, blk, 0, ctx->stream, (int64_t)p0, (int64_t)p1, gr.r0, gr.r1, d_poff, st, pt, d_err);
            hipLaunchKernelGGL(k_pt_net, pgrid, blk, 0, ctx->stream, (int64_t)p0, (int64_t)p1, st, pt);
            XC_HIP(ctx, hipGetLastError());
            mark(4);
            if (nf > 0 || hasx) {
                const PlGroup pg = {n, s0, gr.r0, E, ny, nx, flip, cap, (const long long*)e_from, (const long long*)e_to, tab, root, slot, pcnt, d_poff};
                const dim3 lgrid(cp_blocks(ng * nchunk * nx));             // no more threads than the group's table has nodes
                hipLaunchKernelGGL(k_pp_init, pgrid, blk, 0, ctx->stream, (int64_t)p0, (int64_t)p1, nf, pp);
                if (nchunk > 1) hipLaunchKernelGGL(k_pl_carry, lgrid, blk, 0, ctx->stream, ng, rows, nchunk, pg, st, pt, carry, d_err);
                // pass 1: the first PP_PASS fields and the keys of x; pass 2: the other fields and the places of the keys
                const int n1 = std::min(nf, PP_PASS), n2 = nf - n1;
                if (hasx) pp_launch_pass<1>(n1, lgrid, ctx->stream, ng, rows, nchunk, ncont, pg, st, pt, carry, w, w_per_slab, d_fld, 0, nf, mxg, pp, d_err);
                else pp_launch_pass<0>(n1, lgrid, ctx->stream, ng, rows, nchunk, ncont, pg, st, pt, carry, w, w_per_slab, d_fld, 0, nf, mxg, pp, d_err);
                if (hasx) pp_launch_pass<2>(n2, lgrid, ctx->stream, ng, rows, nchunk, ncont, pg, st, pt, carry, w, w_per_slab, d_fld, n1, nf, mxg, pp, d_err);
                else if (n2 > 0) pp_launch_pass<0>(n2, lgrid, ctx->stream, ng, rows, nchunk, ncont, pg, st, pt, carry, w, w_per_slab, d_fld, n1, nf, mxg, pp, d_err);
                XC_HIP(ctx, hipGetLastError());
                mark(5);
                if (nf > 0) {
                    hipLaunchKernelGGL(k_pp_fold, pgrid, blk, 0, ctx->stream, (int64_t)p0, (int64_t)p1, gr.r0, gr.r1, d_poff, nf, st, pt, pp, d_err);
                    XC_HIP(ctx, hipGetLastError());
                }
                mark(6);
            }
        } else {
            mark(2);
        }
        hipLaunchKernelGGL(k_cp_unscatter, grid, blk, 0, ctx->stream, n, s0, E, (const long long*)e_from, rid, tab);
        XC_HIP(ctx, hipGetLastError());
        mark(0);
    }
    for (; done < nrange; ++done) poff[(size_t)done + 1] = poff[(size_t)done] + (long long)hp[(size_t)done];
    ctx->cpprops_rounds = rounds_total; ctx->cpprops_groups = (int)groups.size();
    const long long np = poff[(size_t)nrange];
    int herr = 0;
    XC_HIP(ctx, hipMemcpyAsync(&herr, d_err, 4, hipMemcpyDeviceToHost, ctx->stream));
    XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (herr & CP_ERR_EDGE) { settle(); return fail(ctx, XC_EBADARG, std::string(who) + ": an edge id outside [0, 2 ny nx)"); }
    if (herr & CP_ERR_LINK) { settle(); return fail(ctx, XC_EBADARG, std::string(who) + ": the records are not those of one xc_contour_segments call (a repeated edge id)"); }
    if (herr) { settle(); return fail(ctx, XC_EBADARG, std::string(who) + ": the records are not those of one xc_contour_segments call (rings that enclose each other)"); }
    if (np > capacity) { settle(); return 1; }
    XC_HIP(ctx, hipMemcpyAsync(d_poff, poff.data(), (size_t)(nrange + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_pi_finish, dim3(cp_blocks(np)), blk, 0, ctx->stream, (int64_t)np, nrange, ncont, d_poff, st, mx, (long long*)first_edge,
                       (long long*)nseg, (int*)closed, (int*)winding, (long long*)n_in, sum_w, sum_wf);
    XC_HIP(ctx, hipGetLastError());
    mark(3);
    hipLaunchKernelGGL(k_pt_finish, dim3(cp_blocks(np)), blk, 0, ctx->stream, (int64_t)np, nrange, ncont, d_poff, st, pt, mx, (long long*)parent,
                       (int*)depth, (int*)nchild, (long long*)n_net, net_w, net_wf);
    XC_HIP(ctx, hipGetLastError());
    mark(4);
    if (nf > 0 || hasx) {
        hipLaunchKernelGGL(k_pp_finish, dim3(cp_blocks(np * (nf + hasx))), blk, 0, ctx->stream, (int64_t)np, nrange, ncont, nf, hasx, capacity,
                           d_poff, st, pp, mxg, net_g, sum_g, x_min, x_max, (long long*)at_min, (long long*)at_max);
        XC_HIP(ctx, hipGetLastError());
    }
    mark(6);
    XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    settle();
    return XC_OK;
}

}  // namespace xc

// ------------------------------------------------------------------------------------ C ABI
int xc_contour_piece_props_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to,
                               const double* pts, int64_t ny, int64_t nx, int periodic, int flip, int ncont, const double* w,
                               int w_per_slab, const void* f, int f_dtype, int64_t capacity, uint64_t* piece_count, int64_t* first_edge,
                               int64_t* nseg, int32_t* closed, int32_t* winding, int64_t* n_in, double* sum_w, double* sum_wf,
                               int64_t* parent, int32_t* depth, int32_t* nchild, int64_t* n_net, double* net_w, double* net_wf,
                               int nf, const void* const* g, const int* g_dtype, const int* g_per_slab, const void* x, int x_dtype,
                               double* net_g, double* sum_g, double* x_min, double* x_max, int64_t* at_min, int64_t* at_max)
{
    XC_CTX(ctx);
    return xc::launch_contour_piece_props(ctx, nrange, count, e_from, e_to, pts, ny, nx, periodic, flip, ncont, w, w_per_slab, f, f_dtype,
                                          capacity, piece_count, first_edge, nseg, closed, winding, n_in, sum_w, sum_wf, parent, depth,
                                          nchild, n_net, net_w, net_wf, nf, g, g_dtype, g_per_slab, x, x_dtype, net_g, sum_g, x_min, x_max,
                                          at_min, at_max);
}

int xc_last_cpprops_profile(xc_ctx* ctx, double* ms, int* rounds, int* groups)
{
    if (!ctx) return xc::fail(nullptr, XC_EBADARG, "null context");
    if (ms) for (int k = 0; k < 7; ++k) ms[k] = (double)ctx->cpprops_ms[k];
    if (rounds) *rounds = ctx->cpprops_rounds;
    if (groups) *groups = ctx->cpprops_groups;
    return XC_OK;
}

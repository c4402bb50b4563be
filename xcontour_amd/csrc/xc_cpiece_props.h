// K21 -- what every ring HOLDS of further fields (gfx950): per ring the exact sums of up to XC_PROPS_MAXF fields over its NET nodes (the
// nodes K20 would label with the ring) and over its whole inside set, and the minimum and maximum of one field over its net nodes with the
// flat node each sits on, beside K19's records, from K12's segment records on the device.  No label map is allocated.
//
// The rule (include/xcontour_hip.h, K21 section).  The mapping is K20's scan (xc_cpiece_label.h): a column is scanned from
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
//
// This header holds K21's device code and the host steps that launch it; xc_cprecords.hip is the launcher.  Included inside
// namespace xc { namespace { ... } } after xc_cpiece_label.h.
#pragma once

constexpr int PP_PASS = 4;                    // fields of one pass of the scan
constexpr unsigned long long PP_NOKEY = ~0ull;  // no key yet (minimum), no place yet; the key of no value: a NaN's
constexpr unsigned long long PP_SIGN = 1ull << 63;

#include "xc_cpiece_field.h"

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

// the staged records of K21 for `cap` pieces and nf fields, taken from the launcher's carve (xc_carve.h)
inline void pp_carve(Carve& c, int64_t cap, int nf, PpStage& pp)
{
    const size_t n = (size_t)cap;
    pp.net = c.take<unsigned long long>(n * (size_t)nf * CP_L); pp.gro = c.take<unsigned long long>(n * (size_t)nf * CP_L);
    pp.kmin = c.take<unsigned long long>(n); pp.kmax = c.take<unsigned long long>(n);
    pp.amin = c.take<unsigned long long>(n); pp.amax = c.take<unsigned long long>(n);
    pp.flg = c.take<int>(n); pp.gflg = c.take<int>(n);
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

// ---------------------------------------------------------------- the host steps of K21, each launched from one place (xc_cprecords.hip)
// the scan of the ng ranges of a group.  Pass 1: the first PP_PASS fields and the keys of x; pass 2: the other fields and the places of
// the keys
inline void pp_launch_scan(hipStream_t stream, int64_t ng, int64_t rows, int64_t nchunk, int ncont, const PlGroup& g, const PiStage& st,
                           const PtStage& pt, const int* carry, const double* w, int w_per_slab, const PpField* fld, int nf, int hasx,
                           const unsigned long long* mxg, const PpStage& pp, int* err)
{
    const dim3 lgrid(cp_blocks(ng * nchunk * g.nx));                       // no more threads than the group's table has nodes
    const int n1 = std::min(nf, PP_PASS), n2 = nf - n1;
    if (hasx) pp_launch_pass<1>(n1, lgrid, stream, ng, rows, nchunk, ncont, g, st, pt, carry, w, w_per_slab, fld, 0, nf, mxg, pp, err);
    else pp_launch_pass<0>(n1, lgrid, stream, ng, rows, nchunk, ncont, g, st, pt, carry, w, w_per_slab, fld, 0, nf, mxg, pp, err);
    if (hasx) pp_launch_pass<2>(n2, lgrid, stream, ng, rows, nchunk, ncont, g, st, pt, carry, w, w_per_slab, fld, n1, nf, mxg, pp, err);
    else if (n2 > 0) pp_launch_pass<0>(n2, lgrid, stream, ng, rows, nchunk, ncont, g, st, pt, carry, w, w_per_slab, fld, n1, nf, mxg, pp, err);
}

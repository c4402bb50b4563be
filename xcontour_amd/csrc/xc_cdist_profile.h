// K28 -- composites by distance (xc_contour_distance_profile_dev; the rule is in include/xcontour_hip.h, K28 section): what it adds to
// K27's tile pass (included inside xc_cdist.hip's anonymous namespace after xc_cdist_search.h, xc_cpiece_sum.h and xc_cpiece_field.h).
// k_cd_profile runs cd_search and then bins the lane's distance into the caller's edges and adds the node, its weight and its weighted
// fields to the (range, bin)'s words -- K17's exact sums (xc_cpiece_sum.h), through an LDS window laid into the search's segment chunk,
// or straight to memory where the tile spans more than CDP_SPAN bins; k_cd_profile_finish rounds the words once.  No plane is written.
//
// Its LDS is the segment chunk of the search (sseg), free once the search is over: the smaller one, the plane's
// CD_CHUNK * CD_ND_PLANE = 1280 64-bit words, holds CDP_EDGES_LDS edges, the window of CDP_SPAN bins x CDP_MAXCH channels x CP_L words and
// the window's counts -- the profile kernel has the LDS footprint of k_cd_dist and its occupancy.
//   CDP_SPAN 16: the distances of a 16 x 16 tile span at most its diagonal, so a tile touches more than 16 bins only where the bins are
//   narrower than 1/11 of a tile (the wide-span fallback); 16 x 9 x 5 = 720 words, with 512 edges 1232 + 8 words of counts <= 1280.
#pragma once

constexpr int CDP_SPAN = 16;                  // bins of the LDS window
constexpr int CDP_MAXCH = 1 + XC_PROPS_MAXF;  // channels: the area, then the fields
constexpr int CDP_EDGES_LDS = 512;            // edges kept in LDS; a longer table is read through the cache
constexpr int CDP_MAX_EDGES = 4097;

// What K28 adds to a tile pass.  A node with the final distance d belongs to bin b when edges[b] <= d < edges[b + 1]; d == edges[M]
// belongs to bin M - 1 (np.histogram's rule); a node with d = +inf, or outside [edges[0], edges[M]], belongs nowhere.  Per (range, bin):
// the nodes, and per channel (0: the area w; 1 + m: w f_m, the product rounded once) the CP_L words of the exact sum (xc_cpiece_sum.h).
struct CdProf {
    int nedge, nf, ncont, global;                                          // edges; fields; ranges per slab; every tile takes the global path
    const double *edges, *w; int w_per_slab; const PpField* fld;
    const unsigned long long *mxw, *mxg;                                   // the bounds: mxw[2 s] of |w|, mxg[s nf + m] of |w f_m|
    unsigned long long *acc, *cnt; int* bflag;                             // acc[range][bin][channel][CP_L], cnt[range][bin], bflag[range][bin][channel]
    unsigned long long* tiles;                                             // tiles that took the LDS window, the global path
};

// the bin of d among the nedge ascending edges e, -1 for none: the number of edges <= d, less one, the last edge closed
__device__ __forceinline__ int cdp_bin(double d, const double* e, int nedge)
{
    if (!(d >= e[0]) || !(d <= e[nedge - 1])) return -1;
    int lo = 0, hi = nedge;
    while (lo < hi) {                                                      // at most 13 steps
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= d) lo = mid + 1; else hi = mid;
    }
    return lo == nedge ? nedge - 2 : lo - 1;
}

// One workgroup per tile per range, as k_cd_dist: K27's search, then the accumulation.  The workgroup's lanes span bins [bmin, bmax].
// Up to CDP_SPAN bins (and unless P.global): every term is added whole to a window of LDS words with LDS integer atomics, then every
// non-zero word goes to the global words with one 64-bit atomic.  More: every term goes to the global words (cp_add).  Integer sums of
// the same chunks either way: the same words.
template <bool SPHERE>
__global__ __launch_bounds__(CD_TPB)
void k_cd_profile(const CdArgs A, const CdProf P)
{
    constexpr int ND = SPHERE ? CD_ND_SPHERE : CD_ND_PLANE;
    constexpr int WIN = CDP_SPAN * CDP_MAXCH * CP_L;
    static_assert(CDP_EDGES_LDS + WIN + (CDP_SPAN + 1) / 2 <= CD_CHUNK * CD_ND_PLANE, "K28's window lives in the search's segment chunk");
    __shared__ double sseg[CD_CHUNK * ND];
    __shared__ int sid[CD_CHUNK];
    __shared__ double sred[CD_TPB / 64];
    __shared__ int stop[CDP_MAXCH];
    const CdHit h = cd_search<SPHERE>(A, sseg, sid, sred);
    const int t = threadIdx.x;
    const int nch = 1 + P.nf, M = P.nedge - 1;
    const size_t sl = (size_t)(h.r / P.ncont);
    double* sedge = sseg;                                                  // the chunk is free once every lane has left the search
    unsigned long long* swin = reinterpret_cast<unsigned long long*>(sseg) + CDP_EDGES_LDS;
    unsigned* scnt = reinterpret_cast<unsigned*>(swin + WIN);
    const bool lds_edges = P.nedge <= CDP_EDGES_LDS;
    __syncthreads();
    if (lds_edges) for (int i = t; i < P.nedge; i += CD_TPB) sedge[i] = P.edges[i];
    if (t < nch) stop[t] = t == 0 ? ci_top(P.mxw[2 * sl]) : ci_top(P.mxg[sl * (size_t)P.nf + (size_t)(t - 1)]);
    __syncthreads();
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    const int b = h.valid && h.bslot >= 0 ? cdp_bin(h.d, lds_edges ? sedge : P.edges, P.nedge) : -1;
    const double dmin = cd_wg_min(b >= 0 ? (double)b : inf, sred), dmax = cd_wg_max(b >= 0 ? (double)b : -inf, sred);
    if (!(dmin <= dmax)) return;                                           // no node of the tile lies in a bin (uniform)
    const int bmin = (int)dmin, span = (int)dmax - bmin + 1;
    const bool window = span <= CDP_SPAN && !P.global;
    if (t == 0) atomicAdd(P.tiles + (window ? 0 : 1), 1ull);
    if (window) {
        for (int i = t; i < span * nch * CP_L; i += CD_TPB) swin[i] = 0ull;
        if (t < span) scnt[t] = 0u;
        __syncthreads();
    }
    if (b >= 0) {
        const size_t node = (size_t)h.row * (size_t)A.nx + (size_t)h.col, npl = (size_t)A.ny * (size_t)A.nx;
        const size_t gbin = (size_t)h.r * (size_t)M + (size_t)b;
        unsigned long long* words = window ? swin + (size_t)(b - bmin) * (size_t)nch * CP_L : P.acc + gbin * (size_t)nch * CP_L;
        if (window) atomicAdd(scnt + (b - bmin), 1u); else atomicAdd(P.cnt + gbin, 1ull);
        const double wv = P.w ? P.w[(P.w_per_slab ? sl * npl : 0) + node] : 1.0;
        for (int ch = 0; ch < nch; ++ch) {
            const double v = ch == 0 ? wv : __dmul_rn(wv, pp_load(P.fld[ch - 1], sl, node));
            if (v == v) cp_add(words + ch * CP_L, P.bflag + gbin * (size_t)nch + (size_t)ch, 1, v, stop[ch]);
        }
    }
    if (!window) return;
    __syncthreads();
    unsigned long long* dst = P.acc + ((size_t)h.r * (size_t)M + (size_t)bmin) * (size_t)nch * CP_L;
    for (int i = t; i < span * nch * CP_L; i += CD_TPB) { const unsigned long long v = swin[i]; if (v) atomicAdd(dst + i, v); }
    if (t < span && scnt[t]) atomicAdd(P.cnt + (size_t)h.r * (size_t)M + (size_t)(bmin + t), (unsigned long long)scnt[t]);
}

// one thread per (range, bin, channel): the words carried and rounded once; a flagged sum is NaN and sets the caller's flag word of its
// (range, channel)
__global__ __launch_bounds__(CP_TPB)
void k_cd_profile_finish(int64_t nrange, int M, int nf, int ncont, const unsigned long long* __restrict__ acc,
                         const unsigned long long* __restrict__ cnt, const int* __restrict__ bflag, const unsigned long long* __restrict__ mxw,
                         const unsigned long long* __restrict__ mxg, long long* __restrict__ nodes, double* __restrict__ area,
                         double* __restrict__ sums, int* __restrict__ flags)
{
    const int nch = 1 + nf;
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= nrange * M * nch) return;
    const int ch = (int)(i % nch);
    const int64_t rb = i / nch, r = rb / M, s = r / ncont;
    const int top = ch == 0 ? ci_top(mxw[2 * s]) : ci_top(mxg[(size_t)s * nf + (ch - 1)]);
    const bool bad = bflag[i] != 0;
    const double v = bad ? __longlong_as_double(0x7ff8000000000000ll) : cp_to_double(acc + (size_t)i * CP_L, top);
    if (bad) atomicOr(flags + r * nch + ch, 1);
    if (ch == 0) { nodes[rb] = (long long)cnt[rb]; area[rb] = v; }
    else sums[(size_t)(ch - 1) * (size_t)(nrange * M) + (size_t)rb] = v;
}

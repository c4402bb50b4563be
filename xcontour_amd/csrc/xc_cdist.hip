// K27 -- how far every node lies from a contour, and which part of it is nearest (gfx950): the distance from each node of the plane to
// the selected pieces of K12's segment records, on the device.
//
// K25 brought contour VECTORS back onto the plane; this brings the contour's geometry back: the cross-contour coordinate of every
// front-relative composite (distance from the vortex edge, from a jet axis, from an SSH front).  The reference's scripts get it by
// tracing a level and querying a KD-tree on the host (tests/test_breaking.py uses scipy.spatial).  Build-defined.
//
// Input: count[nrange], e_from, e_to, pts as xc_contour_segments[_periodic]_dev wrote them; pieces, rings, winding, `select` and the main
// ring's tie rule are K16's (xc_cpiece_select.h); ycoord, xcoord, period, radius with K13's meaning: a record end point (rho, gamma) maps
// to coordinates as K13 maps it (np.interp on the node floor(.), column nx of a periodic plane at xcoord[0] + period); node (r, c) is
// (ycoord[r], xcoord[c]).  xc_cdist_metric.h states the two metrics, operation by operation.
//   plane  (radius == 0): d2 of xc_cdist_metric.h; with `periodic` the minimum over px, px + period, px - period; dist = sqrt(min d2)
//   sphere (radius > 0, radians): c2 of xc_cdist_metric.h; dist = radius * 2 asin(min(1, sqrt(min c2) / 2)), one asin per node
//   edge   the e_from of the segment with the smallest d2 / c2, the smallest id among equal bit patterns;  piece  its piece's first_edge
//   dist = +inf, edge = piece = -1 where the range has no selected segment, or the distance exceeds max_dist (> 0 and finite);
//   negate_mask flips the sign of every finite dist where it is 1.
// min is order-free: no output depends on the order of the segments, of arrival, on the launch geometry or on the workspace cap.
//
// Per GROUP of consecutive ranges (xc_cpiece_link.h: K13's groups under K13's cap, indices group-local):
//   phase A (K13's kernels), k_co_root, k_co_piece, k_co_pick (K16's selection)
//   k_cd_count      one thread per segment of a selected piece: its coarse BLOCK is the CD_B x CD_B cells around the cell of e_from; one
//                   integer atomic add per segment
//   k_cd_scan       one workgroup per range: the exclusive scan of the block counts (where each block's segments start in the table),
//                   the cursors, and the list of the non-empty blocks
//   k_cd_fill       one thread per selected segment: its slot from the block's cursor, then the segment in metric space -- plane:
//                   (a, u, uu), sphere: (a, b, n, nn) as unit vectors --, its id and its piece's first_edge.  Order inside a block is
//                   whatever the atomics gave: nothing depends on it.
//   k_cd_box        one thread per non-empty block: the box that holds every foot the metric can compute on its segments
//   k_cp_unscatter  the table is handed on clean
//   k_cd_dist       one workgroup per tile of CD_T x CD_T nodes per range, one node per lane (the search is the device function
//                   cd_search, which K28's k_cd_profile calls too).  The tile's own box; with pruning an upper
//                   bound W on every node's result from the far distance to the nearest block; then every non-empty block whose lower
//                   bound does not exceed W (or max_dist) is staged through LDS in chunks of CD_CHUNK segments and every lane takes the
//                   minimum; W shrinks to the tile's worst best-distance after every block.  The bounds are conservative
//                   (xc_cdist_metric.h says why), so a skipped block holds no segment that could win or tie: pruned and unpruned
//                   results are the same bits.
// Ranges outside every group have no segment: k_cd_none writes their planes.  Every index taken from a record is checked before any
// output is written (k_cd_check): a refusal writes nothing.
//
// K28 -- composites by distance (xc_contour_distance_profile_dev; the rule is in include/xcontour_hip.h, K28 section).  The same launcher
// and the same phases up to the tile pass; k_cd_profile runs cd_search and then bins the lane's distance into the caller's edges and adds
// the node, its weight and its weighted fields to the (range, bin)'s words -- K17's exact sums (xc_cpiece_sum.h), through an LDS window
// laid into the search's segment chunk, or straight to memory where the tile spans more than CDP_SPAN bins; k_cd_profile_finish rounds
// the words once.  No plane is written.
#include "xc_capi.h"
#include <algorithm>
#include <cmath>
#include <string>
#include <type_traits>
#include <vector>

namespace xc {
namespace {

#include "xc_binning.h"
#include "xc_clen_cell.h"

#include "xc_cpiece_link.h"
#include "xc_cpiece_select.h"
#include "xc_cpiece_sum.h"
#include "xc_cinside_bound.h"
#include "xc_cpiece_field.h"
#include "xc_cdist_metric.h"

constexpr int CD_T = 16;                      // a tile of nodes is CD_T x CD_T: one node per lane of a CD_TPB workgroup
constexpr int CD_TPB = CD_T * CD_T;
constexpr int CD_CHUNK = 256;                 // segments of a block staged through LDS at a time
constexpr int CD_B = 32;                      // a coarse block is CD_B x CD_B cells
constexpr int CD_NBOX_PLANE = 4, CD_NBOX_SPHERE = 6;

// K28's accumulation.  Its LDS is the segment chunk of the search (sseg), free once the search is over: the smaller one, the plane's
// CD_CHUNK * CD_ND_PLANE = 1280 64-bit words, holds CDP_EDGES_LDS edges, the window of CDP_SPAN bins x CDP_MAXCH channels x CP_L words and
// the window's counts -- the profile kernel has the LDS footprint of k_cd_dist and its occupancy.
//   CDP_SPAN 16: the distances of a 16 x 16 tile span at most its diagonal, so a tile touches more than 16 bins only where the bins are
//   narrower than 1/11 of a tile (the wide-span fallback); 16 x 9 x 5 = 720 words, with 512 edges 1232 + 8 words of counts <= 1280.
constexpr int CDP_SPAN = 16;                  // bins of the LDS window
constexpr int CDP_MAXCH = 1 + XC_PROPS_MAXF;  // channels: the area, then the fields
constexpr int CDP_EDGES_LDS = 512;            // edges kept in LDS; a longer table is read through the cache
constexpr int CDP_MAX_EDGES = 4097;

__global__ __launch_bounds__(CP_TPB)
void k_cd_check(int64_t total, long long E, const long long* __restrict__ e_from, const long long* __restrict__ e_to, int* __restrict__ err)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= total) return;
    const long long a = e_from[i], b = e_to[i];
    if (a < 0 || a >= E || b < 0 || b >= E) *err = CP_ERR_EDGE;
}

// the planes of the ranges [ra, rb): no selected segment
__global__ __launch_bounds__(CP_TPB)
void k_cd_none(size_t at, size_t n, double* __restrict__ dist, long long* __restrict__ edge, long long* __restrict__ piece)
{
    const size_t i = (size_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= n) return;
    dist[at + i] = __longlong_as_double(0x7ff0000000000000ll);
    if (edge) edge[at + i] = -1;
    if (piece) piece[at + i] = -1;
}

// cos and sin of the coordinates, once per row and column: cy, sy [ny], cx, sx [nx]
__global__ __launch_bounds__(CP_TPB)
void k_cd_trig(int64_t ny, int64_t nx, const double* __restrict__ fy, const double* __restrict__ fx, double* __restrict__ trig)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i < ny) { trig[i] = cos(fy[i]); trig[ny + i] = sin(fy[i]); }
    if (i < nx) { trig[2 * ny + i] = cos(fx[i]); trig[2 * ny + nx + i] = sin(fx[i]); }
}

// the coarse block of the cell of an edge id in [0, E)
__device__ __forceinline__ int64_t cd_block_of(long long e, int64_t nx, int64_t nbc)
{
    const long long node = e >> 1, row = node / nx, col = node - row * nx;
    return (int64_t)(row / CD_B) * nbc + (int64_t)(col / CD_B);
}

// whether segment i of the group is one of a selected piece (with a checked id)
__device__ __forceinline__ bool cd_takes(int64_t i, long long s0, int64_t r0, long long E, int select, const long long* __restrict__ e_from,
                                         const int* __restrict__ rid, const int* __restrict__ root, const int* __restrict__ prv,
                                         const int* __restrict__ lab, const unsigned* __restrict__ pn, const int* __restrict__ pw,
                                         const unsigned long long* __restrict__ key)
{
    int w; bool ismain;
    const long long ef = e_from[s0 + i];
    return ef >= 0 && ef < E && co_selected(select, prv[i] >= 0, root[i], lab[i], pn, pw, key[r0 + rid[i]], w, ismain);
}

#define XC_CD_SEL int select, const long long* __restrict__ e_from, const int* __restrict__ rid, const int* __restrict__ root, \
                  const int* __restrict__ prv, const int* __restrict__ lab, const unsigned* __restrict__ pn, const int* __restrict__ pw, \
                  const unsigned long long* __restrict__ key

__global__ __launch_bounds__(CP_TPB)
void k_cd_count(int64_t n, long long s0, int64_t r0, long long E, int64_t nx, int64_t nbc, int64_t nb, XC_CD_SEL, int* __restrict__ bcnt)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= n) return;
    if (!cd_takes(i, s0, r0, E, select, e_from, rid, root, prv, lab, pn, pw, key)) return;
    atomicAdd(bcnt + (size_t)rid[i] * (size_t)nb + (size_t)cd_block_of(e_from[s0 + i], nx, nbc), 1);
}

// One workgroup per range of the group.  bcnt[g][nb]: counts in, cursors (the exclusive scan) out; lcount[g], and per non-empty block in
// ascending block order lstart, lcnt.  Both scans ride in one 64-bit word: the count above, the non-empty flag below.
__global__ __launch_bounds__(CP_TPB)
void k_cd_scan(int64_t nb, int* __restrict__ bcnt, int* __restrict__ lcount, int* __restrict__ lstart, int* __restrict__ lcnt)
{
    __shared__ unsigned long long sh[CP_TPB];
    __shared__ unsigned long long carry;
    const int64_t g = blockIdx.x;
    const int t = threadIdx.x;
    int* bc = bcnt + (size_t)g * (size_t)nb;
    if (t == 0) carry = 0ull;
    __syncthreads();
    for (int64_t base = 0; base < nb; base += CP_TPB) {
        const int64_t i = base + t;
        const int v = i < nb ? bc[i] : 0;
        const unsigned long long mine = ((unsigned long long)(unsigned)v << 32) | (v > 0 ? 1ull : 0ull);
        sh[t] = mine;
        __syncthreads();
        for (int d = 1; d < CP_TPB; d <<= 1) {
            const unsigned long long add = t >= d ? sh[t - d] : 0ull;
            __syncthreads();
            sh[t] += add;
            __syncthreads();
        }
        const unsigned long long excl = carry + sh[t] - mine;
        if (i < nb) {
            bc[i] = (int)(excl >> 32);
            if (v > 0) {
                const size_t at = (size_t)g * (size_t)nb + (size_t)(excl & 0xffffffffull);
                lstart[at] = (int)(excl >> 32); lcnt[at] = v;
            }
        }
        __syncthreads();
        if (t == CP_TPB - 1) carry += sh[t];
        __syncthreads();
    }
    if (t == 0) lcount[g] = (int)(carry & 0xffffffffull);
}

// index space -> coordinates, as K13's k_cp_reduce maps an end point
__device__ __forceinline__ double cd_ycoord(double rr, int64_t ny, const double* __restrict__ fy)
{
    int64_t i0 = (int64_t)floor(rr);
    i0 = i0 < 0 ? 0 : (i0 > ny - 1 ? ny - 1 : i0);
    const int64_t i1 = i0 + 1 < ny ? i0 + 1 : ny - 1;
    return interp_at(rr, (double)i0, fy[i0], fy[i1]);
}
__device__ __forceinline__ double cd_xcoord(double cc, int64_t nx, int wrap, double period, const double* __restrict__ fx)
{
    const int64_t cmax = wrap ? nx : nx - 1;                               // the last node column; column nx is column 0 one period on
    int64_t j0 = (int64_t)floor(cc);
    j0 = j0 < 0 ? 0 : (j0 > cmax ? cmax : j0);
    const int64_t j1 = j0 + 1 < cmax ? j0 + 1 : cmax;
    const double x0 = j0 < nx ? fx[j0] : __dadd_rn(fx[0], period), x1 = j1 < nx ? fx[j1] : __dadd_rn(fx[0], period);
    return interp_at(cc, (double)j0, x0, x1);
}

template <bool SPHERE>
__global__ __launch_bounds__(CP_TPB)
void k_cd_fill(int64_t n, long long s0, int64_t r0, long long E, int64_t ny, int64_t nx, int64_t nbc, int64_t nb, int wrap, double period,
               XC_CD_SEL, const long long* __restrict__ off, const double* __restrict__ pts, const double* __restrict__ fy,
               const double* __restrict__ fx, int* __restrict__ bcnt, double* __restrict__ tseg, int* __restrict__ tid, int* __restrict__ tpiece)
{
    constexpr int ND = SPHERE ? CD_ND_SPHERE : CD_ND_PLANE;
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= n) return;
    if (!cd_takes(i, s0, r0, E, select, e_from, rid, root, prv, lab, pn, pw, key)) return;
    const int r = rid[i];
    const long long ef = e_from[s0 + i];
    const long long base = off[r0 + r] - s0, cnt = off[r0 + r + 1] - off[r0 + r];
    const long long slot = atomicAdd(bcnt + (size_t)r * (size_t)nb + (size_t)cd_block_of(ef, nx, nbc), 1);
    if (slot < 0 || slot >= cnt) return;                                   // (the cursors of one range hand out fewer slots than it has segments)
    const size_t at = (size_t)(base + slot);
    const double2 pa = *reinterpret_cast<const double2*>(pts + 4 * (size_t)(s0 + i)), pb = *reinterpret_cast<const double2*>(pts + 4 * (size_t)(s0 + i) + 2);
    const double y1 = cd_ycoord(pa.x, ny, fy), y2 = cd_ycoord(pb.x, ny, fy);
    const double x1 = cd_xcoord(pa.y, nx, wrap, period, fx), x2 = cd_xcoord(pb.y, nx, wrap, period, fx);
    double* o = tseg + at * ND;
    if constexpr (SPHERE) {
        const double c1 = cos(y1), c2 = cos(y2);
        const CdV a = {__dmul_rn(c1, cos(x1)), __dmul_rn(c1, sin(x1)), sin(y1)}, b = {__dmul_rn(c2, cos(x2)), __dmul_rn(c2, sin(x2)), sin(y2)};
        const CdV nv = cd_cross(a, {__dsub_rn(b.x, a.x), __dsub_rn(b.y, a.y), __dsub_rn(b.z, a.z)});     // (xc_cdist_metric.h: why not a x b)
        o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = b.x; o[4] = b.y; o[5] = b.z; o[6] = nv.x; o[7] = nv.y; o[8] = nv.z; o[9] = cd_dot(nv, nv);
    } else {
        const double uy = __dsub_rn(y2, y1), ux = __dsub_rn(x2, x1);
        o[0] = y1; o[1] = x1; o[2] = uy; o[3] = ux; o[4] = cd_sq2(uy, ux);
    }
    tid[at] = (int)ef;
    tpiece[at] = lab[i];
}

// one thread per (range of the group, non-empty block): the block's box (xc_cdist_metric.h)
template <bool SPHERE>
__global__ __launch_bounds__(CP_TPB)
void k_cd_box(int64_t ng, int64_t nb, long long s0, int64_t r0, const long long* __restrict__ off, const int* __restrict__ lcount,
              const int* __restrict__ lstart, const int* __restrict__ lcnt, const double* __restrict__ tseg, double* __restrict__ box)
{
    constexpr int ND = SPHERE ? CD_ND_SPHERE : CD_ND_PLANE, NBOX = SPHERE ? CD_NBOX_SPHERE : CD_NBOX_PLANE;
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= ng * nb) return;
    const int64_t g = i / nb, k = i - g * nb;
    if (k >= lcount[g]) return;
    const long long base = off[r0 + g] - s0, cnt = off[r0 + g + 1] - off[r0 + g];
    long long a0 = lstart[i], a1 = a0 + lcnt[i];
    if (a0 < 0) a0 = 0;
    if (a1 > cnt) a1 = cnt;
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
    for (long long j = a0; j < a1; ++j) {
        const double* s = tseg + (size_t)(base + j) * ND;
        if constexpr (SPHERE) {
            const CdV a = {s[0], s[1], s[2]}, b = {s[3], s[4], s[5]};
            const double grow = cd_seg_grow(a, b, s[9]);
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                lo[d] = fmin(lo[d], __dsub_rn(fmin(s[d], s[3 + d]), grow));
                hi[d] = fmax(hi[d], __dadd_rn(fmax(s[d], s[3 + d]), grow));
            }
        } else {
#pragma unroll
            for (int d = 0; d < 2; ++d) {
                const double e = __dadd_rn(s[d], s[2 + d]);
                lo[d] = fmin(lo[d], fmin(s[d], e));
                hi[d] = fmax(hi[d], fmax(s[d], e));
            }
        }
    }
    double* o = box + (size_t)i * NBOX;
#pragma unroll
    for (int d = 0; d < NBOX / 2; ++d) { o[d] = lo[d]; o[NBOX / 2 + d] = hi[d]; }
}

// a workgroup's minimum / maximum: sh holds one double per wave
__device__ __forceinline__ double cd_wg_min(double v, double* sh)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = fmin(v, __shfl_xor(v, d));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    v = sh[0];
#pragma unroll
    for (int k = 1; k < CD_TPB / 64; ++k) v = fmin(v, sh[k]);
    return v;
}
__device__ __forceinline__ double cd_wg_max(double v, double* sh) { return -cd_wg_min(-v, sh); }

struct CdArgs {
    int64_t ra, g0, ny, nx, nty, ntx, nb;                                  // the first range of the launch, of the group; the plane, its tiles, its blocks
    int wrap, prune; double period, radius, cap; long long s0;
    const double *fy, *fx, *trig; const long long* off;
    const int *lcount, *lstart, *lcnt; const double *box, *tseg; const int *tid, *tpiece;
    const unsigned char* mask; double* dist; long long *edge, *piece; unsigned long long* pairs;
};

// what the search leaves a lane: its node, and the node's result as K27 stores it
struct CdHit {
    bool valid; int64_t r, row, col; size_t at;                            // the lane has a node; its range, the node, its place in a plane stack
    double d; int bid, bslot; long long base;                              // the final distance (sign and cap applied); the winner and its slot
};

// The per-tile search of K27, for K27 (k_cd_dist) and K28 (k_cd_profile): the node set-up, the bounds, the pruned walk over the blocks
// staged through LDS, and the finish to d.  sseg [CD_CHUNK * ND], sid [CD_CHUNK] and sred [CD_TPB / 64] are the workgroup's; every lane
// of the workgroup calls it (it holds barriers).  Lanes may still read sseg when it returns.
template <bool SPHERE>
__device__ __forceinline__ CdHit cd_search(const CdArgs& A, double* sseg, int* sid, double* sred)
{
    constexpr int ND = SPHERE ? CD_ND_SPHERE : CD_ND_PLANE, NBOX = SPHERE ? CD_NBOX_SPHERE : CD_NBOX_PLANE;
    const int64_t ntile = A.nty * A.ntx;
    const int64_t tile = (int64_t)blockIdx.x % ntile, r = A.ra + (int64_t)blockIdx.x / ntile, g = r - A.g0;
    const int64_t tr = tile / A.ntx, tc = tile - tr * A.ntx;
    const int t = threadIdx.x;
    const int64_t row = tr * CD_T + (t >> 4), col = tc * CD_T + (t & 15);
    const bool valid = row < A.ny && col < A.nx;
    const int64_t rr = row < A.ny ? row : A.ny - 1, cc = col < A.nx ? col : A.nx - 1;      // a lane off the plane shadows a node of the tile
    const double inf = __longlong_as_double(0x7ff0000000000000ll);

    // the node, and the tile's box
    double py = 0.0, px[3] = {0.0, 0.0, 0.0};
    CdV p = {0.0, 0.0, 0.0};
    double tlo[3], thi[3], txlo[3], txhi[3];
    int nimg = 1;
    if constexpr (SPHERE) {
        const double cy = A.trig[rr], sy = A.trig[A.ny + rr], cx = A.trig[2 * A.ny + cc], sx = A.trig[2 * A.ny + A.nx + cc];
        p = {__dmul_rn(cy, cx), __dmul_rn(cy, sx), sy};
        tlo[0] = cd_wg_min(p.x, sred); thi[0] = cd_wg_max(p.x, sred);
        tlo[1] = cd_wg_min(p.y, sred); thi[1] = cd_wg_max(p.y, sred);
        tlo[2] = cd_wg_min(p.z, sred); thi[2] = cd_wg_max(p.z, sred);
    } else {
        py = A.fy[rr]; px[0] = A.fx[cc];
        if (A.wrap) { nimg = 3; px[1] = __dadd_rn(px[0], A.period); px[2] = __dsub_rn(px[0], A.period); }
        tlo[0] = cd_wg_min(py, sred); thi[0] = cd_wg_max(py, sred);
        for (int k = 0; k < nimg; ++k) { txlo[k] = cd_wg_min(px[k], sred); txhi[k] = cd_wg_max(px[k], sred); }
    }
    // conservative bounds of the tile against the box b (xc_cdist_metric.h): squared on the plane, plain distances on the sphere
    auto lower = [&](const double* b) {
        if constexpr (SPHERE) {
            double s = 0.0;
            for (int d = 0; d < 3; ++d) { const double q = cd_gap(tlo[d], thi[d], b[d], b[3 + d]); s += q * q; }
            return sqrt(s);
        } else {
            const double gy = cd_gap(tlo[0], thi[0], b[0], b[2]);
            double m = inf;
            for (int k = 0; k < nimg; ++k) { const double gx = cd_gap(txlo[k], txhi[k], b[1], b[3]); m = fmin(m, cd_sq2(gy, gx)); }
            return m;
        }
    };
    auto upper = [&](const double* b) {
        if constexpr (SPHERE) {
            double s = 0.0;
            for (int d = 0; d < 3; ++d) { const double q = cd_far(tlo[d], thi[d], b[d], b[3 + d]); s += q * q; }
            const double u = sqrt(s) + CD_SLACK;
            return u * u * (1.0 + 1e-12);
        } else {
            const double gy = cd_far(tlo[0], thi[0], b[0], b[2]);
            double m = inf;
            for (int k = 0; k < nimg; ++k) { const double gx = cd_far(txlo[k], txhi[k], b[1], b[3]); m = fmin(m, cd_sq2(gy, gx)); }
            return m;
        }
    };
    // whether a block with the lower bound lb cannot hold a winner under the squared bound w2
    auto beyond = [&](double lb, double w2) {
        if constexpr (SPHERE) { const double l = lb - CD_SLACK; return l > 0.0 && l * l > w2 * (1.0 + 1e-12); }
        else return lb > w2;
    };
    // the cap as a bound on the squared metric that no capped-away candidate stays below (sqrt and asin are monotone)
    double cap2 = inf;
    if (A.cap > 0.0 && A.cap < inf) {
        if constexpr (SPHERE) {
            const double h = A.cap / A.radius * 0.5;                       // dist > cap  <=  chord > 2 sin(h) (1 + slack)
            if (h < 1.5707963) { const double c = 2.0 * sin(h) * (1.0 + 1e-9) + CD_SLACK; cap2 = c * c; }
        } else {
            cap2 = A.cap * A.cap * (1.0 + 1e-12);                          // sqrt(d2) > cap for every d2 above this
        }
    }

    const int nl = A.lcount[g];
    const size_t lat = (size_t)g * (size_t)A.nb;
    const long long base = A.off[r] - A.s0, cnt = A.off[r + 1] - A.off[r];
    double w2 = cap2;
    if (A.prune && nl > 0) {
        double u = inf;
        for (int k = t; k < nl; k += CD_TPB) u = fmin(u, upper(A.box + (lat + k) * NBOX));
        w2 = fmin(w2, cd_wg_min(u, sred));
    }

    double best = inf;
    int bid = 0x7fffffff, bslot = -1;
    unsigned long long visited = 0ull, nsel = 0ull;
    for (int k = 0; k < nl; ++k) {
        long long a0 = A.lstart[lat + k], a1 = a0 + A.lcnt[lat + k];
        if (a0 < 0) a0 = 0;
        if (a1 > cnt) a1 = cnt;
        nsel += (unsigned long long)(a1 > a0 ? a1 - a0 : 0);
        if (A.prune && beyond(lower(A.box + (lat + k) * NBOX), w2)) continue;          // (uniform over the workgroup)
        visited += (unsigned long long)(a1 > a0 ? a1 - a0 : 0);
        for (long long c0 = a0; c0 < a1; c0 += CD_CHUNK) {
            const int m = (int)(a1 - c0 < CD_CHUNK ? a1 - c0 : CD_CHUNK);
            __syncthreads();
            if (t < m) {
                const double* s = A.tseg + (size_t)(base + c0 + t) * ND;
#pragma unroll
                for (int d = 0; d < ND; ++d) sseg[t * ND + d] = s[d];
                sid[t] = A.tid[base + c0 + t];
            }
            __syncthreads();
            for (int j = 0; j < m; ++j) {
                const double* s = sseg + j * ND;
                double d2;
                if constexpr (SPHERE) {
                    d2 = cd_c2_sphere(p, {s[0], s[1], s[2]}, {s[3], s[4], s[5]}, {s[6], s[7], s[8]}, s[9]);
                } else {
                    d2 = cd_d2_plane(py, px[0], s[0], s[1], s[2], s[3], s[4]);
                    if (nimg == 3) {
                        d2 = fmin(d2, cd_d2_plane(py, px[1], s[0], s[1], s[2], s[3], s[4]));
                        d2 = fmin(d2, cd_d2_plane(py, px[2], s[0], s[1], s[2], s[3], s[4]));
                    }
                }
                const int id = sid[j];
                if (d2 < best || (d2 == best && id < bid)) { best = d2; bid = id; bslot = (int)(c0 + j); }
            }
        }
        if (A.prune) w2 = fmin(w2, cd_wg_max(best, sred));
    }

    if (t == 0) {
        const int64_t ry = A.ny - tr * CD_T, rx = A.nx - tc * CD_T, vr = ry < CD_T ? ry : CD_T, vc = rx < CD_T ? rx : CD_T;
        atomicAdd(A.pairs, visited * (unsigned long long)(vr * vc));
        atomicAdd(A.pairs + 1, nsel * (unsigned long long)(vr * vc));
    }
    CdHit h = {valid, r, row, col, 0, inf, bid, -1, base};
    if (!valid) return h;
    double d = inf;
    if (bslot >= 0) {
        if constexpr (SPHERE) {
            const double hc = __dmul_rn(__dsqrt_rn(best), 0.5);
            d = __dmul_rn(A.radius, __dmul_rn(2.0, asin(hc < 1.0 ? hc : 1.0)));
        } else {
            d = __dsqrt_rn(best);
        }
        if (A.cap > 0.0 && d > A.cap) { d = inf; bslot = -1; }
    }
    h.at = ((size_t)r * (size_t)A.ny + (size_t)row) * (size_t)A.nx + (size_t)col;
    if (A.mask && bslot >= 0 && A.mask[h.at]) d = -d;
    h.d = d; h.bslot = bslot;
    return h;
}

template <bool SPHERE>
__global__ __launch_bounds__(CD_TPB)
void k_cd_dist(const CdArgs A)
{
    constexpr int ND = SPHERE ? CD_ND_SPHERE : CD_ND_PLANE;
    __shared__ double sseg[CD_CHUNK * ND];
    __shared__ int sid[CD_CHUNK];
    __shared__ double sred[CD_TPB / 64];
    const CdHit h = cd_search<SPHERE>(A, sseg, sid, sred);
    if (!h.valid) return;
    A.dist[h.at] = h.d;
    if (A.edge) A.edge[h.at] = h.bslot >= 0 ? (long long)h.bid : -1ll;
    if (A.piece) A.piece[h.at] = h.bslot >= 0 ? (long long)A.tpiece[h.base + h.bslot] : -1ll;
}

// ---------------------------------------------------------------------------------- K28: composites by distance
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

}  // namespace

// the period of a longitude ring in radians as the facade hands it over: float64(deg2rad(float32(360)))
static const double CD_RING = (double)6.2831855f;

// One call of xc_contour_distance_dev or xc_contour_distance_profile_dev: the caller's pointers and scalars in the order of the C ABI.
// `profile` says which: K27 writes planes, K28 bins them where they are made.
struct CdCall {
    const char* who; CpProfile* prof;
    int64_t nrange; const uint64_t* count; const int64_t *e_from, *e_to; const double* pts; int64_t ny, nx; int periodic, select;
    const double *ycoord, *xcoord; double period, radius, max_dist; const uint8_t* negate_mask;
    double* dist; int64_t *edge, *piece;
    bool profile; int nedge; const double* edges; int ncont; const double* w; int w_per_slab; int nf; const void* const* f;
    const int *f_dtype, *f_per_slab; int64_t* nodes; double *area, *sums; int32_t* flags;
};

// One call.  Waits for the stream three times: for K12's counts (they size the groups and fix the rounds), for the word that says whether
// the ids were in range (before anything is written), and for the pair counts of the profile.
static int launch_cdist(xc_ctx* ctx, const CdCall& c)
{
    const std::string who_s(c.who);
    auto refuse = [&](const char* what) { return fail(ctx, XC_EBADARG, who_s + what); };
    const char* who = c.who;
    const int64_t nrange = c.nrange, ny = c.ny, nx = c.nx;
    const int periodic = c.periodic;
    const double period = c.period, radius = c.radius, max_dist = c.max_dist;
    if (!c.count || !c.ycoord || !c.xcoord || nrange < 1 || ny < 1 || nx < 1) return refuse(": bad arguments");
    if (c.profile ? (!c.nodes || !c.area || !c.flags) : !c.dist) return refuse(": bad arguments");
    XC_TRY(co_check_select(ctx, who, periodic, c.select));
    if (!(radius >= 0.0) || !std::isfinite(radius)) return refuse(": radius must be finite and >= 0");
    if (periodic && (!std::isfinite(period) || period == 0.0 || nx < 2)) return refuse(": a periodic plane needs a finite, non-zero period and nx >= 2");
    if (radius > 0.0 && periodic && period != CD_RING && period != -CD_RING)
        return refuse(": on the sphere the period is float64(deg2rad(float32(+-360))): the plane is a sphere or none");
    if (max_dist != max_dist) return refuse(": max_dist is NaN");
    XC_TRY(co_check_plane(ctx, who, periodic, ny, nx));
    if (nrange > ((int64_t)1 << 40) / (ny * nx)) return refuse(": nrange ny nx must stay below 2^40");
    const int nf = c.profile ? c.nf : 0, M = c.profile ? c.nedge - 1 : 0, nch = 1 + nf;
    int64_t nslab = 1;
    if (c.profile) {
        bool ok = c.edges && c.nedge >= 2 && c.nedge <= CDP_MAX_EDGES;
        for (int i = 0; ok && i < c.nedge; ++i) ok = std::isfinite(c.edges[i]) && (i == 0 || c.edges[i] > c.edges[i - 1]);
        if (!ok) return refuse(": edges must be 2 to 4097 finite, strictly ascending float64 values");
        if (nf < 0 || nf > XC_PROPS_MAXF) return refuse(": at most 8 fields (XC_PROPS_MAXF)");
        if (nf > 0 && (!c.f || !c.f_dtype || !c.f_per_slab || !c.sums)) return refuse(": the fields, their dtypes and sums go together");
        for (int m = 0; m < nf; ++m)
            if (!c.f[m] || (c.f_dtype[m] != XC_F32 && c.f_dtype[m] != XC_F64)) return refuse(": a field is a device plane of XC_F32 or XC_F64");
        if (c.ncont < 1 || nrange % c.ncont != 0) return refuse(": nrange must be a multiple of ncont >= 1");
        nslab = nrange / c.ncont;
        if (nslab > 65535) return refuse(": more than 65535 slabs");
    }
    const long long E = 2 * ny * nx;
    const int wrap = periodic ? 1 : 0;
    const bool sphere = radius > 0.0;
    CpProfile& prof = *c.prof;
    profile_clear(prof);
    unsigned long long* hstat = c.profile ? ctx->cdprofile_stat : ctx->cdist_pairs;
    for (int i = 0; i < (c.profile ? 4 : 2); ++i) hstat[i] = 0;

    CpPlan pl;                                                               // (no group without segments: the outputs are written all the same)
    XC_TRY(cp_plan(ctx, who, nrange, c.count, nullptr, c.e_from, c.e_to, c.pts, E, pl));
    const int64_t nbr = (ny + CD_B - 1) / CD_B, nbc = (nx + CD_B - 1) / CD_B, nb = nbr * nbc;
    const int64_t nty = (ny + CD_T - 1) / CD_T, ntx = (nx + CD_T - 1) / CD_T, ntile = nty * ntx;
    const int nd = sphere ? CD_ND_SPHERE : CD_ND_PLANE, nbox = sphere ? CD_NBOX_SPHERE : CD_NBOX_PLANE;
    // workspace: off | key, nsel, err, pairs and tiles; K28: mxw, mxg, acc, cnt, bflag (cleared together) | K28: edges, fld | trig | per
    //            group: bcnt, lcount, lstart, lcnt, box | the segment table (tseg, tid, tpiece) | the tail (xc_cpiece_link.h)
    long long* d_off; unsigned long long *key, *pairs, *mxw, *mxg, *acc, *cnt; int *nsel, *d_err, *bflag, *bcnt, *lcount, *lstart, *lcnt, *tid, *tpiece;
    double *d_edges, *trig, *box, *tseg; PpField* d_fld; size_t b_zero = 0; CpTail tail;
    auto lay = [&](Carve a) {
        d_off = a.take<long long>((size_t)nrange + 1);
        b_zero = a.mark();
        key = a.take<unsigned long long>((size_t)nrange); nsel = a.take<int>((size_t)nrange); d_err = a.take<int>(CP_SMALL);
        pairs = a.take<unsigned long long>(4);
        const size_t nbin = c.profile ? (size_t)nrange * (size_t)M : 0;
        mxw = a.take<unsigned long long>(c.profile ? (size_t)nslab * 2 : 0);
        mxg = a.take<unsigned long long>(c.profile ? (size_t)nslab * (size_t)std::max(nf, 1) : 0);
        acc = a.take<unsigned long long>(nbin * (size_t)nch * CP_L); cnt = a.take<unsigned long long>(nbin); bflag = a.take<int>(nbin * (size_t)nch);
        b_zero = a.mark() - b_zero;
        d_edges = a.take<double>(c.profile ? (size_t)c.nedge : 0); d_fld = a.take<PpField>(c.profile ? XC_PROPS_MAXF : 0);
        trig = a.take<double>(sphere ? (size_t)(2 * ny + 2 * nx) : 0);
        const size_t gb = (size_t)pl.gmax * (size_t)nb;
        bcnt = a.take<int>(gb); lcount = a.take<int>((size_t)pl.gmax); lstart = a.take<int>(gb); lcnt = a.take<int>(gb);
        box = a.take<double>(gb * (size_t)nbox);
        tseg = a.take<double>((size_t)pl.nmax * (size_t)nd); tid = a.take<int>((size_t)pl.nmax); tpiece = a.take<int>((size_t)pl.nmax);
        cp_carve_tail(a, pl, 6, tail);
        return a.at;
    };
    XC_TRY(lay_out(ctx, &ctx->cpiece_ws, &ctx->cpiece_ws_bytes, lay));

    // the stages of the profiles: 0 table, 1 rounds, 2 select, 3 binning, 4 distance; K28: 5 bound, 6 finish
    StageTimer tm(ctx, prof.ms);                                             // where the time goes (xc_set_kernel_timing)
    CpRun run(ctx, tm, pl, c.e_from, c.e_to, d_off, tail, d_err);
    const dim3 blk(CP_TPB);
    const size_t npl = (size_t)ny * (size_t)nx;

    tm.mark(-1);
    XC_HIP(ctx, hipMemsetAsync(key, 0, b_zero, ctx->stream));
    if (pl.total > 0) {                                                      // the ids first: a refusal writes nothing
        hipLaunchKernelGGL(k_cd_check, dim3(cp_blocks(pl.total)), blk, 0, ctx->stream, (int64_t)pl.total, E, (const long long*)c.e_from,
                           (const long long*)c.e_to, d_err);
        XC_HIP(ctx, hipGetLastError());
        int herr = 0;
        XC_TRY(cp_read_err(ctx, d_err, &herr));
        if (herr) return refuse(": an edge id outside [0, 2 ny nx)");
    }
    if (sphere) {
        hipLaunchKernelGGL(k_cd_trig, dim3(cp_blocks(std::max(ny, nx))), blk, 0, ctx->stream, ny, nx, c.ycoord, c.xcoord, trig);
        XC_HIP(ctx, hipGetLastError());
    }
    tm.mark(3);
    PpField hfld[XC_PROPS_MAXF] = {};
    if (c.profile) {                                                         // the edges and the fields as the kernels read them; the windows' tops
        for (int m = 0; m < nf; ++m) hfld[m] = {c.f[m], c.f_per_slab[m] ? (unsigned long long)npl : 0ull, c.f_dtype[m] == XC_F32 ? 1 : 0, 0};
        XC_HIP(ctx, hipMemcpyAsync(d_edges, c.edges, (size_t)c.nedge * 8, hipMemcpyHostToDevice, ctx->stream));
        XC_HIP(ctx, hipMemcpyAsync(d_fld, hfld, sizeof(hfld), hipMemcpyHostToDevice, ctx->stream));
        ci_launch_bound(ctx->stream, (int64_t)npl, nslab, c.w, c.w_per_slab, nullptr, 0, mxw);
        if (nf > 0) pp_launch_bound(ctx->stream, (int64_t)npl, nslab, nf, c.w, c.w_per_slab, d_fld, mxg);
        XC_HIP(ctx, hipGetLastError());
        tm.mark(5);
    }
    XC_TRY(run.upload_off());
    XC_TRY(run.fill_table());
    tm.mark(0);

    // K27: the planes of the ranges [a, b) without any segment (K28's words of such a range stay zero)
    auto none = [&](int64_t a, int64_t b) -> int {
        if (c.profile) return XC_OK;
        for (int64_t r = a; r < b; ++r) {
            hipLaunchKernelGGL(k_cd_none, dim3((unsigned)((npl + CP_TPB - 1) / CP_TPB)), blk, 0, ctx->stream, (size_t)r * npl, npl, c.dist,
                               (long long*)c.edge, (long long*)c.piece);
        }
        XC_HIP(ctx, hipGetLastError());
        return XC_OK;
    };
    CdArgs A;
    A.ny = ny; A.nx = nx; A.nty = nty; A.ntx = ntx; A.nb = nb; A.wrap = wrap; A.prune = ctx->cdist_prune; A.period = wrap ? period : 0.0;
    A.radius = radius; A.cap = (max_dist > 0.0 && std::isfinite(max_dist)) ? max_dist : 0.0;
    A.fy = c.ycoord; A.fx = c.xcoord; A.trig = trig; A.off = d_off; A.lcount = lcount; A.lstart = lstart; A.lcnt = lcnt; A.box = box; A.tseg = tseg;
    A.tid = tid; A.tpiece = tpiece; A.mask = c.negate_mask; A.dist = c.dist; A.edge = (long long*)c.edge; A.piece = (long long*)c.piece; A.pairs = pairs;
    CdProf P = {};
    if (c.profile) {
        P.nedge = c.nedge; P.nf = nf; P.ncont = c.ncont; P.global = ctx->cdprofile_global; P.edges = d_edges; P.w = c.w; P.w_per_slab = c.w_per_slab;
        P.fld = d_fld; P.mxw = mxw; P.mxg = mxg; P.acc = acc; P.cnt = cnt; P.bflag = bflag; P.tiles = pairs + 2;
    }

    int64_t done = 0;                                                       // the ranges written so far
    for (const CpGroup& g : pl.groups) {
        const int64_t ng = g.r1 - g.r0;
        XC_TRY(none(done, g.r0));
        XC_HIP(ctx, hipMemsetAsync(bcnt, 0, (size_t)ng * (size_t)nb * 4, ctx->stream));
        tm.mark(3);
        run.begin(g);
        XC_TRY(run.rounds());
        const CoRoles s = co_launch_select(run, wrap, nx, c.pts, c.select, nsel, key);
        XC_HIP(ctx, hipGetLastError());
        tm.mark(2);
#define XC_CD_SEL_ARGS c.select, run.e_from, tail.rid, s.root, run.b.prv, run.b.lab, s.pn, s.pw, key
        hipLaunchKernelGGL(k_cd_count, run.grid, blk, 0, ctx->stream, run.n, run.s0, g.r0, E, nx, nbc, nb, XC_CD_SEL_ARGS, bcnt);
        hipLaunchKernelGGL(k_cd_scan, dim3((unsigned)ng), blk, 0, ctx->stream, nb, bcnt, lcount, lstart, lcnt);
        const dim3 bgrid(cp_blocks(ng * nb));
        if (sphere) {
            hipLaunchKernelGGL((k_cd_fill<true>), run.grid, blk, 0, ctx->stream, run.n, run.s0, g.r0, E, ny, nx, nbc, nb, wrap, A.period,
                               XC_CD_SEL_ARGS, d_off, c.pts, c.ycoord, c.xcoord, bcnt, tseg, tid, tpiece);
            hipLaunchKernelGGL((k_cd_box<true>), bgrid, blk, 0, ctx->stream, ng, nb, run.s0, g.r0, d_off, lcount, lstart, lcnt, tseg, box);
        } else {
            hipLaunchKernelGGL((k_cd_fill<false>), run.grid, blk, 0, ctx->stream, run.n, run.s0, g.r0, E, ny, nx, nbc, nb, wrap, A.period,
                               XC_CD_SEL_ARGS, d_off, c.pts, c.ycoord, c.xcoord, bcnt, tseg, tid, tpiece);
            hipLaunchKernelGGL((k_cd_box<false>), bgrid, blk, 0, ctx->stream, ng, nb, run.s0, g.r0, d_off, lcount, lstart, lcnt, tseg, box);
        }
#undef XC_CD_SEL_ARGS
        XC_HIP(ctx, hipGetLastError());
        tm.mark(3);
        XC_TRY(run.end());
        // the tiles of the group's ranges: as many launches as keep a grid below 2^31 blocks
        const int64_t step = std::max<int64_t>(1, (((int64_t)1 << 31) - 1) / ntile);
        A.g0 = g.r0; A.s0 = run.s0;
        for (int64_t ra = g.r0; ra < g.r1; ra += step) {
            A.ra = ra;
            const dim3 grid((unsigned)(std::min<int64_t>(step, g.r1 - ra) * ntile));
            if (c.profile) {
                if (sphere) hipLaunchKernelGGL((k_cd_profile<true>), grid, dim3(CD_TPB), 0, ctx->stream, A, P);
                else hipLaunchKernelGGL((k_cd_profile<false>), grid, dim3(CD_TPB), 0, ctx->stream, A, P);
            } else {
                if (sphere) hipLaunchKernelGGL((k_cd_dist<true>), grid, dim3(CD_TPB), 0, ctx->stream, A);
                else hipLaunchKernelGGL((k_cd_dist<false>), grid, dim3(CD_TPB), 0, ctx->stream, A);
            }
            XC_HIP(ctx, hipGetLastError());
        }
        done = g.r1;
        tm.mark(4);
    }
    XC_TRY(none(done, nrange));
    tm.mark(4);
    if (c.profile) {
        const int64_t nout = nrange * M * nch;
        XC_HIP(ctx, hipMemsetAsync(c.flags, 0, (size_t)nrange * (size_t)nch * 4, ctx->stream));
        hipLaunchKernelGGL(k_cd_profile_finish, dim3(cp_blocks(nout)), blk, 0, ctx->stream, nrange, M, nf, c.ncont, acc, cnt, bflag, mxw, mxg,
                           (long long*)c.nodes, c.area, c.sums, (int*)c.flags);
        XC_HIP(ctx, hipGetLastError());
        tm.mark(6);
    }
    run.report(prof);
    XC_HIP(ctx, hipMemcpyAsync(hstat, pairs, c.profile ? 32 : 16, hipMemcpyDeviceToHost, ctx->stream));
    XC_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return XC_OK;
}

}  // namespace xc

// ------------------------------------------------------------------------------------ C ABI
int xc_contour_distance_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to, const double* pts,
                            int64_t ny, int64_t nx, int periodic, int select, const double* ycoord, const double* xcoord, double period,
                            double radius, double max_dist, const uint8_t* negate_mask, double* dist, int64_t* edge, int64_t* piece)
{
    XC_CTX(ctx);
    xc::CdCall c = {};
    c.who = "xc_contour_distance"; c.prof = &ctx->prof_cdist;
    c.nrange = nrange; c.count = count; c.e_from = e_from; c.e_to = e_to; c.pts = pts; c.ny = ny; c.nx = nx; c.periodic = periodic;
    c.select = select; c.ycoord = ycoord; c.xcoord = xcoord; c.period = period; c.radius = radius; c.max_dist = max_dist;
    c.negate_mask = negate_mask; c.dist = dist; c.edge = edge; c.piece = piece;
    return xc::launch_cdist(ctx, c);
}

int xc_contour_distance_profile_dev(xc_ctx* ctx, int64_t nrange, const uint64_t* count, const int64_t* e_from, const int64_t* e_to,
                                    const double* pts, int64_t ny, int64_t nx, int periodic, int select, const double* ycoord,
                                    const double* xcoord, double period, double radius, double max_dist, const uint8_t* negate_mask,
                                    int nedge, const double* edges, int ncont, const double* w, int w_per_slab, int nf, const void* const* f,
                                    const int* f_dtype, const int* f_per_slab, int64_t* nodes, double* area, double* sums, int32_t* flags)
{
    XC_CTX(ctx);
    xc::CdCall c = {};
    c.who = "xc_contour_distance_profile"; c.prof = &ctx->prof_cdprofile;
    c.nrange = nrange; c.count = count; c.e_from = e_from; c.e_to = e_to; c.pts = pts; c.ny = ny; c.nx = nx; c.periodic = periodic;
    c.select = select; c.ycoord = ycoord; c.xcoord = xcoord; c.period = period; c.radius = radius; c.max_dist = max_dist;
    c.negate_mask = negate_mask;
    c.profile = true; c.nedge = nedge; c.edges = edges; c.ncont = ncont; c.w = w; c.w_per_slab = w_per_slab; c.nf = nf; c.f = f;
    c.f_dtype = f_dtype; c.f_per_slab = f_per_slab; c.nodes = nodes; c.area = area; c.sums = sums; c.flags = flags;
    return xc::launch_cdist(ctx, c);
}

int xc_set_cdist_prune(xc_ctx* ctx, int on)
{
    if (!ctx) return xc::fail(nullptr, XC_EBADARG, "null context");
    ctx->cdist_prune = on ? 1 : 0;
    return XC_OK;
}

int xc_set_cdprofile_global(xc_ctx* ctx, int on)
{
    if (!ctx) return xc::fail(nullptr, XC_EBADARG, "null context");
    ctx->cdprofile_global = on ? 1 : 0;
    return XC_OK;
}

int xc_last_cdist_profile(xc_ctx* ctx, double* ms, int64_t* pairs_visited, int64_t* pairs_total, int* groups)
{
    if (!ctx) return xc::fail(nullptr, XC_EBADARG, "null context");
    const xc::CpProfile& p = ctx->prof_cdist;
    if (ms) { ms[0] = (double)p.ms[0] + (double)p.ms[1] + (double)p.ms[2]; ms[1] = (double)p.ms[3]; ms[2] = (double)p.ms[4]; }
    if (pairs_visited) *pairs_visited = (int64_t)ctx->cdist_pairs[0];
    if (pairs_total) *pairs_total = (int64_t)ctx->cdist_pairs[1];
    if (groups) *groups = p.groups;
    return XC_OK;
}

int xc_last_cdprofile_profile(xc_ctx* ctx, double* ms, int64_t* pairs_visited, int64_t* pairs_total, int64_t* tiles_window,
                              int64_t* tiles_global, int* groups)
{
    if (!ctx) return xc::fail(nullptr, XC_EBADARG, "null context");
    const xc::CpProfile& p = ctx->prof_cdprofile;
    if (ms) {
        ms[0] = (double)p.ms[0] + (double)p.ms[1] + (double)p.ms[2]; ms[1] = (double)p.ms[3]; ms[2] = (double)p.ms[4];
        ms[3] = (double)p.ms[5]; ms[4] = (double)p.ms[6];
    }
    if (pairs_visited) *pairs_visited = (int64_t)ctx->cdprofile_stat[0];
    if (pairs_total) *pairs_total = (int64_t)ctx->cdprofile_stat[1];
    if (tiles_window) *tiles_window = (int64_t)ctx->cdprofile_stat[2];
    if (tiles_global) *tiles_global = (int64_t)ctx->cdprofile_stat[3];
    if (groups) *groups = p.groups;
    return XC_OK;
}

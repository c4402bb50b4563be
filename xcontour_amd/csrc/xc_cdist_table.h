// K27 / K28, the segment table of a group (xc_cdist.hip runs them; included inside its anonymous namespace, after xc_cpiece_select.h and
// xc_cdist_metric.h): the selected segments of every range binned by coarse block and stored in metric space.
//   k_cd_count      one thread per segment of a selected piece: its coarse BLOCK is the CD_B x CD_B cells around the cell of e_from; one
//                   integer atomic add per segment
//   k_cd_scan       one workgroup per range: the exclusive scan of the block counts (where each block's segments start in the table),
//                   the cursors, and the list of the non-empty blocks
//   k_cd_fill       one thread per selected segment: its slot from the block's cursor, then the segment in metric space -- plane:
//                   (a, u, uu), sphere: (a, b, n, nn) as unit vectors --, its id and its piece's first_edge.  Order inside a block is
//                   whatever the atomics gave: nothing depends on it.
//   k_cd_box        one thread per non-empty block: the box that holds every foot the metric can compute on its segments
// Ranges outside every group have no segment: k_cd_none writes their planes.  Every index taken from a record is checked before any
// output is written (k_cd_check): a refusal writes nothing.  k_cd_trig: the sphere's node coordinates as unit vectors, once per call.
#pragma once

constexpr int CD_B = 32;                      // a coarse block is CD_B x CD_B cells
constexpr int CD_NBOX_PLANE = 4, CD_NBOX_SPHERE = 6;

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

// K16's selection as k_cd_count and k_cd_fill take it, by value: the operands of co_selected for the segments of the group at hand
struct CdSel {
    int select; const long long* __restrict__ e_from; const int* __restrict__ rid; const int* __restrict__ root; const int* __restrict__ prv;
    const int* __restrict__ lab; const unsigned* __restrict__ pn; const int* __restrict__ pw; const unsigned long long* __restrict__ key;
};

// whether segment i of the group is one of a selected piece (with a checked id)
__device__ __forceinline__ bool cd_takes(int64_t i, long long s0, int64_t r0, long long E, const CdSel& S)
{
    int w; bool ismain;
    const long long ef = S.e_from[s0 + i];
    return ef >= 0 && ef < E && co_selected(S.select, S.prv[i] >= 0, S.root[i], S.lab[i], S.pn, S.pw, S.key[r0 + S.rid[i]], w, ismain);
}

__global__ __launch_bounds__(CP_TPB)
void k_cd_count(int64_t n, long long s0, int64_t r0, long long E, int64_t nx, int64_t nbc, int64_t nb, const CdSel S, int* __restrict__ bcnt)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= n) return;
    if (!cd_takes(i, s0, r0, E, S)) return;
    atomicAdd(bcnt + (size_t)S.rid[i] * (size_t)nb + (size_t)cd_block_of(S.e_from[s0 + i], nx, nbc), 1);
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
               const CdSel S, const long long* __restrict__ off, const double* __restrict__ pts, const double* __restrict__ fy,
               const double* __restrict__ fx, int* __restrict__ bcnt, double* __restrict__ tseg, int* __restrict__ tid, int* __restrict__ tpiece)
{
    constexpr int ND = SPHERE ? CD_ND_SPHERE : CD_ND_PLANE;
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= n) return;
    if (!cd_takes(i, s0, r0, E, S)) return;
    const int r = S.rid[i];
    const long long ef = S.e_from[s0 + i];
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
    tpiece[at] = S.lab[i];
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

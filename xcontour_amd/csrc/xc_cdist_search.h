// K27 / K28, the tile pass over a group's segment table (xc_cdist_table.h; included inside xc_cdist.hip's anonymous namespace after it).
//   k_cd_dist       one workgroup per tile of CD_T x CD_T nodes per range, one node per lane (the search is the device function
//                   cd_search, which K28's k_cd_profile calls too).  The tile's own box; with pruning an upper
//                   bound W on every node's result from the far distance to the nearest block; then every non-empty block whose lower
//                   bound does not exceed W (or max_dist) is staged through LDS in chunks of CD_CHUNK segments and every lane takes the
//                   minimum; W shrinks to the tile's worst best-distance after every block.  The bounds are conservative
//                   (xc_cdist_metric.h says why), so a skipped block holds no segment that could win or tie: pruned and unpruned
//                   results are the same bits.
#pragma once

constexpr int CD_T = 16;                      // a tile of nodes is CD_T x CD_T: one node per lane of a CD_TPB workgroup
constexpr int CD_TPB = CD_T * CD_T;
constexpr int CD_CHUNK = 256;                 // segments of a block staged through LDS at a time

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

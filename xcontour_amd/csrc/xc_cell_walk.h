// The tile walk of the marching-squares kernels K10 (xc_clen.hip) and K12 (xc_cseg.hip), and its launch geometry.
// Included inside namespace xc { namespace { ... } } after xc_binning.h and xc_levels.h.
//
// Mapping (like K9 at stride 1): tiles of 32 cell rows x 252 cell columns, 4 waves of 63 cells; lanes along X; every lane loads ONE
// corner per row and takes its right neighbour from the next lane (DPP), carrying the previous row, so every tracer row is read from
// HBM once per tile.  grid (bps, nslab, level groups); a block walks the tiles blockIdx.x, + bps, ...  A NaN-free cell crosses exactly
// the levels with mn <= c < mx: the index range between the two lower bounds (LevelSearch::crossed of xc_levels.h).
//
// The seam rule (WRAP, periodic X): the plane gains one cell column, index nx-1 -- the seam cell --, whose left corners are node
// column nx-1 and whose right corners are node column 0.  Tiles cover nx cell columns, and the lane whose column is nx -- the right
// neighbour of the seam cell's lane, a cell lane or the wave's halo lane 63 -- loads node column 0, so the seam cell takes its right
// corners by the same DPP shift as every other cell.  WRAP is a compile-time variant: the plain kernels pay nothing for it.  nx >= 2;
// Y never wraps.  What a kernel adds to this is its own: K10 the seam cell's coordinate, K12 its edge ids and right column.
#pragma once

constexpr int WALK_RB = 32;                 // cell rows per tile
constexpr int WALK_TPB = 256;               // threads per block
constexpr int WALK_W = 252;                 // cell columns per tile: 4 waves x 63 cells

// Tiles of a plane and blocks per slab: the launch's share of ~2048 blocks, at least 8, enough that no block walks more than
// max_tiles tiles, and no more than tiles.  bps_rule: the XC_CLEN_BPS_* rule that set bps; a plane without cells: 0 tiles, bps 0, rule 0.
struct WalkGeometry { int64_t ntj, nti, ntile, bps; int bps_rule; };

inline WalkGeometry walk_geometry(int64_t ny, int64_t nx, bool wrap, int64_t nslab, int64_t max_tiles)
{
    WalkGeometry g{};
    const int64_t ncx = wrap ? nx : nx - 1, ncy = ny - 1;
    g.ntj = ncy > 0 ? (ncy + WALK_RB - 1) / WALK_RB : 0;
    g.nti = ncx > 0 ? (ncx + WALK_W - 1) / WALK_W : 0;
    g.ntile = g.ntj * g.nti;
    if (g.ntile > 0) {
        g.bps = 2048 / nslab; g.bps_rule = XC_CLEN_BPS_SHARE;
        if (g.bps < 8) { g.bps = 8; g.bps_rule = XC_CLEN_BPS_FLOOR; }
        const int64_t need = (g.ntile + max_tiles - 1) / max_tiles;
        if (g.bps < need) { g.bps = need; g.bps_rule = XC_CLEN_BPS_CAPACITY; }
        if (g.bps > g.ntile) { g.bps = g.ntile; g.bps_rule = XC_CLEN_BPS_NTILE; }
    }
    return g;
}

// One block's tiles of slab `qs`.  per_tile(i, c) runs once per tile on EVERY lane -- i: the lane's cell column, c: the node column it
// loads -- so it may shift across lanes; lanes without a cell still load and shift.  per_level(k, r, c, ul, ur, ll, lr) runs per
// (NaN-free cell (r, c), crossed level k of s_cx) on the lanes that have one: divergent, no cross-lane moves there.
template <typename TQ, bool WRAP, typename PerTile, typename PerLevel>
__device__ __forceinline__ void cell_walk(const TQ* __restrict__ qs, int64_t ny, int64_t nx, int64_t ntj, int64_t nti, int bps,
                                          const double* __restrict__ s_cx, int ng, const LevelSearch& ls,
                                          PerTile&& per_tile, PerLevel&& per_level)
{
    const int64_t ncx = WRAP ? nx : nx - 1, ncy = ny - 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t tile = blockIdx.x; tile < ntj * nti; tile += bps) {
        const int64_t tj = tile / nti, ti = tile - tj * nti;
        const int64_t i = ti * WALK_W + wave * 63 + lane;                                // this lane's cell column
        const int64_t j0 = tj * WALK_RB, j1 = (j0 + WALK_RB < ncy) ? j0 + WALK_RB : ncy;
        const bool cell = lane < 63 && i < ncx;
        int64_t c = i < nx - 1 ? i : nx - 1;                                             // corner column loaded by this lane
        if constexpr (WRAP) { if (i == nx) c = 0; }                                      // column nx is column 0
        per_tile(i, c);
        double ul = (double)qs[(size_t)j0 * nx + c];
        double ur = lane_shift_keep<DPP_WAVE_SHL1>(ul, ul);
        constexpr int B = 4;
        for (int64_t jb = j0; jb < j1; jb += B) {
            TQ v[B];
#pragma unroll
            for (int b = 0; b < B; ++b) {                                                // all loads of the batch in flight together
                const int64_t jj = (jb + b < j1) ? jb + b : j1 - 1;
                v[b] = qs[(size_t)(jj + 1) * nx + c];
            }
#pragma unroll
            for (int b = 0; b < B; ++b) {
                const int64_t r = jb + b;
                if (r >= j1) break;                                                      // wave-uniform
                const double ll = (double)v[b], lr = lane_shift_keep<DPP_WAVE_SHL1>(ll, ll);
                const bool hasnan = (ul != ul) | (ur != ur) | (ll != ll) | (lr != lr);
                if (cell && !hasnan) {
                    const double mn = fmin(fmin(ul, ur), fmin(ll, lr)), mx = fmax(fmax(ul, ur), fmax(ll, lr));
                    int klo, khi;
                    ls.crossed(s_cx, ng, mn, mx, klo, khi);
                    for (int k = klo; k < khi; ++k) per_level(k, r, c, ul, ur, ll, lr);
                }
                ul = ll; ur = lr;
            }
        }
    }
}

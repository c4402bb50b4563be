// K20 -- which ring HOLDS each node (gfx950): per range a dense int32 map [ny][nx] naming the innermost ring round every node, -1 for none,
// beside K19's records, from K12's segment records on the device.
//
// The rule (include/xcontour_hip.h, K20 section): with I_p K18's inside set of ring p, label[r][c] is the ring with (r, c) in I_p and the
// fewest inside nodes; open pieces are transparent.
//
// The mapping rests on K19's facts (xc_cpiece_tree.h) and one more.  Without flip row 0 lies outside every ring, with flip row ny - 1 does:
// a column is scanned from that row, down without flip and up with it, and the scan starts in state -1 (no ring).
//   CROSSING   of a ring x (not open) at V(e, c): x's inside lies below it iff (s == S_x) != (winding_x != 0 && flip) (K18's s and S).
//              Inside on the far side of the walker: it enters x and the state becomes x.  Inside on the near side: it leaves x and
//              the state becomes par[x] (K19's parent) -- a vertical edge carries at most one vertex of a level, so the node across
//              that edge lies in every ring round x and in no sibling of x: in par[x] and no deeper.  One register, no stack.
//   ROW CHUNKS a node's label is the state behind the nearest crossing of a ring behind it in its column, wherever the scan began.  So a
//              column is cut into chunks of rows (pl_geometry: at least PL_ROWS rows each, at most PL_CHUNKS chunks; ny alone decides).
//              With more than one chunk k_pl_carry first leaves, per (range, chunk, column), the state behind the chunk's last crossing
//              of a ring, or PL_NONE; a chunk then starts from the nearest carry behind it that is not PL_NONE, else from -1.
//
// Per group, after K19's stages and before k_cp_unscatter (the edge table, root[], slot[], the signs and par[] still stand):
//   k_pl_carry   one thread per (range of the group, chunk but the last, column): the carry of the chunk
//   k_pl_scan    one thread per (range of the group, chunk, column): at most PL_CHUNKS carries looked back at, then the chunk's rows: the
//                label of a node is stored, then the edge behind it is crossed
// Lanes of a wave take consecutive columns: the table reads tab[V(e, c)] sit 8 bytes apart and the label stores are contiguous.  root[],
// slot[], e_from, e_to and the staged records are read at crossings only.  Ranges of the call that no group holds (no segments) are set
// to -1 with a memset.  Every index taken from a record or a table is checked before it addresses anything; every loop ends within ny
// steps; no kernel waits for another block; no LDS, no scratch.
//
// This header holds what a scan knows of a crossing, the carry pass, K20's scan and the host steps that launch them; K21
// (xc_cpiece_props.h) runs the carry pass and pl_cross too.  The row chunks (pl_geometry) and the thread mapping (pl_thread) are in
// xc_cpiece_link.h.  Included inside namespace xc { namespace { ... } } after xc_cpiece_tree.h.
#pragma once

constexpr int PL_NONE = -2;                   // a carry: no ring crosses the column inside the chunk

// the state behind table entry j of range r (pieces [lo, hi)): the ring entered, the parent of the ring left (-1: none), or PL_NONE
// where no ring crosses.  States are rows of the range as packed: p - lo.
__device__ __forceinline__ int pl_cross(int j, int64_t r, long long lo, long long hi, const PlGroup& g, const PiStage& st, const PtStage& pt,
                                        int* __restrict__ err)
{
    if (j < 0 || j >= g.n) return PL_NONE;
    int t; bool open;
    const int64_t x = pi_piece_of(j, r, g.cap, g.root, g.slot, g.piece_count, g.poff, t, open, err);
    if (x < 0 || open) return PL_NONE;
    int64_t xrow, xcol; int s;
    if (!pi_crossing(g.e_from[g.s0 + j], g.e_to[g.s0 + j], g.E, g.ny, g.nx, xrow, xcol, s)) return PL_NONE;
    const int S = pt_sign(st, x);
    if (S == 0) return PL_NONE;
    const bool below = (s == S) != (st.wd[x] != 0 && g.flip);              // x's inside lies below this crossing
    const long long q = below != (g.flip != 0) ? (long long)x : pt.par[x];  // on the walker's far side: entered; else left for its parent
    return (q >= lo && q < hi) ? (int)(q - lo) : -1;
}

__global__ __launch_bounds__(CP_TPB)
void k_pl_carry(int64_t ng, int64_t rows, int64_t nchunk, PlGroup g, PiStage st, PtStage pt, int* __restrict__ carry, int* __restrict__ err)
{
    int64_t rl, k, c;
    if (!pl_thread(ng, nchunk, g.nx, rl, k, c) || k == nchunk - 1) return;  // nothing lies behind the last chunk
    const int64_t r = g.r0 + rl;
    const long long lo = g.poff[r], hi = g.poff[r + 1];
    const int* tp = g.tab + (size_t)rl * (size_t)g.E + 2 * (size_t)c + 1;   // tp[2 nx e] = tab[V(e, c)]
    int last = PL_NONE;
    // the chunk's nodes are steps [k rows, (k + 1) rows) of the scan; the edge behind the node of step t is edge t, t < ny - 1
    const int64_t t1 = (k + 1) * rows < g.ny - 1 ? (k + 1) * rows : g.ny - 1;
    for (int64_t t = k * rows; t < t1; ++t) {
        const int64_t e = g.flip ? g.ny - 2 - t : t;
        const int v = pl_cross(tp[2 * (size_t)g.nx * (size_t)e], r, lo, hi, g, st, pt, err);
        if (v != PL_NONE) last = v;
    }
    carry[(size_t)(rl * nchunk + k) * (size_t)g.nx + (size_t)c] = last;
}

__global__ __launch_bounds__(CP_TPB)
void k_pl_scan(int64_t ng, int64_t rows, int64_t nchunk, PlGroup g, PiStage st, PtStage pt, const int* __restrict__ carry,
               int* __restrict__ label, int* __restrict__ err)
{
    int64_t rl, k, c;
    if (!pl_thread(ng, nchunk, g.nx, rl, k, c)) return;
    const int64_t r = g.r0 + rl;
    const long long lo = g.poff[r], hi = g.poff[r + 1];
    const int* tp = g.tab + (size_t)rl * (size_t)g.E + 2 * (size_t)c + 1;
    int state = -1;
    for (int64_t kk = k - 1; kk >= 0; --kk) {                                // at most PL_CHUNKS - 1 steps
        const int v = carry[(size_t)(rl * nchunk + kk) * (size_t)g.nx + (size_t)c];
        if (v != PL_NONE) { state = v; break; }
    }
    int* out = label + (size_t)r * (size_t)g.ny * (size_t)g.nx + (size_t)c;
    const int64_t t1 = (k + 1) * rows < g.ny ? (k + 1) * rows : g.ny;
    for (int64_t t = k * rows; t < t1; ++t) {
        const int64_t at = g.flip ? g.ny - 1 - t : t;                        // 0 <= at < ny
        out[(size_t)at * (size_t)g.nx] = state;
        if (t == g.ny - 1) break;
        const int64_t e = g.flip ? at - 1 : at;                              // the edge to the next node: 0 <= e < ny - 1
        const int v = pl_cross(tp[2 * (size_t)g.nx * (size_t)e], r, lo, hi, g, st, pt, err);
        if (v != PL_NONE) state = v;
    }
}

// ---------------------------------------------------------------- the host steps of K20, each launched from one place (xc_cprecords.hip)
// the ranges [ra, rb) of the map hold no ring: -1 everywhere
inline hipError_t pl_blank(hipStream_t stream, int32_t* label, int64_t npl, int64_t ra, int64_t rb)
{
    if (!label || rb <= ra) return hipSuccess;
    return hipMemsetAsync(label + (size_t)ra * (size_t)npl, 0xff, (size_t)(rb - ra) * (size_t)npl * 4, stream);
}

// the carries of the ng ranges of a group, where a column has more than one chunk (K20 and K21); one thread per (range, chunk, column)
inline void pl_launch_carry(hipStream_t stream, int64_t ng, int64_t rows, int64_t nchunk, const PlGroup& g, const PiStage& st, const PtStage& pt,
                            int* carry, int* err)
{
    if (nchunk > 1) hipLaunchKernelGGL(k_pl_carry, dim3(cp_blocks(ng * nchunk * g.nx)), dim3(CP_TPB), 0, stream, ng, rows, nchunk, g, st, pt, carry, err);
}

// the map of the group's ranges
inline void pl_launch_scan(hipStream_t stream, int64_t ng, int64_t rows, int64_t nchunk, const PlGroup& g, const PiStage& st, const PtStage& pt,
                           const int* carry, int32_t* label, int* err)
{
    hipLaunchKernelGGL(k_pl_scan, dim3(cp_blocks(ng * nchunk * g.nx)), dim3(CP_TPB), 0, stream, ng, rows, nchunk, g, st, pt, carry, (int*)label, err);
}

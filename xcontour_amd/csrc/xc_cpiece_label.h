// K20's column scan, shared by K20 (xc_cplabel.hip) and K21 (xc_cpprops.hip); xc_cplabel.hip's header states the rule and the mapping: the
// row chunks of a column, what a scan needs of its group, the state behind a crossing, the thread mapping and the carry pass.
// Included inside namespace xc { namespace { ... } } after xc_cpiece_tree.h.
#pragma once

constexpr int PL_ROWS = 16;                   // a chunk of a column has at least this many rows ...
constexpr int PL_CHUNKS = 32;                 // ... and a column at most this many chunks
constexpr int PL_NONE = -2;                   // a carry: no ring crosses the column inside the chunk

// the chunks of a column: `rows` rows each (the last one what is left), `nchunk` of them
inline void pl_geometry(int64_t ny, int64_t* rows, int64_t* nchunk)
{
    int64_t R = (ny + PL_CHUNKS - 1) / PL_CHUNKS;
    if (R < PL_ROWS) R = PL_ROWS;
    *rows = R; *nchunk = (ny + R - 1) / R;
}

// what a scan needs of its group
struct PlGroup {
    int64_t n; long long s0; int64_t r0; long long E; int64_t ny, nx; int flip; int64_t cap;
    const long long* e_from; const long long* e_to; const int* tab; const int* root; const int* slot;
    const unsigned long long* piece_count; const long long* poff;
};

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

// thread -> (range of the group, chunk, column), columns fastest
__device__ __forceinline__ bool pl_thread(int64_t ng, int64_t nchunk, int64_t nx, int64_t& rl, int64_t& k, int64_t& c)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= ng * nchunk * nx) return false;
    const int64_t rk = i / nx;
    c = i - rk * nx; rl = rk / nchunk; k = rk - rl * nchunk;
    return true;
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

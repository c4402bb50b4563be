// K19 -- which piece of a contour is NESTED in which (gfx950): per ring its parent (the innermost ring that encloses it), its depth, the
// number of its children and what it bounds NET of them, beside K18's records, from K12's segment records on the device.
//
// The rule (include/xcontour_hip.h, K19 section): with I_p K18's inside set of ring p, a encloses b iff I_b is a subset of I_a; parent[b] is
// the enclosing ring with the fewest inside nodes; open pieces are transparent; the net records are those of I_p minus its children's sets.
//
// The mapping rests on K18's facts (xc_cpiece_interior.h) and two more.  Rings of one range do not meet, so two of them are nested or disjoint,
// and a ring other than b holds ALL of I_b as soon as it holds the one node that lies across b's boundary from a node of I_b.  And down a
// column a ring's crossings alternate, so a walker that enters a ring it started outside of is outside again behind that ring's next
// crossing: whatever it meets in between is nested in that ring and cannot hold the start node.
//   OUTSIDE NODE   without flip row 0 lies outside EVERY ring (P = 0 there): the node ABOVE a ring's topmost crossing (the smallest odd
//                  e_from among its crossings) is outside it, and between that node and row 0 the column never meets the ring again.
//                  With flip row 0 lies INSIDE every ring that goes round, and it is row ny - 1 that lies outside every ring (a ring of
//                  winding 0 has an even number of crossings above it, one that goes round an odd number): the node BELOW a ring's
//                  bottommost crossing is outside it.  A walk that ends on the row that is outside everything has missed no ring.
//   PARENT WALK    from that node away from the ring, to row 0 (with flip: to row ny - 1).  A crossing of another ring x has x's inside BELOW it iff
//                  (s == S_x) != (winding_x != 0 && flip) (K18's s and S).  Inside on the walker's side: the walker is inside x, and x is
//                  the innermost such ring -- parent = x.  Inside on the far side: the walker enters x from outside and skips everything up
//                  to x's next crossing in this column.  Crossings of open pieces are ignored.  One `skip` register; at most ny steps.
//
// Per group, between K18's walks and k_cp_unscatter (the edge table, root[] and slot[] still stand):
//   k_pt_init    the staged tree records of the group's pieces are cleared
//   k_pt_top     one thread per segment: one 64-bit integer atomicMin of its crossing's key onto its ring (e_from, or ~e_from with
//                flip, when the walks go down, so that one minimum serves both)
//   k_pt_parent  one thread per ring: the parent walk; one integer atomic counts the child at its parent
//   k_pt_depth   one thread per ring chases its parents, at most the range's piece count of them; a chase that does not end there sets
//                PT_ERR_TREE in the err word (XC_EBADARG after the call)
//   k_pt_net     every ring with a parent adds its NEGATED n_in and limbs to the parent's net words, with 64-bit integer atomics.  K18's
//                limbs are signed sums of 32-bit chunks in two's-complement 64-bit words, so negation is exact, and the words of
//                (gross - children) are the words the net nodes alone would have given: cp_to_double rounds the exact net sum once.
// k_pt_finish adds the gross and the net words and writes the records, after k_pi_finish has written K18's.  Every index taken from a
// record or a table is checked before it addresses anything; no kernel waits for another block; no LDS, no scratch.
//
// This header holds the staged tree records of a call's pieces, the top crossings, the parent walks, the depths, the net words, the
// finish pass and the host step that launches the stages of a group.  Included inside namespace xc { namespace { ... } } after
// xc_cpiece_interior.h.
#pragma once

constexpr int PT_ERR_TREE = 4;                // beside CP_ERR_EDGE and CP_ERR_LINK: a chase of parents that does not end
constexpr unsigned long long PT_NONE = ~0ull;

// the staged tree records (behind K18's in ctx->cpiece_acc), `cap` of each
struct PtStage {
    unsigned long long* net;      // [cap][2 CP_L] minus the limbs of the children's sum_w, sum_wf
    unsigned long long* key;      // the crossing next to the ring's outside node: e_from, or ~e_from with flip (the parent walks go down)
    unsigned long long* nnet;     // minus the children's inside nodes
    long long* par;               // the parent's index in the table, -1
    int* nch;                     // children
    int* dep;                     // depth
};

// the staged tree records of `cap` pieces, taken from the launcher's carve (xc_carve.h)
inline void pt_carve(Carve& c, int64_t cap, PtStage& pt)
{
    const size_t n = (size_t)cap;
    pt.net = c.take<unsigned long long>(n * 2 * CP_L);
    pt.key = c.take<unsigned long long>(n); pt.nnet = c.take<unsigned long long>(n); pt.par = c.take<long long>(n);
    pt.nch = c.take<int>(n); pt.dep = c.take<int>(n);
}

__global__ __launch_bounds__(CP_TPB)
void k_pt_init(int64_t p0, int64_t p1, PtStage pt)
{
    const int64_t p = p0 + (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (p >= p1) return;
#pragma unroll
    for (int j = 0; j < 2 * CP_L; ++j) pt.net[(size_t)p * 2 * CP_L + j] = 0ull;
    pt.key[p] = PT_NONE; pt.nnet[p] = 0ull; pt.par[p] = -1ll; pt.nch[p] = 0; pt.dep[p] = 0;
}

// K18's sign of a ring: a crossing with s == S has the side of parity 1 below it (0: a ring without crossings, no K12 output)
__device__ __forceinline__ int pt_sign(const PiStage& st, int64_t p)
{
    const long long a = (long long)st.sa[p], b = (long long)st.sb[p];
    return st.wd[p] != 0 ? (int)(a > 0) - (int)(a < 0) : (int)(b < 0) - (int)(b > 0);
}

__global__ __launch_bounds__(CP_TPB)
void k_pt_top(int64_t n, long long s0, int64_t r0, long long E, int64_t ny, int64_t nx, int flip, int64_t cap,
              const long long* __restrict__ e_from, const long long* __restrict__ e_to, const int* __restrict__ rid,
              const int* __restrict__ root, const int* __restrict__ slot, const unsigned long long* __restrict__ piece_count,
              const long long* __restrict__ poff, PiStage st, PtStage pt, int* __restrict__ err)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= n) return;
    const long long ef = e_from[s0 + i];
    int64_t row, col; int s;
    if (!pi_crossing(ef, e_to[s0 + i], E, ny, nx, row, col, s)) return;
    int t; bool open;
    const int64_t p = pi_piece_of(i, r0 + rid[i], cap, root, slot, piece_count, poff, t, open, err);
    if (p < 0 || open) return;
    atomicMin(pt.key + p, flip ? ~(unsigned long long)ef : (unsigned long long)ef);
}

__global__ __launch_bounds__(CP_TPB)
void k_pt_parent(int64_t p0, int64_t p1, int64_t n, long long s0, int64_t r0, int64_t r1, long long E, int64_t ny, int64_t nx, int flip,
                 int64_t cap, const long long* __restrict__ e_from, const long long* __restrict__ e_to, const int* __restrict__ tab,
                 const int* __restrict__ root, const int* __restrict__ slot, const unsigned long long* __restrict__ piece_count,
                 const long long* __restrict__ poff, PiStage st, PtStage pt, int* __restrict__ err)
{
    const int64_t p = p0 + (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (p >= p1 || !st.cl[p]) return;
    const unsigned long long key = pt.key[p];
    if (key == PT_NONE) return;
    const bool down = flip != 0;
    const long long ef = (long long)(down ? ~key : key);
    if (!(ef & 1) || ef < 0 || ef >= E) return;
    const int64_t row = (ef >> 1) / nx, col = (ef >> 1) - row * nx;
    if (row >= ny - 1) return;
    const int64_t r = cp_range_of(poff, r0, r1, p);                       // poff[r0 .. r1] stand for the group
    const int* tp = tab + (size_t)(r - r0) * (size_t)E + 2 * (size_t)col + 1;   // tp[2 nx r'] = tab[V(r', col)]
    const int j0 = tp[2 * (size_t)nx * (size_t)row];
    const int me = (j0 >= 0 && j0 < n) ? root[j0] : -1;
    int skip = -1;
    int64_t parent = -1;
    // the edges of the walk are rows [0, row - 1] (up) or [row + 1, ny - 2] (down): never more than ny steps
    const int64_t dir = down ? 1 : -1;
    for (int64_t e = row + dir; e >= 0 && e < ny - 1; e += dir) {
        const int j = tp[2 * (size_t)nx * (size_t)e];
        if (j < 0 || j >= n) continue;
        const int tj = root[j];
        if (skip >= 0) { if (tj == skip) skip = -1; continue; }
        if (tj == me) break;                                              // (records that are no K12 output)
        int t; bool open;
        const int64_t x = pi_piece_of(j, r, cap, root, slot, piece_count, poff, t, open, err);
        if (x < 0 || open) continue;
        int64_t xrow, xcol; int s;
        if (!pi_crossing(e_from[s0 + j], e_to[s0 + j], E, ny, nx, xrow, xcol, s)) continue;
        const int S = pt_sign(st, x);
        if (S == 0) continue;
        const bool below = (s == S) != (st.wd[x] != 0 && flip);            // x's inside lies below this crossing
        if (below != down) { parent = x; break; }                         // ... on the walker's side: the innermost ring round it
        skip = tj;                                                         // entered from outside: up to x's next crossing
    }
    if (parent < 0) return;
    pt.par[p] = parent;
    atomicAdd(pt.nch + parent, 1);
}

__global__ __launch_bounds__(CP_TPB)
void k_pt_depth(int64_t p0, int64_t p1, int64_t r0, int64_t r1, const long long* __restrict__ poff, PiStage st, PtStage pt,
                int* __restrict__ err)
{
    const int64_t p = p0 + (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (p >= p1 || !st.cl[p]) return;
    const int64_t r = cp_range_of(poff, r0, r1, p);
    const long long lo = poff[r], hi = poff[r + 1];                        // a parent is a piece of the same range
    int d = 0;
    for (long long q = pt.par[p]; q >= 0; q = pt.par[q]) {
        if (q < lo || q >= hi || q >= p1 || d >= hi - lo) { *err = PT_ERR_TREE; d = 0; break; }
        ++d;
    }
    pt.dep[p] = d;
}

__global__ __launch_bounds__(CP_TPB)
void k_pt_net(int64_t p0, int64_t p1, PiStage st, PtStage pt)
{
    const int64_t p = p0 + (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (p >= p1 || !st.cl[p]) return;
    const long long q = pt.par[p];
    if (q < p0 || q >= p1) return;
    atomicAdd(pt.nnet + q, 0ull - st.cnt[p]);
    const unsigned long long* a = st.acc + (size_t)p * 2 * CP_L;
    unsigned long long* d = pt.net + (size_t)q * 2 * CP_L;
#pragma unroll
    for (int l = 0; l < 2 * CP_L; ++l) if (a[l]) atomicAdd(d + l, 0ull - a[l]);
}

__global__ __launch_bounds__(CP_TPB)
void k_pt_finish(int64_t np, int64_t nrange, int ncont, const long long* __restrict__ poff, PiStage st, PtStage pt,
                 const unsigned long long* __restrict__ mx, long long* __restrict__ parent, int* __restrict__ depth,
                 int* __restrict__ nchild, long long* __restrict__ n_net, double* __restrict__ net_w, double* __restrict__ net_wf)
{
    const int64_t p = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (p >= np) return;
    const int64_t s = cp_range_of(poff, 0, nrange, p) / ncont;
    const int cl = st.cl[p], fl = st.flg[p];
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    parent[p] = cl ? pt.par[p] : -1ll; depth[p] = cl ? pt.dep[p] : 0; nchild[p] = cl ? pt.nch[p] : 0;
    n_net[p] = cl ? (long long)(st.cnt[p] + pt.nnet[p]) : -1ll;
    unsigned long long a[2 * CP_L];
#pragma unroll
    for (int l = 0; l < 2 * CP_L; ++l) a[l] = st.acc[(size_t)p * 2 * CP_L + l] + pt.net[(size_t)p * 2 * CP_L + l];
    net_w[p] = (!cl || (fl & 1)) ? qnan : cp_to_double(a, ci_top(mx[2 * s]));
    if (net_wf) net_wf[p] = (!cl || (fl & 2)) ? qnan : cp_to_double(a + CP_L, ci_top(mx[2 * s + 1]));
}

// ---------------------------------------------------------------- the host step of K19, launched from one place (xc_cprecords.hip)
// the tree stages of a group (ranges [g.r0, r1), pieces [p0, p1)), behind K18's walks
inline void pt_launch_group(hipStream_t stream, const PlGroup& g, int64_t r1, int64_t p0, int64_t p1, const int* rid, const PiStage& st,
                            const PtStage& pt, int* err)
{
    const dim3 grid(cp_blocks(g.n)), pgrid(cp_blocks(p1 - p0)), blk(CP_TPB);
    hipLaunchKernelGGL(k_pt_init, pgrid, blk, 0, stream, p0, p1, pt);
    hipLaunchKernelGGL(k_pt_top, grid, blk, 0, stream, g.n, g.s0, g.r0, g.E, g.ny, g.nx, g.flip, g.cap, g.e_from, g.e_to, rid, g.root, g.slot,
                       g.piece_count, g.poff, st, pt, err);
    hipLaunchKernelGGL(k_pt_parent, pgrid, blk, 0, stream, p0, p1, g.n, g.s0, g.r0, r1, g.E, g.ny, g.nx, g.flip, g.cap, g.e_from, g.e_to, g.tab,
                       g.root, g.slot, g.piece_count, g.poff, st, pt, err);
    hipLaunchKernelGGL(k_pt_depth, pgrid, blk, 0, stream, p0, p1, g.r0, r1, g.poff, st, pt, err);
    hipLaunchKernelGGL(k_pt_net, pgrid, blk, 0, stream, p0, p1, st, pt);
}

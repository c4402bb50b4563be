// K18 -- what lies INSIDE EVERY PIECE of a contour (gfx950): per ring the nodes it encloses and the sums of w and w f over them, from K12's
// segment records on the device.  K17 (xc_cinside.hip) answers for one selection per range and scans the whole plane for it; this answers
// for every piece of every range in one call, at a cost proportional to the nodes the rings enclose.
//
// The rule (include/xcontour_hip.h, K18 section) is K17's with the selection being one piece p:
//   X_p[r][c] = 1 iff V(r, c) carries a meridian crossing of a segment of p;  P_p[r][c] = XOR over r' < r of X_p[r'][c];
//   ring of winding 0: inside = P_p;  ring of winding != 0: inside = P_p ^ flip;  open piece: n_in = -1, both sums NaN.
// Pieces, closed, winding, nseg, first_edge and the slots are K13's; the sums are K17's (xc_cpiece_sum.h, the tops of xc_cinside_bound.h).
//
// The mapping rests on two facts about a ring of K12's records: it is a simple closed curve, so down one column its crossings alternate
// between entering and leaving; and the ids alone say which of the two a crossing is, up to one sign per ring:
//   a segment with e_from = V(r, c) lies in cell (r, c) when its e_to is H(r, c), H(r+1, c) or V(r, (c+1) % nx), else in cell (r, c-1)
//   (the seam cell for c = 0 of a periodic plane).  By K12's direction table (xc_cseg_cell.h) a segment that starts on a cell's left edge
//   has the node BELOW the crossing above the level, one that starts on a cell's right edge the node ABOVE it: s = +1 / -1.
//   The ring's sign S, from two integer sums over its crossings: winding 0 -- the crossings pair up into (entering at row a, leaving at
//   row b > a) with opposite s, so B = sum of s x row is -(the nodes enclosed) when the entering ones have s = +1 and +(...) otherwise:
//   S = +1 for B < 0, -1 for B > 0.  Winding != 0 -- every column has one crossing more with the parity-1 side below it than above it, so
//   A = sum of s is +-nx: S = the sign of A.  A crossing with s == S has the side of parity 1 below it.
// nx == 2 on a periodic plane makes V(r, c+1) and V(r, c-1) the same edge: nx < 3 with periodic is refused.
//
// Per GROUP of consecutive ranges (xc_cpiece_link.h: K13's groups under K13's cap, indices group-local):
//   phase A (K13's kernels), k_cp_root (K13's roots and slots, xc_cpiece_slot.h)
//   the host reads the group's piece counts (they place the group's pieces in the table; once the pieces no longer fit `capacity` the
//   rest of the call only counts)
//   k_pi_init       the staged records of the group's pieces are cleared
//   k_pi_piece      one thread per segment, integer atomics onto its piece: nseg, the winding by K13's seam count, A and B; the root
//                   writes first_edge and closed
//   k_pi_walk       one thread per segment with odd e_from of a ring and s == S.  Winding 0, or winding != 0 without flip: it walks DOWN
//                   its column from row r + 1, reading the group's edge table -- tab[V(r', c)] is the segment that starts there, root[] of
//                   it its piece -- and stops behind the next crossing of its own piece, or at row ny - 1.  Winding != 0 with flip: it
//                   walks UP from row r and stops before the previous crossing of its own piece, or at row 0.  n_in and the limbs of both
//                   sums stay in registers; one set of 64-bit integer atomics onto the piece's slot closes the walk.  At most ny steps.
//   k_cp_unscatter  the table is handed on clean
// Around the groups: k_ci_bound (K17's maxima behind the windows) and k_pi_finish (the limbs rounded to double, the records written to
// the caller's arrays -- only when all pieces fit).  The edge-table reads of a walk run along a column: one 4-byte read per step from a
// line of its own (DESIGN.md says what that costs).  Every index taken from a record or a table is checked before it addresses
// anything; no kernel waits for another block.
//
// This header holds the staged records of a call's pieces, the per-segment pass that gives every ring its sign, the column walks, the
// finish pass and the host steps that launch them; xc_cprecords.hip is the launcher of K18-K21.  Included inside
// namespace xc { namespace { ... } } after xc_cpiece_link.h, xc_cpiece_slot.h, xc_cpiece_sum.h and xc_cinside_bound.h.
#pragma once

// the staged per-piece records (ctx->cpiece_acc), `cap` of each
struct PiStage {
    unsigned long long* acc;      // [cap][2 CP_L] the limbs of sum_w, sum_wf
    unsigned long long* cnt;      // inside nodes
    unsigned long long* sa;       // A = sum of s over the crossings (two's complement)
    unsigned long long* sb;       // B = sum of s x row
    unsigned long long* ns;       // nseg
    long long* fe;                // first_edge
    int* wd;                      // winding (seam count)
    int* cl;                      // closed
    int* flg;                     // 1: sum_w is NaN, 2: sum_wf is NaN
};

// the staged records of `cap` pieces, taken from the launcher's carve (xc_carve.h)
inline void pi_carve(Carve& c, int64_t cap, PiStage& st)
{
    const size_t n = (size_t)cap;
    st.acc = c.take<unsigned long long>(n * 2 * CP_L);
    st.cnt = c.take<unsigned long long>(n); st.sa = c.take<unsigned long long>(n); st.sb = c.take<unsigned long long>(n);
    st.ns = c.take<unsigned long long>(n); st.fe = c.take<long long>(n);
    st.wd = c.take<int>(n); st.cl = c.take<int>(n); st.flg = c.take<int>(n);
}

// what the stages of a group need of it: n segments from s0 on, ranges from r0 on, the edge table, the roots and the slots (K20's and
// K21's scans take it whole)
struct PlGroup {
    int64_t n; long long s0; int64_t r0; long long E; int64_t ny, nx; int flip; int64_t cap;
    const long long* e_from; const long long* e_to; const int* tab; const int* root; const int* slot;
    const unsigned long long* piece_count; const long long* poff;
};

__global__ __launch_bounds__(CP_TPB)
void k_pi_init(int64_t p0, int64_t p1, PiStage st)
{
    const int64_t p = p0 + (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (p >= p1) return;
#pragma unroll
    for (int j = 0; j < 2 * CP_L; ++j) st.acc[(size_t)p * 2 * CP_L + j] = 0ull;
    st.cnt[p] = 0ull; st.sa[p] = 0ull; st.sb[p] = 0ull; st.ns[p] = 0ull;
    st.fe[p] = -1ll; st.wd[p] = 0; st.cl[p] = 0; st.flg[p] = 0;
}

// the piece of segment i of a group: its index in the table, or -1 (records that are no K12 output: never past the table)
__device__ __forceinline__ int64_t pi_piece_of(int64_t i, int64_t r, int64_t cap, const int* __restrict__ root, const int* __restrict__ slot,
                                               const unsigned long long* __restrict__ piece_count, const long long* __restrict__ poff,
                                               int& t, bool& open, int* __restrict__ err)
{
    t = root[i];                                                          // (k_cp_root left 0 <= t < n)
    const int ps = slot[t];
    open = ps < 0;
    const unsigned long long sl = (unsigned)(ps & 0x7fffffff);
    if (sl >= piece_count[r]) { *err = CP_ERR_LINK; return -1; }
    const int64_t p = poff[r] + (int64_t)sl;
    return p < cap ? p : -1;
}

// the crossing a segment starts with: e_from = V(row, col) with row < ny - 1 (a vertical edge of row ny - 1 bounds no node); s = +1 when
// the segment lies in cell (row, col), -1 when in the cell to the left
__device__ __forceinline__ bool pi_crossing(long long ef, long long et, long long E, int64_t ny, int64_t nx, int64_t& row, int64_t& col, int& s)
{
    if (!(ef & 1) || ef < 0 || ef >= E) return false;
    const long long node = ef >> 1;
    row = node / nx; col = node - row * nx;
    if (row >= ny - 1) return false;
    const long long right = 2 * (row * nx + (col + 1 == nx ? 0 : col + 1)) + 1;
    s = (et == 2 * node || et == 2 * (node + nx) || et == right) ? 1 : -1;
    return true;
}

__global__ __launch_bounds__(CP_TPB)
void k_pi_piece(int64_t n, long long s0, int64_t r0, long long E, int64_t ny, int64_t nx, int wrap, int64_t cap,
                const long long* __restrict__ e_from, const long long* __restrict__ e_to, const double* __restrict__ pts,
                const int* __restrict__ rid, const int* __restrict__ root, const int* __restrict__ slot,
                const unsigned long long* __restrict__ piece_count, const long long* __restrict__ poff, PiStage st, int* __restrict__ err)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= n) return;
    int t; bool open;
    const int64_t p = pi_piece_of(i, r0 + rid[i], cap, root, slot, piece_count, poff, t, open, err);
    if (p < 0) return;
    const long long ef = e_from[s0 + i];
    atomicAdd(st.ns + p, 1ull);
    if (t == (int)i) { st.fe[p] = ef; st.cl[p] = open ? 0 : 1; }
    if (open) return;
    if (wrap) {
        const double xn = (double)nx;
        const double c1 = pts[4 * (size_t)(s0 + i) + 1], c2 = pts[4 * (size_t)(s0 + i) + 3];
        const int w = (int)(c2 == xn) - (int)(c1 == xn);
        if (w != 0) atomicAdd(st.wd + p, w);
    }
    int64_t row, col; int s;
    if (!pi_crossing(ef, e_to[s0 + i], E, ny, nx, row, col, s)) return;
    atomicAdd(st.sa + p, (unsigned long long)(long long)s);
    if (row) atomicAdd(st.sb + p, (unsigned long long)((long long)s * (long long)row));
}

template <typename FT>
__global__ __launch_bounds__(CP_TPB)
void k_pi_walk(int64_t n, long long s0, int64_t r0, long long E, int64_t ny, int64_t nx, int flip, int ncont, int64_t cap,
               const long long* __restrict__ e_from, const long long* __restrict__ e_to, const int* __restrict__ tab,
               const int* __restrict__ rid, const int* __restrict__ root, const int* __restrict__ slot,
               const unsigned long long* __restrict__ piece_count, const long long* __restrict__ poff,
               const double* __restrict__ w, int w_per_slab, const FT* __restrict__ f, const unsigned long long* __restrict__ mx,
               PiStage st, int* __restrict__ err)
{
    constexpr bool HASF = !std::is_void<FT>::value;
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= n) return;
    const int rl = rid[i];
    const int64_t r = r0 + rl;
    int64_t row, col; int s;
    if (!pi_crossing(e_from[s0 + i], e_to[s0 + i], E, ny, nx, row, col, s)) return;
    int t; bool open;
    const int64_t p = pi_piece_of(i, r, cap, root, slot, piece_count, poff, t, open, err);
    if (p < 0 || open) return;
    const int wd = st.wd[p];
    const long long a = (long long)st.sa[p], b = (long long)st.sb[p];
    const int S = wd != 0 ? (int)(a > 0) - (int)(a < 0) : (int)(b < 0) - (int)(b > 0);
    if (S == 0 || s != S) return;
    const bool up = wd != 0 && flip;

    const int64_t sl = r / ncont;
    const size_t npl = (size_t)ny * (size_t)nx;
    const double* wp = w ? w + (w_per_slab ? (size_t)sl * npl : 0) + (size_t)col : nullptr;
    const int top_w = ci_top(mx[2 * sl]);
    int top_f = 0;
    if constexpr (HASF) top_f = ci_top(mx[2 * sl + 1]);
    const int* tp = tab + (size_t)rl * (size_t)E + 2 * (size_t)col + 1;   // tp[2 nx r'] = tab[V(r', col)]
    unsigned long long nin = 0ull, aw[CP_L], af[CP_L];
#pragma unroll
    for (int l = 0; l < CP_L; ++l) { aw[l] = 0ull; af[l] = 0ull; }
    int bad = 0;
    // the nodes of the walk are rows [row + 1, ny - 1] at most (down) or [0, row] at most (up), row < ny - 1: never more than ny steps
    int64_t at = up ? row : row + 1;
    for (int64_t step = 0; step < ny; ++step) {
        const size_t node = (size_t)at * (size_t)nx;
        ++nin;
        const double v = wp ? wp[node] : 1.0;
        if (v == v && !cp_add_private(aw, v, top_w)) bad |= 1;
        if constexpr (HASF) {
            const double tv = __dmul_rn(v, (double)f[(size_t)sl * npl + node + (size_t)col]);
            if (tv == tv && !cp_add_private(af, tv, top_f)) bad |= 2;
        }
        if (up ? at == 0 : at == ny - 1) break;
        const int64_t edge = up ? at - 1 : at;                            // the vertical edge between this node and the next one: 0 <= edge < ny - 1
        const int j = tp[2 * (size_t)nx * (size_t)edge];
        if (j >= 0 && j < n && root[j] == t) break;                       // the next crossing of the same piece
        at += up ? -1 : 1;
    }
    atomicAdd(st.cnt + p, nin);
    unsigned long long* pa = st.acc + (size_t)p * 2 * CP_L;
#pragma unroll
    for (int l = 0; l < CP_L; ++l) if (aw[l]) atomicAdd(pa + l, aw[l]);
    if constexpr (HASF) {
#pragma unroll
        for (int l = 0; l < CP_L; ++l) if (af[l]) atomicAdd(pa + CP_L + l, af[l]);
    }
    if (bad) atomicOr(st.flg + p, bad);
}

__global__ __launch_bounds__(CP_TPB)
void k_pi_finish(int64_t np, int64_t nrange, int ncont, const long long* __restrict__ poff, PiStage st,
                 const unsigned long long* __restrict__ mx, long long* __restrict__ first_edge, long long* __restrict__ nseg,
                 int* __restrict__ closed, int* __restrict__ winding, long long* __restrict__ n_in, double* __restrict__ sum_w,
                 double* __restrict__ sum_wf)
{
    const int64_t p = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (p >= np) return;
    const int64_t s = cp_range_of(poff, 0, nrange, p) / ncont;
    const int cl = st.cl[p], fl = st.flg[p];
    const double qnan = __longlong_as_double(0x7ff8000000000000ll);
    first_edge[p] = st.fe[p]; nseg[p] = (long long)st.ns[p]; closed[p] = cl; winding[p] = cl ? st.wd[p] : 0;
    n_in[p] = cl ? (long long)st.cnt[p] : -1ll;
    sum_w[p] = (!cl || (fl & 1)) ? qnan : cp_to_double(st.acc + (size_t)p * 2 * CP_L, ci_top(mx[2 * s]));
    if (sum_wf) sum_wf[p] = (!cl || (fl & 2)) ? qnan : cp_to_double(st.acc + (size_t)p * 2 * CP_L + CP_L, ci_top(mx[2 * s + 1]));
}

// ---------------------------------------------------------------- the host steps of K18, each launched from one place (xc_cprecords.hip)
// the staged records of the group's pieces [p0, p1) cleared, then the per-segment pass
inline void pi_launch_piece(hipStream_t stream, const PlGroup& g, int64_t p0, int64_t p1, int wrap, const double* pts, const int* rid,
                            const PiStage& st, int* err)
{
    hipLaunchKernelGGL(k_pi_init, dim3(cp_blocks(p1 - p0)), dim3(CP_TPB), 0, stream, p0, p1, st);
    hipLaunchKernelGGL(k_pi_piece, dim3(cp_blocks(g.n)), dim3(CP_TPB), 0, stream, g.n, g.s0, g.r0, g.E, g.ny, g.nx, wrap, g.cap, g.e_from, g.e_to,
                       pts, rid, g.root, g.slot, g.piece_count, g.poff, st, err);
}

// the column walks for an integrand of f_dtype (f null: none)
inline void pi_launch_walk(hipStream_t stream, const PlGroup& g, int ncont, const int* rid, const double* w, int w_per_slab, const void* f,
                           int f_dtype, const unsigned long long* mx, const PiStage& st, int* err)
{
#define XC_PI_WALK(FT_) hipLaunchKernelGGL((k_pi_walk<FT_>), dim3(cp_blocks(g.n)), dim3(CP_TPB), 0, stream, g.n, g.s0, g.r0, g.E, g.ny, g.nx, g.flip, \
                                           ncont, g.cap, g.e_from, g.e_to, g.tab, rid, g.root, g.slot, g.piece_count, g.poff, w, w_per_slab,       \
                                           (const FT_*)f, mx, st, err)
    if (!f) XC_PI_WALK(void); else if (f_dtype == XC_F32) XC_PI_WALK(float); else XC_PI_WALK(double);
#undef XC_PI_WALK
}

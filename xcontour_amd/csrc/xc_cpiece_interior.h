// K18's per-piece interiors, shared by K18 (xc_cpinside.hip) and K19 (xc_cptree.hip); xc_cpinside.hip's header states the rule: the staged
// records of a call's pieces, the per-segment pass that gives every ring its sign, the column walks and the finish pass.  Included
// inside namespace xc { namespace { ... } } after xc_cpiece_link.h, xc_cpiece_slot.h, xc_cpiece_sum.h and xc_cinside_bound.h.
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

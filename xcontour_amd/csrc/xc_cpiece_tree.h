// K19's tree of pieces, shared by K19 (xc_cptree.hip) and K20 (xc_cplabel.hip); xc_cptree.hip's header states the rule and the mapping:
// the staged tree records of a call's pieces, the top crossings, the parent walks, the depths, the net words and the finish pass.
// Included inside namespace xc { namespace { ... } } after xc_cpiece_interior.h.
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

// The per-piece phase behind a SELECTION of pieces, shared by K16 (xc_coverturn.hip), K17 (xc_cinside.hip) and K24 (xc_cfold.hip), with
// the refusals the three entries have in common (co_check_select, co_check_plane): after phase A
// (xc_cpiece_link.h) has left label = the piece's smallest e_from and prev >= 0 on the members of a ring,
//   k_co_root   root(i) = tab[range][label], the segment that carries its piece's sums; the sums start at 0
//   k_co_piece  onto the root, integer atomic adds: nseg, and on a periodic plane the winding by K13's seam count (+1 where
//               c2 == nx, -1 where c1 == nx: on a ring every jump across the seam is one of each kind)
//   k_co_pick   roots only: a root counts into nsel[range] when its piece is selected ('all': every piece; 'circumpolar': a ring of
//               winding != 0; one atomic per wave where the wave lies in one range), and a ring of winding != 0 bids for the range's
//               main ring with ONE 64-bit atomic max on co_key: most segments first, then the smallest first_edge.  first_edge is
//               unique within a range, so the winning key names one piece.
//   co_selected whether a segment's piece is selected (0 all, 1 circumpolar, 2 main: the piece whose key won), once the keys stand
// Included inside namespace xc { namespace { ... } } after xc_cpiece_link.h.
#pragma once

constexpr unsigned long long CO_FE = 0x7fffffffull;          // the low 31 bits of a key: 2^31 - 1 - first_edge

// The refusals of the entry `who` that every selected-piece entry has, each called where the entry's own checks stand: `select` ...
inline int co_check_select(xc_ctx* ctx, const char* who, int periodic, int select)
{
    if (select < 0 || select > 2) return fail(ctx, XC_EBADARG, std::string(who) + ": select is 0 (all), 1 (circumpolar) or 2 (main)");
    if (select != 0 && !periodic)
        return fail(ctx, XC_EBADARG, std::string(who) + ": select != 0 needs periodic != 0 (no piece goes round a plain plane)");
    return XC_OK;
}
// ... and the plane (nx >= 1)
inline int co_check_plane(xc_ctx* ctx, const char* who, int periodic, int64_t ny, int64_t nx)
{
    if (periodic && nx < 2) return fail(ctx, XC_EBADARG, std::string(who) + ": a periodic plane needs nx >= 2");
    if (ny > ((int64_t)1 << 30) / nx) return fail(ctx, XC_EBADARG, std::string(who) + ": plane too large for 32-bit labels (2 ny nx < 2^31)");
    return XC_OK;
}

__global__ __launch_bounds__(CP_TPB)
void k_co_root(int64_t n, long long E, const int* __restrict__ tab, const int* __restrict__ rid, const int* __restrict__ lab,
               int* __restrict__ root, unsigned* __restrict__ pn, int* __restrict__ pw)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= n) return;
    const int l = lab[i];
    int t = (l >= 0 && l < E) ? tab[(size_t)rid[i] * E + l] : (int)i;
    if (t < 0 || t >= n) t = (int)i;
    root[i] = t;
    pn[i] = 0u; pw[i] = 0;
}

__global__ __launch_bounds__(CP_TPB)
void k_co_piece(int64_t n, long long s0, int wrap, int64_t nx, const double* __restrict__ pts, const int* __restrict__ root,
                unsigned* __restrict__ pn, int* __restrict__ pw)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    if (i >= n) return;
    const int t = root[i];
    atomicAdd(pn + t, 1u);
    if (wrap) {
        const double xn = (double)nx;
        const double c1 = pts[4 * (size_t)(s0 + i) + 1], c2 = pts[4 * (size_t)(s0 + i) + 3];
        const int w = (int)(c2 == xn) - (int)(c1 == xn);
        if (w != 0) atomicAdd(pw + t, w);
    }
}

// the key a ring of winding != 0 bids with
__device__ __forceinline__ unsigned long long co_key(unsigned nseg, int first_edge)
{
    return ((unsigned long long)nseg << 31) | (CO_FE - ((unsigned long long)(unsigned)first_edge & CO_FE));
}

__global__ __launch_bounds__(CP_TPB)
void k_co_pick(int64_t n, int64_t r0, int select, const int* __restrict__ rid, const int* __restrict__ root, const int* __restrict__ prv,
               const int* __restrict__ lab, const unsigned* __restrict__ pn, const int* __restrict__ pw, int* __restrict__ nsel,
               unsigned long long* __restrict__ key)
{
    const int64_t i = (int64_t)blockIdx.x * CP_TPB + threadIdx.x;
    const bool valid = i < n;
    int r = -1;
    bool sel = false;
    if (valid) {
        r = rid[i];
        if (root[i] == (int)i) {
            const bool circ = prv[i] >= 0 && pw[i] != 0;
            sel = select == 0 || (select == 1 && circ);
            if (circ) atomicMax(key + r0 + r, co_key(pn[i], lab[i]));
        }
    }
    const int rf = __builtin_amdgcn_readfirstlane(r);
    if (__all(!valid || r == rf)) {                                   // the wave lies in one range: one atomic for all its roots
        const unsigned long long m = __ballot(sel);
        if (m != 0ull && (threadIdx.x & 63) == 0) atomicAdd(nsel + r0 + rf, (int)__popcll(m));
    } else if (sel) {
        atomicAdd(nsel + r0 + r, 1);
    }
}

// Segment i of a group, after k_co_pick: is its piece selected?  ring: prv[i] >= 0; t = root[i] (k_co_root left 0 <= t < n); lab_i its
// label; key_r the winning key of its range.  w: the winding of its ring (0 for an open piece); ismain: its piece is the main ring.
__device__ __forceinline__ bool co_selected(int select, bool ring, int t, int lab_i, const unsigned* __restrict__ pn,
                                            const int* __restrict__ pw, unsigned long long key_r, int& w, bool& ismain)
{
    w = ring ? pw[t] : 0;
    const bool circ = w != 0;
    ismain = circ && co_key(pn[t], lab_i) == key_r;
    return select == 0 || (select == 1 ? circ : ismain);
}

// The three selection launches of the group `run` stands in, behind its rounds: root, pn and pw take the free buffers nxt, lab2 and nxt2
struct CoRoles { int* root; unsigned* pn; int* pw; };
inline CoRoles co_launch_select(const CpRun& run, int wrap, int64_t nx, const double* pts, int select, int* nsel, unsigned long long* key)
{
    const CpRoles& b = run.b;
    const CoRoles s = {b.nxt, (unsigned*)b.lab2, b.nxt2};
    const dim3 blk(CP_TPB);
    hipStream_t stream = run.ctx->stream;
    hipLaunchKernelGGL(k_co_root, run.grid, blk, 0, stream, run.n, run.pl.E, run.t.tab, run.t.rid, b.lab, s.root, s.pn, s.pw);
    hipLaunchKernelGGL(k_co_piece, run.grid, blk, 0, stream, run.n, run.s0, wrap, nx, pts, s.root, s.pn, s.pw);
    hipLaunchKernelGGL(k_co_pick, run.grid, blk, 0, stream, run.n, run.g.r0, select, run.t.rid, s.root, b.prv, b.lab, s.pn, s.pw, nsel, key);
    return s;
}

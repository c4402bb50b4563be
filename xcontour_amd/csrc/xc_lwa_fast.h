// K7F, the interval kernel: k_lwa_check (its premises, on the device) and k_lwa_fast.  Included inside namespace xc { namespace { ... } }
// of xc_lwa.hip, behind xc_lwa_walk.h.
#pragma once

// =====================================================================================
// K7F  large planes: O(ny log ny) per column instead of O(J * band)            (round 4)
// =====================================================================================
// With q' = s q, Q' = s Q (s = +1 if increase else -1; Q' non-decreasing in j -- it is the sorted reference state) the
// sum of core.py:789 is, per column x and target row j,
//     lwa[j, x] = s * (  sum_{y >= j, q'_y < Q'_j} (Q'_j - q'_y) W_y   [near side, mask3 = +1]
//                      + sum_{y <  j, q'_y > Q'_j} (q'_y - Q'_j) W_y ) [far side,  mask3 = -1],   W = (dA / max dA) * M.
// Because Q' is monotone, the targets a cell (y, x) contributes to form ONE interval of j: with b = #{j: Q'_j < q'_y} and
// a = #{j: Q'_j <= q'_y} (two bounds of one binary search) the cell is a near-side term of j in [a, y] (if a <= y) or a
// far-side term of j in [y + 1, b - 1] (if b >= y + 2), never both.  Either way it adds +W at index p (= a or b) and -W at
// index y + 1 of a difference array D0, and the same with (q'_y - c) W in D1 (c: a reference level that keeps the two big
// terms of the final difference small).  Prefix sums S0, S1 over j then give lwa = s ((Q'_j - c) S0_j - S1_j).
// One binary search and four LDS adds per cell; the band walk costs O(band) per (cell, target group).  The sums are formed
// in another order and through a difference of two products: agreement with the bit-exact kernels is ~1e-13 relative to
// the column's largest value (tests: 1e-9), not bit for bit -- so this path serves planes of more than kLwaFastMinRows rows
// (where the band walk takes milliseconds) and only after k_lwa_check has PROVED its premises (no NaN in Q, Q' monotone,
// the coordinate strictly monotone); xc_set_lwa_exact(ctx, 1) keeps the band walk everywhere.
constexpr int kLwaFastMinRows = 512;

__global__ __launch_bounds__(256)
void k_lwa_check(const double* __restrict__ Q, const double* __restrict__ coord, int ny, int increase, unsigned* __restrict__ flag, unsigned epoch)
{
    const double* Qs = Q + (size_t)blockIdx.x * ny;
    const double s = increase ? 1.0 : -1.0;
    const bool cinc = lwa_coord_incre(coord, ny);
    int bad = 0;
    for (int j = threadIdx.x; j < ny; j += 256) {
        const double v = Qs[j];
        bad |= !(fabs(v) < dinf());   // finite: NaN fails, and so does an infinite level ((Q'_j - c) * S0 = inf * 0 = NaN in the interval kernel where the reference sums to 0)
        if (j + 1 < ny) {
            bad |= !(s * Qs[j + 1] >= s * v);                          // (a NaN neighbour fails too)
            bad |= cinc ? !(coord[j + 1] > coord[j]) : !(coord[j + 1] < coord[j]);
        }
    }
    if (__syncthreads_or(bad) && threadIdx.x == 0) atomicMax(flag, epoch);      // the word holds the epoch of the last call whose check failed
}

// (round 5) The kernel is PERSISTENT over column groups -- `gridDim.x` workgroups (one per CU: the difference arrays fill the LDS)
// walk the groups b, b + gridDim.x, ... -- so that
//   * Q' and the bucket table below are staged once per workgroup, not once per group;
//   * the cells of the NEXT group are requested before this group's prefix sums, transform and stores (a group used to pay its
//     ~5 us of load latency with nothing else in flight: one workgroup per CU);
//   * bracket search: a table G of LWA_NB + 1 row indices over equal-width value buckets of [Q'_0, Q'_last] -- G[k] = number of levels
//     whose bucket is below k, the bucket being the SAME monotone function of the value for levels and cells -- confines the lower
//     bound of a cell of bucket k to [G[k], G[k + 1]] exactly (no float consistency needed between an edge and a cell), so the 11
//     dependent LDS reads of a full binary search over 1801 levels become ~1 (measured by ablation: the search was 32 of the 108 us);
//   * the prefix sums use all sixteen waves (two waves per array: 128 pieces) instead of eight.
constexpr int LWA_NB = 4096;
// The kernel's LDS.  ONE walk of the layout: with a null base it only adds up `bytes` (the CG ladder of the plan, the launch), with the
// kernel's it hands out the arrays.  D1 follows D0 directly: the kernel clears both with one loop.
struct LwaFastLds {
    double* Qs;          // [ny + 1]      Q' = s Q (ny used)
    double *D0, *D1;     // [CG][ny + 1]  the difference arrays
    int* G;              // [LWA_NB + 1]  the bucket table
    size_t bytes;
};
__host__ __device__ __forceinline__ LwaFastLds lwa_fast_lds(void* base, int ny, int CG)
{
    const int L = ny + 1;
    size_t n = 0;                                                    // doubles handed out so far
    auto take = [&](size_t doubles) { double* p = base ? (double*)base + n : nullptr; n += doubles; return p; };
    LwaFastLds l;
    l.Qs = take(L); l.D0 = take((size_t)CG * L); l.D1 = take((size_t)CG * L); l.G = (int*)take(0);
    l.bytes = n * 8 + (size_t)(LWA_NB + 1) * 4;
    return l;
}
template <typename T>
__global__ __launch_bounds__(1024)
void k_lwa_fast(const T* __restrict__ q, const double* __restrict__ Q, const double* __restrict__ dA, int dA_rank, double dA_max,
                const double* __restrict__ M, int M_rank, int ny, int64_t nx, int increase, int side, int CG, int64_t nvb,
                double* __restrict__ out, unsigned* __restrict__ gate, unsigned epoch)
{
    if (gate && *gate == epoch) return;          // k_lwa_check found a premise broken: the band walk enqueued behind this kernel runs instead (gate NULL: the caller vouches)
    extern __shared__ __align__(16) double sm[];
    const int tid = threadIdx.x, nthr = blockDim.x, slab = blockIdx.y;
    const int L = ny + 1;
    const LwaFastLds l = lwa_fast_lds(sm, ny, CG);
    double* Qs = l.Qs;  double* D0 = l.D0;  double* D1 = l.D1;  int* G = l.G;
    __shared__ double s_half[16];
    const double s = increase ? 1.0 : -1.0;
    const double* Qg = Q + (size_t)slab * ny;
    for (int j = tid; j < ny; j += nthr) Qs[j] = s * Qg[j];
    __syncthreads();
    const double cref = Qs[ny / 2];
    const double q0 = Qs[0], qw_ = Qs[ny - 1] - q0;
    const double bscale = (qw_ > 0.0) ? (double)LWA_NB / qw_ : 0.0;
    auto bucket = [&](double v) { return (int)fmin(fmax((v - q0) * bscale, 0.0), (double)(LWA_NB - 1)); };      // monotone in v; NaN -> 0
    for (int j = tid; j <= ny; j += nthr) {                            // Q' is sorted: level j opens the buckets (k_{j-1}, k_j]
        const int kp = j == 0 ? -1 : bucket(Qs[j - 1]), kj = j < ny ? bucket(Qs[j]) : LWA_NB;
        for (int k = kp + 1; k <= kj; ++k) G[k] = j;
    }
    const T* qs = q + (size_t)slab * ny * nx;
    double* os = out + (size_t)slab * ny * nx;
    // Column groups that share 128-byte lines (16 float64 columns = 16 / CG groups) go to ONE XCD: workgroups are dealt round-robin
    // over the eight XCDs (b and b + 8 share one), each XCD has its own L2, and a group touches only CG * 8 bytes of every line of
    // its rows -- with the plain order the four groups of a line ran on four XCDs and every line of the tracer, the weights and the
    // output crossed the fabric four times (measured: 0.176 -> 0.148 ms per cfg2-sized slab; two / one columns per workgroup: 0.217 / 0.362).
    // virtual block vb = 8 k + xcd  ->  group ((k / GQ) * 8 + xcd) * GQ + k % GQ, GQ = 16 / CG groups per line; vb runs over nvb
    // (a multiple of 8 GQ) in steps of gridDim.x (a multiple of 8: vb keeps its XCD) and the surplus groups are skipped.
    const int GQ = 16 / CG;
    auto group_x0 = [&](int64_t vb) { const int64_t kq = vb >> 3, xcd = vb & 7; return (((kq / GQ) * 8 + xcd) * GQ + (kq % GQ)) * CG; };
    // cells: row-major over (y, column of the group); CPT cells per thread and round: all their loads are issued first (a workgroup
    // of 1024 threads x 8 covers the 7204 cells of four cfg2 columns in ONE round of loads), then the CPT searches advance together
    constexpr int CPT = 8;
    T qraw[CPT];
    double da[CPT], mm_[CPT];
    const double inv_max = 1.0 / dA_max;
    const bool da_row = dA_rank == XC_DA_ROW, m_row = M_rank == XC_DA_NONE ? da_row : (M_rank == XC_DA_ROW);
    const double* Mp = M_rank == XC_DA_NONE ? dA : M;
    // cell i of a group: row i >> cshift, column i & (CG - 1) (CG is 4, 2 or 1: no integer division -- with a runtime `ncol` the four
    // index computations per cell were ~1300 instructions per thread and group, ~9 of a group's ~28 us); columns >= ncol of a ragged
    // last group are simply not there
    const int cshift = CG == 4 ? 2 : (CG == 2 ? 1 : 0), cmask = CG - 1;
    const int ncell = ny << cshift;
    // Addresses: a uniform base (the group's first column: scalar registers) + a 32-bit byte offset per cell; a plane-rank weight
    // shares the tracer's element offset, a row-rank one uses the row.  (Per-cell 64-bit addresses of three arrays, kept alive over the
    // group loop as loop invariants, cost 71 spilled VGPRs in the first persistent version.)  The launcher admits planes of < 2^29 cells.
    auto request = [&](int64_t x0, int ncol, int i0) {                 // the loads of one round of one group (clamped: never out of bounds)
        asm volatile("" : "+v"(i0));                                   // (not a loop invariant: the few index operations per cell are recomputed, not kept in 24 registers)
        const char* qb = (const char*)(qs + x0);
        const char* db = (const char*)(da_row ? dA : dA + x0);
        const char* mb = (const char*)(m_row ? Mp : Mp + x0);
#pragma unroll
        for (int u = 0; u < CPT; ++u) {
            const int i = i0 + u * nthr;
            const unsigned y = (unsigned)((i < ncell ? i : 0) >> cshift), c = (unsigned)((i & cmask) < ncol ? (i & cmask) : 0);
            const unsigned e = y * (unsigned)nx + c;                       // element offset from the group's first column
            qraw[u] = *(const T*)(qb + (size_t)(e * (unsigned)sizeof(T)));
            da[u] = *(const double*)(db + (size_t)((da_row ? y : e) * 8u));    // branch-free: the rank picks the INDEX (three loads per cell, no control flow)
            mm_[u] = *(const double*)(mb + (size_t)((m_row ? y : e) * 8u));    // (no M: the weight itself, from the same line -- core.py:789 with M = dA)
        }
    };
    int64_t vb = blockIdx.x;
    while (vb < nvb && group_x0(vb) >= nx) vb += gridDim.x;
    if (vb < nvb) { const int64_t x0 = group_x0(vb); request(x0, (int)((nx - x0 < CG) ? nx - x0 : CG), tid); }
    while (vb < nvb) {
        const int64_t x0 = group_x0(vb);
        const int ncol = (int)((nx - x0 < CG) ? nx - x0 : CG);
        int64_t vnext = vb + gridDim.x;
        while (vnext < nvb && group_x0(vnext) >= nx) vnext += gridDim.x;
        for (int i = tid; i < 2 * CG * L; i += nthr) D0[i] = 0.0;
        __syncthreads();                                               // (also: Qs, G of the prologue; the stores of the group before)
        for (int i0 = tid; i0 < ncell; i0 += CPT * nthr) {
            if (i0 != tid) request(x0, ncol, i0);                      // (planes of more than 2048 rows: further rounds, not prefetched)
            int lo[CPT], hi[CPT];
            double qv[CPT], wv[CPT];
            bool ok[CPT];
#pragma unroll
            for (int u = 0; u < CPT; ++u) {
                const int i = i0 + u * nthr;
                ok[u] = i < ncell && (i & cmask) < ncol;
                qv[u] = s * (double)qraw[u];
                wv[u] = (da[u] * inv_max) * mm_[u];                       // (u * wei) * M of core.py:789, weights first (wei = dA / max: here times the reciprocal -- eight float64 divisions per thread and group were ~7 % of the kernel; this path is not the bit-exact one)
                // an INFINITE tracer cell is a premise this kernel cannot check ahead of time: +-inf into the difference arrays turns every
                // row behind the cell into inf - inf = NaN, where the reference's per-row sums stay finite.  Stamp the flag: the gated band
                // walk enqueued behind this kernel then runs and overwrites the plane (mode 3 has no gate: the caller vouched for finite cells)
                if (gate && ok[u] && fabs(qv[u]) == dinf()) atomicMax(gate, epoch);
                ok[u] = ok[u] && (qv[u] == qv[u]) && (wv[u] == wv[u]);    // NaN tracer / weight: the term is NaN and nansum skips it
                const int k = bucket(qv[u]);
                lo[u] = ok[u] ? G[k] : 0; hi[u] = ok[u] ? G[k + 1] : 0;   // lower bound: first j with Q'_j >= q'
            }
            for (int step = 0; step < 32; ++step) {                       // ceil(log2(ny + 1)) steps at most; ~1 behind the bucket table
                bool any = false;
#pragma unroll
                for (int u = 0; u < CPT; ++u)
                    if (lo[u] < hi[u]) { const int mid = (lo[u] + hi[u]) >> 1; if (Qs[mid] < qv[u]) lo[u] = mid + 1; else hi[u] = mid; any = true; }
                if (!any) break;
            }
#pragma unroll
            for (int u = 0; u < CPT; ++u) {
                if (!ok[u]) continue;
                const int i = i0 + u * nthr, y = i >> cshift, c = i & cmask;
                const int b = lo[u];
                int a = b;
                while (a < ny && Qs[a] == qv[u]) ++a;                      // upper bound: ties with a level are rare
                int p = -1;
                if (a <= y) { if (side != 2) p = a; }                      // near-side term of targets [a, y]
                else if (b >= y + 2) { if (side != 1) p = b; }             // far-side term of targets [y + 1, b - 1]
                if (p >= 0) {
                    double* d0 = D0 + (size_t)c * L;
                    double* d1 = D1 + (size_t)c * L;
                    const double w = wv[u], qw = (qv[u] - cref) * w;
                    atomicAdd(d0 + p, w);  atomicAdd(d0 + y + 1, -w);
                    atomicAdd(d1 + p, qw); atomicAdd(d1 + y + 1, -qw);
                }
            }
        }
        // the next group's first round of loads is requested HERE: its latency runs under this group's prefix sums and stores (while the
        // searches run the registers are needed: requested before them, 60 VGPRs spilled and the kernel was slower than without)
        __builtin_amdgcn_sched_barrier(0);                             // (the scheduler must not lift these loads above the searches)
        if (vnext < nvb) { const int64_t xn = group_x0(vnext); request(xn, (int)((nx - xn < CG) ? nx - xn : CG), tid); }
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        // prefix sums over j, in place: an array is cut into 64 * split contiguous pieces, every lane sums its piece (independent LDS
        // reads, one dependent add each), ONE wave scan of the piece totals (the second wave of an array adds the first one's
        // total), then the piece is written back with its offset.  Then lwa[j] = s ((Q'_j - c) S0_j - S1_j) overwrites D0.
        {
            const int wave = tid >> 6, lane = tid & 63, nw = nthr >> 6;
            const int split = (4 * ncol <= nw) ? 2 : 1;
            const int per = (ny + 64 * split - 1) / (64 * split);
            for (int t0 = 0; t0 < 2 * ncol * split; t0 += nw) {
                const int task = t0 + wave;
                const bool on = task < 2 * ncol * split;
                const int arr = on ? task / split : 0, h = task % split;
                double* d = (arr & 1 ? D1 : D0) + (size_t)(arr >> 1) * L;
                int j0 = (h * 64 + lane) * per, j1 = j0 + per;
                if (j1 > ny) j1 = ny;
                if (!on) j1 = j0;
                double tot = 0.0;
                for (int j = j0; j < j1; ++j) tot += d[j];
                double v = tot;                                            // inclusive scan of the piece totals over the lanes
                for (int o = 1; o < 64; o <<= 1) { const double tt = __shfl_up(v, o); if (lane >= o) v += tt; }
                double base = 0.0;
                if (split == 2) {                                          // (uniform over the workgroup: ncol is)
                    if (on && h == 0 && lane == 63) s_half[arr] = v;
                    __syncthreads();
                    if (on && h == 1) base = s_half[arr];
                    __syncthreads();
                }
                double run = base + (v - tot);                             // sum of the pieces before this lane's
                for (int j = j0; j < j1; ++j) { run += d[j]; d[j] = run; }
            }
        }
        __syncthreads();
        // lwa and its store in one sweep (a thread reads only the two sums of its own cell: nothing to wait for in between)
#pragma unroll 2
        for (int i = tid; i < ncell; i += nthr) {
            const int y = i >> cshift, c = i & cmask;
            if (c < ncol) os[(size_t)y * nx + x0 + c] = s * ((Qs[y] - cref) * D0[(size_t)c * L + y] - D1[(size_t)c * L + y]);
        }
        __syncthreads();                                               // D0 is cleared at the top of the next group
        vb = vnext;
    }
}

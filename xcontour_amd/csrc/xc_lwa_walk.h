// K7, the band walk (bit-exact): what every walk shares, written once, and the three kernels built from it -- k_lwa_prep + k_lwa (any
// plane) and k_lwa_strip (one launch, the strip of the tracer in LDS).  Included inside namespace xc { namespace { ... } } of xc_lwa.hip.
#pragma once

constexpr int LWA_RB = 8;     // rows per load batch of k_lwa; rowinfo is padded by as many rows
constexpr int LWA_SW = 8;     // k_lwa_strip: waves per workgroup = target rows in flight per workgroup (cfg3: 256 workgroups, one per CU)

// a value every lane of the wave holds: hand it to the scalar unit
__device__ __forceinline__ double lane_uniform(double v)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(u & 0xffffffffu));
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(u >> 32));
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// ---------------------------------------------------------------- the rules of the walk
// core.py:736-738: the direction of the coordinate
template <typename I>
__device__ __forceinline__ bool lwa_coord_incre(const double* coord, I ny) { return !(coord[ny - 1] < coord[0]); }

// core.py:757: row y' (coordinate cy) is on the near side of target row j (coordinate cj)
__device__ __forceinline__ bool lwa_near(int coord_incre, double cy, double cj) { return coord_incre ? (cy >= cj) : (cy <= cj); }

// part (core.py:773-784): 'upper' keeps mask3 > 0 (the near side) if increase else mask3 < 0 (the far side).
// 0: both sides, 1: the near side only, -1: the far side only
__host__ __device__ __forceinline__ int lwa_keep(int part, int increase) { return part == 0 ? 0 : (((part == 1) == (increase != 0)) ? 1 : -1); }

// Can row y' contribute to target row j?  mask3(j, y', x) != 0 needs qe < 0 on the near side or qe > 0 on the far side of row j (the other
// way round with inc_eff == 0), and the NaN-skipping extrema of the strip's rows bound qe:
//   V1: qe = q[y',x] - Q[j]  in [rmin - Q_j, rmax - Q_j]   (rmin / rmax of row y', tlo = thi = Q_j);
//   V2: qe = q[j,x]  - Q[y'] in [tlo - Q_y, thi - Q_y]     (tlo / thi: min / max of tracer row j, Qy = Q[y']).
// `near`: lwa_near of the two rows.  keep != 0 drops the side that `part` does not keep; k_lwa passes 0 here (its band is found over both
// sides) and applies `keep` in lwa_add_term, k_lwa_strip does it the other way round.
template <bool V2>
__device__ __forceinline__ bool lwa_row_needed(double rmin, double rmax, double Qy, double tlo, double thi, bool near, int inc_eff, int keep)
{
    const bool anypos = V2 ? (thi > Qy) : (rmax > thi);
    const bool anyneg = V2 ? (tlo < Qy) : (rmin < tlo);
    const bool nd = near ? (inc_eff ? anyneg : anypos) : (inc_eff ? anypos : anyneg);
    return nd && !(keep != 0 && (keep > 0) != near);
}

// the ballot `hit` of lwa_row_needed over rows yy .. yy + 63 widens the span [y0, y1) of rows to walk
template <typename I>
__device__ __forceinline__ void lwa_span_add(unsigned long long hit, I yy, I& y0, I& y1)
{
    if (hit) {
        const I first = yy + (__ffsll((long long)hit) - 1), last = yy + 63 - __clzll((long long)hit);
        y0 = first < y0 ? first : y0; y1 = last + 1 > y1 ? last + 1 : y1;
    }
}

// One term of core.py:789 for (target row j, row y', column x): acc += |qe * mask3 * wei * M|, skipped like nansum skips it when it is NaN.
// mask3 (core.py:759-766 / 865-872) with the side of row y' WAVE-UNIFORM (cy, cj are):  mask3 != 0  <=>  u > 0 with u = -qe on the side
// where mask3 = +-1 needs qe < 0 and u = +qe on the other; qe * mask3 = -+u exactly (a - b and b - a are exact negations, as are x * (-1)
// and -x), so the term is -+((u * wei) * M) bit for bit with numpy's products taken in its order, and only |term| is accumulated: every
// term of a sum has the same sign, which lwa_result puts on at the end (negation commutes with rounding).  Qj: V1 the level Q[j], V2 the
// tracer on target row j; qv: V1 the tracer on row y', V2 the level Q[y'] (qe = a - b, core.py:754 / 860).
// (u > 0 stays a branch: for most (j, y') pairs no lane contributes and the wave skips the products; a branch-free select version
//  measured 89 vs 63 us on cfg3.)
template <bool V2>
__device__ __forceinline__ void lwa_add_term(double& acc, int coord_incre, double cy, double cj, int keep, int inc_eff,
                                             double Qj, double qv, double wei, double mv)
{
    const bool m = lwa_near(coord_incre, cy, cj);
    if (keep != 0 && (keep > 0) != m) return;                              // 'upper' / 'lower' keep one side (core.py:775-784)
    const double a = V2 ? Qj : qv, b = V2 ? qv : Qj;
    const double u = (m == (inc_eff != 0)) ? __dsub_rn(b, a) : __dsub_rn(a, b);
    if (u > 0.0) {
        const double term = __dmul_rn(__dmul_rn(u, wei), mv);
        if (term == term) acc = __dadd_rn(acc, term);                      // nansum
    }
}

// -(sum of terms), core.py:789, from the sum of |term|; an empty sum is -0.0 there
__device__ __forceinline__ double lwa_result(double acc, int inc_eff) { return inc_eff ? (acc == 0.0 ? -0.0 : acc) : -acc; }

// ---------------------------------------------------------------- the scratch of k_lwa_prep + k_lwa
//  * wei = dA.squeeze() / max(dA) (core.py:723-724), same rank as dA: it does not depend on the target row, so one division per cell
//    instead of one per (target row, cell);
//  * rowinfo[slab][ny + LWA_RB][2] = {coord, Q} (padded, contiguous: wide scalar loads in k_lwa);
//  * stripmm[slab][strip][ny][2]: NaN-skipping min / max of every 64-column strip of every tracer row (lwa_row_needed).
// The two index expressions give the doubles in front of a pair; the layout is sized through them.  (Macros: as a function -- forced
// inline, constexpr, arguments by value or by reference -- the second one changed the register allocation and the schedule of
// k_lwa_prep's store loop.)
#define LWA_ROWINFO_AT(ny, slab, y) (((size_t)(slab) * ((ny) + LWA_RB) + (y)) * 2)
#define LWA_STRIPMM_AT(ny, nstrip, slab, strip, y) ((((size_t)(slab) * (nstrip) + (strip)) * (ny) + (y)) * 2)
struct LwaScratch { double *wei, *rowinfo, *stripmm; int64_t nstrip; size_t bytes; };
// ONE walk of the layout: with a null base it only adds up `bytes`
inline LwaScratch lwa_scratch(void* base, int64_t nslab, int64_t ny, int64_t nx, int dA_rank)
{
    LwaScratch w;
    w.nstrip = (nx + 63) / 64;
    w.bytes = 0;
    auto take = [&](double*& p, size_t n) { p = base ? (double*)((char*)base + w.bytes) : nullptr; w.bytes += n * 8; };
    take(w.wei, (size_t)(dA_rank == XC_DA_ROW ? ny : ny * nx));
    take(w.rowinfo, LWA_ROWINFO_AT(ny, nslab, 0));
    take(w.stripmm, LWA_STRIPMM_AT(ny, w.nstrip, nslab, 0, 0));
    return w;
}

// Once per call, one block per (row, slab, chunk of 64 strips): fills the scratch above.  A strip row whose extrema exclude a contribution
// (almost all rows away from the band where the tracer is displaced across Q[j]) adds nothing for the wave that owns the strip and is
// never loaded by it.
template <typename T>
__global__ __launch_bounds__(256)
void k_lwa_prep(const T* __restrict__ q, const double* __restrict__ Q, const double* __restrict__ coord,
                const double* __restrict__ dA, int dA_rank, double dA_max,
                int64_t ny, int64_t nx, int64_t nstrip, double* __restrict__ wei, double* __restrict__ rowinfo,
                double* __restrict__ stripmm, const unsigned* __restrict__ gate, unsigned epoch)
{
    if (gate && *gate != epoch) return;      // the interval kernel (K7F) took this call: its premises held (k_lwa_check)
    const int64_t y = blockIdx.x, slab = blockIdx.y;
    const double inf = dinf();
    double* ri = rowinfo + LWA_ROWINFO_AT(ny, slab, y);
    if (y >= ny) {                                        // padding rows are never inside a band
        if (threadIdx.x == 0 && blockIdx.z == 0) { ri[0] = coord[ny - 1]; ri[1] = dnan(); }
        return;
    }
    if (threadIdx.x == 0 && blockIdx.z == 0) { ri[0] = coord[y]; ri[1] = Q[(size_t)slab * ny + y]; }
    const T* row = q + ((size_t)slab * ny + y) * nx;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // blockIdx.z: chunk of 64 strips (a very wide, short plane would otherwise walk all its strips in one block)
    const int64_t st1 = ((int64_t)blockIdx.z + 1) * 64 < nstrip ? ((int64_t)blockIdx.z + 1) * 64 : nstrip;
    for (int64_t st = (int64_t)blockIdx.z * 64 + wave; st < st1; st += 4) {
        const int64_t x = st * 64 + lane;
        double mn = inf, mx = -inf;
        if (x < nx) {
            const double v = (double)row[x];
            mn = fmin(mn, v); mx = fmax(mx, v);
            if (slab == 0 && dA_rank != XC_DA_ROW) wei[y * nx + x] = __ddiv_rn(dA[y * nx + x], dA_max);
        }
        for (int o = 32; o > 0; o >>= 1) { mn = fmin(mn, __shfl_xor(mn, o)); mx = fmax(mx, __shfl_xor(mx, o)); }
        if (lane == 0) {
            double* sm = stripmm + LWA_STRIPMM_AT(ny, nstrip, slab, st, y);
            sm[0] = mn; sm[1] = mx;
        }
    }
    if (slab == 0 && dA_rank == XC_DA_ROW && threadIdx.x == 0 && blockIdx.z == 0) wei[y] = __ddiv_rn(dA[y], dA_max);
}

// The streaming walk: lanes along X (coalesced row reads), a wave owns a 64-column strip and JT target rows; the grid has one column of
// blocks per strip (gridDim.x = nstrip).
// V2: cal_local_wave_activity2 (core.py:802-905): qe = q[row j] - Q[all rows], opposite sign convention.
// JT target rows per thread: 1 for small problems (more waves in flight), 4 when the slab is large
// (each thread re-streams its column once per JT targets).
template <typename T, bool V2, int JT>
__global__ __launch_bounds__(256)
void k_lwa(const T* __restrict__ q, const double* __restrict__ Q, const double* __restrict__ coord,
           const double* __restrict__ wei_, int dA_rank,
           const double* __restrict__ M, int M_rank, const double* __restrict__ rowinfo,
           const double* __restrict__ stripmm,
           int64_t ny, int64_t nx, int increase, int part, double* __restrict__ out, const unsigned* __restrict__ gate, unsigned epoch)
{
    if (gate && *gate != epoch) return;      // (see k_lwa_prep)
    const int coord_incre = lwa_coord_incre(coord, ny);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t x = (int64_t)blockIdx.x * 64 + lane;
    const int64_t j0 = ((int64_t)blockIdx.y * 4 + wave) * JT;
    if (j0 >= ny) return;
    const size_t so = (size_t)blockIdx.z * ny * nx;
    const T* qs = q + so;
    const double* Qs = Q + (size_t)blockIdx.z * ny;
    const bool active = x < nx;

    const double* rinfo = rowinfo + LWA_ROWINFO_AT(ny, blockIdx.z, 0);
    const double* smm = stripmm + LWA_STRIPMM_AT(ny, gridDim.x, blockIdx.z, blockIdx.x, 0);      // this wave's strip
    double Qj[JT], cj[JT], acc[JT];
    double tlo[JT], thi[JT];            // wave-uniform: V1 the target level Q[j] (both), V2 min / max of the strip of tracer row j
#pragma unroll
    for (int t = 0; t < JT; ++t) {
        const int64_t j = (j0 + t < ny) ? j0 + t : ny - 1;
        tlo[t] = V2 ? smm[2 * j] : Qs[j]; thi[t] = V2 ? smm[2 * j + 1] : Qs[j];
        Qj[t] = V2 ? (active ? (double)qs[j * nx + x] : 0.0) : Qs[j];      // V2: the tracer on target row j
        cj[t] = coord[j]; acc[t] = 0.0;
    }
    const int inc_eff = V2 ? !increase : increase;                          // core.py:865-872 vs 759-766
    const int keep = lwa_keep(part, increase);

    // rows are consumed strictly in y' order (numpy's axis-0 nansum order), but the loads of RB rows
    // are issued together so that their latency overlaps
    constexpr int RB = LWA_RB;
    const int64_t xl = active ? x : 0;
    // Band of rows that can contribute to this wave's targets, found once with the lanes spread over y': rows outside [y0, y1) -- almost
    // all rows away from where the tracer is displaced across Q[j] -- are never loaded.  (Rows inside the band that cannot contribute
    // still add nothing.)  The extrema are those of THIS wave's 64-column strip, so a meandering front costs each wave only its own part.
    int64_t y0 = ny, y1 = 0;
    for (int64_t yy = 0; yy < ny; yy += 64) {
        const int64_t y = (yy + lane < ny) ? yy + lane : ny - 1;
        const double rmin = smm[2 * y], rmax = smm[2 * y + 1], cyr = rinfo[2 * y], Qy = rinfo[2 * y + 1];
        bool nd = false;
#pragma unroll
        for (int t = 0; t < JT; ++t)
            nd |= lwa_row_needed<V2>(rmin, rmax, Qy, tlo[t], thi[t], lwa_near(coord_incre, cyr, cj[t]), inc_eff, 0);
        lwa_span_add(__ballot(nd && yy + lane < ny), yy, y0, y1);
    }
    for (int64_t yb = y0 & ~(int64_t)(RB - 1); yb < y1; yb += RB) {
        double qv_[RB], wv_[RB], mv_[RB], cy_[RB];
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const int64_t y = (yb + r < ny) ? yb + r : ny - 1;
            qv_[r] = V2 ? Qs[y] : (double)qs[y * nx + xl];
            cy_[r] = rinfo[2 * y];
            wv_[r] = (dA_rank == XC_DA_ROW) ? wei_[y] : wei_[y * nx + xl];
            mv_[r] = (M_rank == XC_DA_ROW) ? M[y] : M[y * nx + xl];
        }
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            if (yb + r >= ny) break;
            const double cy = lane_uniform(cy_[r]);                                     // the same value in every lane: keep the side test scalar
#pragma unroll
            for (int t = 0; t < JT; ++t)
                lwa_add_term<V2>(acc[t], coord_incre, cy, cj[t], keep, inc_eff, Qj[t], qv_[r], wv_[r], mv_[r]);   // wv_: dA / max(dA), core.py:724
        }
    }
    if (active) {
#pragma unroll
        for (int t = 0; t < JT; ++t)
            if (j0 + t < ny) out[so + (size_t)(j0 + t) * nx + x] = lwa_result(acc[t], inc_eff);
    }
}

// ---- small planes (the reference's own 256 x 512 field, X-Z sections): ONE launch, no prologue kernel.  A workgroup of LWA_SW waves
// owns a 64-column strip and LWA_SW consecutive target rows (one per wave, lanes along X):
//   (a) the whole strip of the tracer goes into LDS (row pitch 65: a thread can walk a row without bank conflicts), with the
//       (coord, Q) pairs and the per-row weights;  (b) one thread per row takes the NaN-skipping extrema of the strip's rows;
//   (c) every wave finds the band of rows that can contribute to its target from those (as k_lwa does) and the workgroup takes
//       the union;  (d) wei = dA / max(dA) and a 2-D metric are staged for the union band only, `wchunk` rows at a time -- the
//       f64 divisions are done for the rows that matter, once per workgroup;  (e) the waves walk their bands out of LDS.
// Same arithmetic and order as k_lwa (bit-identical).  k_lwa_prep + k_lwa remain for planes whose strip does not fit the LDS.
//
// The kernel's LDS.  ONE walk of the layout: with a null base it only adds up `bytes` (the launcher), with the kernel's it hands out the arrays.
struct LwaStripLds {
    double *c, *Q, *mn, *mx, *wr, *Mr;      // [ny] each: coord, Q, min, max of the strip's rows, row wei, row M
    double *wei, *Mp;                       // [wchunk][64] each, where the weight / the metric is a plane
    int* band;                              // [2] + padding to 64 bytes: the union band
    void* q;                                // [ny][65] of the tracer's type
    size_t bytes;
};
__host__ __device__ __forceinline__ LwaStripLds lwa_strip_lds(void* base, int64_t ny, size_t tsize, bool wplane, bool mplane, int wchunk)
{
    LwaStripLds l;
    size_t off = 0;
    auto take = [&](auto*& p, size_t bytes) {
        p = base ? (std::remove_reference_t<decltype(p)>)((char*)base + off) : nullptr;
        off += bytes;
    };
    take(l.c, (size_t)ny * 8); take(l.Q, (size_t)ny * 8); take(l.mn, (size_t)ny * 8); take(l.mx, (size_t)ny * 8);
    take(l.wr, (size_t)ny * 8); take(l.Mr, (size_t)ny * 8);
    take(l.wei, wplane ? (size_t)wchunk * 64 * 8 : 0); take(l.Mp, mplane ? (size_t)wchunk * 64 * 8 : 0);
    take(l.band, 64); take(l.q, (size_t)ny * 65 * tsize);
    l.bytes = (off + 15) & ~(size_t)15;
    return l;
}

template <typename T, bool V2>
__global__ __launch_bounds__(64 * LWA_SW)
void k_lwa_strip(const T* __restrict__ q, const double* __restrict__ Q, const double* __restrict__ coord,
                 const double* __restrict__ dA, int dA_rank, double dA_max, const double* __restrict__ M, int M_rank,
                 int64_t ny_, int64_t nx_, int increase, int part, int wchunk, double* __restrict__ out,
                 const unsigned* __restrict__ gate, unsigned epoch)
{
    if (gate && *gate != epoch) return;      // (see k_lwa_prep)
    extern __shared__ __align__(16) double sm[];
    const int ny = (int)ny_, nx = (int)nx_;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const bool wplane = dA_rank == XC_DA_PLANE, mplane = M_rank == XC_DA_PLANE;
    const LwaStripLds l = lwa_strip_lds(sm, ny, sizeof(T), wplane, mplane, wchunk);
    double* s_c = l.c;  double* s_Q = l.Q;  double* s_mn = l.mn;  double* s_mx = l.mx;  double* s_wr = l.wr;  double* s_Mr = l.Mr;
    double* s_wei = l.wei;  double* s_Mp = l.Mp;  int* s_band = l.band;  T* s_q = (T*)l.q;
    const size_t so = (size_t)blockIdx.z * ny * nx;
    const T* qs = q + so;
    const double* Qs = Q + (size_t)blockIdx.z * ny;
    const int x0 = blockIdx.x * 64, x = x0 + lane;
    const bool active = x < nx;
    const int xl = active ? x : nx - 1;
    const double inf = dinf(), nan = dnan();

    // (a) the strip: wave w takes rows w, w + LWA_SW, ...; sixteen loads in flight per lane
    for (int yb = wave; yb < ny; yb += LWA_SW * 16) {
        T r[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) { const int y = yb + LWA_SW * k; r[k] = qs[(size_t)(y < ny ? y : ny - 1) * nx + xl]; }
#pragma unroll
        for (int k = 0; k < 16; ++k) { const int y = yb + LWA_SW * k; if (y < ny) s_q[y * 65 + lane] = active ? r[k] : (T)nan; }   // beyond the plane: NaN -> no contribution
    }
    for (int y = tid; y < ny; y += 64 * LWA_SW) {
        s_c[y] = coord[y]; s_Q[y] = Qs[y];
        s_wr[y] = wplane ? 0.0 : __ddiv_rn(dA[y], dA_max);                    // core.py:723-724 (row weights: once per row)
        s_Mr[y] = mplane ? 0.0 : M[y];
    }
    __syncthreads();
    // (b) NaN-skipping extrema of the strip's rows
    for (int y = tid; y < ny; y += 64 * LWA_SW) {
        double mn[4] = {inf, inf, inf, inf}, mx[4] = {-inf, -inf, -inf, -inf};   // four independent chains: the LDS reads pipeline
#pragma unroll
        for (int c = 0; c < 64; c += 4) {
#pragma unroll
            for (int k = 0; k < 4; ++k) { const double v = (double)s_q[y * 65 + c + k]; mn[k] = fmin(mn[k], v); mx[k] = fmax(mx[k], v); }
        }
        s_mn[y] = fmin(fmin(mn[0], mn[1]), fmin(mn[2], mn[3])); s_mx[y] = fmax(fmax(mx[0], mx[1]), fmax(mx[2], mx[3]));
    }
    __syncthreads();

    const int coord_incre = lwa_coord_incre(s_c, ny);
    const int inc_eff = V2 ? !increase : increase;                             // core.py:865-872 vs 759-766
    const int keep = lwa_keep(part, increase);
    const int j = blockIdx.y * LWA_SW + wave;                                  // this wave's target row (idle beyond the plane, but it joins the barriers)
    const bool live = j < ny;
    const int jc = live ? j : ny - 1;
    const double tlo = V2 ? s_mn[jc] : s_Q[jc], thi = V2 ? s_mx[jc] : s_Q[jc], cj = s_c[jc];
    // lane's row yl of a group of 64: can it contribute to target j?
    auto needed = [&](int yl) {
        const int y = yl < ny ? yl : ny - 1;
        return lwa_row_needed<V2>(s_mn[y], s_mx[y], s_Q[y], tlo, thi, lwa_near(coord_incre, s_c[y], cj), inc_eff, keep);
    };
    // (c) the band of rows that can contribute to target j (lanes spread over y')
    int y0 = ny, y1 = 0;
    for (int yy = 0; yy < ny && live; yy += 64) lwa_span_add(__ballot(needed(yy + lane) && yy + lane < ny), yy, y0, y1);
    const double Qj = V2 ? (double)s_q[jc * 65 + lane] : s_Q[jc];
    double acc = 0.0;
    // (d) plane weights: the union band of the LWA_SW targets, staged `wchunk` rows at a time; row weights: nothing to stage,
    //     one "chunk" = the wave's own band, no barriers
    const bool staged = wplane || mplane;                                      // workgroup-uniform
    int Y0 = y0, Y1 = y1;
    if (staged) {
        if (tid == 0) { s_band[0] = ny; s_band[1] = 0; }
        __syncthreads();
        if (lane == 0 && live && y0 < y1) { atomicMin(&s_band[0], y0); atomicMax(&s_band[1], y1); }
        __syncthreads();
        Y0 = s_band[0]; Y1 = s_band[1];
    }
    const int step = staged ? wchunk : (Y1 > Y0 ? Y1 - Y0 : 1);
    for (int yc = Y0; yc < Y1; yc += step) {
        const int nr = (Y1 - yc < step) ? Y1 - yc : step;
        if (staged) {
            for (int i0 = tid; i0 < nr * 64; i0 += 64 * LWA_SW * 4) {
                double dr[4], mr[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int i = i0 + 64 * LWA_SW * k;
                    const int r = (i < nr * 64 ? i : nr * 64 - 1) >> 6, c = i & 63;
                    const size_t g = (size_t)(yc + r) * nx + (x0 + c < nx ? x0 + c : nx - 1);
                    dr[k] = wplane ? dA[g] : 0.0; mr[k] = mplane ? M[g] : 0.0;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int i = i0 + 64 * LWA_SW * k;
                    if (i < nr * 64) {
                        if (wplane) s_wei[i] = __ddiv_rn(dr[k], dA_max);    // core.py:723-724, for the rows that matter
                        if (mplane) s_Mp[i] = mr[k];
                    }
                }
            }
            __syncthreads();
        }
        // (e) this wave's rows of the chunk, in y' order -- only the rows whose extrema allow a contribution (the test of (c),
        //     a ballot per 64 rows; the span between the first and the last such row is mostly rows that cannot contribute)
        const int ya = y0 > yc ? y0 : yc, yb_ = y1 < yc + nr ? y1 : yc + nr;
        for (int yy = ya & ~63; yy < yb_ && live; yy += 64) {
            const int yl = yy + lane;
            unsigned long long hit = __ballot(needed(yl) && yl >= ya && yl < yb_);
            while (hit) {
                // four contributing rows per turn: their LDS reads are issued together, the arithmetic follows in row order
                int yr[4]; bool on[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    on[k] = hit != 0ull;
                    yr[k] = on[k] ? yy + (__ffsll((long long)hit) - 1) : yr[k > 0 ? k - 1 : 0];
                    if (k == 0 && !on[0]) yr[0] = yy;
                    hit &= hit - (on[k] ? 1ull : 0ull);
                }
                double cy[4], qv[4], wv[4], mv[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    cy[k] = s_c[yr[k]];
                    qv[k] = V2 ? s_Q[yr[k]] : (double)s_q[yr[k] * 65 + lane];
                    wv[k] = wplane ? s_wei[(yr[k] - yc) * 64 + lane] : s_wr[yr[k]];
                    mv[k] = mplane ? s_Mp[(yr[k] - yc) * 64 + lane] : s_Mr[yr[k]];
                }
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (on[k]) lwa_add_term<V2>(acc, coord_incre, cy[k], cj, 0, inc_eff, Qj, qv[k], wv[k], mv[k]);   // (`keep`: these rows passed it)
            }
        }
        if (staged) __syncthreads();
    }
    if (live && active) out[so + (size_t)j * nx + x] = lwa_result(acc, inc_eff);
}

// The per-cell rule of the contour-length kernels, shared by K10 (xc_clen.hip: all levels of a plane), K11 (xc_lclen.hip: one
// level per sliding window) and K15 (xc_cline.hip: line integrals): the segments one NaN-free cell emits for one crossed level and
// their lengths (cell_segments), added to a fixed-point accumulator in LDS (cell_level).  The rule itself is stated in the header of xc_clen.hip.  Also here, because more than one kernel needs them:
// the case index and the four edge points of a cell (cell_case, cell_edges: K10, K11 and K12's xc_cseg_cell.h), the fold of an LDS
// accumulator into carried limbs (clen_carry, clen_carry_top: K10, K11) and the block-wide coordinate maxima behind the window
// constants (window_maxima: K13's k_cp_area_window; clen_segment_bound: k_clen_window, K15's k_cline_window).  Included inside namespace xc { namespace { ... } } after
// xc_binning.h.
#pragma once

constexpr int CLEN_COPY_CELLS = 32767;      // cells one LDS copy of a block may receive (2 segments x 2^48 per cell < 2^64 per word)
constexpr int CLEN_WORDS = kDetWords;       // limbs + the trash word of a low chunk under the window
constexpr unsigned CLEN_FLAG = 1u << 28;    // count word: a non-finite length was seen (k_det3_reduce channel-0 flag)

__device__ __forceinline__ double frac_of(double a, double b, double c) { return a == b ? 0.0 : __ddiv_rn(__dsub_rn(c, a), __dsub_rn(b, a)); }

// np.interp(x, arange(n), F) for x = i0 + f, f in [0, 1]: F[j] on a node (the last node included), else the slope formula
__device__ __forceinline__ double interp_at(double x, double i0, double F0, double F1)
{
    if (x == i0) return F0;
    if (x == i0 + 1.0) return F1;
    return __dadd_rn(__dmul_rn(__dsub_rn(F1, F0), __dsub_rn(x, i0)), F0);
}

template <bool LATLON>
__device__ __forceinline__ double seg_len(double x1, double y1, double x2, double y2)
{
    if constexpr (LATLON) {                                       // __geodist (utils.py:741-761), in its operation order
        const double sa = sin(__dmul_rn(__dsub_rn(y2, y1), 0.5)), sb = sin(__dmul_rn(__dsub_rn(x2, x1), 0.5));
        const double a = __dadd_rn(__dmul_rn(sa, sa), __dmul_rn(__dmul_rn(cos(y1), cos(y2)), __dmul_rn(sb, sb)));
        return __dmul_rn(2.0, asin(__dsqrt_rn(a)));
    } else {
        return hypot(__dsub_rn(x1, x2), __dsub_rn(y1, y2));
    }
}

__device__ __forceinline__ void add_len(unsigned long long* acc, unsigned* cnt, double w, int c0w)
{
    unsigned long long hi, lo; int E;
    const int j = det_split(w, c0w, hi, lo, E);
    lds_add(acc + (j - 1), hi);
    lds_add(acc + j, lo);
    lds_add(cnt, E == 2047 ? CLEN_FLAG | 1u : 1u);
}

// case = (ul > c) + 2 (ur > c) + 4 (ll > c) + 8 (lr > c)
__device__ __forceinline__ int cell_case(double ul, double ur, double ll, double lr, double c)
{
    return (int)(ul > c) | ((int)(ur > c) << 1) | ((int)(ll > c) << 2) | ((int)(lr > c) << 3);
}

// The four edge points of a cell in index space, each one correctly rounded sub / div / add: the columns of the top and bottom
// points, the rows of the left and right points.  (rT, cL): the cell's first row / column as doubles.
__device__ __forceinline__ void cell_edges(double ul, double ur, double ll, double lr, double c, double rT, double cL,
                                           double& tc, double& bc, double& lrow, double& rrow)
{
    tc = __dadd_rn(cL, frac_of(ul, ur, c)); bc = __dadd_rn(cL, frac_of(ll, lr, c));
    lrow = __dadd_rn(rT, frac_of(ul, ll, c)); rrow = __dadd_rn(rT, frac_of(ur, lr, c));
}

// One NaN-free cell and one crossed level: its (up to two) segments.  (rT, rB): the cell's rows as doubles, (cL, cR) its
// columns; (yT, yB) / (xL, xR) the coordinates of those nodes.  Every kept segment (coincident end points: dropped) goes to
// emit(u, v, pu, pv, len) -- u, v: its end points' ids (0 top, 1 bottom, 2 left, 3 right); pu, pv: where they lie on their edge in index
// space (the column of a top / bottom point, the row of a left / right one); len: seg_len of their coordinates.  The ONE definition of the
// segments, their end points and their lengths: K10 and K11 sum `len` (cell_level), K15 a function of all five (xc_cline_cell.h).
template <bool LATLON, typename Emit>
__device__ __forceinline__ void cell_segments(double ul, double ur, double ll, double lr, double c, double rT, double cL,
                                              double yT, double yB, double xL, double xR, Emit&& emit)
{
    const bool a = ul > c, b = ur > c, d = ll > c, e = lr > c;
    const int cs = cell_case(ul, ur, ll, lr, c);
    const double rB = rT + 1.0, cR = cL + 1.0;
    // the four edge points in index space, then in coordinates
    double tc, bc, lr_, rr;
    cell_edges(ul, ur, ll, lr, c, rT, cL, tc, bc, lr_, rr);
    const double tx = interp_at(tc, cL, xL, xR), bx = interp_at(bc, cL, xL, xR);
    const double ly = interp_at(lr_, rT, yT, yB), ry = interp_at(rr, rT, yT, yB);
    // point ids: 0 top, 1 bottom, 2 left, 3 right
    const bool eT = a != b, eB = d != e, eL = a != d, eR = b != e;
    const int p = eT ? 0 : (eB ? 1 : 2);
    const int q = cs == 9 ? 2 : (eR ? 3 : (eL ? 2 : 1));
    auto row = [&](int i) { return i == 0 ? rT : i == 1 ? rB : i == 2 ? lr_ : rr; };
    auto col = [&](int i) { return i == 0 ? tc : i == 1 ? bc : i == 2 ? cL : cR; };
    auto ycd = [&](int i) { return i == 0 ? yT : i == 1 ? yB : i == 2 ? ly : ry; };
    auto xcd = [&](int i) { return i == 0 ? tx : i == 1 ? bx : i == 2 ? xL : xR; };
    auto pos = [&](int i) { return i == 0 ? tc : i == 1 ? bc : i == 2 ? lr_ : rr; };
    // the first segment joins p and q; the saddles 6 / 9 add (bottom, left) / (bottom, right).  One loop body: the length
    // arithmetic (sin / cos / asin on the sphere) is emitted once
    const int nseg = (cs == 6 || cs == 9) ? 2 : 1;
#pragma unroll 1
    for (int t = 0; t < nseg; ++t) {
        const int u = t == 0 ? p : 1, v = t == 0 ? q : (cs == 6 ? 2 : 3);
        if (!(row(u) == row(v) && col(u) == col(v))) emit(u, v, pos(u), pos(v), seg_len<LATLON>(xcd(u), ycd(u), xcd(v), ycd(v)));
    }
}

// ... and their lengths added to one fixed-point accumulator (K10, K11)
template <bool LATLON>
__device__ __forceinline__ void cell_level(double ul, double ur, double ll, double lr, double c, double rT, double cL,
                                           double yT, double yB, double xL, double xR,
                                           unsigned long long* acc, unsigned* cnt, int c0w)
{
    cell_segments<LATLON>(ul, ur, ll, lr, c, rT, cL, yT, yB, xL, xR,
                          [&](int, int, double, double, double len) { add_len(acc, cnt, len, c0w); });
}

// One LDS accumulator (the CLEN_WORDS words add_len adds to, and its count word) folded into carried limbs: words 1..3 give their
// low 48 bits to their limb and the rest to the limb above, word 0 stays whole, the trash word is dropped; the count word gives its
// count to n and its CLEN_FLAG to flag.
__device__ __forceinline__ void clen_carry(unsigned long long (&acc)[kDetLimbsX], unsigned long long& n, unsigned& flag,
                                           const unsigned long long* words, unsigned cntword)
{
#pragma unroll
    for (int l = 0; l < kDetLimbsX; ++l) {
        const unsigned long long x = words[l];
        acc[l] += x & 0xffffffffffffull;
        if (l > 0) acc[l - 1] += x >> kDetLimbBits; else acc[0] += x & ~0xffffffffffffull;
    }
    n += cntword & 0x0fffffffu; flag |= cntword & CLEN_FLAG;
}

// ... and after the last fold the carries once more, from the last limb up: limbs 1..3 < 2^48
__device__ __forceinline__ void clen_carry_top(unsigned long long (&acc)[kDetLimbsX])
{
#pragma unroll
    for (int l = kDetLimbsX - 1; l > 0; --l) { acc[l - 1] += acc[l] >> kDetLimbBits; acc[l] &= 0xffffffffffffull; }
}

// What the window constants are bounded by, over one block of 256 threads (every thread calls it and gets both): my = the largest
// |fy[i + 1] - fy[i]| (YDIFF) or the largest |fy[i]|, mx = the largest |fx[i + 1] - fx[i]|, the seam cell fx[nx - 1] to
// fx[0] + period among them when wrap.
template <bool YDIFF>
__device__ __forceinline__ void window_maxima(const double* __restrict__ fy, int64_t ny, const double* __restrict__ fx, int64_t nx,
                                              bool wrap, double period, double& my, double& mx)
{
    const int tid = threadIdx.x;
    my = 0.0; mx = 0.0;
    for (int64_t i = tid; i + (YDIFF ? 1 : 0) < ny; i += 256) my = fmax(my, fabs(YDIFF ? fy[i + 1] - fy[i] : fy[i]));
    for (int64_t i = tid; i + 1 < nx; i += 256) mx = fmax(mx, fabs(fx[i + 1] - fx[i]));
    if (wrap && tid == 0) mx = fmax(mx, fabs(__dadd_rn(fx[0], period) - fx[nx - 1]));
    for (int o = 32; o > 0; o >>= 1) { my = fmax(my, __shfl_xor(my, o)); mx = fmax(mx, __shfl_xor(mx, o)); }
    __shared__ double s_m[2][4];
    if ((tid & 63) == 0) { s_m[0][tid >> 6] = my; s_m[1][tid >> 6] = mx; }
    __syncthreads();
    my = fmax(fmax(s_m[0][0], s_m[0][1]), fmax(s_m[0][2], s_m[0][3]));
    mx = fmax(fmax(s_m[1][0], s_m[1][1]), fmax(s_m[1][2], s_m[1][3]));
}

// K10's bound on one segment, from the plane's coordinates (every thread of a block of 256 calls it): pi on the unit sphere, else the
// largest cell diagonal (period != 0: the seam cell, fx[nx-1] to fx[0] + period, among them)
__device__ __forceinline__ double clen_segment_bound(const double* __restrict__ fy, int64_t ny, const double* __restrict__ fx, int64_t nx,
                                                     int latlon, double period)
{
    double my, mx;
    window_maxima<true>(fy, ny, fx, nx, period != 0.0, period, my, mx);
    return latlon ? 3.2 : 1.0000001 * hypot(mx, my);
}

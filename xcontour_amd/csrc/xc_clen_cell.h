// The per-cell rule of the contour-length kernels, shared by K10 (xc_clen.hip: all levels of a plane) and K11 (xc_lclen.hip: one
// level per sliding window): the segments one NaN-free cell emits for one crossed level and their lengths, added to a fixed-point
// accumulator in LDS.  The rule itself is stated in the header of xc_clen.hip.  Included inside namespace xc { namespace { ... } }
// after xc_binning.h.
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

// One NaN-free cell and one crossed level: its (up to two) segments.  (rT, rB): the cell's rows as doubles, (cL, cR) its
// columns; (yT, yB) / (xL, xR) the coordinates of those nodes.
template <bool LATLON>
__device__ __forceinline__ void cell_level(double ul, double ur, double ll, double lr, double c, double rT, double cL,
                                           double yT, double yB, double xL, double xR,
                                           unsigned long long* acc, unsigned* cnt, int c0w)
{
    const bool a = ul > c, b = ur > c, d = ll > c, e = lr > c;
    const int cs = (int)a | ((int)b << 1) | ((int)d << 2) | ((int)e << 3);
    const double rB = rT + 1.0, cR = cL + 1.0;
    // the four edge points in index space, then in coordinates
    const double tc = __dadd_rn(cL, frac_of(ul, ur, c)), bc = __dadd_rn(cL, frac_of(ll, lr, c));
    const double lr_ = __dadd_rn(rT, frac_of(ul, ll, c)), rr = __dadd_rn(rT, frac_of(ur, lr, c));
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
    // the first segment joins p and q; the saddles 6 / 9 add (bottom, left) / (bottom, right).  One loop body: the length
    // arithmetic (sin / cos / asin on the sphere) is emitted once
    const int nseg = (cs == 6 || cs == 9) ? 2 : 1;
#pragma unroll 1
    for (int t = 0; t < nseg; ++t) {
        const int u = t == 0 ? p : 1, v = t == 0 ? q : (cs == 6 ? 2 : 3);
        if (!(row(u) == row(v) && col(u) == col(v))) add_len(acc, cnt, seg_len<LATLON>(xcd(u), ycd(u), xcd(v), ycd(v)), c0w);
    }
}

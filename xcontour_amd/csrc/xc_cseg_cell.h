// The per-cell rule of the contour-segment kernel K12 (xc_cseg.hip): the DIRECTED segments one NaN-free cell emits for one crossed
// level.  The rule is K10's (header of xc_clen.hip; cell_case and cell_edges come from xc_clen_cell.h) with two differences: every segment has a
// start and an end, in the order of skimage's _get_contour_segments (fully_connected='low'), and a segment whose two end points
// coincide is kept (the join needs it; the facade drops the repeated vertex).  Included inside namespace xc { namespace { ... } }
// after xc_clen_cell.h.
#pragma once

// end point ids: 0 top, 1 bottom, 2 left, 3 right
constexpr int CSEG_T = 0, CSEG_B = 1, CSEG_L = 2, CSEG_R = 3;

// case -> (start, end) of its first segment, two bits per case.  Cases 0 and 15 emit nothing (never asked for).
//   1 T->L   2 R->T   3 R->L   4 L->B   5 T->B   6 R->T (then L->B)   7 R->B
//   8 B->R   9 T->L (then B->R)   10 B->T   11 B->L   12 L->R   13 T->R   14 L->T
constexpr unsigned cseg_pack(const int (&t)[16])
{
    unsigned w = 0u;
    for (int i = 0; i < 16; ++i) w |= (unsigned)t[i] << (2 * i);
    return w;
}
constexpr int CSEG_START_TBL[16] = {0, CSEG_T, CSEG_R, CSEG_R, CSEG_L, CSEG_T, CSEG_R, CSEG_R,
                                    CSEG_B, CSEG_T, CSEG_B, CSEG_B, CSEG_L, CSEG_T, CSEG_L, 0};
constexpr int CSEG_END_TBL[16] = {0, CSEG_L, CSEG_T, CSEG_L, CSEG_B, CSEG_B, CSEG_T, CSEG_B,
                                  CSEG_R, CSEG_L, CSEG_T, CSEG_L, CSEG_R, CSEG_R, CSEG_T, 0};
constexpr unsigned CSEG_START = cseg_pack(CSEG_START_TBL), CSEG_END = cseg_pack(CSEG_END_TBL);

// segments of a crossed cell (case 1 .. 14): two at a saddle, else one
__device__ __forceinline__ int cseg_count(int cs) { return (cs == 6 || cs == 9) ? 2 : 1; }

// One NaN-free cell (r0, c0) and one crossed level: `emit(e_from, e_to, r1, c1, r2, c2)` once per segment, in the rule's order.
// rT / cL: the cell's first row / column as doubles; hT: the id of its top edge, 2 (r0 nx + c0); nx2 = 2 nx; rwrap: what the id of
// its right edge is short of hT + 3 -- 0, except for the seam cell of a periodic plane (c0 = nx - 1), whose right edge is column
// 0's, 2 r0 nx + 1: nx2.
// Edge ids: horizontal (r, c)-(r, c+1): 2 (r nx + c); vertical (r, c)-(r+1, c): 2 (r nx + c) + 1.
template <typename Emit>
__device__ __forceinline__ void cseg_cell(double ul, double ur, double ll, double lr, double c, double rT, double cL,
                                          int64_t hT, int64_t nx2, int64_t rwrap, Emit&& emit)
{
    const int cs = cell_case(ul, ur, ll, lr, c);
    const double rB = rT + 1.0, cR = cL + 1.0;
    double tc, bc, lrow, rrow;
    cell_edges(ul, ur, ll, lr, c, rT, cL, tc, bc, lrow, rrow);
    auto row = [&](int i) { return i == CSEG_T ? rT : i == CSEG_B ? rB : i == CSEG_L ? lrow : rrow; };
    auto col = [&](int i) { return i == CSEG_T ? tc : i == CSEG_B ? bc : i == CSEG_L ? cL : cR; };
    auto eid = [&](int i) { return i == CSEG_T ? hT : i == CSEG_B ? hT + nx2 : i == CSEG_L ? hT + 1 : hT + 3 - rwrap; };
    const int nseg = cseg_count(cs);
#pragma unroll 1
    for (int t = 0; t < nseg; ++t) {
        // the saddles' second segment: 6 -> (L, B), 9 -> (B, R)
        const int u = t == 0 ? (int)((CSEG_START >> (2 * cs)) & 3u) : (cs == 6 ? CSEG_L : CSEG_B);
        const int v = t == 0 ? (int)((CSEG_END >> (2 * cs)) & 3u) : (cs == 6 ? CSEG_B : CSEG_R);
        emit(eid(u), eid(v), row(u), col(u), row(v), col(v));
    }
}

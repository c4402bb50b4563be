// The per-cell rule of K15 (xc_cline.hip): what one NaN-free cell adds, for one crossed level, to the two fixed-point channels of a
// line integral -- channel 0 the segment lengths, channel 1 the trapezoid terms of the integrand -- and the signed fold of channel 1.
// The segments, their end points and their lengths are cell_segments of xc_clen_cell.h: K10's own.  The rule is stated in the header of
// xc_cline.hip.  Included inside namespace xc { namespace { ... } } after xc_binning.h and xc_clen_cell.h.
#pragma once

constexpr int CLINE_NCH = 2;                        // channels per (slab, level): lengths, terms
constexpr int CLINE_WORDS = CLINE_NCH * CLEN_WORDS; // LDS words of one (level, copy): per channel the limbs and their trash word
// cells one LDS copy of a block may receive: terms are signed (two's complement chunks, |chunk| < 2^48), so a word must stay inside a
// SIGNED 64-bit integer: 2 segments x 16383 cells x 2^48 < 2^63 -- half of CLEN_COPY_CELLS
constexpr int CLINE_COPY_CELLS = 16383;
constexpr unsigned CLINE_FLAG = CLEN_FLAG << 1;     // count word: a non-finite term was seen (k_det3_reduce channel-1 flag)

// One kept segment: its length to channel 0, its term to channel 1 (signed), one count.  acc: the CLINE_WORDS words of a (level, copy).
__device__ __forceinline__ void add_len_term(unsigned long long* acc, unsigned* cnt, double len, double term, int c0len, int c0term)
{
    unsigned long long hi, lo; int El, Et;
    const int jl = det_split(len, c0len, hi, lo, El);
    lds_add(acc + (jl - 1), hi);
    lds_add(acc + jl, lo);
    const int jt = det_split(term, c0term, hi, lo, Et);
    const unsigned long long sm = (unsigned long long)(__double_as_longlong(term) >> 63);     // a negative term: two's complement chunks
    hi = (hi ^ sm) - sm; lo = (lo ^ sm) - sm;
    lds_add(acc + CLEN_WORDS + (jt - 1), hi);
    lds_add(acc + CLEN_WORDS + jt, lo);
    lds_add(cnt, 1u);
    if (El == 2047 || Et == 2047) atomicOr(cnt, (El == 2047 ? CLEN_FLAG : 0u) | (Et == 2047 ? CLINE_FLAG : 0u));   // (rare)
}

// One NaN-free cell and one crossed level.  (Ful, Fur, Fll, Flr): the integrand on the cell's corners, in float64.  An end point takes the
// integrand as it takes its coordinate: interp_at along its edge -- top (Ful, Fur), bottom (Fll, Flr), left (Ful, Fll), right (Fur, Flr).
// term = (0.5 (F(u) + F(v))) len: one add, one multiply by 0.5, one multiply by len.  A NaN F(u) or F(v): the segment adds nothing.
template <bool LATLON>
__device__ __forceinline__ void cline_cell_level(double ul, double ur, double ll, double lr, double Ful, double Fur, double Fll, double Flr,
                                                 double c, double rT, double cL, double yT, double yB, double xL, double xR,
                                                 unsigned long long* acc, unsigned* cnt, int c0len, int c0term)
{
    auto Fat = [&](int i, double p) {
        return i == 0 ? interp_at(p, cL, Ful, Fur) : i == 1 ? interp_at(p, cL, Fll, Flr)
             : i == 2 ? interp_at(p, rT, Ful, Fll) : interp_at(p, rT, Fur, Flr);
    };
    cell_segments<LATLON>(ul, ur, ll, lr, c, rT, cL, yT, yB, xL, xR,
        [&](int u, int v, double pu, double pv, double len) {
            const double Fu = Fat(u, pu), Fv = Fat(v, pv);
            if (Fu != Fu || Fv != Fv) return;
            add_len_term(acc, cnt, len, __dmul_rn(__dmul_rn(0.5, __dadd_rn(Fu, Fv)), len), c0len, c0term);
        });
}

// The term words of one LDS accumulator folded into carried limbs, SIGNED (the fold of the deterministic histogram's partials, xc_hist_kernel.h):
// from the last limb up, every limb below the first ends in [0, 2^48) and gives the rest -- of either sign -- to the limb above; the first
// stays signed, the trash word is dropped.  (The length words and the count word fold through clen_carry, unchanged.)
__device__ __forceinline__ void cline_carry_signed(long long (&acc)[kDetLimbsX], const unsigned long long* words)
{
    long long carry = 0;
#pragma unroll
    for (int l = kDetLimbsX - 1; l >= 0; --l) {
        long long v = acc[l] + (long long)words[l] + carry;
        carry = 0;
        if (l > 0) { carry = v >> kDetLimbBits; v -= carry << kDetLimbBits; }
        acc[l] = v;
    }
}

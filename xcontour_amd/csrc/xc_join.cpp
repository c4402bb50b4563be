// xc_join_segments: the directed segments of K12 (xc_cseg.hip) joined into polylines.  Host only -- no device, no context, no HIP
// header: this file also compiles with a plain C++ compiler.
//
// Per range (one level of one slab) the segments form disjoint chains and rings: every grid edge is the start of at most one segment
// and the end of at most one.  next(i) is the segment whose e_from == e_to[i], prev(i) the one whose e_to == e_from[i], both found by
// sort and binary search on the edge ids (no float comparison, no dense edge table).  A segment without prev heads an open polyline;
// every remaining segment lies on a ring, which starts at its segment of smallest e_from.  The polylines of a range are ordered by
// the smallest e_from they contain.  A duplicate e_from or e_to within a range is XC_EBADARG; every walk is bounded by the range size.
#include <cstdint>
#include <algorithm>
#include <vector>
#include "../../include/xcontour_hip.h"

namespace {

struct Poly { int64_t key, start, len; uint8_t closed; };   // smallest e_from, position in the walk buffer, segments, ring?

// index (into the range) of the entry of `idx` (sorted by key[idx]) whose key equals `want`, or -1
inline int64_t find_edge(const std::vector<int64_t>& idx, const int64_t* key, int64_t want)
{
    int64_t lo = 0, hi = (int64_t)idx.size();
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (key[idx[mid]] < want) lo = mid + 1; else hi = mid; }
    return (lo < (int64_t)idx.size() && key[idx[lo]] == want) ? idx[lo] : -1;
}

}  // namespace

extern "C" int xc_join_segments(int64_t nrange, const int64_t* off, const int64_t* e_from, const int64_t* e_to,
                                int64_t* order, int64_t* poly_off, uint8_t* poly_closed, int64_t* range_poly_off)
{
    if (nrange < 0 || !off || !poly_off || !range_poly_off) return XC_EBADARG;
    if (off[0] != 0) return XC_EBADARG;
    for (int64_t r = 0; r < nrange; ++r)
        if (off[r + 1] < off[r]) return XC_EBADARG;
    const int64_t total = off[nrange];
    if (total > 0 && (!e_from || !e_to || !order || !poly_closed)) return XC_EBADARG;
    int64_t npoly = 0;
    poly_off[0] = 0;
    range_poly_off[0] = 0;
    std::vector<int64_t> by_from, by_to, next, walk;
    std::vector<uint8_t> has_prev, seen;
    std::vector<Poly> polys;
    for (int64_t r = 0; r < nrange; ++r) {
        const int64_t b = off[r], n = off[r + 1] - b;
        const int64_t* ef = e_from + b;
        const int64_t* et = e_to + b;
        if (n > 0) {
            by_from.resize((size_t)n); by_to.resize((size_t)n);
            for (int64_t i = 0; i < n; ++i) by_from[(size_t)i] = by_to[(size_t)i] = i;
            std::sort(by_from.begin(), by_from.end(), [&](int64_t a, int64_t c) { return ef[a] < ef[c]; });
            std::sort(by_to.begin(), by_to.end(), [&](int64_t a, int64_t c) { return et[a] < et[c]; });
            for (int64_t i = 1; i < n; ++i)
                if (ef[by_from[(size_t)i]] == ef[by_from[(size_t)i - 1]] || et[by_to[(size_t)i]] == et[by_to[(size_t)i - 1]]) return XC_EBADARG;
            next.assign((size_t)n, -1); has_prev.assign((size_t)n, 0); seen.assign((size_t)n, 0);
            for (int64_t i = 0; i < n; ++i) {
                next[(size_t)i] = find_edge(by_from, ef, et[i]);
                has_prev[(size_t)i] = find_edge(by_to, et, ef[i]) >= 0;
            }
            walk.clear(); polys.clear();
            // heads first, then what is left (rings) from the smallest e_from up: both in ascending e_from
            for (int pass = 0; pass < 2; ++pass)
                for (int64_t j = 0; j < n; ++j) {
                    const int64_t h = by_from[(size_t)j];
                    if (seen[(size_t)h] || (pass == 0 && has_prev[(size_t)h])) continue;
                    Poly p = {ef[h], (int64_t)walk.size(), 0, (uint8_t)pass};
                    int64_t i = h;
                    for (int64_t step = 0; step < n && i >= 0 && !seen[(size_t)i]; ++step) {
                        seen[(size_t)i] = 1;
                        walk.push_back(i);
                        if (ef[i] < p.key) p.key = ef[i];
                        ++p.len;
                        i = next[(size_t)i];
                    }
                    if (pass == 1 && i != h) return XC_EBADARG;          // (cannot happen with unique ids: a ring comes back to its start)
                    polys.push_back(p);
                }
            if ((int64_t)walk.size() != n) return XC_EBADARG;
            std::sort(polys.begin(), polys.end(), [](const Poly& a, const Poly& c) { return a.key < c.key; });
            int64_t at = b;
            for (const Poly& p : polys) {
                for (int64_t t = 0; t < p.len; ++t) order[at + t] = b + walk[(size_t)(p.start + t)];
                at += p.len;
                poly_closed[npoly] = p.closed;
                poly_off[++npoly] = at;
            }
        }
        range_poly_off[r + 1] = npoly;
    }
    return XC_OK;
}

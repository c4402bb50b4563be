// The two metrics of K27 (xc_cdist.hip): the squared distance from a node to ONE segment, on the plane and on the unit sphere, every
// operation rounded once in the order written here (the build has -ffp-contract=off; tests/cdist_ref.py restates both in numpy, the
// plane bit for bit).  Also here, because they are proved against these very operations: the conservative bounds behind the pruning.
// Included inside namespace xc { namespace { ... } }.
#pragma once

// ---------------------------------------------------------------- the plane
// A segment a -> b is stored as (ay, ax, uy, ux, uu): u = b - a, uu = uy uy + ux ux.  Node p:
//   w = p - a;  t = 0 if uu == 0 else clamp((wy uy + wx ux) / uu, 0, 1);  f = a + t u;  d2 = (py - fy)^2 + (px - fx)^2
constexpr int CD_ND_PLANE = 5;
__device__ __forceinline__ double cd_d2_plane(double py, double px, double ay, double ax, double uy, double ux, double uu)
{
    const double wy = __dsub_rn(py, ay), wx = __dsub_rn(px, ax);
    double t = 0.0;
    if (uu != 0.0) {
        t = __ddiv_rn(__dadd_rn(__dmul_rn(wy, uy), __dmul_rn(wx, ux)), uu);
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    }
    const double fy = __dadd_rn(ay, __dmul_rn(t, uy)), fx = __dadd_rn(ax, __dmul_rn(t, ux));
    const double dy = __dsub_rn(py, fy), dx = __dsub_rn(px, fx);
    return __dadd_rn(__dmul_rn(dy, dy), __dmul_rn(dx, dx));
}

// Bounds on the plane are EXACT statements about the computed d2, by the monotonicity of correctly rounded +, -, * alone:
//   the computed foot f lies in [a, fl(a + u)] per coordinate (0 <= t <= 1, so fl(t u) lies between 0 and u, and fl(a + .) is monotone):
//   a block's box is the hull of a and fl(a + u) over its segments;
//   for a node p in the tile's box and f in the block's box, fl(py - fy) is at least the rounded gap between the two intervals and at
//   most the rounded far distance, in absolute value; squares and their sum are monotone on non-negative values.
// So cd_lb2_plane <= every computed d2 of (tile node, block segment) <= cd_ub2_plane: no slack is needed.
__device__ __forceinline__ double cd_gap(double tlo, double thi, double blo, double bhi)
{
    const double g = fmax(__dsub_rn(tlo, bhi), __dsub_rn(blo, thi));
    return g > 0.0 ? g : 0.0;
}
__device__ __forceinline__ double cd_far(double tlo, double thi, double blo, double bhi)
{
    return fmax(__dsub_rn(thi, blo), __dsub_rn(bhi, tlo));
}
__device__ __forceinline__ double cd_sq2(double y, double x) { return __dadd_rn(__dmul_rn(y, y), __dmul_rn(x, x)); }

// ---------------------------------------------------------------- the unit sphere
// A segment is stored as (a[3], b[3], n[3], nn): unit vectors (cos y cos x, cos y sin x, sin y), n = a x (b - a), nn = n . n.
// (a x b in exact arithmetic; but the products of a x b are of size 1 and cancel down to |n|, the arc's length, which leaves n off its
// direction by ulp(1) / |n| -- 1e-12 for a segment that cuts a cell's corner, more than the distance's stated accuracy --, whereas
// b - a is exact for an arc that short and its products are of the size of |n| themselves.)  Node p:
//   nn == 0:                                   c2 = |p - a|^2
//   (a x p) . n >= 0 and (p x b) . n >= 0:     s2 = (p . n)^2 / nn;  c2 = 2 s2 / (1 + sqrt(1 - min(s2, 1)))   (the foot lies on the arc)
//   else:                                      c2 = min(|p - a|^2, |p - b|^2)
// Products first, then sums from the left: x y' - ... as written; a dot product is ((x x' + y y') + z z').
constexpr int CD_ND_SPHERE = 10;
struct CdV { double x, y, z; };
__device__ __forceinline__ CdV cd_cross(const CdV& a, const CdV& b)
{
    return {__dsub_rn(__dmul_rn(a.y, b.z), __dmul_rn(a.z, b.y)), __dsub_rn(__dmul_rn(a.z, b.x), __dmul_rn(a.x, b.z)),
            __dsub_rn(__dmul_rn(a.x, b.y), __dmul_rn(a.y, b.x))};
}
__device__ __forceinline__ double cd_dot(const CdV& a, const CdV& b)
{
    return __dadd_rn(__dadd_rn(__dmul_rn(a.x, b.x), __dmul_rn(a.y, b.y)), __dmul_rn(a.z, b.z));
}
__device__ __forceinline__ double cd_chord2(const CdV& p, const CdV& a)
{
    const CdV d = {__dsub_rn(p.x, a.x), __dsub_rn(p.y, a.y), __dsub_rn(p.z, a.z)};
    return cd_dot(d, d);
}
__device__ __forceinline__ double cd_c2_sphere(const CdV& p, const CdV& a, const CdV& b, const CdV& n, double nn)
{
    const double ca = cd_chord2(p, a);
    if (nn == 0.0) return ca;
    if (cd_dot(cd_cross(a, p), n) >= 0.0 && cd_dot(cd_cross(p, b), n) >= 0.0) {
        const double pn = cd_dot(p, n);
        const double s2 = __ddiv_rn(__dmul_rn(pn, pn), nn);
        return __ddiv_rn(__dmul_rn(2.0, s2), __dadd_rn(1.0, __dsqrt_rn(__dsub_rn(1.0, s2 < 1.0 ? s2 : 1.0))));
    }
    const double cb = cd_chord2(p, b);
    return ca < cb ? ca : cb;
}

// Bounds on the sphere are Euclidean, in 3-D, with slack:
//   every point of the arc a -> b lies within the sagitta 1 - cos(theta / 2) <= |a - b|^2 / 4 (theta <= pi) of its chord, so inside the
//   hull of a and b grown by that much on every side;
//   sqrt(c2) as computed differs from the true chord to the arc by the rounding of some thirty operations on values <= 2 (below 1e-14)
//   and, where the foot is taken on the arc, by the error of n's direction and of the two sign tests, both below 16 ulp / |n|: a box is
//   grown by CD_NERR / sqrt(nn) as well (nn > 0 only; a value that overflows only keeps the block from being pruned);
//   the comparison itself leaves CD_SLACK.
// A node's box is the hull of the unit vectors of the tile's nodes; gap / far distance of two boxes bound every |p - point| between them.
constexpr double CD_SLACK = 1e-9;
constexpr double CD_NERR = 64.0 * 2.220446049250313e-16;
__device__ __forceinline__ double cd_seg_grow(const CdV& a, const CdV& b, double nn)
{
    double g = __dmul_rn(0.2500000003, cd_chord2(a, b));
    if (nn > 0.0) g = __dadd_rn(g, __ddiv_rn(CD_NERR, __dsqrt_rn(nn)));
    return g;
}

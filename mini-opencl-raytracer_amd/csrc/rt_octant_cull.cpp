// rt_octant_cull.cpp -- the octant-cull certificate (rt_octant_cull.hpp).
//
// The claim.  RayTriangle (kernel_bvh.cl:98-153; tri_eval_v, rt_kernels_body.hpp) rejects a triangle
// when det < 1e-8, with  det = dot(e1, cross(d, e2)).  For a triangle {p1, e1, e2} as the device holds it
// and an octant o (bit k = invDir[k] < 0), bit o of the mask says: for EVERY ray of that octant, every
// evaluation of det the three math policies use is below 1e-8 or NaN.  Below 1e-8: tri_accept's
// `det - 1e-8` is negative and not NaN, the minimum over the reject terms is negative, the test rejects.
// NaN: inv_det, u, v and t are NaN, `h.t - t > 0` is false, nothing is accepted.  Either way the test
// leaves {t, prim, u, v} as they were, for the closest-hit and the any-hit step alike.
//
// The six products.  With pvec = cross(d, e2),
//     det = e1.x (d.y e2.z - d.z e2.y) + e1.y (d.z e2.x - d.x e2.z) + e1.z (d.x e2.y - d.y e2.x)
// is a sum of six triple products p_1..p_6.  Grouped by the direction component they contain,
//     det = d.x c.x + d.y c.y + d.z c.z,   c.k = a.k - b.k,
//     a.x = e1.z e2.y, b.x = e1.y e2.z;  a.y = e1.x e2.z, b.y = e1.z e2.x;  a.z = e1.y e2.x, b.z = e1.x e2.y
// (c = cross(e2, e1): the geometric normal, reversed).
//
// The rule.  Octant o is certified when, with s.k = -1 where bit k of o is set and +1 where it is clear,
// every k satisfies one of
//   (Z) a.k and b.k are both exactly zero (a factor of each is +-0), or
//   (S) s.k c.k < 0  and  |c.k| >= 2^-18 (|a.k| + |b.k|),
// and every vertex coordinate is finite with |coordinate| <= 2^20 (R).  The products of two floats are
// exact in double, where the rule is evaluated; the one rounding of a.k - b.k keeps its sign (an IEEE
// difference of distinct numbers is never zero) and moves the margin by 2^-53, against the factor 8 of
// room below.
//
// Why it holds.
//   The direction.  Every walk's direction is a unit vector, the zero vector or all NaN (normalize's
//   guards, rt_math.hpp; rt_path_kill.cpp argues the same): |d.k| <= 2.  A NaN component makes each of
//   its products NaN (finite e1, e2 by (R): no product is exempt, x * NaN is NaN even for x = 0), and det
//   NaN.  Otherwise invDir.k = rcp(d.k) carries d.k's sign under the three rcp's (IEEE division; the
//   Newton form on its exact range; the shipped frexp/ldexp form), +-inf for +-0 and for denormals that
//   overflow: bit k set means d.k < 0 or d.k = -0, bit k clear means d.k > 0 or d.k = +0.  So
//   s.k d.k >= 0, and under (S) or (Z)  d.k c.k = |d.k| s.k c.k <= 0  for every k:
//       D = d.x c.x + d.y c.y + d.z c.z = -(|d.x| |c.x| + |d.y| |c.y| + |d.z| |c.z|)
//         <= -2^-18 (|p_1| + ... + |p_6|) = -2^-18 S.
//   A +-0 component -- -0 sits in the negative octant, +0 in the positive one -- contributes +-0 products
//   to D and to S alike; with d = 0 both are 0.
//   The roundings.  Each p_i reaches det through two multiplications, the subtraction inside pvec and two
//   additions of the dot product.  The pinned policy rounds all five; the device-library and the shipped
//   policy (cross.x = fma(a.y, b.z, b.y * -a.z), dot = fma(z, z', fma(y, y', x x'))) round fewer; any
//   other association or contraction of the same expression has at most five roundings on a product's
//   way.  By (R) |e1.k|, |e2.k| <= 2^21 and every intermediate stays below 2^45: nothing overflows.
//   Without underflow the computed value is therefore  sum p_i (1 + th_i)  with |th_i| <= (1 + 2^-24)^5 - 1
//   < 2^-21, i.e. at most D + 2^-21 S <= (2^-21 - 2^-18) S <= 0.  This is where a rule that looked at
//   signs alone would fail: the side faces of a box rotated about z have e1 = (ax, ay, 0), e2 = (ax, ay,
//   h); c.z = ay ax - ax ay is 0 in exact arithmetic, but a.z and b.z are not zero, and in fp32
//   the two d.z products reach det through different roundings and need not cancel.  (S) refuses c.z = 0
//   with a.z != 0, so such a triangle is certified in no octant: that is the 12.5 % of tests a sign rule
//   would cull against the 5.4 % this one does.  Skinny triangles under the margin are refused likewise.
//   Underflow.  Each of the at most 11 operations may instead round with an absolute error of 2^-149,
//   which later factors scale by at most 2^21 (1 + 2^-21): the computed value is at most 11 * 2^-128 +
//   the bound above.  Whichever sign rounding gives a tiny det, it is below 2^-124 < 1e-8.
//   (Z) needs no argument of its own -- zero products are zero terms of D and S -- but it is what lets
//   an axis-plane triangle through: there two of the three c.k have a.k = b.k = 0.
//
// What is certified.  A triangle in an axis plane (c along one axis, the other four products exactly
// zero) is certified in the 4 octants whose sign on that axis agrees with c's: Cornell's walls, floor,
// ceiling, light and box tops.  A triangle whose three c.k are all non-zero is certified in the one octant
// opposite to their signs, when the margin holds on every axis; a degenerate one (e1 or e2 zero) in all 8.
#include "rt_octant_cull.hpp"

#include <cmath>

namespace rtp {

namespace {

constexpr float kCoordMax = 0x1p20f;  // (R)
constexpr double kMargin = 0x1p-18;   // (S)

bool coord_ok(const rt_float3& p) {
    return std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z) && std::fabs(p.x) <= kCoordMax &&
           std::fabs(p.y) <= kCoordMax && std::fabs(p.z) <= kCoordMax;
}

}  // namespace

CullEdges octant_cull_edges(const rt_cl_triangle& t) {
    const rt_float3 &p1 = t.v1.position, &p2 = t.v2.position, &p3 = t.v3.position;
    return CullEdges{{p2.x - p1.x, p2.y - p1.y, p2.z - p1.z}, {p3.x - p1.x, p3.y - p1.y, p3.z - p1.z}};
}

uint8_t octant_cull_mask(const rt_cl_triangle& t) {
    if (!coord_ok(t.v1.position) || !coord_ok(t.v2.position) || !coord_ok(t.v3.position)) return 0;
    const CullEdges e = octant_cull_edges(t);
    // per axis k: 0 = (Z), -1 / +1 = the sign of c.k under (S), 2 = refused
    int sign[3];
    for (int k = 0; k < 3; ++k) {
        const int i = (k + 2) % 3, j = (k + 1) % 3;  // a.k = e1.i e2.j, b.k = e1.j e2.i
        const double a = (double)e.e1[i] * e.e2[j], b = (double)e.e1[j] * e.e2[i];
        const double c = a - b;
        if (a == 0.0 && b == 0.0)
            sign[k] = 0;
        else if (c != 0.0 && std::fabs(c) >= kMargin * (std::fabs(a) + std::fabs(b)))
            sign[k] = c < 0.0 ? -1 : 1;
        else
            return 0;
    }
    uint8_t mask = 0;
    for (uint32_t o = 0; o < 8; ++o) {
        bool ok = true;
        for (int k = 0; k < 3; ++k) {
            const int s = ((o >> k) & 1u) ? -1 : 1;
            ok = ok && (sign[k] == 0 || s * sign[k] < 0);
        }
        if (ok) mask |= (uint8_t)(1u << o);
    }
    return mask;
}

uint32_t octant_cull_masks(const rt_cl_triangle* tris, uint32_t n_tris, uint8_t* mask) {
    uint32_t pairs = 0;
    for (uint32_t i = 0; i < n_tris; ++i) {
        mask[i] = octant_cull_mask(tris[i]);
        pairs += (uint32_t)__builtin_popcount(mask[i]);
    }
    return pairs;
}

}  // namespace rtp

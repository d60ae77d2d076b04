// rt_path_kill.cpp -- the path-kill certificate (rt_path_kill.hpp).
//
// The claim.  A path is dead once beta = (+-0, +-0, +-0) after a bounce that goes on (shade_bounce
// returned true).  Render (kernel_bvh.cl:349-384) still walks and shades it; step_body ends it there
// (radiance = max(radiance, 0), as when the bounces run out).  Both give the same bits iff, on every
// later segment of the dead path, (1) every X in  radiance += beta * X  is finite -- then the term is
// +-0, and r + (+-0) == r for every r that is not -0; radiance starts at +0 and +0 + (-0) = +0, so it
// is never -0 -- and (2) beta stays +-0: every factor `mul` it is multiplied by is finite.  A segment
// that ends the path (a miss, or the `pdf <= 0 || pdf != pdf` break) is what the kill does anyway.
//
// What a dead path meets, and the clause that keeps it finite.  Below, "unit" means of length within
// 1e-3 of 1, and P = R + 2^18 with R the largest |root bound|.
//
//   The ray.  Its direction is normalize(wi) (InitRay): by normalize's guards (rt_math.hpp) that is a
//   unit vector, the zero vector or all NaN, never infinite.  With d zero or NaN RayTriangle's det is 0
//   or NaN and no triangle is accepted: the segment misses.
//
//   The origin at a hit.  Every walk starts at the root with isect.t = kMaxDist = 1e5 and reaches a
//   triangle only if the root's RayBounds passes: max(0, near_i) <= min(1e5, far_i) over the axes, NaN
//   slab values skipped (fmax / fmin).  Take an axis with o_i > bmax_i + 2^18 (the other side mirrors
//   it).  Both differences b - o_i are negative and of size >= 2^18 * (1 - 2^-24); |1/d_i| >= 0.99 or
//   infinite.  d_i >= 0: the far value is negative (or -inf), so t1 < 0 <= t0.  d_i < 0: the near value
//   is >= 0.99 * 0.99 * 2^18 > 1e5 >= t1.  o_i infinite: the same signs with infinite values.  Neither
//   product is NaN (no 0 * inf: the differences are not zero) nor underflows.  o_i NaN: tvec is NaN, t
//   is NaN, `t < isect.t` fails.  So a segment that hits has a finite origin with |o_i| <= P.
//
//   The hit.  With |o_i| <= P <= 2^21, vertices of |coordinate| <= 2^20 (clause G1) and a unit d, every
//   product in RayTriangle stays below 2^75, and 1/det <= 1e8: det, u, v, t are finite, so the early
//   returns hold as written -- 0 <= u, v and u + v <= 1 (a NaN u or v would pass them; there is none).
//   t has no lower bound in the reference and a grazing hit's t is noise of size up to 1e8 * |e1| |e2|
//   |tvec|; it is finite all the same, so hit_position is finite, and so is the next origin.  A far
//   origin then misses (above): positions do not compound from segment to segment.
//
//   The normal.  n = normalize(n1 * w + n2 * u + n3 * v), w = (1 - u) - v, weights in [-1e-7, 1] that
//   sum to 1 within rounding.  Clause G2: the three normals are finite with length in [1/2, 2], and
//   either bit-equal -- the sum is n1 * (w + u + v) -- or pairwise of non-negative dot product -- then
//   |sum|^2 >= (w^2 + u^2 + v^2) / 4 >= 1 / 12.  Neither vanishes nor overflows: n is a unit vector.
//
//   Emission (clause M1: every material field finite, |field| <= 2^40): beta * emission * 50 is +-0.
//
//   The diffuse lobe.  wi is a unit vector (onb of a unit n, sinT^2 + c^2 = 1 within rounding).
//   pdf = dot(wi, n) / pi; not positive: the break.  Else mul = (diffuse / pi * dot) / (dot / pi), the
//   quotient of two roundings of dot / pi times |diffuse| -- at most 2 |diffuse| + 1 even when dot is
//   denormal.  Finite.
//
//   The specular lobe, per material one of (clause M2):
//   (a) a2pi = a2m1 = +inf (roughness 0: alpha = 2 / 0 - 2).  D = a2pi / (c^2 * a2m1 + 1)^2 is
//       inf / inf for c != 0, and NaN through 0 * inf or a NaN c otherwise, whatever 1 / (alpha + 1) is;
//       pdf = D * c / ... is NaN: the break.  (Or SampleSpecular's early `return 0` with pdf = 0: the
//       break.)
//   (b) -1.5 <= 1 / (alpha + 1) <= -0.75, 0 <= a2m1 <= 2^20, 0 <= a2pi <= 2^20 (Cornell: -1.0002, 3, 1.27).
//       r is k / 2^32 in [0, 1].  r > 0: c = pow(r, 1 / (alpha + 1)) lies in [0.99, 2^48 * 1.01] under any
//       pow that is accurate to 1 %; sinT = sqrt(max(0, 1 - c^2)) <= 0.15; wh = normalize(n * c + ...)
//       is a unit vector, wi its reflection of the unit wo, of wo's length.  (c^2 * a2m1 + 1) >= 1, so D
//       is in [0, a2pi] (0 when the square overflows: pdf = 0, the break).  pdf = D * c / (4 * m), m =
//       max(dot(wo, wh), 0) <= 1.01.  m = 0: pdf is +inf or 0 / 0 -- NaN breaks, and f * dot / inf = +-0
//       for the finite f * dot.  m > 0: pdf >= D * c / 4.04 while f * dot(wi, n) <= |specular| * D / 0.001
//       * 1.01 (denom >= 0.001), so |mul| <= 4200 |specular| / c; with D or pdf denormal the quotient of the
//       two roundings is at most twice that.  Finite.
//       r = 0: c = +inf, sinT = sqrt(max(0, -inf)) = 0, n * c holds inf or 0 * inf: wh and wi are NaN
//       and `dot(wi, n) * dot(wo, n) < 1e-6` is false.  a2m1 = 0: c^2 * a2m1 = NaN, D = NaN.  a2m1 > 0:
//       D = a2pi / inf = 0 and D * c = 0 * inf = NaN.  Either way pdf is NaN although its denominator is
//       4 * max(NaN, 0) = 0: the break.  (A pow that returns a finite value at 0 falls under r > 0.)
//   A NaN wi otherwise never arises on a dead path (n, wo and c are finite), which matters: with a
//   finite D it would leave pdf = D * c / (4 * max(NaN, 0)) = +inf and go on with mul = NaN.
//
//   The light (launch clause L1: lightType <= 0).  LightPixel is max(dot(n, -lightDirection), 0) for a
//   unit n: finite, times the finite diffuse.  Type 1's 1 / (0.8 d^2) can be infinite.  Types >= 2 read
//   the hit position, which is finite but may be of size 2^100 after a grazing hit, where dot(n, L)
//   overflows: refused as well (sufficient, not necessary).
//
//   The sky (L2: skyboxIntensity finite): a miss adds beta * (0.5 * sky) = +-0.
//
//   L3: lightBounces > 1 -- with one bounce no path goes on after its first shading.
#include "rt_path_kill.hpp"

#include <cmath>
#include <cstring>

namespace rtp {

namespace {

constexpr float kFieldMax = 0x1p40f;   // M1
constexpr float kCoordMax = 0x1p20f;   // G1
constexpr float kGgxMax = 0x1p20f;     // M2 (b)

bool fin_le(float x, float lim) { return std::isfinite(x) && std::fabs(x) <= lim; }

bool refuse(const char** why, const char* clause) {
    if (why) *why = clause;
    return false;
}

bool normal_ok(const rt_float3& n) {
    if (!std::isfinite(n.x) || !std::isfinite(n.y) || !std::isfinite(n.z)) return false;
    const double l2 = (double)n.x * n.x + (double)n.y * n.y + (double)n.z * n.z;
    return l2 >= 0.25 && l2 <= 4.0;
}
double dot3(const rt_float3& a, const rt_float3& b) {
    return (double)a.x * b.x + (double)a.y * b.y + (double)a.z * b.z;
}
bool same_bits(const rt_float3& a, const rt_float3& b) { return std::memcmp(&a, &b, 3 * sizeof(float)) == 0; }

}  // namespace

bool path_kill_scene_ok(const float* mats, uint32_t n_mats, const rt_cl_triangle* tris, uint32_t n_tris,
                        const float* root, const char** why) {
    if (why) *why = "";
    if (!mats || !tris || n_mats == 0 || n_tris == 0) return refuse(why, "no scene");
    // the root bounds as the walk sees them; unknown after a device refit
    if (!root) return refuse(why, "root bounds unknown");
    for (int i = 0; i < 6; ++i)
        if (!fin_le(root[i], kCoordMax)) return refuse(why, "root bounds");
    for (uint32_t m = 0; m < n_mats; ++m) {
        const float* r = mats + 16 * (size_t)m;
        // M1: diffuse, specular, emission
        for (int q = 0; q < 3; ++q)
            for (int c = 0; c < 3; ++c)
                if (!fin_le(r[4 * q + c], kFieldMax)) return refuse(why, "material field");
        const float inv_a1 = r[3], a2pi = r[7], a2m1 = r[11];
        // M2 (a): every specular sample breaks
        const bool always_breaks = std::isinf(a2pi) && a2pi > 0.0f && std::isinf(a2m1) && a2m1 > 0.0f;
        // M2 (b): D, D / denom and f * dot / pdf are finite for every r
        const bool finite_lobe = inv_a1 >= -1.5f && inv_a1 <= -0.75f && a2m1 >= 0.0f && a2m1 <= kGgxMax &&
                                 a2pi >= 0.0f && a2pi <= kGgxMax;
        if (!always_breaks && !finite_lobe) return refuse(why, "specular lobe");
    }
    for (uint32_t t = 0; t < n_tris; ++t) {
        const rt_cl_triangle& tr = tris[t];
        const rt_cl_vertex* v[3] = {&tr.v1, &tr.v2, &tr.v3};
        for (int i = 0; i < 3; ++i) {
            // G1
            if (!fin_le(v[i]->position.x, kCoordMax) || !fin_le(v[i]->position.y, kCoordMax) ||
                !fin_le(v[i]->position.z, kCoordMax))
                return refuse(why, "vertex");
            // G2
            if (!normal_ok(v[i]->normal)) return refuse(why, "normal length");
        }
        const rt_float3 &n1 = tr.v1.normal, &n2 = tr.v2.normal, &n3 = tr.v3.normal;
        const bool equal = same_bits(n1, n2) && same_bits(n1, n3);
        if (!equal && !(dot3(n1, n2) >= 0.0 && dot3(n1, n3) >= 0.0 && dot3(n2, n3) >= 0.0))
            return refuse(why, "opposed normals");
    }
    return true;
}

}  // namespace rtp

// rt_view_cull.cpp -- the view-cull rule (rt_view_cull.hpp).  Pure arithmetic in double, kept where a
// CPU test can sweep it against the kernel's own fp32 camera ray and box test (tests/test_view_cull.py).
//
// The argument.  CreateRay (kernel_bvh.cl:386-403) sends the sample (px + jx, py + jy), jx, jy in
// [0, 1] -- a point of the pixel's closed square -- along  dir = x * R + y * U + F,  R = cross(F, U),
//     x = (2 * (px + jx) / W - 1) * angle * aspect,   y = (2 * (py + jy) / H - 1) * angle
// (its  -(1 - 2 * ...)  is that sign; row 0 is y = -angle).  A point c in front of the camera is
//     c - pos = w * (xc * R + yc * U + F),  w > 0,
// and a ray meets it only if (x, y) = (xc, yc).  A point of a convex box is a convex combination of
// its 8 corners c_i; with every w_i > 0 its (xc, yc) is a combination of the corners' (x_i, y_i) with
// positive weights, so it lies in their convex hull, hence in their bounding rectangle.  A sample
// outside that rectangle cannot meet the box; a tile none of whose pixels' squares touches the
// rectangle is culled.  When a corner has w <= 0 (the camera inside, beside or behind part of the box)
// the cone over the corners is not bounded by the rectangle and the rule answers "all".
//
// The margins.  The kernel does this in fp32, so the rule decides for a larger box and a larger rectangle:
//   * the box grows by kBoxMargin * scale on every side, scale = the largest |c_i - pos| component.
//     The slab test (oct_step) forms t = (b - o) * rcp(d): two roundings and a reciprocal of at most
//     2.5 ulp (the shipped policy), under 5 ulp = 6e-7 relative in t, which is the same as moving the
//     plane b by 6e-7 * |b - o| <= 6e-7 * scale.  kBoxMargin = 2^-10 is 1600 times that.
//   * the rectangle grows by kPixelMargin = 2 pixels.  camera_dir, normalize and ray_from_unit put
//     under 8 ulp = 1e-6 relative on a direction component of size <= ~1.3, against a pixel pitch of
//     2 * angle / H in y (the same in x): 1.6e-6 * H pixels, 0.1 pixel at the 65536 rows the rule
//     accepts; (float)px + j rounds by at most 2^-8 pixel below 65536 columns, and the double
//     evaluation of angle and aspect differs from the fp32 one by 1e-7 relative, 0.007 pixel.  Two
//     pixels are 15 times the sum.
// At 4K the two margins together cost about one tile ring (under 2 % of the visible tiles).
#include "rt_view_cull.hpp"

#include <cmath>

namespace rtp {

namespace {

constexpr double kBoxMargin = 1.0 / 1024.0;
constexpr double kPixelMargin = 2.0;
constexpr uint32_t kMaxSide = 65536;   // image sides the pixel margin was derived for
constexpr double kMinDepthRatio = 1e-6;  // a corner this close to the camera plane counts as behind it

void cross3(const double a[3], const double b[3], double out[3]) {
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}
double dot3(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

}  // namespace

ViewRect view_cull_rect(uint32_t W, uint32_t H, const float pos[3], const float front[3], const float up[3],
                        const float bmin[3], const float bmax[3]) {
    const ViewRect all{};
    if (W == 0 || H == 0 || W > kMaxSide || H > kMaxSide) return all;
    double P[3], F[3], U[3], lo[3], hi[3];
    for (int i = 0; i < 3; ++i) {
        P[i] = pos[i], F[i] = front[i], U[i] = up[i], lo[i] = bmin[i], hi[i] = bmax[i];
        if (!std::isfinite(P[i]) || !std::isfinite(F[i]) || !std::isfinite(U[i]) || !std::isfinite(lo[i]) ||
            !std::isfinite(hi[i]) || !(lo[i] <= hi[i]))
            return all;
    }
    double R[3];
    cross3(F, U, R);
    // det(R, U, F) = R . cross(U, F) = -|R|^2: near zero when front and up are (nearly) parallel
    double UxF[3], FxR[3], RxU[3];
    cross3(U, F, UxF);
    cross3(F, R, FxR);
    cross3(R, U, RxU);
    const double det = dot3(R, UxF);
    const double lenR = std::sqrt(dot3(R, R)), lenU = std::sqrt(dot3(U, U)), lenF = std::sqrt(dot3(F, F));
    if (!std::isfinite(det) || !(std::fabs(det) > 1e-9 * lenR * lenU * lenF)) return all;

    double scale = 0.0;
    for (int i = 0; i < 3; ++i) scale = std::fmax(scale, std::fmax(std::fabs(lo[i] - P[i]), std::fabs(hi[i] - P[i])));
    const double grow = kBoxMargin * scale;
    const double angle = std::tan(0.5 * (45.0 * 3.1415 / 180.0));  // kernel_bvh.cl:392
    const double aspect = (double)W / (double)H;

    double x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY, wmin = INFINITY, wmax = 0.0;
    for (int c = 0; c < 8; ++c) {
        double v[3];
        for (int i = 0; i < 3; ++i) v[i] = ((c >> i) & 1 ? hi[i] + grow : lo[i] - grow) - P[i];
        // Cramer: v = a * R + b * U + w * F
        const double a = dot3(v, UxF) / det, b = dot3(v, FxR) / det, w = dot3(v, RxU) / det;
        if (!std::isfinite(a) || !std::isfinite(b) || !std::isfinite(w) || !(w > 0.0)) return all;
        wmin = std::fmin(wmin, w), wmax = std::fmax(wmax, w);
        // the inverse of camera_dir's pixel mapping: sample coordinates in pixels
        const double sx = (a / w / (angle * aspect) + 1.0) * 0.5 * (double)W;
        const double sy = (b / w / angle + 1.0) * 0.5 * (double)H;
        if (!std::isfinite(sx) || !std::isfinite(sy)) return all;
        x0 = std::fmin(x0, sx), x1 = std::fmax(x1, sx);
        y0 = std::fmin(y0, sy), y1 = std::fmax(y1, sy);
    }
    if (!(wmin > kMinDepthRatio * wmax)) return all;
    // pixel px can hold a sample in [px, px + 1]: it is kept when that meets [x0 - m, x1 + m]
    const double fx0 = std::floor(x0 - kPixelMargin - 1.0), fx1 = std::floor(x1 + kPixelMargin) + 1.0;
    const double fy0 = std::floor(y0 - kPixelMargin - 1.0), fy1 = std::floor(y1 + kPixelMargin) + 1.0;
    const double px0 = std::fmax(fx0, 0.0), px1 = std::fmin(fx1, (double)W);
    const double py0 = std::fmax(fy0, 0.0), py1 = std::fmin(fy1, (double)H);
    if (!(px0 < px1) || !(py0 < py1)) return all;  // the box is off-screen: nothing to anchor a rectangle
    ViewRect r;
    r.tx0 = (uint32_t)px0 / 8u, r.tx1 = ((uint32_t)px1 + 7u) / 8u;
    r.ty0 = (uint32_t)py0 / 8u, r.ty1 = ((uint32_t)py1 + 7u) / 8u;
    return r;
}

}  // namespace rtp

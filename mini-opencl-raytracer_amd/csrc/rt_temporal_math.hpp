// rt_temporal_math.hpp -- steps 2-4 of rtEnqueueTemporalAccumulate's definition (include/rt_hip.h):
// the world point of a pixel, its projection into the previous view, the range test and the tap
// indices; and step 5's surface test of a tap, which rtEnqueueReprojectSamples shares.  Step 2 (the point)
// and step 3 (project_point) are separate, because the motion variants take the point from a motion record
// and rtEnqueueFrameMotion takes step 2's direction as its ray.  This is where a value read from a buffer (a
// depth, a previous point) ends up deciding an address, so the
// kernel (rt_temporal.hip) and a CPU program (tests/native/temporal_plan_main.cpp, built with
// sanitizers) compile this same text: the address logic is swept on the CPU over every class of
// bit pattern before a GPU runs it.
//
// The rules that make it safe: comparisons are written so that a NaN fails them; a float becomes an
// integer only after the range test has placed it in [-1, W) (W <= 2^31); a tap's index is formed
// only after its integer coordinates were tested against the image.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_TM_FN __host__ __device__ inline
#else
#define RT_TM_FN inline
#endif

namespace rtt {

// the host constants of the definition (rtp::temporal_plan computes them, in fp32) and both cameras
struct TemporalConsts {
    float A;                       // 0x1.a82408p-2f
    float invW, invH, asp, ia, ib;
    float fW, fH;                  // (float)W, (float)H
    float cpos[3], cfront[3], cup[3], cright[3];  // the current view; right = cross(front, up)
    float ppos[3], pfront[3], pup[3], pright[3];  // the previous view
};

constexpr float kTanHalfFov = 0x1.a82408p-2f;

RT_TM_FN float dot3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

RT_TM_FN void cross3(const float* a, const float* b, float* out) {
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

struct Reprojection {
    bool ok;        // steps 3 and 4 passed: x0, y0, tx, ty are set
    int32_t x0, y0;  // in [-1, W - 1] and [-1, H - 1]
    float tx, ty;
    float de;       // the point's distance from the previous camera
};

struct Projection {
    float zf;       // the point's distance along the previous view's front; fx and fy mean something only when zf > 0
    float fx, fy;   // its pixel coordinates in the previous view
    float de;       // its distance from the previous camera
};

// Step 2's direction d of pixel (x, y)'s centre ray in the current view, not normalised (additions and
// products only: the same in a translation unit with relaxed division; rtEnqueueFrameMotion's ray).
RT_TM_FN void centre_dir(const TemporalConsts& k, uint32_t x, uint32_t y, float* d) {
    const float sx = ((2.0f * (((float)x + 0.5f) * k.invW) - 1.0f) * k.A) * k.asp;
    const float sy = (2.0f * (((float)y + 0.5f) * k.invH) - 1.0f) * k.A;
    for (int c = 0; c < 3; ++c) d[c] = (k.cright[c] * sx + k.cup[c] * sy) + k.cfront[c];
}

// Step 2: the world point of pixel (x, y) at the current view's depth.
RT_TM_FN void world_point(const TemporalConsts& k, uint32_t x, uint32_t y, float depth, float* X) {
    float d[3];
    centre_dir(k, x, y, d);
    const float rl = 1.0f / sqrtf(dot3(d, d));
    for (int c = 0; c < 3; ++c) X[c] = k.cpos[c] + (d[c] * rl) * depth;
}

// Step 3 for the world point X: floating point only, any bit pattern.
RT_TM_FN Projection project_point(const TemporalConsts& k, const float* X) {
    float v[3];
    for (int c = 0; c < 3; ++c) v[c] = X[c] - k.ppos[c];
    Projection p;
    p.zf = dot3(v, k.pfront);
    const float a = dot3(v, k.pright) / p.zf, b = dot3(v, k.pup) / p.zf;
    p.fx = ((a * k.ia + 1.0f) * 0.5f) * k.fW - 0.5f;
    p.fy = ((b * k.ib + 1.0f) * 0.5f) * k.fH - 0.5f;
    p.de = sqrtf(dot3(v, v));
    return p;
}

// Steps 2 and 3 for pixel (x, y) with the current view's depth.
RT_TM_FN Projection project(const TemporalConsts& k, uint32_t x, uint32_t y, float depth) {
    float X[3];
    world_point(k, x, y, depth, X);
    return project_point(k, X);
}

// Step 4 on a projection.  Defined for every bit pattern in `p`.
RT_TM_FN Reprojection in_range(const TemporalConsts& k, const Projection& p) {
    Reprojection r;
    r.ok = false, r.x0 = 0, r.y0 = 0, r.tx = 0.0f, r.ty = 0.0f, r.de = p.de;
    if (!(p.zf > 0.0f)) return r;
    // 4: the range, before anything becomes an integer
    if (!(p.fx > -1.0f && p.fx < k.fW && p.fy > -1.0f && p.fy < k.fH)) return r;
    const float x0f = floorf(p.fx), y0f = floorf(p.fy);
    r.tx = p.fx - x0f, r.ty = p.fy - y0f;
    r.x0 = (int32_t)x0f, r.y0 = (int32_t)y0f;
    r.ok = true;
    return r;
}

// Steps 2-4.  Defined for every bit pattern of `depth`.
RT_TM_FN Reprojection reproject(const TemporalConsts& k, uint32_t x, uint32_t y, float depth) {
    return in_range(k, project(k, x, y, depth));
}

// Steps 3 and 4 of the motion variants, whose step 2 is X = motion[p].prev_point.  Defined for every bit
// pattern of X.
RT_TM_FN Reprojection reproject_point(const TemporalConsts& k, const float* X) {
    return in_range(k, project_point(k, X));
}

// Tap (i, j) of a reprojection that passed: true and its record index when it lies inside the W x H
// image.  (float)W may round above W, so x0 + i is tested against W itself.
RT_TM_FN bool tap_index(const Reprojection& r, int i, int j, uint32_t W, uint32_t H, uint64_t* index) {
    const int64_t qx = (int64_t)r.x0 + i, qy = (int64_t)r.y0 + j;
    if (!r.ok || qx < 0 || qx >= (int64_t)W || qy < 0 || qy >= (int64_t)H) return false;
    *index = (uint64_t)qy * W + (uint64_t)qx;
    return true;
}

RT_TM_FN float tap_weight(const Reprojection& r, int i, int j) {
    return (i ? r.tx : 1.0f - r.tx) * (j ? r.ty : 1.0f - r.ty);
}

// The part of a history tap's test that needs its features only: q inside the image, covered, on the
// centre's surface.  `tol` is depth_tolerance * de.  False for a NaN anywhere.  (The sample reprojection
// need not fetch the statistics of a tap that fails here.)
RT_TM_FN bool tap_on_surface(bool inside, float coverage, float depth, const float* normal, const float* centre_normal,
                             float de, float tol, float normal_threshold) {
    return inside && coverage > 0.0f && fabsf(depth - de) <= tol && dot3(centre_normal, normal) >= normal_threshold;
}

}  // namespace rtt

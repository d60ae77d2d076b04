// rt_temporal.hpp -- the temporal-reprojection kernel (rt_temporal.hip), launched by
// rtEnqueueTemporalAccumulate (rt_capi.cpp) from rtp::temporal_plan (rt_temporal_plan.hpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_temporal_plan.hpp"

namespace rtt {

struct TemporalArgs {
    const float4* cur;            // {r, g, b, w}: width * height slots
    const float4* cur_features;   // rt_pixel_features as two float4 per pixel: {albedo, depth}, {normal, coverage}
    const float4* hist;           // the previous output; nullptr (with hist_features): no history
    const float4* hist_features;
    float4* out;                  // never one of the inputs
    uint32_t width, height, tilesX;
    float cur_frames, history_frames, max_history, depth_tolerance, normal_threshold;
    TemporalConsts k;
};

// ---- how the two reprojection kernels (rt_temporal.hip, rt_reproject.hip) open ----
constexpr int kTileW = (int)rtp::kTemporalTileW, kTileH = (int)rtp::kTemporalTileH;
constexpr int kThreads = (int)rtp::kTemporalThreads;

// The thread's pixel in tile blockIdx.x of the plan: a wave per row, a lane per column.  It may lie
// outside the image.
struct Pixel {
    uint64_t x, y;
};
__device__ __forceinline__ Pixel tile_pixel(uint32_t tilesX) {
    const uint32_t tx = blockIdx.x % tilesX, ty = blockIdx.x / tilesX;
    return Pixel{(uint64_t)tx * kTileW + (threadIdx.x & (kTileW - 1)), (uint64_t)ty * kTileH + (threadIdx.x / kTileW)};
}

// What a history tap is tested against: the pixel's reprojection `r`, which passes only for a covered
// centre (fn is its {normal, coverage}), the centre's normal and the depth tolerance at its distance.
struct Centre {
    Reprojection r;
    float nrm[3], tol;
};
__device__ __forceinline__ Centre centre_of(Reprojection r, float4 fn, float depth_tolerance) {
    r.ok = r.ok && fn.w > 0.0f;
    return Centre{r, {fn.x, fn.y, fn.z}, depth_tolerance * r.de};
}
// The motion variants' centre: the point is the record's prev_point (any bit pattern), a record without
// a hit (prim < 0) has no history, and the taps are tested against the record's prev_normal.  `coverage`
// is the current features'.
__device__ __forceinline__ Centre centre_of_motion(const TemporalConsts& k, float4 m0, float4 m1, float coverage,
                                                   float depth_tolerance) {
    const float X[3] = {m0.x, m0.y, m0.z};
    Reprojection r = reproject_point(k, X);
    r.ok = r.ok && coverage > 0.0f && __float_as_int(m0.w) >= 0;
    return Centre{r, {m1.x, m1.y, m1.z}, depth_tolerance * r.de};
}

// One launch over p.grid workgroups on `st`.  hipErrorInvalidValue for a plan that does not match
// the arguments: nothing is launched.
// `motion` (rt_pixel_motion as two float4 per pixel: {prev_point, prim}, {prev_normal, flags}) is non-null
// exactly when the plan has motion; it is a kernel argument of its own, so the plain kernels keep theirs.
hipError_t launch_temporal(const TemporalArgs& a, const float4* motion, const rtp::TemporalPlan& p, hipStream_t st);

}  // namespace rtt

// rt_reproject.hpp -- the kernel that reprojects the adaptive sample statistics (rt_reproject.hip),
// launched by rtEnqueueReprojectSamples (rt_capi.cpp) from rtp::reproject_plan (rt_reproject_plan.hpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_reproject_plan.hpp"

namespace rtrs {

struct ReprojectArgs {
    const float4* hist_stats;     // rt_pixel_stats as two float4 per pixel: {sum, n}, {mean_y, m2_y, reserved}
    const float4* hist_features;  // rt_pixel_features as two float4 per pixel: {albedo, depth}, {normal, coverage}
    const float4* cur_features;
    float4* out_stats;            // never one of the inputs
    uint32_t width, height, tilesX;
    float max_history, depth_tolerance, normal_threshold;
    rtt::TemporalConsts k;
};

// One launch over p.grid workgroups on `st`.  hipErrorInvalidValue for a plan that does not match
// the arguments: nothing is launched.
// `motion` (rt_pixel_motion as two float4 per pixel) is non-null exactly when the plan has motion; it is a
// kernel argument of its own, so the plain kernel keeps its arguments.
hipError_t launch_reproject(const ReprojectArgs& a, const float4* motion, const rtp::ReprojectPlan& p, hipStream_t st);

}  // namespace rtrs

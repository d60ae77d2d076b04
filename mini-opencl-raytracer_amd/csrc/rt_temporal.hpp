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

// One launch over p.grid workgroups on `st`.  hipErrorInvalidValue for a plan that does not match
// the arguments: nothing is launched.
hipError_t launch_temporal(const TemporalArgs& a, const rtp::TemporalPlan& p, hipStream_t st);

}  // namespace rtt

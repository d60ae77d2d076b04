// rt_reproject_plan.hpp -- how one reprojection of the adaptive sample statistics
// (rtEnqueueReprojectSamples) is launched, as a pure function of plain values (rt_reproject_plan.cpp): no
// HIP, no allocation, no globals.  The C ABI fills a ReprojectIn, calls reproject_plan and launches one
// kernel (rt_reproject.hip) with the plan's constants and grid.
//
// The constants and the grid are the temporal pass's (rt_temporal_plan.hpp): the same fp32 host
// constants from the same routine, and workgroup b of the 1-D grid is tile (b % tiles_x, b / tiles_x)
// of kTemporalTileW contiguous columns (one wave's lanes) by kTemporalTileH rows (one wave each).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "rt_reproject_math.hpp"
#include "rt_temporal_plan.hpp"

namespace rtp {

constexpr uint32_t kReprojectStatsBytes = 32, kReprojectFeatureBytes = 32;

struct ReprojectIn {
    bool params_ok;                 // params != NULL
    uint64_t width, height;
    TemporalView cur, prev;
    float max_history, depth_tolerance, normal_threshold;
    bool hist_stats_ok, hist_features_ok, cur_features_ok, out_ok;  // each a buffer of this context
    bool out_is_input;                                              // `out_stats` is one of the three inputs
    uint64_t hist_stats_bytes, hist_features_bytes, cur_features_bytes, out_bytes;
    // rtEnqueueReprojectSamplesMotion (all false / zero: rtEnqueueReprojectSamples itself)
    bool motion_given, motion_ok;   // the handle is not NULL; a buffer of this context
    uint64_t motion_bytes;
};

struct ReprojectPlan {
    uint32_t width, height;
    bool has_motion;                // step 2 is motion[p].prev_point (rt_pixel_motion records)
    rtt::TemporalConsts k;
    float max_history, depth_tolerance, normal_threshold;
    uint32_t tiles_x, tiles_y;
    uint32_t grid;                  // workgroups of kTemporalThreads
};

// RT_SUCCESS, or, in this order: RT_INVALID_VALUE (no params; width or height zero; width * height >
// 2^31; a camera component not finite; max_history not finite, not an integer value, < 1 or > 2^20;
// depth_tolerance not finite or outside [0, 1]; normal_threshold not finite or outside [-1, 1]),
// RT_INVALID_MEM_OBJECT (a buffer that is not this context's; `out_stats` one of the inputs, `motion` among
// them), RT_INVALID_BUFFER_SIZE (any buffer below 32 B per pixel).
int reproject_plan(const ReprojectIn& in, ReprojectPlan* out);

}  // namespace rtp

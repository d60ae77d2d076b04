// rt_reproject_plan.cpp -- the plan of one reprojection of the sample statistics
// (rt_reproject_plan.hpp): the argument checks in their documented order, then the temporal plan's
// view_consts and temporal_tiles for the fp32 host constants of the definition (include/rt_hip.h) and the
// grid.  Pure arithmetic, kept where a CPU test can sweep it (tests/native/reproject_samples_plan_main.cpp).
#include "rt_reproject_plan.hpp"

#include <cmath>

#include "../../include/rt_status.h"

namespace rtp {

int reproject_plan(const ReprojectIn& in, ReprojectPlan* out) {
    *out = ReprojectPlan{};
    ReprojectPlan& p = *out;
    if (!in.params_ok) return RT_INVALID_VALUE;
    if (!image_size_ok(in.width, in.height)) return RT_INVALID_VALUE;
    if (!view_finite(in.cur) || !view_finite(in.prev)) return RT_INVALID_VALUE;
    if (!(finite_in(in.max_history, 1.0f, rtrs::kReprojectMaxHistory) && std::floor(in.max_history) == in.max_history))
        return RT_INVALID_VALUE;
    if (!finite_in(in.depth_tolerance, 0.0f, 1.0f) || !finite_in(in.normal_threshold, -1.0f, 1.0f)) return RT_INVALID_VALUE;

    if (!in.hist_stats_ok || !in.hist_features_ok || !in.cur_features_ok || !in.out_ok) return RT_INVALID_MEM_OBJECT;
    if (in.motion_given && !in.motion_ok) return RT_INVALID_MEM_OBJECT;
    if (in.out_is_input) return RT_INVALID_MEM_OBJECT;

    const uint64_t pixels = in.width * in.height;
    if (pixels > in.hist_stats_bytes / kReprojectStatsBytes || pixels > in.hist_features_bytes / kReprojectFeatureBytes ||
        pixels > in.cur_features_bytes / kReprojectFeatureBytes || pixels > in.out_bytes / kReprojectStatsBytes)
        return RT_INVALID_BUFFER_SIZE;
    if (in.motion_given && pixels > in.motion_bytes / kTemporalMotionBytes) return RT_INVALID_BUFFER_SIZE;

    p.has_motion = in.motion_given;
    p.width = (uint32_t)in.width, p.height = (uint32_t)in.height;
    p.k = view_consts(in.width, in.height, in.cur, in.prev);
    p.max_history = in.max_history, p.depth_tolerance = in.depth_tolerance, p.normal_threshold = in.normal_threshold;
    temporal_tiles(in.width, in.height, &p.tiles_x, &p.tiles_y, &p.grid);
    return RT_SUCCESS;
}

}  // namespace rtp

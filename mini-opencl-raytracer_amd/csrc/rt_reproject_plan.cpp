// rt_reproject_plan.cpp -- the plan of one reprojection of the sample statistics
// (rt_reproject_plan.hpp): the argument checks in their documented order, then the temporal plan's own
// routine for the fp32 host constants of the definition (include/rt_hip.h) and the grid.  Pure
// arithmetic, kept where a CPU test can sweep it (tests/native/reproject_samples_plan_main.cpp).
#include "rt_reproject_plan.hpp"

#include <cmath>

#include "../../include/rt_status.h"

namespace rtp {

namespace {

bool view_finite(const TemporalView& v) {
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(v.pos[c]) || !std::isfinite(v.front[c]) || !std::isfinite(v.up[c])) return false;
    return true;
}

}  // namespace

int reproject_plan(const ReprojectIn& in, ReprojectPlan* out) {
    *out = ReprojectPlan{};
    ReprojectPlan& p = *out;
    if (!in.params_ok) return RT_INVALID_VALUE;
    if (in.width == 0 || in.height == 0) return RT_INVALID_VALUE;
    // (each factor first: their product cannot wrap)
    if (in.width > kTemporalMaxPixels || in.height > kTemporalMaxPixels || in.width * in.height > kTemporalMaxPixels)
        return RT_INVALID_VALUE;
    if (!view_finite(in.cur) || !view_finite(in.prev)) return RT_INVALID_VALUE;
    // (every comparison is false for a NaN, so the finite test comes first)
    if (!(std::isfinite(in.max_history) && in.max_history >= 1.0f && in.max_history <= rtrs::kReprojectMaxHistory &&
          std::floor(in.max_history) == in.max_history))
        return RT_INVALID_VALUE;
    if (!(std::isfinite(in.depth_tolerance) && in.depth_tolerance >= 0.0f && in.depth_tolerance <= 1.0f))
        return RT_INVALID_VALUE;
    if (!(std::isfinite(in.normal_threshold) && in.normal_threshold >= -1.0f && in.normal_threshold <= 1.0f))
        return RT_INVALID_VALUE;

    if (!in.hist_stats_ok || !in.hist_features_ok || !in.cur_features_ok || !in.out_ok) return RT_INVALID_MEM_OBJECT;
    if (in.out_is_input) return RT_INVALID_MEM_OBJECT;

    const uint64_t pixels = in.width * in.height;
    if (pixels > in.hist_stats_bytes / kReprojectStatsBytes || pixels > in.hist_features_bytes / kReprojectFeatureBytes ||
        pixels > in.cur_features_bytes / kReprojectFeatureBytes || pixels > in.out_bytes / kReprojectStatsBytes)
        return RT_INVALID_BUFFER_SIZE;

    // The constants and the grid: temporal_plan as it is, on a call without history of one frame whose
    // buffers are exactly large enough.  Everything it checks was checked above, so it cannot refuse.
    TemporalIn t{};
    t.params_ok = true;
    t.width = in.width, t.height = in.height;
    t.cur = in.cur, t.prev = in.prev;
    t.cur_frames = 1.0f, t.history_frames = 0.0f, t.max_history = 1.0f;
    t.depth_tolerance = in.depth_tolerance, t.normal_threshold = in.normal_threshold;
    t.cur_ok = t.cur_features_ok = t.out_ok = true;
    t.cur_bytes = t.out_bytes = pixels * kTemporalPixelBytes;
    t.cur_features_bytes = pixels * kTemporalFeatureBytes;
    TemporalPlan tp;
    const int rc = temporal_plan(t, &tp);
    if (rc != RT_SUCCESS) return rc;

    p.width = tp.width, p.height = tp.height;
    p.k = tp.k;
    p.max_history = in.max_history, p.depth_tolerance = in.depth_tolerance, p.normal_threshold = in.normal_threshold;
    p.tiles_x = tp.tiles_x, p.tiles_y = tp.tiles_y, p.grid = tp.grid;
    return RT_SUCCESS;
}

}  // namespace rtp

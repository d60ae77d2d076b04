// rt_temporal_plan.cpp -- the plan of one temporal reprojection (rt_temporal_plan.hpp): the argument
// checks in their documented order, the fp32 host constants of the definition (include/rt_hip.h) and
// the grid.  Pure arithmetic, kept where a CPU test can sweep it (tests/native/temporal_plan_main.cpp).
#include "rt_temporal_plan.hpp"

#include <cmath>

#include "../../include/rt_status.h"

namespace rtp {

namespace {

bool view_finite(const TemporalView& v) {
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(v.pos[c]) || !std::isfinite(v.front[c]) || !std::isfinite(v.up[c])) return false;
    return true;
}

// (every comparison is false for a NaN, so the finite test comes first)
bool frames_ok(float f) { return std::isfinite(f) && f >= 1.0f && f <= kTemporalMaxFrames; }

}  // namespace

int temporal_plan(const TemporalIn& in, TemporalPlan* out) {
    *out = TemporalPlan{};
    TemporalPlan& p = *out;
    if (!in.params_ok) return RT_INVALID_VALUE;
    if (in.width == 0 || in.height == 0) return RT_INVALID_VALUE;
    // (each factor first: their product cannot wrap)
    if (in.width > kTemporalMaxPixels || in.height > kTemporalMaxPixels || in.width * in.height > kTemporalMaxPixels)
        return RT_INVALID_VALUE;
    if (!view_finite(in.cur) || !view_finite(in.prev)) return RT_INVALID_VALUE;
    if (!frames_ok(in.cur_frames)) return RT_INVALID_VALUE;
    if (!(in.history_frames == 0.0f || frames_ok(in.history_frames))) return RT_INVALID_VALUE;
    if (!frames_ok(in.max_history) || in.max_history < in.cur_frames) return RT_INVALID_VALUE;
    if (!(std::isfinite(in.depth_tolerance) && in.depth_tolerance >= 0.0f && in.depth_tolerance <= 1.0f))
        return RT_INVALID_VALUE;
    if (!(std::isfinite(in.normal_threshold) && in.normal_threshold >= -1.0f && in.normal_threshold <= 1.0f))
        return RT_INVALID_VALUE;

    if (in.hist_given != in.hist_features_given) return RT_INVALID_MEM_OBJECT;
    if (!in.cur_ok || !in.cur_features_ok || !in.out_ok) return RT_INVALID_MEM_OBJECT;
    if (in.hist_given && (!in.hist_ok || !in.hist_features_ok)) return RT_INVALID_MEM_OBJECT;
    if (in.out_is_input) return RT_INVALID_MEM_OBJECT;

    const uint64_t pixels = in.width * in.height;
    if (pixels > in.cur_bytes / kTemporalPixelBytes || pixels > in.cur_features_bytes / kTemporalFeatureBytes ||
        pixels > in.out_bytes / kTemporalPixelBytes)
        return RT_INVALID_BUFFER_SIZE;
    if (in.hist_given &&
        (pixels > in.hist_bytes / kTemporalPixelBytes || pixels > in.hist_features_bytes / kTemporalFeatureBytes))
        return RT_INVALID_BUFFER_SIZE;

    p.width = (uint32_t)in.width, p.height = (uint32_t)in.height;
    p.has_history = in.hist_given;
    rtt::TemporalConsts& k = p.k;
    k.A = rtt::kTanHalfFov;
    k.fW = (float)in.width, k.fH = (float)in.height;
    k.invW = 1.0f / k.fW, k.invH = 1.0f / k.fH;
    k.asp = k.fW / k.fH;
    k.ia = 1.0f / (k.A * k.asp), k.ib = 1.0f / k.A;
    for (int c = 0; c < 3; ++c) {
        k.cpos[c] = in.cur.pos[c], k.cfront[c] = in.cur.front[c], k.cup[c] = in.cur.up[c];
        k.ppos[c] = in.prev.pos[c], k.pfront[c] = in.prev.front[c], k.pup[c] = in.prev.up[c];
    }
    rtt::cross3(k.cfront, k.cup, k.cright);
    rtt::cross3(k.pfront, k.pup, k.pright);
    p.cur_frames = in.cur_frames, p.history_frames = in.history_frames, p.max_history = in.max_history;
    p.depth_tolerance = in.depth_tolerance, p.normal_threshold = in.normal_threshold;
    p.tiles_x = (uint32_t)((in.width + kTemporalTileW - 1) / kTemporalTileW);
    p.tiles_y = (uint32_t)((in.height + kTemporalTileH - 1) / kTemporalTileH);
    // <= (w / 64 + 1) (h / 4 + 1) with w h <= 2^31: below 2^31
    p.grid = (uint32_t)((uint64_t)p.tiles_x * p.tiles_y);
    return RT_SUCCESS;
}

}  // namespace rtp

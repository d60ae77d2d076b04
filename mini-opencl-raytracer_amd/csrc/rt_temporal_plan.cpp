// rt_temporal_plan.cpp -- the plan of one temporal reprojection (rt_temporal_plan.hpp): the argument
// checks in their documented order, the fp32 host constants of the definition (include/rt_hip.h) and
// the grid.  Pure arithmetic, kept where a CPU test can sweep it (tests/native/temporal_plan_main.cpp).
#include "rt_temporal_plan.hpp"

#include <cmath>

#include "../../include/rt_status.h"

namespace rtp {

// (every comparison is false for a NaN, so the finite test comes first)
bool finite_in(float v, float lo, float hi) { return std::isfinite(v) && v >= lo && v <= hi; }

bool view_finite(const TemporalView& v) {
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(v.pos[c]) || !std::isfinite(v.front[c]) || !std::isfinite(v.up[c])) return false;
    return true;
}

bool image_size_ok(uint64_t width, uint64_t height) {
    // (each factor first: their product cannot wrap)
    return width != 0 && height != 0 && width <= kTemporalMaxPixels && height <= kTemporalMaxPixels &&
           width * height <= kTemporalMaxPixels;
}

rtt::TemporalConsts view_consts(uint64_t width, uint64_t height, const TemporalView& cur, const TemporalView& prev) {
    rtt::TemporalConsts k{};
    k.A = rtt::kTanHalfFov;
    k.fW = (float)width, k.fH = (float)height;
    k.invW = 1.0f / k.fW, k.invH = 1.0f / k.fH;
    k.asp = k.fW / k.fH;
    k.ia = 1.0f / (k.A * k.asp), k.ib = 1.0f / k.A;
    for (int c = 0; c < 3; ++c) {
        k.cpos[c] = cur.pos[c], k.cfront[c] = cur.front[c], k.cup[c] = cur.up[c];
        k.ppos[c] = prev.pos[c], k.pfront[c] = prev.front[c], k.pup[c] = prev.up[c];
    }
    rtt::cross3(k.cfront, k.cup, k.cright);
    rtt::cross3(k.pfront, k.pup, k.pright);
    return k;
}

void temporal_tiles(uint64_t width, uint64_t height, uint32_t* tiles_x, uint32_t* tiles_y, uint32_t* grid) {
    *tiles_x = (uint32_t)((width + kTemporalTileW - 1) / kTemporalTileW);
    *tiles_y = (uint32_t)((height + kTemporalTileH - 1) / kTemporalTileH);
    // <= (w / 64 + 1) (h / 4 + 1) with w h <= 2^31: below 2^31
    *grid = (uint32_t)((uint64_t)*tiles_x * *tiles_y);
}

int temporal_plan(const TemporalIn& in, TemporalPlan* out) {
    *out = TemporalPlan{};
    TemporalPlan& p = *out;
    if (!in.params_ok) return RT_INVALID_VALUE;
    if (!image_size_ok(in.width, in.height)) return RT_INVALID_VALUE;
    if (!view_finite(in.cur) || !view_finite(in.prev)) return RT_INVALID_VALUE;
    if (!finite_in(in.cur_frames, 1.0f, kTemporalMaxFrames)) return RT_INVALID_VALUE;
    if (!(in.history_frames == 0.0f || finite_in(in.history_frames, 1.0f, kTemporalMaxFrames))) return RT_INVALID_VALUE;
    if (!finite_in(in.max_history, in.cur_frames, kTemporalMaxFrames)) return RT_INVALID_VALUE;
    if (!finite_in(in.depth_tolerance, 0.0f, 1.0f) || !finite_in(in.normal_threshold, -1.0f, 1.0f)) return RT_INVALID_VALUE;

    if (in.hist_given != in.hist_features_given) return RT_INVALID_MEM_OBJECT;
    if (!in.cur_ok || !in.cur_features_ok || !in.out_ok) return RT_INVALID_MEM_OBJECT;
    if (in.hist_given && (!in.hist_ok || !in.hist_features_ok)) return RT_INVALID_MEM_OBJECT;
    if (in.motion_given && !in.motion_ok) return RT_INVALID_MEM_OBJECT;
    if (in.out_is_input) return RT_INVALID_MEM_OBJECT;

    const uint64_t pixels = in.width * in.height;
    if (pixels > in.cur_bytes / kTemporalPixelBytes || pixels > in.cur_features_bytes / kTemporalFeatureBytes ||
        pixels > in.out_bytes / kTemporalPixelBytes)
        return RT_INVALID_BUFFER_SIZE;
    if (in.hist_given &&
        (pixels > in.hist_bytes / kTemporalPixelBytes || pixels > in.hist_features_bytes / kTemporalFeatureBytes))
        return RT_INVALID_BUFFER_SIZE;
    if (in.motion_given && pixels > in.motion_bytes / kTemporalMotionBytes) return RT_INVALID_BUFFER_SIZE;

    p.width = (uint32_t)in.width, p.height = (uint32_t)in.height;
    p.has_history = in.hist_given;
    p.has_motion = in.motion_given;
    p.k = view_consts(in.width, in.height, in.cur, in.prev);
    p.cur_frames = in.cur_frames, p.history_frames = in.history_frames, p.max_history = in.max_history;
    p.depth_tolerance = in.depth_tolerance, p.normal_threshold = in.normal_threshold;
    temporal_tiles(in.width, in.height, &p.tiles_x, &p.tiles_y, &p.grid);
    return RT_SUCCESS;
}

}  // namespace rtp

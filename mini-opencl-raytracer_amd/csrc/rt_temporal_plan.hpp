// rt_temporal_plan.hpp -- how one temporal reprojection (rtEnqueueTemporalAccumulate) is launched, as
// a pure function of plain values (rt_temporal_plan.cpp): no HIP, no allocation, no globals.  The C
// ABI fills a TemporalIn, calls temporal_plan and launches one kernel (rt_temporal.hip) with the
// plan's constants and grid.
//
// The grid: workgroup b of the 1-D grid is tile (b % tiles_x, b / tiles_x), a tile being
// kTemporalTileW contiguous columns (one wave's lanes) of kTemporalTileH rows (one wave each).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "rt_temporal_math.hpp"

namespace rtp {

constexpr uint64_t kTemporalMaxPixels = 1ull << 31;
constexpr uint32_t kTemporalTileW = 64, kTemporalTileH = 4;
constexpr uint32_t kTemporalThreads = kTemporalTileW * kTemporalTileH;
constexpr uint32_t kTemporalPixelBytes = 16, kTemporalFeatureBytes = 32, kTemporalMotionBytes = 32;
constexpr float kTemporalMaxFrames = 0x1p20f;   // of cur_frames, history_frames and max_history
constexpr float kTemporalMinWeight = 0x1p-6f;   // step 6: the least sum of counted bilinear weights

struct TemporalView {
    float pos[3], front[3], up[3];
};

struct TemporalIn {
    bool params_ok;                 // params != NULL
    uint64_t width, height;
    TemporalView cur, prev;
    float cur_frames, history_frames, max_history, depth_tolerance, normal_threshold;
    bool hist_given, hist_features_given;             // the handle is not NULL
    bool cur_ok, cur_features_ok, out_ok;             // each a buffer of this context
    bool hist_ok, hist_features_ok;                   // (looked at only when given)
    bool out_is_input;                                // `out` is one of the four inputs
    uint64_t cur_bytes, cur_features_bytes, hist_bytes, hist_features_bytes, out_bytes;
    // rtEnqueueTemporalAccumulateMotion (all false / zero: rtEnqueueTemporalAccumulate itself)
    bool motion_given, motion_ok;                     // the handle is not NULL; a buffer of this context
    uint64_t motion_bytes;
};

struct TemporalPlan {
    uint32_t width, height;
    bool has_history;
    bool has_motion;                // step 2 is motion[p].prev_point (rt_pixel_motion records)
    rtt::TemporalConsts k;
    float cur_frames, history_frames, max_history, depth_tolerance, normal_threshold;
    uint32_t tiles_x, tiles_y;
    uint32_t grid;                  // workgroups of kTemporalThreads
};

// The parts temporal_plan shares with the plan of the sample reprojection (rt_reproject_plan.hpp), which
// runs on the same views and the same tiles: each a row of the checks below or a piece of the plan.
bool finite_in(float v, float lo, float hi);             // finite and in [lo, hi]
bool view_finite(const TemporalView& v);
bool image_size_ok(uint64_t width, uint64_t height);     // neither zero, width * height <= 2^31
// the fp32 host constants of the definition (include/rt_hip.h) for an image that passed image_size_ok
rtt::TemporalConsts view_consts(uint64_t width, uint64_t height, const TemporalView& cur, const TemporalView& prev);
void temporal_tiles(uint64_t width, uint64_t height, uint32_t* tiles_x, uint32_t* tiles_y, uint32_t* grid);

// RT_SUCCESS, or, in this order: RT_INVALID_VALUE (no params; width or height zero; width * height >
// 2^31; a camera component not finite; cur_frames not finite, < 1 or > 2^20; history_frames negative,
// not finite, in (0, 1) or > 2^20; max_history not finite, < cur_frames or > 2^20; depth_tolerance not
// finite or outside [0, 1]; normal_threshold not finite or outside [-1, 1]), RT_INVALID_MEM_OBJECT
// (exactly one of hist and hist_features given; a required or given buffer that is not this context's;
// `out` one of the inputs, `motion` among them), RT_INVALID_BUFFER_SIZE (an image below 16 B per pixel,
// features or motion records below 32 B).
int temporal_plan(const TemporalIn& in, TemporalPlan* out);

}  // namespace rtp

// rt_motion_plan.hpp -- how the motion calls are launched, as pure functions of plain values
// (rt_motion_plan.cpp): no HIP, no allocation, no globals.  rtEnqueueExtractVertices, rtEnqueueHitMotion
// and the parts of rtEnqueueFrameMotion that are not its query's (rt_query_plan.hpp): the argument
// checks in their documented order (include/rt_hip.h), the 32-bit ranges and the grids.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "rt_motion_math.hpp"
#include "rt_temporal_plan.hpp"

namespace rtp {

constexpr uint32_t kMotionThreads = 256;             // one record per lane, no LDS (both small kernels)
constexpr uint64_t kMotionMaxTris = 0x40000000ull;   // rtEnqueueUpdateVertices' bound on the triangle array
constexpr uint64_t kMotionMaxHits = 1ull << 31;      // first + n at most (record indices are 32-bit)
constexpr uint32_t kTriangleBytes = 256;

// ---- rtEnqueueExtractVertices ----
struct ExtractIn {
    bool tris_ok, positions_ok;          // each a buffer of this context
    bool normals_given, normals_ok;      // (normals_ok looked at only when given)
    bool out_is_tris;                    // `positions` or `normals` is `tris`
    bool outs_same;                      // `positions` and `normals` are one buffer
    uint64_t tris_bytes, positions_bytes, normals_bytes;
    uint64_t first_tri, n_tris;
};
struct ExtractPlan {
    bool nothing;                        // n_tris == 0: RT_SUCCESS, no launch
    uint32_t first, count;               // triangles [first, first + count)
    uint32_t grid;                       // workgroups of kMotionThreads: one (triangle, vertex) per lane
};
// rtEnqueueUpdateVertices' rows in its order: RT_INVALID_MEM_OBJECT (a buffer that is NULL or another
// context's, `normals` excepted; an output that is `tris`; the two outputs one buffer),
// RT_INVALID_BUFFER_SIZE (first_tri + n_tris beyond `tris`; more than 2^30 triangles; an output under
// 48 * n_tris bytes).
int extract_plan(const ExtractIn& in, ExtractPlan* out);

// ---- the prev_* arguments of rtEnqueueHitMotion and rtEnqueueFrameMotion ----
struct PrevIn {
    bool positions_given, positions_ok;  // (ok: a buffer of this context; looked at only when given)
    bool normals_given, normals_ok;
    bool is_out;                         // either one is the call's output
    uint64_t positions_bytes, normals_bytes;
    uint64_t first_tri, n_tris;          // the moved range
};
int prev_handles(const PrevIn& in);                      // RT_INVALID_MEM_OBJECT rows
int prev_sizes(const PrevIn& in);                        // RT_INVALID_BUFFER_SIZE: a buffer under 48 * n_tris
int prev_range(const PrevIn& in, uint64_t scene_tris);   // RT_INVALID_BUFFER_SIZE: the range beyond the scene

// ---- rtEnqueueHitMotion ----
struct HitMotionIn {
    uint64_t first, n;                   // the range [first, first + n) of `hits` and `motion`
    uint64_t hits_bytes, out_bytes;
    bool out_ok;                         // `motion` is a buffer of this context
    bool out_is_hits;
    bool scene_bound;                    // scene and node slots are bound ...
    uint64_t scene_tris;                 // ... and the triangle buffer's record count
    PrevIn prev;
};
struct HitMotionPlan {
    bool nothing;                        // n == 0: RT_SUCCESS, no launch
    uint32_t first, count;
    uint32_t first_tri, n_tris;          // the moved range, 32-bit (inside the scene: < 2^30)
    uint32_t grid;                       // workgroups of kMotionThreads: record first + i goes to lane i
};
// RT_SUCCESS (out->nothing set when n == 0), or, in this order: RT_INVALID_VALUE (first + n > 2^31),
// RT_INVALID_MEM_OBJECT (`motion` no buffer of the context or `hits` itself; prev_positions NULL with
// n_tris != 0; a given prev_* buffer another context's, or `motion`), RT_INVALID_BUFFER_SIZE (the range
// ends beyond `hits` or `motion`; a given prev_* buffer under 48 * n_tris bytes), RT_INVALID_KERNEL_ARGS
// (scene or node slot unbound), RT_INVALID_BUFFER_SIZE (first_tri + n_tris beyond the scene's triangles).
int hit_motion_plan(const HitMotionIn& in, HitMotionPlan* out);

// ---- rtEnqueueFrameMotion (the checks before the scene is packed; the launch is the query's plan) ----
struct FrameMotionIn {
    bool args_bound;                     // scene, node, WIDTH, HEIGHT and the three camera slots
    uint64_t width, height;
    uint64_t global_work_size;
    uint64_t out_bytes;
    uint64_t scene_tris;
    TemporalView cam;
    PrevIn prev;
};
struct FrameMotionPlan {
    uint32_t count;                      // pixels [0, count)
    uint32_t first_tri, n_tris;
    rtt::TemporalConsts k;               // view_consts of the camera (both views: only the current is read)
};
// RT_SUCCESS, or, in this order: RT_INVALID_KERNEL_ARGS (a slot unbound; WIDTH or HEIGHT zero or
// WIDTH * HEIGHT > 2^31), RT_INVALID_GLOBAL_WORK_SIZE (zero or above 2^31), RT_INVALID_BUFFER_SIZE
// (`motion` under 32 B per work item), then prev_handles, prev_sizes and prev_range.
int frame_motion_plan(const FrameMotionIn& in, FrameMotionPlan* out);

}  // namespace rtp

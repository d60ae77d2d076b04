// rt_motion_plan.cpp -- the plans of the motion calls (rt_motion_plan.hpp): the argument checks in their
// documented order (include/rt_hip.h), the 32-bit ranges and the grids.  Pure arithmetic: a range that
// runs past a buffer starts here, so it is kept where a CPU test can sweep it
// (tests/native/motion_main.cpp).
#include "rt_motion_plan.hpp"

#include "../../include/rt_status.h"

namespace rtp {

int extract_plan(const ExtractIn& in, ExtractPlan* out) {
    *out = ExtractPlan{};
    ExtractPlan& p = *out;
    if (!in.tris_ok || !in.positions_ok || (in.normals_given && !in.normals_ok)) return RT_INVALID_MEM_OBJECT;
    if (in.out_is_tris || in.outs_same) return RT_INVALID_MEM_OBJECT;
    const uint64_t nt = in.tris_bytes / kTriangleBytes;
    if (in.first_tri > nt || in.n_tris > nt - in.first_tri || nt > kMotionMaxTris) return RT_INVALID_BUFFER_SIZE;
    if (in.positions_bytes / rtm::kTriPointsBytes < in.n_tris ||
        (in.normals_given && in.normals_bytes / rtm::kTriPointsBytes < in.n_tris))
        return RT_INVALID_BUFFER_SIZE;
    if (in.n_tris == 0) {
        p.nothing = true;
        return RT_SUCCESS;
    }
    p.first = (uint32_t)in.first_tri, p.count = (uint32_t)in.n_tris;
    p.grid = (uint32_t)((3 * in.n_tris + kMotionThreads - 1) / kMotionThreads);  // n_tris <= 2^30
    return RT_SUCCESS;
}

int prev_handles(const PrevIn& in) {
    if (!in.positions_given && in.n_tris != 0) return RT_INVALID_MEM_OBJECT;
    if ((in.positions_given && !in.positions_ok) || (in.normals_given && !in.normals_ok)) return RT_INVALID_MEM_OBJECT;
    if (in.is_out) return RT_INVALID_MEM_OBJECT;
    return RT_SUCCESS;
}

int prev_sizes(const PrevIn& in) {
    if ((in.positions_given && in.positions_bytes / rtm::kTriPointsBytes < in.n_tris) ||
        (in.normals_given && in.normals_bytes / rtm::kTriPointsBytes < in.n_tris))
        return RT_INVALID_BUFFER_SIZE;
    return RT_SUCCESS;
}

int prev_range(const PrevIn& in, uint64_t scene_tris) {
    // (each term first: their sum cannot wrap)
    if (in.first_tri > scene_tris || in.n_tris > scene_tris - in.first_tri || scene_tris > kMotionMaxTris)
        return RT_INVALID_BUFFER_SIZE;
    return RT_SUCCESS;
}

int hit_motion_plan(const HitMotionIn& in, HitMotionPlan* out) {
    *out = HitMotionPlan{};
    HitMotionPlan& p = *out;
    if (in.first > kMotionMaxHits || in.n > kMotionMaxHits || in.first + in.n > kMotionMaxHits) return RT_INVALID_VALUE;
    if (!in.out_ok || in.out_is_hits) return RT_INVALID_MEM_OBJECT;
    int rc = prev_handles(in.prev);
    if (rc) return rc;
    const uint64_t end = in.first + in.n;
    if (end > in.hits_bytes / rtm::kHitBytes || end > in.out_bytes / rtm::kMotionBytes) return RT_INVALID_BUFFER_SIZE;
    rc = prev_sizes(in.prev);
    if (rc) return rc;
    if (!in.scene_bound) return RT_INVALID_KERNEL_ARGS;
    rc = prev_range(in.prev, in.scene_tris);
    if (rc) return rc;
    if (in.n == 0) {
        p.nothing = true;
        return RT_SUCCESS;
    }
    p.first = (uint32_t)in.first, p.count = (uint32_t)in.n;
    p.first_tri = (uint32_t)in.prev.first_tri, p.n_tris = (uint32_t)in.prev.n_tris;
    p.grid = (uint32_t)((in.n + kMotionThreads - 1) / kMotionThreads);  // <= 2^23
    return RT_SUCCESS;
}

int frame_motion_plan(const FrameMotionIn& in, FrameMotionPlan* out) {
    *out = FrameMotionPlan{};
    FrameMotionPlan& p = *out;
    if (!in.args_bound || !image_size_ok(in.width, in.height)) return RT_INVALID_KERNEL_ARGS;
    if (in.global_work_size == 0 || in.global_work_size > kMotionMaxHits) return RT_INVALID_GLOBAL_WORK_SIZE;
    if (in.out_bytes / rtm::kMotionBytes < in.global_work_size) return RT_INVALID_BUFFER_SIZE;
    int rc = prev_handles(in.prev);
    if (rc) return rc;
    rc = prev_sizes(in.prev);
    if (rc) return rc;
    rc = prev_range(in.prev, in.scene_tris);
    if (rc) return rc;
    p.count = (uint32_t)in.global_work_size;
    p.first_tri = (uint32_t)in.prev.first_tri, p.n_tris = (uint32_t)in.prev.n_tris;
    p.k = view_consts(in.width, in.height, in.cam, in.cam);
    return RT_SUCCESS;
}

}  // namespace rtp

// rt_motion_launch.hpp -- the two small motion kernels (rt_motion.hip), launched by
// rtEnqueueExtractVertices and rtEnqueueHitMotion (rt_capi.cpp) from their plans (rt_motion_plan.hpp).
// rtEnqueueFrameMotion's kernel is a variant of the query's (rt_motion.hpp, rt_kernels.hpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt_cl_types.h"
#include "rt_motion_plan.hpp"

namespace rtmo {

struct HitMotionArgs {
    const float4* hits;            // rt_ray_hit records
    const rt_cl_triangle* tris;    // the scene's 256-B records
    uint32_t n_scene;              // ... and their count
    const float4* prev_positions;  // rt_tri_points of triangles [first_tri, first_tri + n_tris); null: n_tris == 0
    const float4* prev_normals;    // null: the current normals
    float4* out;                   // rt_pixel_motion records as 2 x float4
};

// One launch each on `st`.  hipErrorInvalidValue for a plan that does not match the arguments: nothing
// is launched.
hipError_t launch_extract_vertices(const rt_cl_triangle* tris, const rtp::ExtractPlan& p, float4* positions,
                                   float4* normals, hipStream_t st);
hipError_t launch_hit_motion(const HitMotionArgs& a, const rtp::HitMotionPlan& p, hipStream_t st);

}  // namespace rtmo

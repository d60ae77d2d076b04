// rt_path_kill.hpp -- when a step launch may stop walking a path whose throughput has reached exactly
// zero, as a pure function of the packed materials, the triangles, the root bounds and three launch
// arguments (rt_path_kill.cpp): no HIP, no allocation, no globals.  The rule is sufficient, not
// necessary: a scene or launch it refuses renders as before, with every segment walked.
#pragma once

#include <stdint.h>

#include <cmath>

#include "../../include/rt_cl_types.h"

namespace rtp {

// The scene half, evaluated once per full preparation (rti::DeviceScene) on one policy's material
// table: `mats` holds n_mats packed records of 16 floats -- {diffuse, 1/(alpha + 1)}, {specular,
// alpha^2/pi}, {emission, alpha^2 - 1}, {roughness, alpha, 0, 0} -- exactly as the device formed them
// (material_record); `root` the root node's bounds (min xyz, max xyz), null when the host does not know
// them.  Returns whether a dead path can be dropped; `why` (optional) names the clause that refused.
bool path_kill_scene_ok(const float* mats, uint32_t n_mats, const rt_cl_triangle* tris, uint32_t n_tris,
                        const float* root, const char** why = nullptr);

// The launch half, evaluated by the plan for every launch (clauses L1-L3 of rt_path_kill.cpp; inline:
// the plan's translation unit stands alone in its CPU tests).
inline bool path_kill_launch_ok(int32_t light_type, float skybox_intensity, int32_t light_bounces) {
    return light_type <= 0 && std::isfinite(skybox_intensity) && light_bounces > 1;
}

}  // namespace rtp

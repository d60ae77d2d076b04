// rt_refit.hpp -- vertex update and device-side BVH refit (rt_refit.hip), called by
// rtEnqueueUpdateVertices / rtRefitBVH (rt_capi.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt_cl_types.h"

namespace rtr {

constexpr uint32_t kNoParent = 0xffffffffu;  // the root's parent link

// Everything the refit of one kernel's tree touches.  `nodes` is the caller's CLLinearBVHNode
// buffer (validated by the last full preparation: leaf ranges inside the n_tris triangles, children
// i + 1 and offset > i + 1 inside the tree's n_nodes records); parent / slot / arrivals hold n_nodes
// words each.  The derived layouts are the ones rt_scene_pack.cpp builds; a null pointer = not kept.
struct RefitArgs {
    const rt_cl_triangle* tris;
    uint32_t n_tris;
    rt_cl_bvh_node* nodes;
    uint32_t n_nodes;
    const uint32_t* parent;  // node -> parent (kNoParent: the root)
    const uint32_t* slot;    // node -> record of g_nodes (build_global_nodes renumbers the top)
    uint32_t* arrivals;      // zero on entry (the launch helper clears them on the stream)
    float4* oct;             // octant-major planes A[o][node], B[o][node]
    uint32_t oct_stride, oct_b;
    float4* goct;            // node-major regrouped records, B planes at float4 offset goct_b
    uint32_t goct_b, goct_group;
    float4* g_nodes;         // 64-B records
};

// positions / normals: n records of 48 B ({p1, p2, p3}, 16-B slots, w ignored) -> the xyz of
// v1/v2/v3.position (and .normal when normals != nullptr) of tris[first, first + n)
hipError_t launch_update_vertices(rt_cl_triangle* tris, uint32_t first, uint32_t n, const float4* positions,
                                  const float4* normals, hipStream_t st);

// clears the arrival counters, recomputes every node's bounds bottom-up, then copies the planes into
// the derived layouts; all on `st`, nothing waits on the host
hipError_t launch_refit(const RefitArgs& a, hipStream_t st);

}  // namespace rtr

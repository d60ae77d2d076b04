// rt_trace_plan.hpp -- how one path trace over caller rays (rtEnqueueTracePaths) is checked and
// launched, as a pure function of plain values (rt_trace_plan.cpp): no HIP, no allocation, no
// globals.  The C ABI fills a TraceIn, calls trace_check before the scene is prepared and trace_shape
// after it, looks the kernel's occupancy up for the LDS size that gives, and calls trace_grid.  The
// query's plan (rt_query_plan.hpp) and the render's (rt_launch_plan.hpp) are separate and untouched.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "rt_layout.hpp"
#include "rt_tuning.hpp"

namespace rtp {

constexpr int kTraceLinear = 0, kTraceFrame0 = 1;    // RT_TRACE_LINEAR, RT_TRACE_FRAME0
constexpr uint64_t kTraceMaxRecords = 1ull << 31;    // first + n at most (record indices are 32-bit)
constexpr size_t kTraceLdsBudget = 64 * 1024;        // per-workgroup LDS of the LDS scene path, rings included
constexpr uint32_t kTraceRayBytes = 32, kTraceSeedBytes = 4, kTraceResultBytes = 16;

struct TraceIn {
    // ---- the call's arguments ----
    bool params_given;                   // `params` is not NULL ...
    int encoding;                        // ... and its encoding (RT_TRACE_*)
    uint64_t first, n;                   // the range [first, first + n)
    bool rays_ok, out_ok;                // `rays` / `out`: a buffer of this context
    bool seeds_given, seeds_ok;          // `seeds` is not NULL; ... and a buffer of this context
    bool out_is_input;                   // `out` is also `rays` or `seeds`
    uint64_t rays_bytes, seeds_bytes, out_bytes;  // sizes of the buffers (seeds_bytes unused without `seeds`)
    bool scene_bound;                    // scene, node and material slots are bound
    bool lights_set;                     // LIGHT_BOUNCES, LIGHT_TYPE and SKYBOX_INTENSITY are set
    // ---- the kernel's settings and its packed scene (trace_shape) ----
    int math;                            // RT_MATH_*
    bool stats;                          // rt_stats counters on
    bool shadow_rays;                    // rtKernelSetShadowRays: the kernel that walks shadow rays
    uint32_t n_nodes, n_tris, n_mats;    // the packed scene
    bool oct_ok;                         // every leaf fits the octant records
    bool goct_available;                 // regrouped octant records exist ...
    uint32_t goct_b;                     // ... and their B planes' float4 offset
    bool force_global;
    Tuning tune;                         // trace_refill_min, trace_shade_min, max_blocks and the render's step weights
    int num_cus;
};

struct TracePlan {
    bool nothing;                        // n == 0: RT_SUCCESS, no launch
    // ---- trace_shape ----
    rtk::Variant variant;                // the kernel: scene staged in LDS (B planes at kOctB) or its octant
                                         // and shading records read from HBM/L2
    bool regrouped;                      // HBM/L2 path: walk the regrouped octant records
    size_t smem;                         // dynamic LDS bytes
    uint32_t first, count;               // the range, 32-bit
    uint32_t nUnits;                     // 64-record units: unit j = records first + 64 j .. (the last one may be partial)
    uint32_t octStride, octB, octRecords, nNodes;
    uint32_t refillMin, shadeMin, stepWeightNode, stepWeightLeaf;
    // ---- trace_grid ----
    uint32_t grid;                       // workgroups of kTraceThreads; unit j goes to wave j % (4 grid)
};

// The rows that need no packed scene, in rtEnqueueTracePaths' order: RT_INVALID_VALUE (params NULL;
// an encoding other than the two; first + n > 2^31), RT_INVALID_MEM_OBJECT (rays or out no buffer of
// the context; seeds given and not one; out also an input), RT_INVALID_BUFFER_SIZE (the range ends
// beyond a buffer), RT_INVALID_KERNEL_ARGS (scene, node or material slot unbound; then a light slot
// unset).  RT_SUCCESS otherwise.
int trace_check(const TraceIn& in);
// trace_check, then RT_INVALID_OPERATION (a leaf of more than 127 triangles: no octant records to
// walk), then out->nothing when n == 0, else everything up to the LDS size.
int trace_shape(const TraceIn& in, TracePlan* out);
// The grid, from the occupancy (workgroups per CU) of the kernel trace_shape chose at out->smem.
void trace_grid(const TraceIn& in, int occ, TracePlan* out);

inline int trace_plan(const TraceIn& in, int occ, TracePlan* out) {
    const int rc = trace_shape(in, out);
    if (rc == 0 && !out->nothing) trace_grid(in, occ, out);
    return rc;
}

}  // namespace rtp

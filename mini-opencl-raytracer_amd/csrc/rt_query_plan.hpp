// rt_query_plan.hpp -- how one ray query (rtEnqueueIntersectRays) is launched, as a pure function
// of plain values (rt_query_plan.cpp): no HIP, no allocation, no globals.  The C ABI fills a
// QueryIn, calls query_shape, looks the kernel's occupancy up for the LDS size that gives, and
// calls query_grid.  The render's plan (rt_launch_plan.hpp) is separate and untouched.  surface_plan is the
// same for the surface records of rt_surface.hpp (rtEnqueueHitSurfaces, rtEnqueueFrameFeatures).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "rt_layout.hpp"
#include "rt_tuning.hpp"

namespace rtp {

constexpr int kQueryClosest = 0, kQueryAny = 1;      // RT_QUERY_CLOSEST, RT_QUERY_ANY
constexpr uint64_t kQueryMaxRays = 1ull << 31;       // first + n_rays at most (ray indices are 32-bit)
constexpr size_t kQueryLdsBudget = 64 * 1024;        // per-workgroup LDS of the LDS scene path, rings included

struct QueryIn {
    uint64_t first_ray, n_rays;          // the range [first_ray, first_ray + n_rays)
    uint64_t rays_bytes, hits_bytes;     // sizes of the two buffers
    bool same_buffer;                    // rays and hits are one buffer
    int mode;                            // RT_QUERY_*
    int math;                            // RT_MATH_*
    bool stats;                          // rt_stats counters on
    uint32_t n_nodes, n_tris;            // the packed scene
    bool oct_ok;                         // every leaf fits the octant records
    bool goct_available;                 // regrouped octant records exist ...
    uint32_t goct_b;                     // ... and their B planes' float4 offset
    bool force_global;
    Tuning tune;                         // query_refill_min, max_blocks and the render's step weights
    int num_cus;
};

struct QueryPlan {
    bool nothing;                        // n_rays == 0: RT_SUCCESS, no launch
    // ---- query_shape ----
    rtk::Variant variant;                // the kernel: scene staged in LDS (B planes at kOctB) or its octant
                                         // records walked in HBM/L2; any-hit
    bool regrouped;                      // HBM/L2 path: walk the regrouped octant records
    size_t smem;                         // dynamic LDS bytes
    uint32_t first, count;               // the range, 32-bit
    uint32_t nUnits;                     // 64-ray units: unit j = rays first + 64 j .. (the last one may be partial)
    uint32_t octStride, octB, octRecords, nNodes;
    uint32_t refillMin, stepWeightNode, stepWeightLeaf;
    // ---- query_grid ----
    uint32_t grid;                       // workgroups of kQueryThreads; unit j goes to wave j % (8 grid)
};

// Everything up to the LDS size.  RT_SUCCESS (out->nothing set when n_rays == 0 and the mode is
// valid), or, in this order: RT_INVALID_VALUE (mode; first_ray + n_rays > 2^31), RT_INVALID_MEM_OBJECT (one buffer for
// rays and hits), RT_INVALID_BUFFER_SIZE (the range ends beyond either buffer),
// RT_INVALID_OPERATION (a leaf of more than 127 triangles: no octant records to walk).
int query_shape(const QueryIn& in, QueryPlan* out);
// The grid, from the occupancy (workgroups per CU) of the kernel query_shape chose at out->smem.
void query_grid(const QueryIn& in, int occ, QueryPlan* out);

inline int query_plan(const QueryIn& in, int occ, QueryPlan* out) {
    const int rc = query_shape(in, out);
    if (rc == 0 && !out->nothing) query_grid(in, occ, out);
    return rc;
}

// ---- surface records (rtEnqueueHitSurfaces, and the accumulating launches of rtEnqueueFrameFeatures) ----
constexpr uint32_t kRayBytes = 32, kHitBytes = 16, kSurfaceBytes = 64, kFeatureBytes = 32;
constexpr unsigned kMaxFeatureFrames = 4096;         // rtEnqueueFrameFeatures: coverage stays an exact count

struct SurfaceIn {
    uint64_t first, n;                   // the range [first, first + n)
    uint64_t rays_bytes, hits_bytes;     // sizes of the two inputs
    uint64_t out_bytes;                  // size of the output
    bool out_ok;                         // the output is a buffer of this context
    bool out_is_input;                   // ... and also `rays` or `hits`
    bool rays_is_hits;                   // `rays` and `hits` are one buffer
    bool scene_bound;                    // scene and node slots are bound
    bool accumulate;                     // the output holds rt_pixel_features sums, not rt_surface records
};

struct SurfacePlan {
    bool nothing;                        // n == 0: RT_SUCCESS, no launch
    bool accumulate;                     // the kernel variant
    uint32_t first, count;               // the range, 32-bit
    uint32_t grid;                       // workgroups of kSurfaceThreads: record first + i goes to lane i
};

// RT_SUCCESS (out->nothing set when n == 0), or, in this order: RT_INVALID_VALUE (first + n > 2^31),
// RT_INVALID_MEM_OBJECT (the output is no buffer of the context, or one of the inputs; the inputs are
// one buffer), RT_INVALID_BUFFER_SIZE (the range ends beyond any of the three buffers),
// RT_INVALID_KERNEL_ARGS (scene or node slot unbound).
int surface_plan(const SurfaceIn& in, SurfacePlan* out);

}  // namespace rtp

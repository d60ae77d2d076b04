// rt_launch_plan.hpp -- how one KernelEntry launch hands its work out, as a pure function of plain
// values (rt_launch_plan.cpp): no HIP, no allocation, no globals.  enqueue (rt_capi.cpp) fills a
// PlanIn, calls plan_shape, looks the occupancy of the kernel that names (LaunchPlan::variant) up for
// the LDS size it gives, calls plan_handout, and turns the LaunchPlan into rtk::KernelArgs, resources
// and launches.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "rt_layout.hpp"
#include "rt_path_kill.hpp"
#include "rt_tuning.hpp"
#include "rt_view_cull.hpp"

namespace rtp {

struct PlanIn {
    uint32_t W, H;                          // image size (both > 0)
    uint64_t gws;                           // global work size of the launch
    uint64_t range_first, range_last;       // rtKernelSetWorkRange (last 0: to the end)
    uint32_t n_frames;                      // frames of this launch (>= 1)
    int32_t light_bounces;
    int sched, math;                        // as requested (RT_SCHED_*, RT_MATH_*)
    bool stats, hit_bound;                  // rt_stats counters on; primary-hit buffers bound
    bool fused;                             // radiance slots + accumulation launch (enqueue decides)
    bool overlap;                           // the context's accumulation overlap
    uint32_t band_period, band_phase;       // 8-row band interleave
    uint32_t n_nodes, n_tris, n_mats, n_top;  // the packed scene
    bool oct_ok;                            // every leaf fits the octant records
    bool goct_available;                    // regrouped octant records exist ...
    uint32_t goct_b;                        // ... and their B planes' float4 offset
    bool force_global;
    Tuning tune;                            // rtKernelSetTuning
    int num_cus;
    ViewRect view;                          // tiles that can see the scene (rt_view_cull.hpp); zero: all
    // the path kill (rt_path_kill.hpp): the scene half of its certificate as the packed scene caches it
    // for this launch's math, and the launch arguments its other half reads
    bool kill_scene_ok;
    int32_t light_type;
    float skybox_intensity;
};

struct LaunchPlan {
    bool nothing;                           // no work item in range / no band row: RT_SUCCESS, no launch
    // ---- plan_shape ----
    rtk::Variant variant;                   // the kernel: the schedule the launch runs, the scene walk, ...
    bool wf() const { return variant.sched == rtk::kSchedWavefront; }
    size_t smem;                            // dynamic LDS bytes
    // rtk::KernelArgs scalars
    uint64_t gidBegin, gidEnd;
    uint32_t rowBegin, rowCount, tilesX, nTiles, bandPeriod, bandPhase;
    uint32_t nTop;
    bool regrouped;                         // walk the regrouped octant records (goct_nodes)
    uint32_t octStride, octB, octRecords, nNodes;
    uint32_t refillMin, shadeMin, stepWeightNode, stepWeightLeaf;
    uint32_t flagTiles, nFrames, radStride;
    size_t need, fneed;                     // fused: radiance slots (float4) and frame-flag bytes of the set
    bool own_stream;                        // fused: the render goes to a render stream of its own
    bool pf_slots;                          // per-frame step launch: takes a counter slot, zeroes the other
    bool clear_counter_here;                // the launch's counters are cleared in front of it
    // the tiles the hand-out covers: visW x visH of them from (visTx0, visTy0) of this launch's tile
    // grid -- all of it (0, 0, tilesX, tilesY) unless the view cull applies; visTiles = visW * visH
    uint32_t visTx0, visTy0, visW, visH, visTiles;
    uint32_t pathKill;                      // 1: the launch is certified to drop paths of zero throughput
    // ---- plan_handout ----
    uint64_t grid;
    uint32_t tileMajor, chunkPixels, tailChunk, chunkSplit, tailBase, staticFirst, nParts, partLen;
    bool use_pf_sky;                        // per-frame sky shortcut keys
    // wavefront queues
    uint32_t cap, G, nBlocks, wfRefillMin;
    unsigned grid_s;
};

// RT_COUNTER_PARTS of this build (LaunchPlan::nParts is 0 or this)
uint32_t counter_parts();

// the schedule a launch runs: the wavefront one needs a bounded bounce loop (two launches per
// bounce), else the step schedule renders it (same bits)
int resolve_schedule(int sched, int32_t light_bounces);

// Everything up to the LDS size: returns RT_SUCCESS (out->nothing set when there is no launch to
// make), RT_INVALID_GLOBAL_WORK_SIZE or RT_INVALID_OPERATION.
int plan_shape(const PlanIn& in, LaunchPlan* out);
// The grid and the work hand-out, from the occupancy (workgroups per CU) of the kernel plan_shape
// chose at out->smem; occ_shade: the wavefront shade kernel's (read only when out->wf()).
void plan_handout(const PlanIn& in, int occ, int occ_shade, LaunchPlan* out);

// both steps (occupancies known beforehand: tests)
inline int plan_launch(const PlanIn& in, int occ, int occ_shade, LaunchPlan* out) {
    const int rc = plan_shape(in, out);
    if (rc == 0 && !out->nothing) plan_handout(in, occ, occ_shade, out);
    return rc;
}

}  // namespace rtp

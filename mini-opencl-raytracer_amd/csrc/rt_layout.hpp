// rt_layout.hpp -- layout constants, and the key that names a kernel variant (rtk::Variant), which
// the host side (rt_capi.cpp, rt_scene_pack.cpp, the planners) and the kernels (through
// rt_kernels.hpp) share.  No HIP here.
#pragma once

#include <stdint.h>

namespace rtk {

constexpr int kSchedTiles = 0;  // one pixel per lane per 16x16 tile, all bounces in place
// (1: path regeneration and 3: a per-wave LDS path pool were measured slower than the step
// schedule and retired in round 3; DESIGN.md section 5 keeps their numbers)
constexpr int kSchedStep = 2;   // per-wave state machine: node / triangle steps, batched shading
constexpr int kSchedWavefront = 4;  // extend / shade launches per bounce over HBM ray queues
// frames per fused launch (rtEnqueueKernelFrames splits longer runs)
constexpr uint32_t kMaxFusedFrames = 8;
// step schedule LDS per wave: the finish queue, 64 x {radiance, gid}
constexpr uint32_t kFinishWaveBytes = 64u * 16u;
// step schedule, LDS scenes: per-wave ring of camera rays generated a whole 8x8 tile at a time
// ({dir, seed}, {invDir, sign} (fused launches) + work-item id per slot)
constexpr uint32_t kRingSlots = 64;
constexpr uint32_t kRingWaveBytes = kRingSlots * 32u + kRingSlots * 4u;
constexpr uint32_t kRingWaveBytesPf = kRingSlots * 16u + kRingSlots * 4u;  // per-frame: no invDir
// step schedule: per workgroup, each wave's remaining chunk {next, end} (64-bit word per wave),
// from which its siblings take single tiles once the work counter is dry
constexpr uint32_t kStealBytes = 4u * 8u + 32u;  // (padded to whole float4s)
// END as a walk word that is neither a node (< 2^24) nor a leaf code (count << 24 | first, count
// 1..127): the step schedule's byte-address LDS walk and its octant walk over HBM/L2 (step_body)
constexpr uint32_t kEndWalk = 0xff000000u;
#ifndef RT_GOCT_END_WORD
#define RT_GOCT_END_WORD 1  // the HBM/L2 octant walk's END as kEndWalk (0: its sentinel's word, visited)
#endif

// the view cull (rt_view_cull.hpp): fused step launches hand out only the tiles that can see the scene,
// the accumulation takes the others as primary misses (0: every tile is rendered, for A/B builds)
#ifndef RT_VIEW_CULL
#define RT_VIEW_CULL 1
#endif

// the path kill (rt_path_kill.hpp): certified step launches end a path whose throughput has reached
// exactly zero instead of walking its remaining segments (0: every segment is walked, for A/B builds)
#ifndef RT_PATH_KILL
#define RT_PATH_KILL 1
#endif

// LDS node records of trees with at most kOctBMaxStride records per plane keep their B planes at
// the fixed float4 offset kOctB, so a node step reads B with an immediate offset from A's address
constexpr uint32_t kOctBMaxStride = 64;
// counter partitions: words between two partitions' counters (1 KB), and the most partitions
constexpr uint32_t kPartStride = 256;
constexpr uint32_t kMaxParts = 8;
constexpr uint32_t kOctB = 8 * kOctBMaxStride;

// ---- kernel variants ----
// How a kernel reads the scene: one of four walks, so "B planes at kOctB" without LDS, or octant
// records in HBM/L2 with the scene in LDS, cannot be written down.
enum class Walk : int {
    Lds = 0,          // node records, triangles and shading records staged in LDS
    LdsB = 1,         // ... with the B planes at kOctB (KernelArgs::octB == kOctB)
    GlobalOct = 2,    // scene too large for LDS: its octant records walked in HBM/L2
    GlobalNodes = 3,  // ... its 64-byte node records walked in HBM/L2
};
// Which kernel a launch runs.  The planners (rt_launch_plan.cpp, rt_query_plan.cpp) fill one; the
// launch and its occupancy query (rt_kernels.hpp) both pick the kernel from it.
struct Variant {
    int sched;    // kSched* (renders; ray queries leave it 0)
    int math;     // RT_MATH_*
    Walk walk;
    bool stats;   // rt_stats counters
    bool fused;   // the launch writes radiance slots (step schedule: the entry points' kMode)
    bool any;     // ray queries: any-hit
    bool shadow = false;  // path traces and fused samples: shadow rays (rtKernelSetShadowRays)
    bool lds() const { return walk == Walk::Lds || walk == Walk::LdsB; }
    // dense index for per-variant caches, < kVariantSlots (schedules 0, 2, 4; maths 0..2); shadow is the
    // highest-order factor, so a variant without it has the slot it had before the bit existed
    int slot() const {
        return (((((shadow * 3 + (sched >> 1)) * 3 + math) * 4 + (int)walk) * 2 + stats) * 2 + fused) * 2 + any;
    }
};
constexpr int kVariantSlots = 2 * 3 * 3 * 4 * 2 * 2 * 2;
static_assert((kSchedTiles >> 1) == 0 && (kSchedStep >> 1) == 1 && (kSchedWavefront >> 1) == 2, "Variant::slot");

// ---- wavefront schedule (rt_wavefront.hpp) ----
constexpr unsigned kWfExtendThreads = 512;  // extend workgroup: 8 waves (LDS scene staged once per 8)
constexpr unsigned kWfShadeThreads = 256;   // shade workgroup: one stream, 256 paths per round
constexpr int kWfMaxBounces = 64;            // longer bounce loops run the step schedule
constexpr uint32_t kWfRingBytes = 64u * 32u;  // extend: per-wave ray ring ({o, position}, {d, -})

// ---- ray queries (rt_query.hpp) ----
constexpr unsigned kQueryThreads = 512;          // query workgroup: 8 waves (LDS scene staged once per 8)
constexpr uint32_t kQueryRingBytes = 64u * 32u;  // per-wave ring of 64 rt_ray records

// ---- path tracing over caller rays (rt_trace.hpp) ----
constexpr unsigned kTraceThreads = 256;          // trace workgroup: 4 waves, as the step schedule's
constexpr uint32_t kTraceRingBytes = 64u * 32u + 64u * 4u;  // per-wave ring of 64 {rt_ray, seed} records

// ---- surface records (rt_surface.hpp) ----
constexpr unsigned kSurfaceThreads = 256;        // one record per lane, no LDS

}  // namespace rtk

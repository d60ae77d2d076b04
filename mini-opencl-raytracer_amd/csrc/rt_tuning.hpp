// rt_tuning.hpp -- the knobs of rtKernelSetTuning (rt_hip.h, enum rt_tuning): their defaults with
// the measurements behind them, and one table of ids and ranges that both the setter and the getter
// walk (rt_tuning.cpp).  Pure host code, no HIP.  A kernel holds one Tuning; the planners read it
// through PlanIn::tune and QueryIn::tune.  (RT_TUNE_TOP_NODES is not here: it renumbers the packed
// node records, so it lives with them in rti::DeviceScene.)
#pragma once

#include <stdint.h>

#include "rt_layout.hpp"

namespace rtp {

struct Tuning {
    // step schedule thresholds (lanes), swept on MI355X: LDS scenes (camera-ray ring)
    // profiles/r01/threshold_sweep_ring.txt, shading at 48 since work stealing (44 -> 48: fused
    // -0.3 %, per-frame -0.5 %, profiles/r03/shade_threshold_sweep.txt); scenes read from HBM/L2
    // keep 8 / 48
    uint32_t refill_min = 6, shade_min = 48;
    bool refill_min_set = false;  // RT_TUNE_REFILL_MIN given: also for small per-frame launches (plan_handout)
    // scenes read from HBM/L2: 0 = auto (64-B node records 8 / 48; octant records 16 / 48,
    // profiles/r02/goct_sweep.txt)
    uint32_t refill_min_g = 0, shade_min_g = 0;
    uint32_t w_node = 35, w_leaf = 55;         // step schedule: node / triangle step cost weights
    uint32_t w_node_g = 0, w_leaf_g = 0;       // ... on scenes read from HBM/L2 (0: auto)
    // pixels per work-counter fetch: bulk, and the cap of the launch-sized tail chunk (swept on
    // MI355X: profiles/r02/chunk_sweep.txt; 128 / 64 of round 1 left the counter at its atomic
    // throughput once sky tiles were decided at ring fill: 4K Cornell 1.01 -> 0.79 ms/frame)
    uint32_t chunk_pixels = 0, tail_chunk = 256;  // chunk_pixels 0: auto (512; 1024 pixel-major)
    uint32_t bulk_percent = 80;                // share of the frame handed out in bulk chunks
    int tile_major = -1;               // fused work order: -1 auto, 0 frame-major, 1 tile-major, 2 pixel-major
    int pf_sky = 1;                    // per-frame sky shortcut: 0 off, 1 large launches, 2 always
    int pf_defer = 2;                  // per-frame step launches through radiance slots + accumulation
                                       // (0 never, 1 always, 2 while the previous one still runs)
    uint32_t pf_defer_min = 4u << 20;  // ... (2) from this many work items per launch
    uint32_t pf_batch = rtk::kMaxFusedFrames;  // RT_TUNE_PERFRAME_BATCH: frames coalesced per launch
    int max_blocks = 0;                // persistent grid: workgroups per CU (0 = as many as fit)
    int global_oct = 1;                // scenes not in LDS: walk octant records in HBM/L2 (step;
                                       // bunny proxy 1.80 -> 1.58 ms/frame, profiles/r02/goct_sweep.txt)
    // wavefront schedule (refill at 32 free lanes: bunny proxy 2.62 -> 2.45 ms/frame,
    // profiles/r02/wavefront/sweep_bunny.txt)
    uint32_t wf_refill_min = 32, wf_streams_per_cu = 0, wf_top_limit = 256;  // streams 0: auto
    uint32_t query_refill_min = 32;    // ray queries: RT_TUNE_QUERY_REFILL_MIN
    // path tracing over caller rays (rt_trace.hpp), swept on MI355X at 4K, 9 bounces: refill at 8 free
    // lanes against the query's 32 (Cornell 2.17 -> 1.81 ms, bunny proxy 2.57 -> 2.54 ms); shading keeps
    // the step schedule's 48 (32 is 2 % faster on Cornell, 5 % slower on the proxy) -- profiles/trace/
    uint32_t trace_refill_min = 8, trace_shade_min = 48;
    // RT_TUNE_PATH_KILL: certified step launches drop paths of zero throughput (rt_path_kill.hpp);
    // 0 walks every segment -- same bits either way
    int path_kill = 1;
};

// RT_SUCCESS, or RT_INVALID_VALUE for an id the table does not hold (the retired ones and
// RT_TUNE_TOP_NODES among them) or a value outside the id's row: the setting then stays as it was
int tuning_set(Tuning& t, int param, int value);
int tuning_get(const Tuning& t, int param, int* value);

}  // namespace rtp

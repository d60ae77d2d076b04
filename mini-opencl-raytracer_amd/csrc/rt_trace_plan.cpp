// rt_trace_plan.cpp -- the plan of one path trace over caller rays (rt_trace_plan.hpp): the argument
// checks in the order rt_hip.h documents, the scene path and its LDS size, the 64-record units and
// the grid.  Pure arithmetic: a record traced twice or never, or a range that runs past a buffer,
// starts here, so it is kept where a CPU test can sweep it (tests/native/trace_plan_main.cpp).
#include "rt_trace_plan.hpp"

#include <algorithm>

#include "../../include/rt_status.h"
#include "rt_layout.hpp"
#include "rt_scene_pack.hpp"

namespace rtp {

int trace_check(const TraceIn& in) {
    if (!in.params_given) return RT_INVALID_VALUE;
    if (in.encoding != kTraceLinear && in.encoding != kTraceFrame0) return RT_INVALID_VALUE;
    // (each term first: their sum cannot wrap)
    if (in.first > kTraceMaxRecords || in.n > kTraceMaxRecords || in.first + in.n > kTraceMaxRecords)
        return RT_INVALID_VALUE;
    if (!in.rays_ok || !in.out_ok) return RT_INVALID_MEM_OBJECT;
    if (in.seeds_given && !in.seeds_ok) return RT_INVALID_MEM_OBJECT;
    if (in.out_is_input) return RT_INVALID_MEM_OBJECT;
    const uint64_t end = in.first + in.n;
    if (end > in.rays_bytes / kTraceRayBytes || end > in.out_bytes / kTraceResultBytes ||
        (in.seeds_given && end > in.seeds_bytes / kTraceSeedBytes))
        return RT_INVALID_BUFFER_SIZE;
    if (!in.scene_bound) return RT_INVALID_KERNEL_ARGS;
    if (!in.lights_set) return RT_INVALID_KERNEL_ARGS;
    return RT_SUCCESS;
}

int trace_shape(const TraceIn& in, TracePlan* out) {
    *out = TracePlan{};
    TracePlan& p = *out;
    const int rc = trace_check(in);
    if (rc) return rc;
    if (!in.oct_ok) return RT_INVALID_OPERATION;
    if (in.n == 0) {
        p.nothing = true;
        return RT_SUCCESS;
    }
    p.first = (uint32_t)in.first;
    p.count = (uint32_t)in.n;
    p.nUnits = (uint32_t)((in.n + 63u) / 64u);

    // LDS: octant node records (8 x 32 B per node), triangles and their shading records (48 B each),
    // material records (64 B), plus one {ray, seed} ring per wave
    const size_t rings = (rtk::kTraceThreads / 64) * (size_t)rtk::kTraceRingBytes;
    const size_t scene_bytes =
        (size_t)oct_records(in.n_nodes) * 16 + (size_t)in.n_tris * 96 + (size_t)in.n_mats * 64;
    const bool lds = !in.force_global && scene_bytes + rings <= kTraceLdsBudget;
    p.nNodes = in.n_nodes;
    p.octStride = oct_stride(in.n_nodes);
    p.octB = oct_b(in.n_nodes);
    p.octRecords = oct_records(in.n_nodes);
    if (!lds && RT_GOCT_GROUP && in.goct_available && in.goct_b) {
        // regrouped records, links as walk words (build_oct_nodes_grouped), as the query's walk
        p.regrouped = true;
        p.octStride = RT_GOCT_GROUP;
        p.octB = in.goct_b;
        p.octRecords = 2u * p.octB;
        p.nNodes = RT_GOCT_END_WORD ? rtk::kEndWalk : goct_word(in.n_nodes, RT_GOCT_GROUP);  // the END word
    }
    const rtk::Walk walk = lds ? (p.octB == rtk::kOctB ? rtk::Walk::LdsB : rtk::Walk::Lds) : rtk::Walk::GlobalOct;
    p.variant = rtk::Variant{0, in.math, walk, in.stats, false, false};
    // (the kernel's setting names the instance; nothing else of the plan depends on it)
    p.variant.shadow = in.shadow_rays;
    p.smem = (lds ? scene_bytes : 0) + rings;
    p.refillMin = in.tune.trace_refill_min;
    p.shadeMin = in.tune.trace_shade_min;
    // step weights: the render's, per scene path (rt_launch_plan.cpp)
    const Tuning& t = in.tune;
    p.stepWeightNode = lds ? t.w_node : t.w_node_g ? t.w_node_g : 65u;
    p.stepWeightLeaf = lds ? t.w_leaf : t.w_leaf_g ? t.w_leaf_g : t.w_leaf;
    return RT_SUCCESS;
}

void trace_grid(const TraceIn& in, int occ, TracePlan* out) {
    TracePlan& p = *out;
    const int per_cu = std::max(1, in.tune.max_blocks ? std::min(occ, in.tune.max_blocks) : occ);
    uint64_t grid = (uint64_t)per_cu * (uint64_t)std::max(1, in.num_cus);
    // one unit per wave at least: four waves per workgroup
    const uint64_t wg_waves = rtk::kTraceThreads / 64;
    grid = std::min<uint64_t>(grid, ((uint64_t)p.nUnits + wg_waves - 1) / wg_waves);
    p.grid = (uint32_t)std::max<uint64_t>(grid, 1);
}

}  // namespace rtp

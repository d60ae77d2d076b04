// rt_query_plan.cpp -- the plan of one ray query (rt_query_plan.hpp): the range check, the scene
// path and its LDS size, the 64-ray units and the grid.  Pure arithmetic: a ray answered twice or
// never, or a range that runs past a buffer, starts here, so it is kept where a CPU test can sweep
// it (tests/native/query_plan_main.cpp).  surface_plan: the checks and grid of the surface kernel
// (tests/native/surface_plan_main.cpp).
#include "rt_query_plan.hpp"

#include <algorithm>

#include "../../include/rt_status.h"
#include "rt_layout.hpp"
#include "rt_scene_pack.hpp"

namespace rtp {

int query_shape(const QueryIn& in, QueryPlan* out) {
    *out = QueryPlan{};
    QueryPlan& p = *out;
    if (in.mode != kQueryClosest && in.mode != kQueryAny) return RT_INVALID_VALUE;
    if (in.n_rays == 0) {  // nothing to answer, whatever the rest says
        p.nothing = true;
        return RT_SUCCESS;
    }
    // (each term first: their sum cannot wrap)
    if (in.first_ray > kQueryMaxRays || in.n_rays > kQueryMaxRays || in.first_ray + in.n_rays > kQueryMaxRays)
        return RT_INVALID_VALUE;
    if (in.same_buffer) return RT_INVALID_MEM_OBJECT;
    const uint64_t end = in.first_ray + in.n_rays;
    if (end > in.rays_bytes / 32u || end > in.hits_bytes / 16u) return RT_INVALID_BUFFER_SIZE;
    if (!in.oct_ok) return RT_INVALID_OPERATION;
    p.first = (uint32_t)in.first_ray;
    p.count = (uint32_t)in.n_rays;
    p.nUnits = (uint32_t)((in.n_rays + 63u) / 64u);

    // LDS: octant node records (8 x 32 B per node) and triangles (48 B) -- no shading records --
    // plus one ray ring per wave
    const size_t rings = (rtk::kQueryThreads / 64) * (size_t)rtk::kQueryRingBytes;
    const size_t scene_bytes = (size_t)oct_records(in.n_nodes) * 16 + (size_t)in.n_tris * 48;
    const bool lds = !in.force_global && scene_bytes + rings <= kQueryLdsBudget;
    p.nNodes = in.n_nodes;
    p.octStride = oct_stride(in.n_nodes);
    p.octB = oct_b(in.n_nodes);
    p.octRecords = oct_records(in.n_nodes);
    if (!lds && RT_GOCT_GROUP && in.goct_available && in.goct_b) {
        // regrouped records, links as walk words (build_oct_nodes_grouped), as the render's walk
        p.regrouped = true;
        p.octStride = RT_GOCT_GROUP;
        p.octB = in.goct_b;
        p.octRecords = 2u * p.octB;
        p.nNodes = RT_GOCT_END_WORD ? rtk::kEndWalk : goct_word(in.n_nodes, RT_GOCT_GROUP);  // the END word
    }
    const rtk::Walk walk = lds ? (p.octB == rtk::kOctB ? rtk::Walk::LdsB : rtk::Walk::Lds) : rtk::Walk::GlobalOct;
    p.variant = rtk::Variant{0, in.math, walk, in.stats, false, in.mode == kQueryAny};
    p.smem = (lds ? scene_bytes : 0) + rings;
    p.refillMin = in.tune.query_refill_min;
    // step weights: the render's, per scene path (rt_launch_plan.cpp)
    const Tuning& t = in.tune;
    p.stepWeightNode = lds ? t.w_node : t.w_node_g ? t.w_node_g : 65u;
    p.stepWeightLeaf = lds ? t.w_leaf : t.w_leaf_g ? t.w_leaf_g : t.w_leaf;
    return RT_SUCCESS;
}

void query_grid(const QueryIn& in, int occ, QueryPlan* out) {
    QueryPlan& p = *out;
    const int per_cu = std::max(1, in.tune.max_blocks ? std::min(occ, in.tune.max_blocks) : occ);
    uint64_t grid = (uint64_t)per_cu * (uint64_t)std::max(1, in.num_cus);
    // one unit per wave at least: eight waves per workgroup
    grid = std::min<uint64_t>(grid, ((uint64_t)p.nUnits + 7) / 8);
    p.grid = (uint32_t)std::max<uint64_t>(grid, 1);
}

int surface_plan(const SurfaceIn& in, SurfacePlan* out) {
    *out = SurfacePlan{};
    SurfacePlan& p = *out;
    // (each term first: their sum cannot wrap)
    if (in.first > kQueryMaxRays || in.n > kQueryMaxRays || in.first + in.n > kQueryMaxRays) return RT_INVALID_VALUE;
    if (!in.out_ok || in.out_is_input || in.rays_is_hits) return RT_INVALID_MEM_OBJECT;
    const uint64_t end = in.first + in.n;
    const uint64_t out_record = in.accumulate ? kFeatureBytes : kSurfaceBytes;
    if (end > in.rays_bytes / kRayBytes || end > in.hits_bytes / kHitBytes || end > in.out_bytes / out_record)
        return RT_INVALID_BUFFER_SIZE;
    if (!in.scene_bound) return RT_INVALID_KERNEL_ARGS;
    if (in.n == 0) {
        p.nothing = true;
        return RT_SUCCESS;
    }
    p.accumulate = in.accumulate;
    p.first = (uint32_t)in.first;
    p.count = (uint32_t)in.n;
    p.grid = (uint32_t)((in.n + rtk::kSurfaceThreads - 1) / rtk::kSurfaceThreads);  // <= 2^23
    return RT_SUCCESS;
}

}  // namespace rtp

// rt_tuning.cpp -- the table of rtKernelSetTuning's knobs (rt_tuning.hpp).
#include "rt_tuning.hpp"

#include <limits.h>

#include "../../include/rt_hip.h"

namespace rtp {

namespace {

// one row per RT_TUNE_*: the member (unsigned or signed), the accepted range, and the multiple a
// value must be of
struct Knob {
    int id;
    uint32_t Tuning::*u;
    int Tuning::*i;
    int lo, hi, multiple;
};

constexpr Knob kKnobs[] = {
    {RT_TUNE_REFILL_MIN, &Tuning::refill_min, nullptr, 1, 64, 1},  // (also sets refill_min_set, below)
    {RT_TUNE_SHADE_MIN, &Tuning::shade_min, nullptr, 1, 64, 1},
    {RT_TUNE_REFILL_MIN_GLOBAL, &Tuning::refill_min_g, nullptr, 0, 64, 1},
    {RT_TUNE_SHADE_MIN_GLOBAL, &Tuning::shade_min_g, nullptr, 0, 64, 1},
    {RT_TUNE_STEP_WEIGHT_NODE, &Tuning::w_node, nullptr, 1, 1000, 1},
    {RT_TUNE_STEP_WEIGHT_LEAF, &Tuning::w_leaf, nullptr, 1, 1000, 1},
    {RT_TUNE_STEP_WEIGHT_NODE_GLOBAL, &Tuning::w_node_g, nullptr, 0, 1000, 1},
    {RT_TUNE_STEP_WEIGHT_LEAF_GLOBAL, &Tuning::w_leaf_g, nullptr, 0, 1000, 1},
    {RT_TUNE_CHUNK_PIXELS, &Tuning::chunk_pixels, nullptr, 0, 4096, 64},  // (0: auto)
    {RT_TUNE_TAIL_CHUNK, &Tuning::tail_chunk, nullptr, 64, 4096, 64},
    {RT_TUNE_BULK_PERCENT, &Tuning::bulk_percent, nullptr, 0, 100, 1},
    {RT_TUNE_TILE_MAJOR, nullptr, &Tuning::tile_major, -1, 2, 1},
    {RT_TUNE_MAX_BLOCKS, nullptr, &Tuning::max_blocks, 0, 64, 1},
    {RT_TUNE_PERFRAME_SKY, nullptr, &Tuning::pf_sky, 0, 2, 1},
    {RT_TUNE_WF_REFILL_MIN, &Tuning::wf_refill_min, nullptr, 1, 64, 1},
    {RT_TUNE_WF_STREAMS_PER_CU, &Tuning::wf_streams_per_cu, nullptr, 0, 64, 1},
    {RT_TUNE_WF_TOP_NODES, &Tuning::wf_top_limit, nullptr, 0, 1024, 1},
    {RT_TUNE_GLOBAL_OCT, nullptr, &Tuning::global_oct, 0, 1, 1},
    {RT_TUNE_PERFRAME_DEFER, nullptr, &Tuning::pf_defer, 0, 2, 1},
    {RT_TUNE_PERFRAME_DEFER_MIN, &Tuning::pf_defer_min, nullptr, 0, INT_MAX, 1},  // any value >= 0
    {RT_TUNE_PERFRAME_BATCH, &Tuning::pf_batch, nullptr, 1, (int)rtk::kMaxFusedFrames, 1},
    {RT_TUNE_QUERY_REFILL_MIN, &Tuning::query_refill_min, nullptr, 1, 64, 1},
    {RT_TUNE_TRACE_REFILL_MIN, &Tuning::trace_refill_min, nullptr, 1, 64, 1},
    {RT_TUNE_TRACE_SHADE_MIN, &Tuning::trace_shade_min, nullptr, 1, 64, 1},
    {RT_TUNE_PATH_KILL, nullptr, &Tuning::path_kill, 0, 1, 1},
};

const Knob* find(int param) {
    for (const Knob& k : kKnobs)
        if (k.id == param) return &k;
    return nullptr;
}

}  // namespace

int tuning_set(Tuning& t, int param, int value) {
    const Knob* k = find(param);
    if (!k || value < k->lo || value > k->hi || value % k->multiple) return RT_INVALID_VALUE;
    if (k->u)
        t.*(k->u) = (uint32_t)value;
    else
        t.*(k->i) = value;
    if (param == RT_TUNE_REFILL_MIN) t.refill_min_set = true;
    return RT_SUCCESS;
}

int tuning_get(const Tuning& t, int param, int* value) {
    const Knob* k = find(param);
    if (!k) return RT_INVALID_VALUE;
    *value = k->u ? (int)(t.*(k->u)) : t.*(k->i);
    return RT_SUCCESS;
}

}  // namespace rtp

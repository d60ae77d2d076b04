// rt_adaptive_plan.cpp -- the plans of the adaptive-sampling calls (rt_adaptive_plan.hpp): the argument
// checks in their documented order (the fused sample's too: sample_check), the grids and the select's scratch layout.  Pure arithmetic,
// kept where a CPU test can sweep it (tests/native/adaptive_plan_main.cpp).
#include "rt_adaptive_plan.hpp"

#include <cmath>

#include "../../include/rt_status.h"

namespace rtp {

namespace {

// first + n <= 2^31, without wrapping
bool range_ok(uint64_t first, uint64_t n) {
    return first <= kAdaptiveMaxRecords && n <= kAdaptiveMaxRecords && first + n <= kAdaptiveMaxRecords;
}
// records [first, first + n) lie inside `bytes` at `size` bytes each (range_ok holds)
bool range_inside(uint64_t first, uint64_t n, uint64_t bytes, uint32_t size) { return first + n <= bytes / size; }

// width * height in (0, 2^31], each factor first so that the product cannot wrap
bool image_ok(uint64_t w, uint64_t h) {
    return w != 0 && h != 0 && w <= kAdaptiveMaxRecords && h <= kAdaptiveMaxRecords && w * h <= kAdaptiveMaxRecords;
}

// (every comparison is false for a NaN, so the finite test comes first)
bool param_ok(float f) { return std::isfinite(f) && f >= 0.0f && f <= kAdaptiveMaxParam; }

uint32_t groups(uint64_t n, uint32_t per) { return (uint32_t)((n + per - 1) / per); }
uint64_t align16(uint64_t b) { return (b + 15u) & ~(uint64_t)15u; }

}  // namespace

int accumulate_plan(const AccumIn& in, AccumPlan* out) {
    *out = AccumPlan{};
    if (!range_ok(in.first, in.n)) return RT_INVALID_VALUE;
    if (in.n_pixels == 0 || in.n_pixels > kAdaptiveMaxRecords) return RT_INVALID_VALUE;
    if (!in.results_ok || !in.stats_ok || (in.ids_given && !in.ids_ok)) return RT_INVALID_MEM_OBJECT;
    if (in.stats_is_input) return RT_INVALID_MEM_OBJECT;
    if (in.ids_given && !range_inside(in.first, in.n, in.ids_bytes, kIdBytes)) return RT_INVALID_BUFFER_SIZE;
    if (!range_inside(in.first, in.n, in.results_bytes, kSampleBytes)) return RT_INVALID_BUFFER_SIZE;
    if (in.n_pixels > in.stats_bytes / kStatsBytes) return RT_INVALID_BUFFER_SIZE;
    out->nothing = in.n == 0;
    out->first = (uint32_t)in.first, out->count = (uint32_t)in.n, out->n_pixels = (uint32_t)in.n_pixels;
    out->grid = groups(in.n, kAdaptiveThreads);
    return RT_SUCCESS;
}

int select_plan(const SelectIn& in, SelectPlan* out) {
    *out = SelectPlan{};
    SelectPlan& p = *out;
    if (!in.params_ok) return RT_INVALID_VALUE;
    if (!param_ok(in.threshold) || !param_ok(in.floor_y)) return RT_INVALID_VALUE;
    if (in.min_samples > in.max_samples) return RT_INVALID_VALUE;
    if (in.max_samples == 0 || in.max_samples > kAdaptiveMaxSamples) return RT_INVALID_VALUE;
    if (in.radius > kAdaptiveMaxRadius) return RT_INVALID_VALUE;
    if (!image_ok(in.width, in.height)) return RT_INVALID_VALUE;
    if (!in.stats_ok || !in.ids_ok || !in.result_ok || in.aliased) return RT_INVALID_MEM_OBJECT;
    const uint64_t pixels = in.width * in.height;
    if (pixels > in.stats_bytes / kStatsBytes || pixels > in.ids_bytes / kIdBytes || in.result_bytes < kSelectResultBytes)
        return RT_INVALID_BUFFER_SIZE;
    p.width = (uint32_t)in.width, p.height = (uint32_t)in.height, p.pixels = (uint32_t)pixels;
    p.threshold = in.threshold, p.floor_y = in.floor_y;
    p.min_samples = (float)in.min_samples, p.max_samples = (float)in.max_samples;  // exact: at most 2^20
    p.radius = in.radius;
    p.blocks = groups(pixels, kSelectBlockPixels);  // at most 2^21
    p.scan_passes = groups(p.blocks, kScanThreads);
    p.flags_offset = 0;
    p.sel_offset = align16(pixels);
    p.counts_offset = p.sel_offset + align16(pixels);
    p.scratch_bytes = p.counts_offset + align16((uint64_t)p.blocks * 12u);
    return RT_SUCCESS;
}

int paths_for_plan(const PathsForIn& in, PathsForPlan* out) {
    *out = PathsForPlan{};
    if (!in.slots_set || in.width == 0 || in.height == 0) return RT_INVALID_KERNEL_ARGS;
    if (!range_ok(in.first, in.n)) return RT_INVALID_VALUE;
    if (!in.ids_ok || !in.rays_ok || !in.seeds_ok || in.aliased) return RT_INVALID_MEM_OBJECT;
    if (!range_inside(in.first, in.n, in.ids_bytes, kIdBytes) || !range_inside(in.first, in.n, in.rays_bytes, kPathRayBytes) ||
        !range_inside(in.first, in.n, in.seeds_bytes, kPathSeedBytes))
        return RT_INVALID_BUFFER_SIZE;
    out->nothing = in.n == 0;
    out->first = (uint32_t)in.first, out->count = (uint32_t)in.n;
    out->grid = groups(in.n, kAdaptiveThreads);
    return RT_SUCCESS;
}

int sample_check(const SampleIn& in, SamplePlan* out) {
    *out = SamplePlan{};
    if (!range_ok(in.first, in.n)) return RT_INVALID_VALUE;
    if (in.n_pixels == 0 || in.n_pixels > kAdaptiveMaxRecords) return RT_INVALID_VALUE;
    if (!in.ids_ok || !in.stats_ok || (in.count_given && !in.count_ok) || in.aliased) return RT_INVALID_MEM_OBJECT;
    if (!range_inside(in.first, in.n, in.ids_bytes, kIdBytes)) return RT_INVALID_BUFFER_SIZE;
    if (in.count_given && in.count_bytes < kSelectResultBytes) return RT_INVALID_BUFFER_SIZE;
    if (in.n_pixels > in.stats_bytes / kStatsBytes) return RT_INVALID_BUFFER_SIZE;
    if (!in.slots_set || in.width == 0 || in.height == 0) return RT_INVALID_KERNEL_ARGS;
    if (!in.scene_bound || !in.lights_set) return RT_INVALID_KERNEL_ARGS;
    out->nothing = in.n == 0;
    out->first = (uint32_t)in.first, out->n = (uint32_t)in.n, out->n_pixels = (uint32_t)in.n_pixels;
    return RT_SUCCESS;
}

int resolve_plan(const ResolveIn& in, ResolvePlan* out) {
    *out = ResolvePlan{};
    if (!image_ok(in.width, in.height)) return RT_INVALID_VALUE;
    if (!in.stats_ok || !in.out_ok || in.out_is_input) return RT_INVALID_MEM_OBJECT;
    const uint64_t pixels = in.width * in.height;
    if (pixels > in.stats_bytes / kStatsBytes || pixels > in.out_bytes / kResolvedBytes) return RT_INVALID_BUFFER_SIZE;
    out->pixels = (uint32_t)pixels;
    out->grid = groups(pixels, kAdaptiveThreads);
    return RT_SUCCESS;
}

}  // namespace rtp

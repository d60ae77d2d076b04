// rt_adaptive_plan.hpp -- how the adaptive-sampling calls (rtEnqueueAccumulateSamples, rtEnqueueSelectPixels,
// rtEnqueueCameraPathsFor, rtEnqueueResolveSamples and the fused rtEnqueueSamplePixels) are checked and launched,
// as pure functions of plain values (rt_adaptive_plan.cpp): no HIP, no allocation, no globals.  The C ABI
// fills an *In, calls the plan and launches the kernels of rt_adaptive.hip (the indexed camera paths:
// rt_trace.hpp) with the plan's grids.
//
// The select's shape.  Block b of the three per-pixel kernels takes pixels [b * kSelectBlockPixels,
// (b + 1) * kSelectBlockPixels): kSelectThreads threads, kSelectPixelsPerThread rounds; in round i a
// thread takes pixel b * kSelectBlockPixels + i * kSelectThreads + thread, so a wave's 64 lanes hold 64
// consecutive pixels and ascending pixel order is (round, wave, lane).  The block counts are scanned by
// ONE workgroup of kScanThreads threads, kScanThreads counts per pass with a carry between passes: an
// image of more than kSelectBlockPixels * kScanThreads = 262,144 pixels takes more than one pass.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "rt_trace_plan.hpp"

namespace rtp {

constexpr uint64_t kAdaptiveMaxRecords = 1ull << 31;  // of a range's end, n_pixels and width * height
constexpr uint32_t kStatsBytes = 32, kIdBytes = 4, kSampleBytes = 16, kResolvedBytes = 16, kSelectResultBytes = 16;
constexpr uint32_t kPathRayBytes = 32, kPathSeedBytes = 4;
constexpr float kAdaptiveMaxParam = 0x1p20f;          // of threshold and floor_y
constexpr uint32_t kAdaptiveMaxSamples = 1u << 20;    // of max_samples
constexpr uint32_t kAdaptiveMaxRadius = 2;

constexpr uint32_t kAdaptiveThreads = 256;            // accumulate, resolve, indexed camera paths: a record per thread
constexpr uint32_t kSelectThreads = 256, kSelectPixelsPerThread = 4;
constexpr uint32_t kSelectBlockPixels = kSelectThreads * kSelectPixelsPerThread;
constexpr uint32_t kScanThreads = 256;                // counts per pass of the single scanning workgroup

// ---- rtEnqueueAccumulateSamples ------------------------------------------------------------------
struct AccumIn {
    uint64_t first, n, n_pixels;
    bool ids_given, ids_ok;            // the handle is not NULL; it is a buffer of this context
    bool results_ok, stats_ok;
    bool stats_is_input;               // `stats` is `ids` or `results`
    uint64_t ids_bytes, results_bytes, stats_bytes;
};
struct AccumPlan {
    bool nothing;                      // n == 0: no launch
    uint32_t first, count, n_pixels;
    uint32_t grid;                     // workgroups of kAdaptiveThreads
};
// RT_SUCCESS, or, in this order: RT_INVALID_VALUE (first + n > 2^31; n_pixels 0 or > 2^31),
// RT_INVALID_MEM_OBJECT (results or stats not a buffer of the context; a given ids that is not; stats
// one of the inputs), RT_INVALID_BUFFER_SIZE (the range beyond ids or results; stats below 32 B per pixel).
int accumulate_plan(const AccumIn& in, AccumPlan* out);

// ---- rtEnqueueSelectPixels -----------------------------------------------------------------------
struct SelectIn {
    bool params_ok;                    // params != NULL
    float threshold, floor_y;
    uint32_t min_samples, max_samples, radius;
    uint64_t width, height;
    bool stats_ok, ids_ok, result_ok;
    bool aliased;                      // ids or result is stats, or ids is result
    uint64_t stats_bytes, ids_bytes, result_bytes;
};
struct SelectPlan {
    uint32_t width, height, pixels;    // pixels <= 2^31
    float threshold, floor_y, min_samples, max_samples;  // the two counts as the floats they are compared as
    uint32_t radius;
    uint32_t blocks;                   // workgroups of the per-pixel kernels; the scan is one workgroup
    uint32_t scan_passes;
    // the scratch: two byte planes of `pixels` (hot flag + count rule; selected) and three words per
    // block (selected count, hot count, offset), each part 16-B aligned
    uint64_t flags_offset, sel_offset, counts_offset, scratch_bytes;
};
// RT_SUCCESS, or, in this order: RT_INVALID_VALUE (params NULL; threshold or floor_y negative, not finite
// or above 2^20; min_samples > max_samples; max_samples 0 or above 2^20; radius > 2; width or height zero;
// width * height > 2^31), RT_INVALID_MEM_OBJECT (a buffer not the context's; two of them the same),
// RT_INVALID_BUFFER_SIZE (stats below 32 B per pixel, ids below 4 B per pixel, result below 16 B).
int select_plan(const SelectIn& in, SelectPlan* out);

// ---- rtEnqueueCameraPathsFor ---------------------------------------------------------------------
struct PathsForIn {
    bool slots_set;                    // WIDTH, HEIGHT, FRAME_COUNT and the three camera slots
    uint32_t width, height;            // k's slots (looked at only when set)
    uint64_t first, n;
    bool ids_ok, rays_ok, seeds_ok;
    bool aliased;                      // rays or seeds is ids, or rays is seeds
    uint64_t ids_bytes, rays_bytes, seeds_bytes;
};
struct PathsForPlan {
    bool nothing;
    uint32_t first, count;
    uint32_t grid;                     // workgroups of kAdaptiveThreads
};
// RT_SUCCESS, or, in this order: RT_INVALID_KERNEL_ARGS (a slot unset; WIDTH or HEIGHT zero),
// RT_INVALID_VALUE (first + n > 2^31), RT_INVALID_MEM_OBJECT, RT_INVALID_BUFFER_SIZE (the range beyond
// ids, rays or seeds: 4, 32 and 4 B per record).
int paths_for_plan(const PathsForIn& in, PathsForPlan* out);

// ---- rtEnqueueResolveSamples ---------------------------------------------------------------------
struct ResolveIn {
    uint64_t width, height;
    bool stats_ok, out_ok;
    bool out_is_input;
    uint64_t stats_bytes, out_bytes;
};
struct ResolvePlan {
    uint32_t pixels;                   // <= 2^31
    uint32_t grid;                     // workgroups of kAdaptiveThreads
};
// RT_SUCCESS, or, in this order: RT_INVALID_VALUE (width or height zero; width * height > 2^31),
// RT_INVALID_MEM_OBJECT (a buffer not the context's; out is stats), RT_INVALID_BUFFER_SIZE (stats below
// 32 B per pixel, out below 16 B).
int resolve_plan(const ResolveIn& in, ResolvePlan* out);

// ---- rtEnqueueSamplePixels ------------------------------------------------------------------------
// One launch of the trace's kernel shape (rt_sample.hpp) over the records ids[first, first + m), m = n or
// min(n, the device count): the checks are this call's, the variant, the LDS size and the grid are the
// trace's (trace_shape / trace_grid) with n as the capacity.
struct SampleIn {
    uint64_t first, n, n_pixels;
    bool ids_ok, stats_ok;             // not NULL and a buffer of this context
    bool count_given, count_ok;        // `count` is not NULL; ... and a buffer of this context
    bool aliased;                      // stats is ids or count, or count is ids
    uint64_t ids_bytes, count_bytes, stats_bytes;
    bool slots_set;                    // WIDTH, HEIGHT, FRAME_COUNT and the three camera slots
    uint32_t width, height;            // k's slots (looked at only when set)
    bool scene_bound;                  // scene, node and material slots are bound
    bool lights_set;                   // LIGHT_BOUNCES, LIGHT_TYPE and SKYBOX_INTENSITY are set
    // the kernel's settings and its packed scene, as rtEnqueueTracePaths fills them (sample_shape; the
    // call's own fields of it are not looked at)
    TraceIn scene;
};
struct SamplePlan {
    bool nothing;                      // n == 0: no preparation, no launch
    uint32_t first, n, n_pixels;
    uint32_t capUnits;                 // 64-record units of n: the most the device count can leave
    TracePlan trace;                   // variant, LDS bytes, walk records, thresholds, grid
};
// The rows that need no packed scene, in this order: RT_INVALID_VALUE (first + n > 2^31; n_pixels 0 or >
// 2^31), RT_INVALID_MEM_OBJECT (ids or stats not a buffer of the context; a given count that is not; two of
// them the same), RT_INVALID_BUFFER_SIZE (the range beyond ids; count below 16 B; stats below 32 B per
// pixel), RT_INVALID_KERNEL_ARGS (a camera slot unset; WIDTH or HEIGHT zero; scene, node or material slot
// unbound; a light slot unset).  RT_SUCCESS otherwise, out->nothing when n == 0.
int sample_check(const SampleIn& in, SamplePlan* out);

// After the scene's preparation: sample_check, then trace_shape's RT_INVALID_OPERATION (a leaf of more than
// 127 triangles) and everything up to the LDS size.  Inline, like sample_grid: they call into
// rt_trace_plan.cpp, which the programs that link rt_adaptive_plan.cpp alone do not.
inline TraceIn sample_trace_in(const SampleIn& in) {
    TraceIn t = in.scene;
    t.params_given = true, t.encoding = kTraceLinear;
    t.first = in.first, t.n = in.n;
    t.rays_ok = t.out_ok = true, t.seeds_given = t.seeds_ok = false, t.out_is_input = false;
    t.rays_bytes = t.out_bytes = ~0ull, t.seeds_bytes = 0;  // (no such buffers: the range was checked against ids)
    t.scene_bound = in.scene_bound, t.lights_set = in.lights_set;
    return t;
}
inline int sample_shape(const SampleIn& in, SamplePlan* out) {
    int rc = sample_check(in, out);
    if (rc || out->nothing) return rc;
    rc = trace_shape(sample_trace_in(in), &out->trace);
    if (rc) return rc;
    out->capUnits = out->trace.nUnits;
    return 0;
}
// The grid, from the occupancy (workgroups per CU) of the kernel sample_shape chose at its LDS size.
inline void sample_grid(const SampleIn& in, int occ, SamplePlan* out) { trace_grid(sample_trace_in(in), occ, &out->trace); }
inline int sample_plan(const SampleIn& in, int occ, SamplePlan* out) {
    const int rc = sample_shape(in, out);
    if (rc == 0 && !out->nothing) sample_grid(in, occ, out);
    return rc;
}

}  // namespace rtp

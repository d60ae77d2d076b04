// rt_adaptive.hpp -- the adaptive-sampling kernels' arguments and launches (rt_adaptive.hip): the
// sample accumulation, the select (flags, count, scan, scatter) and the resolve.  The indexed camera
// paths are a kernel of the math policies (rt_trace.hpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_adaptive_math.hpp"
#include "rt_adaptive_plan.hpp"

namespace rta {

struct AccumArgs {
    const uint32_t* ids;      // null: record i is pixel i
    const float4* results;    // rt_path_result records {radiance.xyz, prim}
    float4* stats;            // rt_pixel_stats as 2 x float4
    uint32_t first, count, n_pixels;
};
hipError_t launch_accumulate(const AccumArgs& a, const rtp::AccumPlan& p, hipStream_t st);

struct SelectArgs {
    const float4* stats;
    uint32_t* ids;
    uint4* result;
    uint8_t* scratch;         // rtp::SelectPlan::scratch_bytes, 16-B aligned
};
hipError_t launch_select(const SelectArgs& a, const rtp::SelectPlan& p, hipStream_t st);

struct ResolveArgs {
    const float4* stats;
    float4* out;
};
hipError_t launch_resolve(const ResolveArgs& a, const rtp::ResolvePlan& p, hipStream_t st);

}  // namespace rta

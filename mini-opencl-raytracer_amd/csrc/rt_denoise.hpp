// rt_denoise.hpp -- one iteration of the feature-guided a-trous filter (rt_denoise.hip), launched by
// rtEnqueueDenoise (rt_capi.cpp) per step of rtp::denoise_plan (rt_denoise_plan.hpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_denoise_plan.hpp"

namespace rtd {

struct DenoiseArgs {
    const float4* src;       // this iteration's input colours {r, g, b, w}: width * height slots
    const float4* features;  // rt_pixel_features as two float4 per pixel: {albedo, depth}, {normal, coverage}
    float4* dst;             // never src or features
    uint32_t width, height;
    uint32_t tilesX, tilesPerClass;
    uint32_t terms;          // rtp::DenoiseTerm bits
    float invC, invN, invZ, invA;
};

// The kernel of `step` over t.grid workgroups on `st`.  hipErrorInvalidValue for a step the kernels
// are not built for or a tile shape other than theirs: nothing is launched.
hipError_t launch_denoise(const DenoiseArgs& a, const rtp::DenoiseStep& t, hipStream_t st);

}  // namespace rtd

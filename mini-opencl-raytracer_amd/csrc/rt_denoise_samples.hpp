// rt_denoise_samples.hpp -- one iteration of the variance-guided a-trous filter over the adaptive sample
// statistics (rt_denoise_samples.hip), launched by rtEnqueueDenoiseSamples (rt_capi.cpp) per step of
// rtp::denoise_samples_plan (rt_denoise_plan.hpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_denoise_plan.hpp"

namespace rtd {

struct DenoiseSamplesArgs {
    const float4* stats;     // rt_pixel_stats as two float4 per pixel: staged by the first iteration, n read by the last
    const float4* src;       // a later iteration's input {r, g, b, v}: width * height slots (not read by the first)
    const float4* features;  // rt_pixel_features as two float4 per pixel: {albedo, depth}, {normal, coverage}
    float4* dst;             // never an input
    float* variance;         // the last iteration's variance plane, or null
    uint32_t width, height;
    uint32_t tilesX, tilesPerClass;
    uint32_t terms;          // rtp::DenoiseTerm bits (rtp::kDenoiseLuminance for the luminance term)
    uint32_t last;           // the last iteration: dst receives {enc(rgb), n}
    int encoding;            // rtp::kDenoiseLinear / kDenoiseGamma
    float sigmaL, epsilon;
    float invN, invZ, invA;
};

// The kernel of `step` over t.grid workgroups on `st`; `first`: it stages from the statistics.
// hipErrorInvalidValue for a step the kernels are not built for, a first iteration at another step than 1
// or a tile shape other than theirs: nothing is launched.
hipError_t launch_denoise_samples(const DenoiseSamplesArgs& a, const rtp::DenoiseStep& t, bool first, hipStream_t st);

}  // namespace rtd

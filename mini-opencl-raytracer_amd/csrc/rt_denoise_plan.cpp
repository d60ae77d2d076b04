// rt_denoise_plan.cpp -- the plans of one denoise (rt_denoise_plan.hpp; denoise_plan for rtEnqueueDenoise,
// denoise_samples_plan for rtEnqueueDenoiseSamples, over the same tiles): the argument checks in their
// documented order, the fp32 constants of every iteration, which buffer each iteration reads and
// writes, and the tiles.  Pure arithmetic: a pixel filtered twice or never, a tap outside the staged
// block or a write past a buffer starts here, so it is kept where a CPU test can sweep it
// (tests/native/denoise_plan_main.cpp, tests/native/denoise_samples_plan_main.cpp).
#include "rt_denoise_plan.hpp"

#include <cmath>
#include <initializer_list>

#include "../../include/rt_status.h"

namespace rtp {

namespace {

// 0 disables the term; otherwise [2^-20, 2^20]
bool sigma_ok(float s) { return s == 0.0f || (std::isfinite(s) && s >= kDenoiseSigmaMin && s <= kDenoiseSigmaMax); }

float inv_sq(float s) { return s == 0.0f ? 0.0f : 1.0f / (s * s); }

// iteration i of n: the step, the buffers and the tiles (inv_c is the caller's)
void fill_step(DenoiseStep* step, unsigned i, unsigned n, int src, uint64_t width, uint64_t height) {
    DenoiseStep& t = *step;
    t.step = 1u << i;
    // the last iteration lands in `out`, and the buffers alternate backwards from it
    t.dst = (n - 1 - i) % 2 == 0 ? kDenoiseOut : kDenoiseScratch;
    t.src = src;
    t.rows = denoise_rows(t.step);
    t.stage_w = kDenoiseTileW + 4 * t.step, t.stage_h = t.rows + 4;
    t.lds_bytes = t.stage_w * t.stage_h * kDenoiseCellBytes + kDenoisePadBytes;
    t.tiles_x = (uint32_t)((width + kDenoiseTileW - 1) / kDenoiseTileW);
    t.classes = (uint32_t)(height < t.step ? height : t.step);
    const uint64_t class_rows = (height + t.step - 1) / t.step;  // of class 0, the longest
    t.tiles_per_class = (uint32_t)((class_rows + t.rows - 1) / t.rows);
    // <= (w / 64 + 1) (h / 4 + 16) with w h <= 2^31: below 2^31
    t.grid = (uint32_t)((uint64_t)t.tiles_x * t.classes * t.tiles_per_class);
}

}  // namespace

int denoise_plan(const DenoiseIn& in, DenoisePlan* out) {
    *out = DenoisePlan{};
    DenoisePlan& p = *out;
    if (!in.params_ok) return RT_INVALID_VALUE;
    if (in.iterations < 1 || in.iterations > kDenoiseMaxIterations) return RT_INVALID_VALUE;
    for (float s : {in.sigma_color, in.sigma_normal, in.sigma_depth, in.sigma_albedo})
        if (!sigma_ok(s)) return RT_INVALID_VALUE;
    if (in.width == 0 || in.height == 0) return RT_INVALID_VALUE;
    // (each factor first: their product cannot wrap)
    if (in.width > kDenoiseMaxPixels || in.height > kDenoiseMaxPixels || in.width * in.height > kDenoiseMaxPixels)
        return RT_INVALID_VALUE;
    if (!in.image_ok || !in.features_ok || !in.out_ok || in.out_is_input) return RT_INVALID_MEM_OBJECT;
    const uint64_t pixels = in.width * in.height;
    if (pixels > in.image_bytes / kDenoisePixelBytes || pixels > in.features_bytes / kDenoiseFeatureBytes ||
        pixels > in.out_bytes / kDenoisePixelBytes)
        return RT_INVALID_BUFFER_SIZE;

    p.iterations = in.iterations;
    p.width = (uint32_t)in.width, p.height = (uint32_t)in.height;
    p.scratch_pixels = in.iterations >= 2 ? pixels : 0;
    p.terms = (in.sigma_color != 0.0f ? kDenoiseColor : 0) | (in.sigma_normal != 0.0f ? kDenoiseNormal : 0) |
              (in.sigma_depth != 0.0f ? kDenoiseDepth : 0) | (in.sigma_albedo != 0.0f ? kDenoiseAlbedo : 0);
    p.inv_n = inv_sq(in.sigma_normal), p.inv_z = inv_sq(in.sigma_depth), p.inv_a = inv_sq(in.sigma_albedo);
    for (unsigned i = 0; i < in.iterations; ++i) {
        fill_step(&p.it[i], i, in.iterations, i == 0 ? kDenoiseImage : p.it[i - 1].dst, in.width, in.height);
        p.it[i].inv_c = inv_sq(std::ldexp(in.sigma_color, -(int)i));  // the colour tolerance halves per iteration
    }
    return RT_SUCCESS;
}

int denoise_samples_plan(const DenoiseSamplesIn& in, DenoiseSamplesPlan* out) {
    *out = DenoiseSamplesPlan{};
    DenoiseSamplesPlan& p = *out;
    if (!in.params_ok) return RT_INVALID_VALUE;
    if (in.iterations < 1 || in.iterations > kDenoiseMaxIterations) return RT_INVALID_VALUE;
    for (float s : {in.sigma_luminance, in.sigma_normal, in.sigma_depth, in.sigma_albedo})
        if (!sigma_ok(s)) return RT_INVALID_VALUE;
    if (!(std::isfinite(in.epsilon) && in.epsilon >= kDenoiseEpsilonMin && in.epsilon <= kDenoiseEpsilonMax))
        return RT_INVALID_VALUE;
    if (in.encoding != kDenoiseLinear && in.encoding != kDenoiseGamma) return RT_INVALID_VALUE;
    if (in.width == 0 || in.height == 0) return RT_INVALID_VALUE;
    // (each factor first: their product cannot wrap)
    if (in.width > kDenoiseMaxPixels || in.height > kDenoiseMaxPixels || in.width * in.height > kDenoiseMaxPixels)
        return RT_INVALID_VALUE;
    if (!in.stats_ok || !in.features_ok || !in.out_ok || (in.variance_given && !in.variance_ok) || in.aliased)
        return RT_INVALID_MEM_OBJECT;
    const uint64_t pixels = in.width * in.height;
    if (pixels > in.stats_bytes / kDenoiseStatsBytes || pixels > in.features_bytes / kDenoiseFeatureBytes ||
        pixels > in.out_bytes / kDenoisePixelBytes || (in.variance_given && pixels > in.variance_bytes / kDenoiseVarianceBytes))
        return RT_INVALID_BUFFER_SIZE;

    p.iterations = in.iterations;
    p.width = (uint32_t)in.width, p.height = (uint32_t)in.height;
    p.scratch_pixels = in.iterations >= 2 ? pixels : 0;
    p.terms = (in.sigma_luminance != 0.0f ? kDenoiseLuminance : 0) | (in.sigma_normal != 0.0f ? kDenoiseNormal : 0) |
              (in.sigma_depth != 0.0f ? kDenoiseDepth : 0) | (in.sigma_albedo != 0.0f ? kDenoiseAlbedo : 0);
    p.sigma_luminance = in.sigma_luminance, p.epsilon = in.epsilon;
    p.inv_n = inv_sq(in.sigma_normal), p.inv_z = inv_sq(in.sigma_depth), p.inv_a = inv_sq(in.sigma_albedo);
    p.encoding = in.encoding;
    p.write_variance = in.variance_given;
    for (unsigned i = 0; i < in.iterations; ++i) {
        // (kDenoiseImage: the statistics, which only the first iteration stages from)
        fill_step(&p.it[i], i, in.iterations, i == 0 ? kDenoiseImage : p.it[i - 1].dst, in.width, in.height);
        p.first[i] = i == 0, p.last[i] = i + 1 == in.iterations;
    }
    return RT_SUCCESS;
}

}  // namespace rtp

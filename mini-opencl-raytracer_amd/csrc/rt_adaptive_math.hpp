// rt_adaptive_math.hpp -- the per-pixel pieces of adaptive sampling (include/rt_hip.h, "adaptive
// sampling"): the sample update of a pixel's statistics, the hot test, the selection rule over a window
// of hot flags, and the range tests that guard every index.  Plain host-and-device functions: the
// kernels (rt_adaptive.hip) and the CPU program tests/native/adaptive_plan_main.cpp compile this one
// text.  Every operation is one correctly rounded fp32 operation in the order rt_hip.h writes it
// (nothing contracted, IEEE division, comparisons false for a NaN).
#pragma once

#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RTA_FN __host__ __device__ inline
#else
#define RTA_FN inline
#endif

namespace rta {

// rt_pixel_stats as two 16-B halves: {sum.rgb, n} and {mean_y, m2_y, reserved[2]}
struct Moments {
    float n, mean_y, m2_y;
};

// a value read from an id buffer becomes an index only after this test
RTA_FN bool pixel_in_range(uint32_t p, uint32_t n_pixels) { return p < n_pixels; }

RTA_FN bool finite_channel(float c) { return fabsf(c) <= FLT_MAX; }  // false for a NaN
RTA_FN bool finite_sample(float r, float g, float b) { return finite_channel(r) && finite_channel(g) && finite_channel(b); }

RTA_FN float luminance(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// Welford's update of the luminance moments by one sample.  `div(a, b)` is the IEEE quotient a / b: a
// translation unit whose `/` is not that one (the shipped kernels') passes its own (rt_sample.hpp)
template <class Div>
RTA_FN Moments sample_update(Moments s, float y, Div div) {
    const float n1 = s.n + 1.0f;
    const float d = y - s.mean_y;
    const float mean1 = s.mean_y + div(d, n1);
    const float m21 = s.m2_y + d * (y - mean1);
    return Moments{n1, mean1, m21};
}
struct Quotient {
    RTA_FN float operator()(float a, float b) const { return a / b; }
};
RTA_FN Moments sample_update(Moments s, float y) { return sample_update(s, y, Quotient{}); }

// the variance of the mean luminance above (threshold * (mean + floor))^2; never with fewer than two samples
RTA_FN bool is_hot(Moments s, float threshold, float floor_y) {
    if (!(s.n >= 2.0f)) return false;
    const float v = (s.m2_y / (s.n - 1.0f)) / s.n;
    const float b = threshold * (s.mean_y + floor_y);
    return v > b * b;
}

// how a pixel's own count decides: selected whatever its window, never selected, or by its window
enum Rule : uint32_t { kByWindow = 0, kAlways = 1, kNever = 2 };
RTA_FN uint32_t count_rule(float n, float min_samples, float max_samples) {
    if (n < min_samples) return kAlways;
    if (n >= max_samples) return kNever;
    return kByWindow;
}
RTA_FN bool selected(uint32_t rule, bool any_hot) { return rule == kAlways || (rule == kByWindow && any_hot); }

// the flag byte of a pixel in the select's scratch plane: bit 0 hot, bits 1-2 the count's rule
RTA_FN uint8_t flag_byte(bool hot, uint32_t rule) { return (uint8_t)((hot ? 1u : 0u) | (rule << 1)); }
RTA_FN bool flag_hot(uint8_t f) { return (f & 1u) != 0u; }
RTA_FN uint32_t flag_rule(uint8_t f) { return (uint32_t)f >> 1; }

// the window [lo, hi] of coordinate c (c < size) with the given radius, clipped to [0, size - 1]
RTA_FN void window_range(uint32_t c, uint32_t size, uint32_t radius, uint32_t* lo, uint32_t* hi) {
    *lo = c >= radius ? c - radius : 0u;
    *hi = size - 1u - c >= radius ? c + radius : size - 1u;
}

// whether any flag in the Chebyshev window of pixel p = y * width + x is hot; `flags` holds width * height
// bytes, and every index formed here lies inside it (swept by adaptive_plan_main)
template <class Flags>
RTA_FN bool window_any_hot(const Flags& flags, uint32_t p, uint32_t width, uint32_t height, uint32_t radius) {
    const uint32_t y = p / width, x = p - y * width;
    uint32_t x0, x1, y0, y1;
    window_range(x, width, radius, &x0, &x1);
    window_range(y, height, radius, &y0, &y1);
    bool any = false;
    for (uint32_t yy = y0; yy <= y1; ++yy)
        for (uint32_t xx = x0; xx <= x1; ++xx) any = any || flag_hot(flags[(uint64_t)yy * width + xx]);
    return any;
}

}  // namespace rta

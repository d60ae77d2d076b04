// rt_denoise_samples_math.hpp -- the per-pixel pieces of the variance-guided denoiser (include/rt_hip.h,
// rtEnqueueDenoiseSamples): a statistics record as the {colour, variance of the mean} cell of iteration 0,
// the test that decides whether a cell counts, the luminance tolerance of a centre from the 3 x 3 Gaussian
// of the variance, the update of the sums by one tap, and the result of an iteration.  Plain
// host-and-device functions: the kernel (rt_denoise_samples.hip) and the CPU program
// tests/native/denoise_samples_plan_main.cpp compile this one text.  Every operation is one correctly
// rounded fp32 operation in the order rt_hip.h writes it (nothing contracted, IEEE division and square
// root, comparisons false for a NaN); taps that do not count and terms that are off are dropped by
// select, never by a multiplication.
#pragma once

#include <math.h>
#include <stdint.h>

#include "rt_adaptive_math.hpp"

namespace rtds {

// the colour plane's slot: linear radiance and, in w, the variance of the pixel's mean luminance
struct Cell {
    float r, g, b, v;
};

// a pixel's guides: rt_pixel_features
struct Guide {
    float ax, ay, az, depth;
    float nx, ny, nz, coverage;
};

// iteration 0's input from a statistics record {sum.rgb, n}, {mean_y, m2_y}: a single sample is taken to
// be as uncertain as it is bright, and a pixel without samples never counts
RTA_FN Cell stats_cell(float sum_r, float sum_g, float sum_b, float n, float mean_y, float m2_y) {
    if (!(n >= 1.0f)) return Cell{0.0f, 0.0f, 0.0f, -1.0f};
    const float v = n >= 2.0f ? (m2_y / (n - 1.0f)) / n : mean_y * mean_y;
    return Cell{sum_r / n, sum_g / n, sum_b / n, v};
}

// the one rule of every iteration, from the staged cell alone: false for a negative or NaN variance
RTA_FN bool counts(float coverage, float v) { return coverage != 0.0f && v >= 0.0f; }

RTA_FN float cell_luminance(const Cell& c) { return rta::luminance(c.r, c.g, c.b); }

// ---- the luminance tolerance of a centre: the 3 x 3 Gaussian of the variance at the tap spacing ----
struct TolSums {
    float sg, sv;
};
// g[d + 1], d = -1 .. 1
RTA_FN float tol_weight(int d) { return d == 0 ? 0.5f : 0.25f; }
RTA_FN TolSums tol_tap(TolSums s, float g, float v, bool counted) {
    const float sg = s.sg + g, sv = s.sv + g * v;
    return TolSums{counted ? sg : s.sg, counted ? sv : s.sv};
}
RTA_FN float tolerance(TolSums s, float sigma_luminance, float epsilon) {
    const float gv = s.sv / s.sg;
    return sigma_luminance * sqrtf(gv) + epsilon;
}

// ---- one tap ------------------------------------------------------------------------------------------
struct Terms {
    bool luminance, normal, depth, albedo;  // a term whose sigma is 0 is left out of the product
    float inv_n, inv_z, inv_a;              // 1 / sigma^2
};

struct Centre {
    Guide f;
    float lum;  // l(c_p)
    float tol;  // of this centre, once
    float rz;   // 1 / max(|depth_p|, 2^-64), once
};
RTA_FN Centre centre_of(const Cell& c, const Guide& f, float tol) {
    return Centre{f, cell_luminance(c), tol, 1.0f / fmaxf(fabsf(f.depth), 0x1p-64f)};
}

struct Sums {
    float w, r, g, b, v;
};

RTA_FN float dot3(float x, float y, float z) { return (x * x + y * y) + z * z; }
RTA_FN float edge(float x) {
    const float m = fmaxf(0.0f, 1.0f - x);
    return m * m;
}

// k: the tap's B3-spline weight.  `counted` false (a tap outside the image is staged with coverage 0):
// the sums come back as they were.
RTA_FN Sums tap_update(Sums s, float k, const Centre& p, const Cell& cq, const Guide& fq, const Terms& t, bool counted) {
    float w = k;
    const float wl = w * edge(fabsf(p.lum - cell_luminance(cq)) / p.tol);
    w = t.luminance ? wl : w;
    const float wn = w * edge(dot3(p.f.nx - fq.nx, p.f.ny - fq.ny, p.f.nz - fq.nz) * t.inv_n);
    w = t.normal ? wn : w;
    const float d = (p.f.depth - fq.depth) * p.rz;
    const float wz = w * edge((d * d) * t.inv_z);
    w = t.depth ? wz : w;
    const float wa = w * edge(dot3(p.f.ax - fq.ax, p.f.ay - fq.ay, p.f.az - fq.az) * t.inv_a);
    w = t.albedo ? wa : w;
    const Sums n{s.w + w, s.r + w * cq.r, s.g + w * cq.g, s.b + w * cq.b, s.v + (w * w) * cq.v};
    return Sums{counted ? n.w : s.w, counted ? n.r : s.r, counted ? n.g : s.g, counted ? n.b : s.b, counted ? n.v : s.v};
}

// rgb = s_rgb / sw, v' = s_v / (sw * sw)
RTA_FN Cell iteration_result(const Sums& s) { return Cell{s.r / s.w, s.g / s.w, s.b / s.w, s.v / (s.w * s.w)}; }

// the B3-spline weight h[d + 2], d = -2 .. 2: rtEnqueueDenoise's
RTA_FN float spline_weight(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

}  // namespace rtds

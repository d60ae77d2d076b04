// rt_reproject_math.hpp -- steps 5 and 6 of rtEnqueueReprojectSamples' definition (include/rt_hip.h):
// the test of a history tap, its per-sample quantities, the bilinear sums and the recombined record.
// Steps 2-4 of the projection and the surface test are rt_temporal_math.hpp's, compiled as they are.  The kernel
// (rt_reproject.hip) and a CPU program (tests/native/reproject_samples_plan_main.cpp, built with
// sanitizers) compile this same text on records that were already loaded: nothing here forms an address.
//
// Every operation is one fp32 operation in the definition's order; a tap that does not count is dropped
// by select, never by a multiplication, so the bytes of such a tap's statistics never reach an output.
#pragma once

#include <math.h>

#include "rt_temporal_math.hpp"

#if defined(__HIPCC__)
#define RT_RM_FN __host__ __device__ inline
#else
#define RT_RM_FN inline
#endif

namespace rtrs {

constexpr float kReprojectMinWeight = 0x1p-6f;  // step 6: the temporal pass's least sum of counted weights
constexpr float kReprojectMaxHistory = 0x1p20f;

// the fp32 fields of an rt_pixel_stats (reserved[2] takes no part)
struct Stats {
    float sum[3], n, mean_y, m2_y;
};

struct TapSums {
    float sw, sm[3], sy, ss, sn;
};

RT_RM_FN TapSums no_taps() { return TapSums{0.0f, {0.0f, 0.0f, 0.0f}, 0.0f, 0.0f, 0.0f}; }

using rtt::tap_on_surface;  // the features' part of a tap's test is the temporal pass's

// One tap with weight bw: counted when it is on the surface and holds at least one sample.
RT_RM_FN void add_tap(TapSums& t, bool on_surface, float bw, const Stats& s) {
    const bool counts = on_surface && s.n >= 1.0f;
    const float sv = s.n >= 2.0f ? s.m2_y / (s.n - 1.0f) : s.mean_y * s.mean_y;
    t.sw = counts ? t.sw + bw : t.sw;
    for (int c = 0; c < 3; ++c) {
        const float m = s.sum[c] / s.n;
        t.sm[c] = counts ? t.sm[c] + bw * m : t.sm[c];
    }
    t.sy = counts ? t.sy + bw * s.mean_y : t.sy;
    t.ss = counts ? t.ss + bw * sv : t.ss;
    t.sn = counts ? t.sn + bw * s.n : t.sn;
}

// Step 6.  False: nothing carried (the caller writes 32 zero bytes).
RT_RM_FN bool merge(const TapSums& t, float max_history, Stats* out) {
    if (!(t.sw >= kReprojectMinWeight)) return false;
    const float n = fminf(floorf(t.sn / t.sw), max_history);
    for (int c = 0; c < 3; ++c) out->sum[c] = (t.sm[c] / t.sw) * n;
    out->n = n;
    out->mean_y = t.sy / t.sw;
    out->m2_y = n >= 2.0f ? (t.ss / t.sw) * (n - 1.0f) : 0.0f;
    return true;
}

}  // namespace rtrs

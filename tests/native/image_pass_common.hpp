// image_pass_common.hpp -- what the stand-alone drivers of the image passes' plans share: the lane-by-lane walk
// of an a-trous iteration's tiles (denoise_plan_main.cpp, denoise_samples_plan_main.cpp) and the views of the
// reprojection plans (temporal_plan_main.cpp, reproject_samples_plan_main.cpp).  CPU only.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../mini-opencl-raytracer_amd/csrc/rt_denoise_plan.hpp"
#include "../../mini-opencl-raytracer_amd/csrc/rt_temporal_plan.hpp"

// One iteration's tiles walked lane by lane as the a-trous kernels map them (csrc/rt_atrous_tile.hpp): every pixel
// is filtered by exactly one lane and each of its 25 taps -- the 9 of a tolerance among them -- lies in a staged
// cell that holds the tap's coordinates.  False (with a message) on the first thing that breaks.
inline bool walk(const rtp::DenoiseStep& t, uint64_t W, uint64_t H, std::vector<uint8_t>& seen) {
    seen.assign(W * H, 0);
    const int64_t s = t.step;
    for (uint32_t b = 0; b < t.grid; ++b) {
        const uint32_t tx = b % t.tiles_x, rest = b / t.tiles_x;
        const uint32_t ty = rest % t.tiles_per_class, cls = rest / t.tiles_per_class;
        if (cls >= t.classes) return std::printf("class %u of %u\n", cls, t.classes), false;
        const int64_t x0 = (int64_t)tx * rtp::kDenoiseTileW, j0 = (int64_t)ty * t.rows;
        for (uint32_t j = 0; j < t.rows; ++j)
            for (uint32_t lx = 0; lx < rtp::kDenoiseTileW; ++lx) {
                const int64_t x = x0 + lx, y = cls + (j0 + j) * s;
                if (x >= (int64_t)W || y >= (int64_t)H) continue;
                if (++seen[y * W + x] != 1) return std::printf("pixel (%lld, %lld) twice\n", (long long)x, (long long)y), false;
                for (int dy = -2; dy <= 2; ++dy)
                    for (int dx = -2; dx <= 2; ++dx) {
                        const int64_t cx = lx + 2 * s + dx * s, cy = (int64_t)j + 2 + dy;
                        if (cx < 0 || cx >= t.stage_w || cy < 0 || cy >= t.stage_h)
                            return std::printf("tap (%d, %d) outside the staged block\n", dx, dy), false;
                        // the coordinates the staging loop gives that cell
                        const int64_t sx = x0 - 2 * s + cx, sy = cls + (j0 - 2 + cy) * s;
                        if (sx != x + dx * s || sy != y + dy * s) return std::printf("cell holds another pixel\n"), false;
                    }
            }
    }
    for (uint64_t i = 0; i < W * H; ++i)
        if (seen[i] != 1) return std::printf("pixel %llu filtered %d times\n", (unsigned long long)i, seen[i]), false;
    return true;
}

inline const rtp::TemporalView kDefaultView = {{0.0f, -25.0f, 8.5f}, {0.0f, 1.0f, 0.0f}, {0.0f, 0.0f, 1.0f}};

// (restated here, independently of the plan's own view_finite)
inline bool finite_view(const rtp::TemporalView& v) {
    for (int c = 0; c < 3; ++c)
        if (!std::isfinite(v.pos[c]) || !std::isfinite(v.front[c]) || !std::isfinite(v.up[c])) return false;
    return true;
}

// rt_atrous_tile.hpp -- what the two a-trous filters (rt_denoise.hip, rt_denoise_samples.hip) share: the
// tile of rtp::denoise_plan a workgroup filters, staged in LDS, and the choice of the kernel built for a
// plan's step.  The edge-stopping arithmetic and what a kernel writes are the kernels' own.
//
// A tile is 64 contiguous columns of kRows rows of one residue class y mod kStep.  It is staged with a
// halo of 2 taps -- (64 + 4 kStep) columns of kRows + 4 class rows -- as three float4 planes (colour;
// albedo, depth; normal, coverage) with 16-B loads whose lanes run along x; then every lane runs the taps
// of its pixels out of LDS: a tap is kStep cells along a staged row, or one staged row up or down.
// Cells outside the image are staged as zeros with coverage 0, so the rule by which a filter skips a
// tap that does not count skips them, and global indices are only ever formed from coordinates tested to
// lie inside the image.  Pixel values never reach an address.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "rt_denoise_plan.hpp"

namespace rtd {

constexpr int kTileW = (int)rtp::kDenoiseTileW, kThreads = (int)rtp::kDenoiseThreads;

template <int kStep>
struct AtrousTile {
    static constexpr int kRows = (int)rtp::denoise_rows(kStep);
    static constexpr int SW = kTileW + 4 * kStep, SH = kRows + 4, kCells = SW * SH;
    // the {normal, coverage} plane starts 4 cells on, so that a staging store's lane pairs (the two
    // halves of one feature record) fall into different banks
    static constexpr int kPlaneB = kCells + (int)rtp::kDenoisePadBytes / 16;
    static_assert((size_t)kCells * rtp::kDenoiseCellBytes + rtp::kDenoisePadBytes <= rtp::kDenoiseLdsBudget,
                  "staged block over the LDS budget");

    uint32_t tilesX, tilesPerClass, width, height;  // as the launch gave them

    // The workgroup's tile, from blockIdx.x.  (Each function below decodes it for itself from the launch's
    // own values and the decodes fold into one: handing the decoded values down instead, or running the
    // filter's rows behind a callable, costs registers -- denoise_atrous<1, false> went from 63 to 65.)
    struct Origin {
        uint32_t cls;    // the residue class y mod kStep
        int64_t W, H;
        int64_t x0, j0;  // the first column; the first row, counted within its class
    };
    __device__ __forceinline__ Origin origin() const {
        const uint32_t tx = blockIdx.x % tilesX, rest = blockIdx.x / tilesX;
        const uint32_t ty = rest % tilesPerClass, cls = rest / tilesPerClass;
        const int64_t W = width, H = height;
        const int64_t x0 = (int64_t)tx * kTileW;
        const int64_t j0 = (int64_t)ty * kRows;
        return Origin{cls, W, H, x0, j0};
    }

    // a shorter class's last tile: nothing to do (the whole workgroup)
    __device__ __forceinline__ bool empty() const {
        const Origin o = origin();
        return (int64_t)o.cls + o.j0 * kStep >= o.H;
    }

    // The colour plane sCol[kCells], lanes along x: load(p) is the cell of pixel p inside the image.
    template <class Load>
    __device__ __forceinline__ void stage_colours(float4* sCol, Load load) const {
        const Origin o = origin();
        for (int c = (int)threadIdx.x; c < kCells; c += kThreads) {
            const int cy = c / SW, cx = c - cy * SW;
            const int64_t x = o.x0 - 2 * kStep + cx, y = (int64_t)o.cls + (o.j0 - 2 + cy) * kStep;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (x >= 0 && x < o.W && y >= 0 && y < o.H) v = load((size_t)(y * o.W + x));
            sCol[c] = v;
        }
    }

    // The feature planes sFeat[kPlaneB + kCells], one 16-B load per lane: {albedo, depth} at c,
    // {normal, coverage} at kPlaneB + c.
    __device__ __forceinline__ void stage_features(float4* sFeat, const float4* features) const {
        const Origin o = origin();
        for (int f = (int)threadIdx.x; f < 2 * kCells; f += kThreads) {
            const int c = f >> 1, half = f & 1;
            const int cy = c / SW, cx = c - cy * SW;
            const int64_t x = o.x0 - 2 * kStep + cx, y = (int64_t)o.cls + (o.j0 - 2 + cy) * kStep;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // outside the image: coverage 0
            if (x >= 0 && x < o.W && y >= 0 && y < o.H) v = features[(size_t)(y * o.W + x) * 2 + half];
            sFeat[half * kPlaneB + c] = v;
        }
    }

    // the staged cell of the centre in tile row j, lane column lx
    static __device__ __forceinline__ int centre(int j, int lx) { return (j + 2) * SW + 2 * kStep + lx; }
    // the staged cell of tap (dx, dy) of the centre at cell cc
    static __device__ __forceinline__ int tap(int cc, int dx, int dy) { return cc + dy * SW + dx * kStep; }
};

// the tile shape of the kernels built for kStep
template <int kStep>
inline bool step_matches(const rtp::DenoiseStep& t) {
    return t.rows == rtp::denoise_rows(kStep) && t.stage_w == rtp::kDenoiseTileW + 4u * kStep && t.stage_h == t.rows + 4u;
}

// launch(std::integral_constant<int, kStep>) for the kStep of `t`.  hipErrorInvalidValue for a step the
// kernels are not built for or a tile shape other than theirs: `launch` is not called.
template <class Launch>
inline hipError_t for_step(const rtp::DenoiseStep& t, Launch launch) {
    auto at = [&](auto step) { return step_matches<decltype(step)::value>(t) ? launch(step) : hipErrorInvalidValue; };
    switch (t.step) {
        case 1: return at(std::integral_constant<int, 1>{});
        case 2: return at(std::integral_constant<int, 2>{});
        case 4: return at(std::integral_constant<int, 4>{});
        case 8: return at(std::integral_constant<int, 8>{});
        case 16: return at(std::integral_constant<int, 16>{});
        default: return hipErrorInvalidValue;
    }
}

}  // namespace rtd

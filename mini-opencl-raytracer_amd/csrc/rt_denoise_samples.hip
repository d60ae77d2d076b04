// rt_denoise_samples.hip -- the variance-guided a-trous filter of rtEnqueueDenoiseSamples (the
// edge-stopping function of SVGF, Schied et al. 2017, over the adaptive sample statistics), one launch
// per iteration.  The filter is defined operation by operation in include/rt_hip.h and restated in numpy
// by tests/denoise_samples_ref.py; the per-pixel arithmetic is rt_denoise_samples_math.hpp, the text a
// CPU program runs under sanitizers.  Every fp32 operation is one correctly rounded IEEE operation in the
// order written there (no contraction, denormals kept, IEEE division and square root -- the standard
// flags, never the shipped kernels' relaxed ones).
//
// The shape is rt_denoise.hip's: a workgroup filters one tile of rtp::denoise_samples_plan out of a block
// staged in LDS; the tile, its staging and its safety rules are rt_atrous_tile.hpp.  The colour plane's w
// slot carries the variance of the pixel's mean luminance, so a cell stays 48 B.  The first iteration
// stages straight from the 32-B statistics records (two 16-B loads per cell, lanes along x) and computes
// {colour, variance} on the way into LDS: there is no resolve pass.  A centre's luminance tolerance comes
// from the inner 3 x 3 of its own taps, which lie in the staged block at every step.  No value of `stats`
// or `features` reaches an address.
#include "rt_denoise_samples.hpp"

#include "../../include/rt_pinned_math.h"
#include "rt_atrous_tile.hpp"
#include "rt_denoise_samples_math.hpp"

#pragma clang fp contract(off)

namespace rtd {

namespace {

__device__ __forceinline__ rtds::Cell cell_of(float4 c) { return rtds::Cell{c.x, c.y, c.z, c.w}; }
__device__ __forceinline__ rtds::Guide guide_of(float4 a, float4 n) {
    return rtds::Guide{a.x, a.y, a.z, a.w, n.x, n.y, n.z, n.w};
}

// kFirst: the colours are staged from the statistics (step 1 only).  kAll: all four edge-stopping terms
// are on (a.terms is not looked at)
template <int kStep, bool kFirst, bool kAll>
__global__ __launch_bounds__(kThreads) void denoise_samples_atrous(DenoiseSamplesArgs a) {
    static_assert(!kFirst || kStep == 1, "the first iteration has step 1");
    using Tile = AtrousTile<kStep>;
    constexpr int kPlaneB = Tile::kPlaneB;
    __shared__ float4 sCol[Tile::kCells];
    __shared__ float4 sFeat[kPlaneB + Tile::kCells];
    const Tile tile{a.tilesX, a.tilesPerClass, a.width, a.height};
    const typename Tile::Origin org = tile.origin();
    if (tile.empty()) return;
    tile.stage_colours(sCol, [&](size_t p) {
        if (!kFirst) return a.src[p];
        const float4 lo = a.stats[2 * p], hi = a.stats[2 * p + 1];
        const rtds::Cell s = rtds::stats_cell(lo.x, lo.y, lo.z, lo.w, hi.x, hi.y);
        return make_float4(s.r, s.g, s.b, s.v);
    });
    tile.stage_features(sFeat, a.features);
    __syncthreads();

    // ---- filter: lane = column, one wave per tile row and pass ----
    const uint32_t tid = threadIdx.x;
    const int lx = (int)(tid & 63u);
    const int64_t x = org.x0 + lx;
    if (x >= org.W) return;
    rtds::Terms terms;
    terms.luminance = kAll || (a.terms & rtp::kDenoiseLuminance), terms.normal = kAll || (a.terms & rtp::kDenoiseNormal);
    terms.depth = kAll || (a.terms & rtp::kDenoiseDepth), terms.albedo = kAll || (a.terms & rtp::kDenoiseAlbedo);
    terms.inv_n = a.invN, terms.inv_z = a.invZ, terms.inv_a = a.invA;
    for (int j = (int)(tid >> 6); j < Tile::kRows; j += kThreads / kTileW) {
        const int64_t y = (int64_t)org.cls + (org.j0 + j) * kStep;
        if (y >= org.H) break;
        const int cc = Tile::centre(j, lx);
        const size_t p = (size_t)(y * org.W + x);
        const float4 cp = sCol[cc];
        const float4 ap = sFeat[cc], np = sFeat[kPlaneB + cc];  // {albedo, depth}, {normal, coverage}
        rtds::Cell o = cell_of(cp);  // a centre that does not count is carried
        if (rtds::counts(np.w, cp.w)) {
            // the tolerance, once per centre: the 3 x 3 Gaussian of the variance over the taps that count
            rtds::TolSums ts{0.0f, 0.0f};
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int q = Tile::tap(cc, dx, dy);
                    const float vq = sCol[q].w;
                    ts = rtds::tol_tap(ts, rtds::tol_weight(dy) * rtds::tol_weight(dx), vq,
                                       rtds::counts(sFeat[kPlaneB + q].w, vq));
                }
            }
            const rtds::Centre centre = rtds::centre_of(o, guide_of(ap, np), rtds::tolerance(ts, a.sigmaL, a.epsilon));
            rtds::Sums s{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
                for (int dx = -2; dx <= 2; ++dx) {
                    const int q = Tile::tap(cc, dx, dy);
                    const float4 cq = sCol[q];
                    const float4 aq = sFeat[q];
                    const float4 nq = sFeat[kPlaneB + q];
                    s = rtds::tap_update(s, rtds::spline_weight(dy) * rtds::spline_weight(dx), centre, cell_of(cq),
                                         guide_of(aq, nq), terms, rtds::counts(nq.w, cq.w));
                }
            }
            o = rtds::iteration_result(s);
        }
        if (!a.last) {
            a.dst[p] = make_float4(o.r, o.g, o.b, o.v);
        } else {
            const float n = a.stats[2 * p].w;
            float4 px = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            float var = 0.0f;
            if (n >= 1.0f) {
                const float g = 0.45454545f;
                const bool enc = a.encoding == rtp::kDenoiseGamma;
                px = make_float4(enc ? pm_pow(o.r, g) : o.r, enc ? pm_pow(o.g, g) : o.g, enc ? pm_pow(o.b, g) : o.b, n);
                var = o.v;
            }
            a.dst[p] = px;
            if (a.variance) a.variance[p] = var;
        }
    }
}

}  // namespace

hipError_t launch_denoise_samples(const DenoiseSamplesArgs& a, const rtp::DenoiseStep& t, bool first, hipStream_t st) {
    // (the kernel of step 1 is the first iteration's, and only that one's)
    if (t.grid == 0 || a.tilesX != t.tiles_x || a.tilesPerClass != t.tiles_per_class || !a.stats || !a.features || !a.dst ||
        (!first && !a.src) || first != (t.step == 1))
        return hipErrorInvalidValue;
    return for_step(t, [&](auto step) {
        constexpr int kStep = decltype(step)::value;
        constexpr bool kFirst = kStep == 1;
        const uint32_t all = rtp::kDenoiseLuminance | rtp::kDenoiseNormal | rtp::kDenoiseDepth | rtp::kDenoiseAlbedo;
        if (a.terms == all)
            hipLaunchKernelGGL((denoise_samples_atrous<kStep, kFirst, true>), dim3(t.grid), dim3(kThreads), 0, st, a);
        else
            hipLaunchKernelGGL((denoise_samples_atrous<kStep, kFirst, false>), dim3(t.grid), dim3(kThreads), 0, st, a);
        return hipGetLastError();
    });
}

}  // namespace rtd

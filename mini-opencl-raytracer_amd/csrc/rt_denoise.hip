// rt_denoise.hip -- the edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) of
// rtEnqueueDenoise, one launch per iteration.  The filter is defined operation by operation in
// include/rt_hip.h and restated in numpy by tests/denoise_ref.py: every fp32 operation here is one
// correctly rounded IEEE operation in the order written there (no contraction, denormals kept,
// IEEE division -- which is why this is a translation unit of its own, built with the standard flags
// and not with the shipped kernels' relaxed division).
//
// A workgroup filters one tile of rtp::denoise_plan, every lane the 25 taps of its pixels, out of a block
// staged in LDS: the tile, its staging and its safety rules are rt_atrous_tile.hpp, which
// rt_denoise_samples.hip shares.
#include "rt_denoise.hpp"

#include "rt_atrous_tile.hpp"

namespace rtd {

namespace {

__device__ __forceinline__ float dot3(float x, float y, float z) { return (x * x + y * y) + z * z; }
__device__ __forceinline__ float edge(float x) {
    const float m = fmaxf(0.0f, 1.0f - x);
    return m * m;
}

// kAll: all four edge-stopping terms are on (a.terms is not looked at)
template <int kStep, bool kAll>
__global__ __launch_bounds__(kThreads) void denoise_atrous(DenoiseArgs a) {
    using Tile = AtrousTile<kStep>;
    constexpr int kPlaneB = Tile::kPlaneB;
    __shared__ float4 sCol[Tile::kCells];
    __shared__ float4 sFeat[kPlaneB + Tile::kCells];
    const Tile tile{a.tilesX, a.tilesPerClass, a.width, a.height};
    const typename Tile::Origin org = tile.origin();
    if (tile.empty()) return;
    tile.stage_colours(sCol, [&](size_t p) { return a.src[p]; });
    tile.stage_features(sFeat, a.features);
    __syncthreads();

    // ---- filter: lane = column, one wave per tile row and pass ----
    const uint32_t tid = threadIdx.x;
    const int lx = (int)(tid & 63u);
    const int64_t x = org.x0 + lx;
    if (x >= org.W) return;
    constexpr float kH[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const bool onC = kAll || (a.terms & rtp::kDenoiseColor), onN = kAll || (a.terms & rtp::kDenoiseNormal);
    const bool onZ = kAll || (a.terms & rtp::kDenoiseDepth), onA = kAll || (a.terms & rtp::kDenoiseAlbedo);
    for (int j = (int)(tid >> 6); j < Tile::kRows; j += kThreads / kTileW) {
        const int64_t y = (int64_t)org.cls + (org.j0 + j) * kStep;
        if (y >= org.H) break;
        const int cc = Tile::centre(j, lx);
        const size_t p = (size_t)(y * org.W + x);
        const float4 cp = sCol[cc];
        const float4 ap = sFeat[cc], np = sFeat[kPlaneB + cc];  // {albedo, depth}, {normal, coverage}
        float4 o = cp;  // an uncovered centre is copied
        if (np.w != 0.0f) {
            const float rz = 1.0f / fmaxf(fabsf(ap.w), 0x1p-64f);
            float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f;
#pragma unroll
            for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
                for (int dx = -2; dx <= 2; ++dx) {
                    const int q = Tile::tap(cc, dx, dy);
                    const float4 cq = sCol[q];
                    const float4 aq = sFeat[q];
                    const float4 nq = sFeat[kPlaneB + q];
                    // a term that is off is left out of the product -- by select, so that the code
                    // stays one straight line (branches here cost the generic kernel 140 VGPRs)
                    float w = kH[dy + 2] * kH[dx + 2];
                    const float wc = w * edge(dot3(cp.x - cq.x, cp.y - cq.y, cp.z - cq.z) * a.invC);
                    w = onC ? wc : w;
                    const float wn = w * edge(dot3(np.x - nq.x, np.y - nq.y, np.z - nq.z) * a.invN);
                    w = onN ? wn : w;
                    const float d = (ap.w - aq.w) * rz;
                    const float wz = w * edge((d * d) * a.invZ);
                    w = onZ ? wz : w;
                    const float wa = w * edge(dot3(ap.x - aq.x, ap.y - aq.y, ap.z - aq.z) * a.invA);
                    w = onA ? wa : w;
                    const bool skip = nq.w == 0.0f;  // uncovered, or outside the image: adds nothing
                    sw = skip ? sw : sw + w;
                    sr = skip ? sr : sr + w * cq.x;
                    sg = skip ? sg : sg + w * cq.y;
                    sb = skip ? sb : sb + w * cq.z;
                }
            }
            o = make_float4(sr / sw, sg / sw, sb / sw, cp.w);
        }
        a.dst[p] = o;
    }
}

}  // namespace

hipError_t launch_denoise(const DenoiseArgs& a, const rtp::DenoiseStep& t, hipStream_t st) {
    if (t.grid == 0 || a.tilesX != t.tiles_x || a.tilesPerClass != t.tiles_per_class) return hipErrorInvalidValue;
    return for_step(t, [&](auto step) {
        constexpr int kStep = decltype(step)::value;
        const uint32_t all = rtp::kDenoiseColor | rtp::kDenoiseNormal | rtp::kDenoiseDepth | rtp::kDenoiseAlbedo;
        if (a.terms == all)
            hipLaunchKernelGGL((denoise_atrous<kStep, true>), dim3(t.grid), dim3(kThreads), 0, st, a);
        else
            hipLaunchKernelGGL((denoise_atrous<kStep, false>), dim3(t.grid), dim3(kThreads), 0, st, a);
        return hipGetLastError();
    });
}

}  // namespace rtd

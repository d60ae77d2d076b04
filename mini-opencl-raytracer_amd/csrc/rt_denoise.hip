// rt_denoise.hip -- the edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) of
// rtEnqueueDenoise, one launch per iteration.  The filter is defined operation by operation in
// include/rt_hip.h and restated in numpy by tests/denoise_ref.py: every fp32 operation here is one
// correctly rounded IEEE operation in the order written there (no contraction, denormals kept,
// IEEE division -- which is why this is a translation unit of its own, built with the standard flags
// and not with the shipped kernels' relaxed division).
//
// A workgroup filters one tile of rtp::denoise_plan: 64 contiguous columns of kRows rows of one
// residue class y mod kStep.  It stages the tile plus a halo of 2 taps -- (64 + 4 kStep) columns of
// kRows + 4 class rows -- in LDS as three float4 planes (colour; albedo, depth; normal, coverage)
// with 16-B loads whose lanes run along x, then every lane runs the 25 taps of its pixels out of
// LDS: a tap is kStep cells along a staged row, or one staged row up or down.  Cells outside the
// image are staged as zeros with coverage 0, so the rule that skips an uncovered tap skips them, and
// global indices are only ever formed from coordinates tested to lie inside the image.  Pixel values
// never reach an address.
#include "rt_denoise.hpp"

namespace rtd {

namespace {

constexpr int kTileW = (int)rtp::kDenoiseTileW, kThreads = (int)rtp::kDenoiseThreads;

__device__ __forceinline__ float dot3(float x, float y, float z) { return (x * x + y * y) + z * z; }
__device__ __forceinline__ float edge(float x) {
    const float m = fmaxf(0.0f, 1.0f - x);
    return m * m;
}

// kAll: all four edge-stopping terms are on (a.terms is not looked at)
template <int kStep, bool kAll>
__global__ __launch_bounds__(kThreads) void denoise_atrous(DenoiseArgs a) {
    constexpr int kRows = (int)rtp::denoise_rows(kStep);
    constexpr int SW = kTileW + 4 * kStep, SH = kRows + 4, kCells = SW * SH;
    // the {normal, coverage} plane starts 4 cells on, so that a staging store's lane pairs (the two
    // halves of one feature record) fall into different banks
    constexpr int kPlaneB = kCells + (int)rtp::kDenoisePadBytes / 16;
    static_assert((size_t)kCells * rtp::kDenoiseCellBytes + rtp::kDenoisePadBytes <= rtp::kDenoiseLdsBudget,
                  "staged block over the LDS budget");
    __shared__ float4 sCol[kCells];
    __shared__ float4 sFeat[kPlaneB + kCells];

    const uint32_t tid = threadIdx.x;
    const uint32_t tx = blockIdx.x % a.tilesX, rest = blockIdx.x / a.tilesX;
    const uint32_t ty = rest % a.tilesPerClass, cls = rest / a.tilesPerClass;
    const int64_t W = a.width, H = a.height;
    const int64_t x0 = (int64_t)tx * kTileW;
    const int64_t j0 = (int64_t)ty * kRows;             // the tile's first row, counted within its class
    if ((int64_t)cls + j0 * kStep >= H) return;         // a shorter class's last tile (the whole workgroup)

    // ---- stage: lanes run along x, one 16-B load each ----
    for (int c = (int)tid; c < kCells; c += kThreads) {
        const int cy = c / SW, cx = c - cy * SW;
        const int64_t x = x0 - 2 * kStep + cx, y = (int64_t)cls + (j0 - 2 + cy) * kStep;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (x >= 0 && x < W && y >= 0 && y < H) v = a.src[(size_t)(y * W + x)];
        sCol[c] = v;
    }
    for (int f = (int)tid; f < 2 * kCells; f += kThreads) {
        const int c = f >> 1, half = f & 1;
        const int cy = c / SW, cx = c - cy * SW;
        const int64_t x = x0 - 2 * kStep + cx, y = (int64_t)cls + (j0 - 2 + cy) * kStep;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // outside the image: coverage 0
        if (x >= 0 && x < W && y >= 0 && y < H) v = a.features[(size_t)(y * W + x) * 2 + half];
        sFeat[half * kPlaneB + c] = v;
    }
    __syncthreads();

    // ---- filter: lane = column, one wave per tile row and pass ----
    constexpr float kH[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const int lx = (int)(tid & 63u);
    const int64_t x = x0 + lx;
    if (x >= W) return;
    const bool onC = kAll || (a.terms & rtp::kDenoiseColor), onN = kAll || (a.terms & rtp::kDenoiseNormal);
    const bool onZ = kAll || (a.terms & rtp::kDenoiseDepth), onA = kAll || (a.terms & rtp::kDenoiseAlbedo);
    for (int j = (int)(tid >> 6); j < kRows; j += kThreads / kTileW) {
        const int64_t y = (int64_t)cls + (j0 + j) * kStep;
        if (y >= H) break;
        const int cc = (j + 2) * SW + 2 * kStep + lx;
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
                    const int q = cc + dy * SW + dx * kStep;
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
        a.dst[(size_t)(y * W + x)] = o;
    }
}

template <int kStep>
hipError_t launch_step(const DenoiseArgs& a, const rtp::DenoiseStep& t, hipStream_t st) {
    if (t.rows != rtp::denoise_rows(kStep) || t.stage_w != rtp::kDenoiseTileW + 4u * kStep || t.stage_h != t.rows + 4u)
        return hipErrorInvalidValue;
    const uint32_t all = rtp::kDenoiseColor | rtp::kDenoiseNormal | rtp::kDenoiseDepth | rtp::kDenoiseAlbedo;
    if (a.terms == all)
        hipLaunchKernelGGL((denoise_atrous<kStep, true>), dim3(t.grid), dim3(kThreads), 0, st, a);
    else
        hipLaunchKernelGGL((denoise_atrous<kStep, false>), dim3(t.grid), dim3(kThreads), 0, st, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_denoise(const DenoiseArgs& a, const rtp::DenoiseStep& t, hipStream_t st) {
    if (t.grid == 0 || a.tilesX != t.tiles_x || a.tilesPerClass != t.tiles_per_class) return hipErrorInvalidValue;
    switch (t.step) {
        case 1: return launch_step<1>(a, t, st);
        case 2: return launch_step<2>(a, t, st);
        case 4: return launch_step<4>(a, t, st);
        case 8: return launch_step<8>(a, t, st);
        case 16: return launch_step<16>(a, t, st);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace rtd

// rt_temporal.hip -- rtEnqueueTemporalAccumulate's kernel: the previous image reprojected into the
// current view and blended with the current frames by per-pixel sample count, one launch.  The
// operation is defined step by step in include/rt_hip.h and restated in numpy by
// tests/temporal_ref.py: every fp32 operation here is one correctly rounded IEEE operation in the
// order written there (no contraction, denormals kept, IEEE division and square root -- which is why
// this is a translation unit of its own, built with the standard flags and not with the shipped
// kernels' relaxed division).
//
// A workgroup takes one tile of rtp::temporal_plan: 64 contiguous columns of 4 rows, a wave per row
// and a lane per column, so `cur`, `cur_features` (two float4 per record) and `out` move as full
// 16-B-per-lane streams.  The four history taps are gathers through the caches: neighbouring lanes
// reproject to neighbouring history pixels, and the 4 rows of a tile share their taps' rows.
//
// Steps 2-4 -- where a depth read from a buffer decides an address -- are rt_temporal_math.hpp, the
// text a CPU program sweeps under sanitizers.  The motion variant (rtEnqueueTemporalAccumulateMotion)
// takes step 2's point and step 5's centre normal from a 32-B rt_pixel_motion stream instead.  A tap's index exists only after its integer
// coordinates were tested against the image; taps that do not count are dropped by select.
#include "rt_temporal.hpp"

namespace rtt {

namespace {

template <bool kHistory, bool kMotion>
__device__ __forceinline__ void temporal_body(const TemporalArgs& a, const float4* motion) {
    const Pixel px = tile_pixel(a.tilesX);
    const uint64_t x = px.x, y = px.y;
    if (x >= a.width || y >= a.height) return;
    const uint64_t p = y * a.width + x;
    const float4 c = a.cur[p];
    float4 o = make_float4(c.x, c.y, c.z, a.cur_frames);  // every "no history" row
    if (kHistory) {
        const float4 fa = a.cur_features[2 * p], fn = a.cur_features[2 * p + 1];  // {albedo, depth}, {normal, coverage}
        const Centre ce = kMotion ? centre_of_motion(a.k, motion[2 * p], motion[2 * p + 1], fn.w, a.depth_tolerance)
                                  : centre_of(reproject(a.k, (uint32_t)x, (uint32_t)y, fa.w), fn, a.depth_tolerance);
        const Reprojection& r = ce.r;
        float sw = 0.0f, sr = 0.0f, sg = 0.0f, sb = 0.0f, sn = 0.0f;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                uint64_t q = 0;
                const bool inside = tap_index(r, i, j, a.width, a.height, &q);
                float4 hz = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hn = hz, hc = hz;  // coverage 0: does not count
                if (inside) {
                    hz = a.hist_features[2 * q], hn = a.hist_features[2 * q + 1];
                    hc = a.hist[q];
                }
                const float nq = a.history_frames != 0.0f ? a.history_frames : hc.w;
                const float hnrm[3] = {hn.x, hn.y, hn.z};
                const bool counts = tap_on_surface(inside, hn.w, hz.w, hnrm, ce.nrm, r.de, ce.tol, a.normal_threshold) && nq >= 1.0f;
                const float bw = tap_weight(r, i, j);
                sw = counts ? sw + bw : sw;
                sr = counts ? sr + bw * hc.x : sr;
                sg = counts ? sg + bw * hc.y : sg;
                sb = counts ? sb + bw * hc.z : sb;
                sn = counts ? sn + bw * nq : sn;
            }
        }
        if (sw >= rtp::kTemporalMinWeight) {
            const float hr = sr / sw, hg = sg / sw, hb = sb / sw, hcount = sn / sw;
            const float n = fminf(hcount + a.cur_frames, a.max_history);
            const float alpha = a.cur_frames / n;
            o = make_float4(hr + (c.x - hr) * alpha, hg + (c.y - hg) * alpha, hb + (c.z - hb) * alpha, n);
        }
    }
    a.out[p] = o;
}

template <bool kHistory>
__global__ __launch_bounds__(kThreads) void temporal_accumulate(TemporalArgs a) {
    temporal_body<kHistory, false>(a, nullptr);
}
__global__ __launch_bounds__(kThreads) void temporal_accumulate_motion(TemporalArgs a, const float4* motion) {
    temporal_body<true, true>(a, motion);
}

}  // namespace

hipError_t launch_temporal(const TemporalArgs& a, const float4* motion, const rtp::TemporalPlan& p, hipStream_t st) {
    if (p.grid == 0 || a.width != p.width || a.height != p.height || a.tilesX != p.tiles_x ||
        (uint64_t)p.tiles_x * p.tiles_y != p.grid || p.has_history != (a.hist != nullptr) ||
        (a.hist != nullptr) != (a.hist_features != nullptr))
        return hipErrorInvalidValue;
    if (p.has_motion != (motion != nullptr)) return hipErrorInvalidValue;
    if (p.has_history && p.has_motion)
        hipLaunchKernelGGL(temporal_accumulate_motion, dim3(p.grid), dim3(kThreads), 0, st, a, motion);
    else if (p.has_history)
        hipLaunchKernelGGL((temporal_accumulate<true>), dim3(p.grid), dim3(kThreads), 0, st, a);
    else  // (no history: the motion records were validated and are not read)
        hipLaunchKernelGGL((temporal_accumulate<false>), dim3(p.grid), dim3(kThreads), 0, st, a);
    return hipGetLastError();
}

}  // namespace rtt

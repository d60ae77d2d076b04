// rt_reproject.hip -- rtEnqueueReprojectSamples' kernel: the per-pixel sample statistics of the
// previous view gathered bilinearly into the current view and recombined into one rt_pixel_stats per
// pixel, one launch.  The operation is defined step by step in include/rt_hip.h and restated in numpy by
// tests/reproject_samples_ref.py: every fp32 operation here is one correctly rounded IEEE operation in
// the order written there (no contraction, denormals kept, IEEE division and square root -- which is
// why this is a translation unit of its own, built with the standard flags and not with the shipped
// kernels' relaxed division).
//
// A workgroup takes one tile of rtp::reproject_plan, the temporal pass's: 64 contiguous columns of 4
// rows, a wave per row and a lane per column, so `cur_features` and `out_stats` (two float4 per record)
// move as full 16-B-per-lane streams.  The four history taps are gathers through the caches:
// neighbouring lanes reproject to neighbouring history pixels, and the 4 rows of a tile share their
// taps' rows.  A tap is 64 B, so it is fetched in two stages: the features of the four taps that lie
// inside the image, independent of one another, and then the statistics of those taps only whose
// features passed the surface tests -- across a disocclusion edge or off the image nothing more is read.
//
// The motion variant (rtEnqueueReprojectSamplesMotion) takes step 2's point and step 5's centre normal from a
// 32-B rt_pixel_motion stream instead of the depth.
//
// Steps 2-4 -- where a depth read from a buffer decides an address -- are rt_temporal_math.hpp, and the
// merge is rt_reproject_math.hpp: the texts a CPU program runs under sanitizers.  A tap's index exists
// only after its integer coordinates were tested against the image; no value of the statistics takes
// part in an address; taps that do not count are dropped by select.
#include "rt_reproject.hpp"

#include "rt_temporal.hpp"

namespace rtrs {

namespace {

template <bool kMotion>
__device__ __forceinline__ void reproject_body(const ReprojectArgs& a, const float4* motion) {
    const rtt::Pixel px = rtt::tile_pixel(a.tilesX);
    const uint64_t x = px.x, y = px.y;
    if (x >= a.width || y >= a.height) return;
    const uint64_t p = y * a.width + x;
    const float4 fa = a.cur_features[2 * p], fn = a.cur_features[2 * p + 1];  // {albedo, depth}, {normal, coverage}
    const rtt::Centre ce =
        kMotion ? rtt::centre_of_motion(a.k, motion[2 * p], motion[2 * p + 1], fn.w, a.depth_tolerance)
                : rtt::centre_of(rtt::reproject(a.k, (uint32_t)x, (uint32_t)y, fa.w), fn, a.depth_tolerance);
    const rtt::Reprojection& r = ce.r;
    // the features of the taps inside the image, then the statistics of those on the centre's surface
    uint64_t q[4];
    bool on[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        q[t] = 0;
        const bool inside = rtt::tap_index(r, t & 1, t >> 1, a.width, a.height, &q[t]);
        float4 hz = make_float4(0.0f, 0.0f, 0.0f, 0.0f), hn = hz;  // coverage 0: does not count
        if (inside) hz = a.hist_features[2 * q[t]], hn = a.hist_features[2 * q[t] + 1];
        const float hnrm[3] = {hn.x, hn.y, hn.z};
        on[t] = tap_on_surface(inside, hn.w, hz.w, hnrm, ce.nrm, r.de, ce.tol, a.normal_threshold);
    }
    float4 s0[4], s1[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        s0[t] = s1[t] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // n 0: does not count
        if (on[t]) s0[t] = a.hist_stats[2 * q[t]], s1[t] = a.hist_stats[2 * q[t] + 1];
    }
    TapSums sums = no_taps();
#pragma unroll
    for (int t = 0; t < 4; ++t) {  // j outer, i inner
        const Stats s = {{s0[t].x, s0[t].y, s0[t].z}, s0[t].w, s1[t].x, s1[t].y};
        add_tap(sums, on[t], rtt::tap_weight(r, t & 1, t >> 1), s);
    }
    Stats m;
    float4 o0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), o1 = o0;  // nothing carried: 32 zero bytes
    if (merge(sums, a.max_history, &m)) {
        o0 = make_float4(m.sum[0], m.sum[1], m.sum[2], m.n);
        o1 = make_float4(m.mean_y, m.m2_y, 0.0f, 0.0f);
    }
    a.out_stats[2 * p] = o0;
    a.out_stats[2 * p + 1] = o1;
}

__global__ __launch_bounds__(rtt::kThreads) void reproject_samples(ReprojectArgs a) { reproject_body<false>(a, nullptr); }
__global__ __launch_bounds__(rtt::kThreads) void reproject_samples_motion(ReprojectArgs a, const float4* motion) {
    reproject_body<true>(a, motion);
}

}  // namespace

hipError_t launch_reproject(const ReprojectArgs& a, const float4* motion, const rtp::ReprojectPlan& p, hipStream_t st) {
    if (p.grid == 0 || a.width != p.width || a.height != p.height || a.tilesX != p.tiles_x ||
        (uint64_t)p.tiles_x * p.tiles_y != p.grid || !a.hist_stats || !a.hist_features || !a.cur_features ||
        !a.out_stats || p.has_motion != (motion != nullptr))
        return hipErrorInvalidValue;
    if (p.has_motion)
        hipLaunchKernelGGL(reproject_samples_motion, dim3(p.grid), dim3(rtt::kThreads), 0, st, a, motion);
    else
        hipLaunchKernelGGL(reproject_samples, dim3(p.grid), dim3(rtt::kThreads), 0, st, a);
    return hipGetLastError();
}

}  // namespace rtrs

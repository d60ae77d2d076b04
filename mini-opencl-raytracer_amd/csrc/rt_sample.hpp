// rt_sample.hpp -- one adaptive sample per listed pixel in one launch (rtEnqueueSamplePixels): the camera
// ray and seed of rtEnqueueCameraPathsFor, the path of rtEnqueueTracePaths and the statistics update of
// rtEnqueueAccumulateSamples without the 36 + 16 B per record that hand a ray, a seed and a radiance from
// one kernel to the next.  Included after rt_trace.hpp by rt_kernels_body.hpp; instantiated per math
// policy by the two kernel TUs, like rt_trace.hpp.
//
// The kernel is rt_trace.hpp's trace_loop with the two ends replaced (SampleEnds):
//   count   every wave reads the optional device count once (a uniform load), clamps it to the n the host
//           range-checked and forms its units from that: m = min(n, count[0]).  The word is compared and
//           clamped, it never forms an address.
//   fill    a unit is 64 ids, one coalesced 4-B load per lane.  A lane whose id passes pixel_in_range
//           computes camera_paths_for's direction and seed and writes them into the ring's layout,
//           compacted by a ballot rank: {origin, gid bits}, {dir, kMaxDist}, seed.  Lanes past m and ids out
//           of range write no entry, so nothing of theirs is traced or counted.  An id enters arithmetic
//           only (gid / W, the seed) before that test and indexes nothing.
//   finish  where the trace stores its result: finite_sample, luminance and sample_update of
//           rt_adaptive_math.hpp on the two float4 halves of stats[gid].
//
// The division.  sample_update's d / n' is the IEEE quotient in every math mode (rt_hip.h), and the
// shipped TU is built with -fno-hip-fp32-correctly-rounded-divide-sqrt, under which a plain `/` is the
// 2.5-ulp one.  The update therefore takes its division as an argument, and this kernel passes IeeeDiv:
// the hardware's correctly rounded sequence (div_scale, rcp, the fma refinement, div_fmas, div_fixup)
// written out with builtins -- the sequence the compiler emits for `/` under the standard flags with fp32
// denormals on, and the one MathPinned::div (RT_PINNED_OP_DIV) compiles to in its own TU.  It does not
// depend on the TU's flags, so all three instantiations use it.
#pragma once

#pragma clang fp contract(off)
#include "rt_adaptive_math.hpp"

namespace rtk {

struct IeeeDiv {
    __device__ __forceinline__ float operator()(float a, float b) const {
        bool scaled_den, scaled_num;
        const float den = __builtin_amdgcn_div_scalef(a, b, false, &scaled_den);
        const float num = __builtin_amdgcn_div_scalef(a, b, true, &scaled_num);
        const float r0 = __builtin_amdgcn_rcpf(den);
        const float e0 = __builtin_fmaf(-den, r0, 1.0f);
        const float r1 = __builtin_fmaf(e0, r0, r0);
        const float q0 = num * r1;
        const float e1 = __builtin_fmaf(-den, q0, num);
        const float q1 = __builtin_fmaf(e1, r1, q0);
        const float e2 = __builtin_fmaf(-den, q1, num);
        return __builtin_amdgcn_div_fixupf(__builtin_amdgcn_div_fmasf(e2, r1, q1, scaled_num), b, a);
    }
};

template <class M>
struct SampleEnds {
    const KernelArgs& a;
    const SampleArgs& q;
    uint32_t m;        // wave-uniform: records of the launch, min(n, the device count)
    uint32_t gid = 0;

    __device__ __forceinline__ SampleEnds(const KernelArgs& a_, const SampleArgs& q_)
        : a(a_), q(q_), m(q_.count ? min(q_.n, q_.count[0]) : q_.n) {}

    __device__ __forceinline__ uint32_t n_units() const { return (m + 63u) >> 6; }  // m <= 2^31

    __device__ __forceinline__ uint32_t fill(uint32_t u0, uint32_t lane, float4* ring, uint32_t* ring_seed) {
        bool have = lane < m - u0;  // (the last unit may be partial)
        uint32_t g = 0;
        if (have) g = q.ids[(size_t)q.first + u0 + lane];  // first + m <= 2^31
        have = have && rta::pixel_in_range(g, q.nPixels);
        const unsigned long long hm = __ballot(have);
        if (have) {
            // camera_paths_for's record for g
            const F3 pos{a.camPos[0], a.camPos[1], a.camPos[2]};
            const F3 front{a.camFront[0], a.camFront[1], a.camFront[2]};
            const F3 up{a.camUp[0], a.camUp[1], a.camUp[2]};
            const float angle = M::tan(0.5f * (45.0f * 3.1415f / 180.0f));  // kernel_bvh.cl:392
            const uint32_t W = a.width, H = a.height;
            const uint32_t py = g / W, px = g - py * W;
            uint32_t seed = g + frame_hash(a.frameCount);
            const F3 d = camera_dir<M>(px, py, W, H, front, up, angle, seed);
            const uint32_t slot = lane_rank(hm);
            ring[2u * slot] = make_float4(pos.x, pos.y, pos.z, __uint_as_float(g));
            ring[2u * slot + 1u] = make_float4(d.x, d.y, d.z, kMaxDist);
            ring_seed[slot] = seed;
        }
        return (uint32_t)__popcll(hm);
    }
    __device__ __forceinline__ void take(uint32_t, const float4& e0) { gid = __float_as_uint(e0.w); }
    // the camera ray's interval starts where camera_paths_for writes it
    __device__ __forceinline__ float tmin(const float4&) const { return -__builtin_inff(); }
    // LIGHT_BOUNCES 0: the composed calls add the trace's zero radiance
    __device__ __forceinline__ void unwalked() { update(f3s(0.0f)); }
    __device__ __forceinline__ void first_hit(int32_t) {}
    template <class>
    __device__ __forceinline__ void finish(F3 r) {
        update(r);
    }
    // accumulate_samples' update of stats[gid] (rt_adaptive.hip), gid in range since fill
    __device__ __forceinline__ void update(F3 s) {
        if (!rta::finite_sample(s.x, s.y, s.z)) return;
        float4* rec = q.stats + 2 * (size_t)gid;
        const float4 lo = rec[0], hi = rec[1];
        const rta::Moments mo =
            rta::sample_update(rta::Moments{lo.w, hi.x, hi.y}, rta::luminance(s.x, s.y, s.z), IeeeDiv{});
        rec[0] = make_float4(lo.x + s.x, lo.y + s.y, lo.z + s.z, mo.n);
        rec[1] = make_float4(mo.mean_y, mo.m2_y, hi.z, hi.w);  // reserved: kept as found
    }
};

// the trace kernel's occupancy: gid replaces pos, prim0 goes (profiles/sample_pixels/register_report.txt)
template <class M, bool kStats, bool kBofs, bool kGlobalOct>
__global__ __launch_bounds__(kTraceThreads) __attribute__((amdgpu_waves_per_eu(RT_TRACE_WAVES, 8)))
void sample_pixels(KernelArgs a, SampleArgs q) {
    SampleEnds<M> e(a, q);
    trace_loop<M, kStats, kBofs, kGlobalOct, false>(a, e, q.refillMin, q.shadeMin);
}
// rtKernelSetShadowRays(k, 1): the trace's shadow walks between the same two ends
template <class M, bool kStats, bool kBofs, bool kGlobalOct>
__global__ __launch_bounds__(kTraceThreads) __attribute__((amdgpu_waves_per_eu(RT_TRACE_WAVES, 8)))
void sample_pixels_shadow(KernelArgs a, SampleArgs q) {
    SampleEnds<M> e(a, q);
    trace_loop<M, kStats, kBofs, kGlobalOct, true>(a, e, q.refillMin, q.shadeMin);
}

template <class M, bool S>
SampleKernelFn sample_pick_s(Walk w) {
    return w == Walk::LdsB  ? sample_pixels<M, S, true, false>
           : w == Walk::Lds ? sample_pixels<M, S, false, false>
                            : sample_pixels<M, S, false, true>;
}
template <class M, bool S>
SampleKernelFn sample_pick_shadow_s(Walk w) {
    return w == Walk::LdsB  ? sample_pixels_shadow<M, S, true, false>
           : w == Walk::Lds ? sample_pixels_shadow<M, S, false, false>
                            : sample_pixels_shadow<M, S, false, true>;
}
template <class M>
SampleKernelFn sample_pick(const Variant& v) {
    if (v.shadow) return v.stats ? sample_pick_shadow_s<M, true>(v.walk) : sample_pick_shadow_s<M, false>(v.walk);
    return v.stats ? sample_pick_s<M, true>(v.walk) : sample_pick_s<M, false>(v.walk);
}

}  // namespace rtk

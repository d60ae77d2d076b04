// rt_motion.hpp -- the motion records of the camera's centre rays in one launch (rtEnqueueFrameMotion):
// per pixel the closest hit of the centre ray and rtEnqueueHitMotion's record of it, without the 32 B of
// ray and the 16 B of hit that the composed calls hand from one kernel to the next.  Included after
// rt_query.hpp by rt_kernels_body.hpp; instantiated per math policy by the two kernel TUs.
//
// The kernel is rt_query.hpp's query_body with the two ends replaced (MotionEnds):
//   fill    a unit is 64 consecutive pixels.  Each lane of the wave computes its pixel's centre ray --
//           rt_temporal_math.hpp's centre_dir on the host constants of view_consts, additions and products
//           only, so the text means the same under the shipped TU's relaxed division -- and writes it into
//           the ring in rt_ray's layout, {origin, -inf}, {dir, kMaxDist}.  Nothing is loaded.  The walk's
//           InitRay normalises the direction in the kernel's math mode, as it does a caller's.
//   finish  where the query stores its hit: rt_motion_math.hpp's hit_motion on the walk's prim and the
//           barycentrics the query re-evaluates, stored as two float4 halves of motion[pixel].
//
// The record is one definition in every math mode, and the shipped TU is built with
// -fno-hip-fp32-correctly-rounded-divide-sqrt, under which `/` and sqrtf are the relaxed ones.  The
// record's 1.0f / sqrtf(l2) is therefore IeeeRsq: the square root through fp64 -- the fp64 square root is
// correctly rounded under either set of flags, and rounding it to fp32 is the correctly rounded fp32 root,
// since 53 >= 2 * 24 + 2 bits rule out a double rounding -- and rt_sample.hpp's IeeeDiv for the quotient.
#pragma once

#pragma clang fp contract(off)
#include "rt_motion_math.hpp"
#include "rt_sample.hpp"

namespace rtk {

struct IeeeRsq {
    __device__ __forceinline__ float operator()(float l2) const {
        return IeeeDiv{}(1.0f, (float)__builtin_sqrt((double)l2));
    }
};

struct MotionEnds {
    const KernelArgs& a;
    const MotionArgs& m;

    __device__ __forceinline__ uint32_t n_units() const { return m.nUnits; }

    __device__ __forceinline__ uint32_t base(uint32_t u0) const { return u0; }
    __device__ __forceinline__ uint32_t fill(uint32_t u0, uint32_t lane, float4* ring) const {
        const uint32_t n = min(64u, m.count - u0);  // (the last unit may be partial)
        if (lane < n) {
            const uint32_t gid = u0 + lane, W = a.width;
            const uint32_t py = gid / W, px = gid - py * W;
            float d[3];
            rtt::centre_dir(m.k, px, py, d);
            ring[2u * lane] = make_float4(m.k.cpos[0], m.k.cpos[1], m.k.cpos[2], -__builtin_inff());
            ring[2u * lane + 1u] = make_float4(d[0], d[1], d[2], kMaxDist);
        }
        return n;
    }

    // pos < m.count, a pixel of this launch; h.prim is the walk's: -1 or a triangle of the scene
    __device__ __forceinline__ void finish(uint32_t pos, const Traversal& h, float u, float v) const {
        const rtm::Motion r = rtm::hit_motion((uint32_t)h.prim, u, v, reinterpret_cast<const float*>(a.trisFull), a.nTris,
                                              reinterpret_cast<const float*>(m.prevPositions),
                                              reinterpret_cast<const float*>(m.prevNormals), m.firstTri, m.nTris,
                                              IeeeRsq{});
        float4* o = m.out + 2 * (size_t)pos;
        o[0] = make_float4(r.prev_point[0], r.prev_point[1], r.prev_point[2], __int_as_float(r.prim));
        o[1] = make_float4(r.prev_normal[0], r.prev_normal[1], r.prev_normal[2], __uint_as_float(r.flags));
    }
};

// the query's occupancy: traversal registers, and at the finish three vertices' worth of gathers
template <class M, bool kStats, bool kBofs, bool kGlobalOct>
__global__ __launch_bounds__(kQueryThreads) __attribute__((amdgpu_waves_per_eu(8, 8)))
void frame_motion(KernelArgs a, MotionArgs m) {
    query_body<M, kStats, kBofs, kGlobalOct, false>(a, MotionEnds{a, m}, m.refillMin);
}

template <class M, bool S>
MotionKernelFn motion_pick_s(Walk w) {
    return w == Walk::LdsB  ? frame_motion<M, S, true, false>
           : w == Walk::Lds ? frame_motion<M, S, false, false>
                            : frame_motion<M, S, false, true>;
}
template <class M>
MotionKernelFn motion_pick(const Variant& v) {
    return v.stats ? motion_pick_s<M, true>(v.walk) : motion_pick_s<M, false>(v.walk);
}

}  // namespace rtk

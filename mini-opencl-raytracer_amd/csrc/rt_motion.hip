// rt_motion.hip -- rtEnqueueExtractVertices' and rtEnqueueHitMotion's kernels for gfx950.
//
//   extract_vertices  the inverse of rt_refit.hip's update_vertices: one work item per (triangle,
//                     vertex), a 12-B-payload gather from the 256-B records and one coalesced 16-B store
//                     per output (w = 0);
//   hit_motion        hits in, previous surface points out: one record per lane, no LDS.  A coalesced
//                     16-B load, gathers by `prim` from the 256-B records or the prev_* buffers, two
//                     16-B stores to the lane's own 32 B.
// The record is defined operation by operation in include/rt_hip.h and restated in numpy by
// tests/motion_ref.py: every fp32 operation is one correctly rounded IEEE operation in the order written
// there (no contraction, denormals kept, IEEE division and square root -- which is why this is a
// translation unit of its own, built with the standard flags and not with the shipped kernels' relaxed
// division).  The arithmetic and the address logic are rt_motion_math.hpp, the text a CPU program runs
// under sanitizers.
#include "rt_motion_launch.hpp"

#include <math.h>

namespace rtmo {

namespace {

__global__ __launch_bounds__(rtp::kMotionThreads) void extract_vertices(const rt_cl_triangle* __restrict__ tris,
                                                                        uint32_t first, uint32_t n3,
                                                                        float4* __restrict__ positions,
                                                                        float4* __restrict__ normals) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n3) return;
    const uint32_t t = i / 3u, v = i - 3u * t;
    const float* src =
        reinterpret_cast<const float*>(tris) + (size_t)(first + t) * rtm::kTriangleFloats + v * rtm::kVertexFloats;
    positions[i] = make_float4(src[0], src[1], src[2], 0.0f);
    if (normals)
        normals[i] = make_float4(src[rtm::kNormalFloat], src[rtm::kNormalFloat + 1], src[rtm::kNormalFloat + 2], 0.0f);
}

struct IeeeRsq {
    __device__ float operator()(float l2) const { return 1.0f / sqrtf(l2); }
};

__global__ __launch_bounds__(rtp::kMotionThreads) void hit_motion(HitMotionArgs a, uint32_t first, uint32_t count,
                                                                  uint32_t first_tri, uint32_t n_tris) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const size_t idx = (size_t)first + i;
    const float4 h = a.hits[idx];
    const rtm::Motion m = rtm::hit_motion(__float_as_uint(h.x), h.z, h.w, reinterpret_cast<const float*>(a.tris),
                                          a.n_scene, reinterpret_cast<const float*>(a.prev_positions),
                                          reinterpret_cast<const float*>(a.prev_normals), first_tri, n_tris, IeeeRsq{});
    a.out[2 * idx] = make_float4(m.prev_point[0], m.prev_point[1], m.prev_point[2], __int_as_float(m.prim));
    a.out[2 * idx + 1] = make_float4(m.prev_normal[0], m.prev_normal[1], m.prev_normal[2], __uint_as_float(m.flags));
}

}  // namespace

hipError_t launch_extract_vertices(const rt_cl_triangle* tris, const rtp::ExtractPlan& p, float4* positions,
                                   float4* normals, hipStream_t st) {
    if (p.nothing) return hipSuccess;
    if (!tris || !positions || p.count == 0 || (uint64_t)p.grid * rtp::kMotionThreads < 3ull * p.count)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(extract_vertices, dim3(p.grid), dim3(rtp::kMotionThreads), 0, st, tris, p.first, 3u * p.count,
                       positions, normals);
    return hipGetLastError();
}

hipError_t launch_hit_motion(const HitMotionArgs& a, const rtp::HitMotionPlan& p, hipStream_t st) {
    if (p.nothing) return hipSuccess;
    if (!a.hits || !a.tris || !a.out || (p.n_tris != 0 && !a.prev_positions) ||
        (uint64_t)p.first_tri + p.n_tris > a.n_scene || (uint64_t)p.grid * rtp::kMotionThreads < p.count)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(hit_motion, dim3(p.grid), dim3(rtp::kMotionThreads), 0, st, a, p.first, p.count, p.first_tri,
                       p.n_tris);
    return hipGetLastError();
}

}  // namespace rtmo

// rt_motion_math.hpp -- the motion record of a hit (rtEnqueueHitMotion, rtEnqueueFrameMotion; the
// definition: include/rt_hip.h): which triangles count as moved, and the previous surface point and
// normal from three vertex positions, three vertex normals and the hit's barycentrics.  The kernels
// (rt_motion.hip; rt_motion.hpp's finish end in the two render TUs) and a CPU program
// (tests/native/motion_main.cpp, built with sanitizers) compile this same text.
//
// `u` and `v` come from a caller's buffer and may have any bit pattern: they enter arithmetic only.
// `prim` forms an address only after the caller range-tested it.  Every operation is one fp32
// operation; 1.0f / sqrtf(l2) is handed in (`rsq`), because a translation unit built with relaxed
// division cannot spell the IEEE pair with `/` and sqrtf.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_MM_FN __host__ __device__ inline
#else
#define RT_MM_FN inline
#endif

namespace rtm {

constexpr uint32_t kMotionBytes = 32, kTriPointsBytes = 48, kHitBytes = 16;
constexpr uint32_t kMoved = 1u;  // rt_pixel_motion::flags

// rt_pixel_motion as the kernels store it: two 16-B halves
struct Motion {
    float prev_point[3];
    int32_t prim;
    float prev_normal[3];
    uint32_t flags;
};

// prim in [first_tri, first_tri + n_tris): one unsigned compare, so n_tris == 0 moves nothing
RT_MM_FN bool moved(uint32_t prim, uint64_t first_tri, uint64_t n_tris) { return (uint64_t)prim - first_tri < n_tris; }

RT_MM_FN Motion miss() { return Motion{{0.0f, 0.0f, 0.0f}, -1, {0.0f, 0.0f, 0.0f}, 0u}; }

// P and N: the three vertices' xyz, row per vertex.  rsq(l2) = 1.0f / sqrtf(l2), two IEEE operations.
template <class Rsq>
RT_MM_FN Motion motion_record(int32_t prim, bool is_moved, const float (*P)[3], const float (*N)[3], float u, float v,
                              Rsq rsq) {
    Motion m;
    const float w = (1.0f - u) - v;
    float nn[3];
    for (int c = 0; c < 3; ++c) {
        m.prev_point[c] = P[0][c] * w + (P[1][c] * u + P[2][c] * v);
        nn[c] = N[0][c] * w + (N[1][c] * u + N[2][c] * v);
    }
    const float l2 = (nn[0] * nn[0] + nn[1] * nn[1]) + nn[2] * nn[2];
    const bool has = l2 > 0.0f;  // (false for a NaN)
    const float rl = rsq(l2);
    for (int c = 0; c < 3; ++c) m.prev_normal[c] = has ? nn[c] * rl : 0.0f;
    m.prim = prim;
    m.flags = is_moved ? kMoved : 0u;
    return m;
}

// Record layouts in floats: the 256-B triangle records (rt_cl_types.h: three 80-B vertices, position at
// float 0 and normal at float 8 of each) and rt_tri_points (three 16-B slots).
constexpr uint32_t kTriangleFloats = 64, kVertexFloats = 20, kNormalFloat = 8, kTriPointsFloats = 12;

// The motion record of hit {prim bits, u, v} on a scene of n_scene triangle records `tris`, with the
// previous vertices of triangles [first_tri, first_tri + n_tris) in prev_pos (and prev_nrm, or null).
// The one unsigned compare turns every index outside the triangle array (negative ones included) into a
// miss before it is used; a moved prim is inside [first_tri, first_tri + n_tris), which the plan placed
// inside the prev_* buffers.
template <class Rsq>
RT_MM_FN Motion hit_motion(uint32_t prim, float u, float v, const float* tris, uint32_t n_scene, const float* prev_pos,
                           const float* prev_nrm, uint32_t first_tri, uint32_t n_tris, Rsq rsq) {
    if (prim >= n_scene) return miss();
    const bool mv = moved(prim, first_tri, n_tris);
    const float* cur = tris + (size_t)prim * kTriangleFloats;
    float P[3][3], N[3][3];
    for (int i = 0; i < 3; ++i) {
        const float* p = mv ? prev_pos + (size_t)(prim - first_tri) * kTriPointsFloats + 4 * i : cur + i * kVertexFloats;
        const float* n = mv && prev_nrm ? prev_nrm + (size_t)(prim - first_tri) * kTriPointsFloats + 4 * i
                                        : cur + i * kVertexFloats + kNormalFloat;
        for (int c = 0; c < 3; ++c) P[i][c] = p[c], N[i][c] = n[c];
    }
    return motion_record((int32_t)prim, mv, P, N, u, v, rsq);
}

}  // namespace rtm

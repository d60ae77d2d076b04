// rt_octant_cull.hpp -- which triangles no ray of an octant can hit from the front: the certificate
// behind the pruned link set of the octant records (rt_scene_pack.cpp, prune_oct_links).  Pure functions
// of the triangle records (rt_octant_cull.cpp): no HIP, no allocation, no globals.  The rule is
// sufficient, not necessary: a refusal only keeps a leaf in an octant's links.
#pragma once

#include <stdint.h>

#include "../../include/rt_cl_types.h"

namespace rtp {

// The triangle as the device holds it (pack_tris): e1 = v2 - v1, e2 = v3 - v1, each one fp32 subtraction.
struct CullEdges {
    float e1[3], e2[3];
};
CullEdges octant_cull_edges(const rt_cl_triangle& t);

// Bit o of the result: every ray whose sign bits are o (bit k = invDir[k] < 0, Ray::sgn) fails
// RayTriangle's `det >= 1e-8` on this triangle, or has a NaN det, under every math policy -- such a test
// accepts nothing.  0 for a triangle with a non-finite or out-of-range (> 2^20) vertex.
uint8_t octant_cull_mask(const rt_cl_triangle& t);

// mask[i] = octant_cull_mask(tris[i]); returns the number of certified (triangle, octant) pairs.
uint32_t octant_cull_masks(const rt_cl_triangle* tris, uint32_t n_tris, uint8_t* mask);

}  // namespace rtp

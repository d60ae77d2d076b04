// rt_view_cull.hpp -- which 8x8 tiles of an image can see the scene at all, as a pure function of the
// image size, the camera slots and the root bounds (rt_view_cull.cpp): no HIP, no allocation, no
// globals.  enqueue (rt_capi.cpp) hands the rectangle to the launch plan (PlanIn::view), which leaves
// the tiles outside it out of a fused render's work; the accumulation gives them the sky constant.
#pragma once

#include <stdint.h>

namespace rtp {

// Tiles [tx0, tx1) x [ty0, ty1) of the image's 8x8 tile grid (tile (0, 0) at pixel (0, 0)).  Every
// camera sample of a pixel outside these tiles misses the root box.  Zero-initialised, or empty in
// either axis: "all" -- nothing is known, every tile is rendered.
struct ViewRect {
    uint32_t tx0, ty0, tx1, ty1;
    bool all() const { return tx1 <= tx0 || ty1 <= ty0; }
};

// W, H: the image; pos, front, up: the camera slots as the launch holds them (un-normalised,
// kernel_bvh.cl:386-403); bmin, bmax: the root node's bounds (nodes[0]).
ViewRect view_cull_rect(uint32_t W, uint32_t H, const float pos[3], const float front[3], const float up[3],
                        const float bmin[3], const float bmax[3]);

}  // namespace rtp

// rt_refit.hip -- moving geometry on the device: vertex update and BVH refit for gfx950.
//
// A refit changes bounds only.  Every layout the render and query kernels walk stores the box
// planes as bit copies of pmin / pmax beside words that depend on the topology alone
// (rt_scene_pack.cpp), so new planes are all a moved mesh needs:
//   update_vertices  caller positions (normals) -> the 256-B CLTriangle records;
//   refit_bounds     one work item per tree node: leaves fold their triangles, then climb the parent
//                    links with per-node arrival counters (the pattern of rt_bvh.hip: bottom_up);
//   refit_spread     one work item per (node, octant): the planes into the octant-major records, the
//                    node-major regrouped records and the 64-B global records.
// The spread is a launch of its own, not part of the climb: inside the climb its up to 17 stores
// per node would sit in front of the agent-scope release every level pays, which writes back what
// the lane dirtied; as a second launch they are plain streaming stores behind a kernel boundary.
// No lane waits on another anywhere: the first arriver at an interior node leaves, the second
// finishes it, and the climb is finite because a parent's index is smaller than its children's.
#include "rt_refit.hpp"

#include <math.h>

namespace rtr {

namespace {

constexpr uint32_t kVertexFloats = sizeof(rt_cl_vertex) / 4;                  // 20
constexpr uint32_t kNormalFloat = offsetof(rt_cl_vertex, normal) / 4;         // 8
constexpr uint32_t kTriangleFloats = sizeof(rt_cl_triangle) / 4;              // 64

// one work item per (triangle, vertex): a coalesced 16-B load, a 12-B-payload store
__global__ __launch_bounds__(256) void update_vertices(rt_cl_triangle* __restrict__ tris, uint32_t first,
                                                       uint32_t n3, const float4* __restrict__ positions,
                                                       const float4* __restrict__ normals) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n3) return;
    const uint32_t t = i / 3u, v = i - 3u * t;
    float* dst = reinterpret_cast<float*>(tris) + (size_t)(first + t) * kTriangleFloats + v * kVertexFloats;
    const float4 p = positions[i];
    dst[0] = p.x;
    dst[1] = p.y;
    dst[2] = p.z;
    if (normals) {
        const float4 nv = normals[i];
        dst[kNormalFloat] = nv.x;
        dst[kNormalFloat + 1] = nv.y;
        dst[kNormalFloat + 2] = nv.z;
    }
}

struct Box {
    float lo[3], hi[3];
};

__device__ inline void grow(Box& b, const rt_float3& p) {
    b.lo[0] = fminf(b.lo[0], p.x), b.lo[1] = fminf(b.lo[1], p.y), b.lo[2] = fminf(b.lo[2], p.z);
    b.hi[0] = fmaxf(b.hi[0], p.x), b.hi[1] = fmaxf(b.hi[1], p.y), b.hi[2] = fmaxf(b.hi[2], p.z);
}

// pmin.xyz / pmax.xyz of one node record; the w slots and bytes 32..47 keep their bytes
__device__ inline void store_box(rt_cl_bvh_node* nd, const Box& b) {
    nd->bounds.pmin.x = b.lo[0], nd->bounds.pmin.y = b.lo[1], nd->bounds.pmin.z = b.lo[2];
    nd->bounds.pmax.x = b.hi[0], nd->bounds.pmax.y = b.hi[1], nd->bounds.pmax.z = b.hi[2];
}

__global__ __launch_bounds__(256) void refit_bounds(const rt_cl_triangle* __restrict__ tris, uint32_t n_tris,
                                                    rt_cl_bvh_node* nodes, uint32_t n_nodes,
                                                    const uint32_t* __restrict__ parent, uint32_t* arrivals) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    const uint32_t cnt = nodes[i].nPrimitives;
    if (cnt == 0u) return;  // interior nodes are finished by the second of their subtrees to arrive
    const uint32_t first = nodes[i].offset;
    if ((uint64_t)first + cnt > n_tris) return;  // (validated by the full preparation)
    Box b;
    for (int a = 0; a < 3; ++a) b.lo[a] = INFINITY, b.hi[a] = -INFINITY;
    for (uint32_t j = 0; j < cnt; ++j) {
        const rt_cl_triangle& t = tris[first + j];
        grow(b, t.v1.position);
        grow(b, t.v2.position);
        grow(b, t.v3.position);
    }
    store_box(&nodes[i], b);
    uint32_t node = parent[i];
    while (node != kNoParent) {
        // release this lane's box, arrive, and -- as the second arriver -- acquire the sibling's
        // (agent scope: the XCDs' L2s are not coherent with each other).  A release before and an
        // acquire after the arrival, not two __threadfence(): each of those is both, twice the price
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        // (the wait the compiler may drop behind the write-back when it can prove the lane's
        // memory counter empty: the arrival must not overtake the box)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (atomicAdd(&arrivals[node], 1u) == 0u) return;  // the sibling subtree finishes this node
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        const uint32_t c1 = node + 1u, c2 = nodes[node].offset;
        if (c2 >= n_nodes) return;  // (validated by the full preparation)
        const rt_cl_bounds b1 = nodes[c1].bounds, b2 = nodes[c2].bounds;
        b.lo[0] = fminf(b1.pmin.x, b2.pmin.x), b.lo[1] = fminf(b1.pmin.y, b2.pmin.y);
        b.lo[2] = fminf(b1.pmin.z, b2.pmin.z);
        b.hi[0] = fmaxf(b1.pmax.x, b2.pmax.x), b.hi[1] = fmaxf(b1.pmax.y, b2.pmax.y);
        b.hi[2] = fmaxf(b1.pmax.z, b2.pmax.z);
        store_box(&nodes[node], b);
        node = parent[node];
    }
}

// one work item per (node, octant): near / far planes chosen by the octant bits exactly as
// build_oct_nodes chooses them; the END sentinels and every link word are not touched
__global__ __launch_bounds__(256) void refit_spread(RefitArgs a) {
    const uint32_t i = blockIdx.x * 32u + (threadIdx.x >> 3), o = threadIdx.x & 7u;  // 32 nodes per workgroup
    if (i >= a.n_nodes) return;
    const rt_cl_bounds bb = a.nodes[i].bounds;
    const float lo[3] = {bb.pmin.x, bb.pmin.y, bb.pmin.z}, hi[3] = {bb.pmax.x, bb.pmax.y, bb.pmax.z};
    float nr[3], fr[3];
    for (int ax = 0; ax < 3; ++ax) {
        const bool neg = (o >> ax) & 1u;
        nr[ax] = neg ? hi[ax] : lo[ax];
        fr[ax] = neg ? lo[ax] : hi[ax];
    }
    const float4 ra = make_float4(nr[0], nr[1], nr[2], fr[0]);
    const float2 rb = make_float2(fr[1], fr[2]);
    if (a.oct) {
        const size_t at = (size_t)o * a.oct_stride + i;
        a.oct[at] = ra;
        *reinterpret_cast<float2*>(&a.oct[(size_t)a.oct_b + at]) = rb;
    }
    if (a.goct) {
        const uint32_t G = a.goct_group;
        const size_t at = (size_t)(i / G) * 8u * G + i % G + (size_t)o * G;  // goct_word(i, G) + o * G
        a.goct[at] = ra;
        *reinterpret_cast<float2*>(&a.goct[(size_t)a.goct_b + at]) = rb;
    }
    if (a.g_nodes && o == 0u) {
        float4* r = a.g_nodes + (size_t)a.slot[i] * 4u;
        r[0] = make_float4(lo[0], lo[1], lo[2], hi[0]);
        *reinterpret_cast<float2*>(&r[1]) = make_float2(hi[1], hi[2]);
    }
}

}  // namespace

hipError_t launch_update_vertices(rt_cl_triangle* tris, uint32_t first, uint32_t n, const float4* positions,
                                  const float4* normals, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const uint32_t n3 = 3u * n;
    hipLaunchKernelGGL(update_vertices, dim3((n3 + 255u) / 256u), dim3(256), 0, st, tris, first, n3, positions,
                       normals);
    return hipGetLastError();
}

hipError_t launch_refit(const RefitArgs& a, hipStream_t st) {
    if (a.n_nodes == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(a.arrivals, 0, (size_t)a.n_nodes * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(refit_bounds, dim3((a.n_nodes + 255u) / 256u), dim3(256), 0, st, a.tris, a.n_tris,
                       a.nodes, a.n_nodes, a.parent, a.arrivals);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(refit_spread, dim3((a.n_nodes + 31u) / 32u), dim3(256), 0, st, a);
    return hipGetLastError();
}

}  // namespace rtr

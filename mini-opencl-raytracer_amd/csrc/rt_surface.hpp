// rt_surface.hpp -- the surface at a ray hit (rtEnqueueHitSurfaces) and, folded over frames, the
// first-hit feature buffers of the camera's rays (rtEnqueueFrameFeatures).  Included at the end of
// rt_kernels_body.hpp; instantiated per math policy by the two kernel TUs, like rt_query.hpp.
//
// Hits in, surfaces out: per record the kernel takes {prim, t, u, v} as the hit record holds them --
// nothing is intersected again -- and evaluates the reference's hit record (kernel_bvh.cl:144-147)
// with the render's own device code: hit_position and shading_normal are what shade_bounce calls,
// so `normal` is the normal the render shades with in that math mode.  The texture coordinate is the
// same weights and madd shape over v1/v2/v3.uv.xy, the geometric normal normalize(cross(e1, e2)) of
// the packed triangle's edges (kernel_bvh.cl:109-110; zero for a zero-area triangle: normalize's
// guard).
//
// Kernel shape: one record per lane, 256-thread workgroups, no LDS.  Per lane three 16-B loads (ray,
// hit), then gathers by `prim`: the 48-B shading record, e1 / e2 of the packed triangle (4 + 16 + 4
// B) and three 8-B uvs from the 256-B triangle records.  A surface leaves as four 16-B stores to the
// lane's own 64 B, so a wave's four stores fill 4 KiB of whole lines between them and L2 merges them;
// plain stores, since a caller typically reads the surfaces next and a non-temporal store would keep
// the lines in L2 all the same.
//
// `prim` comes from a buffer the caller can write: the one unsigned compare `prim >= nTris` turns
// every index outside the triangle array (negative ones included) into a miss before it is used.
#pragma once

namespace rtk {

struct SurfacePoint {
    F3 pos, normal, geo;
    float tu, tv;
    uint32_t material;
};

// the surface of triangle `prim` (< a.nTris) at barycentrics (u, v), distance t along ray {e0, e1}
template <class M>
__device__ __forceinline__ SurfacePoint surface_point(const KernelArgs& a, uint32_t prim, float4 e0, float4 e1,
                                                      float t, float u, float v) {
    SurfacePoint s;
    // InitRay (kernel_bvh.cl:42-55) on the caller's direction, as the query that made the hit
    const Ray r = init_ray<M>(F3{e0.x, e0.y, e0.z}, F3{e1.x, e1.y, e1.z});
    s.pos = hit_position<M>(r, t);
    // the packed shading record: {n1, mtlIndex}, {n2, n3.x}, {n3.yz}
    const float4* rec = a.shadeTris + 3 * (size_t)prim;
    const float4 s1 = rec[0], s2 = rec[1];
    const float2 s3 = *reinterpret_cast<const float2*>(rec + 2);
    s.normal = shading_normal<M>(F3{s1.x, s1.y, s1.z}, F3{s2.x, s2.y, s2.z}, F3{s2.w, s3.x, s3.y}, u, v);
    s.material = __float_as_uint(s1.w);
    // the packed triangle: {p1, e1.x}, {e1.yz, e2.xy}, {e2.z}
    const float4* tri = a.packedTris + 3 * (size_t)prim;
    const float e1x = reinterpret_cast<const float*>(tri)[3];
    const float4 q1 = tri[1];
    const float e2z = reinterpret_cast<const float*>(tri + 2)[0];
    s.geo = normalize<M>(M::cross(F3{e1x, q1.x, q1.y}, F3{q1.z, q1.w, e2z}));
    // kernel_bvh.cl:147, in shading_normal's association order (not normalised)
    const rt_cl_triangle& full = a.trisFull[prim];
    const float2 t1 = *reinterpret_cast<const float2*>(&full.v1.uv);
    const float2 t2 = *reinterpret_cast<const float2*>(&full.v2.uv);
    const float2 t3 = *reinterpret_cast<const float2*>(&full.v3.uv);
    const float w = (1.0f - u) - v;
    s.tu = madd<M>(t1.x, w, madd<M>(t2.x, u, t3.x * v));
    s.tv = madd<M>(t1.y, w, madd<M>(t2.y, u, t3.y * v));
    return s;
}

// kAccumulate false: rt_surface records.  true: rt_pixel_features sums of one frame's hits --
// albedo, normal, depth and coverage each take one fp32 addition per hit, in frame order (one launch
// per frame on one stream); the first frame starts from +0 without reading the output, the last
// scales by s.inv.
template <class M, bool kAccumulate>
__device__ __forceinline__ void hit_surfaces_body(const KernelArgs& a, const SurfaceArgs& s) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= s.count) return;
    const size_t idx = (size_t)s.first + i;
    const float4 h = s.hits[idx];
    const uint32_t prim = __float_as_uint(h.x);
    const bool hit = prim < a.nTris;  // (a negative prim is a large unsigned one)
    if (kAccumulate) {
        float4* o = s.out + 2 * idx;
        float4 f0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), f1 = f0;  // {albedo, depth}, {normal, coverage}
        if (!s.accFirst) {
            f0 = o[0];
            f1 = o[1];
        }
        if (hit) {
            const SurfacePoint p = surface_point<M>(a, prim, s.rays[2 * idx], s.rays[2 * idx + 1], h.y, h.z, h.w);
            // (the index was validated with the scene; the clamp keeps it an index whatever happens)
            const rt_float3 kd = a.materials[p.material < a.nMats ? p.material : 0u].diffuse;
            f0 = make_float4(f0.x + kd.x, f0.y + kd.y, f0.z + kd.z, f0.w + h.y);
            f1 = make_float4(f1.x + p.normal.x, f1.y + p.normal.y, f1.z + p.normal.z, f1.w + 1.0f);
        }
        if (s.accLast) {
            f0 = make_float4(f0.x * s.inv, f0.y * s.inv, f0.z * s.inv, f0.w * s.inv);
            f1 = make_float4(f1.x * s.inv, f1.y * s.inv, f1.z * s.inv, f1.w * s.inv);
        }
        if (hit || s.accFirst || s.accLast) {
            o[0] = f0;
            o[1] = f1;
        }
        return;
    }
    float4* o = s.out + 4 * idx;
    if (!hit) {
        o[0] = make_float4(0.0f, 0.0f, 0.0f, h.y);
        o[1] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
        o[2] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(0xffffffffu));
        o[3] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        return;
    }
    const SurfacePoint p = surface_point<M>(a, prim, s.rays[2 * idx], s.rays[2 * idx + 1], h.y, h.z, h.w);
    o[0] = make_float4(p.pos.x, p.pos.y, p.pos.z, h.y);
    o[1] = make_float4(p.normal.x, p.normal.y, p.normal.z, h.x);
    o[2] = make_float4(p.geo.x, p.geo.y, p.geo.z, __uint_as_float(p.material));
    o[3] = make_float4(p.tu, p.tv, 0.0f, 0.0f);
}

// entry points (instantiated per math policy by the TU that owns it)
template <class M, bool kAccumulate>
__global__ __launch_bounds__(kSurfaceThreads) void hit_surfaces(KernelArgs a, SurfaceArgs s) {
    hit_surfaces_body<M, kAccumulate>(a, s);
}

}  // namespace rtk

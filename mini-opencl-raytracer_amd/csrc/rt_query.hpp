// rt_query.hpp -- batched ray queries over caller-supplied rays (rtEnqueueIntersectRays) and the
// camera's primary rays as such records (rtEnqueueCameraRays).  Included at the end of
// rt_kernels_body.hpp; instantiated per math policy by the two kernel TUs, like rt_wavefront.hpp.
//
// Per ray the query is the reference's InitRay(origin, dir) followed by Intersect
// (kernel_bvh.cl:42-55, 171-219) in its node and triangle order, with two generalisations:
// isect.t starts at the ray's tmax (not MAX_RENDER_DIST), and a triangle the reference would accept
// is accepted only if also t >= tmin.  With tmin = -inf and tmax = 100000 the result is Intersect's
// bit for bit.  Any-hit is the same walk ended at its first acceptance.
//
// Kernel shape: wf_extend_body's (rt_wavefront.hpp).  Persistent waves, eight per SIMD (traversal
// registers only); per wave an LDS ring of 64 rt_ray records filled one 64-ray unit at a time with
// coalesced 16-B loads (unit j = rays first + 64 j ..., units handed statically over the waves);
// free lanes take rays from the ring, a lane whose walk ends stores its 16-B hit and frees itself;
// node and triangle steps in bursts chosen by the step weights.  Two scene paths: octant records
// and packed triangles staged in LDS, or both read from HBM/L2 (no shading records either way).
// The walk uses record indices (oct_step), not LDS byte addresses, so it does not depend on where
// the dynamic LDS starts.  The loop takes its two ends -- where a unit of rays comes from, where a
// finished walk goes -- as a parameter (QueryEnds here; rt_motion.hpp's MotionEnds make the rays from
// pixel indices and store motion records).
#pragma once

namespace rtk {

constexpr uint32_t kQueryRingF4 = kQueryRingBytes / 16u;  // float4 per wave: 64 x {origin, tmin}, {dir, tmax}

// RayTriangle's acceptance (tri_accept, kUV = false) with the query's lower bound beside it: the
// render kernels keep tri_accept itself.  Returns whether the triangle was accepted.
template <class M>
__device__ __forceinline__ bool query_triangle(const float4* tri, int32_t idx, const Ray& r, float tmin,
                                               Traversal& h) {
    const TriEval e = tri_eval<M>(tri, r);
    const float rej = __builtin_fminf(__builtin_fminf(__builtin_fminf(e.det - kHitEps, e.u),
                                                      __builtin_fminf(1.0f - e.u, e.v)),
                                      1.0f - (e.u + e.v));
    const float closer = rej < 0.0f ? -1.0f : h.t - e.t;
    // (tmin = -inf passes every t the reference accepts: a NaN t never gets here, closer is NaN)
    const bool ok = closer > 0.0f && e.t >= tmin;
    if (ok) {
        h.t = e.t;
        h.prim = idx;
    }
    return ok;
}

// The query's two ends, which rtEnqueueFrameMotion replaces (rt_motion.hpp: MotionEnds), the way
// rtEnqueueSamplePixels replaces the trace's:
//   n_units  64-ray units of the launch;
//   base     the position (`pos` below) of the first ray of the unit whose first ray is u0;
//   fill     the wave's ring takes that unit: returns its ray count;
//   finish   the lane's walk of ray `pos` ended with h (prim -1: a miss) and the barycentrics u, v.
struct QueryEnds {
    const QueryArgs& q;
    __device__ __forceinline__ uint32_t n_units() const { return q.nUnits; }
    // the unit's records as 128 float4s, two coalesced loads per lane (the last unit of the range may
    // be partial)
    __device__ __forceinline__ uint32_t base(uint32_t u0) const { return q.first + u0; }
    __device__ __forceinline__ uint32_t fill(uint32_t u0, uint32_t lane, float4* ring) const {
        const uint32_t n = min(64u, q.count - u0);
        const float4* src = q.rays + 2 * (size_t)base(u0);
        if (lane < 2u * n) ring[lane] = src[lane];
        if (lane + 64u < 2u * n) ring[lane + 64u] = src[lane + 64u];
        return n;
    }
    __device__ __forceinline__ void finish(uint32_t pos, const Traversal& h, float u, float v) const {
        q.hits[pos] = make_float4(__int_as_float(h.prim), h.t, u, v);
    }
};

template <class M, bool kStats, bool kBofs, bool kGlobalOct, bool kAny, class Ends>
__device__ __forceinline__ void query_body(const KernelArgs& a, const Ends& q, uint32_t refillMin) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    const uint32_t tid = threadIdx.x, nthr = blockDim.x;
    SceneView sc;
    uint32_t scene_f4;
    if (kGlobalOct) {
        // octant records and triangles of a scene too large for LDS, read from HBM/L2
        sc = SceneView{nullptr, a.packedTris, a.octNodes, nullptr, nullptr};
        scene_f4 = 0;
    } else {
        float4* lo = smem;
        float4* lt = lo + a.octRecords;
        for (uint32_t i = tid; i < a.octRecords; i += nthr) lo[i] = a.octNodes[i];
        for (uint32_t i = tid; i < 3 * a.nTris; i += nthr) lt[i] = a.packedTris[i];
        sc = SceneView{nullptr, lt, lo, nullptr, nullptr};
        scene_f4 = a.octRecords + 3u * a.nTris;
    }
    __syncthreads();

    const uint32_t lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (nthr >> 6) + (tid >> 6));
    const uint32_t nwaves = gridDim.x * (nthr >> 6);
    float4* ring = smem + scene_f4 + (tid >> 6) * kQueryRingF4;

    uint32_t unit = wave;                         // wave-uniform: next unit of this wave
    uint32_t rc_base = 0, rc_head = 0, rc_n = 0;  // wave-uniform: ring entries [rc_head, rc_head + rc_n) of
                                                  // the unit whose first ray is rc_base
    bool exhausted = false;                       // wave-uniform

    LaneStats st;
    Ray ray{};
    Traversal h{0.0f, -1, 0.0f, 0.0f};
    float tmin = 0.0f;
    uint32_t pos = 0;
    // the walk word as in wf_extend_body's LDS path: node < 2^24, leaf code, END (a.nNodes), kNotWalking
    uint32_t cur = kNotWalking, skip = 0u;

    for (;;) {
        // finished walks: the hit record, its barycentrics re-evaluated from the accepted triangle
        // (the same values the acceptance computed, as with_uv); the lane is free
        if (cur == a.nNodes) {
            float u = 0.0f, v = 0.0f;
            if (h.prim >= 0) {
                const TriEval e = tri_eval<M>(sc.tris + 3 * (size_t)h.prim, ray);
                u = e.u;
                v = e.v;
                if (kStats) ++st.hits;
            }
            q.finish(pos, h, u, v);
            cur = kNotWalking;
        }
        uint32_t n_trav = popc_ballot(cur < kLeafMin);
        uint32_t n_leaf = popc_ballot((int32_t)cur >= (int32_t)kLeafMin);
        if (!exhausted && 64u - (n_trav + n_leaf) >= refillMin) {
            // ---- free lanes take rays from the ring; an empty ring loads the next unit ----------
            for (;;) {
                const bool idle = cur == kNotWalking;
                const unsigned long long im = __ballot(idle);
                if (im == 0ull) break;
                if (rc_n == 0u) {
                    if (unit >= q.n_units()) {
                        exhausted = true;
                        break;
                    }
                    const uint32_t u0 = unit * 64u;
                    unit += nwaves;
                    rc_base = q.base(u0);
                    rc_n = q.fill(u0, lane, ring);
                    rc_head = 0;
                }
                const uint32_t rank = lane_rank(im);
                const uint32_t take = min((uint32_t)__popcll(im), rc_n);
                if (idle && rank < take) {
                    const float4 e0 = ring[2u * (rc_head + rank)], e1 = ring[2u * (rc_head + rank) + 1u];
                    pos = rc_base + rc_head + rank;
                    // InitRay (kernel_bvh.cl:42-55) on the caller's direction; isect.t starts at tmax
                    ray = init_ray<M>(F3{e0.x, e0.y, e0.z}, F3{e1.x, e1.y, e1.z});
                    tmin = e0.w;
                    h = Traversal{e1.w, -1, 0.0f, 0.0f};
                    cur = 0u;
                    if (kStats) ++st.rays;
                }
                rc_head += take;
                rc_n -= take;
            }
            n_trav = popc_ballot(cur < kLeafMin);
            n_leaf = popc_ballot((int32_t)cur >= (int32_t)kLeafMin);
        }
        if (n_trav + n_leaf == 0u) {
            if (exhausted) break;
            continue;
        }
        // ---- traversal steps (kernel_bvh.cl:171-219 per lane) ----------------------------------
        const bool leaf_step = n_leaf * a.stepWeightNode > n_trav * a.stepWeightLeaf;
        constexpr int kNodeBurst = kGlobalOct ? RT_GNODE_BURST : RT_NODE_BURST;
        constexpr int kTriBurst = kGlobalOct ? RT_GTRI_BURST : RT_WTRI_BURST;
        if (!leaf_step) {
#pragma unroll
            for (int rep = 0; rep < kNodeBurst; ++rep) {
                if (cur < kLeafMin) {
                    if (kStats && cur != a.nNodes) ++st.visits;
                    cur = oct_step<kBofs>(sc, a, cur, ray, h.t, skip);
                }
            }
        } else {
#pragma unroll
            for (int rep = 0; rep < kTriBurst; ++rep) {
                if ((int32_t)cur >= (int32_t)kLeafMin) {
                    if (kStats) ++st.tests;
                    const uint32_t idx = cur & 0x00ffffffu;
                    const bool ok = query_triangle<M>(sc.tris + 3 * (size_t)idx, (int32_t)idx, ray, tmin, h);
                    cur += 1u - kLeafMin;
                    if (cur < kLeafMin) cur = skip;
                    if (kAny && ok) cur = a.nNodes;  // any-hit: the walk ends at its first acceptance
                }
            }
        }
    }
    if (kStats) flush_stats(a, st, (int)lane);
}

// The primary ray KernelEntry traces for work-item gid (CreateRay, kernel_bvh.cl:386-403, seeded as
// :445), as an rt_ray record: the direction CreateRay hands to InitRay (its normalize(dir)), so the
// query's InitRay reproduces create_ray's ray_from_unit(pos, normalize(normalize(dir))).
template <class M>
__device__ __forceinline__ void camera_rays_body(const KernelArgs& a, float4* rays, uint32_t n) {
    const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n) return;
    const F3 pos{a.camPos[0], a.camPos[1], a.camPos[2]};
    const F3 front{a.camFront[0], a.camFront[1], a.camFront[2]};
    const F3 up{a.camUp[0], a.camUp[1], a.camUp[2]};
    const float angle = M::tan(0.5f * (45.0f * 3.1415f / 180.0f));  // kernel_bvh.cl:392
    const uint32_t W = a.width, H = a.height;
    const uint32_t py = gid / W, px = gid - py * W;
    uint32_t seed = gid + frame_hash(a.frameCount);
    const F3 d = camera_dir<M>(px, py, W, H, front, up, angle, seed);
    rays[2 * (size_t)gid] = make_float4(pos.x, pos.y, pos.z, -__builtin_inff());
    rays[2 * (size_t)gid + 1] = make_float4(d.x, d.y, d.z, kMaxDist);
}

// entry points (instantiated per math policy by the TU that owns it).  Only traversal state is
// live: 8 waves per SIMD, eight per workgroup so the staged scene is shared by eight.
template <class M, bool kStats, bool kBofs, bool kGlobalOct, bool kAny>
__global__ __launch_bounds__(kQueryThreads) __attribute__((amdgpu_waves_per_eu(8, 8)))
void query_rays(KernelArgs a, QueryArgs q) {
    query_body<M, kStats, kBofs, kGlobalOct, kAny>(a, QueryEnds{q}, q.refillMin);
}
template <class M>
__global__ __launch_bounds__(256) void camera_rays(KernelArgs a, float4* rays, uint32_t n) {
    camera_rays_body<M>(a, rays, n);
}

// (a scene not in LDS is walked through its octant records in HBM/L2)
template <class M, bool S, bool A>
QueryKernelFn query_pick_sa(Walk w) {
    return w == Walk::LdsB  ? query_rays<M, S, true, false, A>
           : w == Walk::Lds ? query_rays<M, S, false, false, A>
                            : query_rays<M, S, false, true, A>;
}
template <class M>
QueryKernelFn query_pick(const Variant& v) {
    if (v.stats) return v.any ? query_pick_sa<M, true, true>(v.walk) : query_pick_sa<M, true, false>(v.walk);
    return v.any ? query_pick_sa<M, false, true>(v.walk) : query_pick_sa<M, false, false>(v.walk);
}

}  // namespace rtk

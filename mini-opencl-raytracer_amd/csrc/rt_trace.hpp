// rt_trace.hpp -- path tracing over caller-supplied rays (rtEnqueueTracePaths) and the camera's
// primary rays with their RNG state as such records (rtEnqueueCameraPaths; for a list of work-item
// ids, rtEnqueueCameraPathsFor).  Included at the end of
// rt_kernels_body.hpp; instantiated per math policy by the two kernel TUs, like rt_query.hpp.
//
// Per record the trace is the reference's InitRay(origin, dir) followed by Render
// (kernel_bvh.cl:42-55, 349-384): every Intersect in the reference's node and triangle order, the
// bounce's shading and RNG draws by shade_bounce, the function every render schedule uses.  One
// generalisation, the query's, on the first segment only: isect.t starts at the record's tmax and a
// triangle is accepted only if t >= tmin; later segments are Intersect's (-inf, 100000).
//
// Kernel shape: the query's ring and walk (rt_query.hpp) with the step schedule's shading round.
// Persistent waves, four per workgroup; per wave an LDS ring of 64 {rt_ray, seed} records filled one
// 64-record unit at a time with coalesced loads (unit j = records first + 64 j ..., units handed
// statically over the waves); free lanes take records from the ring once refillMin lanes are free;
// node and triangle steps in bursts chosen by the step weights; a lane whose walk ends waits at END
// until shadeMin lanes wait there, or nobody walks: the wave then runs shade_bounce for them.  A path
// that continues walks again from the root, a path that ends -- a miss, the pdf break, the last
// bounce -- stores its 16-B result with one vector store and frees the lane.  Two scene paths: octant
// records, triangles, shading and material records staged in LDS, or all four read from HBM/L2.
// The walk uses record indices (oct_step), not LDS byte addresses.
#pragma once

namespace rtk {

constexpr uint32_t kTraceRingF4 = kTraceRingBytes / 16u;  // float4 per wave: 128 of rays, 16 of seeds

// The loop's two ends -- where a wave's records come from and where a finished path goes -- are a small
// type the loop is instantiated over; everything between them (the ring's take, the walk, the shading
// round) is one text.  An Ends type provides, per lane unless marked wave-uniform:
//   uint32_t n_units()                          wave-uniform: 64-record units of the launch
//   uint32_t fill(u0, lane, ring, ring_seed)    wave-uniform result: loads the unit whose first record is
//                                               u0 into ring entries [0, result)
//   void take(slot, e0)                         the lane takes entry `slot`, whose first vector is e0
//   void unwalked()                             LIGHT_BOUNCES 0: the taken record ends without a walk
//   float tmin(e0)                              else: the lane starts its walk; where the first segment's
//                                               interval starts
//   void first_hit(prim)                        the first segment's primitive (-1: a miss)
//   void finish(r)                              the path's radiance, clamped at zero
// TraceEnds is rtEnqueueTracePaths: records from the caller's arrays, a 16-B result per record.
struct TraceEnds {
    const TraceArgs& q;
    uint32_t rc_base = 0;  // wave-uniform: first record of the ring's unit
    uint32_t pos = 0;
    int32_t prim0 = -1;

    __device__ __forceinline__ uint32_t n_units() const { return q.nUnits; }
    // the unit's rays as 128 float4s, two coalesced loads per lane, and its seeds, one 4-B load per
    // lane or seed_base + the record's index (the last unit of the range may be partial)
    __device__ __forceinline__ uint32_t fill(uint32_t u0, uint32_t lane, float4* ring, uint32_t* ring_seed) {
        rc_base = q.first + u0;
        const uint32_t rc_n = min(64u, q.count - u0);
        const float4* src = q.rays + 2 * (size_t)rc_base;
        if (lane < 2u * rc_n) ring[lane] = src[lane];
        if (lane + 64u < 2u * rc_n) ring[lane + 64u] = src[lane + 64u];
        if (lane < rc_n) ring_seed[lane] = q.seeds ? q.seeds[(size_t)rc_base + lane] : q.seedBase + (rc_base + lane);
        return rc_n;
    }
    __device__ __forceinline__ void take(uint32_t slot, const float4&) { pos = rc_base + slot; }
    // Render's loop does not run: radiance 0 (either encoding), no first hit
    __device__ __forceinline__ void unwalked() { q.out[pos] = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1)); }
    __device__ __forceinline__ float tmin(const float4& e0) {
        prim0 = -1;  // (the walk starts: no first hit yet)
        return e0.w;
    }
    __device__ __forceinline__ void first_hit(int32_t prim) { prim0 = prim; }
    template <class M>
    __device__ __forceinline__ void finish(F3 r) {
        if (q.encoding != 0) r = gamma_out_step<M>(0u, f3s(0.0f), r);
        q.out[pos] = make_float4(r.x, r.y, r.z, __int_as_float(prim0));
    }
};

//
// kShadow (rtKernelSetShadowRays, rt_hip.h): a bounce that goes on with lightPixel > 0 does not add the
// light's term.  The lane keeps the term and the sampled direction, and walks the shadow ray from the hit
// position first -- [0.01, T], ended at its first acceptance like the query's any-hit walk, in the same
// node and triangle bursts as its neighbours' path walks.  When that walk ends the lane resolves at the top
// of the loop, without waiting for a shading round: the term is added if nothing was hit, then the next
// segment starts from the shadow ray's origin (the hit position) or, after the last bounce, the path
// finishes.  `sh` is 0 on a path walk, kShadowGoOn / kShadowLast on a shadow walk.
constexpr uint32_t kShadowGoOn = 1u, kShadowLast = 2u;

template <class M, bool kStats, bool kBofs, bool kGlobalOct, bool kShadow, class Ends>
__device__ __forceinline__ void trace_loop(const KernelArgs& a, Ends& e, uint32_t refillMin, uint32_t shadeMin) {
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    const uint32_t tid = threadIdx.x, nthr = blockDim.x;
    SceneView sc;
    uint32_t scene_f4;
    if (kGlobalOct) {
        // the records of a scene too large for LDS, read from HBM/L2
        sc = SceneView{nullptr, a.packedTris, a.octNodes, a.shadeTris, a.shadeMats};
        scene_f4 = 0;
    } else {
        float4* lo = smem;
        float4* lt = lo + a.octRecords;
        float4* ls = lt + 3 * a.nTris;
        float4* lm = ls + 3 * a.nTris;
        for (uint32_t i = tid; i < a.octRecords; i += nthr) lo[i] = a.octNodes[i];
        for (uint32_t i = tid; i < 3 * a.nTris; i += nthr) lt[i] = a.packedTris[i];
        for (uint32_t i = tid; i < 3 * a.nTris; i += nthr) ls[i] = a.shadeTris[i];
        for (uint32_t i = tid; i < 4 * a.nMats; i += nthr) lm[i] = a.shadeMats[i];
        sc = SceneView{nullptr, lt, lo, ls, lm};
        scene_f4 = a.octRecords + 6u * a.nTris + 4u * a.nMats;
    }
    __syncthreads();

    const uint32_t lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (nthr >> 6) + (tid >> 6));
    const uint32_t nwaves = gridDim.x * (nthr >> 6);
    float4* ring = smem + scene_f4 + (tid >> 6) * kTraceRingF4;
    uint32_t* ring_seed = reinterpret_cast<uint32_t*>(ring + 128);
    const uint32_t bounces = (uint32_t)a.lightBounces;

    uint32_t unit = wave;            // wave-uniform: next unit of this wave
    uint32_t rc_head = 0, rc_n = 0;  // wave-uniform: ring entries [rc_head, rc_head + rc_n) of the loaded unit
    bool exhausted = false;          // wave-uniform

    LaneStats st;
    Ray ray{};
    Traversal h{0.0f, -1, 0.0f, 0.0f};
    F3 radiance = f3s(0.0f), beta = f3s(1.0f);
    float tmin = 0.0f;
    uint32_t seed = 0, bounce = 0;
    // kShadow: the pending term and the sampled direction of the lane's shadow walk
    F3 term = f3s(0.0f), swi = f3s(0.0f);
    uint32_t sh = 0u;
    // the walk word as in query_body: node < 2^24, leaf code, END (a.nNodes: the walk is over, the lane
    // waits for its shading round), kNotWalking (the lane is free)
    uint32_t cur = kNotWalking, skip = 0u;

    for (;;) {
        if (kShadow && cur == a.nNodes && sh != 0u) {
            // ---- a shadow walk ended: kernel_bvh.cl:378 unless occluded, then :379 or the path's end --
            if (h.prim < 0) radiance = madd<M>(term, beta, radiance);
            if (sh == kShadowGoOn) {
                ray = init_ray<M>(madd<M>(swi, 0.01f, ray.o), swi);
                tmin = -__builtin_inff();
                h = Traversal{kMaxDist, -1, 0.0f, 0.0f};
                cur = 0u;
                if (kStats) ++st.rays;
            } else {
                e.template finish<M>(F3{M::max(radiance.x, 0.0f), M::max(radiance.y, 0.0f), M::max(radiance.z, 0.0f)});
                cur = kNotWalking;
            }
            sh = 0u;
        }
        uint32_t n_trav = popc_ballot(cur < kLeafMin && cur != a.nNodes);
        uint32_t n_leaf = popc_ballot((int32_t)cur >= (int32_t)kLeafMin);
        uint32_t n_ready = popc_ballot(cur == a.nNodes);
        if (!exhausted && 64u - (n_trav + n_leaf + n_ready) >= refillMin) {
            // ---- free lanes take records from the ring; an empty ring loads the next unit -------
            for (;;) {
                const bool idle = cur == kNotWalking;
                const unsigned long long im = __ballot(idle);
                if (im == 0ull) break;
                if (rc_n == 0u) {
                    if (unit >= e.n_units()) {
                        exhausted = true;
                        break;
                    }
                    const uint32_t u0 = unit * 64u;
                    unit += nwaves;
                    rc_n = e.fill(u0, lane, ring, ring_seed);
                    rc_head = 0;
                }
                const uint32_t rank = lane_rank(im);
                const uint32_t take = min((uint32_t)__popcll(im), rc_n);
                if (idle && rank < take) {
                    const float4 e0 = ring[2u * (rc_head + rank)], e1 = ring[2u * (rc_head + rank) + 1u];
                    seed = ring_seed[rc_head + rank];
                    e.take(rc_head + rank, e0);
                    if (bounces == 0u) {
                        e.unwalked();
                    } else {
                        // InitRay (kernel_bvh.cl:42-55) on the record's direction; isect.t starts at tmax
                        ray = init_ray<M>(F3{e0.x, e0.y, e0.z}, F3{e1.x, e1.y, e1.z});
                        tmin = e.tmin(e0);
                        h = Traversal{e1.w, -1, 0.0f, 0.0f};
                        radiance = f3s(0.0f);
                        beta = f3s(1.0f);
                        bounce = 0u;
                        cur = 0u;
                        if (kStats) ++st.rays;
                    }
                }
                rc_head += take;
                rc_n -= take;
            }
            n_trav = popc_ballot(cur < kLeafMin && cur != a.nNodes);
            n_leaf = popc_ballot((int32_t)cur >= (int32_t)kLeafMin);
            n_ready = popc_ballot(cur == a.nNodes);
        }
        if (n_ready >= shadeMin || (n_ready != 0u && n_trav + n_leaf == 0u)) {
            // ---- shading round (kernel_bvh.cl:358-380 per lane) ---------------------------------
            if (cur == a.nNodes) {
                // the hit's barycentrics re-evaluated from the accepted triangle (the values the
                // acceptance computed, as with_uv)
                Traversal hu = h;
                if (h.prim >= 0) {
                    const TriEval ev = tri_eval<M>(sc.tris + 3 * (size_t)h.prim, ray);
                    hu.u = ev.u;
                    hu.v = ev.v;
                }
                if (bounce == 0u) e.first_hit(h.prim);
                bool go;
                if (kShadow) {
                    Lit l;
                    go = shade_surface<M, kStats>(hu, ray, radiance, beta, seed, sc, a, st, l);
                    if (go && l.lp > 0.0f) {
                        // the shadow ray {pos, 0.01, L, T}; what follows it waits in term, swi and sh
                        float tmax;
                        const F3 L = shadow_dir<M>(l.pos, a.lightType, tmax);
                        term = l.term;
                        swi = l.wi;
                        sh = bounce + 1u < bounces ? kShadowGoOn : kShadowLast;
                        ray = init_ray<M>(l.pos, L);
                        tmin = 0.01f;
                        h = Traversal{tmax, -1, 0.0f, 0.0f};
                        cur = 0u;
                        if (kStats) ++st.rays;
                    } else if (go) {
                        // !(lp > 0): lines 378-379 as the reference executes them
                        radiance = madd<M>(l.term, beta, radiance);
                        ray = init_ray<M>(madd<M>(l.wi, 0.01f, l.pos), l.wi);
                    }
                } else {
                    go = shade_bounce<M, kStats>(hu, ray, radiance, beta, seed, sc, a, st);
                }
                ++bounce;
                if (kShadow && sh != 0u) {
                    // (the lane walks its shadow ray)
                } else if (go && bounce < bounces) {
                    // the next segment is the reference's Intersect
                    tmin = -__builtin_inff();
                    h = Traversal{kMaxDist, -1, 0.0f, 0.0f};
                    cur = 0u;
                    if (kStats) ++st.rays;
                } else {
                    e.template finish<M>(F3{M::max(radiance.x, 0.0f), M::max(radiance.y, 0.0f), M::max(radiance.z, 0.0f)});
                    cur = kNotWalking;
                }
            }
            continue;
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
                if (cur < kLeafMin && cur != a.nNodes) {
                    if (kStats) ++st.visits;
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
                    if (kShadow && ok && sh != 0u) cur = a.nNodes;  // any-hit: the shadow walk ends here
                }
            }
        }
    }
    if (kStats) flush_stats(a, st, (int)lane);
}

template <class M, bool kStats, bool kBofs, bool kGlobalOct, bool kShadow>
__device__ __forceinline__ void trace_body(const KernelArgs& a, const TraceArgs& q) {
    TraceEnds e{q};
    trace_loop<M, kStats, kBofs, kGlobalOct, kShadow>(a, e, q.refillMin, q.shadeMin);
}

// camera_rays_body's record for work-item gid, and the RNG state CreateRay leaves behind: gid +
// frame_hash(frameCount) after its two draws, the seed Render goes on with (kernel_bvh.cl:445-447)
template <class M>
__device__ __forceinline__ void camera_paths_body(const KernelArgs& a, float4* rays, uint32_t* seeds, uint32_t n) {
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
    seeds[gid] = seed;
}

// entry points (instantiated per math policy by the TU that owns it).  Walk and shading state are
// both live: RT_TRACE_WAVES per SIMD, the most the register report shows without spills.
#ifndef RT_TRACE_WAVES
#define RT_TRACE_WAVES 4
#endif
template <class M, bool kStats, bool kBofs, bool kGlobalOct>
__global__ __launch_bounds__(kTraceThreads) __attribute__((amdgpu_waves_per_eu(RT_TRACE_WAVES, 8)))
void trace_paths(KernelArgs a, TraceArgs q) {
    trace_body<M, kStats, kBofs, kGlobalOct, false>(a, q);
}
// rtKernelSetShadowRays(k, 1): the same budget (profiles/shadows/register_report.txt)
template <class M, bool kStats, bool kBofs, bool kGlobalOct>
__global__ __launch_bounds__(kTraceThreads) __attribute__((amdgpu_waves_per_eu(RT_TRACE_WAVES, 8)))
void trace_paths_shadow(KernelArgs a, TraceArgs q) {
    trace_body<M, kStats, kBofs, kGlobalOct, true>(a, q);
}
template <class M>
__global__ __launch_bounds__(256) void camera_paths(KernelArgs a, float4* rays, uint32_t* seeds, uint32_t n) {
    camera_paths_body<M>(a, rays, seeds, n);
}

// rtEnqueueCameraPathsFor: records [first, first + n) receive camera_paths_body's bytes for gid = ids[i].
// Any uint32 is a gid: like get_global_id(0) in CreateRay it only enters arithmetic, never an address.
template <class M>
__global__ __launch_bounds__(256) void camera_paths_for(KernelArgs a, const uint32_t* ids, uint32_t first, uint32_t n,
                                                        float4* rays, uint32_t* seeds) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const size_t r = (size_t)first + i;
    const uint32_t gid = ids[r];
    const F3 pos{a.camPos[0], a.camPos[1], a.camPos[2]};
    const F3 front{a.camFront[0], a.camFront[1], a.camFront[2]};
    const F3 up{a.camUp[0], a.camUp[1], a.camUp[2]};
    const float angle = M::tan(0.5f * (45.0f * 3.1415f / 180.0f));  // kernel_bvh.cl:392
    const uint32_t W = a.width, H = a.height;
    const uint32_t py = gid / W, px = gid - py * W;
    uint32_t seed = gid + frame_hash(a.frameCount);
    const F3 d = camera_dir<M>(px, py, W, H, front, up, angle, seed);
    rays[2 * r] = make_float4(pos.x, pos.y, pos.z, -__builtin_inff());
    rays[2 * r + 1] = make_float4(d.x, d.y, d.z, kMaxDist);
    seeds[r] = seed;
}

template <class M, bool S>
TraceKernelFn trace_pick_s(Walk w) {
    return w == Walk::LdsB  ? trace_paths<M, S, true, false>
           : w == Walk::Lds ? trace_paths<M, S, false, false>
                            : trace_paths<M, S, false, true>;
}
template <class M, bool S>
TraceKernelFn trace_pick_shadow_s(Walk w) {
    return w == Walk::LdsB  ? trace_paths_shadow<M, S, true, false>
           : w == Walk::Lds ? trace_paths_shadow<M, S, false, false>
                            : trace_paths_shadow<M, S, false, true>;
}
template <class M>
TraceKernelFn trace_pick(const Variant& v) {
    if (v.shadow) return v.stats ? trace_pick_shadow_s<M, true>(v.walk) : trace_pick_shadow_s<M, false>(v.walk);
    return v.stats ? trace_pick_s<M, true>(v.walk) : trace_pick_s<M, false>(v.walk);
}

}  // namespace rtk

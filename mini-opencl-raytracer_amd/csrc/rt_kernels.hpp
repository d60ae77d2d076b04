// rt_kernels.hpp -- launch interface between the C ABI (rt_capi.cpp) and the kernels: the argument
// structs, one launcher per kernel family taking the rtk::Variant (rt_layout.hpp) its plan chose,
// the occupancy cache keyed by the same Variant, and the table of kernels a math policy provides.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rt_cl_types.h"
#include "rt_layout.hpp"
#include "rt_temporal_math.hpp"

namespace rtk {

// Everything KernelEntry's 14 arguments carry (kernel_bvh.cl:415-431), plus the packed
// scene, the work-item range of this launch and the optional extension outputs.
struct KernelArgs {
    float4* result;                     // slot 0: float3 per work-item, 16-byte stride
    const rt_cl_triangle* trisFull;     // slot 1 (normals, material index)
    const rt_cl_material* materials;    // slot 3
    const float4* packedTris;           // derived from slot 1: 3 x float4 per triangle
    const float4* octNodes;             // derived from slot 2: [node][octant] resolved records (LDS path)
    const float4* gNodes;               // derived from slot 2: 64-B node records (global path)
    const float4* shadeTris;            // derived from slot 1: {n1, mtlIndex}, {n2, n3.x}, {n3.yz} per triangle
    const float4* shadeMats;            // derived from slot 3: {diffuse, 1/(a+1)}, {specular, a^2/pi}, {emission, a^2-1}, {rough, a}
    uint32_t nNodes, nTris, nMats;
    uint32_t octStride;                 // LDS path: records per octant plane (nodes, END sentinel, odd pad)
    uint32_t octB;                      // LDS path: float4 offset of the B planes (8 * octStride, or kOctB)
    uint32_t octRecords;                // LDS path: float4s of node records (octB + 8 * octStride)
    uint32_t nTop;                      // global path: leading gNodes records staged in LDS
    uint32_t width, height;             // slots 4, 5
    uint32_t frameCount;                // slot 6 (slot 7, frameSeed, is unused by the reference)
    int32_t lightBounces, lightType;    // slots 8, 9
    float skyboxIntensity;              // slot 10
    float camPos[3], camFront[3], camUp[3];  // slots 11-13 (w ignored)
    // work decomposition: work-items [gidBegin, gidEnd), rows [rowBegin, rowEnd)
    uint64_t gidBegin, gidEnd;
    uint32_t rowBegin, rowCount, tilesX, nTiles;  // tiles: 16x16 (tile schedule) or 8x8 (regen)
    uint32_t* workCounter;              // persistent schedules: next chunk (zeroed per launch)
    uint32_t chunkPixels, tailChunk;    // pixels per chunk (multiples of 64: whole 8x8 tiles), bulk / tail
    uint32_t chunkSplit;                // bulk chunks cover pixels [0, chunkSplit) of the tile order
    uint32_t refillMin, shadeMin;       // step schedule batching thresholds (lanes)
    uint32_t stepWeightNode, stepWeightLeaf;  // step schedule: relative cost of node / triangle steps
    uint32_t bandPeriod, bandPhase;     // 8-row bands: this launch renders bands b % period == phase
    // extensions
    int32_t* hitIds;                    // primary hit primitive per work-item (-1 = miss)
    float* hitT;                        // primary isect.t per work-item
    unsigned long long* stats;          // [rays, node visits, triangle tests, hits, 4 phase-cycle sums]
    // rtEnqueueKernelFrames (step schedule): frames frameCount .. frameCount + nFrames - 1 in one
    // launch; radiance per (frame slot, gid) in radBuf[slot * radStride + gid] (null: one frame)
    float4* radBuf;
    // primary-miss flags: 1 = radiance (K_rad x3), not in radBuf.  flagTiles 0: one byte per
    // [slot * radStride + gid]; flagTiles 1 (the LDS walk's ray ring): one 64-bit word per
    // [slot * nTiles + tile], bit = pixel's lane in the tile, written once by the wave that
    // generated the tile's camera rays; every path not decided at its camera ray stores its
    // radiance.  flagTiles 2 (the HBM/L2 octant walk): no flags, every path stores it
    uint8_t* frameFlags;
    uint32_t flagTiles;
    uint32_t nFrames, radStride;
    uint32_t tileMajor;                 // fused: work items ordered (tile, frame) instead of (frame, tile)
    // per-frame launches (step schedule): sky-pixel shortcut key, chained launch to launch --
    // pfKeyIn = the value all-sky pixels hold if they followed the chain, pfKeyOut = this launch's
    const uint32_t* pfKeyIn;
    uint32_t* pfKeyOut;
    // (appended fields: the earlier ones keep their offsets)
    uint32_t* workCounterClear;         // per-frame step launches: the other counter slot, zeroed by this launch
    uint32_t tailBase;                  // first tail work item the tail counter hands out (next_chunk)
    uint32_t staticFirst;               // step schedule: waves start with their own tail chunk (no bulk region)
    // counter partitions (per-frame launches without a bulk region): nParts (a power of two) contiguous
    // ranges of partLen work items, each with its tail counter at workCounter[kPartStride * q + 1]
    uint32_t nParts, partLen;
    // the view cull (rt_view_cull.hpp; fused step launches): the work items are the frames of the
    // visW x visH tiles from (visTx0, visTy0) of the launch's tile grid, visTiles = visW * visH; the
    // tiles outside are not rendered, and accum_frames takes every frame of theirs as a primary miss.
    // Without a cull: (0, 0, tilesX, tile rows, nTiles).  radStride, the flag words and the
    // accumulation's grid stay in the full grid's numbering.
    uint32_t visTx0, visTy0, visW, visH, visTiles;
    // the path kill (rt_path_kill.hpp; step launches without stats): 1 = the launch is certified, and a
    // path whose beta is (+-0, +-0, +-0) after a bounce ends there as if its bounces had run out
    uint32_t pathKill;
};

using KernelFn = void (*)(KernelArgs);

// ---- wavefront schedule (rt_wavefront.hpp) ----------------------------------------------------
// Per bounce b: extend(b) walks the BVH for every queued ray, shade(b) shades every queued path
// and appends the continuations to the other queue.
struct WfArgs {
    const float4* inQ;        // bounce-b queue: 4 planes of `cap` float4:
                              //   {o.xyz, path}, {d.xyz, seed}, {beta.xyz, -}, {radiance.xyz, -}
    float4* outQ;             // bounce-(b+1) queue, same layout (written by shade)
    float2* hits;             // [cap] {t, primitive bits}: extend(b) -> shade(b)
    const uint32_t* inCnt;    // [G + 1]: entries per stream of inQ, [G] = their maximum
    uint32_t* outCnt;         // [G + 1]: the same for outQ
    uint32_t cap;             // entries per plane (nBlocks * 64)
    uint32_t G;               // streams
    uint32_t nBlocks;         // 64-entry blocks of the work-item space (nTiles * nFrames)
    uint32_t bounce;          // this launch's bounce index
    uint32_t refillMin;       // extend: take new rays once this many lanes are free
};
using WfKernelFn = void (*)(KernelArgs, WfArgs);
struct WfKernels {
    WfKernelFn extend, shade;
};
// the launches of one wavefront render: for b < lightBounces, extend(b) then shade(b); queues and
// counts alternate between q[0]/q[1] and cnt[0]/cnt[1]
hipError_t launch_wavefront(const KernelArgs& a, WfArgs w, float4* const q[2], uint32_t* const cnt[2],
                            const Variant& v, unsigned grid_e, size_t smem_e, unsigned grid_s, hipStream_t st);

// ---- ray queries (rt_query.hpp) ------------------------------------------------------------------
// rtEnqueueIntersectRays: KernelArgs carries the packed scene (packedTris, octNodes, nNodes, nTris,
// octStride, octB, octRecords), the step weights and the stats pointer; the rest is unused.
struct QueryArgs {
    const float4* rays;       // rt_ray records as 2 x float4: {origin, tmin}, {dir, tmax}
    float4* hits;             // rt_ray_hit records: {prim bits, t, u, v}
    uint32_t first, count;    // the range [first, first + count) of both arrays
    uint32_t nUnits;          // 64-ray units of the range (the last one may be partial)
    uint32_t refillMin;       // take new rays once this many lanes are free
};
using QueryKernelFn = void (*)(KernelArgs, QueryArgs);
hipError_t launch_query(const KernelArgs& a, const QueryArgs& q, const Variant& v, unsigned grid, size_t smem,
                        hipStream_t st);
// rtEnqueueCameraRays: width, height, frameCount and the camera slots of `a`; one rt_ray per work-item
hipError_t launch_camera_rays(const KernelArgs& a, float4* rays, uint32_t n, int math, hipStream_t st);

// ---- motion records of the camera's centre rays (rt_motion.hpp) ------------------------------------
// rtEnqueueFrameMotion: KernelArgs carries what a query's does plus trisFull (the current vertices).
struct MotionArgs {
    const float4* prevPositions;  // rt_tri_points of triangles [firstTri, firstTri + nTris); null: nTris == 0
    const float4* prevNormals;    // null: the current normals
    float4* out;                  // rt_pixel_motion records as 2 x float4, one per pixel
    uint32_t firstTri, nTris;     // the moved range, inside the scene's triangles
    uint32_t count;               // pixels [0, count)
    uint32_t nUnits;              // 64-pixel units (the last one may be partial)
    uint32_t refillMin;           // take new pixels once this many lanes are free
    rtt::TemporalConsts k;        // the host constants of the centre ray (the current view's)
};
using MotionKernelFn = void (*)(KernelArgs, MotionArgs);
hipError_t launch_motion(const KernelArgs& a, const MotionArgs& m, const Variant& v, unsigned grid, size_t smem,
                         hipStream_t st);

// ---- path tracing over caller rays (rt_trace.hpp) -------------------------------------------------
// rtEnqueueTracePaths: KernelArgs carries the packed scene with its shading and material records
// (packedTris, octNodes, shadeTris, shadeMats, nNodes, nTris, nMats, octStride, octB, octRecords),
// lightBounces, lightType, skyboxIntensity, the step weights and the stats pointer; the rest is unused.
struct TraceArgs {
    const float4* rays;       // rt_ray records as 2 x float4: {origin, tmin}, {dir, tmax}
    const uint32_t* seeds;    // the RNG state each record's Render starts with; null: seedBase + index
    float4* out;              // rt_path_result records: {radiance.xyz, first prim bits}
    uint32_t first, count;    // the range [first, first + count) of the arrays
    uint32_t nUnits;          // 64-record units of the range (the last one may be partial)
    uint32_t refillMin;       // take new records once this many lanes are free
    uint32_t shadeMin;        // shade once this many lanes' walks have ended
    uint32_t seedBase;
    int32_t encoding;         // RT_TRACE_LINEAR / RT_TRACE_FRAME0
};
using TraceKernelFn = void (*)(KernelArgs, TraceArgs);
hipError_t launch_trace(const KernelArgs& a, const TraceArgs& q, const Variant& v, unsigned grid, size_t smem,
                        hipStream_t st);
// rtEnqueueCameraPaths: launch_camera_rays' records plus each work-item's seed after CreateRay
hipError_t launch_camera_paths(const KernelArgs& a, float4* rays, uint32_t* seeds, uint32_t n, int math,
                               hipStream_t st);
// rtEnqueueCameraPathsFor: records [first, first + n) of `rays` and `seeds` for the work-items ids[first ...]
hipError_t launch_camera_paths_for(const KernelArgs& a, const uint32_t* ids, uint32_t first, uint32_t n, float4* rays,
                                   uint32_t* seeds, unsigned grid, int math, hipStream_t st);

// ---- one adaptive sample per listed pixel (rt_sample.hpp) -----------------------------------------
// rtEnqueueSamplePixels: KernelArgs carries what rtEnqueueTracePaths' does plus width, height,
// frameCount and the camera slots.
struct SampleArgs {
    const uint32_t* ids;      // work-item ids; records [first, first + m) are sampled
    const uint32_t* count;    // null: m = n; else m = min(n, count[0]), read on the device
    float4* stats;            // rt_pixel_stats records as 2 x float4, nPixels of them
    uint32_t first, n;        // first + n <= 2^31, inside `ids`
    uint32_t nPixels;         // ids from nPixels on are skipped
    uint32_t refillMin;       // take new records once this many lanes are free
    uint32_t shadeMin;        // shade once this many lanes' walks have ended
};
using SampleKernelFn = void (*)(KernelArgs, SampleArgs);
hipError_t launch_sample(const KernelArgs& a, const SampleArgs& q, const Variant& v, unsigned grid, size_t smem,
                         hipStream_t st);

// ---- surface records of ray hits (rt_surface.hpp) ------------------------------------------------
// rtEnqueueHitSurfaces / rtEnqueueFrameFeatures: KernelArgs carries trisFull (uvs), packedTris (e1, e2),
// shadeTris (normals, mtlIndex), nTris and -- accumulating variant only -- materials; the rest is unused.
struct SurfaceArgs {
    const float4* rays;       // rt_ray records as 2 x float4
    const float4* hits;       // rt_ray_hit records
    float4* out;              // rt_surface records (4 x float4), or rt_pixel_features (2 x float4) when accumulating
    uint32_t first, count;    // the range [first, first + count) of all three arrays
    uint32_t accFirst;        // accumulating: the sums start at +0 (the output is not read)
    uint32_t accLast;         // accumulating: the sums are scaled by `inv` before they are stored
    float inv;                // 1.0f / n_frames, the IEEE quotient (computed on the host)
};
using SurfaceKernelFn = void (*)(KernelArgs, SurfaceArgs);
hipError_t launch_surfaces(const KernelArgs& a, const SurfaceArgs& s, int math, bool accumulate, unsigned grid,
                           hipStream_t st);

hipError_t launch_kernel_entry(const KernelArgs& a, const Variant& v, unsigned grid, size_t smem, hipStream_t st);
// accumulate the fused frames' radiances into the output (one pixel per lane)
// (`key`: 4 words of per-kernel state for the sky shortcut, zeroed once; accum_key_body)
hipError_t launch_accum_frames(const KernelArgs& a, int math, uint32_t* key, hipStream_t st);
// rtDiagGammaPow (tests): gamma_check_body's sweep; `out` is 3 device words {mismatches, UINT32_MAX, 0}
struct GammaCheckArgs {
    unsigned long long* out;
    unsigned long long count;  // operand bit patterns first .. first + count - 1, count <= 2^32
    uint32_t first;
    uint32_t check;     // 0: pow_gamma against the policy's pow; 1: the frame-1 lemma
    uint32_t exponent;  // 0: 2.2f, 1: 0.454545f, 2: 0.45454545f (check 0)
};
hipError_t launch_gamma_check(const GammaCheckArgs& g, int math, hipStream_t st);
hipError_t launch_pinned_math(int op, const float* a, const float* b, float* out, size_t n, hipStream_t st);
hipError_t launch_pack(const rt_cl_triangle* tris, uint32_t n_tris, float4* pt, float4* ps,
                       const rt_cl_material* mats, uint32_t n_mats, float4* pm, hipStream_t st);

// Workgroups per CU of a kernel at a dynamic LDS size, remembered per (kernel family, variant): the
// runtime is asked on the first use and again when the LDS size differs.  The kernel is picked as
// the launch picks it, from the same Variant.
enum class Family : int { Entry, WfExtend, WfShade, Query, Trace, Sample, Motion };
struct OccupancyCache {
    struct Entry {
        int blocks;   // 0: not asked yet
        size_t smem;
    };
    Entry e[(int)Family::Motion + 1][kVariantSlots] = {};
    int get(Family f, const Variant& v, size_t smem);
};

// The kernels of one math policy, listed by the TU that instantiates it: rt_kernels.hip holds the
// pinned and devicelib tables; the shipped one is all rt_kernels_shipped.hip exports (own TU:
// OpenCL-default / and sqrt).
struct Policy {
    KernelFn (*entry)(const Variant&);
    WfKernels (*wavefront)(const Variant&);
    QueryKernelFn (*query)(const Variant&);
    void (*accum_frames)(KernelArgs, const uint32_t*);
    void (*accum_key)(KernelArgs, uint32_t*);
    void (*camera_rays)(KernelArgs, float4*, uint32_t);
    void (*pack_mats)(const rt_cl_material*, float4*, uint32_t);  // the policy's material records
    SurfaceKernelFn surfaces, surfaces_accum;  // hit_surfaces<M, false / true>
    TraceKernelFn (*trace)(const Variant&);
    void (*camera_paths)(KernelArgs, float4*, uint32_t*, uint32_t);
    void (*camera_paths_for)(KernelArgs, const uint32_t*, uint32_t, uint32_t, float4*, uint32_t*);
    SampleKernelFn (*sample)(const Variant&);
    MotionKernelFn (*motion)(const Variant&);
    void (*gamma_check)(GammaCheckArgs);
};
const Policy& shipped_policy();
// the step schedule's entry points are specialised per launch kind (step_body kMode: 1 fused, 2
// per-frame); stats builds and RT_SPECIALIZE_FUSED 0 use the generic body (kMode 0)
#ifndef RT_SPECIALIZE_FUSED
#define RT_SPECIALIZE_FUSED 1
#endif

}  // namespace rtk

/*
 * rt_hip.h -- C ABI of the MI355X hot path (librt_hip.so).
 *
 * Drop-in for the reference's OpenCL device boundary: the CLContext / CLKernel wrapper
 * (/root/reference/CLutils.h:107-145, CLutils.cpp:9-77) and the clCreateBuffer calls of
 * its callers (CLBVHnode.cpp:209-236, CLRaytracer.cpp:122-137).  Plain C types only;
 * every entry point returns 0 (RT_SUCCESS) or a negative cl_int-style code from
 * rt_status.h -- no exception crosses the ABI (the C++ wrapper in rt_cl_compat.hpp
 * turns codes back into the reference's CLException).
 *
 * The kernel "KernelEntry" is precompiled for gfx950 (no runtime JIT).  It takes the
 * reference's 14 argument slots (RenderKernelArgument_t, CLutils.h:11-27):
 *    0 BUFFER_OUT (rt_mem)       4 WIDTH (uint)        8 LIGHT_BOUNCES (int)
 *    1 BUFFER_SCENE (rt_mem)     5 HEIGHT (uint)       9 LIGHT_TYPE (int)
 *    2 BUFFER_NODE (rt_mem)      6 FRAME_COUNT (uint) 10 SKYBOX_INTENSITY (float)
 *    3 BUFFER_MATERIAL (rt_mem)  7 FRAME_SEED (uint)  11-13 CAMERA_POS/FRONT/UP (float3,
 *                                                        16 bytes, w ignored)
 * Buffers hold the CLTriangle / CLLinearBVHNode / CLMaterial bytes of rt_cl_types.h;
 * the output is one 16-byte float3 slot per work-item, as the reference's.
 */
#ifndef RT_HIP_H
#define RT_HIP_H

#include <stddef.h>
#include <stdint.h>

#include "rt_cl_types.h"
#include "rt_status.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rt_context_s* rt_context; /* cl::Context + in-order cl::CommandQueue */
typedef struct rt_mem_s* rt_mem;         /* cl::Buffer */
typedef struct rt_kernel_s* rt_kernel;   /* cl::Kernel */

/* cl_mem_flags values (CL/cl.h) accepted by rtCreateBuffer */
#define RT_MEM_READ_WRITE (1u << 0)
#define RT_MEM_WRITE_ONLY (1u << 1)
#define RT_MEM_READ_ONLY (1u << 2)
#define RT_MEM_COPY_HOST_PTR (1u << 5)

/* RenderKernelArgument_t (CLutils.h:11-27) */
enum rt_kernel_arg {
    RT_ARG_BUFFER_OUT = 0,
    RT_ARG_BUFFER_SCENE = 1,
    RT_ARG_BUFFER_NODE = 2,
    RT_ARG_BUFFER_MATERIAL = 3,
    RT_ARG_WIDTH = 4,
    RT_ARG_HEIGHT = 5,
    RT_ARG_FRAME_COUNT = 6,
    RT_ARG_FRAME_SEED = 7,
    RT_ARG_LIGHT_BOUNCES = 8,
    RT_ARG_LIGHT_TYPE = 9,
    RT_ARG_SKYBOX_INTENSITY = 10,
    RT_ARG_CAMERA_POS = 11,
    RT_ARG_CAMERA_FRONT = 12,
    RT_ARG_CAMERA_UP = 13,
    RT_ARG_COUNT = 14
};

/* ---- reference surface --------------------------------------------------------------- */

/* CLContext::CLContext(platform) (CLutils.cpp:9-35): context + in-order queue on GPU
 * `device_index` (the reference always takes device[0]). */
int rtCreateContext(int device_index, rt_context* out);
int rtReleaseContext(rt_context ctx);

/* cl::Buffer(context, flags, size, host_ptr) (CLBVHnode.cpp:215-236,
 * CLRaytracer.cpp:132-135).  With RT_MEM_COPY_HOST_PTR the device gets a copy of
 * `size` bytes of `host_ptr` and the caller keeps its memory.  Other buffers are
 * zero-filled (the reference leaves the output buffer uninitialised). */
int rtCreateBuffer(rt_context ctx, uint64_t flags, size_t size, const void* host_ptr, rt_mem* out);
int rtReleaseBuffer(rt_mem mem);

/* CLKernel::CLKernel(file, devices) (CLutils.cpp:52-66).  The only kernel name is
 * "KernelEntry"; any other -> RT_INVALID_KERNEL_NAME. */
int rtCreateKernel(rt_context ctx, const char* name, rt_kernel* out);
int rtReleaseKernel(rt_kernel k);

/* CLKernel::SetArgument(index, data, size) (CLutils.cpp:68-77).  Buffer slots take a
 * pointer to an rt_mem and size == sizeof(rt_mem); scalar slots size 4; float3 slots
 * size 16 (the reference's host float3, CLmathlib.hpp:18-54).  Values are copied;
 * they persist across launches (set-then-launch, as in RenderFrame). */
int rtSetKernelArg(rt_kernel k, unsigned index, size_t size, const void* value);

/* CLContext::ExecuteKernel(kernel, workSize) (CLutils.cpp:44-50): one work-item per
 * pixel, 1-D NDRange of `global_work_size` (= width*height in the reference).
 * Asynchronous on the context's in-order stream. */
int rtEnqueueKernel(rt_context ctx, rt_kernel k, size_t global_work_size);
/* Extension: frames FRAME_COUNT .. FRAME_COUNT + n_frames - 1 rendered and accumulated into
 * BUFFER_OUT exactly as n_frames rtEnqueueKernel calls with those frame counts would (the
 * reference's RenderFrame loop, CLRaytracer.cpp:35-47, without the per-frame read-back).  The
 * step schedule runs them as ONE launch over (frame, pixel) work items -- one ramp-up and one
 * drain instead of n_frames -- plus a per-pixel accumulation launch; other schedules launch
 * per frame.  The FRAME_COUNT slot is left unchanged; hit buffers receive the last frame's.
 * The accumulation launch runs on a second stream of the context, overlapping the next
 * fused render; every other call on the context (buffer reads/writes/copies, per-frame
 * launches, rtFinish, rtContextGetStream) is ordered after it, so the context still behaves
 * as one in-order queue.  rtContextSetAccumOverlap(ctx, 0) keeps it on the main stream. */
int rtEnqueueKernelFrames(rt_context ctx, rt_kernel k, size_t global_work_size, unsigned n_frames);

/* CLContext::ReadBuffer (CLutils.cpp:37-42, non-blocking in the reference) and
 * CLContext::Finish (CLutils.h:122-125). */
int rtEnqueueReadBuffer(rt_context ctx, rt_mem mem, int blocking, size_t offset, size_t size,
                        void* dst);
int rtFinish(rt_context ctx);

/* ---- extensions (no reference counterpart) ------------------------------------------- */

int rtEnqueueWriteBuffer(rt_context ctx, rt_mem mem, int blocking, size_t offset, size_t size,
                         const void* src);

/* Math policy of the kernel:
 *   RT_MATH_PINNED    -- bit-identical to the pinned CPU semantics of rt_pinned_math.h (oracle);
 *   RT_MATH_DEVICELIB -- the AMD OpenCL device-library builtins the reference kernel
 *                        gets on this GPU, contraction off, correctly rounded / and sqrt
 *                        (the reference built -ffp-contract=off
 *                        -cl-fp32-correctly-rounded-divide-sqrt);
 *   RT_MATH_SHIPPED   -- default: the reference as clBuildProgram(" -I . ") builds it on this GPU
 *                        (CLutils.cpp:52-66): devicelib builtins plus the compiler's default
 *                        FP contraction and OpenCL C's 2.5-ulp division / 3-ulp sqrt. */
#define RT_MATH_PINNED 0
#define RT_MATH_DEVICELIB 1
#define RT_MATH_SHIPPED 2
int rtKernelSetMathMode(rt_kernel k, int mode);

/* Work schedule of the kernel (same results, different lane scheduling):
 * RT_SCHED_TILES           -- one pixel per lane for all of its bounces (16x16 tiles): the
 *                             reference's own shape (one work-item per pixel);
 * RT_SCHED_STEP (default)  -- per-wave state machine: every step advances each lane by one
 *                             BVH node or one triangle; shading and pixel refill run when
 *                             enough lanes are ready;
 * RT_SCHED_WAVEFRONT       -- wavefront path tracing: per bounce an extend
 *                             launch (traversal only, persistent waves pulling rays from an
 *                             HBM ray queue) and a shade launch (one lane per queued path,
 *                             continuations compacted into the next queue); radiance goes to
 *                             per-frame slots and the fused accumulation launch, for
 *                             rtEnqueueKernel too.  Queues take 72 B per work-item and frame.
 *                             lightBounces outside 1..64 run the step schedule. */
#define RT_SCHED_TILES 0
#define RT_SCHED_STEP 2
#define RT_SCHED_WAVEFRONT 4
/* (1 and 3 -- path regeneration and a per-wave LDS path pool -- were measured slower than
 * RT_SCHED_STEP and retired in round 3: rtKernelSetSchedule returns RT_INVALID_VALUE) */
int rtKernelSetSchedule(rt_kernel k, int sched);

/* Device-side BVH build (extension) over the `n_tris` CLTriangle records of
 * `tris` (file order), for meshes too large to build on the host quickly: the triangles sorted
 * by Morton code, then clustered bottom-up (PLOC: mutual nearest neighbours by union surface
 * area within a window of the sorted order -- SAH-like trees) or split by the radix tree of
 * the codes (a linear BVH, cheaper to build and slower to render; rtBuildBVHEx).  Permutes `tris` in place into leaf order and writes the
 * depth-first CLLinearBVHNode[] into `nodes` (capacity >= (2*n_tris - 1) * 48 bytes), count
 * in *n_nodes -- the node contract of CLBVHnode.cpp:161-183, so the buffers bind to
 * KernelEntry as they are (the tree is the first *n_nodes records; the rest of a 2n-1 buffer is
 * ignored, see rtValidateBVH).  The tree is not the host SAH tree (hit IDs may differ where
 * triangles tie).  Triangles past n_tris and every node record from *n_nodes to the buffer's end
 * keep their bytes.  max_prims_in_node 0 builds as 1, above 65535 as 65535 (nPrimitives has 16
 * bits).  The output is a function of the input alone (one rounding per fp32 operation, a stable
 * sort), and its bounds follow the rule of rtRefitBVH, the fold from +inf / -inf included: a
 * freshly built tree is a fixed point of the refit, for non-finite vertices too.
 * Errors (nothing is written): RT_INVALID_VALUE for a method that is neither RT_BVH_*, n_tris == 0
 * or >= 2^30, or a NULL n_nodes; RT_INVALID_MEM_OBJECT for a NULL buffer, another context's, or
 * tris == nodes (the build would overwrite its own input); RT_INVALID_BUFFER_SIZE for `tris` under
 * n_tris * 256 bytes or `nodes` under (2*n_tris - 1) * 48. */
int rtBuildBVH(rt_context ctx, rt_mem tris, size_t n_tris, unsigned max_prims_in_node, rt_mem nodes,
               size_t* n_nodes);
/* The same with the tree's topology chosen: RT_BVH_PLOC (rtBuildBVH's) or RT_BVH_LBVH. */
#define RT_BVH_LBVH 0
#define RT_BVH_PLOC 1
int rtBuildBVHEx(rt_context ctx, rt_mem tris, size_t n_tris, unsigned max_prims_in_node, int method, rt_mem nodes,
                 size_t* n_nodes);

/* Restrict the next launches to work-items [first, last) (pixel-row tiles for
 * multi-GPU sharding); last = 0 means "to global_work_size".  Work-item ids, and
 * therefore seeds and output slots, stay global. */
int rtKernelSetWorkRange(rt_kernel k, uint64_t first, uint64_t last);

/* Interleaved 8-row bands for load-balanced multi-GPU sharding: the next launches render
 * only the bands b (rows 8b..8b+7 of the work range) with b % period == phase.  (1, 0)
 * = every band.  Not available with RT_SCHED_TILES (RT_INVALID_OPERATION at launch). */
int rtKernelSetRowInterleave(rt_kernel k, unsigned period, unsigned phase);

/* 2-D device copies for packing / unpacking band-interleaved tiles around a collective:
 * `rows` rows of `width_bytes`, source and destination row pitches in bytes. */
int rtEnqueueCopyBufferRectToPointer(rt_context ctx, rt_mem src, size_t src_offset, size_t src_pitch,
                                     size_t width_bytes, size_t rows, void* dst_device, size_t dst_pitch);
int rtEnqueueCopyPointerRectToBuffer(rt_context ctx, const void* src_device, size_t src_pitch, rt_mem dst,
                                     size_t dst_offset, size_t dst_pitch, size_t width_bytes, size_t rows);

/* Primary-ray outputs per work-item: hit primitive index into the BVH-ordered triangle
 * array (-1 = miss) and isect.t.  Pass NULL to disable. Buffers need 4 B per work-item. */
int rtKernelSetHitBuffers(rt_kernel k, rt_mem hit_ids, rt_mem hit_t);

/* Counters (section 8(d) of SURVEY.md): rays = Intersect() calls, node visits,
 * triangle tests, closest hits.  Enabling selects an instrumented kernel variant. */
typedef struct rt_stats {
    uint64_t rays, node_visits, tri_tests, hits;
    uint64_t launches;
    double kernel_ms;  /* sum of KernelEntry durations (HIP events) when timing is on; ray queries
                        * (rtEnqueueIntersectRays), surface records and feature buffers add theirs,
                        * and count in `launches` */
    /* diagnostic (step schedule, stats on): shader-clock cycles summed over waves spent
     * refilling/finishing pixels, traversing, shading, and in total */
    uint64_t cycles_refill, cycles_traverse, cycles_shade, cycles_total;
    /* diagnostic (step schedule, stats on): node steps, lanes served by node steps,
     * triangle steps, lanes served, shading rounds, lanes shaded, refill rounds, lanes freed,
     * then summed over all steps: lanes of the other traversal kind, lanes waiting to shade,
     * free lanes; last, in the default stats build only, the refill's pop iterations (launches with
     * the camera-ray ring; the RT_TIMELINE and RT_LDS_CONFLICTS diagnostic builds keep other
     * things in these words) */
    uint64_t sched[12];
    double accum_ms;   /* sum of the fused frames' accumulation launches (rtEnqueueKernelFrames);
                        * when overlapped (default) the spans include the wait for the render */
    double render_period_ms; /* timed renders: mean interval between the ends of consecutive
                              * launches -- the per-launch time of back-to-back renders, which
                              * overlap (a launch's event span also holds its wait for the CUs
                              * the previous one frees) */
} rt_stats;
int rtKernelSetStats(rt_kernel k, int enable);
int rtKernelSetTiming(rt_kernel k, int enable);
int rtKernelGetStats(rt_kernel k, rt_stats* out);
int rtKernelResetStats(rt_kernel k);

/* The path kill (step schedule).  A path whose throughput (the reference's `beta`) has become exactly
 * (0, 0, 0) can add nothing but +-0 to its pixel; a launch that is certified -- the scene's materials,
 * normals and vertices and the launch's lightType, skyboxIntensity and lightBounces pass a host rule
 * under which no later segment can turn that into NaN -- ends such a path at once, as if its bounces
 * had run out: the same bits, fewer segments.  Launches with stats on are never certified (the
 * counters stay the reference's); they count the segments that reach shading with zero throughput
 * instead, hits and misses apart (together: the segments a certified launch does not walk).
 * scene_certified: the scene half of the rule for the kernel's math mode as of the last launch
 * (0 also after rtRefitBVH, until the next full preparation); launch_certified: whether the last
 * render launch carried the kill.  Synchronises like rtKernelGetStats. */
typedef struct rt_path_kill_info {
    uint64_t zero_hits, zero_misses;
    int32_t scene_certified, launch_certified;
} rt_path_kill_info;
int rtKernelGetPathKill(rt_kernel k, rt_path_kill_info* out);

/* The node collapse (octant-record walks: every schedule on LDS-resident scenes, and the HBM/L2 walk of
 * the regrouped records).  Where a node's near child is interior and has bitwise the node's own box,
 * the child's box test repeats the one just passed; the packed scene keeps a second set of records
 * whose links lead past such children, and launches walk it: the same leaves and triangles in the same
 * order, the same results, fewer node visits.  Launches with stats on walk the plain records (the
 * counters stay the reference's), and so does every launch after rtRefitBVH until the next full
 * preparation, since the refit moves boxes and no links.
 * collapsed_links: link words the second set changes (0: the scene has no such pair);
 * scene_collapsible: the set may be walked as of the last preparation (0 after rtRefitBVH, and in builds
 * with RT_NODE_COLLAPSE=0); launch_collapsed: whether the kernel's last launch -- render, ray query or
 * path trace -- walked it.  Flushes coalesced frames; does not wait for the device. */
typedef struct rt_node_collapse_info {
    uint32_t collapsed_links;
    int32_t scene_collapsible, launch_collapsed;
} rt_node_collapse_info;
int rtKernelGetNodeCollapse(rt_kernel k, rt_node_collapse_info* out);

/* The gate skip (the same walks as the node collapse, which it contains).  In a tree whose every box lies
 * inside its parent's box plane by plane, an interior node's box test decides no result: where it fails,
 * every box below fails too, leaves included, and leaves keep their test.  For such scenes the second set
 * of records leads past the interior nodes whose test costs more visits than it saves (a surface-area
 * estimate, csrc/rt_scene_pack.cpp), in hit and miss links alike, and the third set is built from it: the
 * same leaves and triangles in the same order, the same results.  The conditions are the collapse's: stats
 * launches and launches after rtRefitBVH walk the plain records.
 * gate_links: link words the set changes against the plain one (the collapsed ones among them; 0: the
 * tree does not nest, or a build with RT_GATE_SKIP=0); scene_nested: the scene has such a set and it may be
 * walked as of the last preparation; launch_gate_skipped: whether the kernel's last launch walked it
 * (launch_collapsed is 1 as well then).  Flushes coalesced frames; does not wait for the device. */
typedef struct rt_gate_skip_info {
    uint32_t gate_links;
    int32_t scene_nested, launch_gate_skipped;
} rt_gate_skip_info;
int rtKernelGetGateSkip(rt_kernel k, rt_gate_skip_info* out);

/* The octant cull (the same walks as the node collapse).  RayTriangle rejects det < 1e-8, and for a
 * triangle in an axis plane the sign of det is the sign of one direction component: no ray of four of
 * the eight octants can hit it.  A host certificate (csrc/rt_octant_cull.cpp) decides per triangle and
 * octant whether every evaluation of det, under every math mode, is below 1e-8 or NaN; the packed scene
 * keeps a third set of records, built from the collapsed one, in which no link of an octant leads to a
 * leaf -- or a whole subtree -- whose triangles are all certified for it.  Launches walk it: the same
 * accepted hits, the same results, without the box tests and triangle tests that could accept nothing.
 * The certificate refuses what it cannot prove through fp32 rounding: triangles whose det has two
 * products of one direction component that cancel only in exact arithmetic (the side faces of a box
 * rotated about an axis), triangles so thin that the component's margin is under 2^-18, and vertices
 * that are not finite or lie beyond 2^20.  Launches with stats on walk the plain records, and so does
 * every launch after rtRefitBVH until the next full preparation, since moved vertices are not certified.
 * pruned_links: link words the third set changes against the collapsed one (counted there also for a scene
 * with a gate-skipped set, whose launches walk the pruned form of that set); contracted_links: words
 * changed by contracting interior nodes with one live child (always 0: not built); scene_certified: the
 * set may be walked as of the last preparation (0 after rtRefitBVH, and in builds with RT_OCTANT_CULL=0);
 * launch_pruned: whether the kernel's last launch -- render, ray query or path trace -- walked it
 * (rtKernelGetNodeCollapse's launch_collapsed is 1 as well then: the set contains the collapse).
 * Flushes coalesced frames; does not wait for the device. */
typedef struct rt_octant_cull_info {
    uint32_t pruned_links, contracted_links;
    int32_t scene_certified, launch_pruned;
} rt_octant_cull_info;
int rtKernelGetOctantCull(rt_kernel k, rt_octant_cull_info* out);

/* ---- batched ray queries over caller rays ------------------------------------------------
 * The scene is the one bound to `k` (BUFFER_SCENE, BUFFER_NODE), packed and validated exactly as
 * a render launch does (rtValidateBVH first: RT_INVALID_MEM_OBJECT on a bad tree).  A query runs
 * in k's math mode and honours rtKernelForceGlobalScene; BUFFER_OUT and BUFFER_MATERIAL need not
 * be bound (a bound material buffer is validated as for a render).
 *
 * rtEnqueueIntersectRays answers rays [first_ray, first_ray + n_rays) of `rays` (rt_ray records)
 * into the same slots of `hits` (rt_ray_hit records); the other slots are not touched.  Per ray it
 * is the reference's InitRay(origin, dir) followed by Intersect (kernel_bvh.cl:42-55, 171-219) in
 * the reference's node and triangle order -- `dir` is normalised by the kernel and need not be
 * unit length -- with two generalisations: isect.t starts at `tmax` instead of MAX_RENDER_DIST, and
 * a triangle the reference would accept is accepted only if also t >= tmin.  With tmin = -INFINITY
 * and tmax = 100000.0f the result is Intersect's bit for bit, its negative-t hits and one-sided
 * (det >= 1e-8) culling included; tmin > tmax always misses.
 *   RT_QUERY_CLOSEST  the full walk: the closest accepted triangle.
 *   RT_QUERY_ANY      the same walk stopped at its first accepted triangle (deterministic: the
 *                     closest-hit walk's first acceptance); hits exactly when closest-hit does.
 * A hit writes prim = the index into the BVH-ordered triangle array (as rtKernelSetHitBuffers), t,
 * and the triangle's barycentrics u, v (the hit point is v1 + u (v2 - v1) + v (v3 - v1)); a miss
 * writes {-1, tmax, 0, 0}.
 * Errors (nothing is launched): a mode other than the two RT_INVALID_VALUE; n_rays == 0 RT_SUCCESS
 * with no launch; a missing scene or node buffer RT_INVALID_KERNEL_ARGS; first_ray + n_rays > 2^31
 * RT_INVALID_VALUE; `rays` and `hits` the same buffer RT_INVALID_MEM_OBJECT; first_ray + n_rays
 * beyond either buffer's size RT_INVALID_BUFFER_SIZE; a BVH leaf of more than 127 triangles
 * RT_INVALID_OPERATION (queries walk the octant records, which hold leaves up to that size).
 *
 * rtEnqueueCameraRays writes, for every work-item gid in [0, global_work_size), the primary ray
 * KernelEntry would trace for it with k's current WIDTH, HEIGHT, FRAME_COUNT and camera slots, in
 * k's math mode (seed gid + frame_hash(frameCount)): origin = camPos, tmin = -INFINITY, tmax =
 * 100000.0f, dir = the direction CreateRay hands to InitRay (its normalize(dir), before InitRay
 * normalises again), so feeding the record to rtEnqueueIntersectRays reproduces the primary ray
 * exactly.  rtKernelSetWorkRange and rtKernelSetRowInterleave are ignored: every gid is written.
 * Errors: those slots unset or WIDTH / HEIGHT zero RT_INVALID_KERNEL_ARGS; global_work_size 0 or
 * above 2^32 - 1 RT_INVALID_GLOBAL_WORK_SIZE; `rays` smaller than 32 B per work-item
 * RT_INVALID_BUFFER_SIZE.
 *
 * Both are asynchronous on the context's in-order queue like every other call: coalesced per-frame
 * launches (PERFRAME_BATCH) are launched first, pending fused-frame accumulations are ordered
 * before them, they count as "another call touching the context" for the deferral rules above, and
 * later reads of `hits` / `rays` see the results.  With rtKernelSetStats on, a query adds its rays,
 * node visits, triangle tests and hits to rt_stats (an any-hit query counts only what it walked). */
typedef struct rt_ray {
    float origin[3];
    float tmin;
    float dir[3];
    float tmax;
} rt_ray; /* 32 B */
typedef struct rt_ray_hit {
    int32_t prim;
    float t, u, v;
} rt_ray_hit; /* 16 B */
#define RT_QUERY_CLOSEST 0
#define RT_QUERY_ANY 1
int rtEnqueueIntersectRays(rt_context ctx, rt_kernel k, rt_mem rays, size_t first_ray, size_t n_rays, int mode,
                           rt_mem hits);
int rtEnqueueCameraRays(rt_context ctx, rt_kernel k, size_t global_work_size, rt_mem rays);

/* ---- path tracing over caller rays -----------------------------------------------------------
 * rtEnqueueTracePaths runs the reference's Render (kernel_bvh.cl:349-384) for records [first,
 * first + n) of `rays` (rt_ray) and writes the same slots of `out` (rt_path_result); the other slots
 * are not touched.  The scene, the material buffer, LIGHT_BOUNCES, LIGHT_TYPE and SKYBOX_INTENSITY
 * are those bound to `k`; the scene is prepared exactly as a render launch prepares it (rtValidateBVH
 * and the material check included).  The call runs in k's math mode and honours
 * rtKernelForceGlobalScene.  WIDTH, HEIGHT, FRAME_COUNT, the camera slots and BUFFER_OUT are not read
 * and need not be set.
 * Per record i (the absolute index): seed = seeds ? seeds[i] : params->seed_base + (uint32_t)i, with
 * uint32 wrap (seed_base is ignored when `seeds` is given); ray = InitRay(origin, dir), `dir`
 * normalised as the query normalises it; then Render(&ray, &scene, &seed): every Intersect in the
 * reference's node and triangle order, shading and RNG draws those of the render kernels.  One
 * generalisation, for the first segment only and the query's: isect.t starts at the record's tmax and
 * a triangle is accepted only if t >= tmin; later segments are the reference's Intersect.  With tmin =
 * -INFINITY and tmax = 100000.0f the whole path is the reference's bit for bit.  A first segment that
 * misses inside its window adds the sky term and ends the path, as a miss does.
 *   radiance  RT_TRACE_LINEAR: max(radiance, 0) per channel, as Render returns it.  RT_TRACE_FRAME0:
 *             that value as KernelEntry stores it at frameCount == 0, pow(., 0.45454545f) in k's
 *             math mode.
 *   prim      the first segment's hit primitive (as rtKernelSetHitBuffers' id), -1 on a miss and
 *             when LIGHT_BOUNCES is 0 (radiance 0 then).
 * Non-finite origins or directions may produce any radiance; every walk still ends, and no value
 * from `rays` or `seeds` ever becomes an address.
 * Ordering is a query's: asynchronous on the context's in-order queue, coalesced per-frame launches
 * first, after the pending accumulations, "another call touching the context" for the deferral
 * rules; `out` counts as written.  With rtKernelSetStats on it adds rays (one per Intersect), node
 * visits, triangle tests and hits; with timing on, kernel_ms and launches.  After
 * rtEnqueueUpdateVertices + rtRefitBVH it sees the moved geometry without a full preparation.
 * Errors (nothing is launched), in this order after the context and the kernel: `params` NULL or an
 * encoding other than the two RT_INVALID_VALUE; first + n > 2^31 RT_INVALID_VALUE; `rays` or `out`
 * NULL or of another context, a non-NULL `seeds` of another context, or `out` the same buffer as
 * `rays` or `seeds` RT_INVALID_MEM_OBJECT; the range beyond any buffer (32, 4 and 16 B per record)
 * RT_INVALID_BUFFER_SIZE; scene, node or material slot unbound, or LIGHT_BOUNCES, LIGHT_TYPE or
 * SKYBOX_INTENSITY unset RT_INVALID_KERNEL_ARGS; a BVH leaf of more than 127 triangles
 * RT_INVALID_OPERATION; n == 0 RT_SUCCESS with no launch.
 *
 * rtEnqueueCameraPaths writes `rays` byte for byte as rtEnqueueCameraRays does (same errors) and
 * seeds[gid], the RNG state after CreateRay's two draws: the reference's HashUInt32 applied twice to
 * gid + frame_hash(FRAME_COUNT).  Feeding both buffers to rtEnqueueTracePaths continues exactly the
 * path KernelEntry traces for that work-item.  Extra errors: `seeds` NULL, of another context or the
 * same buffer as `rays` RT_INVALID_MEM_OBJECT; `seeds` smaller than 4 B per work-item
 * RT_INVALID_BUFFER_SIZE. */
typedef struct rt_path_result {
    float radiance[3];
    int32_t prim;
} rt_path_result; /* 16 B */
#define RT_TRACE_LINEAR 0 /* max(radiance, 0) as Render returns it */
#define RT_TRACE_FRAME0 1 /* the value KernelEntry stores at frameCount == 0 */
typedef struct rt_trace_params {
    uint32_t seed_base;
    int encoding;
} rt_trace_params;
/* (kernel_bvh.cl:378, the analytic light's term, follows rtKernelSetShadowRays below) */
int rtEnqueueTracePaths(rt_context ctx, rt_kernel k, rt_mem rays, rt_mem seeds /* may be NULL */, size_t first,
                        size_t n, const rt_trace_params* params, rt_mem out);
int rtEnqueueCameraPaths(rt_context ctx, rt_kernel k, size_t global_work_size, rt_mem rays, rt_mem seeds);

/* ---- shadow rays for the analytic light (extension) ---------------------------------------------
 * The reference's Render adds lightPixel(...) * diffuse * beta at every shaded hit (kernel_bvh.cl:378) and
 * casts no shadow ray: its light shines through walls.  rtKernelSetShadowRays(k, 1) makes
 * rtEnqueueTracePaths and rtEnqueueSamplePixels test that term against the scene first; 0, the default,
 * is the reference.  It is a kernel setting like the math mode: it flushes the held frames as every
 * kernel setting does and costs nothing until one of those two calls reads it.
 * rtEnqueueKernel, rtEnqueueKernelFrames under every schedule, the ray queries, the surface, feature and
 * motion passes do not read it: they are the reference's KernelEntry and stay bit for bit what they are
 * whatever the setting.
 *
 * With the setting on, Render is the reference's with one change at line 378.  Let lp be lightPixel's
 * value for the hit, evaluated exactly where the reference evaluates it (after beta *= mul).
 *   !(lp > 0.0f)  (zero, negative, NaN): line 378 executes as in the reference.  No shadow ray is traced
 *                 and nothing is counted.
 *   otherwise     one shadow ray is answered with the semantics of RT_QUERY_ANY for the rt_ray
 *                 {origin = isect.pos, tmin = 0.01f, dir = L, tmax = T} in k's math mode: isect.pos is the
 *                 hit position ray.origin + ray.dir * t, the value the next ray's origin is formed from;
 *                 for LIGHT_TYPE <= 0, L = -lightDirection = (0.5, -0.4, 0.1) and T = 100000.0f; for
 *                 LIGHT_TYPE >= 1, L = lightPosition - X, the vector lightPixel forms, and
 *                 T = sqrt(dot(L, L)).  The query's InitRay normalises L, so t is in world units.  The
 *                 triangle test is the reference's one-sided RayTriangle with the query's two
 *                 generalisations (isect.t starts at T; an accepted triangle also needs t >= tmin) and
 *                 nothing else: an occluder blocks only if the reference's test would accept it, and hits
 *                 with t < 0.01 -- the surface itself, a duplicated face -- are discarded.
 *                 If the query hits, line 378 is skipped: radiance keeps its bits.  If it misses, line 378
 *                 executes as in the reference.
 * No RNG draw is added or moved; beta, the next ray (line 379) and every later segment are the
 * reference's.  The shadow ray is cast wherever line 378 is reached, on the last bounce too.
 * With rtKernelSetStats on, each shadow ray adds one to rays plus the node visits and triangle tests it
 * walked (an any-hit walk counts only what it walked); hits stays the count of shaded surface hits.
 * Shadow walks read the record set of the launch's other walks (plain, collapsed or pruned; after a
 * refit the moved boxes).  With the setting off every result and every counter is what it was before the
 * setting existed.
 * Errors: a NULL kernel RT_INVALID_KERNEL; `enable` other than 0 or 1, or a NULL `enable` pointer,
 * RT_INVALID_VALUE (the setting keeps its value). */
int rtKernelSetShadowRays(rt_kernel k, int enable);
int rtKernelGetShadowRays(rt_kernel k, int* enable);

/* ---- adaptive sampling: per-pixel sample statistics and selection (extension) ------------------
 * Four calls that let a progressive renderer put its paths where the noise is: per-pixel statistics
 * of linear path results, the selection of the pixels that still need samples as a compacted list in
 * ascending order, camera paths for such a list, and the resolve of the statistics into the
 * {r, g, b, w} image rtEnqueueDenoise and rtEnqueueTemporalAccumulate take.  One round is
 *   rtEnqueueSelectPixels -> read `result` -> rtEnqueueCameraPathsFor -> rtEnqueueTracePaths
 *   (RT_TRACE_LINEAR) -> rtEnqueueAccumulateSamples, each over records [0, selected).
 *
 * Every operation below is one correctly rounded fp32 operation; nothing is contracted, denormals are
 * kept, `/` is the IEEE division, comparisons are IEEE comparisons (false for a NaN).  The definition
 * is the same in every math mode of `k`, except where rtEnqueueCameraPathsFor says otherwise.
 *
 * rt_pixel_stats, 32 B per pixel, all zero = no samples: the sum of the samples' linear radiance, the
 * sample count n (an integer value held as a float, exact to 2^24), and Welford's running mean and sum
 * of squared deviations of the samples' luminance.  reserved[2] is kept as found.
 *
 * 1. rtEnqueueAccumulateSamples, for records i in [first, first + n): p = ids[i] (uint32; `ids` may be
 *    NULL, then p = i), s = results[i].radiance (an rt_path_result as RT_TRACE_LINEAR writes it).  The
 *    record is skipped and stats[p] left untouched when p >= n_pixels (a value from `ids` becomes an
 *    address only after this test) or a channel c of s is not finite, !(fabsf(c) <= FLT_MAX).
 *    Otherwise, on stats[p]:
 *      y       = (0.2126f * s.r + 0.7152f * s.g) + 0.0722f * s.b
 *      n'      = n + 1.0f
 *      d       = y - mean_y
 *      mean_y' = mean_y + d / n'
 *      m2_y'   = m2_y + d * (y - mean_y')
 *      sum'    = sum + s            per channel
 *    The ids of one call are meant to be distinct; if they are not, the record of a repeated pixel ends
 *    as some mixture of its duplicates' updates and nothing outside that record is touched.  Several
 *    samples per pixel are several calls; the in-order queue fixes their order.
 *    Errors, in this order after the context and the kernel: first + n > 2^31, n_pixels 0 or above 2^31
 *    RT_INVALID_VALUE; `results` or `stats` NULL or of another context, a non-NULL `ids` of another
 *    context, or `stats` the same buffer as `ids` or `results` RT_INVALID_MEM_OBJECT; the range beyond
 *    `ids` (4 B per record) or `results` (16 B), or `stats` under 32 * n_pixels bytes
 *    RT_INVALID_BUFFER_SIZE; n == 0 RT_SUCCESS with no launch.
 *
 * 2. rtEnqueueSelectPixels.  Pixel p = (x, y) is record y * width + x of `stats`, which is only read.
 *    A pixel q with n >= 2.0f is hot exactly when
 *      v = (m2_y / (n - 1.0f)) / n
 *      b = threshold * (mean_y + floor_y)
 *      v > b * b
 *    (the variance of the mean luminance above the square of the allowed error); a pixel with fewer than
 *    two samples is not hot.  Pixel p is selected when n_p < (float)min_samples, not selected when n_p >=
 *    (float)max_samples, and otherwise selected exactly when some q with |dx|, |dy| <= radius inside the
 *    image is hot.  ids[0 .. selected) receives the selected pixel indices in ascending order, the slots
 *    from `selected` on keep their bytes, and `result` receives {selected, number of hot pixels, 0, 0}.
 *    The result is a function of the inputs alone: the compaction is an ordered one (per-block counts, a
 *    scan of the block counts, ballot / lane-prefix ranks inside a wave), no atomic append.  Its scratch
 *    belongs to the kernel object, grown before anything is enqueued and freed at release.
 *    Errors: `params` NULL, threshold or floor_y negative, not finite or above 2^20, min_samples >
 *    max_samples, max_samples 0 or above 2^20, radius > 2, width or height zero, width * height > 2^31
 *    RT_INVALID_VALUE; a buffer NULL or of another context, or `ids` or `result` the same buffer as
 *    `stats` or as each other RT_INVALID_MEM_OBJECT; `stats` under 32 B per pixel, `ids` under 4 B per
 *    pixel or `result` under 16 B RT_INVALID_BUFFER_SIZE.
 *
 * 3. rtEnqueueCameraPathsFor: for records i in [first, first + n), rays[i] and seeds[i] receive exactly
 *    the bytes rtEnqueueCameraPaths writes to rays[gid] and seeds[gid] for gid = ids[i], from k's current
 *    WIDTH, HEIGHT, FRAME_COUNT and camera slots, in k's math mode.  Any uint32 is a valid gid: it only
 *    enters arithmetic, as get_global_id(0) does in CreateRay.
 *    Errors, in this order: one of those slots unset, or WIDTH or HEIGHT zero RT_INVALID_KERNEL_ARGS;
 *    first + n > 2^31 RT_INVALID_VALUE; a buffer NULL or of another context, or `rays` or `seeds` the
 *    same buffer as `ids` or as each other RT_INVALID_MEM_OBJECT; the range beyond any buffer (4, 32 and
 *    4 B per record) RT_INVALID_BUFFER_SIZE; n == 0 RT_SUCCESS with no launch.
 *
 * 4. rtEnqueueResolveSamples: out[p] = {g(sum.r / n), g(sum.g / n), g(sum.b / n), n} with g(x) =
 *    pm_pow(x, 0.45454545f) of rt_pinned_math.h in every math mode; a pixel with n == 0 gets sixteen
 *    zero bytes.  The layout is BUFFER_OUT's with w the sample count, so the result feeds
 *    rtEnqueueDenoise and rtEnqueueTemporalAccumulate (history_frames = 0) as it is.  Bytes of `out` past
 *    width * height * 16 are not touched.  Behaviour is specified for finite, non-negative sums; other
 *    values may propagate in any way, but none becomes an address.
 *    Errors: width or height zero, width * height > 2^31 RT_INVALID_VALUE; a buffer NULL or of another
 *    context, or `out` the same buffer as `stats` RT_INVALID_MEM_OBJECT; `stats` under 32 B per pixel or
 *    `out` under 16 B RT_INVALID_BUFFER_SIZE.
 *
 * Ordering of all four is a query's: asynchronous on the context's in-order queue, coalesced per-frame
 * launches first, after the pending accumulations, "another call touching the context" for the
 * deferral rules; `stats` (call 1), `ids` and `result`, `rays` and `seeds`, and `out` count as written.
 * With timing on each call adds to kernel_ms and counts as one launch.  No scene need be bound for
 * calls 1, 2 and 4. */
typedef struct rt_pixel_stats {
    float sum[3];   /* sum of the samples' linear radiance */
    float n;        /* samples taken */
    float mean_y;   /* running mean of the luminance */
    float m2_y;     /* running sum of squared deviations of the luminance */
    uint32_t reserved[2];
} rt_pixel_stats; /* 32 B */
typedef struct rt_adaptive_params {
    float threshold;      /* relative standard error of the mean luminance above which a pixel is hot */
    float floor_y;        /* added to the mean luminance, so that dark pixels do not dominate */
    uint32_t min_samples; /* a pixel below this count is always selected */
    uint32_t max_samples; /* a pixel at or above this count is never selected */
    uint32_t radius;      /* 0..2: Chebyshev distance within which a hot pixel selects its neighbours */
} rt_adaptive_params; /* 20 B */
typedef struct rt_select_result { uint32_t selected, hot, reserved[2]; } rt_select_result; /* 16 B */
int rtEnqueueAccumulateSamples(rt_context ctx, rt_kernel k, rt_mem ids /* may be NULL */, rt_mem results, size_t first,
                               size_t n, size_t n_pixels, rt_mem stats);
int rtEnqueueSelectPixels(rt_context ctx, rt_kernel k, rt_mem stats, unsigned width, unsigned height,
                          const rt_adaptive_params* params, rt_mem ids, rt_mem result);
int rtEnqueueCameraPathsFor(rt_context ctx, rt_kernel k, rt_mem ids, size_t first, size_t n, rt_mem rays, rt_mem seeds);
int rtEnqueueResolveSamples(rt_context ctx, rt_kernel k, rt_mem stats, unsigned width, unsigned height, rt_mem out);

/* ---- adaptive sampling: one sample for the listed pixels in one launch (extension) ----------------
 * rtEnqueueSamplePixels is the round's three calls -- rtEnqueueCameraPathsFor, rtEnqueueTracePaths
 * (RT_TRACE_LINEAR, the seeds given) and rtEnqueueAccumulateSamples -- as one kernel that keeps the ray,
 * the seed and the radiance in registers, and that can take its record count from device memory, so that a
 * round needs no host read:
 *   rtEnqueueSelectPixels -> rtEnqueueSamplePixels(ids, count = the select's `result`, n = width * height).
 *
 * Let m = n when `count` is NULL, else m = min(n, c) with c the first uint32 of `count`
 * (rt_select_result.selected) as it stands when the launch runs.  The word is compared and clamped against
 * n, which the host has range-checked; it never forms an address.  For records i in [first, first + m),
 * gid = ids[i]:
 *   - gid >= n_pixels: the record is skipped before anything is traced; stats is untouched and nothing of
 *     it is counted in rt_stats.  (A gid becomes an address only after this test.)
 *   - otherwise {ray, seed} are exactly what rtEnqueueCameraPathsFor writes for gid (k's WIDTH, HEIGHT,
 *     FRAME_COUNT and camera slots, in k's math mode), s is the radiance rtEnqueueTracePaths returns for
 *     that ray and seed (RT_TRACE_LINEAR; scene, materials, LIGHT_BOUNCES, LIGHT_TYPE, SKYBOX_INTENSITY and
 *     rtKernelForceGlobalScene as bound to k), and stats[gid] receives rtEnqueueAccumulateSamples' update by
 *     s: the non-finite skip applies, reserved[2] is kept as found, mean_y' = mean_y + d / n' is the IEEE
 *     quotient in every math mode, and a LIGHT_BOUNCES of 0 adds a zero sample as the composed calls do.
 * `stats` ends with the bytes the three calls leave over the same range with n replaced by m, in every math
 * mode.  Repeated ids: some mixture of the duplicates' updates, nothing outside that record.  Records of
 * `ids` and `stats` outside those named are not touched; `ids` and `count` are only read.  A device count
 * of 0 still launches; the kernel finds nothing to do.
 *
 * Ordering is a query's (queued, coalesced frames first, after the pending accumulations, "another call
 * touching the context"); `stats` counts as written.  With stats on it adds rays, node visits, triangle
 * tests and hits as rtEnqueueTracePaths would for the in-range records; with timing on it is one launch.
 * After rtEnqueueUpdateVertices + rtRefitBVH it sees the moved geometry without a full preparation, and it
 * walks the node-collapse records whenever the trace would.
 *
 * Errors (nothing prepared or launched), in this order after the context and the kernel: first + n > 2^31,
 * n_pixels 0 or above 2^31 RT_INVALID_VALUE; `ids` or `stats` NULL or of another context, a non-NULL
 * `count` of another context, `stats` the same buffer as `ids` or `count`, or `count` the same buffer as
 * `ids` RT_INVALID_MEM_OBJECT; the range beyond `ids` (4 B per record), `count` under 16 B or `stats` under
 * 32 * n_pixels bytes RT_INVALID_BUFFER_SIZE; one of WIDTH, HEIGHT, FRAME_COUNT or the camera slots unset,
 * WIDTH or HEIGHT zero, the scene, node or material slot unbound, or LIGHT_BOUNCES, LIGHT_TYPE or
 * SKYBOX_INTENSITY unset RT_INVALID_KERNEL_ARGS; n == 0 RT_SUCCESS with nothing prepared or launched; then
 * the scene preparation's own errors, and a leaf of more than 127 triangles RT_INVALID_OPERATION. */
/* (the analytic light's term follows rtKernelSetShadowRays, as in rtEnqueueTracePaths) */
int rtEnqueueSamplePixels(rt_context ctx, rt_kernel k, rt_mem ids, rt_mem count /* may be NULL */, size_t first,
                          size_t n, size_t n_pixels, rt_mem stats);

/* ---- surface records of ray hits, and first-hit feature buffers ----------------------------
 * rtEnqueueHitSurfaces writes, for records [first, first + n) of `rays` (rt_ray) and `hits`
 * (rt_ray_hit), the same slots of `surfaces` (rt_surface); the other slots are not touched.  The
 * scene is the one bound to `k`, prepared exactly as a query prepares it, and the call runs in k's
 * math mode M.  u, v and t are taken from the hit record as they are: nothing is intersected again.
 * Per record with 0 <= prim < the scene's triangle count:
 *   position    origin' + dir' * t of the ray InitRay(origin, dir) makes (kernel_bvh.cl:42-55, :144):
 *               dir is normalised as the query normalised it.
 *   normal      normalize(n1 * w + (n2 * u + n3 * v)), w = (1 - u) - v (kernel_bvh.cl:146) -- computed
 *               by the device code the render shades with, so it is the render's normal in mode M,
 *               bit for bit.
 *   texcoord    the same weights over v1/v2/v3.uv.xy (kernel_bvh.cl:147); not normalised.
 *   geo_normal  normalize(cross(v2 - v1, v3 - v1)); the zero vector for a zero-area triangle.
 *   material    the triangle's mtlIndex.  The material buffer is not read and need not be bound.
 *   t, prim     copied from the hit; reserved is written as 0.
 * Any other prim is a miss: prim = -1, t copied, material = 0xFFFFFFFF, every other word 0.  The hit
 * buffer is the caller's to write, so an index outside the triangle array is never used as one.
 * Errors (nothing is launched), checked in this order: first + n > 2^31 RT_INVALID_VALUE; `surfaces`
 * the same buffer as `rays` or `hits`, a buffer of another context or NULL, or `rays` and `hits` one
 * buffer, RT_INVALID_MEM_OBJECT; the range beyond any of the three buffers (32, 16 and 64 B per
 * record) RT_INVALID_BUFFER_SIZE; scene or node slot unbound RT_INVALID_KERNEL_ARGS; n == 0
 * RT_SUCCESS with no launch.
 * Ordering is a query's: asynchronous on the context's in-order queue, coalesced per-frame launches
 * first, after the pending accumulations; `surfaces` counts as written for the buffers' generations;
 * with timing on the launch adds to kernel_ms and `launches`.  After rtEnqueueUpdateVertices +
 * rtRefitBVH it sees the moved positions and normals without a full preparation.
 *
 * rtEnqueueFrameFeatures writes per work-item gid in [0, global_work_size) the first-hit features of
 * frames FRAME_COUNT .. FRAME_COUNT + n_frames - 1 (uint32 wrap), averaged over the same jittered
 * camera rays the render traces for them.  Four sums start at +0.0f; per frame, in frame order, the
 * ray is rtEnqueueCameraRays' record for gid, the hit its RT_QUERY_CLOSEST answer, and a hit adds --
 * one fp32 addition each -- materials[material].diffuse.xyz to albedo, the surface normal to normal, t
 * to depth and 1.0f to coverage; a miss adds nothing.  After the last frame every sum is multiplied
 * once by 1.0f / (float)n_frames (the IEEE quotient in every math mode).  The mean normal is not
 * normalised again.  `features` is never read, FRAME_COUNT stays as set, and work range and row
 * interleave are ignored as for rtEnqueueCameraRays.  It runs as three launches per frame on the
 * context's queue (camera rays, closest-hit query, the surface kernel folding into `features`) over
 * 48 B of scratch per work-item that the kernel object owns, grows before anything is enqueued and
 * frees when it is released; nothing waits on the host.  With timing on the whole call counts as one
 * launch.
 * Errors (nothing is launched): n_frames 0 or above 4096 RT_INVALID_VALUE; WIDTH, HEIGHT,
 * FRAME_COUNT or a camera slot unset, WIDTH or HEIGHT zero, or scene, node or material slot unbound
 * RT_INVALID_KERNEL_ARGS; global_work_size 0 or above 2^32 - 1 RT_INVALID_GLOBAL_WORK_SIZE;
 * `features` smaller than 32 B per work-item RT_INVALID_BUFFER_SIZE; a BVH leaf of more than 127
 * triangles RT_INVALID_OPERATION; `features` NULL or of another context RT_INVALID_MEM_OBJECT. */
typedef struct rt_surface {
    float position[3];   float    t;           /* t copied from the hit */
    float normal[3];     int32_t  prim;        /* shading normal; prim copied, -1 = miss */
    float geo_normal[3]; uint32_t material;    /* mtlIndex of the triangle; 0xFFFFFFFF on a miss */
    float texcoord[2];   uint32_t reserved[2]; /* written as 0 */
} rt_surface; /* 64 B */
typedef struct rt_pixel_features {
    float albedo[3]; float depth;
    float normal[3]; float coverage;
} rt_pixel_features; /* 32 B */
int rtEnqueueHitSurfaces(rt_context ctx, rt_kernel k, rt_mem rays, rt_mem hits, size_t first, size_t n,
                         rt_mem surfaces);
int rtEnqueueFrameFeatures(rt_context ctx, rt_kernel k, size_t global_work_size, unsigned n_frames, rt_mem features);

/* ---- feature-guided denoiser (extension) -----------------------------------------------------
 * rtEnqueueDenoise filters a rendered image on the device with an edge-avoiding a-trous wavelet
 * filter (Dammertz et al. 2010) guided by the buffer rtEnqueueFrameFeatures writes.  `image` and `out`
 * hold width * height slots of 16 B, {r, g, b, w} fp32 (BUFFER_OUT's layout, and a gathered image's);
 * `features` holds as many rt_pixel_features.  Pixel p = (x, y) is record y * width + x.  The filter
 * is one definition in every math mode of `k`; every operation below is one correctly rounded fp32
 * operation, nothing is contracted and denormals are kept.
 *   iterations  i = 0 .. params->iterations - 1 with step s = 2^i; iteration 0 reads `image`, every
 *               later one the output of the one before; the features are the same in all of them.
 *   taps        q = p + s * (dx, dy), dy outer and dx inner, each -2 .. 2 in that order, with kernel
 *               weight k = h[dy + 2] * h[dx + 2], h = {1/16, 1/4, 3/8, 1/4, 1/16}.  A tap whose q lies
 *               outside the image or has coverage_q == 0 is skipped: it adds nothing.
 *   centre      a pixel with coverage_p == 0 is copied unchanged, all 16 bytes.
 *   weight      dot3(a) = (a.x * a.x + a.y * a.y) + a.z * a.z;  e(x) = m * m, m = max(0, 1 - x).
 *               With c the iteration's input colour:
 *                 x_c = dot3(c_p - c_q) * inv_c[i]          x_n = dot3(normal_p - normal_q) * inv_n
 *                 d = (depth_p - depth_q) * rz_p,  x_z = (d * d) * inv_z,
 *                     rz_p = 1.0f / max(fabsf(depth_p), 0x1p-64f), once per centre
 *                 x_a = dot3(albedo_p - albedo_q) * inv_a
 *                 w = (((k * e(x_c)) * e(x_n)) * e(x_z)) * e(x_a)
 *               inv_X = 1.0f / (sigma_X * sigma_X), computed on the host in fp32; for colour the sigma
 *               of iteration i is ldexpf(sigma_color, -i) (the tolerance halves per iteration).  A
 *               sigma of 0 disables its term: it is left out of the product.
 *   sums        sum_w += w; sum_r += w * c_q.r; likewise g and b; all four start at +0.0f.
 *   output      rgb = sum_rgb / sum_w, three IEEE divisions (the centre tap has w = 9/64, so sum_w > 0);
 *               the w slot is that pixel's w slot of `image`, carried through every iteration.
 * Behaviour is specified for finite inputs.  Non-finite pixel or feature values may propagate in any
 * way, but no value of either buffer ever becomes an address.
 * Two or more iterations alternate between `out` and one scratch image of 16 B per pixel that the
 * kernel object owns, grows before anything is enqueued and frees when it is released: iteration i
 * writes `out` when iterations - 1 - i is even, else the scratch, so the last one lands in `out`.
 * `image` and `features` are never written, and bytes of `out` past width * height * 16 are not touched.
 * No scene need be bound to `k`.
 * Ordering is a query's: asynchronous on the context's in-order queue, coalesced per-frame launches
 * first, after the pending accumulations; `out` counts as written for the buffers' generations; with
 * timing on the whole call adds to kernel_ms and counts as one launch.
 * Errors (nothing is launched or allocated), checked in this order after the context and the kernel:
 * params NULL, iterations outside 1 .. 5, a sigma that is negative, not finite, in (0, 2^-20) or above
 * 2^20, width or height zero, or width * height > 2^31 RT_INVALID_VALUE; a buffer that is NULL or
 * another context's, or `out` the same buffer as `image` or `features`, RT_INVALID_MEM_OBJECT; any of
 * the three buffers too small RT_INVALID_BUFFER_SIZE. */
typedef struct rt_denoise_params {
    unsigned iterations;
    float sigma_color, sigma_normal, sigma_depth, sigma_albedo;
} rt_denoise_params;
int rtEnqueueDenoise(rt_context ctx, rt_kernel k, rt_mem image, rt_mem features, unsigned width, unsigned height,
                     const rt_denoise_params* params, rt_mem out);

/* ---- variance-guided denoiser over the adaptive sample statistics (extension) ------------------
 * rtEnqueueDenoiseSamples filters what adaptive sampling has gathered with the a-trous filter above, on
 * linear radiance and with the edge-stopping function of SVGF (Schied et al. 2017): the luminance
 * tolerance of every centre is proportional to the standard deviation of that pixel's mean, which the
 * statistics hold, and the variance is filtered along with the colour.  A pixel of 4 samples is
 * smoothed hard and a converged one barely.  `stats` holds width * height rt_pixel_stats, `features` as
 * many rt_pixel_features, `out` as many slots of 16 B {r, g, b, sample count} (rtEnqueueResolveSamples'
 * layout) and `variance`, which may be NULL, as many floats.  Pixel p = (x, y) is record y * width + x.
 * The filter is one definition in every math mode of `k`; every operation below is one correctly
 * rounded fp32 operation, nothing is contracted, denormals are kept, `/` and sqrtf are IEEE, and
 * comparisons are IEEE comparisons (false for a NaN).
 *   input       of iteration 0, per pixel q from stats[q]:
 *                 c_q = sum / n, three divisions
 *                 v_q = n >= 2.0f ? (m2_y / (n - 1.0f)) / n : mean_y * mean_y
 *               (the variance of the mean luminance; a single sample is taken to be as uncertain as it
 *               is bright).  A pixel with !(n >= 1.0f) has c_q = 0 and v_q = -1.0f.
 *   counting    a pixel counts when coverage_q != 0 && v_q >= 0.0f: the one rule in every iteration,
 *               decided from the iteration's input alone.  A negative or NaN variance never enters a sum.
 *   luminance   l(c) = (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b
 *   iterations  i = 0 .. params->iterations - 1 with step s = 2^i; the input of a later iteration is the
 *               {r, g, b, v} image of the one before; the features are the same in all of them.
 *   centre      a centre that does not count keeps its {r, g, b, v} unchanged.
 *   tolerance   for a centre that counts, once per centre: over the taps q = p + s * (dx, dy), dy outer
 *               and dx inner, each -1 .. 1, that lie inside the image and count, with weight
 *               g = g1[dy + 1] * g1[dx + 1], g1 = {1/4, 1/2, 1/4}:  sg += g; sv += g * v_q; both from
 *               +0.0f.  gv = sv / sg;  tol = sigma_luminance * sqrtf(gv) + epsilon.  (At step 1 SVGF's
 *               3 x 3 Gaussian of the variance; at larger steps taken at the tap spacing.)
 *   taps        the 25 taps and their weight k are rtEnqueueDenoise's.  A tap outside the image or one
 *               that does not count adds nothing.  With dot3, e, x_n, x_z, rz_p, x_a, inv_n, inv_z and
 *               inv_a as defined there and x_l = fabsf(l(c_p) - l(c_q)) / tol:
 *                 w = (((k * e(x_l)) * e(x_n)) * e(x_z)) * e(x_a)
 *               A sigma of 0 disables its term: it is left out of the product.
 *   sums        sw += w; s_r += w * c_q.r, likewise g and b; s_v += (w * w) * v_q; all from +0.0f.
 *   result      rgb = s_rgb / sw, three divisions; v' = s_v / (sw * sw).
 *   output      after the last iteration, with n_p read from stats[p]: out[p] = {enc(r), enc(g),
 *               enc(b), n_p}, enc(x) = x for RT_DENOISE_LINEAR and pm_pow(x, 0.45454545f) of
 *               rt_pinned_math.h for RT_DENOISE_GAMMA (rtEnqueueResolveSamples' encoding); variance[p]
 *               = v', or the carried v of a centre that does not count.  A pixel with !(n_p >= 1.0f)
 *               gets sixteen zero bytes and variance +0.0f.
 * Behaviour is specified for finite inputs.  Others may propagate in any way, but no value of `stats` or
 * `features` ever becomes an address, and skipped taps and disabled terms are dropped by select, never
 * by a multiplication.
 * Two or more iterations alternate between `out` and the scratch image rtEnqueueDenoise uses, by its
 * rule: the last iteration lands in `out`; the scratch is grown before anything is enqueued.  `stats`
 * and `features` are never written, bytes of `out` past width * height * 16 and of `variance` past
 * width * height * 4 are not touched, and no scene need be bound to `k`.
 * Ordering is rtEnqueueDenoise's: asynchronous on the context's in-order queue, coalesced per-frame
 * launches first, after the pending accumulations; `out` and `variance` count as written; with timing
 * on the whole call adds to kernel_ms and counts as one launch.
 * Errors (nothing is launched or allocated), checked in this order after the context and the kernel:
 * RT_INVALID_VALUE for params NULL, iterations outside 1 .. 5, one of the four sigmas negative, not
 * finite, in (0, 2^-20) or above 2^20, epsilon not finite or outside [2^-40, 2^20], an encoding other
 * than the two, width or height zero, or width * height > 2^31; RT_INVALID_MEM_OBJECT for a required
 * buffer that is NULL or another context's, a non-NULL `variance` of another context, or `out` or
 * `variance` the same buffer as an input or as each other; RT_INVALID_BUFFER_SIZE for `stats` or
 * `features` under 32 B per pixel, `out` under 16 B or `variance` under 4 B. */
#define RT_DENOISE_LINEAR 0   /* rgb as filtered */
#define RT_DENOISE_GAMMA  1   /* pm_pow(rgb, 0.45454545f) of rt_pinned_math.h, as rtEnqueueResolveSamples */
typedef struct rt_denoise_samples_params {
    unsigned iterations;        /* 1 .. 5 */
    float sigma_luminance;      /* tolerance in standard deviations of the mean; 0 leaves the term out */
    float sigma_normal, sigma_depth, sigma_albedo;   /* exactly rt_denoise_params' */
    float epsilon;              /* added to the luminance tolerance, in [2^-40, 2^20] */
    int encoding;               /* RT_DENOISE_LINEAR / RT_DENOISE_GAMMA */
} rt_denoise_samples_params;
int rtEnqueueDenoiseSamples(rt_context ctx, rt_kernel k, rt_mem stats, rt_mem features, unsigned width,
                            unsigned height, const rt_denoise_samples_params* params, rt_mem out,
                            rt_mem variance /* may be NULL: 4 B per pixel */);

/* ---- temporal reprojection (extension) --------------------------------------------------------
 * rtEnqueueTemporalAccumulate carries an image across a camera move: for every pixel of the current
 * view it rebuilds the world point from the feature buffer's depth, projects it into the previous
 * camera, fetches the previous image bilinearly from the taps that lie on the same surface, and blends
 * it with the current frames by per-pixel sample count.  `cur`, `hist` and `out` hold width * height
 * slots of 16 B, {r, g, b, w} fp32 (BUFFER_OUT's layout, a denoised image's, and this call's own
 * output); `cur_features` and `hist_features` hold as many rt_pixel_features, taken at params->cur and
 * params->prev.  Pixel p = (x, y) is record y * width + x; out.w carries the pixel's sample count.
 * `hist` and `hist_features` are both NULL (no history yet) or both buffers.  The blend runs on the
 * stored, gamma-encoded values -- the space the denoiser filters in.
 * The operation is one definition in every math mode of `k`; every operation below is one correctly
 * rounded fp32 operation, nothing is contracted, denormals are kept, and comparisons are ordinary IEEE
 * comparisons (false for a NaN).  W = width, H = height.
 *   helpers     dot3(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z
 *               cross(a, b) = (a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x)
 *   constants   computed on the host in fp32: A = 0x1.a82408p-2f (the fp32 nearest to tan of the fp32
 *               0.5f * (45.0f * 3.1415f / 180.0f), kernel_bvh.cl:392); invW = 1.0f / (float)W,
 *               invH = 1.0f / (float)H, asp = (float)W / (float)H, ia = 1.0f / (A * asp), ib = 1.0f / A,
 *               right_c = cross(cur.front, cur.up), right_p = cross(prev.front, prev.up).
 * Per pixel, with c = cur[p] and f = cur_features[p]; every "no history" below writes
 * {c.r, c.g, c.b, cur_frames}:
 *   1 centre    no history if `hist` is NULL or !(f.coverage > 0).
 *   2 point     (the centre ray of CreateRay, the jitter at its mean)
 *               sx = ((2.0f * (((float)x + 0.5f) * invW) - 1.0f) * A) * asp
 *               sy = (2.0f * (((float)y + 0.5f) * invH) - 1.0f) * A
 *               d = (right_c * sx + cur.up * sy) + cur.front, per component
 *               u = d * (1.0f / sqrtf(dot3(d, d)));  X = cur.pos + u * f.depth
 *   3 project   v = X - prev.pos;  zf = dot3(v, prev.front); no history unless zf > 0
 *               a = dot3(v, right_p) / zf, b = dot3(v, prev.up) / zf (IEEE divisions)
 *               fx = ((a * ia + 1.0f) * 0.5f) * (float)W - 0.5f
 *               fy = ((b * ib + 1.0f) * 0.5f) * (float)H - 0.5f
 *               de = sqrtf(dot3(v, v))
 *               (the exact inverse of CreateRay only for a unit front perpendicular to a unit up, as
 *               the reference's cameras are; an approximation for others, and as safe)
 *   4 range     no history unless fx > -1.0f && fx < (float)W && fy > -1.0f && fy < (float)H; only
 *               then x0f = floorf(fx), tx = fx - x0f, x0 = (int)x0f in [-1, W - 1]; likewise y.
 *   5 taps      q = (x0 + i, y0 + j), j outer and i inner, each 0 then 1, with weight
 *               bw = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty).  With
 *               n_q = history_frames != 0 ? history_frames : hist[q].w a tap counts only when q lies
 *               inside the image, hist_features[q].coverage > 0,
 *               fabsf(hist_features[q].depth - de) <= depth_tolerance * de,
 *               dot3(f.normal, hist_features[q].normal) >= normal_threshold, and n_q >= 1.0f.  A tap
 *               that does not count adds nothing and is never multiplied in.  Sums start at +0.0f:
 *               sw += bw; sr += bw * hist[q].r, likewise g and b; sn += bw * n_q.
 *   6 blend     no history unless sw >= 0x1p-6f.  Otherwise h = s_rgb / sw, hn = sn / sw,
 *               n = fminf(hn + cur_frames, max_history), alpha = cur_frames / n,
 *               out.rgb = h + (c - h) * alpha per channel (difference, product, sum), out.w = n.
 * This holds for every input bit pattern, non-finite ones included (IEEE leaves the sign and payload
 * of a NaN result open): no index is formed from a coordinate that was not range-tested first, no
 * float is converted to an integer outside [-1, 2^31), and taps that do not count are dropped by
 * select, never by a multiplication with zero.
 * `cur`, `hist` and both feature buffers are never written (inputs may alias one another), bytes of
 * `out` past width * height * 16 are not touched, and no scene need be bound to `k`.
 * Ordering is rtEnqueueDenoise's: asynchronous on the context's in-order queue, coalesced per-frame
 * launches first, after the pending accumulations; `out` counts as written for the buffers'
 * generations; with timing on the call adds to kernel_ms and counts as one launch.
 * Errors (nothing is launched), checked in this order after the context and the kernel:
 * RT_INVALID_VALUE for params NULL; width or height zero or width * height > 2^31; a camera component
 * that is not finite; cur_frames not finite, < 1 or > 2^20; history_frames negative, not finite, in
 * (0, 1) or > 2^20; max_history not finite, < cur_frames or > 2^20; depth_tolerance not finite or
 * outside [0, 1]; normal_threshold not finite or outside [-1, 1].  RT_INVALID_MEM_OBJECT for exactly
 * one of `hist` and `hist_features` NULL; a required buffer that is NULL or another context's; `out`
 * the same buffer as any input.  RT_INVALID_BUFFER_SIZE for any buffer too small. */
typedef struct rt_view { float pos[3], front[3], up[3]; } rt_view;
typedef struct rt_temporal_params {
    rt_view cur, prev;        /* cameras of `cur`/`cur_features` and of `hist`/`hist_features` */
    float cur_frames;         /* frames averaged in `cur`, >= 1 */
    float history_frames;     /* 0: a history pixel's sample count is its w slot; else this value for every pixel */
    float max_history;        /* cap of the sample count, >= cur_frames */
    float depth_tolerance;    /* relative, 0 .. 1 */
    float normal_threshold;   /* -1 .. 1 */
} rt_temporal_params;
int rtEnqueueTemporalAccumulate(rt_context ctx, rt_kernel k, rt_mem cur, rt_mem cur_features,
                                rt_mem hist /* may be NULL */, rt_mem hist_features /* NULL iff hist is */,
                                unsigned width, unsigned height, const rt_temporal_params* params, rt_mem out);

/* ---- reprojection of the adaptive sample statistics (extension) ---------------------------------
 * rtEnqueueReprojectSamples carries the per-pixel statistics of adaptive sampling across a camera move:
 * for every pixel of the current view it finds, as rtEnqueueTemporalAccumulate does, the point of the
 * previous view that shows the same surface, gathers the statistics of the taps around it that lie on
 * that surface, and recombines them into one rt_pixel_stats -- a mean, a per-sample luminance variance
 * and an integer sample count of at most max_history.  A pixel that finds nothing (a disocclusion, a
 * point outside the previous image, an uncovered pixel) gets 32 zero bytes, rt_pixel_stats' "no
 * samples", which rtEnqueueSelectPixels selects unconditionally; the pixels that keep statistics are
 * selected only where those still say so.  `hist_stats` and `out_stats` hold width * height
 * rt_pixel_stats, `hist_features` and `cur_features` as many rt_pixel_features, taken at params->prev and
 * params->cur.  Pixel p = (x, y) is record y * width + x.
 * The operation is one definition in every math mode of `k`; every operation below is one correctly
 * rounded fp32 operation, nothing is contracted, denormals are kept, `/` and sqrtf are IEEE, and
 * comparisons are IEEE comparisons (false for a NaN).  Helpers, constants, W and H are
 * rtEnqueueTemporalAccumulate's.  Per pixel, with f = cur_features[p]; every "nothing carried" below
 * writes 32 zero bytes:
 *   1 centre    nothing carried unless f.coverage > 0.
 *   2 point, 3 project, 4 range
 *               steps 2 to 4 of rtEnqueueTemporalAccumulate as they stand there, with "nothing carried"
 *               for "no history": they give x0, y0, tx, ty and de.
 *   5 taps      q = (x0 + i, y0 + j), j outer and i inner, each 0 then 1, with weight
 *               bw = (i ? tx : 1.0f - tx) * (j ? ty : 1.0f - ty).  With s = hist_stats[q] and
 *               g = hist_features[q] a tap counts only when q lies inside the image, g.coverage > 0,
 *               fabsf(g.depth - de) <= depth_tolerance * de, dot3(f.normal, g.normal) >= normal_threshold,
 *               and s.n >= 1.0f.  For a tap that counts
 *                 m  = s.sum / s.n                                  per channel, three divisions
 *                 sv = s.n >= 2.0f ? s.m2_y / (s.n - 1.0f) : s.mean_y * s.mean_y
 *               (sv is the per-sample variance of the luminance; a single sample is taken to be as
 *               uncertain as it is bright, rtEnqueueDenoiseSamples' rule stated per sample).  Sums start
 *               at +0.0f: sw += bw; sm += bw * m per channel; sy += bw * s.mean_y; ss += bw * sv;
 *               sn += bw * s.n.  A tap that does not count adds nothing and is never multiplied in.
 *   6 result    nothing carried unless sw >= 0x1p-6f.  Otherwise
 *                 n'         = fminf(floorf(sn / sw), max_history)
 *                 out.sum    = (sm / sw) * n'                       per channel
 *                 out.n      = n'
 *                 out.mean_y = sy / sw
 *                 out.m2_y   = n' >= 2.0f ? (ss / sw) * (n' - 1.0f) : +0.0f
 *               and reserved[2] = 0.  n' is an integer value held as a float, as rt_pixel_stats requires,
 *               and at least 1: every counted s.n is, and rounding is monotone.
 * Behaviour is specified for every bit pattern of the depths and the coverages, and of the statistics of
 * taps that do not count; the statistics of taps that count are specified for finite, non-negative
 * values only (others may propagate in any way).  No index is formed from a coordinate that was not
 * range-tested first, and no value of `hist_stats` ever takes part in an address.
 * The three inputs are never written and may alias one another; `out_stats` may be none of them; bytes
 * of `out_stats` past width * height * 32 are not touched; no scene need be bound to `k`.
 * Ordering is rtEnqueueDenoise's: asynchronous on the context's in-order queue, coalesced per-frame
 * launches first, after the pending accumulations, "another call touching the context" for the
 * deferral rules; `out_stats` counts as written for the buffers' generations; with timing on the call
 * adds to kernel_ms and counts as one launch.
 * Errors (nothing is launched), checked in this order after the context and the kernel:
 * RT_INVALID_VALUE for params NULL; width or height zero or width * height > 2^31; a camera component
 * that is not finite; max_history not finite, not an integer value, < 1 or > 2^20; depth_tolerance not
 * finite or outside [0, 1]; normal_threshold not finite or outside [-1, 1].  RT_INVALID_MEM_OBJECT for
 * a buffer that is NULL or another context's; `out_stats` the same buffer as any input.
 * RT_INVALID_BUFFER_SIZE for any buffer under 32 B per pixel. */
typedef struct rt_reproject_params {
    rt_view cur, prev;       /* cameras of cur_features / out_stats and of hist_stats / hist_features */
    float max_history;       /* cap of a carried sample count: an integer value in [1, 2^20] */
    float depth_tolerance;   /* relative, 0 .. 1   (rt_temporal_params') */
    float normal_threshold;  /* -1 .. 1            (rt_temporal_params') */
} rt_reproject_params;
int rtEnqueueReprojectSamples(rt_context ctx, rt_kernel k, rt_mem hist_stats, rt_mem hist_features,
                              rt_mem cur_features, unsigned width, unsigned height,
                              const rt_reproject_params* params, rt_mem out_stats);

/* ---- moving geometry: vertex update + device-side BVH refit (extension) ----
 * For a mesh whose triangles move while the tree's shape stays put.  Both enqueue calls are
 * asynchronous on the context's in-order queue and never wait on the host: they launch the
 * coalesced per-frame launches first, run after every render, accumulation and query enqueued so
 * far, and later launches and queries see the new geometry.
 *
 * rtEnqueueUpdateVertices overwrites v1/v2/v3.position.xyz (and, when `normals` is non-NULL,
 * v*.normal.xyz) of triangles [first_tri, first_tri + n_tris) of `tris` from records [0, n_tris)
 * of `positions` / `normals` (rt_tri_points, 48 B; the w slots are ignored).  Indices are the
 * triangle buffer's own (BVH leaf order).  Nothing else in a record is touched.
 *
 * rtRefitBVH recomputes the bounds of the tree bound to k (BUFFER_NODE) from the triangles bound
 * to k (BUFFER_SCENE), writes them into the node buffer's CLLinearBVHNode records and into every
 * derived record k holds, and repacks k's triangle / shading records.  Topology, axis flags, leaf
 * ranges, the records past the tree's end and every non-bounds byte of a node record (the w slots
 * of pmin / pmax included) stay as they are.
 *   Bounds rule: a leaf's box is the fminf / fmaxf fold (from +inf / -inf) over the nine position
 * coordinates of each of its triangles, read from the 256-B records; an interior box is the fminf /
 * fmaxf of its two children's.  So a NaN coordinate is ignored and an infinity kept.  The sign of
 * a zero bound is unspecified: the slab test cannot tell, since 0 * inf is NaN for either sign and
 * every other comparison treats +0 and -0 alike.  rtsRefitBounds (rt_scene.h) is the same rule on
 * host arrays.
 *   Safety: a refit never validates, so it may only follow changes that cannot alter topology or
 * material indices.  Every buffer keeps a second, "structural" generation that every writer but
 * these two calls bumps (rtEnqueueWriteBuffer, rtBuildBVH, rect copies, ray / hit outputs).  When
 * k was never prepared, or the structural generation of its triangle or node buffer is not the one
 * k packed, rtRefitBVH first runs the ordinary host-side preparation of a launch (read-back,
 * rtValidateBVH, packing: RT_INVALID_MEM_OBJECT on a malformed tree), then refits; otherwise
 * nothing leaves the device and the next launch finds k's packed scene current.  Other kernels
 * bound to the same buffers see a changed generation and prepare in full at their next launch.
 * The material buffer is checked and packed when bound and not required (a kernel used for
 * queries only refits without one).
 *   Errors (nothing is launched): scene or node slot unbound RT_INVALID_KERNEL_ARGS; a buffer of
 * another context or NULL (`normals` excepted) RT_INVALID_MEM_OBJECT; `positions` or `normals` the
 * same buffer as `tris` RT_INVALID_MEM_OBJECT; first_tri + n_tris beyond `tris`, or `positions` /
 * `normals` smaller than 48 * n_tris, RT_INVALID_BUFFER_SIZE.  n_tris == 0: RT_SUCCESS, no launch.
 * What was accumulated from the old geometry is the caller's choice: restart it, as after a camera move,
 * or take the "before" vertices with rtEnqueueExtractVertices just ahead of the update and carry the
 * history across with the motion records below (rtEnqueueFrameMotion and the two ...Motion calls). */
typedef struct rt_tri_points { rt_float3 p1, p2, p3; } rt_tri_points; /* 48 B, w ignored */
int rtEnqueueUpdateVertices(rt_context ctx, rt_mem tris, size_t first_tri, size_t n_tris, rt_mem positions,
                            rt_mem normals /* may be NULL */);
int rtRefitBVH(rt_context ctx, rt_kernel k);
/* counts since kernel creation: full host-side scene preparations, device refits */
int rtDiagScenePrepares(rt_kernel k, uint64_t* full, uint64_t* refits);

/* ---- motion records: where a surface point was at the previous time (extension) ----------------
 * The two reprojections above know the camera's motion only.  A motion record says, per hit or per
 * pixel, where the surface point that is seen now was before the geometry moved, so that they can
 * follow it (rtEnqueueTemporalAccumulateMotion, rtEnqueueReprojectSamplesMotion).
 *
 * rtEnqueueExtractVertices is the inverse of rtEnqueueUpdateVertices: records [0, n_tris) of `positions`
 * (and, when non-NULL, `normals`) receive v1/v2/v3.position.xyz (.normal.xyz) of triangles
 * [first_tri, first_tri + n_tris) of `tris` as rt_tri_points, the w slots written as 0.  `tris` is only
 * read.  Ordering is rtEnqueueUpdateVertices': asynchronous on the context's in-order queue, coalesced
 * per-frame launches first, never waiting on the host -- a caller takes the "before" snapshot on the
 * device, just ahead of the update.  Errors (nothing is launched), rtEnqueueUpdateVertices' in its order:
 * a buffer of another context or NULL (`normals` excepted), or an output that is `tris`, or `positions`
 * and `normals` one buffer, RT_INVALID_MEM_OBJECT; first_tri + n_tris beyond `tris`, or an output
 * smaller than 48 * n_tris, RT_INVALID_BUFFER_SIZE.  n_tris == 0: RT_SUCCESS, no launch.
 *
 * rtEnqueueHitMotion: hits in, previous surface points out, in the mould of rtEnqueueHitSurfaces.  For
 * records [first, first + n) of `hits` (rt_ray_hit, as a query wrote them; the rays are not needed) it
 * writes the same slots of `motion` (rt_pixel_motion).  `prev_positions` (and `prev_normals`) hold the
 * vertices of triangles [first_tri, first_tri + n_tris) at the previous time, as rtEnqueueExtractVertices
 * wrote them; every other triangle, and every normal when `prev_normals` is NULL, is where the scene
 * bound to k has it now.  The definition is the same in every math mode of k; every operation is one
 * correctly rounded fp32 operation, nothing is contracted, denormals are kept, `/` and sqrtf are IEEE.
 * Per record h = hits[i], with nTris the scene's triangle count:
 *   miss        (uint32)h.prim >= nTris (one unsigned compare: negative indices too) writes prim = -1 and
 *               every other word 0.
 *   moved       moved = (uint64)h.prim - first_tri < n_tris, unsigned: n_tris == 0 moves nothing.
 *   vertices    P1..P3 = prev_positions[h.prim - first_tri] when moved, else the current
 *               v1/v2/v3.position.xyz of the 256-B record; N1..N3 = prev_normals[h.prim - first_tri] when
 *               moved and prev_normals is non-NULL, else the current v*.normal.xyz.
 *   point       w = (1.0f - h.u) - h.v;  prev_point.c = P1.c * w + (P2.c * h.u + P3.c * h.v)
 *   normal      nn.c = N1.c * w + (N2.c * h.u + N3.c * h.v);  l2 = dot3(nn, nn);
 *               prev_normal = l2 > 0 ? nn * (1.0f / sqrtf(l2)) : 0   (per component; false for a NaN)
 *   record      prim = h.prim, flags = moved ? RT_MOTION_MOVED : 0.
 * u and v may have any bit pattern (IEEE leaves the sign and payload of a NaN result open); nothing read from
 * `hits` but the range-tested prim forms an address.
 * `hits`, the prev_* buffers and the scene are never written; slots of `motion` outside the range are
 * not touched.  Ordering, timing and launch counting are rtEnqueueHitSurfaces' (one launch).
 * Errors (nothing is launched), in this order after the context, the kernel and `hits`:
 * RT_INVALID_VALUE for first + n > 2^31; RT_INVALID_MEM_OBJECT for `motion` NULL, another context's or
 * `hits` itself, prev_positions NULL with n_tris != 0, a given prev_* buffer of another context or the
 * same as `motion`; RT_INVALID_BUFFER_SIZE for a range beyond `hits` or `motion`, or a given prev_*
 * buffer under 48 * n_tris bytes; RT_INVALID_KERNEL_ARGS for an unbound scene or node slot;
 * RT_INVALID_BUFFER_SIZE for first_tri + n_tris beyond the scene's triangle count.  n == 0: RT_SUCCESS.
 *
 * rtEnqueueFrameMotion: for every pixel gid in [0, global_work_size), x = gid % WIDTH, y = gid / WIDTH,
 * the closest hit of the pixel's centre ray followed by rtEnqueueHitMotion's record of it, as one fused
 * launch: no ray and no hit goes through memory.
 *   the ray     one definition in every math mode: origin = k's camera position;
 *               dir = (right * sx + up * sy) + front per component, with sx, sy and
 *               right = cross(front, up) exactly as step 2 of rtEnqueueTemporalAccumulate states them
 *               and its host constants taken from k's WIDTH, HEIGHT and camera slots; not normalised;
 *               tmin = -INFINITY, tmax = 100000.0f.  No operation of it is contracted.
 *   the hit     RT_QUERY_CLOSEST's answer for that rt_ray in k's math mode (InitRay normalises dir
 *               there), its u and v as the query re-evaluates them.  rtKernelForceGlobalScene, the
 *               node-collapse records and the rt_stats counters behave as for a query.
 *   the record  rtEnqueueHitMotion's, for {prim, u, v}.
 * After rtEnqueueUpdateVertices and rtRefitBVH the call sees the moved geometry without a full
 * preparation.  Ordering is rtEnqueueFrameFeatures'; with timing on the call counts as one launch.
 * Errors (nothing is launched), in this order after the context, the kernel and `motion`:
 * RT_INVALID_KERNEL_ARGS for an unbound scene, node, WIDTH, HEIGHT or camera slot, or WIDTH or HEIGHT
 * zero or WIDTH * HEIGHT > 2^31; RT_INVALID_GLOBAL_WORK_SIZE for zero or more than 2^31;
 * RT_INVALID_BUFFER_SIZE for `motion` under 32 B per work item; then rtEnqueueHitMotion's rows for the
 * prev_* arguments; then a query's (RT_INVALID_OPERATION: a leaf of more than 127 triangles). */
#define RT_MOTION_MOVED 1u
typedef struct rt_pixel_motion {
    float prev_point[3];   /* the surface point at the previous time */
    int32_t prim;          /* the triangle that is seen now; -1: none, every other word 0 */
    float prev_normal[3];  /* the unit shading normal there at the previous time, or 0 */
    uint32_t flags;        /* RT_MOTION_MOVED: the triangle is one of [first_tri, first_tri + n_tris) */
} rt_pixel_motion; /* 32 B */
int rtEnqueueExtractVertices(rt_context ctx, rt_mem tris, size_t first_tri, size_t n_tris, rt_mem positions,
                             rt_mem normals /* may be NULL */);
int rtEnqueueHitMotion(rt_context ctx, rt_kernel k, rt_mem hits, size_t first, size_t n,
                       rt_mem prev_positions /* NULL only when n_tris == 0 */, rt_mem prev_normals /* may be NULL */,
                       size_t first_tri, size_t n_tris, rt_mem motion);
int rtEnqueueFrameMotion(rt_context ctx, rt_kernel k, size_t global_work_size,
                         rt_mem prev_positions /* NULL only when n_tris == 0 */, rt_mem prev_normals /* may be NULL */,
                         size_t first_tri, size_t n_tris, rt_mem motion);

/* rtEnqueueTemporalAccumulateMotion and rtEnqueueReprojectSamplesMotion.  With `motion` NULL each is
 * its counterpart above exactly: the same bytes, the same errors.  With `motion`, width * height
 * rt_pixel_motion records of the current view (rtEnqueueFrameMotion's), the definitions change in three
 * places only:
 *   1 centre    additionally "no history" / "nothing carried" when motion[p].prim < 0.
 *   2 point     X = motion[p].prev_point.
 *   5 taps      the centre normal is motion[p].prev_normal, not f.normal.
 * Steps 3, 4 and 6 stand as they are.  f.depth and params->cur no longer enter the arithmetic; both
 * are still validated.  X may have any bit pattern: the range test of step 4 comes before any integer
 * conversion, and a tap's index is formed only after its coordinates were tested against the image.
 * `motion` is never written.  Additional errors, with their rows: RT_INVALID_MEM_OBJECT for a `motion`
 * of another context or the same buffer as the output; RT_INVALID_BUFFER_SIZE for one under 32 B per
 * pixel. */
int rtEnqueueTemporalAccumulateMotion(rt_context ctx, rt_kernel k, rt_mem cur, rt_mem cur_features,
                                      rt_mem hist /* may be NULL */, rt_mem hist_features /* NULL iff hist is */,
                                      rt_mem motion /* may be NULL */, unsigned width, unsigned height,
                                      const rt_temporal_params* params, rt_mem out);
int rtEnqueueReprojectSamplesMotion(rt_context ctx, rt_kernel k, rt_mem hist_stats, rt_mem hist_features,
                                    rt_mem cur_features, rt_mem motion /* may be NULL */, unsigned width,
                                    unsigned height, const rt_reproject_params* params, rt_mem out_stats);

/* Where the scene lives: 1 = staged in LDS (when it fits), 0 = read from HBM/L2. */
int rtKernelGetSceneInLDS(rt_kernel k, int* in_lds);
/* Force the global-memory path even if the scene fits in LDS (testing). */
int rtKernelForceGlobalScene(rt_kernel k, int force);

/* Device-to-device copy of [offset, offset+size) of `src` to a device address (e.g. a
 * collective's staging tensor), asynchronous on the context's stream. */
int rtEnqueueCopyBufferToPointer(rt_context ctx, rt_mem src, size_t offset, size_t size, void* dst_device);

/* Device address of a buffer and the context's HIP stream (for collectives/interop).  The
 * stream is returned after pending fused-frame accumulations have been ordered into it; work
 * enqueued on it directly after a later rtEnqueueKernelFrames must call this again first. */
int rtBufferGetDevicePointer(rt_mem mem, void** dptr);
int rtBufferGetSize(rt_mem mem, size_t* size);
int rtContextGetStream(rt_context ctx, void** hip_stream);
/* Extension (multi-GPU gather): with `enable`, rtEnqueueCopyBufferRectToPointer runs on the
 * context's accumulation stream, right after the fused-frame accumulations enqueued so far
 * and before later ones, instead of joining them into the main stream -- so the next fused
 * render is not held up by the read-back.  Work that consumes the copied bytes waits on the
 * stream rtContextGetAccumStream returns (e.g. an event recorded there after the copies);
 * later calls on the context stay ordered after the copies as before. */
int rtContextSetReadbackOnAccumStream(rt_context ctx, int enable);
int rtContextGetAccumStream(rt_context ctx, void** hip_stream);
int rtContextGetDevice(rt_context ctx, int* device_index);

/* Host-only check (no GPU) of a flattened BVH against the contract KernelEntry relies on
 * (CLBVHnode.cpp:161-183).  The tree is the prefix [0, end) of the n_nodes records, `end` = one
 * past the leaf that node 0's chain of second children reaches (depth-first layout); records
 * past it are never read (by the reference's walk from node 0 either), so a node buffer may be
 * larger than its tree -- e.g. rtBuildBVH's buffer of 2n-1 records holding `count`.  Within the
 * tree: interior node i has children i+1 and offset > i+1, both < end, axis <= 2; leaves
 * [offset, offset + nPrimitives) lie within the n_tris triangles; every node but the root has
 * exactly one parent (one tree, every node reachable).  Every launch runs it on the bound
 * arrays first (RT_INVALID_MEM_OBJECT, never a GPU walk).  *depth = the deepest leaf's depth. */
int rtValidateBVH(const void* nodes, size_t n_nodes, size_t n_tris, int* depth);

/* Scheduling parameters of the persistent schedules (extension; no effect on results, only on
 * speed -- every value renders the same bits).  Defaults were swept on MI355X
 * (profiles/r01/ *_sweep*.txt); these calls exist for re-tuning, replacing environment reads so
 * that library behaviour does not depend on the caller's environment.  Out-of-range values ->
 * RT_INVALID_VALUE.
 *   REFILL_MIN / SHADE_MIN            step schedule, LDS scenes: finish + refill when this many
 *                                     lanes are free (1-64, default 6); shade when this many are
 *                                     ready (1-64, default 48)
 *   REFILL_MIN_GLOBAL / SHADE_MIN_GLOBAL  the same for scenes read from HBM/L2 (0-64; default 0 =
 *                                     auto: 32 / 48 walking octant records, 8 / 48 the 64-B records)
 *   STEP_WEIGHT_NODE / STEP_WEIGHT_LEAF   relative cost of a node / triangle step (35 / 55)
 *   STEP_WEIGHT_NODE_GLOBAL / STEP_WEIGHT_LEAF_GLOBAL  the same for scenes read from HBM/L2 (0 =
 *                                     auto: 65 / 55 walking octant records, else the LDS weights)
 *   CHUNK_PIXELS / TAIL_CHUNK         pixels per work-counter fetch, multiples of 64: bulk chunk
 *                                     (0 = auto: 512, 1024 in the pixel-major order) / largest tail
 *                                     chunk (256; a launch uses the largest
 *                                     power-of-two multiple of 64 up to it that gives every
 *                                     wave >= 2.5 tail chunks)
 *   BULK_PERCENT                      share of the work handed out in bulk chunks (80)
 *   TOP_NODES                         global path: top-of-tree nodes staged in LDS (0-1024, 384)
 *   TILE_MAJOR                        fused work order: -1 auto (default: scenes in HBM/L2 pixel-major
 *                                     for 2, 4 or 8 frames, else tile-major for large launches and
 *                                     frame-major for small ones; LDS scenes frame-major),
 *                                     0 frame-major, 1 tile-major (a tile's frames back to back),
 *                                     2 pixel-major (a pixel's frames side by side in a wave; 2, 4 or 8
 *                                     frames on scenes in HBM/L2, otherwise tile-major)
 *   PERFRAME_SKY                      per-frame sky shortcut: 0 off, 1 large launches (default),
 *                                     2 always
 *   WF_REFILL_MIN                     wavefront extend: take queued rays once this many lanes
 *                                     are free (1-64, default 32)
 *   WF_STREAMS_PER_CU                 wavefront queues: streams per compute unit (0-64; default 0 =
 *                                     the shade workgroups one CU holds at once)
 *   WF_TOP_NODES                      wavefront extend, global path: top-of-tree nodes staged in
 *                                     LDS (0-1024, default 256)
 *   GLOBAL_OCT                        step schedule, scenes not in LDS: 1 (default) = walk the
 *                                     octant-resolved node records (32 B per node and octant) in
 *                                     HBM/L2, 0 = the 64-B node records with the top of the tree
 *                                     in LDS
 *   PERFRAME_DEFER                    step schedule, rtEnqueueKernel: 1 = render into a radiance slot
 *                                     and accumulate in a second launch (as a fused launch of one
 *                                     frame), so frames queued back to back overlap (4K Cornell
 *                                     1.11 -> 0.92 ms/frame); 0 = accumulate inside the render
 *                                     (faster when the host synchronises every frame, as the
 *                                     reference's RenderFrame does, and for small frames);
 *                                     2 (default) = defer a launch of at least PERFRAME_DEFER_MIN
 *                                     work items when the host has not waited on the context
 *                                     through this API (rtFinish, a blocking read or write) since
 *                                     the kernel's previous per-frame launch -- i.e. frames are
 *                                     being queued -- and no stream or device pointer of the
 *                                     context has been handed out (rtContextGetStream,
 *                                     rtContextGetAccumStream, rtBufferGetDevicePointer: the host
 *                                     may then synchronise outside the library, which this rule
 *                                     cannot see; such a host's frames launch on the main stream,
 *                                     at once -- see PERFRAME_BATCH).  Results never change.
 *   PERFRAME_DEFER_MIN                work items from which PERFRAME_DEFER 2 defers (default 4 Mi)
 *   MAX_BLOCKS                        persistent schedules: workgroups per CU of the grid (0 =
 *                                     as many as fit, default; fewer = fewer waves per SIMD)
 *   PERFRAME_BATCH                    step schedule: rtEnqueueKernel calls of this kernel queued
 *                                     back to back with consecutive frameCount and otherwise equal
 *                                     arguments (FRAME_SEED aside: KernelEntry never reads it) are
 *                                     coalesced into one fused launch of up to this many frames
 *                                     (1..8, default 8; 1 = every call launches).  The launch is
 *                                     made before any other call touches the context -- a read, a
 *                                     write, rtFinish, another launch, a kernel setting, a release
 *                                     -- so results are the same bits at every point the host can
 *                                     observe; kernels with stats or timing on are not coalesced.
 *                                     An error of a coalesced launch is returned by the next call
 *                                     on the context that returns one (rtFinish at the latest; a
 *                                     frame enqueued over such an error is not queued).  Once the
 *                                     context's stream (rtContextGetStream, rtContextGetAccumStream)
 *                                     or a device pointer of one of its buffers
 *                                     (rtBufferGetDevicePointer) has been handed out, the host may
 *                                     synchronise outside the library, so from then on every
 *                                     rtEnqueueKernel launches at once.
 *   QUERY_REFILL_MIN                  ray queries (rtEnqueueIntersectRays): take rays from the ring
 *                                     once this many lanes are free (1-64, default 32)
 *   TRACE_REFILL_MIN, TRACE_SHADE_MIN path tracing over caller rays (rtEnqueueTracePaths): take records
 *                                     from the ring once this many lanes are free (1-64, default
 *                                     8), and shade once this many walks have ended
 *                                     (1-64, default 48, the step schedule's)
 *   PATH_KILL                         step schedule: 1 (default) = a launch whose scene and arguments
 *                                     pass the path-kill certificate ends a path once its throughput
 *                                     is exactly zero (rtKernelGetPathKill); 0 = every segment is
 *                                     walked.  Results never change. */
enum rt_tuning {
    RT_TUNE_REFILL_MIN = 0,
    RT_TUNE_SHADE_MIN = 1,
    RT_TUNE_REFILL_MIN_GLOBAL = 2,
    RT_TUNE_SHADE_MIN_GLOBAL = 3,
    RT_TUNE_STEP_WEIGHT_NODE = 4,
    RT_TUNE_STEP_WEIGHT_LEAF = 5,
    RT_TUNE_CHUNK_PIXELS = 6,
    RT_TUNE_TAIL_CHUNK = 7,
    RT_TUNE_BULK_PERCENT = 8,
    RT_TUNE_TOP_NODES = 9,
    /* 10-12: the retired pool schedule's thresholds (RT_INVALID_VALUE) */
    RT_TUNE_TILE_MAJOR = 13,
    RT_TUNE_PERFRAME_SKY = 14,
    RT_TUNE_WF_REFILL_MIN = 15,
    RT_TUNE_WF_STREAMS_PER_CU = 16,
    RT_TUNE_WF_TOP_NODES = 17,
    RT_TUNE_GLOBAL_OCT = 18,
    RT_TUNE_PERFRAME_DEFER = 19,
    RT_TUNE_MAX_BLOCKS = 20,
    RT_TUNE_PERFRAME_DEFER_MIN = 21,
    /* 22: the retired speculative walk's switch (RT_INVALID_VALUE) */
    RT_TUNE_PERFRAME_BATCH = 23,
    RT_TUNE_STEP_WEIGHT_NODE_GLOBAL = 24,
    RT_TUNE_STEP_WEIGHT_LEAF_GLOBAL = 25,
    RT_TUNE_QUERY_REFILL_MIN = 26,
    /* 27: never assigned (RT_INVALID_VALUE) */
    RT_TUNE_TRACE_REFILL_MIN = 28,
    RT_TUNE_TRACE_SHADE_MIN = 29,
    RT_TUNE_PATH_KILL = 30
};
int rtKernelSetTuning(rt_kernel k, int param, int value);
int rtKernelGetTuning(rt_kernel k, int param, int* value);

/* Fused frames' accumulation on the context's second stream, overlapping the next render
 * (default 1), or on the main stream (0).  Synchronises the context. */
int rtContextSetAccumOverlap(rt_context ctx, int enable);

/* ---- multi-GPU: band sharding + RCCL gather (extension) -----------------------
 * The reference renders on one OpenCL device (CLRaytracer.cpp:104-120, CLutils.cpp:29).  Pixels
 * are independent -- the seed depends only on the global work-item id and frameCount
 * (kernel_bvh.cl:445) and the accumulation is per pixel (:449-455) -- so a frame shards by
 * interleaved 8-row bands (band b -> rank b % nranks; rtCommShardKernel) rendered at their
 * global positions, with one exchange at the end: the bands are gathered to a root rank (copy
 * engines over xGMI, or RCCL; rtCommSetTransport), byte-identical to a one-GPU render.
 *
 * Communicators: one rank per GPU, either one process per GPU (rtCommGetUniqueId on one rank,
 * the 128-byte id passed to the others by any host means, rtCommInitRank everywhere) or one
 * process driving several GPUs, one context each (rtCommInitAll = ncclCommInitAll). */
typedef struct rt_comm_s* rt_comm;
#define RT_COMM_ID_BYTES 128
int rtCommGetUniqueId(void* id /* RT_COMM_ID_BYTES */);
int rtCommInitRank(rt_context ctx, int nranks, const void* id, int rank, rt_comm* out);
int rtCommInitAll(const rt_context* ctxs, int n, rt_comm* comms_out);
/* A world of n ranks inside this process WITHOUT RCCL: the same sharding and copy-engine gather as
 * above, the ranks linked by address.  The contexts may share one device (several ranks on one
 * GPU), so the N > 1 gather runs where there is only one GPU.  Every gather and reduction must
 * pass all n communicators (n_local == n); n <= 64. */
int rtCommInitLoopback(const rt_context* ctxs, int n, rt_comm* comms_out);
/* A world of processes on one node WITHOUT RCCL -- e.g. several ranks sharing one GPU, which RCCL
 * refuses: rank `rank` of `nranks`, one process each, meeting through files in the directory `dir`
 * (the same for every rank, empty, on a file system they share; rank 0 writes the world's id into
 * it -- a directory holding an earlier world's is refused, RT_INVALID_VALUE -- and the others wait
 * up to a minute for it, so exchange files an earlier world left are never read; the caller
 * removes the directory after rtCommDestroy).  Setup
 * exchanges, rtCommAllReduceF64 and rtCommBarrier go through the files (each waits at most a
 * minute for the slowest rank); the gathers run on the copy engines over IPC mappings exactly as
 * in an RCCL world (RT_COMM_TRANSPORT_RCCL is refused).  It ships because it is the only way to
 * run the one-process-per-GPU gather (IPC handles, the trial round, flags written into another
 * process's memory) on a machine with one GPU: bench.py --shared-world and the GPU tests use it. */
int rtCommInitShared(rt_context ctx, int nranks, int rank, const char* dir, rt_comm* out);
int rtCommDestroy(rt_comm comm);
int rtCommGetRank(rt_comm comm, int* rank, int* nranks);
/* The kernel renders this rank's bands: rtKernelSetRowInterleave(k, nranks, rank).  The gather's
 * plan counts bands from image row 0, so a kernel with a work range (rtKernelSetWorkRange) is
 * refused (RT_INVALID_OPERATION), and so is setting one on a kernel sharded this way. */
int rtCommShardKernel(rt_comm comm, rt_kernel k);
/* Gather the band-sharded image: every rank's bands of its `out` buffer (width x height pixels
 * of 16 bytes, rendered after rtCommShardKernel) are assembled in the root's `root_dst` (NULL =
 * the root's own `out`).  `comms`/`outs`: the n_local communicators this host thread drives
 * (1 per process in the one-process-per-GPU setup) and their output buffers.  Asynchronous and
 * pipelined, so neither the next fused render nor the next accumulation waits for a transfer:
 *   copy engines (default transport): each rank's copy engine writes its bands, straight from
 *     its `out` (after the fused-frame accumulations and per-frame launches enqueued so far),
 *     into the rows they occupy in the root's destination -- no staging, no pack or unpack
 *     kernel, no compute unit anywhere in the gather -- and raises an arrival flag in the root's
 *     memory; the root's reads of the image wait for every flag.  The root's own bands are in
 *     place when it gathers into its own `out`; else its copy engine copies them like any rank's.
 *     A rank's copies of gather k start once the root has enqueued gather k and finished the
 *     calls it queued before (reads of image k - 1): the root's image never changes under a read
 *     queued on it.  The destination is part of the plan, with the size and the root: in a world
 *     of one rank per process the root refuses (RT_INVALID_OPERATION) a gather into another
 *     buffer until the plan is rebuilt (a size or root change, or rtCommSetTransport -- collective
 *     steps); a destination released meanwhile stays allocated until then.
 *   RCCL: each rank packs its bands into a staging slot on its accumulation stream, grouped
 *     ncclSend/ncclRecv move the slots to the root on the communicator's stream, and the root
 *     unpacks them on a third stream; two staging slots, so step k's gather overlaps step k+1's
 *     render.
 * The communicator's streams run at the device's greatest stream priority.  Every later call on a
 * context that reads or writes memory (rtFinish, rtEnqueueReadBuffer, per-frame launches, ...) is
 * ordered after its part of the gather. */
int rtCommEnqueueGatherBands(const rt_comm* comms, const rt_mem* outs, int n_local, unsigned width,
                             unsigned height, int root, rt_mem root_dst);
/* How the gather moves the bands (set alike on every rank, before a gather; a change takes effect
 * at the next gather, which rebuilds the plan -- a collective step):
 *   RT_COMM_TRANSPORT_COPY_ENGINES (default): the copy engines (SDMA; over xGMI between GPUs) write
 *     every band into the root's destination -- mapped by IPC handle (exchanged with one
 *     ncclAllGather per plan, then checked with one trial copy and flag round across the world)
 *     or, for ranks driven by one process, by address.  Arrival and release are flags
 *     (hipStreamWriteValue64 / hipStreamWaitValue64) between the processes, events within one.  No
 *     compute unit is used for the transfer, so it runs beside a persistent render.  A world in
 *     which some rank cannot map the root's memory falls back to RCCL transfers for the plan
 *     (rtCommGetStatus reports it).
 *   RT_COMM_TRANSPORT_RCCL: grouped ncclSend/ncclRecv on the communicator stream (the root's own
 *     bands too: a device-local send), i.e. RCCL's transfer kernel, with the pack and unpack copies.
 *   RT_COMM_TRANSPORT_COPY_ENGINES_IPC: the copy engines with the links always set up the
 *     multi-process way (IPC handles through ncclAllGather, a world-wide ncclAllReduce on the
 *     outcome) even when every rank is driven by this process -- the one-process-per-GPU path,
 *     selectable at any world size (one local communicator per call).
 * Loopback worlds always use the copy engines. */
#define RT_COMM_TRANSPORT_COPY_ENGINES 0
#define RT_COMM_TRANSPORT_RCCL 1
#define RT_COMM_TRANSPORT_COPY_ENGINES_IPC 2
int rtCommSetTransport(rt_comm comm, int transport);
/* *transport: the requested one; *active: the one the current plan runs (-1: no plan yet). */
int rtCommGetTransport(rt_comm comm, int* transport, int* active);
/* What the communicator's current plan does (self-description for benchmarks and logs). */
#define RT_COMM_FALLBACK_NONE 0
#define RT_COMM_FALLBACK_NO_PEER_ACCESS 1  /* one process, several GPUs: no peer access */
#define RT_COMM_FALLBACK_IPC_MAP 2         /* some rank could not export or map an IPC handle */
#define RT_COMM_FALLBACK_HANDSHAKE 3       /* the trial copy / flag round failed or timed out */
typedef struct rt_comm_status {
    int rank, nranks;
    int transport;         /* requested (rtCommSetTransport) */
    int active;            /* the current plan's transport, -1 before the first gather */
    int fallback;          /* 1: the plan asked for the copy engines and runs RCCL instead */
    int fallback_reason;   /* RT_COMM_FALLBACK_* */
    unsigned copies_per_gather;        /* copy commands this rank issues per gather */
    unsigned long long bytes_per_gather;  /* bytes this rank moves per gather */
    unsigned long long gathers;        /* gathers enqueued with the current plan */
    double last_xfer_ms;   /* the last completed gather's transfer on this rank (its copies, or
                              its RCCL transfer; -1: none measured) */
} rt_comm_status;
int rtCommGetStatus(rt_comm comm, rt_comm_status* out);
/* Test hooks.  RT_COMM_OPT_FAIL_LINKS (value 1): this rank reports its copy-engine links as
 * broken at the next plan's link step, so the world takes the RCCL fallback (what a world whose
 * IPC mappings or trial round fail does). */
#define RT_COMM_OPT_FAIL_LINKS 1
/* RT_COMM_OPT_REPLAN_PERIOD (value 2): gathers per plan before the world re-plans collectively
 * (default 65,534, the flag values a copy-engine plan holds; 1 .. 65,534; every rank of the world
 * must set the same value before its next gather).  RT_COMM_OPT_SYSTEM_ACQUIRE (value 3): the
 * root's first read of a gathered image runs its system-scope acquire (L1 + every XCD's L2) even
 * when every writer is on the root's device -- it always does when another device's copy engines
 * write the image. */
#define RT_COMM_OPT_REPLAN_PERIOD 2
#define RT_COMM_OPT_SYSTEM_ACQUIRE 3
int rtCommSetOption(rt_comm comm, int option, int value);
/* Blocking reductions of `count` doubles per local rank (values: n_local x count, in place),
 * op RT_COMM_SUM or RT_COMM_MAX; rtCommBarrier = a one-value reduction. */
#define RT_COMM_SUM 0
#define RT_COMM_MAX 1
int rtCommAllReduceF64(const rt_comm* comms, int n_local, double* values, int count, int op);
int rtCommBarrier(const rt_comm* comms, int n_local);

/* The pack plan behind the gather (host-only, no GPU needed): the 2-D copies moving rank
 * `phase`'s bands (period ranks) of a width x height image between the image
 * ([img_offset + i*img_pitch, +width) bytes) and a dense staging buffer
 * ([stage_offset + i*width, +width)); at most 2 rects; *staging_bytes = the per-rank staging
 * size (the largest rank's share). */
typedef struct rt_rect {
    uint64_t img_offset, img_pitch, width, rows, stage_offset;
} rt_rect;
int rtBandPackPlan(unsigned width, unsigned height, unsigned period, unsigned phase, rt_rect* rects,
                   int capacity, int* n_rects, size_t* staging_bytes);

/* The pinned math policy's builtins evaluated on the GPU, element-wise over n host values (for
 * tests: the same device functions the pinned KernelEntry runs).  op: RT_PINNED_OP_*; b is read
 * by the two-operand ops only.  Blocking. */
#define RT_PINNED_OP_RCP 0    /* 1.0f / a  (correctly rounded) */
#define RT_PINNED_OP_DIV 1    /* a / b     (correctly rounded) */
#define RT_PINNED_OP_SQRT 2   /* sqrt(a)   (correctly rounded) */
#define RT_PINNED_OP_RSQRT 3  /* 1.0f / sqrt(a), two rounded operations (normalize's, a >= 2^-126) */
#define RT_PINNED_OP_POW 4    /* pow(a, b) (rt_pinned_math.h pm_pow) */
#define RT_PINNED_OP_SIN 5
#define RT_PINNED_OP_COS 6
int rtDiagPinnedMath(int device_index, int op, const float* a, const float* b, float* out, size_t n);

/* The gamma code's pow for literal exponents and its frame-1 shortcut, checked on the GPU over the operand
 * bit patterns first .. first + count - 1 (count <= 2^32 - first) under one math mode (for tests).
 *   RT_GAMMA_CHECK_POW:   the step kernels' pow for the literal `exponent` (0: 2.2f, 1: 0.454545f,
 *                         2: 0.45454545f) against the mode's plain pow(x, literal), bit for bit;
 *   RT_GAMMA_CHECK_LEMMA: bits(pow(x, 2.2f) * 0.0f) against +0 (`exponent` is not read).
 * *mismatches = patterns that differ, *first_bad = the smallest of them (UINT32_MAX: none),
 * *first_bits = the compared bits (the new pow's / the product's) at `first`.  Blocking. */
#define RT_GAMMA_CHECK_POW 0
#define RT_GAMMA_CHECK_LEMMA 1
int rtDiagGammaPow(int device_index, int math, int check, int exponent, uint32_t first, uint64_t count,
                   uint64_t* mismatches, uint32_t* first_bad, uint32_t* first_bits);

/* Library identification (for smoke checks): returns a static string. */
const char* rtGetBuildInfo(void);

#ifdef __cplusplus
}
#endif

#endif /* RT_HIP_H */

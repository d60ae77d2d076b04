// rt_capi.cpp -- the C ABI of include/rt_hip.h over the HIP runtime.
//
// Objects mirror the reference's OpenCL objects one to one:
//   rt_context = cl::Context + in-order cl::CommandQueue (CLutils.cpp:9-35) -> one HIP
//                device + one non-blocking HIP stream;
//   rt_mem     = cl::Buffer (CLBVHnode.cpp:215-236, CLRaytracer.cpp:132-135) -> hipMalloc
//                allocation (+ a host shadow of what the host last wrote, used to
//                validate scene arrays before any kernel reads them);
//   rt_kernel  = cl::Kernel "KernelEntry" (CLutils.cpp:52-77) -> the argument slots and
//                the derived packed scene the HIP kernels read.
// Safety: the node/triangle/material arrays are validated on the host before the first
// launch that uses them (child indices strictly increasing, leaf ranges inside the
// triangle array, material indices in range, depth <= 64), so a malformed scene is an
// error code, never an out-of-bounds or non-terminating GPU walk.
// That validation and the record packing live in rt_scene_pack.cpp, how a launch hands its work out
// in rt_launch_plan.cpp, and rtKernelSetTuning's knobs in rt_tuning.cpp (all pure host code); the
// packed scene and the rule that keeps it current in rt_device_scene.cpp, the kernel's other device
// resources (timing events, radiance sets, wavefront queues, work counters) in rt_kernel_state.cpp.
// A plan names its kernel by a rtk::Variant, which the launch and the occupancy cache
// (rt_kernels.hpp) both take.  A launch reads its argument slots from a rti::LaunchArgs value
// (rt_launch_args.hpp): rtSetKernelArg alone writes the kernel's, and held-back frames launch with
// their own copy.  This file keeps the objects, the streams and the launches.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <limits>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/rt_cl_types.h"
#include "../../include/rt_hip.h"
#include "rt_adaptive.hpp"
#include "rt_adaptive_plan.hpp"
#include "rt_bvh.hpp"
#include "rt_denoise.hpp"
#include "rt_denoise_plan.hpp"
#include "rt_denoise_samples.hpp"
#include "rt_device_scene.hpp"
#include "rt_internal.hpp"
#include "rt_kernel_state.hpp"
#include "rt_kernels.hpp"
#include "rt_launch_plan.hpp"
#include "rt_motion_launch.hpp"
#include "rt_motion_plan.hpp"
#include "rt_query_plan.hpp"
#include "rt_refit.hpp"
#include "rt_reproject.hpp"
#include "rt_reproject_plan.hpp"
#include "rt_scene_pack.hpp"
#include "rt_temporal.hpp"
#include "rt_temporal_plan.hpp"
#include "rt_trace_plan.hpp"
#include "rt_tuning.hpp"

namespace {

constexpr uint64_t kKnownFlags =
    RT_MEM_READ_WRITE | RT_MEM_WRITE_ONLY | RT_MEM_READ_ONLY | RT_MEM_COPY_HOST_PTR;
#ifndef RT_TIMELINE
#define RT_TIMELINE 0
#endif
// diagnostic timeline builds (-DRT_TIMELINE=1, scripts/timeline.py) write three 64-bin histograms after
// the primary hit ids: such a build requires hit buffers that long
constexpr size_t kHitPad = RT_TIMELINE ? 192 : 0;
// diagnostic count builds (-DRT_NODE_COLLAPSE_STATS=1): stats launches walk the collapsed links too, so
// their node_visits against the default build's is the exact number of visits the collapse removes
// (the other counters stay; such a build's visits are not the reference's).  "The collapsed links" are the
// gate-skipped ones where the scene has them: with -DRT_GATE_SKIP=0, or -DRT_GATE_SELECT=1, the same launch
// counts the collapse alone, or the plain-ratio selection (profiles/r14/removed_visits.txt)
#ifndef RT_NODE_COLLAPSE_STATS
#define RT_NODE_COLLAPSE_STATS 0
#endif
// ... and (-DRT_OCTANT_CULL_STATS=1) the pruned links: node_visits and tri_tests against the default
// build's are the exact lane visits and tests the octant cull removes
#ifndef RT_OCTANT_CULL_STATS
#define RT_OCTANT_CULL_STATS 0
#endif

}  // namespace

using rti::map_hip;
using rti::mark_device_write;
using rti::qs;

struct rt_kernel_s {
    rt_context ctx = nullptr;
    rti::LaunchArgs args;  // the 14 slots, written by rtSetKernelArg alone
    int math = RT_MATH_SHIPPED;  // the reference as its host builds it (rt_hip.h)
    int sched = RT_SCHED_STEP;
    rtp::Tuning tune;  // rtKernelSetTuning's knobs (rt_tuning.hpp)
    uint32_t band_period = 1, band_phase = 0;  // 8-row band interleave (multi-GPU sharding)
    uint64_t range_first = 0, range_last = 0;
    bool comm_sharded = false;  // bands set by rtCommShardKernel: the gather's plan needs the whole frame
    rt_mem hit_ids = nullptr, hit_t = nullptr;
    bool stats = false, timing = false, force_global = false;
    bool shadow_rays = false;  // rtKernelSetShadowRays: read by rtEnqueueTracePaths and rtEnqueueSamplePixels alone
    uint64_t launches = 0;
    uint64_t pf_waits = ~0ull;         // ctx->host_waits at the previous per-frame step launch
    bool last_lds = false;
    bool last_kill = false;            // the last render launch carried the path kill (rtKernelGetPathKill)
    bool last_collapsed = false;       // the last launch walked the collapsed links (rtKernelGetNodeCollapse)
    bool last_pruned = false;          // ... the pruned links, which contain them (rtKernelGetOctantCull)
    // the device resources, each with its own invariant (rt_device_scene.hpp, rt_kernel_state.hpp,
    // rt_internal.hpp, rt_kernels.hpp)
    rti::DeviceScene scene;  // the derived packed scene
    rti::LaunchTimer timer;  // rtKernelSetTiming's event brackets
    rti::RadianceSets rad;  // fused frames: radiance per (frame slot, work-item)
    rti::WavefrontQueues wfq;  // wavefront schedule: ray queues
    rti::WorkCounters counters;  // chunk counters, sky keys, rt_stats words
    rti::FeatureScratch feat;  // rtEnqueueFrameFeatures: a frame's camera rays and hits
    rti::DenoiseScratch denoise;  // rtEnqueueDenoise, rtEnqueueDenoiseSamples: the ping-pong image
    rti::AdaptiveScratch adaptive;  // rtEnqueueSelectPixels: flag planes and block counts
    rtk::OccupancyCache occ;  // workgroups per CU of the kernels launched so far

    // (the caller has drained the context's streams, or nothing was ever launched)
    void release_parts() {
        timer.release();
        rad.release();
        wfq.release();
        counters.release();
        scene.release();
        feat.release();
        denoise.release();
        adaptive.release();
    }
};

namespace {

using rti::LaunchArgs;
using rti::LaunchTimer;

int ensure_device(rt_context ctx) {
    if (!ctx) return RT_INVALID_CONTEXT;
    return map_hip(hipSetDevice(ctx->device));
}

// an error of an earlier coalesced launch (rti::flush_frames), else rc
int pending_error(rt_context ctx, int rc) {
    if (ctx && ctx->pend_error != RT_SUCCESS) {
        const int e = ctx->pend_error;
        ctx->pend_error = RT_SUCCESS;
        return e;
    }
    return rc;
}

// the context's coalesced frames, when they are `k`'s (a setting of k is about to change how
// they would launch)
void flush_kernel(rt_kernel k) {
    if (k && k->ctx && k->ctx->held.k == k) (void)rti::flush_frames(k->ctx);
}

// another call touches the context: its coalesced frames launch first, and an error of theirs is
// that call's status
int flush_first(rt_context ctx) {
    const int rc = rti::flush_frames(ctx);
    return rc ? pending_error(ctx, rc) : RT_SUCCESS;
}

// k's packed scene is that of the buffers bound in `a` (a malformed scene is refused here, before any
// launch)
int prepare_scene(rt_kernel k, const LaunchArgs& a) { return k->scene.prepare(k->ctx, a.tris(), a.nodes(), a.materials()); }

// a render launch's arguments: every slot set, the work size, the image size, the output and hit
// buffers (what enqueue checks first, and rtEnqueueKernel before it holds a frame back)
int check_launch_args(rt_kernel k, const LaunchArgs& a, size_t global_work_size) {
    if (!a.complete()) return RT_INVALID_KERNEL_ARGS;
    if (global_work_size == 0 || global_work_size > 0xffffffffull) return RT_INVALID_GLOBAL_WORK_SIZE;
    if (a.width() == 0 || a.height() == 0) return RT_INVALID_KERNEL_ARGS;
    if (a.out()->size < global_work_size * 16) return RT_INVALID_GLOBAL_WORK_SIZE;
    if (k->hit_ids && (k->hit_ids->size < (global_work_size + kHitPad) * 4 || k->hit_t->size < global_work_size * 4))
        return RT_INVALID_MEM_OBJECT;
    return RT_SUCCESS;
}

// the image size, the frame and the camera slots
void fill_camera(const LaunchArgs& la, uint32_t frame, rtk::KernelArgs* a) {
    a->width = la.width(), a->height = la.height(), a->frameCount = frame;
    for (int i = 0; i < 3; ++i) {
        a->camPos[i] = la.f3[0][i];
        a->camFront[i] = la.f3[1][i];
        a->camUp[i] = la.f3[2][i];
    }
}

// The shared head of the calls that launch on the context's queue for a kernel: the device, the
// kernel handle, the buffers that must be the context's, then the coalesced frames.
int queue_head(rt_context ctx, rt_kernel k, std::initializer_list<rt_mem> mems) {
    const int rc = ensure_device(ctx);
    if (rc) return rc;
    if (!k || k->ctx != ctx) return RT_INVALID_KERNEL;
    for (rt_mem m : mems)
        if (!m || m->ctx != ctx) return RT_INVALID_MEM_OBJECT;
    return flush_first(ctx);
}

// The shared tail of the auxiliary enqueues.  `launch(st)` issues the call's launch or launches on
// the context's stream, after the pending accumulations and gathers and inside the kernel's timing
// bracket; `written` then counts as written by the device and the call as one launch.
template <class Launch>
int launch_on_queue(rt_context ctx, rt_kernel k, rt_mem written, Launch&& launch) {
    hipStream_t st = qs(ctx);
    LaunchTimer::Bracket timed = k->timer.bracket(k->timing, st, LaunchTimer::kRender);
    if (!timed.begin()) return RT_OUT_OF_RESOURCES;
    const hipError_t e = launch(st);
    if (e != hipSuccess) return map_hip(e);
    timed.end();
    mark_device_write(written, true);
    const int rc = k->timer.drain_if_many();
    if (rc) return rc;
    ++k->launches;
    return pending_error(ctx, RT_SUCCESS);
}

// the cameras of the two reprojection calls
rtp::TemporalView view_of(const rt_view& v) {
    rtp::TemporalView o;
    for (int c = 0; c < 3; ++c) o.pos[c] = v.pos[c], o.front[c] = v.front[c], o.up[c] = v.up[c];
    return o;
}

// The frame of the two a-trous denoise calls once their plan `p` stands: the scratch, before anything is
// enqueued (growing it waits for nothing: rt_internal.hpp), then one launch per iteration, in order on the
// context's stream after the pending accumulations and gathers, until one fails.  `step(i, t, src, dst, st)`
// launches iteration i from and into the buffers its DenoiseStep `t` names (`image` is the first one's
// source slot).
template <class Plan, class Step>
int enqueue_atrous(rt_context ctx, rt_kernel k, const Plan& p, float4* image, rt_mem out, Step&& step) {
    if (p.scratch_pixels) {
        const hipError_t me = k->denoise.reserve((size_t)p.scratch_pixels);
        if (me != hipSuccess) return map_hip(me);
    }
    float4* const bufs[3] = {image, static_cast<float4*>(out->dptr), k->denoise.image()};
    return launch_on_queue(ctx, k, out, [&](hipStream_t st) {
        hipError_t e = hipSuccess;
        for (unsigned i = 0; i < p.iterations && e == hipSuccess; ++i) {
            const rtp::DenoiseStep& t = p.it[i];
            e = step(i, t, bufs[t.src], bufs[t.dst], st);
        }
        return e;
    });
}

}  // namespace

extern "C" {

int rtCreateContext(int device_index, rt_context* out) {
    if (!out) return RT_INVALID_VALUE;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return RT_DEVICE_NOT_FOUND;
    if (device_index < 0 || device_index >= n) return RT_INVALID_DEVICE;
    hipError_t e = hipSetDevice(device_index);
    if (e != hipSuccess) return map_hip(e);
    rt_context c = new (std::nothrow) rt_context_s();
    if (!c) return RT_OUT_OF_HOST_MEMORY;
    c->device = device_index;
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->astream, hipStreamNonBlocking);
    for (hipStream_t& r : c->rstream)
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&r, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->atail, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->mtail, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->gtail, hipEventDisableTiming);
    if (e != hipSuccess) {
        if (c->stream) (void)hipStreamDestroy(c->stream);
        if (c->astream) (void)hipStreamDestroy(c->astream);
        for (hipStream_t r : c->rstream)
            if (r) (void)hipStreamDestroy(r);
        delete c;
        return RT_INVALID_COMMAND_QUEUE;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_index) == hipSuccess) {
        c->num_cus = prop.multiProcessorCount;
        // MI300-class parts: 8 XCDs, CU-mask bits interleaved across them
        // (scripts/probes/cu_mask_probe.hip, profiles/r04/cu_mask_probe.txt)
        if ((std::strncmp(prop.gcnArchName, "gfx94", 5) == 0 || std::strncmp(prop.gcnArchName, "gfx95", 5) == 0) &&
            c->num_cus % 8 == 0)
            c->n_xcd = 8;
    }
    if (c->num_cus <= 0) c->num_cus = 256;
    *out = c;
    return RT_SUCCESS;
}

int rtReleaseContext(rt_context ctx) {
    int rc = ensure_device(ctx);
    if (rc) return rc;
    (void)hipStreamSynchronize(qs(ctx));
    (void)hipStreamSynchronize(ctx->astream);
    (void)hipStreamDestroy(ctx->stream);
    (void)hipStreamDestroy(ctx->astream);
    for (hipStream_t r : ctx->rstream) {
        (void)hipStreamSynchronize(r);
        (void)hipStreamDestroy(r);
    }
    (void)hipEventDestroy(ctx->atail);
    (void)hipEventDestroy(ctx->mtail);
    (void)hipEventDestroy(ctx->gtail);
    delete ctx;
    return RT_SUCCESS;
}

int rtCreateBuffer(rt_context ctx, uint64_t flags, size_t size, const void* host_ptr, rt_mem* out) {
    if (!out) return RT_INVALID_VALUE;
    *out = nullptr;
    int rc = ensure_device(ctx);
    if (rc) return rc;
    if (flags & ~kKnownFlags) return RT_INVALID_VALUE;
    if (size == 0) return RT_INVALID_BUFFER_SIZE;
    const bool copy = (flags & RT_MEM_COPY_HOST_PTR) != 0;
    if (copy != (host_ptr != nullptr)) return RT_INVALID_HOST_PTR;
    rt_mem m = new (std::nothrow) rt_mem_s();
    if (!m) return RT_OUT_OF_HOST_MEMORY;
    m->ctx = ctx;
    m->size = size;
    m->flags = flags;
    hipError_t e = hipMalloc(&m->dptr, size);
    if (e != hipSuccess) {
        delete m;
        return map_hip(e);
    }
    if (copy) {
        try {
            m->shadow.assign(static_cast<const uint8_t*>(host_ptr),
                             static_cast<const uint8_t*>(host_ptr) + size);
        } catch (const std::bad_alloc&) {
            (void)hipFree(m->dptr);
            delete m;
            return RT_OUT_OF_HOST_MEMORY;
        }
        m->shadow_valid = true;
        e = hipMemcpyAsync(m->dptr, host_ptr, size, hipMemcpyHostToDevice, qs(ctx));
    } else {
        e = hipMemsetAsync(m->dptr, 0, size, qs(ctx));
    }
    if (e == hipSuccess) e = hipStreamSynchronize(qs(ctx));
    if (e != hipSuccess) {
        (void)hipFree(m->dptr);
        delete m;
        return map_hip(e);
    }
    *out = m;
    return RT_SUCCESS;
}

int rtReleaseBuffer(rt_mem m) {
    if (!m || m->released) return RT_INVALID_MEM_OBJECT;
    int rc = ensure_device(m->ctx);
    if (rc) return rc;
    (void)hipStreamSynchronize(qs(m->ctx));
    if (m->pins > 0) {  // a gather plan still writes into it: freed when the plan lets go
        m->released = true;
        return RT_SUCCESS;
    }
    (void)hipFree(m->dptr);
    delete m;
    return RT_SUCCESS;
}

int rtCreateKernel(rt_context ctx, const char* name, rt_kernel* out) {
    if (!out) return RT_INVALID_VALUE;
    *out = nullptr;
    int rc = ensure_device(ctx);
    if (rc) return rc;
    if (!name || std::strcmp(name, "KernelEntry") != 0) return RT_INVALID_KERNEL_NAME;
    rt_kernel k = new (std::nothrow) rt_kernel_s();
    if (!k) return RT_OUT_OF_HOST_MEMORY;
    k->ctx = ctx;
    const hipError_t e = k->counters.create(qs(ctx));
    if (e != hipSuccess) {
        k->release_parts();
        delete k;
        return map_hip(e);
    }
    *out = k;
    return RT_SUCCESS;
}

int rtReleaseKernel(rt_kernel k) {
    if (!k) return RT_INVALID_KERNEL;
    int rc = ensure_device(k->ctx);
    if (rc) return rc;
    flush_kernel(k);
    (void)hipStreamSynchronize(qs(k->ctx));
    (void)hipStreamSynchronize(k->ctx->astream);
    k->release_parts();
    delete k;
    return RT_SUCCESS;
}

int rtSetKernelArg(rt_kernel k, unsigned index, size_t size, const void* value) {
    if (!k) return RT_INVALID_KERNEL;
    if (index >= RT_ARG_COUNT) return RT_INVALID_ARG_INDEX;
    if (!value) return RT_INVALID_ARG_VALUE;
    if (index <= RT_ARG_BUFFER_MATERIAL) {
        if (size != sizeof(rt_mem)) return RT_INVALID_ARG_SIZE;
        rt_mem m = *static_cast<const rt_mem*>(value);
        if (!m || m->ctx != k->ctx) return RT_INVALID_MEM_OBJECT;
        k->args.bufs[index] = m;
    } else if (index <= RT_ARG_SKYBOX_INTENSITY) {
        if (size != 4) return RT_INVALID_ARG_SIZE;
        std::memcpy(&k->args.u32[index], value, 4);
    } else {
        if (size != 16) return RT_INVALID_ARG_SIZE;
        std::memcpy(k->args.f3[index - RT_ARG_CAMERA_POS], value, 16);
    }
    k->args.set[index] = true;
    return RT_SUCCESS;
}

// frames first_frame .. first_frame + n_frames - 1 of `k` with the arguments `args` (whose
// FRAME_COUNT slot is not read), as one launch
static int enqueue(rt_context ctx, rt_kernel k, const rti::LaunchArgs& args, size_t global_work_size,
                   uint32_t first_frame, uint32_t n_frames);

}  // extern "C"

void rti::unpin(rt_mem m) {
    if (--m->pins > 0 || !m->released) return;
    (void)hipFree(m->dptr);  // (the plan has synchronised the streams that wrote it)
    delete m;
}

int rti::flush_frames(rt_context ctx) {
    if (!ctx || !ctx->held.k) return RT_SUCCESS;
    // taken out first: enqueue's own qs() calls find nothing held.  The frames launch with the
    // arguments they were enqueued with, whatever the kernel's slots hold by now
    const HeldFrames h = ctx->held.take();
    const int rc = enqueue(ctx, h.k, h.args, h.gws, h.f0, h.n);
    if (rc != RT_SUCCESS && ctx->pend_error == RT_SUCCESS) ctx->pend_error = rc;
    return rc;
}

extern "C" {

// Frame coalescing (RT_TUNE_PERFRAME_BATCH).  The reference's host issues one ExecuteKernel per
// frame (CLRaytracer.cpp:52-55); a host that queues frames without looking at them in between
// gets them as fused launches (rtEnqueueKernelFrames: bit-identical to the per-frame launches,
// test_fused_frames.py), one launch tail per run instead of one per frame.  The frame is checked
// here as a launch would check it, so argument and scene errors still come back from this call.
int rtEnqueueKernel(rt_context ctx, rt_kernel k, size_t global_work_size) {
    // (not once a stream or a device pointer of the context has been handed out: the host may then
    // synchronise behind the library's back, e.g. hipStreamSynchronize on the exposed stream, and
    // must find every frame it enqueued launched)
    const bool coalesce = ctx && k && k->ctx == ctx && k->tune.pf_batch > 1 && k->sched == RT_SCHED_STEP && !k->stats &&
                          !k->timing && !ctx->mexposed && !ctx->dexposed;
    if (!coalesce) {
        const int rc = flush_first(ctx);
        if (rc) return rc;
        if (!k) {  // (after the context's own check, as enqueue orders them)
            const int dc = ensure_device(ctx);
            return dc ? dc : RT_INVALID_KERNEL;
        }
        return enqueue(ctx, k, k->args, global_work_size, k->args.frame_count(), 1);
    }
    int rc = ensure_device(ctx);
    if (rc) return rc;
    rc = check_launch_args(k, k->args, global_work_size);
    if (rc) return rc;
    const uint32_t f = k->args.frame_count();
    // an error of an earlier held launch is reported now, and this frame is not queued: the
    // caller retrying it starts a fresh run instead of accumulating it twice
    if (ctx->pend_error != RT_SUCCESS) return pending_error(ctx, RT_SUCCESS);
    if (ctx->held.continues(k, global_work_size, k->args, f, k->tune.pf_batch)) {
        ++ctx->held.n;  // the next frame of the run
        return RT_SUCCESS;
    }
    rc = flush_first(ctx);
    if (rc) return rc;
    rc = prepare_scene(k, k->args);  // (a malformed scene is refused now, not at the launch)
    if (rc) return rc;
    ctx->held = rti::HeldFrames{k, global_work_size, f, 1, k->args};
    return pending_error(ctx, RT_SUCCESS);
}

int rtEnqueueKernelFrames(rt_context ctx, rt_kernel k, size_t global_work_size, unsigned n_frames) {
    if (n_frames == 0) return RT_INVALID_VALUE;
    if (const int rc = flush_first(ctx)) return rc;
    if (!k) return RT_INVALID_KERNEL;
    // fused launches of at most kMaxFusedFrames frames each; one launch per frame for a single frame
    // and for the schedules that have no fused form: same results
    const bool fuse = n_frames > 1 && (k->sched == RT_SCHED_STEP || k->sched == RT_SCHED_WAVEFRONT);
    const uint32_t f0 = k->args.frame_count();
    int rc = RT_SUCCESS;
    for (unsigned done = 0; done < n_frames && rc == RT_SUCCESS;) {
        const unsigned n = fuse ? std::min<unsigned>(n_frames - done, rtk::kMaxFusedFrames) : 1;
        rc = enqueue(ctx, k, k->args, global_work_size, f0 + done, n);
        done += n;
    }
    return rc;
}

// ---- enqueue's steps: the resources, streams and launches of one LaunchPlan (rt_launch_plan.hpp) ----

// the plan's inputs: plain values of the launch, the kernel's settings and its packed scene
static rtp::PlanIn plan_inputs(rt_context ctx, rt_kernel k, const LaunchArgs& la, size_t global_work_size,
                               uint32_t n_frames, bool fused) {
    rtp::PlanIn in{};
    in.W = la.width(), in.H = la.height();
    in.light_bounces = la.light_bounces();
    in.gws = global_work_size;
    in.range_first = k->range_first, in.range_last = k->range_last;
    in.n_frames = n_frames;
    in.sched = k->sched, in.math = k->math;
    in.stats = k->stats, in.hit_bound = k->hit_ids != nullptr;
    in.fused = fused, in.overlap = ctx->overlap;
    in.band_period = k->band_period, in.band_phase = k->band_phase;
    const rti::DeviceScene& sc = k->scene;
    in.n_nodes = sc.n_nodes(), in.n_tris = sc.n_tris(), in.n_mats = sc.n_mats(), in.n_top = sc.n_top();
    in.oct_ok = sc.oct_ok();
    in.goct_available = sc.goct() != nullptr, in.goct_b = sc.goct_b();
    in.force_global = k->force_global;
    in.tune = k->tune;
    in.num_cus = ctx->num_cus;
    // the tiles that can see the scene, from this launch's own camera slots and the root bounds as they
    // are now (held frames share one argument copy, so one rectangle serves a fused launch)
    if (const float* rb = sc.root_bounds()) in.view = rtp::view_cull_rect(in.W, in.H, la.f3[0], la.f3[1], la.f3[2], rb, rb + 3);
    // the path kill: the scene's cached certificate for this math's material table, and the launch's own
    // arguments for the plan's half of it
    in.kill_scene_ok = sc.path_kill_ok(k->math == RT_MATH_SHIPPED);
    in.light_type = la.light_type(), in.skybox_intensity = la.skybox_intensity();
    return in;
}

// The octant records a launch of walk `w` reads: the collapsed link set (rt_scene_pack.cpp,
// collapse_oct_links) unless the launch reports traversal counters -- a stats launch's visits stay the
// reference's -- or the scene's boxes were moved by a device refit since they were packed.  The kernels
// are the same either way: only this pointer differs.  Where the octant-cull certificate is known too
// (rt_octant_cull.cpp) the launch takes the pruned set (prune_oct_links), which is the collapsed set less
// the links into subtrees no ray of the octant can hit, under the same two conditions.  For a scene whose
// boxes nest, "the collapsed set" is the gate-skipped one (gate_skip_oct_links), which contains it, and the
// pruned set is built over that: rti::DeviceScene hands out whichever the scene has.  Remembers the
// choice for rtKernelGetNodeCollapse, rtKernelGetGateSkip and rtKernelGetOctantCull.
static const float4* oct_records(rt_kernel k, rtk::Walk w, bool regrouped) {
    const rti::DeviceScene& sc = k->scene;
    const bool pruned = sc.cull_ok() && (!k->stats || RT_OCTANT_CULL_STATS);
    const bool collapsed = sc.collapse_ok() && (!k->stats || RT_NODE_COLLAPSE_STATS || pruned);
    k->last_collapsed = collapsed && w != rtk::Walk::GlobalNodes;
    k->last_pruned = pruned && w != rtk::Walk::GlobalNodes;
    if (pruned) return regrouped ? sc.goct_pruned() : sc.oct_nodes_pruned();
    if (collapsed) return regrouped ? sc.goct_collapsed() : sc.oct_nodes_collapsed();
    return regrouped ? sc.goct() : sc.oct_nodes();
}

// KernelEntry's arguments: the plan's scalars plus the kernel's pointers (the radiance set and the
// work counters follow, once their resources are there)
static void fill_args(rt_kernel k, const LaunchArgs& la, uint32_t first_frame, const rtp::LaunchPlan& p,
                      rtk::KernelArgs* args) {
    rtk::KernelArgs& a = *args;
    std::memset(&a, 0, sizeof(a));
    a.result = static_cast<float4*>(la.out()->dptr);
    a.trisFull = static_cast<const rt_cl_triangle*>(la.tris()->dptr);
    a.materials = static_cast<const rt_cl_material*>(la.materials()->dptr);
    const rti::DeviceScene& sc = k->scene;
    a.packedTris = sc.packed_tris();
    a.octNodes = oct_records(k, p.variant.walk, p.regrouped);
    a.gNodes = sc.g_nodes();
    a.shadeTris = sc.shade_tris();
    a.shadeMats = sc.shade_mats() + (k->math == RT_MATH_SHIPPED ? 4 * (size_t)sc.n_mats() : 0);
    a.nMats = sc.n_mats(), a.nTris = sc.n_tris();
    a.nNodes = p.nNodes, a.octStride = p.octStride, a.octB = p.octB, a.octRecords = p.octRecords, a.nTop = p.nTop;
    fill_camera(la, first_frame, &a);
    a.lightBounces = la.light_bounces(), a.lightType = la.light_type();
    a.skyboxIntensity = la.skybox_intensity();
    a.gidBegin = p.gidBegin, a.gidEnd = p.gidEnd;
    a.rowBegin = p.rowBegin, a.rowCount = p.rowCount, a.tilesX = p.tilesX, a.nTiles = p.nTiles;
    a.bandPeriod = p.bandPeriod, a.bandPhase = p.bandPhase;
    a.visTx0 = p.visTx0, a.visTy0 = p.visTy0, a.visW = p.visW, a.visH = p.visH, a.visTiles = p.visTiles;
    a.pathKill = p.pathKill;
    a.chunkPixels = p.chunkPixels, a.tailChunk = p.tailChunk, a.chunkSplit = p.chunkSplit, a.tailBase = p.tailBase;
    a.staticFirst = p.staticFirst, a.nParts = p.nParts, a.partLen = p.partLen;
    a.refillMin = p.refillMin, a.shadeMin = p.shadeMin;
    a.stepWeightNode = p.stepWeightNode, a.stepWeightLeaf = p.stepWeightLeaf;
    a.flagTiles = p.flagTiles, a.tileMajor = p.tileMajor, a.nFrames = p.nFrames, a.radStride = p.radStride;
    a.hitIds = k->hit_ids ? static_cast<int32_t*>(k->hit_ids->dptr) : nullptr;
    a.hitT = k->hit_t ? static_cast<float*>(k->hit_t->dptr) : nullptr;
    a.stats = k->counters.stats();
    // per-frame launches: their own counters (two slots in turn with RT_PF_COUNTER_SLOTS, below)
    a.workCounter = k->counters.per_frame();
    if (p.use_pf_sky) {
        a.pfKeyIn = k->counters.key_in();
        a.pfKeyOut = k->counters.key_out();
    }
}

// the stream a fused render of radiance set `rs` goes to, made to wait for what it must follow
static int pick_render_stream(rt_context ctx, rt_kernel k, bool own_stream, int rs, hipStream_t* rstr) {
    if (own_stream) {
        // the set's own render stream, after everything queued on the main stream so far
        // (buffer writes, per-frame launches) but not after the previous step's render or
        // accumulation: it fills the CUs that render's draining waves free.  (With hit
        // buffers bound the renders stay in order on the main stream: each writes them.)
        *rstr = ctx->rstream[ctx->rnext];
        ctx->rnext = (ctx->rnext + 1) % RT_RENDER_STREAMS;
        hipError_t me = rti::main_tail_wait(ctx, *rstr);
        if (me != hipSuccess) return map_hip(me);
    }
    // the render writes the set: after the accumulation that last read it
    return map_hip(k->rad.wait_free(rs, *rstr));
}

// fused frames: the gamma accumulation of every frame, in order, per pixel -- on the
// accumulation stream after this render, overlapping whatever the main stream runs next
// (the next fused render uses the other radiance set); qs() joins it back
static int enqueue_accum(rt_context ctx, rt_kernel k, const rtk::KernelArgs& a, hipStream_t rstr) {
    hipStream_t as = ctx->stream;
    if (!ctx->overlap) ctx->mdirty = true;
    // The render left its chunk counters for this accumulation to clear (accum_key_body); if
    // the accumulation cannot be enqueued, clear them behind the render (same stream as the
    // set's next render), so that render does not start with spent counters and skip tiles.
    auto fail = [&](int rc) {
        (void)hipMemsetAsync(a.workCounter, 0, 16, rstr);
        return rc;
    };
    hipError_t e = hipSuccess;
    if (ctx->overlap) {
        as = ctx->astream;
        e = k->rad.after_render(rstr, as);
        if (e != hipSuccess) return fail(map_hip(e));
    }
    LaunchTimer::Bracket timed = k->timer.bracket(k->timing, as, LaunchTimer::kAccum);
    if (!timed.begin()) return fail(RT_OUT_OF_RESOURCES);
    // (a root's gather copies of the previous image read `out`: the accumulation that rewrites
    // it comes after them)
    e = rti::out_read_wait(ctx, as);
    if (e != hipSuccess) return fail(map_hip(e));
#ifndef RT_DIAG_NO_ACCUM  // diagnostic A/B builds only (wrong images): the render without its accumulation
    e = rtk::launch_accum_frames(a, k->math, k->counters.fused_keys(), as);
    if (e != hipSuccess) return fail(map_hip(e));
#endif
    timed.end();
    if (ctx->overlap) {
        e = k->rad.accumulated(as, ctx->atail);
        if (e != hipSuccess) return map_hip(e);
        ctx->apending = true;
    }
    return RT_SUCCESS;
}

static int enqueue(rt_context ctx, rt_kernel k, const LaunchArgs& args, size_t global_work_size,
                   uint32_t first_frame, uint32_t n_frames) {
    // 1. the handles, the arguments, the scene
    int rc = ensure_device(ctx);
    if (rc) return rc;
    if (!k || k->ctx != ctx) return RT_INVALID_KERNEL;
    rc = check_launch_args(k, args, global_work_size);
    if (rc) return rc;
    rc = prepare_scene(k, args);
    if (rc) return rc;

    // 2. defer, fused
    const int si = rtp::resolve_schedule(k->sched, args.light_bounces());
    const bool wf = si == rtk::kSchedWavefront;
    // radiance per (frame slot, work-item) + the accumulation launch: fused frames, every wavefront
    // render, and (RT_TUNE_PERFRAME_DEFER) per-frame step launches -- then consecutive renders need
    // not wait for each other, only the accumulations are ordered
    // A loop that synchronises every frame -- the reference's RenderFrame: ExecuteKernel,
    // ReadBuffer, Finish -- gains nothing from it and pays the second launch, and so do small
    // frames; frames queued back to back gain (4K Cornell 1.11 -> 0.92 ms/frame).  So by default
    // (PERFRAME_DEFER 2) a large launch defers when the host has not waited on the context through
    // this API since the kernel's previous per-frame launch: the host is queueing, not waiting
    // (profiles/r03/perframe_defer_auto.txt).  "Queueing" = no host wait on the context (rtFinish,
    // a blocking read or write) since the previous per-frame launch: no GPU-side query, which
    // would itself cost the read-back loop (an event after every render: 3.63 -> 4.07 ms/frame).
    bool defer = false;
    if (n_frames == 1 && si == RT_SCHED_STEP && k->tune.pf_defer) {
        defer = k->tune.pf_defer == 1 ||
                (k->tune.pf_defer == 2 && k->pf_waits == ctx->host_waits && global_work_size >= k->tune.pf_defer_min &&
                 !ctx->mexposed && !ctx->dexposed);  // (a host that can synchronise outside the library)
        k->pf_waits = ctx->host_waits;
    }
    const bool fused = n_frames > 1 || wf || defer;
    // a launch that accumulates in-kernel read-modify-writes the output: after the pending
    // accumulations
    if (!fused) (void)qs(ctx);

    // 3. the plan (rt_launch_plan.cpp), with the kernel's occupancy at the LDS size it chose
    const rtp::PlanIn in = plan_inputs(ctx, k, args, global_work_size, n_frames, fused);
    rtp::LaunchPlan p;
    rc = rtp::plan_shape(in, &p);
    if (rc || p.nothing) return rc;
    const rtk::Variant& v = p.variant;
    rtp::plan_handout(in, k->occ.get(wf ? rtk::Family::WfExtend : rtk::Family::Entry, v, p.smem),
                      wf ? k->occ.get(rtk::Family::WfShade, v, 0) : 0, &p);

    // 4. the kernel's arguments
    rtk::KernelArgs a;
    fill_args(k, args, first_frame, p, &a);

    // 5, 6. fused: the radiance set and the stream this launch's render goes to
    hipStream_t rstr = ctx->stream;
    if (fused) {
        const int rs = k->rad.current(ctx->overlap);
        rc = k->rad.ensure(ctx, rs, p.need, p.fneed);
        if (rc) return rc;
        rc = pick_render_stream(ctx, k, p.own_stream, rs, &rstr);
        if (rc) return rc;
        a.radBuf = k->rad.radiance(rs);
        a.frameFlags = k->rad.flags(rs);
        // one chunk counter per radiance set: renders of the two sets may run together
        a.workCounter = k->counters.fused(rs);
    }
    // everything below (counter clear, timing events, the render; the accumulation when it is not
    // overlapped) goes to rstr: the main stream unless a render stream was taken above
    if (rstr == ctx->stream) ctx->mdirty = true;
    k->last_lds = v.lds();
    k->last_kill = p.pathKill != 0u;

    // 7. wavefront: the ray queues
    rtk::WfArgs wa{};
    float4* wq[2] = {};
    uint32_t* wcnt[2] = {};
    if (wf) {
        rc = k->wfq.ensure((size_t)p.cap, p.G, rstr);
        if (rc) return rc;
        wq[0] = k->wfq.queue(0), wq[1] = k->wfq.queue(1);
        wcnt[0] = k->wfq.counts(0, p.G), wcnt[1] = k->wfq.counts(1, p.G);
        wa.hits = k->wfq.hits();
        wa.cap = p.cap, wa.G = p.G, wa.nBlocks = p.nBlocks, wa.refillMin = p.wfRefillMin;
    }

    // 8. the counter slot or clear, the timing events, the launch
    if (p.pf_slots) {
        a.workCounter = k->counters.per_frame_in_use();
        a.workCounterClear = k->counters.per_frame_to_clear();
    } else if (p.clear_counter_here) {
        hipError_t me = hipMemsetAsync(a.workCounter, 0, 16, rstr);
        if (me != hipSuccess) return map_hip(me);
    }
    LaunchTimer::Bracket timed = k->timer.bracket(k->timing, rstr, LaunchTimer::kRender);
    if (!timed.begin()) return RT_OUT_OF_RESOURCES;
    hipError_t e = wf ? rtk::launch_wavefront(a, wa, wq, wcnt, v, (unsigned)p.grid, p.smem, p.grid_s, rstr)
                      : rtk::launch_kernel_entry(a, v, (unsigned)p.grid, p.smem, rstr);
    if (e != hipSuccess) return map_hip(e);
    timed.end();
    if (a.pfKeyIn) k->counters.flip_key();
    if (p.pf_slots) k->counters.flip_per_frame_slot();  // flips only when the launch call reported success

    // 9. fused: the accumulation launch
    if (fused) {
        rc = enqueue_accum(ctx, k, a, rstr);
        if (rc) return rc;
    }
    // 10. bookkeeping
    rc = k->timer.drain_if_many();
    if (rc) return rc;
    ++k->launches;
    return RT_SUCCESS;
}

// ---- batched ray queries (rt_query.hpp; the plan: rt_query_plan.cpp) ----------------------------

// the query plan's inputs: the range, the two buffers, the kernel's settings and its packed scene
// (packed false: before the scene is packed -- the range and argument checks only)
static rtp::QueryIn query_inputs(rt_context ctx, rt_kernel k, size_t rays_bytes, size_t first_ray, size_t n_rays,
                                 int mode, size_t hits_bytes, bool same_buffer, bool packed) {
    rtp::QueryIn in{};
    in.first_ray = first_ray, in.n_rays = n_rays;
    in.rays_bytes = rays_bytes, in.hits_bytes = hits_bytes;
    in.same_buffer = same_buffer;
    in.mode = mode;
    in.math = k->math, in.stats = k->stats;
    in.oct_ok = true;
    if (packed) {
        const rti::DeviceScene& sc = k->scene;
        in.n_nodes = sc.n_nodes(), in.n_tris = sc.n_tris();
        in.oct_ok = sc.oct_ok();
        in.goct_available = sc.goct() != nullptr, in.goct_b = sc.goct_b();
    }
    in.force_global = k->force_global;
    in.tune = k->tune;
    in.num_cus = ctx->num_cus;
    return in;
}

// a planned query's arguments: the packed scene of k, the range and the two arrays
static void fill_query_args(rt_kernel k, const rtp::QueryPlan& p, const float4* rays, float4* hits, rtk::KernelArgs* args,
                            rtk::QueryArgs* qargs) {
    rtk::KernelArgs& a = *args;
    std::memset(&a, 0, sizeof(a));
    a.packedTris = k->scene.packed_tris();
    a.octNodes = oct_records(k, p.variant.walk, p.regrouped);
    a.nTris = k->scene.n_tris();
    a.nNodes = p.nNodes, a.octStride = p.octStride, a.octB = p.octB, a.octRecords = p.octRecords;
    a.stepWeightNode = p.stepWeightNode, a.stepWeightLeaf = p.stepWeightLeaf;
    a.stats = k->counters.stats();
    rtk::QueryArgs& q = *qargs;
    q = rtk::QueryArgs{};
    q.rays = rays;
    q.hits = hits;
    q.first = p.first, q.count = p.count, q.nUnits = p.nUnits, q.refillMin = p.refillMin;
}

int rtEnqueueIntersectRays(rt_context ctx, rt_kernel k, rt_mem rays, size_t first_ray, size_t n_rays, int mode,
                           rt_mem hits) {
    // 1. the handles and the range: no scene is packed and nothing launched on an error
    int rc = queue_head(ctx, k, {rays, hits});
    if (rc) return rc;
    rtp::QueryPlan p;
    rc = rtp::query_shape(query_inputs(ctx, k, rays->size, first_ray, n_rays, mode, hits->size, rays == hits, false), &p);
    if (rc || p.nothing) return pending_error(ctx, rc);
    if (!k->args.has({RT_ARG_BUFFER_SCENE, RT_ARG_BUFFER_NODE})) return RT_INVALID_KERNEL_ARGS;
    // 2. the scene, packed and validated as a render launch does (materials only when bound)
    rc = prepare_scene(k, k->args);
    if (rc) return rc;
    // 3. the plan, with the kernel's occupancy at the LDS size it chose
    const rtp::QueryIn in = query_inputs(ctx, k, rays->size, first_ray, n_rays, mode, hits->size, false, true);
    rc = rtp::query_shape(in, &p);
    if (rc || p.nothing) return rc;
    rtp::query_grid(in, k->occ.get(rtk::Family::Query, p.variant, p.smem), &p);
    // 4. the arguments
    rtk::KernelArgs a;
    rtk::QueryArgs q;
    fill_query_args(k, p, static_cast<const float4*>(rays->dptr), static_cast<float4*>(hits->dptr), &a, &q);
    // 5. the launch, on the context's stream after the pending accumulations and gathers
    k->last_lds = p.variant.lds();
    return launch_on_queue(ctx, k, hits,
                           [&](hipStream_t st) { return rtk::launch_query(a, q, p.variant, p.grid, p.smem, st); });
}

int rtEnqueueCameraRays(rt_context ctx, rt_kernel k, size_t global_work_size, rt_mem rays) {
    const int rc = queue_head(ctx, k, {rays});
    if (rc) return rc;
    if (!k->args.has({RT_ARG_WIDTH, RT_ARG_HEIGHT, RT_ARG_FRAME_COUNT, RT_ARG_CAMERA_POS, RT_ARG_CAMERA_FRONT,
                      RT_ARG_CAMERA_UP}))
        return RT_INVALID_KERNEL_ARGS;
    if (global_work_size == 0 || global_work_size > 0xffffffffull) return RT_INVALID_GLOBAL_WORK_SIZE;
    rtk::KernelArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_camera(k->args, k->args.frame_count(), &a);
    if (a.width == 0 || a.height == 0) return RT_INVALID_KERNEL_ARGS;
    if (rays->size / sizeof(rt_ray) < global_work_size) return RT_INVALID_BUFFER_SIZE;
    const hipError_t e =
        rtk::launch_camera_rays(a, static_cast<float4*>(rays->dptr), (uint32_t)global_work_size, k->math, qs(ctx));
    if (e != hipSuccess) return map_hip(e);
    mark_device_write(rays, true);
    return pending_error(ctx, RT_SUCCESS);
}

// ---- path tracing over caller rays (rt_trace.hpp; the plan: rt_trace_plan.cpp) -------------------

// a planned trace's arguments: the packed scene of k with its shading and material records, the three
// light slots, the range and the arrays
static void fill_trace_args(rt_kernel k, const rtp::TracePlan& p, rtk::KernelArgs* args) {
    rtk::KernelArgs& a = *args;
    std::memset(&a, 0, sizeof(a));
    const rti::DeviceScene& sc = k->scene;
    a.packedTris = sc.packed_tris();
    a.octNodes = oct_records(k, p.variant.walk, p.regrouped);
    a.shadeTris = sc.shade_tris();
    a.shadeMats = sc.shade_mats() + (k->math == RT_MATH_SHIPPED ? 4 * (size_t)sc.n_mats() : 0);
    a.nTris = sc.n_tris(), a.nMats = sc.n_mats();
    a.nNodes = p.nNodes, a.octStride = p.octStride, a.octB = p.octB, a.octRecords = p.octRecords;
    a.lightBounces = k->args.light_bounces(), a.lightType = k->args.light_type();
    a.skyboxIntensity = k->args.skybox_intensity();
    a.stepWeightNode = p.stepWeightNode, a.stepWeightLeaf = p.stepWeightLeaf;
    a.stats = k->counters.stats();
}

int rtEnqueueTracePaths(rt_context ctx, rt_kernel k, rt_mem rays, rt_mem seeds, size_t first, size_t n,
                        const rt_trace_params* params, rt_mem out) {
    // 1. the handles, then the coalesced frames: another call touches the context
    int rc = queue_head(ctx, k, {});
    if (rc) return rc;
    // 2. the arguments, in the plan's order: no scene is packed and nothing launched on an error
    rtp::TraceIn in{};
    in.params_given = params != nullptr;
    in.encoding = params ? params->encoding : 0;
    in.first = first, in.n = n;
    in.rays_ok = rays && rays->ctx == ctx, in.out_ok = out && out->ctx == ctx;
    in.seeds_given = seeds != nullptr, in.seeds_ok = seeds && seeds->ctx == ctx;
    in.out_is_input = out && (out == rays || out == seeds);
    in.rays_bytes = in.rays_ok ? rays->size : 0, in.out_bytes = in.out_ok ? out->size : 0;
    in.seeds_bytes = in.seeds_ok ? seeds->size : 0;
    in.scene_bound = k->args.has({RT_ARG_BUFFER_SCENE, RT_ARG_BUFFER_NODE, RT_ARG_BUFFER_MATERIAL});
    in.lights_set = k->args.has({RT_ARG_LIGHT_BOUNCES, RT_ARG_LIGHT_TYPE, RT_ARG_SKYBOX_INTENSITY});
    in.oct_ok = true;
    rc = rtp::trace_check(in);
    if (rc) return pending_error(ctx, rc);
    // 3. the scene, packed and validated as a render launch does
    rc = prepare_scene(k, k->args);
    if (rc) return rc;
    // 4. the plan, with the kernel's occupancy at the LDS size it chose
    in.math = k->math, in.stats = k->stats, in.shadow_rays = k->shadow_rays;
    const rti::DeviceScene& sc = k->scene;
    in.n_nodes = sc.n_nodes(), in.n_tris = sc.n_tris(), in.n_mats = sc.n_mats();
    in.oct_ok = sc.oct_ok();
    in.goct_available = sc.goct() != nullptr, in.goct_b = sc.goct_b();
    in.force_global = k->force_global;
    in.tune = k->tune;
    in.num_cus = ctx->num_cus;
    rtp::TracePlan p;
    rc = rtp::trace_shape(in, &p);
    if (rc || p.nothing) return pending_error(ctx, rc);
    rtp::trace_grid(in, k->occ.get(rtk::Family::Trace, p.variant, p.smem), &p);
    // 5. the arguments
    rtk::KernelArgs a;
    fill_trace_args(k, p, &a);
    rtk::TraceArgs q{};
    q.rays = static_cast<const float4*>(rays->dptr);
    q.seeds = seeds ? static_cast<const uint32_t*>(seeds->dptr) : nullptr;
    q.out = static_cast<float4*>(out->dptr);
    q.first = p.first, q.count = p.count, q.nUnits = p.nUnits;
    q.refillMin = p.refillMin, q.shadeMin = p.shadeMin;
    q.seedBase = params->seed_base, q.encoding = params->encoding;
    // 6. the launch, on the context's stream after the pending accumulations and gathers
    k->last_lds = p.variant.lds();
    return launch_on_queue(ctx, k, out,
                           [&](hipStream_t st) { return rtk::launch_trace(a, q, p.variant, p.grid, p.smem, st); });
}

int rtEnqueueCameraPaths(rt_context ctx, rt_kernel k, size_t global_work_size, rt_mem rays, rt_mem seeds) {
    // (rtEnqueueCameraRays' checks in its order, the seeds' where the rays' are)
    const int rc = queue_head(ctx, k, {rays, seeds});
    if (rc) return rc;
    if (rays == seeds) return RT_INVALID_MEM_OBJECT;
    if (!k->args.has({RT_ARG_WIDTH, RT_ARG_HEIGHT, RT_ARG_FRAME_COUNT, RT_ARG_CAMERA_POS, RT_ARG_CAMERA_FRONT,
                      RT_ARG_CAMERA_UP}))
        return RT_INVALID_KERNEL_ARGS;
    if (global_work_size == 0 || global_work_size > 0xffffffffull) return RT_INVALID_GLOBAL_WORK_SIZE;
    rtk::KernelArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_camera(k->args, k->args.frame_count(), &a);
    if (a.width == 0 || a.height == 0) return RT_INVALID_KERNEL_ARGS;
    if (rays->size / sizeof(rt_ray) < global_work_size || seeds->size / 4 < global_work_size)
        return RT_INVALID_BUFFER_SIZE;
    const hipError_t e = rtk::launch_camera_paths(a, static_cast<float4*>(rays->dptr), static_cast<uint32_t*>(seeds->dptr),
                                                  (uint32_t)global_work_size, k->math, qs(ctx));
    if (e != hipSuccess) return map_hip(e);
    mark_device_write(rays, true);
    mark_device_write(seeds, true);
    return pending_error(ctx, RT_SUCCESS);
}

// ---- surface records of ray hits (rt_surface.hpp; the plan: rt_query_plan.cpp surface_plan) -------

// the surface kernel's arguments: the scene records it gathers from, packed by prepare_scene
static void fill_surface_args(rt_kernel k, rtk::KernelArgs* args) {
    rtk::KernelArgs& a = *args;
    std::memset(&a, 0, sizeof(a));
    a.trisFull = static_cast<const rt_cl_triangle*>(k->args.tris()->dptr);
    a.packedTris = k->scene.packed_tris();
    a.shadeTris = k->scene.shade_tris();
    a.nTris = k->scene.n_tris();
}

int rtEnqueueHitSurfaces(rt_context ctx, rt_kernel k, rt_mem rays, rt_mem hits, size_t first, size_t n,
                         rt_mem surfaces) {
    // 1. the handles and the range: no scene is packed and nothing launched on an error
    int rc = queue_head(ctx, k, {rays, hits});
    if (rc) return rc;
    rtp::SurfaceIn in{};
    in.first = first, in.n = n;
    in.rays_bytes = rays->size, in.hits_bytes = hits->size;
    in.out_ok = surfaces && surfaces->ctx == ctx;
    in.out_bytes = in.out_ok ? surfaces->size : 0;
    in.out_is_input = surfaces == rays || surfaces == hits;
    in.rays_is_hits = rays == hits;
    in.scene_bound = k->args.has({RT_ARG_BUFFER_SCENE, RT_ARG_BUFFER_NODE});
    rtp::SurfacePlan p;
    rc = rtp::surface_plan(in, &p);
    if (rc || p.nothing) return pending_error(ctx, rc);
    // 2. the scene, packed and validated as a query does (materials only when bound)
    rc = prepare_scene(k, k->args);
    if (rc) return rc;
    // 3. the arguments
    rtk::KernelArgs a;
    fill_surface_args(k, &a);
    rtk::SurfaceArgs s{};
    s.rays = static_cast<const float4*>(rays->dptr);
    s.hits = static_cast<const float4*>(hits->dptr);
    s.out = static_cast<float4*>(surfaces->dptr);
    s.first = p.first, s.count = p.count;
    // 4. the launch, on the context's stream after the pending accumulations and gathers
    return launch_on_queue(ctx, k, surfaces,
                           [&](hipStream_t st) { return rtk::launch_surfaces(a, s, k->math, false, p.grid, st); });
}

int rtEnqueueFrameFeatures(rt_context ctx, rt_kernel k, size_t global_work_size, unsigned n_frames, rt_mem features) {
    // 1. the handles and the arguments: nothing is allocated or launched on an error
    int rc = queue_head(ctx, k, {features});
    if (rc) return rc;
    if (n_frames == 0 || n_frames > rtp::kMaxFeatureFrames) return RT_INVALID_VALUE;
    if (!k->args.has({RT_ARG_BUFFER_SCENE, RT_ARG_BUFFER_NODE, RT_ARG_BUFFER_MATERIAL, RT_ARG_WIDTH, RT_ARG_HEIGHT,
                      RT_ARG_FRAME_COUNT, RT_ARG_CAMERA_POS, RT_ARG_CAMERA_FRONT, RT_ARG_CAMERA_UP}))
        return RT_INVALID_KERNEL_ARGS;
    rtk::KernelArgs cam;
    std::memset(&cam, 0, sizeof(cam));
    fill_camera(k->args, k->args.frame_count(), &cam);
    if (cam.width == 0 || cam.height == 0) return RT_INVALID_KERNEL_ARGS;
    if (global_work_size == 0 || global_work_size > 0xffffffffull) return RT_INVALID_GLOBAL_WORK_SIZE;
    if (features->size / rtp::kFeatureBytes < global_work_size) return RT_INVALID_BUFFER_SIZE;
    // 2. the scene, and the plans of the frame's query and fold over the scratch (RT_INVALID_OPERATION:
    // a leaf of more than 127 triangles, as for queries)
    rc = prepare_scene(k, k->args);
    if (rc) return rc;
    const size_t gws = global_work_size;
    const rtp::QueryIn qin =
        query_inputs(ctx, k, gws * rtp::kRayBytes, 0, gws, RT_QUERY_CLOSEST, gws * rtp::kHitBytes, false, true);
    rtp::QueryPlan qp;
    rc = rtp::query_shape(qin, &qp);
    if (rc) return rc;
    rtp::query_grid(qin, k->occ.get(rtk::Family::Query, qp.variant, qp.smem), &qp);
    rtp::SurfaceIn sin{};
    sin.n = gws;
    sin.rays_bytes = gws * rtp::kRayBytes, sin.hits_bytes = gws * rtp::kHitBytes, sin.out_bytes = features->size;
    sin.out_ok = true, sin.scene_bound = true, sin.accumulate = true;
    rtp::SurfacePlan sp;
    rc = rtp::surface_plan(sin, &sp);
    if (rc) return rc;
    // 3. the scratch, before anything is enqueued (growing it waits for nothing: rt_internal.hpp)
    const hipError_t me = k->feat.reserve(gws);
    if (me != hipSuccess) return map_hip(me);
    // 4. the arguments
    rtk::KernelArgs qa, sa;
    rtk::QueryArgs q;
    fill_query_args(k, qp, k->feat.rays(), k->feat.hits(), &qa, &q);
    fill_surface_args(k, &sa);
    sa.materials = static_cast<const rt_cl_material*>(k->args.materials()->dptr);
    sa.nMats = k->scene.n_mats();
    rtk::SurfaceArgs s{};
    s.rays = k->feat.rays();
    s.hits = k->feat.hits();
    s.out = static_cast<float4*>(features->dptr);
    s.first = sp.first, s.count = sp.count;
    s.inv = 1.0f / (float)n_frames;
    // 5. per frame, in frame order on the context's stream: the camera's rays, their closest hits, the fold
    k->last_lds = qp.variant.lds();
    return launch_on_queue(ctx, k, features, [&](hipStream_t st) {
        hipError_t e = hipSuccess;
        for (unsigned f = 0; f < n_frames && e == hipSuccess; ++f) {
            cam.frameCount = k->args.frame_count() + f;  // (uint32 wrap, as the render's)
            s.accFirst = f == 0, s.accLast = f + 1 == n_frames;
            e = rtk::launch_camera_rays(cam, k->feat.rays(), (uint32_t)gws, k->math, st);
            if (e == hipSuccess) e = rtk::launch_query(qa, q, qp.variant, qp.grid, qp.smem, st);
            if (e == hipSuccess) e = rtk::launch_surfaces(sa, s, k->math, true, sp.grid, st);
        }
        return e;
    });
}

// ---- feature-guided a-trous denoise (rt_denoise.hip; the plan: rt_denoise_plan.cpp) ---------------

int rtEnqueueDenoise(rt_context ctx, rt_kernel k, rt_mem image, rt_mem features, unsigned width, unsigned height,
                     const rt_denoise_params* params, rt_mem out) {
    // 1. the handles and the plan: nothing is allocated or launched on an error
    int rc = queue_head(ctx, k, {});
    if (rc) return rc;
    rtp::DenoiseIn in{};
    in.params_ok = params != nullptr;
    if (params) {
        in.iterations = params->iterations;
        in.sigma_color = params->sigma_color, in.sigma_normal = params->sigma_normal;
        in.sigma_depth = params->sigma_depth, in.sigma_albedo = params->sigma_albedo;
    }
    in.width = width, in.height = height;
    in.image_ok = image && image->ctx == ctx;
    in.features_ok = features && features->ctx == ctx;
    in.out_ok = out && out->ctx == ctx;
    in.out_is_input = out && (out == image || out == features);
    in.image_bytes = in.image_ok ? image->size : 0;
    in.features_bytes = in.features_ok ? features->size : 0;
    in.out_bytes = in.out_ok ? out->size : 0;
    rtp::DenoisePlan p;
    rc = rtp::denoise_plan(in, &p);
    if (rc) return pending_error(ctx, rc);
    // 2. the scratch and one launch per iteration
    rtd::DenoiseArgs a{};
    a.features = static_cast<const float4*>(features->dptr);
    a.width = p.width, a.height = p.height;
    a.terms = p.terms;
    a.invN = p.inv_n, a.invZ = p.inv_z, a.invA = p.inv_a;
    return enqueue_atrous(ctx, k, p, static_cast<float4*>(image->dptr), out,
                          [&](unsigned, const rtp::DenoiseStep& t, const float4* src, float4* dst, hipStream_t st) {
                              a.src = src, a.dst = dst;
                              a.tilesX = t.tiles_x, a.tilesPerClass = t.tiles_per_class;
                              a.invC = t.inv_c;
                              return rtd::launch_denoise(a, t, st);
                          });
}

// ---- variance-guided a-trous denoise over the sample statistics (rt_denoise_samples.hip; the plan:
// rt_denoise_plan.cpp) -------------------------------------------------------------------------------

int rtEnqueueDenoiseSamples(rt_context ctx, rt_kernel k, rt_mem stats, rt_mem features, unsigned width, unsigned height,
                            const rt_denoise_samples_params* params, rt_mem out, rt_mem variance) {
    // 1. the handles and the plan: nothing is allocated or launched on an error
    int rc = queue_head(ctx, k, {});
    if (rc) return rc;
    rtp::DenoiseSamplesIn in{};
    in.params_ok = params != nullptr;
    if (params) {
        in.iterations = params->iterations;
        in.sigma_luminance = params->sigma_luminance, in.sigma_normal = params->sigma_normal;
        in.sigma_depth = params->sigma_depth, in.sigma_albedo = params->sigma_albedo;
        in.epsilon = params->epsilon, in.encoding = params->encoding;
    }
    in.width = width, in.height = height;
    in.stats_ok = stats && stats->ctx == ctx;
    in.features_ok = features && features->ctx == ctx;
    in.out_ok = out && out->ctx == ctx;
    in.variance_given = variance != nullptr, in.variance_ok = variance && variance->ctx == ctx;
    in.aliased = (out && (out == stats || out == features)) ||
                 (variance && (variance == stats || variance == features || variance == out));
    in.stats_bytes = in.stats_ok ? stats->size : 0;
    in.features_bytes = in.features_ok ? features->size : 0;
    in.out_bytes = in.out_ok ? out->size : 0;
    in.variance_bytes = in.variance_ok ? variance->size : 0;
    rtp::DenoiseSamplesPlan p;
    rc = rtp::denoise_samples_plan(in, &p);
    if (rc) return pending_error(ctx, rc);
    // 2. the scratch rtEnqueueDenoise uses and one launch per iteration (the first stages from the
    // statistics: its src slot is not read)
    rtd::DenoiseSamplesArgs a{};
    a.stats = static_cast<const float4*>(stats->dptr);
    a.features = static_cast<const float4*>(features->dptr);
    a.variance = p.write_variance ? static_cast<float*>(variance->dptr) : nullptr;
    a.width = p.width, a.height = p.height;
    a.terms = p.terms, a.encoding = p.encoding;
    a.sigmaL = p.sigma_luminance, a.epsilon = p.epsilon;
    a.invN = p.inv_n, a.invZ = p.inv_z, a.invA = p.inv_a;
    return enqueue_atrous(ctx, k, p, nullptr, out,
                          [&](unsigned i, const rtp::DenoiseStep& t, const float4* src, float4* dst, hipStream_t st) {
                              a.src = src, a.dst = dst;
                              a.tilesX = t.tiles_x, a.tilesPerClass = t.tiles_per_class;
                              a.last = p.last[i] ? 1u : 0u;
                              const hipError_t e = rtd::launch_denoise_samples(a, t, p.first[i], st);
                              // (the last iteration is launched only after every other one was)
                              if (e == hipSuccess && p.last[i] && p.write_variance) mark_device_write(variance, true);
                              return e;
                          });
}

// ---- temporal reprojection (rt_temporal.hip; the plan: rt_temporal_plan.cpp) -----------------------

// (motion null: rtEnqueueTemporalAccumulate itself)
static int enqueue_temporal(rt_context ctx, rt_kernel k, rt_mem cur, rt_mem cur_features, rt_mem hist,
                            rt_mem hist_features, rt_mem motion, unsigned width, unsigned height,
                            const rt_temporal_params* params, rt_mem out) {
    // 1. the handles and the plan: nothing is launched on an error
    int rc = queue_head(ctx, k, {});
    if (rc) return rc;
    rtp::TemporalIn in{};
    in.params_ok = params != nullptr;
    if (params) {
        in.cur = view_of(params->cur), in.prev = view_of(params->prev);
        in.cur_frames = params->cur_frames, in.history_frames = params->history_frames;
        in.max_history = params->max_history;
        in.depth_tolerance = params->depth_tolerance, in.normal_threshold = params->normal_threshold;
    }
    in.width = width, in.height = height;
    in.hist_given = hist != nullptr, in.hist_features_given = hist_features != nullptr;
    in.cur_ok = cur && cur->ctx == ctx;
    in.cur_features_ok = cur_features && cur_features->ctx == ctx;
    in.out_ok = out && out->ctx == ctx;
    in.hist_ok = hist && hist->ctx == ctx;
    in.hist_features_ok = hist_features && hist_features->ctx == ctx;
    in.out_is_input = out && (out == cur || out == cur_features || out == hist || out == hist_features || out == motion);
    in.motion_given = motion != nullptr, in.motion_ok = motion && motion->ctx == ctx;
    in.motion_bytes = in.motion_ok ? motion->size : 0;
    in.cur_bytes = in.cur_ok ? cur->size : 0;
    in.cur_features_bytes = in.cur_features_ok ? cur_features->size : 0;
    in.hist_bytes = in.hist_ok ? hist->size : 0;
    in.hist_features_bytes = in.hist_features_ok ? hist_features->size : 0;
    in.out_bytes = in.out_ok ? out->size : 0;
    rtp::TemporalPlan p;
    rc = rtp::temporal_plan(in, &p);
    if (rc) return pending_error(ctx, rc);
    // 2. one launch, in order on the context's stream after the pending accumulations and gathers
    rtt::TemporalArgs a{};
    a.cur = static_cast<const float4*>(cur->dptr);
    a.cur_features = static_cast<const float4*>(cur_features->dptr);
    a.hist = p.has_history ? static_cast<const float4*>(hist->dptr) : nullptr;
    a.hist_features = p.has_history ? static_cast<const float4*>(hist_features->dptr) : nullptr;
    a.out = static_cast<float4*>(out->dptr);
    const float4* records = p.has_motion ? static_cast<const float4*>(motion->dptr) : nullptr;
    a.width = p.width, a.height = p.height, a.tilesX = p.tiles_x;
    a.cur_frames = p.cur_frames, a.history_frames = p.history_frames, a.max_history = p.max_history;
    a.depth_tolerance = p.depth_tolerance, a.normal_threshold = p.normal_threshold;
    a.k = p.k;
    return launch_on_queue(ctx, k, out, [&](hipStream_t st) { return rtt::launch_temporal(a, records, p, st); });
}

int rtEnqueueTemporalAccumulate(rt_context ctx, rt_kernel k, rt_mem cur, rt_mem cur_features, rt_mem hist,
                                rt_mem hist_features, unsigned width, unsigned height,
                                const rt_temporal_params* params, rt_mem out) {
    return enqueue_temporal(ctx, k, cur, cur_features, hist, hist_features, nullptr, width, height, params, out);
}

int rtEnqueueTemporalAccumulateMotion(rt_context ctx, rt_kernel k, rt_mem cur, rt_mem cur_features, rt_mem hist,
                                      rt_mem hist_features, rt_mem motion, unsigned width, unsigned height,
                                      const rt_temporal_params* params, rt_mem out) {
    return enqueue_temporal(ctx, k, cur, cur_features, hist, hist_features, motion, width, height, params, out);
}

// ---- reprojection of the sample statistics (rt_reproject.hip; the plan: rt_reproject_plan.cpp) ------

// (motion null: rtEnqueueReprojectSamples itself)
static int enqueue_reproject(rt_context ctx, rt_kernel k, rt_mem hist_stats, rt_mem hist_features, rt_mem cur_features,
                             rt_mem motion, unsigned width, unsigned height, const rt_reproject_params* params,
                             rt_mem out_stats) {
    // 1. the handles and the plan: nothing is launched on an error
    int rc = queue_head(ctx, k, {});
    if (rc) return rc;
    rtp::ReprojectIn in{};
    in.params_ok = params != nullptr;
    if (params) {
        in.cur = view_of(params->cur), in.prev = view_of(params->prev);
        in.max_history = params->max_history;
        in.depth_tolerance = params->depth_tolerance, in.normal_threshold = params->normal_threshold;
    }
    in.width = width, in.height = height;
    in.hist_stats_ok = hist_stats && hist_stats->ctx == ctx;
    in.hist_features_ok = hist_features && hist_features->ctx == ctx;
    in.cur_features_ok = cur_features && cur_features->ctx == ctx;
    in.out_ok = out_stats && out_stats->ctx == ctx;
    in.out_is_input = out_stats && (out_stats == hist_stats || out_stats == hist_features || out_stats == cur_features ||
                                    out_stats == motion);
    in.motion_given = motion != nullptr, in.motion_ok = motion && motion->ctx == ctx;
    in.motion_bytes = in.motion_ok ? motion->size : 0;
    in.hist_stats_bytes = in.hist_stats_ok ? hist_stats->size : 0;
    in.hist_features_bytes = in.hist_features_ok ? hist_features->size : 0;
    in.cur_features_bytes = in.cur_features_ok ? cur_features->size : 0;
    in.out_bytes = in.out_ok ? out_stats->size : 0;
    rtp::ReprojectPlan p;
    rc = rtp::reproject_plan(in, &p);
    if (rc) return pending_error(ctx, rc);
    // 2. one launch, in order on the context's stream after the pending accumulations and gathers
    rtrs::ReprojectArgs a{};
    a.hist_stats = static_cast<const float4*>(hist_stats->dptr);
    a.hist_features = static_cast<const float4*>(hist_features->dptr);
    a.cur_features = static_cast<const float4*>(cur_features->dptr);
    a.out_stats = static_cast<float4*>(out_stats->dptr);
    const float4* records = p.has_motion ? static_cast<const float4*>(motion->dptr) : nullptr;
    a.width = p.width, a.height = p.height, a.tilesX = p.tiles_x;
    a.max_history = p.max_history, a.depth_tolerance = p.depth_tolerance, a.normal_threshold = p.normal_threshold;
    a.k = p.k;
    return launch_on_queue(ctx, k, out_stats, [&](hipStream_t st) { return rtrs::launch_reproject(a, records, p, st); });
}

int rtEnqueueReprojectSamples(rt_context ctx, rt_kernel k, rt_mem hist_stats, rt_mem hist_features, rt_mem cur_features,
                              unsigned width, unsigned height, const rt_reproject_params* params, rt_mem out_stats) {
    return enqueue_reproject(ctx, k, hist_stats, hist_features, cur_features, nullptr, width, height, params, out_stats);
}

int rtEnqueueReprojectSamplesMotion(rt_context ctx, rt_kernel k, rt_mem hist_stats, rt_mem hist_features,
                                    rt_mem cur_features, rt_mem motion, unsigned width, unsigned height,
                                    const rt_reproject_params* params, rt_mem out_stats) {
    return enqueue_reproject(ctx, k, hist_stats, hist_features, cur_features, motion, width, height, params, out_stats);
}

// ---- adaptive sampling (rt_adaptive.hip, rt_trace.hpp; the plans: rt_adaptive_plan.cpp) -------------

int rtEnqueueAccumulateSamples(rt_context ctx, rt_kernel k, rt_mem ids, rt_mem results, size_t first, size_t n,
                               size_t n_pixels, rt_mem stats) {
    // 1. the handles and the plan: nothing is launched on an error
    int rc = queue_head(ctx, k, {});
    if (rc) return rc;
    rtp::AccumIn in{};
    in.first = first, in.n = n, in.n_pixels = n_pixels;
    in.ids_given = ids != nullptr, in.ids_ok = ids && ids->ctx == ctx;
    in.results_ok = results && results->ctx == ctx, in.stats_ok = stats && stats->ctx == ctx;
    in.stats_is_input = stats && (stats == ids || stats == results);
    in.ids_bytes = in.ids_ok ? ids->size : 0, in.results_bytes = in.results_ok ? results->size : 0;
    in.stats_bytes = in.stats_ok ? stats->size : 0;
    rtp::AccumPlan p;
    rc = rtp::accumulate_plan(in, &p);
    if (rc || p.nothing) return pending_error(ctx, rc);
    // 2. one launch, in order on the context's stream after the pending accumulations and gathers
    rta::AccumArgs a{};
    a.ids = ids ? static_cast<const uint32_t*>(ids->dptr) : nullptr;
    a.results = static_cast<const float4*>(results->dptr);
    a.stats = static_cast<float4*>(stats->dptr);
    a.first = p.first, a.count = p.count, a.n_pixels = p.n_pixels;
    return launch_on_queue(ctx, k, stats, [&](hipStream_t st) { return rta::launch_accumulate(a, p, st); });
}

int rtEnqueueSelectPixels(rt_context ctx, rt_kernel k, rt_mem stats, unsigned width, unsigned height,
                          const rt_adaptive_params* params, rt_mem ids, rt_mem result) {
    // 1. the handles and the plan: nothing is allocated or launched on an error
    int rc = queue_head(ctx, k, {});
    if (rc) return rc;
    rtp::SelectIn in{};
    in.params_ok = params != nullptr;
    if (params) {
        in.threshold = params->threshold, in.floor_y = params->floor_y;
        in.min_samples = params->min_samples, in.max_samples = params->max_samples, in.radius = params->radius;
    }
    in.width = width, in.height = height;
    in.stats_ok = stats && stats->ctx == ctx, in.ids_ok = ids && ids->ctx == ctx;
    in.result_ok = result && result->ctx == ctx;
    in.aliased = (ids && (ids == stats || ids == result)) || (result && result == stats);
    in.stats_bytes = in.stats_ok ? stats->size : 0, in.ids_bytes = in.ids_ok ? ids->size : 0;
    in.result_bytes = in.result_ok ? result->size : 0;
    rtp::SelectPlan p;
    rc = rtp::select_plan(in, &p);
    if (rc) return pending_error(ctx, rc);
    // 2. the scratch, before anything is enqueued (growing it waits for nothing: rt_internal.hpp)
    const hipError_t me = k->adaptive.reserve((size_t)p.scratch_bytes);
    if (me != hipSuccess) return map_hip(me);
    // 3. flags, count, scan, scatter: in order on the context's stream after the pending accumulations
    rta::SelectArgs a{};
    a.stats = static_cast<const float4*>(stats->dptr);
    a.ids = static_cast<uint32_t*>(ids->dptr);
    a.result = static_cast<uint4*>(result->dptr);
    a.scratch = k->adaptive.bytes();
    return launch_on_queue(ctx, k, ids, [&](hipStream_t st) {
        const hipError_t e = rta::launch_select(a, p, st);
        if (e == hipSuccess) mark_device_write(result, true);
        return e;
    });
}

int rtEnqueueCameraPathsFor(rt_context ctx, rt_kernel k, rt_mem ids, size_t first, size_t n, rt_mem rays, rt_mem seeds) {
    // 1. the handles and the plan: nothing is launched on an error
    int rc = queue_head(ctx, k, {});
    if (rc) return rc;
    rtp::PathsForIn in{};
    in.slots_set = k->args.has({RT_ARG_WIDTH, RT_ARG_HEIGHT, RT_ARG_FRAME_COUNT, RT_ARG_CAMERA_POS, RT_ARG_CAMERA_FRONT,
                                RT_ARG_CAMERA_UP});
    rtk::KernelArgs a;
    std::memset(&a, 0, sizeof(a));
    if (in.slots_set) fill_camera(k->args, k->args.frame_count(), &a);
    in.width = a.width, in.height = a.height;
    in.first = first, in.n = n;
    in.ids_ok = ids && ids->ctx == ctx, in.rays_ok = rays && rays->ctx == ctx, in.seeds_ok = seeds && seeds->ctx == ctx;
    in.aliased = (rays && (rays == ids || rays == seeds)) || (seeds && seeds == ids);
    in.ids_bytes = in.ids_ok ? ids->size : 0, in.rays_bytes = in.rays_ok ? rays->size : 0;
    in.seeds_bytes = in.seeds_ok ? seeds->size : 0;
    rtp::PathsForPlan p;
    rc = rtp::paths_for_plan(in, &p);
    if (rc || p.nothing) return pending_error(ctx, rc);
    // 2. one launch in k's math mode, in order on the context's stream
    return launch_on_queue(ctx, k, rays, [&](hipStream_t st) {
        const hipError_t e = rtk::launch_camera_paths_for(a, static_cast<const uint32_t*>(ids->dptr), p.first, p.count,
                                                          static_cast<float4*>(rays->dptr),
                                                          static_cast<uint32_t*>(seeds->dptr), p.grid, k->math, st);
        if (e == hipSuccess) mark_device_write(seeds, true);
        return e;
    });
}

// One sample for the listed pixels in one launch (rt_sample.hpp): rtEnqueueTracePaths' six steps, with the
// camera slots and the statistics where the trace has the caller's arrays.
int rtEnqueueSamplePixels(rt_context ctx, rt_kernel k, rt_mem ids, rt_mem count, size_t first, size_t n, size_t n_pixels,
                          rt_mem stats) {
    // 1. the handles, then the coalesced frames: another call touches the context
    int rc = queue_head(ctx, k, {});
    if (rc) return rc;
    // 2. the arguments, in the plan's order: no scene is packed and nothing launched on an error
    rtp::SampleIn in{};
    in.first = first, in.n = n, in.n_pixels = n_pixels;
    in.ids_ok = ids && ids->ctx == ctx, in.stats_ok = stats && stats->ctx == ctx;
    in.count_given = count != nullptr, in.count_ok = count && count->ctx == ctx;
    in.aliased = (stats && (stats == ids || stats == count)) || (count && count == ids);
    in.ids_bytes = in.ids_ok ? ids->size : 0, in.stats_bytes = in.stats_ok ? stats->size : 0;
    in.count_bytes = in.count_ok ? count->size : 0;
    in.slots_set = k->args.has({RT_ARG_WIDTH, RT_ARG_HEIGHT, RT_ARG_FRAME_COUNT, RT_ARG_CAMERA_POS, RT_ARG_CAMERA_FRONT,
                                RT_ARG_CAMERA_UP});
    if (in.slots_set) in.width = k->args.width(), in.height = k->args.height();
    in.scene_bound = k->args.has({RT_ARG_BUFFER_SCENE, RT_ARG_BUFFER_NODE, RT_ARG_BUFFER_MATERIAL});
    in.lights_set = k->args.has({RT_ARG_LIGHT_BOUNCES, RT_ARG_LIGHT_TYPE, RT_ARG_SKYBOX_INTENSITY});
    rtp::SamplePlan p;
    rc = rtp::sample_check(in, &p);
    if (rc || p.nothing) return pending_error(ctx, rc);
    // 3. the scene, packed and validated as a render launch does
    rc = prepare_scene(k, k->args);
    if (rc) return rc;
    // 4. the plan, with the kernel's occupancy at the LDS size it chose
    rtp::TraceIn& t = in.scene;
    t.math = k->math, t.stats = k->stats, t.shadow_rays = k->shadow_rays;
    const rti::DeviceScene& sc = k->scene;
    t.n_nodes = sc.n_nodes(), t.n_tris = sc.n_tris(), t.n_mats = sc.n_mats();
    t.oct_ok = sc.oct_ok();
    t.goct_available = sc.goct() != nullptr, t.goct_b = sc.goct_b();
    t.force_global = k->force_global;
    t.tune = k->tune;
    t.num_cus = ctx->num_cus;
    rc = rtp::sample_shape(in, &p);
    if (rc || p.nothing) return pending_error(ctx, rc);
    rtp::sample_grid(in, k->occ.get(rtk::Family::Sample, p.trace.variant, p.trace.smem), &p);
    // 5. the arguments: the trace's, the camera's, the ids, the count and the statistics
    rtk::KernelArgs a;
    fill_trace_args(k, p.trace, &a);
    fill_camera(k->args, k->args.frame_count(), &a);
    rtk::SampleArgs q{};
    q.ids = static_cast<const uint32_t*>(ids->dptr);
    q.count = count ? static_cast<const uint32_t*>(count->dptr) : nullptr;
    q.stats = static_cast<float4*>(stats->dptr);
    q.first = p.first, q.n = p.n, q.nPixels = p.n_pixels;
    q.refillMin = p.trace.refillMin, q.shadeMin = p.trace.shadeMin;
    // 6. the launch, on the context's stream after the pending accumulations and gathers
    k->last_lds = p.trace.variant.lds();
    return launch_on_queue(ctx, k, stats, [&](hipStream_t st) {
        return rtk::launch_sample(a, q, p.trace.variant, p.trace.grid, p.trace.smem, st);
    });
}

int rtEnqueueResolveSamples(rt_context ctx, rt_kernel k, rt_mem stats, unsigned width, unsigned height, rt_mem out) {
    // 1. the handles and the plan: nothing is launched on an error
    int rc = queue_head(ctx, k, {});
    if (rc) return rc;
    rtp::ResolveIn in{};
    in.width = width, in.height = height;
    in.stats_ok = stats && stats->ctx == ctx, in.out_ok = out && out->ctx == ctx;
    in.out_is_input = out && out == stats;
    in.stats_bytes = in.stats_ok ? stats->size : 0, in.out_bytes = in.out_ok ? out->size : 0;
    rtp::ResolvePlan p;
    rc = rtp::resolve_plan(in, &p);
    if (rc) return pending_error(ctx, rc);
    // 2. one launch, in order on the context's stream after the pending accumulations and gathers
    rta::ResolveArgs a{};
    a.stats = static_cast<const float4*>(stats->dptr);
    a.out = static_cast<float4*>(out->dptr);
    return launch_on_queue(ctx, k, out, [&](hipStream_t st) { return rta::launch_resolve(a, p, st); });
}

int rtBuildBVH(rt_context ctx, rt_mem tris, size_t n_tris, unsigned max_prims_in_node, rt_mem nodes,
               size_t* n_nodes) {
    return rtBuildBVHEx(ctx, tris, n_tris, max_prims_in_node, RT_BVH_PLOC, nodes, n_nodes);
}

int rtBuildBVHEx(rt_context ctx, rt_mem tris, size_t n_tris, unsigned max_prims_in_node, int method, rt_mem nodes,
                 size_t* n_nodes) {
    if (method != RT_BVH_LBVH && method != RT_BVH_PLOC) return RT_INVALID_VALUE;
    int rc = ensure_device(ctx);
    if (rc) return rc;
    (void)rti::flush_frames(ctx);
    if (!tris || !nodes || tris->ctx != ctx || nodes->ctx != ctx) return RT_INVALID_MEM_OBJECT;
    if (tris == nodes) return RT_INVALID_MEM_OBJECT;  // the build would overwrite its own input
    if (!n_nodes || n_tris == 0 || n_tris >= (1u << 30)) return RT_INVALID_VALUE;
    if (tris->size < n_tris * sizeof(rt_cl_triangle)) return RT_INVALID_BUFFER_SIZE;
    if (nodes->size < (2 * n_tris - 1) * sizeof(rt_cl_bvh_node)) return RT_INVALID_BUFFER_SIZE;
    const uint32_t mp = std::max(1u, std::min(max_prims_in_node, 65535u));
    void* scratch = nullptr;
    const size_t scratch_size = rtb::scratch_bytes((uint32_t)n_tris);
    if (scratch_size == 0) return RT_OUT_OF_RESOURCES;  // rocPRIM could not size its temporaries
    hipError_t e = hipMalloc(&scratch, scratch_size);
    if (e != hipSuccess) return map_hip(e);
    uint32_t count = 0;
    e = rtb::build(static_cast<rt_cl_triangle*>(tris->dptr), (uint32_t)n_tris, mp,
                   static_cast<rt_cl_bvh_node*>(nodes->dptr), &count, scratch, qs(ctx), method);
    if (e == hipSuccess) e = hipStreamSynchronize(qs(ctx));
    (void)hipFree(scratch);
    if (e != hipSuccess) return map_hip(e);
    for (rt_mem m : {tris, nodes}) mark_device_write(m, true);
    *n_nodes = count;
    return RT_SUCCESS;
}

// ---- moving geometry (rt_refit.hip) --------------------------------------------------------------

int rtEnqueueUpdateVertices(rt_context ctx, rt_mem tris, size_t first_tri, size_t n_tris, rt_mem positions,
                            rt_mem normals) {
    int rc = ensure_device(ctx);
    if (rc) return rc;
    if (!tris || !positions || tris->ctx != ctx || positions->ctx != ctx || (normals && normals->ctx != ctx))
        return RT_INVALID_MEM_OBJECT;
    if (positions == tris || normals == tris) return RT_INVALID_MEM_OBJECT;
    const size_t nt = tris->size / sizeof(rt_cl_triangle);
    if (first_tri > nt || n_tris > nt - first_tri || nt > 0x40000000ull) return RT_INVALID_BUFFER_SIZE;
    if (positions->size / sizeof(rt_tri_points) < n_tris || (normals && normals->size / sizeof(rt_tri_points) < n_tris))
        return RT_INVALID_BUFFER_SIZE;
    if (n_tris == 0) return RT_SUCCESS;
    // coalesced frames launch first, reading (and packing) the scene as it was
    rc = flush_first(ctx);
    if (rc) return rc;
    const hipError_t e = rtr::launch_update_vertices(
        static_cast<rt_cl_triangle*>(tris->dptr), (uint32_t)first_tri, (uint32_t)n_tris,
        static_cast<const float4*>(positions->dptr), normals ? static_cast<const float4*>(normals->dptr) : nullptr,
        qs(ctx));
    if (e != hipSuccess) return map_hip(e);
    mark_device_write(tris, false);  // positions and normals only
    return pending_error(ctx, RT_SUCCESS);
}

int rtRefitBVH(rt_context ctx, rt_kernel k) {
    int rc = ensure_device(ctx);
    if (rc) return rc;
    if (!k || k->ctx != ctx) return RT_INVALID_KERNEL;
    if (!k->args.has({RT_ARG_BUFFER_SCENE, RT_ARG_BUFFER_NODE})) return RT_INVALID_KERNEL_ARGS;
    rc = flush_first(ctx);  // coalesced frames launch first, on the scene as it was
    if (rc) return rc;
    rc = k->scene.refit(ctx, k->args.tris(), k->args.nodes(), k->args.materials());
    return rc ? rc : pending_error(ctx, RT_SUCCESS);
}

int rtDiagScenePrepares(rt_kernel k, uint64_t* full, uint64_t* refits) {
    if (!k) return RT_INVALID_KERNEL;
    if (full) *full = k->scene.full_prepares();
    if (refits) *refits = k->scene.refits();
    return RT_SUCCESS;
}

// ---- motion records (rt_motion.hip, rt_motion.hpp; the plans: rt_motion_plan.cpp) ------------------

int rtEnqueueExtractVertices(rt_context ctx, rt_mem tris, size_t first_tri, size_t n_tris, rt_mem positions,
                             rt_mem normals) {
    int rc = ensure_device(ctx);
    if (rc) return rc;
    rtp::ExtractIn in{};
    in.tris_ok = tris && tris->ctx == ctx, in.positions_ok = positions && positions->ctx == ctx;
    in.normals_given = normals != nullptr, in.normals_ok = normals && normals->ctx == ctx;
    in.out_is_tris = tris && (positions == tris || normals == tris);
    in.outs_same = positions && positions == normals;
    in.tris_bytes = in.tris_ok ? tris->size : 0, in.positions_bytes = in.positions_ok ? positions->size : 0;
    in.normals_bytes = in.normals_ok ? normals->size : 0;
    in.first_tri = first_tri, in.n_tris = n_tris;
    rtp::ExtractPlan p;
    rc = rtp::extract_plan(in, &p);
    if (rc || p.nothing) return rc;
    // coalesced frames launch first: they were enqueued before this snapshot
    rc = flush_first(ctx);
    if (rc) return rc;
    const hipError_t e = rtmo::launch_extract_vertices(static_cast<const rt_cl_triangle*>(tris->dptr), p,
                                                       static_cast<float4*>(positions->dptr),
                                                       normals ? static_cast<float4*>(normals->dptr) : nullptr, qs(ctx));
    if (e != hipSuccess) return map_hip(e);
    mark_device_write(positions, true);
    if (normals) mark_device_write(normals, true);
    return pending_error(ctx, RT_SUCCESS);
}

// the prev_* arguments of the two motion calls as their plans take them
static rtp::PrevIn prev_inputs(rt_context ctx, rt_mem prev_positions, rt_mem prev_normals, size_t first_tri,
                               size_t n_tris, rt_mem out) {
    rtp::PrevIn in{};
    in.positions_given = prev_positions != nullptr, in.positions_ok = prev_positions && prev_positions->ctx == ctx;
    in.normals_given = prev_normals != nullptr, in.normals_ok = prev_normals && prev_normals->ctx == ctx;
    in.is_out = out && (prev_positions == out || prev_normals == out);
    in.positions_bytes = in.positions_ok ? prev_positions->size : 0;
    in.normals_bytes = in.normals_ok ? prev_normals->size : 0;
    in.first_tri = first_tri, in.n_tris = n_tris;
    return in;
}

int rtEnqueueHitMotion(rt_context ctx, rt_kernel k, rt_mem hits, size_t first, size_t n, rt_mem prev_positions,
                       rt_mem prev_normals, size_t first_tri, size_t n_tris, rt_mem motion) {
    // 1. the handles and the ranges: no scene is packed and nothing launched on an error
    int rc = queue_head(ctx, k, {hits});
    if (rc) return rc;
    rtp::HitMotionIn in{};
    in.first = first, in.n = n;
    in.hits_bytes = hits->size;
    in.out_ok = motion && motion->ctx == ctx;
    in.out_bytes = in.out_ok ? motion->size : 0;
    in.out_is_hits = motion == hits;
    in.scene_bound = k->args.has({RT_ARG_BUFFER_SCENE, RT_ARG_BUFFER_NODE});
    in.scene_tris = in.scene_bound ? k->args.tris()->size / sizeof(rt_cl_triangle) : 0;
    in.prev = prev_inputs(ctx, prev_positions, prev_normals, first_tri, n_tris, motion);
    rtp::HitMotionPlan p;
    rc = rtp::hit_motion_plan(in, &p);
    if (rc || p.nothing) return pending_error(ctx, rc);
    // 2. the scene, packed and validated as a query does (materials only when bound)
    rc = prepare_scene(k, k->args);
    if (rc) return rc;
    if ((uint64_t)p.first_tri + p.n_tris > k->scene.n_tris()) return RT_INVALID_BUFFER_SIZE;
    // 3. the launch, on the context's stream after the pending accumulations and gathers
    rtmo::HitMotionArgs a{};
    a.hits = static_cast<const float4*>(hits->dptr);
    a.tris = static_cast<const rt_cl_triangle*>(k->args.tris()->dptr);
    a.n_scene = k->scene.n_tris();
    a.prev_positions = p.n_tris ? static_cast<const float4*>(prev_positions->dptr) : nullptr;
    a.prev_normals = p.n_tris && prev_normals ? static_cast<const float4*>(prev_normals->dptr) : nullptr;
    a.out = static_cast<float4*>(motion->dptr);
    return launch_on_queue(ctx, k, motion, [&](hipStream_t st) { return rtmo::launch_hit_motion(a, p, st); });
}

int rtEnqueueFrameMotion(rt_context ctx, rt_kernel k, size_t global_work_size, rt_mem prev_positions,
                         rt_mem prev_normals, size_t first_tri, size_t n_tris, rt_mem motion) {
    // 1. the handles and the arguments: nothing is packed or launched on an error
    int rc = queue_head(ctx, k, {motion});
    if (rc) return rc;
    rtp::FrameMotionIn in{};
    in.args_bound = k->args.has({RT_ARG_BUFFER_SCENE, RT_ARG_BUFFER_NODE, RT_ARG_WIDTH, RT_ARG_HEIGHT,
                                 RT_ARG_CAMERA_POS, RT_ARG_CAMERA_FRONT, RT_ARG_CAMERA_UP});
    rtk::KernelArgs cam;
    std::memset(&cam, 0, sizeof(cam));
    if (in.args_bound) {
        fill_camera(k->args, 0, &cam);
        in.scene_tris = k->args.tris()->size / sizeof(rt_cl_triangle);
    }
    in.width = cam.width, in.height = cam.height;
    for (int c = 0; c < 3; ++c) in.cam.pos[c] = cam.camPos[c], in.cam.front[c] = cam.camFront[c], in.cam.up[c] = cam.camUp[c];
    in.global_work_size = global_work_size;
    in.out_bytes = motion->size;
    in.prev = prev_inputs(ctx, prev_positions, prev_normals, first_tri, n_tris, motion);
    rtp::FrameMotionPlan mp;
    rc = rtp::frame_motion_plan(in, &mp);
    if (rc) return pending_error(ctx, rc);
    // 2. the scene, and the plan of the closest-hit query over one ray per pixel (RT_INVALID_OPERATION:
    // a leaf of more than 127 triangles, as for queries)
    rc = prepare_scene(k, k->args);
    if (rc) return rc;
    if ((uint64_t)mp.first_tri + mp.n_tris > k->scene.n_tris()) return RT_INVALID_BUFFER_SIZE;
    const size_t gws = global_work_size;
    const rtp::QueryIn qin =
        query_inputs(ctx, k, gws * rtp::kRayBytes, 0, gws, RT_QUERY_CLOSEST, gws * rtp::kHitBytes, false, true);
    rtp::QueryPlan qp;
    rc = rtp::query_shape(qin, &qp);
    if (rc) return rc;
    rtp::query_grid(qin, k->occ.get(rtk::Family::Motion, qp.variant, qp.smem), &qp);
    // 3. the arguments: the query's, the current vertices and the image width
    rtk::KernelArgs a;
    rtk::QueryArgs q;
    fill_query_args(k, qp, nullptr, nullptr, &a, &q);
    a.trisFull = static_cast<const rt_cl_triangle*>(k->args.tris()->dptr);
    a.width = cam.width, a.height = cam.height;
    rtk::MotionArgs m{};
    m.prevPositions = mp.n_tris ? static_cast<const float4*>(prev_positions->dptr) : nullptr;
    m.prevNormals = mp.n_tris && prev_normals ? static_cast<const float4*>(prev_normals->dptr) : nullptr;
    m.out = static_cast<float4*>(motion->dptr);
    m.firstTri = mp.first_tri, m.nTris = mp.n_tris;
    m.count = mp.count, m.nUnits = qp.nUnits, m.refillMin = qp.refillMin;
    m.k = mp.k;
    // 4. one launch, on the context's stream after the pending accumulations and gathers
    k->last_lds = qp.variant.lds();
    return launch_on_queue(ctx, k, motion,
                           [&](hipStream_t st) { return rtk::launch_motion(a, m, qp.variant, qp.grid, qp.smem, st); });
}

// the host waits for the context's queue
static hipError_t host_wait(rt_context ctx) {
    ++ctx->host_waits;
    return hipStreamSynchronize(qs(ctx));
}

int rtEnqueueReadBuffer(rt_context ctx, rt_mem m, int blocking, size_t offset, size_t size, void* dst) {
    int rc = ensure_device(ctx);
    if (rc) return rc;
    if (!m || m->ctx != ctx) return RT_INVALID_MEM_OBJECT;
    if (!dst || offset > m->size || size > m->size - offset) return RT_INVALID_VALUE;
    hipError_t e = hipMemcpyAsync(dst, static_cast<uint8_t*>(m->dptr) + offset, size,
                                  hipMemcpyDeviceToHost, qs(ctx));
    if (e == hipSuccess && blocking) e = host_wait(ctx);
    return pending_error(ctx, map_hip(e));
}

int rtEnqueueWriteBuffer(rt_context ctx, rt_mem m, int blocking, size_t offset, size_t size,
                         const void* src) {
    int rc = ensure_device(ctx);
    if (rc) return rc;
    if (!m || m->ctx != ctx) return RT_INVALID_MEM_OBJECT;
    if (!src || offset > m->size || size > m->size - offset) return RT_INVALID_VALUE;
    // coalesced frames launch first, reading (and packing) the scene as it was
    (void)rti::flush_frames(ctx);
    if (m->shadow_valid) std::memcpy(m->shadow.data() + offset, src, size);
    ++m->generation;
    ++m->structural;
    hipError_t e = hipMemcpyAsync(static_cast<uint8_t*>(m->dptr) + offset, src, size,
                                  hipMemcpyHostToDevice, qs(ctx));
    if (e == hipSuccess && blocking) e = host_wait(ctx);
    return pending_error(ctx, map_hip(e));
}

int rtEnqueueCopyBufferToPointer(rt_context ctx, rt_mem m, size_t offset, size_t size, void* dst) {
    int rc = ensure_device(ctx);
    if (rc) return rc;
    if (!m || m->ctx != ctx) return RT_INVALID_MEM_OBJECT;
    if (!dst || offset > m->size || size > m->size - offset) return RT_INVALID_VALUE;
    return map_hip(hipMemcpyAsync(dst, static_cast<uint8_t*>(m->dptr) + offset, size,
                                  hipMemcpyDeviceToDevice, qs(ctx)));
}

int rtFinish(rt_context ctx) {
    int rc = ensure_device(ctx);
    if (rc) return rc;
    return pending_error(ctx, map_hip(host_wait(ctx)));
}

int rtKernelSetMathMode(rt_kernel k, int mode) {
    if (!k) return RT_INVALID_KERNEL;
    flush_kernel(k);
    if (mode != RT_MATH_PINNED && mode != RT_MATH_DEVICELIB && mode != RT_MATH_SHIPPED) return RT_INVALID_VALUE;
    k->math = mode;
    return RT_SUCCESS;
}

int rtKernelSetShadowRays(rt_kernel k, int enable) {
    if (!k) return RT_INVALID_KERNEL;
    flush_kernel(k);
    if (enable != 0 && enable != 1) return RT_INVALID_VALUE;
    k->shadow_rays = enable == 1;
    return RT_SUCCESS;
}

int rtKernelGetShadowRays(rt_kernel k, int* enable) {
    if (!k) return RT_INVALID_KERNEL;
    if (!enable) return RT_INVALID_VALUE;
    *enable = k->shadow_rays ? 1 : 0;
    return RT_SUCCESS;
}

int rtKernelSetSchedule(rt_kernel k, int sched) {
    if (!k) return RT_INVALID_KERNEL;
    flush_kernel(k);
    if (sched != RT_SCHED_TILES && sched != RT_SCHED_STEP &&
        sched != RT_SCHED_WAVEFRONT)
        return RT_INVALID_VALUE;
    k->sched = sched;
    return RT_SUCCESS;
}

int rtKernelSetRowInterleave(rt_kernel k, unsigned period, unsigned phase) {
    if (!k) return RT_INVALID_KERNEL;
    flush_kernel(k);
    if (period == 0 || phase >= period) return RT_INVALID_VALUE;
    k->band_period = period;
    k->band_phase = phase;
    k->comm_sharded = false;
    return RT_SUCCESS;
}

}  // extern "C"

// rtCommShardKernel: the gather's band plan counts bands from image row 0, the kernel from the
// first row of its work range -- so a comm-sharded kernel renders whole frames only
int rti::shard_kernel(rt_kernel k, unsigned period, unsigned phase) {
    flush_kernel(k);
    if (!k) return RT_INVALID_KERNEL;
    if (k->range_first != 0 || k->range_last != 0) return RT_INVALID_OPERATION;
    int rc = rtKernelSetRowInterleave(k, period, phase);
    if (rc == RT_SUCCESS) k->comm_sharded = true;
    return rc;
}

extern "C" {

int rtEnqueueCopyBufferRectToPointer(rt_context ctx, rt_mem src, size_t src_offset, size_t src_pitch,
                                     size_t width_bytes, size_t rows, void* dst, size_t dst_pitch) {
    int rc = ensure_device(ctx);
    if (rc) return rc;
    (void)rti::flush_frames(ctx);
    if (!src || src->ctx != ctx || !dst) return RT_INVALID_MEM_OBJECT;
    if (rows == 0 || width_bytes == 0) return RT_SUCCESS;
    if (width_bytes > src_pitch || width_bytes > dst_pitch) return RT_INVALID_VALUE;
    if (src_offset + (rows - 1) * src_pitch + width_bytes > src->size) return RT_INVALID_VALUE;
    if (ctx->readback_on_astream && ctx->overlap) {
        // after every accumulation enqueued so far, before any later one (astream is in order),
        // and after everything already queued on the main stream (a per-frame launch writes
        // `out` there; a fused render's tail is the accumulation's own dependency, so waiting on
        // it costs the overlap nothing); later main-stream work that joins (qs) waits for the
        // copy too
        hipError_t e = rti::main_tail_wait(ctx, ctx->astream);
        // ... and after the gathers queued so far (their unpack writes a root's image; nothing
        // else on astream waits for it)
        if (e == hipSuccess) e = rti::gather_wait(ctx, ctx->astream);
        if (e == hipSuccess)
            e = hipMemcpy2DAsync(dst, dst_pitch, static_cast<uint8_t*>(src->dptr) + src_offset, src_pitch,
                                 width_bytes, rows, hipMemcpyDeviceToDevice, ctx->astream);
        if (e == hipSuccess) e = hipEventRecord(ctx->atail, ctx->astream);
        if (e == hipSuccess) ctx->apending = true;
        return map_hip(e);
    }
    return map_hip(hipMemcpy2DAsync(dst, dst_pitch, static_cast<uint8_t*>(src->dptr) + src_offset, src_pitch,
                                    width_bytes, rows, hipMemcpyDeviceToDevice, qs(ctx)));
}

int rtContextSetReadbackOnAccumStream(rt_context ctx, int enable) {
    int rc = ensure_device(ctx);
    if (rc) return rc;
    (void)rti::flush_frames(ctx);
    ctx->readback_on_astream = enable != 0;
    return RT_SUCCESS;
}

int rtContextGetAccumStream(rt_context ctx, void** s) {
    if (!ctx) return RT_INVALID_CONTEXT;
    if (!s) return RT_INVALID_VALUE;
    if (!ctx->overlap) ctx->mexposed = true;  // the main stream leaves the library's view
    ctx->dexposed = true;  // the caller may synchronise with the stream outside the library
    (void)rti::flush_frames(ctx);
    *s = ctx->overlap ? ctx->astream : qs(ctx);
    return RT_SUCCESS;
}

int rtEnqueueCopyPointerRectToBuffer(rt_context ctx, const void* src, size_t src_pitch, rt_mem dst,
                                     size_t dst_offset, size_t dst_pitch, size_t width_bytes, size_t rows) {
    int rc = ensure_device(ctx);
    if (rc) return rc;
    (void)rti::flush_frames(ctx);
    if (!dst || dst->ctx != ctx || !src) return RT_INVALID_MEM_OBJECT;
    if (rows == 0 || width_bytes == 0) return RT_SUCCESS;
    if (width_bytes > src_pitch || width_bytes > dst_pitch) return RT_INVALID_VALUE;
    if (dst_offset + (rows - 1) * dst_pitch + width_bytes > dst->size) return RT_INVALID_VALUE;
    mark_device_write(dst, true);  // a scene buffer is re-read and repacked
    return map_hip(hipMemcpy2DAsync(static_cast<uint8_t*>(dst->dptr) + dst_offset, dst_pitch, src, src_pitch,
                                    width_bytes, rows, hipMemcpyDeviceToDevice, qs(ctx)));
}

int rtKernelSetWorkRange(rt_kernel k, uint64_t first, uint64_t last) {
    if (!k) return RT_INVALID_KERNEL;
    flush_kernel(k);
    if (last != 0 && last < first) return RT_INVALID_VALUE;
    if (k->comm_sharded && (first != 0 || last != 0)) return RT_INVALID_OPERATION;
    k->range_first = first;
    k->range_last = last;
    return RT_SUCCESS;
}

int rtKernelSetHitBuffers(rt_kernel k, rt_mem ids, rt_mem t) {
    if (!k) return RT_INVALID_KERNEL;
    flush_kernel(k);
    if ((ids == nullptr) != (t == nullptr)) return RT_INVALID_MEM_OBJECT;
    if (ids && (ids->ctx != k->ctx || t->ctx != k->ctx)) return RT_INVALID_MEM_OBJECT;
    k->hit_ids = ids;
    k->hit_t = t;
    return RT_SUCCESS;
}

int rtKernelSetStats(rt_kernel k, int enable) {
    if (!k) return RT_INVALID_KERNEL;
    flush_kernel(k);
    k->stats = enable != 0;
    return RT_SUCCESS;
}

int rtKernelSetTiming(rt_kernel k, int enable) {
    if (!k) return RT_INVALID_KERNEL;
    flush_kernel(k);
    k->timing = enable != 0;
    return RT_SUCCESS;
}

int rtKernelGetStats(rt_kernel k, rt_stats* out) {
    if (!k || !out) return RT_INVALID_VALUE;
    flush_kernel(k);
    int rc = ensure_device(k->ctx);
    if (rc) return rc;
    unsigned long long h[rti::WorkCounters::kStatWords] = {};
    hipError_t e = hipMemcpyAsync(h, k->counters.stats(), sizeof(h), hipMemcpyDeviceToHost, qs(k->ctx));
    if (e == hipSuccess) e = hipStreamSynchronize(qs(k->ctx));
    if (e != hipSuccess) return map_hip(e);
    rc = k->timer.drain();
    if (rc) return rc;
    out->rays = h[0];
    out->node_visits = h[1];
    out->tri_tests = h[2];
    out->hits = h[3];
    out->cycles_refill = h[4];
    out->cycles_traverse = h[5];
    out->cycles_shade = h[6];
    out->cycles_total = h[7];
    for (int i = 0; i < 12; ++i) out->sched[i] = h[8 + i];
    out->launches = k->launches;
    out->kernel_ms = k->timer.kernel_ms();
    out->accum_ms = k->timer.accum_ms();
    out->render_period_ms = k->timer.render_period_ms();
    return RT_SUCCESS;
}

int rtKernelGetPathKill(rt_kernel k, rt_path_kill_info* out) {
    if (!k || !out) return RT_INVALID_VALUE;
    flush_kernel(k);
    int rc = ensure_device(k->ctx);
    if (rc) return rc;
    unsigned long long h[2] = {};
    hipError_t e = hipMemcpyAsync(h, k->counters.stats() + rti::WorkCounters::kZeroBetaWord, sizeof(h),
                                  hipMemcpyDeviceToHost, qs(k->ctx));
    if (e == hipSuccess) e = hipStreamSynchronize(qs(k->ctx));
    if (e != hipSuccess) return map_hip(e);
    out->zero_hits = h[0];
    out->zero_misses = h[1];
    out->scene_certified = k->scene.path_kill_ok(k->math == RT_MATH_SHIPPED) ? 1 : 0;
    out->launch_certified = k->last_kill ? 1 : 0;
    return RT_SUCCESS;
}

int rtKernelGetNodeCollapse(rt_kernel k, rt_node_collapse_info* out) {
    if (!k || !out) return RT_INVALID_VALUE;
    flush_kernel(k);
    out->collapsed_links = k->scene.collapsed_links();
    out->scene_collapsible = k->scene.collapse_ok() ? 1 : 0;
    out->launch_collapsed = k->last_collapsed ? 1 : 0;
    return RT_SUCCESS;
}

int rtKernelGetGateSkip(rt_kernel k, rt_gate_skip_info* out) {
    if (!k || !out) return RT_INVALID_VALUE;
    flush_kernel(k);
    out->gate_links = k->scene.gate_links();
    out->scene_nested = k->scene.gate_skipped() && k->scene.collapse_ok() ? 1 : 0;
    out->launch_gate_skipped = k->scene.gate_skipped() && k->last_collapsed ? 1 : 0;
    return RT_SUCCESS;
}

int rtKernelGetOctantCull(rt_kernel k, rt_octant_cull_info* out) {
    if (!k || !out) return RT_INVALID_VALUE;
    flush_kernel(k);
    out->pruned_links = k->scene.pruned_links();
    out->contracted_links = 0;  // single-child interior nodes are not contracted (rt_scene_pack.cpp)
    out->scene_certified = k->scene.cull_ok() ? 1 : 0;
    out->launch_pruned = k->last_pruned ? 1 : 0;
    return RT_SUCCESS;
}

int rtKernelResetStats(rt_kernel k) {
    if (!k) return RT_INVALID_KERNEL;
    flush_kernel(k);
    int rc = ensure_device(k->ctx);
    if (rc) return rc;
    rc = k->timer.drain();
    if (rc) return rc;
    k->launches = 0;
    k->timer.reset();
    hipError_t e = k->counters.zero_stats(qs(k->ctx));
    if (e == hipSuccess) e = hipStreamSynchronize(qs(k->ctx));
    return map_hip(e);
}

int rtKernelGetSceneInLDS(rt_kernel k, int* in_lds) {
    if (!k || !in_lds) return RT_INVALID_VALUE;
    *in_lds = k->last_lds ? 1 : 0;
    return RT_SUCCESS;
}

int rtKernelForceGlobalScene(rt_kernel k, int force) {
    if (!k) return RT_INVALID_KERNEL;
    flush_kernel(k);
    k->force_global = force != 0;
    return RT_SUCCESS;
}

int rtBufferGetDevicePointer(rt_mem m, void** dptr) {
    if (!m || !dptr) return RT_INVALID_VALUE;
    (void)rti::flush_frames(m->ctx);  // the caller may touch the bytes
    // ... at any later time, after synchronising outside the library: no more frame coalescing
    if (m->ctx) m->ctx->dexposed = true;
    *dptr = m->dptr;
    return RT_SUCCESS;
}

int rtBufferGetSize(rt_mem m, size_t* size) {
    if (!m || !size) return RT_INVALID_VALUE;
    *size = m->size;
    return RT_SUCCESS;
}

int rtContextGetStream(rt_context ctx, void** s) {
    if (!ctx || !s) return RT_INVALID_VALUE;
    // the caller may enqueue there, or synchronise with it, without going through the library
    // (qs below also launches any coalesced frames; none are held back from now on)
    ctx->mexposed = true;
    *s = qs(ctx);
    return RT_SUCCESS;
}

}  // extern "C"


extern "C" {

int rtContextGetDevice(rt_context ctx, int* d) {
    if (!ctx || !d) return RT_INVALID_VALUE;
    *d = ctx->device;
    return RT_SUCCESS;
}

int rtValidateBVH(const void* nodes, size_t n_nodes, size_t n_tris, int* depth) {
    if (!nodes || n_nodes == 0 || n_nodes >= (1u << 30) || n_tris >= (1ull << 32)) return RT_INVALID_VALUE;
    int d = 0;
    uint32_t used = 0;
    int rc = rtp::check_nodes(static_cast<const rt_cl_bvh_node*>(nodes), (uint32_t)n_nodes, (uint32_t)n_tris, &d, &used);
    if (rc == RT_SUCCESS && depth) *depth = d;
    return rc;
}

int rtKernelSetTuning(rt_kernel k, int param, int value) {
    if (!k) return RT_INVALID_KERNEL;
    flush_kernel(k);
    if (param == RT_TUNE_TOP_NODES) {  // renumbers the packed node records: the scene is packed again
        if (value < 0 || value > 1024) return RT_INVALID_VALUE;
        k->scene.top_limit = (uint32_t)value;
        k->scene.invalidate();
        return RT_SUCCESS;
    }
    return rtp::tuning_set(k->tune, param, value);
}

int rtKernelGetTuning(rt_kernel k, int param, int* value) {
    if (!k) return RT_INVALID_KERNEL;
    if (!value) return RT_INVALID_VALUE;
    if (param == RT_TUNE_TOP_NODES) {
        *value = (int)k->scene.top_limit;
        return RT_SUCCESS;
    }
    return rtp::tuning_get(k->tune, param, value);
}

int rtContextSetAccumOverlap(rt_context ctx, int enable) {
    int rc = ensure_device(ctx);
    if (rc) return rc;
    // switching modes: everything queued so far completes on the old arrangement first
    hipError_t e = hipStreamSynchronize(qs(ctx));
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->astream);
    if (e != hipSuccess) return map_hip(e);
    ctx->overlap = enable != 0;
    return RT_SUCCESS;
}

int rtDiagPinnedMath(int device_index, int op, const float* a, const float* b, float* out, size_t n) {
    if (op < RT_PINNED_OP_RCP || op > RT_PINNED_OP_COS || !a || !out) return RT_INVALID_VALUE;
    const bool two = op == RT_PINNED_OP_DIV || op == RT_PINNED_OP_POW;
    if (two && !b) return RT_INVALID_VALUE;
    if (n == 0) return RT_SUCCESS;
    if (n > ((size_t)1 << 28)) return RT_INVALID_BUFFER_SIZE;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return RT_DEVICE_NOT_FOUND;
    if (device_index < 0 || device_index >= count) return RT_INVALID_DEVICE;
    hipError_t e = hipSetDevice(device_index);
    float* d = nullptr;
    const size_t bytes = n * sizeof(float);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d), 3 * bytes);
    if (e == hipSuccess) e = hipMemcpy(d, a, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess && two) e = hipMemcpy(d + n, b, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = rtk::launch_pinned_math(op, d, d + n, d + 2 * n, n, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, d + 2 * n, bytes, hipMemcpyDeviceToHost);
    if (d) (void)hipFree(d);
    return map_hip(e);
}

int rtDiagGammaPow(int device_index, int math, int check, int exponent, uint32_t first, uint64_t count,
                   uint64_t* mismatches, uint32_t* first_bad, uint32_t* first_bits) {
    if (math < RT_MATH_PINNED || math > RT_MATH_SHIPPED || check < RT_GAMMA_CHECK_POW || check > RT_GAMMA_CHECK_LEMMA ||
        exponent < 0 || exponent > 2 || !mismatches || !first_bad || !first_bits)
        return RT_INVALID_VALUE;
    if (count > ((uint64_t)1 << 32) - first) return RT_INVALID_VALUE;  // the sweep stays inside 2^32 patterns
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return RT_DEVICE_NOT_FOUND;
    if (device_index < 0 || device_index >= ndev) return RT_INVALID_DEVICE;
    hipError_t e = hipSetDevice(device_index);
    unsigned long long* d = nullptr;
    unsigned long long h[3] = {0ull, 0xffffffffull, 0ull};
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&d), sizeof h);
    if (e == hipSuccess) e = hipMemcpy(d, h, sizeof h, hipMemcpyHostToDevice);
    if (e == hipSuccess)
        e = rtk::launch_gamma_check(rtk::GammaCheckArgs{d, count, first, (uint32_t)check, (uint32_t)exponent}, math, nullptr);
    if (e == hipSuccess) e = hipMemcpy(h, d, sizeof h, hipMemcpyDeviceToHost);
    if (d) (void)hipFree(d);
    if (e != hipSuccess) return map_hip(e);
    *mismatches = h[0];
    *first_bad = (uint32_t)h[1];
    *first_bits = (uint32_t)h[2];
    return RT_SUCCESS;
}

const char* rtGetBuildInfo(void) {
    return "librt_hip: KernelEntry for gfx950 (HIP), math modes pinned|devicelib|shipped, scene in LDS or HBM";
}

}  // extern "C"

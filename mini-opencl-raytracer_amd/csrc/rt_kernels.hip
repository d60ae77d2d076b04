// rt_kernels.hip -- KernelEntry entry points for the pinned and devicelib math policies,
// the scene packing kernels and the host-side launch helpers: one rtk::Policy table per math
// policy (the shipped one from rt_kernels_shipped.hip), through which every launcher and the
// occupancy cache pick their kernel.  The device code is rt_kernels_body.hpp.
#include "rt_kernel_pick.hpp"

#pragma clang fp contract(off)

namespace rtk {

// Entry points per math policy: the devicelib body fits 80 VGPRs with a small spill, and
// 6 waves per SIMD measured 7 % faster than the 4 its natural 113 VGPRs allow
// (profiles/r01/occupancy_ab.txt); the fp64-heavy pinned body stays at its natural budget.
// (LDS scenes 5 waves per SIMD, scenes read from HBM/L2 6, as for the shipped policy)
template <bool kStats, bool kBofs, int kMode>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_STEP_DEVICELIB_WAVES, 8)))
void kernel_entry_step_devicelib_lds(KernelArgs a) {
    step_body<MathDeviceLib, true, kStats, kBofs, false, kMode>(a);
}
template <bool kStats, int kMode>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_STEP_GLOBAL_WAVES, 8)))
void kernel_entry_step_devicelib_global(KernelArgs a) {
    step_body<MathDeviceLib, false, kStats, false, false, kMode>(a);
}
template <bool kStats, int kMode>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_STEP_GOCT_WAVES, 8)))
void kernel_entry_step_devicelib_goct(KernelArgs a) {
    step_body<MathDeviceLib, true, kStats, false, true, kMode>(a);
}
// The pinned body on LDS scenes: 5 waves per SIMD (96 VGPRs, 80 B of spills) against the 4 its
// natural 116 VGPRs allow -- 4K Cornell 8 spp 1.044 -> 1.007 ms/frame (profiles/r06/pinned_ab.txt);
// the HBM/L2 walks keep their natural budget (1: no register cap)
#ifndef RT_STEP_PINNED_WAVES
#define RT_STEP_PINNED_WAVES 5
#endif
template <bool kLdsScene, bool kStats, bool kBofs, bool kGlobalOct, int kMode>
__global__ __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(kLdsScene && !kGlobalOct ? RT_STEP_PINNED_WAVES : 1, 8)))
void kernel_entry_step_pinned(KernelArgs a) {
    step_body<MathPinned, kLdsScene, kStats, kBofs, kGlobalOct, kMode>(a);
}


// ---- scene packing (runs once per bound scene) -----------------------------------------------
__global__ void pack_shade(const rt_cl_triangle* __restrict__ in, float4* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const rt_cl_triangle& t = in[i];
    out[3 * i] = make_float4(t.v1.normal.x, t.v1.normal.y, t.v1.normal.z, __uint_as_float(t.mtlIndex));
    out[3 * i + 1] = make_float4(t.v2.normal.x, t.v2.normal.y, t.v2.normal.z, t.v3.normal.x);
    out[3 * i + 2] = make_float4(t.v3.normal.y, t.v3.normal.z, 0.0f, 0.0f);
}

__global__ void pack_mats(const rt_cl_material* __restrict__ in, float4* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    material_record<MathDeviceLib>(in[i], out + 4 * i);
}

__global__ void pack_tris(const rt_cl_triangle* __restrict__ in, float4* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const rt_float3 p1 = in[i].v1.position, p2 = in[i].v2.position, p3 = in[i].v3.position;
    // e1 = t2 - t1, e2 = t3 - t1 exactly as kernel_bvh.cl:109-110 computes them
    // 9 floats in a 48-B slot, packed so that a lane reads them with two 16-B and one 4-B
    // access (3 x 12-B reads cost twice the LDS cycles of 3 x 16-B ones)
    out[3 * i] = make_float4(p1.x, p1.y, p1.z, p2.x - p1.x);
    out[3 * i + 1] = make_float4(p2.y - p1.y, p2.z - p1.z, p3.x - p1.x, p3.y - p1.y);
    out[3 * i + 2] = make_float4(p3.z - p1.z, 0.0f, 0.0f, 0.0f);
}

}  // namespace rtk

// ---- host-side launch helpers ------------------------------------------------------------
namespace rtk {

template <>
struct StepEntry<MathDeviceLib> {
    template <bool S, int kMode>
    static KernelFn get(Walk w) {
        switch (w) {
            case Walk::Lds: return kernel_entry_step_devicelib_lds<S, false, kMode>;
            case Walk::LdsB: return kernel_entry_step_devicelib_lds<S, true, kMode>;
            case Walk::GlobalOct: return kernel_entry_step_devicelib_goct<S, kMode>;
            default: return kernel_entry_step_devicelib_global<S, kMode>;
        }
    }
};
template <>
struct StepEntry<MathPinned> {
    template <bool S, int kMode>
    static KernelFn get(Walk w) {
        switch (w) {
            case Walk::Lds: return kernel_entry_step_pinned<true, S, false, false, kMode>;
            case Walk::LdsB: return kernel_entry_step_pinned<true, S, true, false, kMode>;
            case Walk::GlobalOct: return kernel_entry_step_pinned<true, S, false, true, kMode>;
            default: return kernel_entry_step_pinned<false, S, false, false, kMode>;
        }
    }
};

template <class M>
__global__ __launch_bounds__(256) RT_ACCUM_OCC void accum_frames(KernelArgs a, const uint32_t* key) {
    accum_frames_body<M>(a, key);
}
template <class M>
__global__ void accum_key(KernelArgs a, uint32_t* key) {
    accum_key_body<M>(a, key);
}
template <class M>
__global__ __launch_bounds__(256) void gamma_check(GammaCheckArgs g) {
    gamma_check_body<M>(g);
}

// the kernels of a math policy (pack_mats: the IEEE material records serve both policies of this TU)
static const Policy& policy(int math) {
    static const Policy devicelib = {pick_entry<MathDeviceLib>,   wf_pick<MathDeviceLib>,  query_pick<MathDeviceLib>,
                                     accum_frames<MathDeviceLib>, accum_key<MathDeviceLib>, camera_rays<MathDeviceLib>,
                                     pack_mats,
                                     hit_surfaces<MathDeviceLib, false>, hit_surfaces<MathDeviceLib, true>,
                                     trace_pick<MathDeviceLib>, camera_paths<MathDeviceLib>,
                                     camera_paths_for<MathDeviceLib>, sample_pick<MathDeviceLib>,
                                     motion_pick<MathDeviceLib>, gamma_check<MathDeviceLib>};
    static const Policy pinned = {pick_entry<MathPinned>,   wf_pick<MathPinned>,  query_pick<MathPinned>,
                                  accum_frames<MathPinned>, accum_key<MathPinned>, camera_rays<MathPinned>,
                                  pack_mats,
                                  hit_surfaces<MathPinned, false>, hit_surfaces<MathPinned, true>,
                                     trace_pick<MathPinned>, camera_paths<MathPinned>,
                                     camera_paths_for<MathPinned>, sample_pick<MathPinned>,
                                     motion_pick<MathPinned>, gamma_check<MathPinned>};
    return math == MathShipped::kId ? shipped_policy() : math == MathDeviceLib::kId ? devicelib : pinned;
}

hipError_t launch_kernel_entry(const KernelArgs& a, const Variant& v, unsigned grid, size_t smem, hipStream_t st) {
    hipLaunchKernelGGL(policy(v.math).entry(v), dim3(grid), dim3(256), smem, st, a);
    return hipGetLastError();
}

hipError_t launch_accum_frames(const KernelArgs& a, int math, uint32_t* key, hipStream_t st) {
    const Policy& p = policy(math);
    const dim3 grid((a.nTiles + kAccumWgWaves - 1u) / kAccumWgWaves);
    hipLaunchKernelGGL(p.accum_key, dim3(1), dim3(64), 0, st, a, key);
    hipLaunchKernelGGL(p.accum_frames, grid, dim3(64 * kAccumWgWaves), 0, st, a, key);
    return hipGetLastError();
}

// ---- wavefront schedule ------------------------------------------------------------------------
hipError_t launch_wavefront(const KernelArgs& a, WfArgs w, float4* const q[2], uint32_t* const cnt[2],
                            const Variant& v, unsigned grid_e, size_t smem_e, unsigned grid_s, hipStream_t st) {
    const WfKernels kf = policy(v.math).wavefront(v);
    for (int b = 0; b < a.lightBounces; ++b) {
        w.bounce = (uint32_t)b;
        w.inQ = q[b & 1];
        w.outQ = q[(b + 1) & 1];
        w.inCnt = cnt[b & 1];
        w.outCnt = cnt[(b + 1) & 1];
        hipLaunchKernelGGL(kf.extend, dim3(grid_e), dim3(kWfExtendThreads), smem_e, st, a, w);
        hipLaunchKernelGGL(kf.shade, dim3(grid_s), dim3(kWfShadeThreads), 0, st, a, w);
    }
    return hipGetLastError();
}

// ---- ray queries (rt_query.hpp) ------------------------------------------------------------------
hipError_t launch_query(const KernelArgs& a, const QueryArgs& q, const Variant& v, unsigned grid, size_t smem,
                        hipStream_t st) {
    hipLaunchKernelGGL(policy(v.math).query(v), dim3(grid), dim3(kQueryThreads), smem, st, a, q);
    return hipGetLastError();
}

// ---- motion records of the camera's centre rays (rt_motion.hpp) ------------------------------------
hipError_t launch_motion(const KernelArgs& a, const MotionArgs& m, const Variant& v, unsigned grid, size_t smem,
                         hipStream_t st) {
    hipLaunchKernelGGL(policy(v.math).motion(v), dim3(grid), dim3(kQueryThreads), smem, st, a, m);
    return hipGetLastError();
}

hipError_t launch_camera_rays(const KernelArgs& a, float4* rays, uint32_t n, int math, hipStream_t st) {
    const dim3 grid((unsigned)(((uint64_t)n + 255u) / 256u));
    hipLaunchKernelGGL(policy(math).camera_rays, grid, dim3(256), 0, st, a, rays, n);
    return hipGetLastError();
}

// ---- path tracing over caller rays (rt_trace.hpp) -------------------------------------------------
hipError_t launch_trace(const KernelArgs& a, const TraceArgs& q, const Variant& v, unsigned grid, size_t smem,
                        hipStream_t st) {
    hipLaunchKernelGGL(policy(v.math).trace(v), dim3(grid), dim3(kTraceThreads), smem, st, a, q);
    return hipGetLastError();
}

// ---- one adaptive sample per listed pixel (rt_sample.hpp) -----------------------------------------
hipError_t launch_sample(const KernelArgs& a, const SampleArgs& q, const Variant& v, unsigned grid, size_t smem,
                         hipStream_t st) {
    hipLaunchKernelGGL(policy(v.math).sample(v), dim3(grid), dim3(kTraceThreads), smem, st, a, q);
    return hipGetLastError();
}

hipError_t launch_camera_paths(const KernelArgs& a, float4* rays, uint32_t* seeds, uint32_t n, int math,
                               hipStream_t st) {
    const dim3 grid((unsigned)(((uint64_t)n + 255u) / 256u));
    hipLaunchKernelGGL(policy(math).camera_paths, grid, dim3(256), 0, st, a, rays, seeds, n);
    return hipGetLastError();
}

hipError_t launch_camera_paths_for(const KernelArgs& a, const uint32_t* ids, uint32_t first, uint32_t n, float4* rays,
                                   uint32_t* seeds, unsigned grid, int math, hipStream_t st) {
    if ((uint64_t)grid * 256u < n) return hipErrorInvalidValue;
    hipLaunchKernelGGL(policy(math).camera_paths_for, dim3(grid), dim3(256), 0, st, a, ids, first, n, rays, seeds);
    return hipGetLastError();
}

// ---- surface records (rt_surface.hpp) ------------------------------------------------------------
hipError_t launch_surfaces(const KernelArgs& a, const SurfaceArgs& s, int math, bool accumulate, unsigned grid,
                           hipStream_t st) {
    const Policy& p = policy(math);
    hipLaunchKernelGGL(accumulate ? p.surfaces_accum : p.surfaces, dim3(grid), dim3(kSurfaceThreads), 0, st, a, s);
    return hipGetLastError();
}

// ---- occupancy ---------------------------------------------------------------------------------
int OccupancyCache::get(Family f, const Variant& v, size_t smem) {
    Entry& c = e[(int)f][v.slot()];
    if (c.blocks != 0 && c.smem == smem) return c.blocks;
    const Policy& p = policy(v.math);
    const void* fn = nullptr;
    int threads = 256;
    switch (f) {
        case Family::Entry: fn = reinterpret_cast<const void*>(p.entry(v)); break;
        case Family::WfExtend: fn = reinterpret_cast<const void*>(p.wavefront(v).extend), threads = kWfExtendThreads; break;
        case Family::WfShade: fn = reinterpret_cast<const void*>(p.wavefront(v).shade), threads = kWfShadeThreads; break;
        case Family::Query: fn = reinterpret_cast<const void*>(p.query(v)), threads = kQueryThreads; break;
        case Family::Trace: fn = reinterpret_cast<const void*>(p.trace(v)), threads = kTraceThreads; break;
        case Family::Sample: fn = reinterpret_cast<const void*>(p.sample(v)), threads = kTraceThreads; break;
        case Family::Motion: fn = reinterpret_cast<const void*>(p.motion(v)), threads = kQueryThreads; break;
    }
    int blocks = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, fn, threads, smem) != hipSuccess) blocks = 1;
    c = Entry{blocks > 0 ? blocks : 1, smem};
    return c.blocks;
}

// rtDiagPinnedMath: the pinned policy's builtins, element-wise (tests)
__global__ void pinned_math_kernel(int op, const float* __restrict__ a, const float* __restrict__ b,
                                   float* __restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = a[i];
    float r;
    switch (op) {
        case 0: r = MathPinned::rcp(x); break;
        case 1: r = MathPinned::div(x, b[i]); break;
        case 2: r = MathPinned::sqrt(x); break;
        case 3: r = MathPinned::rsqrt(x); break;
        case 4: r = MathPinned::pow(x, b[i]); break;
        case 5: r = MathPinned::sin(x); break;
        default: r = MathPinned::cos(x); break;
    }
    out[i] = r;
}

hipError_t launch_gamma_check(const GammaCheckArgs& g, int math, hipStream_t st) {
    // grid-stride: a fixed grid whatever the count
    if (g.count) hipLaunchKernelGGL(policy(math).gamma_check, dim3(256u * 8u), dim3(256), 0, st, g);
    return hipGetLastError();
}

hipError_t launch_pinned_math(int op, const float* a, const float* b, float* out, size_t n, hipStream_t st) {
    if (n) hipLaunchKernelGGL(pinned_math_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, op, a, b, out, n);
    return hipGetLastError();
}

hipError_t launch_pack(const rt_cl_triangle* tris, uint32_t n_tris, float4* pt, float4* ps,
                       const rt_cl_material* mats, uint32_t n_mats, float4* pm, hipStream_t st) {
    if (n_tris) hipLaunchKernelGGL(pack_tris, dim3((n_tris + 255) / 256), dim3(256), 0, st, tris, pt, n_tris);
    if (n_tris) hipLaunchKernelGGL(pack_shade, dim3((n_tris + 255) / 256), dim3(256), 0, st, tris, ps, n_tris);
    if (n_mats) hipLaunchKernelGGL(pack_mats, dim3((n_mats + 255) / 256), dim3(256), 0, st, mats, pm, n_mats);
    // the shipped policy's material records (2.5-ulp divisions) follow the IEEE ones
    if (n_mats)
        hipLaunchKernelGGL(shipped_policy().pack_mats, dim3((n_mats + 255) / 256), dim3(256), 0, st, mats,
                           pm + 4 * (size_t)n_mats, n_mats);
    return hipGetLastError();
}

}  // namespace rtk


// rt_kernels_shipped.hip -- KernelEntry under the MathShipped policy: the reference kernel as
// the AMD OpenCL compiler builds it by default (clBuildProgram(" -I . "), CLutils.cpp:52-66).
//
// The policy spells out every reference `/` and sqrt as the backend's OpenCL-accuracy
// expansions (MathShipped::rcp/div/sqrt) and every fp-contract=on fusion as an fma at the
// reference's expression site (madd, rt_math.hpp).  This TU is also compiled with
// -fno-hip-fp32-correctly-rounded-divide-sqrt, so any division left to the compiler gets the
// same OpenCL accuracy instead of the HIP default.  Only MathShipped is instantiated here, and
// the TU exports one thing: shipped_policy(), the table of its kernels (rt_kernels.hpp).
#include "rt_kernel_pick.hpp"

#pragma clang fp contract(off)

namespace rtk {

// LDS-resident scenes run 5 waves per SIMD (VALU-bound); scenes read from HBM/L2 run 6 (load
// latency to hide: bunny proxy -2.4 %, profiles/r01/global_path_waves_ab.txt)
template <bool kStats, bool kBofs, int kMode>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_STEP_DEVICELIB_WAVES, 8)))
void kernel_entry_step_shipped_lds(KernelArgs a) {
    step_body<MathShipped, true, kStats, kBofs, false, kMode>(a);
}
template <bool kStats, int kMode>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_STEP_GLOBAL_WAVES, 8)))
void kernel_entry_step_shipped_global(KernelArgs a) {
    step_body<MathShipped, false, kStats, false, false, kMode>(a);
}
// octant records read from HBM/L2 (scenes too large for LDS): the LDS path's walk
template <bool kStats, int kMode>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(RT_STEP_GOCT_WAVES, 8)))
void kernel_entry_step_shipped_goct(KernelArgs a) {
    step_body<MathShipped, true, kStats, false, true, kMode>(a);
}

__global__ void pack_mats_shipped(const rt_cl_material* __restrict__ in, float4* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    material_record<MathShipped>(in[i], out + 4 * i);
}

__global__ __launch_bounds__(256) RT_ACCUM_OCC void accum_frames_shipped(KernelArgs a, const uint32_t* key) {
    accum_frames_body<MathShipped>(a, key);
}
__global__ void accum_key_shipped(KernelArgs a, uint32_t* key) {
    accum_key_body<MathShipped>(a, key);
}
__global__ __launch_bounds__(256) void gamma_check_shipped(GammaCheckArgs g) { gamma_check_body<MathShipped>(g); }

template <>
struct StepEntry<MathShipped> {
    template <bool S, int kMode>
    static KernelFn get(Walk w) {
        switch (w) {
            case Walk::Lds: return kernel_entry_step_shipped_lds<S, false, kMode>;
            case Walk::LdsB: return kernel_entry_step_shipped_lds<S, true, kMode>;
            case Walk::GlobalOct: return kernel_entry_step_shipped_goct<S, kMode>;
            default: return kernel_entry_step_shipped_global<S, kMode>;
        }
    }
};

const Policy& shipped_policy() {
    static const Policy shipped = {pick_entry<MathShipped>, wf_pick<MathShipped>, query_pick<MathShipped>,
                                   accum_frames_shipped,    accum_key_shipped,    camera_rays<MathShipped>,
                                   pack_mats_shipped,
                                   hit_surfaces<MathShipped, false>, hit_surfaces<MathShipped, true>,
                                   trace_pick<MathShipped>, camera_paths<MathShipped>,
                                   camera_paths_for<MathShipped>, sample_pick<MathShipped>,
                                   motion_pick<MathShipped>, gamma_check_shipped};
    return shipped;
}

}  // namespace rtk

// rt_launch_args.hpp -- a render launch's arguments as a value: the 14 slots of rtSetKernelArg
// (cl::Kernel::setArg, CLRaytracer.cpp:137-150) and the per-frame launches held back for coalescing.
// A launch reads its slots from the LaunchArgs it is handed, never from the kernel object, so the
// frames of a held run launch with the copy taken when they were enqueued and a launch never writes
// the kernel's slots.  Pure host code: no HIP header (tests/test_held_frames.py builds it with g++).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <initializer_list>

#include "../../include/rt_hip.h"

namespace rti {

struct LaunchArgs {
    bool set[RT_ARG_COUNT] = {};
    rt_mem bufs[4] = {};              // slots 0..3
    uint32_t u32[RT_ARG_COUNT] = {};  // slots 4..10 (raw 4-byte values)
    float f3[3][4] = {};              // slots 11..13

    bool has(std::initializer_list<int> slots) const {
        for (int i : slots)
            if (!set[i]) return false;
        return true;
    }
    bool complete() const {
        for (bool s : set)
            if (!s) return false;
        return true;
    }
    rt_mem out() const { return bufs[RT_ARG_BUFFER_OUT]; }
    rt_mem tris() const { return bufs[RT_ARG_BUFFER_SCENE]; }
    rt_mem nodes() const { return bufs[RT_ARG_BUFFER_NODE]; }
    rt_mem materials() const { return bufs[RT_ARG_BUFFER_MATERIAL]; }
    uint32_t width() const { return u32[RT_ARG_WIDTH]; }
    uint32_t height() const { return u32[RT_ARG_HEIGHT]; }
    uint32_t frame_count() const { return u32[RT_ARG_FRAME_COUNT]; }
    int32_t light_bounces() const { return as<int32_t>(RT_ARG_LIGHT_BOUNCES); }
    int32_t light_type() const { return as<int32_t>(RT_ARG_LIGHT_TYPE); }
    float skybox_intensity() const { return as<float>(RT_ARG_SKYBOX_INTENSITY); }

    // every slot a launch reads holds the same bits (FRAME_COUNT is the frame, which the caller
    // compares; FRAME_SEED is never read by KernelEntry, kernel_bvh.cl:415-456)
    bool same_but_frame(const LaunchArgs& o) const {
        for (int i = RT_ARG_WIDTH; i < RT_ARG_CAMERA_POS; ++i)
            if (i != RT_ARG_FRAME_COUNT && i != RT_ARG_FRAME_SEED && u32[i] != o.u32[i]) return false;
        return std::memcmp(f3, o.f3, sizeof(f3)) == 0 && std::memcmp(bufs, o.bufs, sizeof(bufs)) == 0;
    }

private:
    template <class T>
    T as(int slot) const {
        T v;
        std::memcpy(&v, &u32[slot], 4);
        return v;
    }
};

// Per-frame launches queued back to back and not launched yet (rtEnqueueKernel, frame coalescing):
// frames f0 .. f0 + n - 1 of `k` over `gws` work-items, with the arguments they were enqueued with.
// Nothing is held while k is null.
struct HeldFrames {
    rt_kernel k = nullptr;
    size_t gws = 0;
    uint32_t f0 = 0, n = 0;
    LaunchArgs args;

    // frame `f` of (kernel, gws, a) is the next frame of this run, which holds fewer than `batch`
    // frames.  Frame 0 starts a chain (it ignores the stored image), so it never continues one --
    // f0 + n wrapping to 0 included.
    bool continues(rt_kernel kernel, size_t work, const LaunchArgs& a, uint32_t f, uint32_t batch) const {
        return k != nullptr && k == kernel && gws == work && n < batch && f == f0 + n && f != 0u &&
               args.same_but_frame(a);
    }
    // the run, taken out: nothing is held afterwards
    HeldFrames take() {
        const HeldFrames h = *this;
        k = nullptr;
        return h;
    }
};

}  // namespace rti

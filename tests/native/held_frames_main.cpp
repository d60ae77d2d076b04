// held_frames_main.cpp -- stand-alone driver of the frame-coalescing rule (csrc/rt_launch_args.hpp:
// rti::HeldFrames::continues), CPU only; built by tests/test_held_frames.py with plain g++ and once
// more with -fsanitize=address,undefined.  Prints one line per case, "NAME 0" or "NAME 1": whether the
// frame continues the held run.  The expected answers are in the test, not here.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../mini-opencl-raytracer_amd/csrc/rt_launch_args.hpp"

namespace {

// handles are opaque here: distinct addresses are all the rule looks at
char g_objects[8];
rt_kernel kernel(int i) { return reinterpret_cast<rt_kernel>(&g_objects[i]); }
rt_mem mem(int i) { return reinterpret_cast<rt_mem>(&g_objects[2 + i]); }

rti::LaunchArgs base_args() {
    rti::LaunchArgs a;
    for (int i = 0; i < RT_ARG_COUNT; ++i) a.set[i] = true;
    for (int i = 0; i < 4; ++i) a.bufs[i] = mem(i);
    for (int i = RT_ARG_WIDTH; i <= RT_ARG_SKYBOX_INTENSITY; ++i) a.u32[i] = 100u + (uint32_t)i;
    for (int s = 0; s < 3; ++s)
        for (int c = 0; c < 4; ++c) a.f3[s][c] = 1.0f + (float)(4 * s + c);
    return a;
}

constexpr size_t kGws = 4096;

// a run of `n` frames from `f0`, held with base_args()
rti::HeldFrames run(uint32_t f0, uint32_t n) {
    rti::LaunchArgs a = base_args();
    a.u32[RT_ARG_FRAME_COUNT] = f0;
    return rti::HeldFrames{kernel(0), kGws, f0, n, a};
}

void say(const char* name, bool continues) { std::printf("%s %d\n", name, continues ? 1 : 0); }
void say(const char* name, int i, bool continues) { std::printf("%s%d %d\n", name, i, continues ? 1 : 0); }

}  // namespace

int main() {
    const rti::LaunchArgs a = base_args();

    // a run of 1 at batch 2 continues once and not twice
    rti::HeldFrames h = run(5, 1);
    say("batch2_first", h.continues(kernel(0), kGws, a, 6, 2));
    ++h.n;
    say("batch2_second", h.continues(kernel(0), kGws, a, 7, 2));
    say("batch1", run(5, 1).continues(kernel(0), kGws, a, 6, 1));
    say("batch8_full", run(5, 8).continues(kernel(0), kGws, a, 13, 8));
    say("batch8_last", run(5, 7).continues(kernel(0), kGws, a, 12, 8));

    // the frame number
    say("wrap_to_zero", run(0xffffffffu, 1).continues(kernel(0), kGws, a, 0, 8));
    say("wrap_past_zero", run(0xfffffffeu, 1).continues(kernel(0), kGws, a, 0xffffffffu, 8));
    say("from_zero", run(0, 1).continues(kernel(0), kGws, a, 1, 8));
    say("gap", run(5, 1).continues(kernel(0), kGws, a, 7, 8));
    say("repeat", run(5, 1).continues(kernel(0), kGws, a, 5, 8));
    say("back", run(5, 1).continues(kernel(0), kGws, a, 4, 8));

    // nothing held; another kernel; another work size
    say("nothing_held", rti::HeldFrames{}.continues(kernel(0), 0, rti::LaunchArgs{}, 0, 8));
    say("nothing_held_next", rti::HeldFrames{}.continues(nullptr, 0, rti::LaunchArgs{}, 1, 8));
    say("other_kernel", run(5, 1).continues(kernel(1), kGws, a, 6, 8));
    say("other_gws", run(5, 1).continues(kernel(0), kGws + 1, a, 6, 8));

    // every slot changed alone
    for (int i = 0; i < 4; ++i) {
        rti::LaunchArgs b = a;
        b.bufs[i] = mem(4);
        say("buf", i, run(5, 1).continues(kernel(0), kGws, b, 6, 8));
    }
    for (int i = RT_ARG_WIDTH; i <= RT_ARG_SKYBOX_INTENSITY; ++i) {
        rti::LaunchArgs b = a;
        b.u32[i] ^= 1u;
        say("u32_", i, run(5, 1).continues(kernel(0), kGws, b, 6, 8));
    }
    for (int s = 0; s < 3; ++s)
        for (int c = 0; c < 4; ++c) {
            rti::LaunchArgs b = a;
            b.f3[s][c] += 0.5f;
            say("cam", 4 * s + c, run(5, 1).continues(kernel(0), kGws, b, 6, 8));
        }
    // bits, not values: -0.0f is another camera
    {
        rti::HeldFrames z = run(5, 1);
        z.args.f3[0][0] = 0.0f;
        rti::LaunchArgs b = z.args;
        b.f3[0][0] = -0.0f;
        say("cam_negative_zero", z.continues(kernel(0), kGws, b, 6, 8));
    }

    // take() empties the run and hands it out whole
    rti::HeldFrames t = run(9, 3);
    const rti::HeldFrames got = t.take();
    say("taken_is_empty", t.k == nullptr && !t.continues(kernel(0), kGws, a, 12, 8));
    say("taken_is_whole", got.k == kernel(0) && got.gws == kGws && got.f0 == 9 && got.n == 3 &&
                              got.args.frame_count() == 9 && got.continues(kernel(0), kGws, a, 12, 8));

    // the typed readers
    rti::LaunchArgs r = a;
    const int32_t bounces = -3;
    const float sky = 0.75f;
    std::memcpy(&r.u32[RT_ARG_LIGHT_BOUNCES], &bounces, 4);
    std::memcpy(&r.u32[RT_ARG_SKYBOX_INTENSITY], &sky, 4);
    say("readers", r.light_bounces() == -3 && r.skybox_intensity() == 0.75f && r.width() == 100u + RT_ARG_WIDTH &&
                       r.height() == 100u + RT_ARG_HEIGHT && r.light_type() == 100 + RT_ARG_LIGHT_TYPE &&
                       r.out() == mem(0) && r.tris() == mem(1) && r.nodes() == mem(2) && r.materials() == mem(3));
    rti::LaunchArgs partial;
    partial.set[RT_ARG_WIDTH] = true;
    say("has_some", partial.has({RT_ARG_WIDTH}) && !partial.has({RT_ARG_WIDTH, RT_ARG_HEIGHT}) && !partial.complete() &&
                        a.complete());
    return 0;
}

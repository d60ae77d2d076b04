// denoise_plan_main.cpp -- stand-alone driver of the denoise plan (csrc/rt_denoise_plan.cpp denoise_plan), CPU only.
//   denoise_plan_main sweep   plans a sweep of image sizes and iteration counts and checks on every plan: each
//                             iteration reads what the one before wrote (the first the image), never writes what
//                             it reads, and the last writes `out`; the scratch is asked for exactly when used; the
//                             staged block is within the LDS budget; walking every lane of every workgroup of the
//                             grid as rt_denoise.hip maps them, every pixel is filtered by exactly one lane and each
//                             of its 25 taps lies in a staged cell that holds the tap's coordinates.  Sizes too
//                             large to walk are checked by their counts.
//   denoise_plan_main errors  the error rows of rtEnqueueDenoise (rt_hip.h) return their codes, in order.
// Exit status 1 if anything breaks.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <vector>

#include "../../include/rt_status.h"
#include "../../mini-opencl-raytracer_amd/csrc/rt_denoise_plan.hpp"
#include "image_pass_common.hpp"

static rtp::DenoiseIn base_in() {
    rtp::DenoiseIn in{};
    in.params_ok = true;
    in.iterations = 3;
    in.sigma_color = 4.0f, in.sigma_normal = 0.5f, in.sigma_depth = 0.1f, in.sigma_albedo = 0.25f;
    in.width = 131, in.height = 77;
    in.image_ok = in.features_ok = in.out_ok = true;
    in.image_bytes = in.out_bytes = 131 * 77 * 16, in.features_bytes = 131 * 77 * 32;
    return in;
}

static rtp::DenoiseIn sized(uint64_t w, uint64_t h, unsigned n) {
    rtp::DenoiseIn in = base_in();
    in.width = w, in.height = h, in.iterations = n;
    in.image_bytes = in.out_bytes = w * h * 16, in.features_bytes = w * h * 32;
    return in;
}

static bool check_plan(const rtp::DenoiseIn& in, const rtp::DenoisePlan& p, bool walk_it, std::vector<uint8_t>& seen) {
    const uint64_t W = in.width, H = in.height;
    if (p.iterations != in.iterations || p.width != W || p.height != H) return std::printf("sizes\n"), false;
    bool scratch_used = false;
    for (unsigned i = 0; i < p.iterations; ++i) {
        const rtp::DenoiseStep& t = p.it[i];
        if (t.step != 1u << i) return std::printf("step\n"), false;
        if (t.src != (i == 0 ? (int)rtp::kDenoiseImage : p.it[i - 1].dst)) return std::printf("src\n"), false;
        if (t.dst == t.src || t.dst == rtp::kDenoiseImage) return std::printf("dst\n"), false;
        if (t.dst != ((p.iterations - 1 - i) % 2 == 0 ? rtp::kDenoiseOut : rtp::kDenoiseScratch)) return std::printf("parity\n"), false;
        scratch_used = scratch_used || t.dst == rtp::kDenoiseScratch;
        if (t.rows == 0 || rtp::kDenoiseThreads % rtp::kDenoiseTileW) return std::printf("rows\n"), false;
        if (t.stage_w != rtp::kDenoiseTileW + 4 * t.step || t.stage_h != t.rows + 4) return std::printf("stage\n"), false;
        if (t.lds_bytes != t.stage_w * t.stage_h * rtp::kDenoiseCellBytes + rtp::kDenoisePadBytes ||
            t.lds_bytes > rtp::kDenoiseLdsBudget)
            return std::printf("lds %u\n", t.lds_bytes), false;
        // counts: the columns, the classes, and the longest class's rows are covered, with no spare tile
        if ((uint64_t)t.tiles_x * rtp::kDenoiseTileW < W || (uint64_t)(t.tiles_x - 1) * rtp::kDenoiseTileW >= W)
            return std::printf("tiles_x\n"), false;
        if (t.classes != (H < t.step ? H : t.step)) return std::printf("classes\n"), false;
        const uint64_t class_rows = (H + t.step - 1) / t.step;
        if ((uint64_t)t.tiles_per_class * t.rows < class_rows || (uint64_t)(t.tiles_per_class - 1) * t.rows >= class_rows)
            return std::printf("tiles_per_class\n"), false;
        const uint64_t grid = (uint64_t)t.tiles_x * t.classes * t.tiles_per_class;
        if (grid == 0 || grid >= (1ull << 31) || t.grid != grid) return std::printf("grid\n"), false;
        if (walk_it && !walk(t, W, H, seen)) return false;
    }
    if (p.it[p.iterations - 1].dst != rtp::kDenoiseOut) return std::printf("last\n"), false;
    if (p.scratch_pixels != (scratch_used ? W * H : 0)) return std::printf("scratch\n"), false;
    if (scratch_used != (p.iterations >= 2)) return std::printf("scratch use\n"), false;
    return true;
}

static int sweep() {
    static const uint64_t widths[] = {1, 2, 5, 40, 61, 63, 64, 65, 127, 128, 131, 200};
    static const uint64_t heights[] = {1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 33, 64, 77, 129, 200};
    static const uint64_t big[][2] = {{3840, 2160}, {1ull << 31, 1}, {1, 1ull << 31}, {65536, 32768}, {46340, 46340},
                                      {(1ull << 31) / 3, 3}, {3, (1ull << 31) / 3}, {1ull << 20, 1ull << 11}};
    unsigned long long plans = 0, failures = 0;
    std::vector<uint8_t> seen;
    auto one = [&](uint64_t w, uint64_t h, unsigned n, bool walk_it) {
        const rtp::DenoiseIn in = sized(w, h, n);
        rtp::DenoisePlan p;
        const int rc = rtp::denoise_plan(in, &p);
        ++plans;
        if ((rc != RT_SUCCESS || !check_plan(in, p, walk_it, seen)) && ++failures <= 20)
            std::printf("broken: %llu x %llu, %u iterations: rc %d\n", (unsigned long long)w, (unsigned long long)h, n, rc);
    };
    for (uint64_t w : widths)
        for (uint64_t h : heights)
            for (unsigned n = 1; n <= rtp::kDenoiseMaxIterations; ++n) one(w, h, n, n == rtp::kDenoiseMaxIterations);
    for (auto& wh : big)
        for (unsigned n = 1; n <= rtp::kDenoiseMaxIterations; ++n) one(wh[0], wh[1], n, false);
    std::printf("sweep: %llu plans, %llu failures\n", plans, failures);
    return failures ? 1 : 0;
}

// the documented order, spelled independently of the plan
static int expected(const rtp::DenoiseIn& in) {
    if (!in.params_ok || in.iterations < 1 || in.iterations > 5) return RT_INVALID_VALUE;
    for (float s : {in.sigma_color, in.sigma_normal, in.sigma_depth, in.sigma_albedo})
        if (!(s == 0.0f || (s >= 0x1p-20f && s <= 0x1p20f))) return RT_INVALID_VALUE;  // (false for a NaN)
    const unsigned __int128 pixels = (unsigned __int128)in.width * in.height;
    if (pixels == 0 || pixels > ((unsigned __int128)1 << 31)) return RT_INVALID_VALUE;
    if (!in.image_ok || !in.features_ok || !in.out_ok || in.out_is_input) return RT_INVALID_MEM_OBJECT;
    if (pixels * 16 > in.image_bytes || pixels * 32 > in.features_bytes || pixels * 16 > in.out_bytes)
        return RT_INVALID_BUFFER_SIZE;
    return RT_SUCCESS;
}

static int errors() {
    int failures = 0;
    auto expect = [&](const char* name, const rtp::DenoiseIn& in, int want) {
        rtp::DenoisePlan p;
        const int rc = rtp::denoise_plan(in, &p);
        const bool ok = rc == want && expected(in) == want;
        std::printf("%s %s: rc %d (want %d, restated %d)\n", ok ? "ok    " : "FAILED", name, rc, want, expected(in));
        if (!ok) ++failures;
    };
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    rtp::DenoiseIn in = base_in();
    expect("valid", in, RT_SUCCESS);
    in = base_in(), in.params_ok = false;
    expect("params_null", in, RT_INVALID_VALUE);
    in = base_in(), in.iterations = 0;
    expect("iterations_zero", in, RT_INVALID_VALUE);
    in = base_in(), in.iterations = 6;
    expect("iterations_six", in, RT_INVALID_VALUE);
    in = base_in(), in.iterations = 5;
    expect("iterations_five", in, RT_SUCCESS);
    in = base_in(), in.sigma_color = -1.0f;
    expect("sigma_negative", in, RT_INVALID_VALUE);
    in = base_in(), in.sigma_normal = nan;
    expect("sigma_nan", in, RT_INVALID_VALUE);
    in = base_in(), in.sigma_depth = inf;
    expect("sigma_infinite", in, RT_INVALID_VALUE);
    in = base_in(), in.sigma_albedo = 0x1p-21f;
    expect("sigma_tiny", in, RT_INVALID_VALUE);
    in = base_in(), in.sigma_albedo = 0x1p-20f;
    expect("sigma_smallest", in, RT_SUCCESS);
    in = base_in(), in.sigma_color = 0x1.000002p20f;
    expect("sigma_huge", in, RT_INVALID_VALUE);
    in = base_in(), in.sigma_color = 0x1p20f;
    expect("sigma_largest", in, RT_SUCCESS);
    in = base_in(), in.sigma_color = in.sigma_normal = in.sigma_depth = in.sigma_albedo = 0.0f;
    expect("sigmas_all_zero", in, RT_SUCCESS);
    in = base_in(), in.sigma_depth = -0.0f;
    expect("sigma_minus_zero", in, RT_SUCCESS);
    in = base_in(), in.width = 0;
    expect("width_zero", in, RT_INVALID_VALUE);
    in = base_in(), in.height = 0;
    expect("height_zero", in, RT_INVALID_VALUE);
    in = sized(65536, 32768 + 1, 1);
    expect("past_2_31", in, RT_INVALID_VALUE);
    in = sized(0xffffffffull, 0xffffffffull, 1), in.image_bytes = in.out_bytes = in.features_bytes = ~0ull;
    expect("product_near_2_64", in, RT_INVALID_VALUE);
    in = sized(65536, 32768, 1);
    expect("exactly_2_31", in, RT_SUCCESS);
    in = base_in(), in.image_ok = false, in.image_bytes = 0;
    expect("image_null", in, RT_INVALID_MEM_OBJECT);
    in = base_in(), in.features_ok = false, in.features_bytes = 0;
    expect("features_null", in, RT_INVALID_MEM_OBJECT);
    in = base_in(), in.out_ok = false, in.out_bytes = 0;
    expect("out_null", in, RT_INVALID_MEM_OBJECT);
    in = base_in(), in.out_is_input = true;
    expect("out_is_an_input", in, RT_INVALID_MEM_OBJECT);
    in = base_in(), in.image_bytes -= 1;
    expect("image_short", in, RT_INVALID_BUFFER_SIZE);
    in = base_in(), in.features_bytes -= 1;
    expect("features_short", in, RT_INVALID_BUFFER_SIZE);
    in = base_in(), in.out_bytes -= 1;
    expect("out_short", in, RT_INVALID_BUFFER_SIZE);
    // the order: the earlier row wins
    in = base_in(), in.iterations = 0, in.out_ok = false, in.image_bytes = 1;
    expect("value_before_mem_object", in, RT_INVALID_VALUE);
    in = base_in(), in.sigma_color = -1.0f, in.out_is_input = true;
    expect("sigma_before_mem_object", in, RT_INVALID_VALUE);
    in = base_in(), in.width = 0, in.image_bytes = 0;
    expect("size_zero_before_buffer_size", in, RT_INVALID_VALUE);
    in = base_in(), in.out_is_input = true, in.out_bytes = 1;
    expect("mem_object_before_size", in, RT_INVALID_MEM_OBJECT);
    // the constants
    in = base_in(), in.iterations = 5;
    rtp::DenoisePlan p;
    bool ok = rtp::denoise_plan(in, &p) == RT_SUCCESS && p.terms == 15 && p.inv_n == 1.0f / (0.5f * 0.5f) &&
              p.inv_z == 1.0f / (0.1f * 0.1f) && p.inv_a == 1.0f / (0.25f * 0.25f);
    for (int i = 0; ok && i < 5; ++i) {
        const float s = std::ldexp(4.0f, -i);
        ok = p.it[i].inv_c == 1.0f / (s * s);
    }
    in.sigma_color = 0.0f, in.sigma_depth = 0.0f;
    ok = ok && rtp::denoise_plan(in, &p) == RT_SUCCESS && p.terms == (rtp::kDenoiseNormal | rtp::kDenoiseAlbedo);
    in = base_in(), in.iterations = 5, in.sigma_color = 0x1p-20f;
    ok = ok && rtp::denoise_plan(in, &p) == RT_SUCCESS && std::isfinite(p.it[4].inv_c) && p.it[4].inv_c == 0x1p48f;
    std::printf("%s constants\n", ok ? "ok    " : "FAILED");
    if (!ok) ++failures;
    return failures ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && std::strcmp(argv[1], "sweep") == 0) return sweep();
    if (argc == 2 && std::strcmp(argv[1], "errors") == 0) return errors();
    std::fprintf(stderr, "usage: denoise_plan_main sweep|errors\n");
    return 2;
}

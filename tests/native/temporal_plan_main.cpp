// temporal_plan_main.cpp -- stand-alone driver of the temporal reprojection's host side, CPU only:
// the plan (csrc/rt_temporal_plan.cpp temporal_plan) and the address logic the kernel compiles
// (csrc/rt_temporal_math.hpp, the same text).
//   temporal_plan_main errors  the error rows of rtEnqueueTemporalAccumulate (rt_hip.h) return their codes, in
//                              order, and the plan's constants are the definition's.
//   temporal_plan_main sweep   calls reproject() / tap_index() over images from 1 x 1 to 4096 x 2160 (and the
//                              widest the plan admits), ordinary, degenerate and extreme cameras, and
//                              adversarial depths: +-0, denormals, +-FLT_MAX, +-inf, NaN, depths that put the point
//                              on or behind the previous camera's plane, and depths found by bisection that put
//                              fx within a few ulps of -1, 0, W - 1 and W.  On every call: a reprojection that
//                              passed has x0 in [-1, W - 1], y0 in [-1, H - 1] and weights in [0, 1], and its
//                              projection lies in the tested range (so the float -> int conversion was in range;
//                              a build with -fsanitize=float-cast-overflow checks the same); every tap reported
//                              inside indexes inside W * H, at its own coordinates; one that did not pass
//                              reports no tap.
// Exit status 1 if anything breaks.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/rt_status.h"
#include "../../mini-opencl-raytracer_amd/csrc/rt_temporal_plan.hpp"
#include "image_pass_common.hpp"

static rtp::TemporalIn sized(uint64_t w, uint64_t h) {
    rtp::TemporalIn in{};
    in.params_ok = true;
    in.width = w, in.height = h;
    in.cur = in.prev = kDefaultView;
    in.cur_frames = 8.0f, in.history_frames = 0.0f, in.max_history = 32.0f;
    in.depth_tolerance = 0.05f, in.normal_threshold = 0.9f;
    in.hist_given = in.hist_features_given = true;
    in.cur_ok = in.cur_features_ok = in.out_ok = in.hist_ok = in.hist_features_ok = true;
    in.cur_bytes = in.hist_bytes = in.out_bytes = w * h * 16;
    in.cur_features_bytes = in.hist_features_bytes = w * h * 32;
    return in;
}

static rtp::TemporalIn base_in() { return sized(131, 77); }

// ---- errors -------------------------------------------------------------------------------------

// the documented order, spelled independently of the plan
static int expected(const rtp::TemporalIn& in) {
    if (!in.params_ok) return RT_INVALID_VALUE;
    const unsigned __int128 pixels = (unsigned __int128)in.width * in.height;
    if (pixels == 0 || pixels > ((unsigned __int128)1 << 31)) return RT_INVALID_VALUE;
    if (!finite_view(in.cur) || !finite_view(in.prev)) return RT_INVALID_VALUE;
    if (!(in.cur_frames >= 1.0f && in.cur_frames <= 0x1p20f)) return RT_INVALID_VALUE;  // (false for a NaN)
    if (!(in.history_frames == 0.0f || (in.history_frames >= 1.0f && in.history_frames <= 0x1p20f))) return RT_INVALID_VALUE;
    if (!(in.max_history >= in.cur_frames && in.max_history <= 0x1p20f)) return RT_INVALID_VALUE;
    if (!(in.depth_tolerance >= 0.0f && in.depth_tolerance <= 1.0f)) return RT_INVALID_VALUE;
    if (!(in.normal_threshold >= -1.0f && in.normal_threshold <= 1.0f)) return RT_INVALID_VALUE;
    if (in.hist_given != in.hist_features_given) return RT_INVALID_MEM_OBJECT;
    if (!in.cur_ok || !in.cur_features_ok || !in.out_ok) return RT_INVALID_MEM_OBJECT;
    if (in.hist_given && (!in.hist_ok || !in.hist_features_ok)) return RT_INVALID_MEM_OBJECT;
    if (in.out_is_input) return RT_INVALID_MEM_OBJECT;
    if (pixels * 16 > in.cur_bytes || pixels * 32 > in.cur_features_bytes || pixels * 16 > in.out_bytes)
        return RT_INVALID_BUFFER_SIZE;
    if (in.hist_given && (pixels * 16 > in.hist_bytes || pixels * 32 > in.hist_features_bytes)) return RT_INVALID_BUFFER_SIZE;
    return RT_SUCCESS;
}

static int errors() {
    int failures = 0;
    auto expect = [&](const char* name, const rtp::TemporalIn& in, int want) {
        rtp::TemporalPlan p;
        const int rc = rtp::temporal_plan(in, &p);
        const bool ok = rc == want && expected(in) == want;
        std::printf("%s %s: rc %d (want %d, restated %d)\n", ok ? "ok    " : "FAILED", name, rc, want, expected(in));
        if (!ok) ++failures;
    };
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    rtp::TemporalIn in = base_in();
    expect("valid", in, RT_SUCCESS);
    in = base_in(), in.hist_given = in.hist_features_given = false, in.hist_ok = in.hist_features_ok = false;
    in.hist_bytes = in.hist_features_bytes = 0;
    expect("valid_without_history", in, RT_SUCCESS);
    in = base_in(), in.params_ok = false;
    expect("params_null", in, RT_INVALID_VALUE);
    in = base_in(), in.width = 0;
    expect("width_zero", in, RT_INVALID_VALUE);
    in = base_in(), in.height = 0;
    expect("height_zero", in, RT_INVALID_VALUE);
    in = sized(65536, 32768 + 1);
    expect("past_2_31", in, RT_INVALID_VALUE);
    in = sized(0xffffffffull, 0xffffffffull), in.cur_bytes = in.hist_bytes = in.out_bytes = ~0ull;
    in.cur_features_bytes = in.hist_features_bytes = ~0ull;
    expect("product_near_2_64", in, RT_INVALID_VALUE);
    in = sized(65536, 32768);
    expect("exactly_2_31", in, RT_SUCCESS);
    in = base_in(), in.cur.pos[1] = nan;
    expect("camera_nan", in, RT_INVALID_VALUE);
    in = base_in(), in.prev.up[2] = inf;
    expect("camera_infinite", in, RT_INVALID_VALUE);
    in = base_in(), in.cur.front[0] = -inf;
    expect("camera_front_infinite", in, RT_INVALID_VALUE);
    in = base_in(), in.cur_frames = nan;
    expect("cur_frames_nan", in, RT_INVALID_VALUE);
    in = base_in(), in.cur_frames = 0.5f;
    expect("cur_frames_below_one", in, RT_INVALID_VALUE);
    in = base_in(), in.cur_frames = 0x1.000002p20f, in.max_history = 0x1.000002p20f;
    expect("cur_frames_huge", in, RT_INVALID_VALUE);
    in = base_in(), in.cur_frames = 0x1p20f, in.max_history = 0x1p20f;
    expect("cur_frames_largest", in, RT_SUCCESS);
    in = base_in(), in.history_frames = -1.0f;
    expect("history_frames_negative", in, RT_INVALID_VALUE);
    in = base_in(), in.history_frames = inf;
    expect("history_frames_infinite", in, RT_INVALID_VALUE);
    in = base_in(), in.history_frames = nan;
    expect("history_frames_nan", in, RT_INVALID_VALUE);
    in = base_in(), in.history_frames = 0.5f;
    expect("history_frames_fraction", in, RT_INVALID_VALUE);
    in = base_in(), in.history_frames = 0x1.000002p20f;
    expect("history_frames_huge", in, RT_INVALID_VALUE);
    in = base_in(), in.history_frames = 1.0f;
    expect("history_frames_one", in, RT_SUCCESS);
    in = base_in(), in.history_frames = -0.0f;
    expect("history_frames_minus_zero", in, RT_SUCCESS);
    in = base_in(), in.max_history = nan;
    expect("max_history_nan", in, RT_INVALID_VALUE);
    in = base_in(), in.max_history = 7.0f;
    expect("max_history_below_cur_frames", in, RT_INVALID_VALUE);
    in = base_in(), in.max_history = 0x1.000002p20f;
    expect("max_history_huge", in, RT_INVALID_VALUE);
    in = base_in(), in.max_history = 8.0f;
    expect("max_history_equals_cur_frames", in, RT_SUCCESS);
    in = base_in(), in.depth_tolerance = nan;
    expect("depth_tolerance_nan", in, RT_INVALID_VALUE);
    in = base_in(), in.depth_tolerance = -0.01f;
    expect("depth_tolerance_negative", in, RT_INVALID_VALUE);
    in = base_in(), in.depth_tolerance = 1.5f;
    expect("depth_tolerance_above_one", in, RT_INVALID_VALUE);
    in = base_in(), in.depth_tolerance = 0.0f;
    expect("depth_tolerance_zero", in, RT_SUCCESS);
    in = base_in(), in.normal_threshold = nan;
    expect("normal_threshold_nan", in, RT_INVALID_VALUE);
    in = base_in(), in.normal_threshold = -1.5f;
    expect("normal_threshold_below", in, RT_INVALID_VALUE);
    in = base_in(), in.normal_threshold = 1.5f;
    expect("normal_threshold_above", in, RT_INVALID_VALUE);
    in = base_in(), in.normal_threshold = -1.0f;
    expect("normal_threshold_lowest", in, RT_SUCCESS);
    in = base_in(), in.hist_features_given = false, in.hist_features_ok = false, in.hist_features_bytes = 0;
    expect("hist_without_features", in, RT_INVALID_MEM_OBJECT);
    in = base_in(), in.hist_given = false, in.hist_ok = false, in.hist_bytes = 0;
    expect("features_without_hist", in, RT_INVALID_MEM_OBJECT);
    in = base_in(), in.cur_ok = false, in.cur_bytes = 0;
    expect("cur_null", in, RT_INVALID_MEM_OBJECT);
    in = base_in(), in.cur_features_ok = false, in.cur_features_bytes = 0;
    expect("cur_features_null", in, RT_INVALID_MEM_OBJECT);
    in = base_in(), in.out_ok = false, in.out_bytes = 0;
    expect("out_null", in, RT_INVALID_MEM_OBJECT);
    in = base_in(), in.hist_ok = false, in.hist_bytes = 0;
    expect("hist_foreign", in, RT_INVALID_MEM_OBJECT);
    in = base_in(), in.hist_features_ok = false, in.hist_features_bytes = 0;
    expect("hist_features_foreign", in, RT_INVALID_MEM_OBJECT);
    in = base_in(), in.out_is_input = true;
    expect("out_is_an_input", in, RT_INVALID_MEM_OBJECT);
    in = base_in(), in.cur_bytes -= 1;
    expect("cur_short", in, RT_INVALID_BUFFER_SIZE);
    in = base_in(), in.cur_features_bytes -= 1;
    expect("cur_features_short", in, RT_INVALID_BUFFER_SIZE);
    in = base_in(), in.hist_bytes -= 1;
    expect("hist_short", in, RT_INVALID_BUFFER_SIZE);
    in = base_in(), in.hist_features_bytes -= 1;
    expect("hist_features_short", in, RT_INVALID_BUFFER_SIZE);
    in = base_in(), in.out_bytes -= 1;
    expect("out_short", in, RT_INVALID_BUFFER_SIZE);
    // the order: the earlier row wins
    in = base_in(), in.cur_frames = 0.0f, in.out_ok = false, in.cur_bytes = 1;
    expect("value_before_mem_object", in, RT_INVALID_VALUE);
    in = base_in(), in.normal_threshold = 2.0f, in.hist_given = false;
    expect("last_value_before_mem_object", in, RT_INVALID_VALUE);
    in = base_in(), in.width = 0, in.cur_bytes = 0;
    expect("size_zero_before_buffer_size", in, RT_INVALID_VALUE);
    in = base_in(), in.out_is_input = true, in.out_bytes = 1;
    expect("mem_object_before_size", in, RT_INVALID_MEM_OBJECT);
    in = base_in(), in.hist_given = false, in.hist_ok = false, in.cur_features_bytes = 1;
    expect("pairing_before_size", in, RT_INVALID_MEM_OBJECT);
    // the constants and the grid
    in = sized(61, 7);
    in.cur = {{0.37f, -25.0f, 8.6f}, {0.5f, 1.0f, 0.25f}, {0.0f, 0.25f, 1.0f}};
    rtp::TemporalPlan p;
    bool ok = rtp::temporal_plan(in, &p) == RT_SUCCESS;
    const rtt::TemporalConsts& k = p.k;
    const float A = 0x1.a82408p-2f;
    uint32_t abits;
    std::memcpy(&abits, &k.A, 4);
    ok = ok && abits == 0x3ED41204u && k.fW == 61.0f && k.fH == 7.0f && k.invW == 1.0f / 61.0f && k.invH == 1.0f / 7.0f &&
         k.asp == 61.0f / 7.0f && k.ia == 1.0f / (A * (61.0f / 7.0f)) && k.ib == 1.0f / A;
    ok = ok && k.cright[0] == 1.0f * 1.0f - 0.25f * 0.25f && k.cright[1] == 0.25f * 0.0f - 0.5f * 1.0f &&
         k.cright[2] == 0.5f * 0.25f - 1.0f * 0.0f;
    ok = ok && k.pright[0] == 1.0f && k.pright[1] == 0.0f && k.pright[2] == 0.0f && k.cpos[0] == 0.37f && k.ppos[1] == -25.0f;
    ok = ok && p.has_history && p.tiles_x == 1 && p.tiles_y == 2 && p.grid == 2 && p.cur_frames == 8.0f && p.max_history == 32.0f;
    in = sized(131, 77);
    ok = ok && rtp::temporal_plan(in, &p) == RT_SUCCESS && p.tiles_x == 3 && p.tiles_y == 20 && p.grid == 60;
    static const uint64_t widest[][2] = {{1ull << 31, 1}, {1, 1ull << 31}, {65536, 32768}};
    for (auto& wh : widest) {
        in = sized(wh[0], wh[1]);
        ok = ok && rtp::temporal_plan(in, &p) == RT_SUCCESS && p.grid > 0 && p.grid < (1u << 31) &&
             (uint64_t)p.tiles_x * rtp::kTemporalTileW >= wh[0] && (uint64_t)p.tiles_y * rtp::kTemporalTileH >= wh[1] &&
             (uint64_t)p.tiles_x * p.tiles_y == p.grid;
    }
    std::printf("%s constants\n", ok ? "ok    " : "FAILED");
    if (!ok) ++failures;
    return failures ? 1 : 0;
}

// ---- sweep --------------------------------------------------------------------------------------

struct Sweep {
    unsigned long long calls = 0, passed = 0, taps = 0, bracketed = 0, failures = 0;
    uint64_t W = 0, H = 0;
    rtt::TemporalConsts k{};

    void fail(const char* what, uint32_t x, uint32_t y, float depth) {
        if (++failures <= 20)
            std::printf("broken: %s at %llu x %llu, pixel (%u, %u), depth %a\n", what, (unsigned long long)W,
                        (unsigned long long)H, x, y, depth);
    }

    void one(uint32_t x, uint32_t y, float depth) {
        ++calls;
        const rtt::Projection pr = rtt::project(k, x, y, depth);
        const rtt::Reprojection r = rtt::reproject(k, x, y, depth);
        if (r.ok) {
            ++passed;
            // the conversion's operand was inside [-1, W): in range for an int32 (W <= 2^31)
            if (!(pr.zf > 0.0f && pr.fx > -1.0f && pr.fx < k.fW && pr.fy > -1.0f && pr.fy < k.fH && k.fW <= 0x1p31f && k.fH <= 0x1p31f))
                fail("passed outside the range", x, y, depth);
            if (r.x0 < -1 || (int64_t)r.x0 > (int64_t)W - 1 || r.y0 < -1 || (int64_t)r.y0 > (int64_t)H - 1)
                fail("x0 or y0 outside [-1, size - 1]", x, y, depth);
            if (!(r.tx >= 0.0f && r.tx <= 1.0f && r.ty >= 0.0f && r.ty <= 1.0f)) fail("tx or ty outside [0, 1]", x, y, depth);
        }
        int inside = 0;
        for (int j = 0; j < 2; ++j)
            for (int i = 0; i < 2; ++i) {
                uint64_t q = ~0ull;
                if (!rtt::tap_index(r, i, j, (uint32_t)W, (uint32_t)H, &q)) continue;
                ++inside, ++taps;
                if (!r.ok) fail("a tap of a reprojection that did not pass", x, y, depth);
                const int64_t qx = (int64_t)r.x0 + i, qy = (int64_t)r.y0 + j;
                if (q >= W * H || qx < 0 || qx >= (int64_t)W || qy < 0 || qy >= (int64_t)H || q != (uint64_t)qy * W + (uint64_t)qx)
                    fail("tap index outside the image", x, y, depth);
                const float bw = rtt::tap_weight(r, i, j);
                if (!(bw >= 0.0f && bw <= 1.0f)) fail("tap weight outside [0, 1]", x, y, depth);
            }
        // x0 in [-1, W - 1] leaves at least one column and one row of taps inside
        if (r.ok && inside == 0) fail("no tap inside after a pass", x, y, depth);
    }

    void around(uint32_t x, uint32_t y, float depth, int ulps) {
        uint32_t bits;
        std::memcpy(&bits, &depth, 4);
        for (int d = -ulps; d <= ulps; ++d) {
            const uint32_t b = bits + (uint32_t)d;
            float f;
            std::memcpy(&f, &b, 4);
            one(x, y, f);
        }
    }
};

static float from_bits(uint32_t b) {
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

static rtp::TemporalView yawed(float px, float py, float pz, double yaw) {
    return {{px, py, pz}, {(float)std::sin(yaw), (float)std::cos(yaw), 0.0f}, {0.0f, 0.0f, 1.0f}};
}

static int sweep() {
    static const uint64_t sizes[][2] = {{1, 1}, {2, 1}, {1, 2}, {5, 3}, {61, 7}, {64, 4}, {65, 5}, {131, 77}, {640, 360},
                                        {1920, 1080}, {4096, 2160}, {16777219, 1}, {1, 16777219}, {33554439, 3},
                                        {1ull << 31, 1}, {1, 1ull << 31}, {65536, 32768}};
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float dmin = std::numeric_limits<float>::denorm_min();
    const float depths[] = {0.0f, -0.0f, dmin, -dmin, 0x1p-140f, -0x1p-130f, FLT_MIN, -FLT_MIN, FLT_MAX, -FLT_MAX, inf, -inf, nan,
                            -nan, from_bits(0x7f800001u), from_bits(0xffc12345u), 1e-30f, 1e-3f, 1.0f, 20.0f, 37.0f, 45.0f, 1e4f,
                            1e10f, 1e30f, -1.0f, -20.0f, -45.0f, -1e10f};
    struct Pair { rtp::TemporalView cur, prev; };
    const rtp::TemporalView def = kDefaultView;
    std::vector<Pair> pairs = {
        {def, def},
        {yawed(0.37f, -25.0f, 8.6f, 0.0), def},
        {yawed(0.0f, -25.0f, 8.5f, 0.2), def},
        {yawed(0.0f, -20.0f, 8.5f, 0.0), def},
        {yawed(0.0f, -25.0f, 8.5f, 3.0), def},
        {def, yawed(0.0f, -20.0f, 8.5f, 0.0)},            // the previous camera ahead: near points fall behind its plane
        {def, yawed(0.5f, -25.0f, 8.5f, 0.0)}, {def, yawed(-0.5f, -25.0f, 8.5f, 0.0)},  // sideways: fx sweeps with depth
        {def, {{0.0f, -25.0f, 9.0f}, {0.0f, 1.0f, 0.0f}, {0.0f, 0.0f, 1.0f}}},
        {def, {{0.0f, -25.0f, 8.0f}, {0.0f, 1.0f, 0.0f}, {0.0f, 0.0f, 1.0f}}},
        {{{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, def},          // degenerate: no direction at all
        {def, {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}},
        {{{0, -25, 8.5f}, {0, 1, 0}, {0, 1, 0}}, def},     // up along front: right is zero
        {{{FLT_MAX, -FLT_MAX, FLT_MAX}, {FLT_MAX, FLT_MAX, FLT_MAX}, {-FLT_MAX, FLT_MAX, 0}}, def},
        {def, {{FLT_MAX, FLT_MAX, -FLT_MAX}, {FLT_MAX, -FLT_MAX, FLT_MAX}, {FLT_MAX, 0, FLT_MAX}}},
        {{{dmin, -dmin, dmin}, {dmin, dmin, 0}, {0, 0, dmin}}, {{0, 0, 0}, {-dmin, dmin, 0}, {0, 0, dmin}}},
        {{{0, -25, 8.5f}, {0, 1e-20f, 0}, {0, 0, 1e20f}}, {{0, -25, 8.5f}, {0, 1e20f, 0}, {0, 0, 1e-20f}}},
    };
    Sweep s;
    for (auto& wh : sizes) {
        const uint64_t W = wh[0], H = wh[1];
        // the pixels: all of a small image, else the corners, the edges' middles and a coarse grid
        std::vector<uint32_t> xs, ys;
        auto axis = [](uint64_t n, std::vector<uint32_t>& out) {
            if (n <= 131) {
                for (uint64_t i = 0; i < n; ++i) out.push_back((uint32_t)i);
                return;
            }
            for (uint64_t i : {(uint64_t)0, (uint64_t)1, n / 7, n / 3, n / 2 - 1, n / 2, n - n / 3, n - 65, n - 64, n - 2, n - 1})
                out.push_back((uint32_t)i);
        };
        axis(W, xs), axis(H, ys);
        for (const Pair& pr : pairs) {
            rtp::TemporalIn in = sized(W, H);
            in.cur = pr.cur, in.prev = pr.prev;
            rtp::TemporalPlan p;
            if (rtp::temporal_plan(in, &p) != RT_SUCCESS) {
                std::printf("broken: no plan for %llu x %llu\n", (unsigned long long)W, (unsigned long long)H);
                ++s.failures;
                continue;
            }
            s.W = W, s.H = H, s.k = p.k;
            const bool small = W * H <= 131 * 77;
            for (uint32_t y : ys)
                for (uint32_t x : xs) {
                    for (float d : depths) s.one(x, y, d);
                    // on and behind the previous camera's plane: the depth at which zf crosses zero, from a
                    // double restatement of the centre ray
                    const rtt::TemporalConsts& k = s.k;
                    const double sx = ((2.0 * ((x + 0.5) / (double)W) - 1.0) * k.A) * k.asp, sy = (2.0 * ((y + 0.5) / (double)H) - 1.0) * k.A;
                    double d[3], len = 0, un = 0, off = 0;
                    for (int c = 0; c < 3; ++c) d[c] = (double)k.cright[c] * sx + (double)k.cup[c] * sy + k.cfront[c], len += d[c] * d[c];
                    for (int c = 0; c < 3; ++c) un += d[c] / std::sqrt(len) * k.pfront[c], off += ((double)k.cpos[c] - k.ppos[c]) * k.pfront[c];
                    const double d0 = -off / un;
                    if (std::isfinite(d0) && std::fabs(d0) > 1e-30 && std::fabs(d0) < 1e30) {
                        s.around(x, y, (float)d0, small ? 4 : 2);
                        s.one(x, y, (float)(0.5 * d0)), s.one(x, y, (float)(2.0 * d0));
                    }
                }
            // fx within a few ulps of -1, 0, W - 1 and W (and fy likewise): bisect the depth, as a bit pattern,
            // at which the coordinate crosses the target; the coordinate is monotonic in the depth for a
            // previous camera moved sideways or up
            const float targets_x[] = {-1.0f, 0.0f, (float)(W - 1), (float)W}, targets_y[] = {-1.0f, 0.0f, (float)(H - 1), (float)H};
            for (int axis_y = 0; axis_y < 2; ++axis_y)
                for (float target : axis_y ? targets_y : targets_x)
                    for (uint32_t x : {xs.front(), xs[xs.size() / 2], xs.back()})
                        for (uint32_t y : {ys.front(), ys[ys.size() / 2], ys.back()}) {
                            auto coord = [&](uint32_t bits) {
                                const rtt::Projection q = rtt::project(s.k, x, y, from_bits(bits));
                                return axis_y ? q.fy : q.fx;
                            };
                            uint32_t lo = 0x3a83126fu /* 1e-3 */, hi = 0x49742400u /* 1e6 */;
                            const bool lo_above = coord(lo) > target, hi_above = coord(hi) > target;
                            if (lo_above == hi_above || std::isnan(coord(lo)) || std::isnan(coord(hi))) continue;
                            while (hi - lo > 1) {
                                const uint32_t mid = lo + (hi - lo) / 2;
                                ((coord(mid) > target) == lo_above ? lo : hi) = mid;
                            }
                            ++s.bracketed;
                            s.around(x, y, from_bits(lo), 6);
                        }
        }
    }
    std::printf("sweep: %llu projections, %llu passed, %llu taps inside, %llu crossings bracketed, %llu failures\n", s.calls,
                s.passed, s.taps, s.bracketed, s.failures);
    return s.failures ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && std::strcmp(argv[1], "sweep") == 0) return sweep();
    if (argc == 2 && std::strcmp(argv[1], "errors") == 0) return errors();
    std::fprintf(stderr, "usage: temporal_plan_main sweep|errors\n");
    return 2;
}

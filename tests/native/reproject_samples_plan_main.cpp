// reproject_samples_plan_main.cpp -- stand-alone driver of the sample reprojection's host side, CPU only:
// the plan (csrc/rt_reproject_plan.cpp reproject_plan) and the texts the kernel compiles
// (csrc/rt_temporal_math.hpp for the projection and the tap indices, csrc/rt_reproject_math.hpp for the
// tap test, the sums and the recombined record).
//   reproject_samples_plan_main errors          the error rows of rtEnqueueReprojectSamples (rt_hip.h) return
//                                               their codes, in order, and the plan's constants and grid are the
//                                               temporal plan's.
//   reproject_samples_plan_main merge IN OUT    reads IN -- uint32 width, height; 18 floats, the current then the
//                                               previous view (pos, front, up); 3 floats max_history,
//                                               depth_tolerance, normal_threshold; then width * height records of
//                                               32 B each of hist_stats, hist_features, cur_features -- and writes
//                                               the width * height output records to OUT, computed per pixel as the
//                                               kernel does: reproject, tap_index, the features' test, the
//                                               statistics of the taps that passed it only, add_tap, merge.
// Exit status 1 if anything breaks.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/rt_status.h"
#include "../../mini-opencl-raytracer_amd/csrc/rt_reproject_plan.hpp"
#include "image_pass_common.hpp"

static rtp::ReprojectIn sized(uint64_t w, uint64_t h) {
    rtp::ReprojectIn in{};
    in.params_ok = true;
    in.width = w, in.height = h;
    in.cur = in.prev = kDefaultView;
    in.max_history = 16.0f, in.depth_tolerance = 0.05f, in.normal_threshold = 0.9f;
    in.hist_stats_ok = in.hist_features_ok = in.cur_features_ok = in.out_ok = true;
    in.hist_stats_bytes = in.hist_features_bytes = in.cur_features_bytes = in.out_bytes = w * h * 32;
    return in;
}

static rtp::ReprojectIn base_in() { return sized(131, 77); }

// ---- errors -------------------------------------------------------------------------------------

// the documented order, spelled independently of the plan
static int expected(const rtp::ReprojectIn& in) {
    if (!in.params_ok) return RT_INVALID_VALUE;
    const unsigned __int128 pixels = (unsigned __int128)in.width * in.height;
    if (pixels == 0 || pixels > ((unsigned __int128)1 << 31)) return RT_INVALID_VALUE;
    if (!finite_view(in.cur) || !finite_view(in.prev)) return RT_INVALID_VALUE;
    if (!(in.max_history >= 1.0f && in.max_history <= 0x1p20f)) return RT_INVALID_VALUE;  // (false for a NaN)
    if (std::fmod(in.max_history, 1.0f) != 0.0f) return RT_INVALID_VALUE;
    if (!(in.depth_tolerance >= 0.0f && in.depth_tolerance <= 1.0f)) return RT_INVALID_VALUE;
    if (!(in.normal_threshold >= -1.0f && in.normal_threshold <= 1.0f)) return RT_INVALID_VALUE;
    if (!in.hist_stats_ok || !in.hist_features_ok || !in.cur_features_ok || !in.out_ok) return RT_INVALID_MEM_OBJECT;
    if (in.out_is_input) return RT_INVALID_MEM_OBJECT;
    if (pixels * 32 > in.hist_stats_bytes || pixels * 32 > in.hist_features_bytes || pixels * 32 > in.cur_features_bytes ||
        pixels * 32 > in.out_bytes)
        return RT_INVALID_BUFFER_SIZE;
    return RT_SUCCESS;
}

static int errors() {
    int failures = 0;
    auto expect = [&](const char* name, const rtp::ReprojectIn& in, int want) {
        rtp::ReprojectPlan p;
        const int rc = rtp::reproject_plan(in, &p);
        const bool ok = rc == want && expected(in) == want;
        std::printf("%s %s: rc %d (want %d, restated %d)\n", ok ? "ok    " : "FAILED", name, rc, want, expected(in));
        if (!ok) ++failures;
    };
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    rtp::ReprojectIn in = base_in();
    expect("valid", in, RT_SUCCESS);
    in = base_in(), in.params_ok = false;
    expect("params_null", in, RT_INVALID_VALUE);
    in = base_in(), in.width = 0;
    expect("width_zero", in, RT_INVALID_VALUE);
    in = base_in(), in.height = 0;
    expect("height_zero", in, RT_INVALID_VALUE);
    in = sized(65536, 32768 + 1);
    expect("past_2_31", in, RT_INVALID_VALUE);
    in = sized(0xffffffffull, 0xffffffffull);
    in.hist_stats_bytes = in.hist_features_bytes = in.cur_features_bytes = in.out_bytes = ~0ull;
    expect("product_near_2_64", in, RT_INVALID_VALUE);
    in = sized(65536, 32768);
    expect("exactly_2_31", in, RT_SUCCESS);
    in = base_in(), in.cur.pos[1] = nan;
    expect("camera_nan", in, RT_INVALID_VALUE);
    in = base_in(), in.prev.up[2] = inf;
    expect("camera_infinite", in, RT_INVALID_VALUE);
    in = base_in(), in.cur.front[0] = -inf;
    expect("camera_front_infinite", in, RT_INVALID_VALUE);
    in = base_in(), in.max_history = nan;
    expect("max_history_nan", in, RT_INVALID_VALUE);
    in = base_in(), in.max_history = inf;
    expect("max_history_infinite", in, RT_INVALID_VALUE);
    in = base_in(), in.max_history = 0.0f;
    expect("max_history_zero", in, RT_INVALID_VALUE);
    in = base_in(), in.max_history = 0.5f;
    expect("max_history_below_one", in, RT_INVALID_VALUE);
    in = base_in(), in.max_history = 3.5f;
    expect("max_history_fraction", in, RT_INVALID_VALUE);
    in = base_in(), in.max_history = -4.0f;
    expect("max_history_negative", in, RT_INVALID_VALUE);
    in = base_in(), in.max_history = 0x1p20f + 1.0f;
    expect("max_history_huge", in, RT_INVALID_VALUE);
    in = base_in(), in.max_history = 1.0f;
    expect("max_history_one", in, RT_SUCCESS);
    in = base_in(), in.max_history = 0x1p20f;
    expect("max_history_largest", in, RT_SUCCESS);
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
    in = base_in(), in.hist_stats_ok = false, in.hist_stats_bytes = 0;
    expect("hist_stats_null", in, RT_INVALID_MEM_OBJECT);
    in = base_in(), in.hist_features_ok = false, in.hist_features_bytes = 0;
    expect("hist_features_null", in, RT_INVALID_MEM_OBJECT);
    in = base_in(), in.cur_features_ok = false, in.cur_features_bytes = 0;
    expect("cur_features_null", in, RT_INVALID_MEM_OBJECT);
    in = base_in(), in.out_ok = false, in.out_bytes = 0;
    expect("out_null", in, RT_INVALID_MEM_OBJECT);
    in = base_in(), in.out_is_input = true;
    expect("out_is_an_input", in, RT_INVALID_MEM_OBJECT);
    in = base_in(), in.hist_stats_bytes -= 1;
    expect("hist_stats_short", in, RT_INVALID_BUFFER_SIZE);
    in = base_in(), in.hist_features_bytes -= 1;
    expect("hist_features_short", in, RT_INVALID_BUFFER_SIZE);
    in = base_in(), in.cur_features_bytes -= 1;
    expect("cur_features_short", in, RT_INVALID_BUFFER_SIZE);
    in = base_in(), in.out_bytes -= 1;
    expect("out_short", in, RT_INVALID_BUFFER_SIZE);
    // the order: the earlier row wins
    in = base_in(), in.max_history = 0.0f, in.out_ok = false, in.hist_stats_bytes = 1;
    expect("value_before_mem_object", in, RT_INVALID_VALUE);
    in = base_in(), in.normal_threshold = 2.0f, in.out_is_input = true;
    expect("last_value_before_mem_object", in, RT_INVALID_VALUE);
    in = base_in(), in.width = 0, in.out_bytes = 0;
    expect("size_zero_before_buffer_size", in, RT_INVALID_VALUE);
    in = base_in(), in.out_is_input = true, in.out_bytes = 1;
    expect("mem_object_before_size", in, RT_INVALID_MEM_OBJECT);
    in = base_in(), in.hist_features_ok = false, in.cur_features_bytes = 1;
    expect("foreign_before_size", in, RT_INVALID_MEM_OBJECT);
    // the constants and the grid: bit for bit the temporal plan's on the same views
    bool ok = true;
    static const uint64_t shapes[][2] = {{1, 1}, {5, 3}, {61, 7}, {131, 77}, {3840, 2160}, {1ull << 31, 1}, {1, 1ull << 31}, {65536, 32768}};
    for (auto& wh : shapes) {
        in = sized(wh[0], wh[1]);
        in.cur = {{0.37f, -25.0f, 8.6f}, {0.5f, 1.0f, 0.25f}, {0.0f, 0.25f, 1.0f}};
        in.max_history = 7.0f, in.depth_tolerance = 0.25f, in.normal_threshold = -0.5f;
        rtp::ReprojectPlan p;
        ok = ok && rtp::reproject_plan(in, &p) == RT_SUCCESS;
        rtp::TemporalIn t{};
        t.params_ok = true, t.width = wh[0], t.height = wh[1], t.cur = in.cur, t.prev = in.prev;
        t.cur_frames = 8.0f, t.max_history = 32.0f, t.depth_tolerance = 0.05f, t.normal_threshold = 0.9f;
        t.cur_ok = t.cur_features_ok = t.out_ok = true;
        t.cur_bytes = t.out_bytes = wh[0] * wh[1] * 16, t.cur_features_bytes = wh[0] * wh[1] * 32;
        rtp::TemporalPlan tp;
        ok = ok && rtp::temporal_plan(t, &tp) == RT_SUCCESS && std::memcmp(&p.k, &tp.k, sizeof(p.k)) == 0;
        ok = ok && p.width == wh[0] && p.height == wh[1] && p.tiles_x == tp.tiles_x && p.tiles_y == tp.tiles_y && p.grid == tp.grid;
        ok = ok && p.grid > 0 && (uint64_t)p.tiles_x * p.tiles_y == p.grid && (uint64_t)p.tiles_x * rtp::kTemporalTileW >= wh[0] &&
             (uint64_t)p.tiles_y * rtp::kTemporalTileH >= wh[1];
        ok = ok && p.max_history == 7.0f && p.depth_tolerance == 0.25f && p.normal_threshold == -0.5f;
        ok = ok && p.k.cright[0] == 1.0f * 1.0f - 0.25f * 0.25f && p.k.pright[0] == 1.0f && p.k.cpos[0] == 0.37f;
    }
    in = sized(131, 77);
    rtp::ReprojectPlan p;
    ok = ok && rtp::reproject_plan(in, &p) == RT_SUCCESS && p.tiles_x == 3 && p.tiles_y == 20 && p.grid == 60;
    std::printf("%s constants\n", ok ? "ok    " : "FAILED");
    if (!ok) ++failures;
    return failures ? 1 : 0;
}

// ---- merge --------------------------------------------------------------------------------------

struct Record {
    float f[8];
};

static bool read_exact(std::FILE* fp, void* dst, size_t n) { return n == 0 || std::fread(dst, 1, n, fp) == n; }

static int merge_file(const char* in_path, const char* out_path) {
    std::FILE* fp = std::fopen(in_path, "rb");
    if (!fp) return std::fprintf(stderr, "cannot read %s\n", in_path), 1;
    uint32_t wh[2];
    float views[18], prm[3];
    bool ok = read_exact(fp, wh, sizeof(wh)) && read_exact(fp, views, sizeof(views)) && read_exact(fp, prm, sizeof(prm));
    const uint64_t W = ok ? wh[0] : 0, H = ok ? wh[1] : 0;
    if (!ok || W == 0 || H == 0 || W * H > (1u << 24)) return std::fclose(fp), std::fprintf(stderr, "bad header\n"), 1;
    const size_t pixels = (size_t)(W * H);
    std::vector<Record> hist_stats(pixels), hist_features(pixels), cur_features(pixels), out(pixels);
    ok = read_exact(fp, hist_stats.data(), pixels * 32) && read_exact(fp, hist_features.data(), pixels * 32) &&
         read_exact(fp, cur_features.data(), pixels * 32);
    std::fclose(fp);
    if (!ok) return std::fprintf(stderr, "short input\n"), 1;

    rtp::ReprojectIn in = sized(W, H);
    for (int c = 0; c < 3; ++c) {
        in.cur.pos[c] = views[c], in.cur.front[c] = views[3 + c], in.cur.up[c] = views[6 + c];
        in.prev.pos[c] = views[9 + c], in.prev.front[c] = views[12 + c], in.prev.up[c] = views[15 + c];
    }
    in.max_history = prm[0], in.depth_tolerance = prm[1], in.normal_threshold = prm[2];
    rtp::ReprojectPlan p;
    const int rc = rtp::reproject_plan(in, &p);
    if (rc != RT_SUCCESS) return std::fprintf(stderr, "plan refused: %d\n", rc), 1;

    unsigned long long carried = 0, fetched = 0;
    for (uint32_t y = 0; y < p.height; ++y)
        for (uint32_t x = 0; x < p.width; ++x) {
            const size_t at = (size_t)y * p.width + x;
            const float* f = cur_features[at].f;  // {albedo, depth}, {normal, coverage}
            rtt::Reprojection r = rtt::reproject(p.k, x, y, f[3]);
            r.ok = r.ok && f[7] > 0.0f;
            const float tol = p.depth_tolerance * r.de;
            rtrs::TapSums sums = rtrs::no_taps();
            for (int t = 0; t < 4; ++t) {  // j outer, i inner
                uint64_t q = 0;
                const bool inside = rtt::tap_index(r, t & 1, t >> 1, p.width, p.height, &q);
                if (inside && q >= pixels) return std::fprintf(stderr, "tap outside the image\n"), 1;
                static const float none[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // coverage 0: does not count
                const float* g = inside ? hist_features[q].f : none;
                const bool on = rtrs::tap_on_surface(inside, g[7], g[3], g + 4, f + 4, r.de, tol, p.normal_threshold);
                const float* s = on ? hist_stats[q].f : none;              // n 0: does not count
                fetched += on;
                const rtrs::Stats st = {{s[0], s[1], s[2]}, s[3], s[4], s[5]};
                rtrs::add_tap(sums, on, rtt::tap_weight(r, t & 1, t >> 1), st);
            }
            Record o{};  // nothing carried: 32 zero bytes
            rtrs::Stats m;
            if (rtrs::merge(sums, p.max_history, &m)) {
                o.f[0] = m.sum[0], o.f[1] = m.sum[1], o.f[2] = m.sum[2], o.f[3] = m.n, o.f[4] = m.mean_y, o.f[5] = m.m2_y;
                ++carried;
            }
            out[at] = o;
        }
    fp = std::fopen(out_path, "wb");
    if (!fp) return std::fprintf(stderr, "cannot write %s\n", out_path), 1;
    ok = std::fwrite(out.data(), 32, pixels, fp) == pixels;
    ok = std::fclose(fp) == 0 && ok;
    std::printf("merge: %llu x %llu, %llu carried, %llu statistics records fetched\n", (unsigned long long)W, (unsigned long long)H,
                carried, fetched);
    return ok ? 0 : 1;
}

int main(int argc, char** argv) {
    if (argc == 2 && std::strcmp(argv[1], "errors") == 0) return errors();
    if (argc == 4 && std::strcmp(argv[1], "merge") == 0) return merge_file(argv[2], argv[3]);
    std::fprintf(stderr, "usage: reproject_samples_plan_main errors | merge IN OUT\n");
    return 2;
}

// sample_plan_main.cpp -- stand-alone driver of rtEnqueueSamplePixels' host side, CPU only: sample_check's
// error rows and sample_plan's units and grid (csrc/rt_adaptive_plan.{hpp,cpp} over csrc/rt_trace_plan.cpp).
//   sample_plan_main errors   every row of the error list alone returns its code, and every pair of rows
//                             broken together returns the earlier row's code; n == 0 passes the checks with
//                             nothing to launch, and does not excuse an error.
//   sample_plan_main sweep    plans n in {0, 1, 63, 64, 65, 2^31 - first} for several offsets, scene sizes
//                             either side of the LDS limit, forced global and occupancies 1..8: the capacity's
//                             units hold every record once, the grid never exceeds occupancy x CUs nor the
//                             waves that have a unit, and for every device count c the units the kernel forms
//                             from m = min(n, c) -- the kernel's own arithmetic, restated -- lie inside the
//                             capacity and inside the ids the host checked.
// Exit status 1 if anything breaks.
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/rt_status.h"
#include "../../mini-opencl-raytracer_amd/csrc/rt_adaptive_plan.hpp"
#include "../../mini-opencl-raytracer_amd/csrc/rt_layout.hpp"

static rtp::SampleIn base_in() {
    rtp::SampleIn in{};
    in.first = 3, in.n = 427, in.n_pixels = 61 * 7;
    in.ids_ok = in.stats_ok = in.count_given = in.count_ok = true;
    in.ids_bytes = (3 + 427) * 4, in.count_bytes = 16, in.stats_bytes = 61 * 7 * 32;
    in.slots_set = true, in.width = 61, in.height = 7;
    in.scene_bound = in.lights_set = true;
    in.scene.n_nodes = 21, in.scene.n_tris = 36, in.scene.n_mats = 8;
    in.scene.oct_ok = true, in.scene.goct_available = true, in.scene.goct_b = 176;
    in.scene.num_cus = 256;
    return in;
}

// one mutation of a valid input per error row, in the documented order
struct Row {
    const char* name;
    void (*break_it)(rtp::SampleIn&);
    int code;
};
static const Row kRows[] = {
    {"range_past_2_31", [](rtp::SampleIn& in) { in.first = (1ull << 31) - 426; }, RT_INVALID_VALUE},
    {"n_pixels_zero", [](rtp::SampleIn& in) { in.n_pixels = 0; }, RT_INVALID_VALUE},
    {"n_pixels_past_2_31", [](rtp::SampleIn& in) { in.n_pixels = (1ull << 31) + 1; }, RT_INVALID_VALUE},
    {"ids_not_of_context", [](rtp::SampleIn& in) { in.ids_ok = false, in.ids_bytes = 0; }, RT_INVALID_MEM_OBJECT},
    {"stats_not_of_context", [](rtp::SampleIn& in) { in.stats_ok = false, in.stats_bytes = 0; }, RT_INVALID_MEM_OBJECT},
    {"count_not_of_context", [](rtp::SampleIn& in) { in.count_ok = false, in.count_bytes = 0; }, RT_INVALID_MEM_OBJECT},
    {"aliased", [](rtp::SampleIn& in) { in.aliased = true; }, RT_INVALID_MEM_OBJECT},
    {"ids_short", [](rtp::SampleIn& in) { in.ids_bytes = (3 + 427) * 4 - 1; }, RT_INVALID_BUFFER_SIZE},
    {"count_short", [](rtp::SampleIn& in) { in.count_bytes = 15; }, RT_INVALID_BUFFER_SIZE},
    {"stats_short", [](rtp::SampleIn& in) { in.stats_bytes = 61 * 7 * 32 - 1; }, RT_INVALID_BUFFER_SIZE},
    {"camera_slot_unset", [](rtp::SampleIn& in) { in.slots_set = false, in.width = in.height = 0; }, RT_INVALID_KERNEL_ARGS},
    {"width_zero", [](rtp::SampleIn& in) { in.width = 0; }, RT_INVALID_KERNEL_ARGS},
    {"height_zero", [](rtp::SampleIn& in) { in.height = 0; }, RT_INVALID_KERNEL_ARGS},
    {"scene_unbound", [](rtp::SampleIn& in) { in.scene_bound = false; }, RT_INVALID_KERNEL_ARGS},
    {"lights_unset", [](rtp::SampleIn& in) { in.lights_set = false; }, RT_INVALID_KERNEL_ARGS},
    {"leaf_too_large", [](rtp::SampleIn& in) { in.scene.oct_ok = false; }, RT_INVALID_OPERATION},
};
constexpr size_t kNRows = sizeof(kRows) / sizeof(kRows[0]);

static int failures = 0;
static void expect(const std::string& name, const rtp::SampleIn& in, int want, int nothing = -1) {
    rtp::SamplePlan p;
    const int rc = rtp::sample_plan(in, 4, &p);
    const bool ok = rc == want && (nothing < 0 || (int)p.nothing == nothing);
    std::printf("%s %s: rc %d (want %d)\n", ok ? "ok    " : "FAILED", name.c_str(), rc, want);
    if (!ok) ++failures;
}

static int errors() {
    rtp::SampleIn in = base_in();
    expect("valid", in, RT_SUCCESS, 0);
    in = base_in(), in.count_given = in.count_ok = false, in.count_bytes = 0;
    expect("valid_without_count", in, RT_SUCCESS, 0);
    in = base_in(), in.first = (1ull << 31) - 427, in.ids_bytes = ~0ull;
    expect("range_exactly_2_31", in, RT_SUCCESS, 0);
    in = base_in(), in.first = ~0ull, in.n = 2;
    expect("range_wraps", in, RT_INVALID_VALUE);
    in = base_in(), in.n_pixels = 1ull << 31, in.stats_bytes = ~0ull;
    expect("n_pixels_exactly_2_31", in, RT_SUCCESS, 0);
    for (size_t i = 0; i < kNRows; ++i) {
        in = base_in();
        kRows[i].break_it(in);
        expect(kRows[i].name, in, kRows[i].code);
        // an empty range does not excuse the rows before it (the leaf test comes after it: nothing is prepared)
        in.n = 0;
        if (i == 0) in.first = (1ull << 31) + 1;  // (that row is about the range itself)
        if (std::strcmp(kRows[i].name, "ids_short") == 0) in.ids_bytes = in.first * 4 - 1;  // (the empty range starts past ids)
        expect(std::string(kRows[i].name) + "_before_n_zero", in, i + 1 == kNRows ? RT_SUCCESS : kRows[i].code,
               i + 1 == kNRows ? 1 : -1);
        // every pair: the earlier row wins
        for (size_t j = i + 1; j < kNRows; ++j) {
            in = base_in();
            kRows[j].break_it(in);
            kRows[i].break_it(in);
            expect(std::string(kRows[i].name) + "_before_" + kRows[j].name, in, kRows[i].code);
        }
    }
    in = base_in(), in.n = 0;
    expect("n_zero", in, RT_SUCCESS, 1);
    in = base_in(), in.n = 0, in.first = 430;
    expect("n_zero_at_the_end_of_ids", in, RT_SUCCESS, 1);
    return failures ? 1 : 0;
}

// the kernel's count clause (rt_sample.hpp SampleEnds): m, its units, and per unit the lanes that hold a record
static uint32_t device_m(uint32_t n, bool given, uint32_t c) { return given ? (c < n ? c : n) : n; }
static uint32_t device_units(uint32_t m) { return (m + 63u) >> 6; }

static int sweep() {
    static const uint64_t firsts[] = {0, 3, 4097, (1ull << 31) - 65};
    struct Scene { uint32_t n_nodes, n_tris, n_mats, goct_b; };
    static const Scene scenes[] = {{21, 36, 8, 176}, {91, 318, 6, 736}, {93, 330, 6, 752}, {49471, 70000, 3, 395776}};
    unsigned long long plans = 0, launched = 0, counts = 0, bad = 0, lds = 0, global = 0;
    auto need = [&](bool ok, const char* what, uint64_t first, uint64_t n) {
        if (!ok && ++bad <= 20) std::printf("broken [%s]: first %llu n %llu\n", what, (unsigned long long)first, (unsigned long long)n);
    };
    for (uint64_t first : firsts) {
        const uint64_t ns[] = {0, 1, 63, 64, 65, (1ull << 31) - first};
        for (uint64_t n : ns)
        for (const Scene& sc : scenes)
        for (int force = 0; force < 2; ++force)
        for (int occ = 1; occ <= 8; ++occ) {
            rtp::SampleIn in = base_in();
            in.first = first, in.n = n, in.ids_bytes = (first + n) * 4;
            in.scene.n_nodes = sc.n_nodes, in.scene.n_tris = sc.n_tris, in.scene.n_mats = sc.n_mats;
            in.scene.goct_b = sc.goct_b, in.scene.force_global = force != 0, in.scene.math = occ % 3, in.scene.stats = (occ & 1) != 0;
            rtp::SamplePlan p;
            const int rc = rtp::sample_plan(in, occ, &p);
            ++plans;
            need(rc == RT_SUCCESS, "accepted", first, n);
            if (rc != RT_SUCCESS) continue;
            need(p.nothing == (n == 0), "nothing_iff_empty", first, n);
            if (p.nothing) continue;
            ++launched;
            (p.trace.variant.lds() ? lds : global) += 1;
            need(p.first == first && p.n == n && p.n_pixels == in.n_pixels, "range_kept", first, n);
            need((uint64_t)p.first + p.n <= rtp::kAdaptiveMaxRecords, "indices_32bit", first, n);
            need(p.capUnits == (n + 63) / 64 && p.capUnits == p.trace.nUnits && p.capUnits >= 1, "capacity_units", first, n);
            need(p.trace.grid >= 1 && p.trace.grid <= (uint64_t)occ * 256u, "grid_within_occupancy", first, n);
            need((uint64_t)p.trace.grid <= ((uint64_t)p.capUnits + 3) / 4, "a_unit_per_wave", first, n);
            need(p.trace.variant.math == in.scene.math && p.trace.variant.stats == in.scene.stats, "variant", first, n);
            need(p.trace.smem <= rtp::kTraceLdsBudget && p.trace.smem >= 4u * rtk::kTraceRingBytes, "lds_bytes", first, n);
            // the device count: whatever the word holds, the kernel's units lie inside the capacity, tile
            // [0, m) without a gap, and the last record it reads is inside what the host checked
            const uint32_t cs[] = {0u, 1u, 63u, 64u, 65u, (uint32_t)n - 1u, (uint32_t)n, (uint32_t)n + 1u, (uint32_t)n + 1000u,
                                   0x7fffffffu, 0x80000000u, 0x80000001u, 0xffffffffu};
            for (int given = 0; given < 2; ++given)
            for (uint32_t c : cs) {
                ++counts;
                const uint32_t m = device_m(p.n, given != 0, c), units = device_units(m);
                need(m <= p.n && (given || m == p.n) && (!given || m == (c < n ? c : n)), "m_clamped", first, n);
                need(units <= p.capUnits && (uint64_t)units * 64 >= m && (units == 0 || (uint64_t)(units - 1) * 64 < m),
                     "units_tile_m", first, n);
                if (units) {
                    const uint32_t u0 = (units - 1) * 64u, left = m - u0;   // the last unit: lanes < left hold a record
                    need(left >= 1 && left <= 64, "last_unit_partial", first, n);
                    need(((uint64_t)p.first + u0 + (left - 1)) * 4 + 4 <= in.ids_bytes, "last_id_inside", first, n);
                }
            }
        }
    }
    if (lds == 0 || global == 0) std::printf("the sweep did not reach both scene paths\n"), ++bad;
    std::printf("sweep: %llu plans, %llu launched (%llu LDS, %llu HBM/L2), %llu device counts, %llu failures\n", plans, launched,
                lds, global, counts, bad);
    return bad ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && std::strcmp(argv[1], "errors") == 0) return errors();
    if (argc == 2 && std::strcmp(argv[1], "sweep") == 0) return sweep();
    std::fprintf(stderr, "usage: sample_plan_main errors|sweep\n");
    return 2;
}

// query_plan_main.cpp -- stand-alone driver of the ray-query plan (csrc/rt_query_plan.cpp), CPU only.
//   query_plan_main sweep   plans a sweep of ray counts, offsets, scene sizes either side of the LDS
//                           limit, forced global, both modes and occupancies 1..8 and checks on every
//                           accepted plan: every ray belongs to exactly one unit, no unit is empty,
//                           the grid never exceeds occupancy x CUs, LDS bytes <= 160 KiB.
//   query_plan_main errors  the error rows of rtEnqueueIntersectRays (rt_hip.h) return their codes.
// Exit status 1 if anything breaks.
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/rt_status.h"
#include "../../mini-opencl-raytracer_amd/csrc/rt_layout.hpp"
#include "../../mini-opencl-raytracer_amd/csrc/rt_query_plan.hpp"
#include "../../mini-opencl-raytracer_amd/csrc/rt_scene_pack.hpp"

static rtp::QueryIn base_in() {
    rtp::QueryIn in{};
    in.first_ray = 0, in.n_rays = 2048;
    in.rays_bytes = 1ull << 40, in.hits_bytes = 1ull << 40;
    in.mode = rtp::kQueryClosest;
    in.n_nodes = 21, in.n_tris = 36;
    in.oct_ok = true, in.goct_available = true, in.goct_b = 176;
    in.num_cus = 256;
    return in;
}

// the invariants of an accepted plan: the names of the broken ones
static std::string broken(const rtp::QueryIn& in, int occ, const rtp::QueryPlan& p) {
    std::string bad;
    auto need = [&](bool ok, const char* name) {
        if (!ok) bad += std::string(bad.empty() ? "" : ",") + name;
    };
    need(p.first == in.first_ray && p.count == in.n_rays, "range_kept");
    const bool lds = p.variant.lds();
    // unit j holds rays [first + 64 j, min(first + 64 j + 64, first + count)): contiguous from `first`,
    // so every ray is in exactly one unit when the units tile [0, count) and none is empty
    // (the units depend on the count alone: walked once per count)
    static uint64_t seen_count = ~0ull, seen_units = 0, covered = 0;
    static bool empty = false, gap = false;
    if (seen_count != p.count || seen_units != p.nUnits) {
        seen_count = p.count, seen_units = p.nUnits;
        covered = 0, empty = false, gap = false;
        for (uint64_t j = 0; j < p.nUnits; ++j) {
            const uint64_t lo = 64 * j, hi = lo + 64 < p.count ? lo + 64 : p.count;
            if (lo != covered) gap = true;
            if (hi <= lo) empty = true;
            covered = hi;
        }
    }
    need(!gap && covered == p.count, "every_ray_in_one_unit");
    need(!empty && p.nUnits >= 1, "no_empty_unit");
    need((uint64_t)p.first + p.count <= rtp::kQueryMaxRays, "indices_32bit");
    need(p.grid >= 1 && p.grid <= (uint64_t)occ * (uint64_t)in.num_cus, "grid_within_occupancy");
    need((uint64_t)p.grid <= ((uint64_t)p.nUnits + 7) / 8, "a_unit_per_workgroup");
    need(p.smem <= 160 * 1024, "lds_160k");
    const size_t rings = (rtk::kQueryThreads / 64) * (size_t)rtk::kQueryRingBytes;
    const size_t scene = (size_t)rtp::oct_records(in.n_nodes) * 16 + (size_t)in.n_tris * 48;
    need(p.smem == (lds ? scene : 0) + rings, "lds_bytes");
    need(!lds || (!in.force_global && p.smem <= rtp::kQueryLdsBudget), "lds_budget");
    need(lds || in.force_global || scene + rings > rtp::kQueryLdsBudget, "lds_when_it_fits");
    need(!lds || (p.octRecords == rtp::oct_records(in.n_nodes) && p.nNodes == in.n_nodes && !p.regrouped),
         "lds_records");
    need((p.variant.walk == rtk::Walk::LdsB) == (lds && p.octB == rtk::kOctB), "bofs");
    need(lds || p.variant.walk == rtk::Walk::GlobalOct, "octant_walk_outside_lds");
    need(p.variant.any == (in.mode == rtp::kQueryAny), "mode");
    need(p.refillMin == in.tune.query_refill_min && p.stepWeightNode > 0 && p.stepWeightLeaf > 0, "tuning");
    return bad;
}

static int sweep() {
    static const uint64_t counts[] = {1, 63, 64, 65, 4097, (1ull << 20) + 37, 1ull << 31};
    static const uint64_t firsts[] = {0, 1, 4097, (1ull << 31) - 65};
    // nodes / triangles: Cornell; just inside and just outside the LDS limit; the bunny proxy
    struct Scene { uint32_t n_nodes, n_tris, goct_b; };
    static const Scene scenes[] = {{21, 36, 176}, {63, 300, 520}, {100, 410, 808}, {110, 450, 888},
                                   {150, 520, 1208}, {49471, 70000, 395776}};
    unsigned long long plans = 0, accepted = 0, failures = 0, lds_plans = 0, global_plans = 0;
    for (uint64_t n : counts)
    for (uint64_t first : firsts)
    for (const Scene& sc : scenes)
    for (int force = 0; force < 2; ++force)
    for (int mode = 0; mode < 2; ++mode)
    for (int occ = 1; occ <= 8; ++occ) {
        rtp::QueryIn in = base_in();
        in.first_ray = first, in.n_rays = n;
        in.n_nodes = sc.n_nodes, in.n_tris = sc.n_tris, in.goct_b = sc.goct_b;
        in.force_global = force != 0, in.mode = mode;
        rtp::QueryPlan p;
        const int rc = rtp::query_plan(in, occ, &p);
        ++plans;
        if (first + n > rtp::kQueryMaxRays) {
            if (rc != RT_INVALID_VALUE) {
                std::printf("range past 2^31 accepted: first %llu n %llu rc %d\n", (unsigned long long)first,
                            (unsigned long long)n, rc);
                ++failures;
            }
            continue;
        }
        if (rc != RT_SUCCESS || p.nothing) {
            std::printf("unexpected rc %d nothing %d: first %llu n %llu\n", rc, (int)p.nothing,
                        (unsigned long long)first, (unsigned long long)n);
            ++failures;
            continue;
        }
        ++accepted;
        (p.variant.lds() ? lds_plans : global_plans) += 1;
        const std::string bad = broken(in, occ, p);
        if (!bad.empty() && ++failures <= 20)
            std::printf("broken [%s]: first %llu n %llu nodes %u tris %u force %d mode %d occ %d\n", bad.c_str(),
                        (unsigned long long)first, (unsigned long long)n, sc.n_nodes, sc.n_tris, force, mode, occ);
    }
    if (lds_plans == 0 || global_plans == 0) {
        std::printf("the sweep did not reach both scene paths\n");
        ++failures;
    }
    std::printf("sweep: %llu plans, %llu accepted (%llu LDS, %llu HBM/L2), %llu failures\n", plans, accepted,
                lds_plans, global_plans, failures);
    return failures ? 1 : 0;
}

static int errors() {
    int failures = 0;
    auto expect = [&](const char* name, const rtp::QueryIn& in, int want, bool nothing = false) {
        rtp::QueryPlan p;
        const int rc = rtp::query_plan(in, 4, &p);
        const bool ok = rc == want && (rc != RT_SUCCESS || p.nothing == nothing);
        std::printf("%s %s: rc %d (want %d)\n", ok ? "ok    " : "FAILED", name, rc, want);
        if (!ok) ++failures;
    };
    rtp::QueryIn in = base_in();
    expect("valid", in, RT_SUCCESS);
    in = base_in(), in.n_rays = 0;
    expect("n_rays_zero", in, RT_SUCCESS, true);
    in = base_in(), in.mode = 2;
    expect("mode_2", in, RT_INVALID_VALUE);
    in = base_in(), in.mode = -1;
    expect("mode_negative", in, RT_INVALID_VALUE);
    in = base_in(), in.rays_bytes = 2048 * 32 - 1;
    expect("rays_buffer_short", in, RT_INVALID_BUFFER_SIZE);
    in = base_in(), in.hits_bytes = 2048 * 16 - 1;
    expect("hits_buffer_short", in, RT_INVALID_BUFFER_SIZE);
    in = base_in(), in.first_ray = 1, in.rays_bytes = 2048 * 32, in.hits_bytes = 2049 * 16;
    expect("offset_past_rays", in, RT_INVALID_BUFFER_SIZE);
    in = base_in(), in.rays_bytes = 2048 * 32, in.hits_bytes = 2048 * 16;
    expect("exact_fit", in, RT_SUCCESS);
    in = base_in(), in.first_ray = 1ull << 31, in.n_rays = 1;
    expect("past_2_31", in, RT_INVALID_VALUE);
    in = base_in(), in.first_ray = 1, in.n_rays = 1ull << 31;
    expect("past_2_31_by_one", in, RT_INVALID_VALUE);
    in = base_in(), in.first_ray = 5, in.n_rays = ~0ull - 2;
    expect("sum_wraps", in, RT_INVALID_VALUE);
    in = base_in(), in.first_ray = 0, in.n_rays = 1ull << 31;
    expect("exactly_2_31", in, RT_SUCCESS);
    in = base_in(), in.same_buffer = true;
    expect("same_buffer", in, RT_INVALID_MEM_OBJECT);
    in = base_in(), in.oct_ok = false;
    expect("leaf_too_large", in, RT_INVALID_OPERATION);
    return failures ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && std::strcmp(argv[1], "sweep") == 0) return sweep();
    if (argc == 2 && std::strcmp(argv[1], "errors") == 0) return errors();
    std::fprintf(stderr, "usage: query_plan_main sweep|errors\n");
    return 2;
}

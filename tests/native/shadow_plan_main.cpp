// shadow_plan_main.cpp -- the shadow-ray setting's way through the plans, swept on the CPU (built by
// tests/test_shadow_plan.py with plain g++ and once more with sanitizers; no GPU, no HIP):
//   slots  rtk::Variant::slot() with the shadow bit as its highest-order factor: every variant without the bit
//          keeps the slot the six older factors gave it, the variants with it take the upper half, and all
//          slots are distinct and below kVariantSlots;
//   sweep  trace_plan and sample_plan over scene sizes, ranges and settings: the variant carries the kernel's
//          setting, and nothing else of an accepted plan -- LDS bytes, walk records, units, thresholds, grid --
//          or of a refused one depends on it.
#include <cstdio>
#include <set>
#include <string>

#include "../../include/rt_status.h"
#include "../../mini-opencl-raytracer_amd/csrc/rt_adaptive_plan.hpp"
#include "../../mini-opencl-raytracer_amd/csrc/rt_layout.hpp"
#include "../../mini-opencl-raytracer_amd/csrc/rt_trace_plan.hpp"

static int failures = 0;
static void need(bool ok, const char* what, long long a = 0, long long b = 0) {
    if (!ok) {
        std::printf("FAILED %s (%lld, %lld)\n", what, a, b);
        ++failures;
    }
}

static int slots() {
    std::set<int> seen;
    const int scheds[3] = {rtk::kSchedTiles, rtk::kSchedStep, rtk::kSchedWavefront};
    int n = 0;
    for (int shadow = 0; shadow < 2; ++shadow)
        for (int sched : scheds)
            for (int math = 0; math < 3; ++math)
                for (int walk = 0; walk < 4; ++walk)
                    for (int bits = 0; bits < 8; ++bits) {
                        const bool stats = bits & 4, fused = bits & 2, any = bits & 1;
                        rtk::Variant v{sched, math, (rtk::Walk)walk, stats, fused, any};
                        need(!v.shadow, "the bit defaults to off");
                        v.shadow = shadow != 0;
                        const int old_slot = (((((sched >> 1) * 3 + math) * 4 + walk) * 2 + stats) * 2 + fused) * 2 + any;
                        const int s = v.slot();
                        need(s >= 0 && s < rtk::kVariantSlots, "slot in range", s);
                        need(shadow ? s == old_slot + rtk::kVariantSlots / 2 : s == old_slot, "slot keeps its number", s, old_slot);
                        need(seen.insert(s).second, "slot distinct", s);
                        ++n;
                    }
    need(n == rtk::kVariantSlots && (int)seen.size() == n, "slots dense", n);
    std::printf("slots: %d variants\n", n);
    return failures;
}

static rtp::TraceIn base_in() {
    rtp::TraceIn in{};
    in.params_given = true, in.encoding = rtp::kTraceLinear;
    in.first = 3, in.n = 2048;
    in.rays_ok = in.out_ok = true, in.seeds_given = in.seeds_ok = true;
    in.rays_bytes = 4096 * 32, in.seeds_bytes = 4096 * 4, in.out_bytes = 4096 * 16;
    in.scene_bound = in.lights_set = true;
    in.math = 2, in.stats = false;
    in.n_nodes = 71, in.n_tris = 36, in.n_mats = 8;
    in.oct_ok = true, in.goct_available = true, in.goct_b = 128;
    in.tune = rtp::Tuning{};
    in.num_cus = 256;
    return in;
}

static bool same_but_shadow(const rtp::TracePlan& a, const rtp::TracePlan& b) {
    rtk::Variant va = a.variant, vb = b.variant;
    va.shadow = vb.shadow = false;
    return a.nothing == b.nothing && va.slot() == vb.slot() && a.regrouped == b.regrouped && a.smem == b.smem &&
           a.first == b.first && a.count == b.count && a.nUnits == b.nUnits && a.octStride == b.octStride &&
           a.octB == b.octB && a.octRecords == b.octRecords && a.nNodes == b.nNodes && a.refillMin == b.refillMin &&
           a.shadeMin == b.shadeMin && a.stepWeightNode == b.stepWeightNode && a.stepWeightLeaf == b.stepWeightLeaf &&
           a.grid == b.grid;
}

static int sweep() {
    long long plans = 0, refused = 0;
    const uint32_t tris[] = {1, 36, 300, 700, 5000};
    const uint64_t counts[] = {0, 1, 64, 65, 2048, 1ull << 31};
    for (uint32_t nt : tris)
        for (uint64_t n : counts)
            for (int math = 0; math < 3; ++math)
                for (int bits = 0; bits < 8; ++bits)
                    for (int occ = 1; occ <= 5; occ += 2) {
                        rtp::TraceIn in = base_in();
                        in.n_tris = nt, in.n_nodes = 2 * nt - 1, in.n = n, in.first = n == (1ull << 31) ? 1 : 3;
                        in.rays_bytes = in.out_bytes = in.seeds_bytes = ~0ull;
                        in.math = math, in.stats = bits & 1, in.force_global = bits & 2, in.oct_ok = !(bits & 4) || nt < 700;
                        rtp::TracePlan p[2];
                        int rc[2];
                        for (int s = 0; s < 2; ++s) {
                            in.shadow_rays = s != 0;
                            p[s] = rtp::TracePlan{};
                            rc[s] = rtp::trace_plan(in, occ, &p[s]);
                        }
                        need(rc[0] == rc[1], "the status does not depend on the setting", rc[0], rc[1]);
                        if (rc[0] != RT_SUCCESS || p[0].nothing) {
                            need(p[0].nothing == p[1].nothing, "nothing");
                            ++refused;
                            continue;
                        }
                        need(!p[0].variant.shadow && p[1].variant.shadow, "the variant carries the setting");
                        need(same_but_shadow(p[0], p[1]), "the rest of the plan is the same", nt, (long long)n);
                        need(p[1].variant.slot() == p[0].variant.slot() + rtk::kVariantSlots / 2, "occupancy slot");
                        // the fused sample's plan goes through the same shape
                        rtp::SampleIn si{};
                        si.first = 0, si.n = n > 4096 ? 4096 : n, si.n_pixels = 4096;
                        si.ids_ok = si.stats_ok = true, si.ids_bytes = ~0ull, si.stats_bytes = ~0ull;
                        si.slots_set = true, si.width = 64, si.height = 64;
                        si.scene_bound = si.lights_set = true;
                        rtp::SamplePlan sp[2];
                        int src[2];
                        for (int s = 0; s < 2; ++s) {
                            in.shadow_rays = s != 0;
                            si.scene = in;
                            sp[s] = rtp::SamplePlan{};
                            src[s] = rtp::sample_plan(si, occ, &sp[s]);
                        }
                        need(src[0] == src[1] && src[0] == RT_SUCCESS, "sample status", src[0], src[1]);
                        if (src[0] == RT_SUCCESS && !sp[0].nothing) {
                            need(!sp[0].trace.variant.shadow && sp[1].trace.variant.shadow, "the sample's variant carries it");
                            need(same_but_shadow(sp[0].trace, sp[1].trace) && sp[0].capUnits == sp[1].capUnits, "sample plan the same");
                        }
                        ++plans;
                    }
    need(plans > 1000 && refused > 100, "coverage", plans, refused);
    std::printf("sweep: %lld plan pairs, %lld refused or empty pairs\n", plans, refused);
    return failures;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "slots") return slots() ? 1 : 0;
    if (mode == "sweep") return sweep() ? 1 : 0;
    std::fprintf(stderr, "usage: %s slots|sweep\n", argv[0]);
    return 2;
}

// plan_main.cpp -- stand-alone driver of the launch plan (csrc/rt_launch_plan.cpp), CPU only.
//   plan_main plan   reads one launch per line from stdin ("name=value" tokens: every PlanIn field
//                    -- the knobs of PlanIn::tune by their own names -- occ, occ_s), prints one JSON
//                    line per launch: rc, nothing, every LaunchPlan field (the variant as si, wf,
//                    lds, goct, bofs and var, the slot of the occupancy cache the plan once
//                    indexed), and "inv": the hand-out invariants that plan breaks ("" = none).
//                    tests/test_launch_plan.py compares these with tests/golden/launch_plans.json;
//                    after a deliberate rule change this output regenerates the table.
//   plan_main sweep  plans a sweep of sizes, frames, bands, scene paths and occupancies and checks
//                    the invariants on every accepted plan; exit status 1 if one breaks.
//   plan_main parts  prints RT_COUNTER_PARTS of this build.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>

#include "../../include/rt_status.h"
#include "../../mini-opencl-raytracer_amd/csrc/rt_launch_plan.hpp"
#include "../../mini-opencl-raytracer_amd/csrc/rt_layout.hpp"

#define PLAN_IN_FIELDS(X)                                                                                     \
    X(W) X(H) X(gws) X(range_first) X(range_last) X(n_frames) X(light_bounces) X(sched) X(math) X(stats)     \
    X(hit_bound) X(fused) X(overlap) X(band_period) X(band_phase) X(n_nodes) X(n_tris) X(n_mats) X(n_top)    \
    X(oct_ok) X(goct_available) X(goct_b) X(force_global) X(num_cus)
#define PLAN_TUNE_FIELDS(X)                                                                                   \
    X(global_oct) X(refill_min) X(refill_min_set) X(shade_min) X(refill_min_g) X(shade_min_g) X(w_node)      \
    X(w_leaf) X(w_node_g) X(w_leaf_g) X(chunk_pixels) X(tail_chunk) X(bulk_percent) X(tile_major) X(pf_sky)  \
    X(max_blocks) X(wf_top_limit) X(wf_streams_per_cu) X(wf_refill_min)
#define PLAN_OUT_FIELDS(X)                                                                                    \
    X(smem) X(grid) X(grid_s) X(gidBegin) X(gidEnd) X(rowBegin)    \
    X(rowCount) X(tilesX) X(nTiles) X(bandPeriod) X(bandPhase) X(nTop) X(regrouped) X(octStride) X(octB)     \
    X(octRecords) X(nNodes) X(refillMin) X(shadeMin) X(stepWeightNode) X(stepWeightLeaf) X(flagTiles)        \
    X(tileMajor) X(chunkPixels) X(tailChunk) X(chunkSplit) X(tailBase) X(staticFirst) X(nParts) X(partLen)   \
    X(nFrames) X(radStride) X(need) X(fneed) X(cap) X(G) X(nBlocks) X(wfRefillMin) X(use_pf_sky)             \
    X(pf_slots) X(clear_counter_here) X(own_stream)

// the hand-out invariants of an accepted plan: the names of the broken ones
static std::string broken(const rtp::PlanIn& in, const rtp::LaunchPlan& p) {
    std::string bad;
    auto need = [&](bool ok, const char* name) {
        if (!ok) bad += std::string(bad.empty() ? "" : ",") + name;
    };
    const uint64_t tot = (uint64_t)p.nTiles * 64u * p.nFrames;
    const rtk::Variant& v = p.variant;
    // (the launch once derived this from KernelArgs::octB by itself)
    need((v.walk == rtk::Walk::LdsB) == (v.lds() && p.octB == rtk::kOctB), "b_plane_walk_matches_octB");
    need(p.chunkPixels % 64 == 0 && p.tailChunk % 64 == 0 && p.chunkPixels > 0, "chunks_whole_tiles");
    const uint32_t t = p.tailChunk / 64;
    need(t >= 1 && (t & (t - 1)) == 0 && p.tailChunk <= in.tune.tail_chunk, "tail_pow2_within_cap");
    need(p.chunkPixels > 0 && p.chunkSplit % p.chunkPixels == 0 && p.chunkSplit <= tot, "split_whole_chunks");
    need(p.chunkSplit <= p.tailBase && p.tailBase <= tot, "tail_base_in_range");
    need(!p.staticFirst || p.chunkSplit == 0, "static_first_without_bulk");
    need(p.nParts == 0 || (p.nParts == rtp::counter_parts() && p.nParts <= rtk::kMaxParts && p.partLen % 64 == 0 &&
                           (uint64_t)p.nParts * p.partLen >= tot),
         "partitions_cover");
    const uint64_t work = (uint64_t)p.nTiles * p.nFrames;
    const uint64_t cap = v.sched == rtk::kSchedTiles ? p.nTiles : p.wf() ? (work + 7) / 8 : (work + 3) / 4;
    need(p.grid >= 1 && p.grid <= (cap ? cap : 1), "grid_within_tiles");
    need(tot <= 0xfff00000ull, "work_items_32bit");
    const size_t extras = p.wf() ? (rtk::kWfExtendThreads / 64) * rtk::kWfRingBytes
                               : 4 * rtk::kFinishWaveBytes + 4 * rtk::kRingWaveBytes + rtk::kStealBytes;
    need(!v.lds() || p.smem <= 64 * 1024 + extras, "lds_budget");
    need(!p.wf() || (p.cap == p.nBlocks * 64u && p.G >= 1 && p.G <= p.nBlocks), "wavefront_queues");
    return bad;
}

static int plan_lines() {
    char line[8192];
    while (std::fgets(line, sizeof(line), stdin)) {
        rtp::PlanIn in{};
        long long occ = 0, occ_s = 0;
        std::istringstream ss(line);
        std::string tok;
        int n = 0;
        while (ss >> tok) {
            const size_t eq = tok.find('=');
            if (eq == std::string::npos) return 2;
            const std::string key = tok.substr(0, eq);
            const long long v = std::strtoll(tok.c_str() + eq + 1, nullptr, 10);
            bool known = key == "occ" || key == "occ_s";
            if (key == "occ") occ = v;
            if (key == "occ_s") occ_s = v;
#define X(f) if (key == #f) { in.f = (decltype(in.f))v; known = true; }
            PLAN_IN_FIELDS(X)
#undef X
#define X(f) if (key == #f) { in.tune.f = (decltype(in.tune.f))v; known = true; }
            PLAN_TUNE_FIELDS(X)
#undef X
            if (!known) {
                std::fprintf(stderr, "plan_main: unknown field %s\n", key.c_str());
                return 2;
            }
            ++n;
        }
        if (n == 0) continue;
        rtp::LaunchPlan p;
        const int rc = rtp::plan_launch(in, (int)occ, (int)occ_s, &p);
        std::printf("{\"rc\":%d,\"nothing\":%d", rc, (int)p.nothing);
        if (rc == RT_SUCCESS && !p.nothing) {
            std::printf(",\"inv\":\"%s\",\"out\":{", broken(in, p).c_str());
            const rtk::Variant& pv = p.variant;
            const bool goct = pv.walk == rtk::Walk::GlobalOct, bofs = pv.walk == rtk::Walk::LdsB;
            std::printf("\"si\":%d,\"wf\":%d,\"lds\":%d,\"goct\":%d,\"bofs\":%d,\"var\":%d", pv.sched, (int)p.wf(),
                        (int)pv.lds(), (int)goct, (int)bofs, (bofs || goct ? 1 : 0) + (pv.fused ? 2 : 0));
            const char* sep = ",";
#define X(f) std::printf("%s\"" #f "\":%lld", sep, (long long)p.f); sep = ",";
            PLAN_OUT_FIELDS(X)
#undef X
            std::printf("}");
        }
        std::printf("}\n");
    }
    return 0;
}

static int sweep() {
    static const uint32_t sizes[][2] = {{8, 8},       {64, 64},     {128, 96},    {500, 300},   {512, 512},
                                        {1280, 720},  {1920, 1080}, {1930, 1091}, {2560, 1440}, {3840, 2160}};
    // scene paths: LDS (Cornell-sized), LDS at the budget, octant walk in HBM/L2, global node records
    struct Scene { uint32_t n_nodes, n_tris, n_mats, n_top, goct_b; int global_oct; };
    static const Scene scenes[] = {{21, 36, 8, 21, 176, 1}, {100, 410, 4, 100, 808, 1},
                                   {49471, 70000, 4, 384, 395776, 1}, {49471, 70000, 4, 384, 395776, 0}};
    static const uint32_t periods[] = {1, 2, 3, 8}, tails[] = {64, 128, 256};
    // step per-frame, step deferred / fused, tiles, wavefront
    struct Kind { int sched; bool defer; };
    static const Kind kinds[] = {{rtk::kSchedStep, false}, {rtk::kSchedStep, true}, {rtk::kSchedTiles, false},
                                 {rtk::kSchedWavefront, false}};
    unsigned long long plans = 0, accepted = 0, failures = 0;
    for (const auto& sz : sizes)
    for (const Scene& sc : scenes)
    for (const Kind& kd : kinds)
    for (uint32_t nf = 1; nf <= 8; ++nf)
    for (uint32_t period : periods)
    for (uint32_t phase = 0; phase < period; ++phase)
    for (uint32_t tail : tails)
    for (int occ = 1; occ <= 8; ++occ) {
        if (kd.sched == rtk::kSchedTiles && nf > 1) continue;  // (no fused form: one launch per frame)
        rtp::PlanIn in{};
        in.W = sz[0], in.H = sz[1], in.gws = (uint64_t)sz[0] * sz[1];
        in.n_frames = nf, in.light_bounces = 9, in.sched = kd.sched, in.math = 2;
        in.fused = nf > 1 || kd.defer || kd.sched == rtk::kSchedWavefront;
        in.overlap = true;
        in.band_period = period, in.band_phase = phase;
        in.n_nodes = sc.n_nodes, in.n_tris = sc.n_tris, in.n_mats = sc.n_mats, in.n_top = sc.n_top;
        in.oct_ok = true, in.goct_available = true, in.goct_b = sc.goct_b, in.tune.global_oct = sc.global_oct;
        in.tune.tail_chunk = tail;  // (the other knobs at their defaults)
        in.num_cus = 256;
        rtp::LaunchPlan p;
        const int rc = rtp::plan_launch(in, occ, occ, &p);
        ++plans;
        if (rc == RT_INVALID_OPERATION && kd.sched == rtk::kSchedTiles && period > 1) continue;
        if (rc != RT_SUCCESS) {
            std::printf("unexpected rc %d: %ux%u frames %u\n", rc, in.W, in.H, nf);
            ++failures;
            continue;
        }
        if (p.nothing) continue;
        ++accepted;
        const std::string bad = broken(in, p);
        if (!bad.empty() && ++failures <= 20)
            std::printf("broken [%s]: %ux%u frames %u sched %d fused %d band %u/%u nodes %u goct %d occ %d tail %u\n",
                        bad.c_str(), in.W, in.H, nf, in.sched, (int)in.fused, period, phase, in.n_nodes,
                        in.tune.global_oct, occ, tail);
    }
    std::printf("sweep: %llu plans, %llu accepted, %llu failures\n", plans, accepted, failures);
    return failures ? 1 : 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && std::strcmp(argv[1], "plan") == 0) return plan_lines();
    if (argc == 2 && std::strcmp(argv[1], "sweep") == 0) return sweep();
    if (argc == 2 && std::strcmp(argv[1], "parts") == 0) return std::printf("%u\n", rtp::counter_parts()) < 0;
    std::fprintf(stderr, "usage: plan_main plan|sweep|parts\n");
    return 2;
}

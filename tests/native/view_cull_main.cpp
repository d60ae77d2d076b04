// view_cull_main.cpp -- stand-alone driver of the view-cull rule (csrc/rt_view_cull.cpp) and of the launch
// plan's use of it (csrc/rt_launch_plan.cpp), CPU only; tests/test_view_cull.py builds it with g++ and
// -fsanitize=address,undefined.
//   view_cull_main rect   reads one view per line from stdin: W H, then pos, front, up, bmin, bmax as 15
//                         fp32 bit patterns (hex); prints "all" or "tx0 ty0 tx1 ty1" per line.
//   view_cull_main plan   reads one launch per line ("name=value" tokens: PlanIn fields, the knobs of
//                         PlanIn::tune, occ, occ_s and the rectangle as vtx0 vty0 vtx1 vty1), prints one
//                         JSON line per launch: rc, nothing and every LaunchPlan field.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>

#include "../../include/rt_status.h"
#include "../../mini-opencl-raytracer_amd/csrc/rt_launch_plan.hpp"
#include "../../mini-opencl-raytracer_amd/csrc/rt_view_cull.hpp"

#define PLAN_IN_FIELDS(X)                                                                                     \
    X(W) X(H) X(gws) X(range_first) X(range_last) X(n_frames) X(light_bounces) X(sched) X(math) X(stats)     \
    X(hit_bound) X(fused) X(overlap) X(band_period) X(band_phase) X(n_nodes) X(n_tris) X(n_mats) X(n_top)    \
    X(oct_ok) X(goct_available) X(goct_b) X(force_global) X(num_cus)
#define PLAN_TUNE_FIELDS(X)                                                                                   \
    X(global_oct) X(refill_min) X(refill_min_set) X(shade_min) X(refill_min_g) X(shade_min_g) X(w_node)      \
    X(w_leaf) X(w_node_g) X(w_leaf_g) X(chunk_pixels) X(tail_chunk) X(bulk_percent) X(tile_major) X(pf_sky)  \
    X(max_blocks) X(wf_top_limit) X(wf_streams_per_cu) X(wf_refill_min)
#define PLAN_OUT_FIELDS(X)                                                                                    \
    X(smem) X(grid) X(grid_s) X(gidBegin) X(gidEnd) X(rowBegin)                                               \
    X(rowCount) X(tilesX) X(nTiles) X(bandPeriod) X(bandPhase) X(nTop) X(regrouped) X(octStride) X(octB)     \
    X(octRecords) X(nNodes) X(refillMin) X(shadeMin) X(stepWeightNode) X(stepWeightLeaf) X(flagTiles)        \
    X(tileMajor) X(chunkPixels) X(tailChunk) X(chunkSplit) X(tailBase) X(staticFirst) X(nParts) X(partLen)   \
    X(nFrames) X(radStride) X(need) X(fneed) X(cap) X(G) X(nBlocks) X(wfRefillMin) X(use_pf_sky)             \
    X(pf_slots) X(clear_counter_here) X(own_stream) X(visTx0) X(visTy0) X(visW) X(visH) X(visTiles)

static int rect_lines() {
    char line[1024];
    while (std::fgets(line, sizeof(line), stdin)) {
        std::istringstream ss(line);
        unsigned W = 0, H = 0;
        float f[15];
        if (!(ss >> W >> H)) continue;
        for (float& v : f) {
            std::string tok;
            if (!(ss >> tok)) return 2;
            const uint32_t bits = (uint32_t)std::strtoul(tok.c_str(), nullptr, 16);
            std::memcpy(&v, &bits, 4);
        }
        const rtp::ViewRect r = rtp::view_cull_rect(W, H, f, f + 3, f + 6, f + 9, f + 12);
        if (r.all())
            std::printf("all\n");
        else
            std::printf("%u %u %u %u\n", r.tx0, r.ty0, r.tx1, r.ty1);
    }
    return 0;
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
            bool known = true;
            if (key == "occ") occ = v;
            else if (key == "occ_s") occ_s = v;
            else if (key == "vtx0") in.view.tx0 = (uint32_t)v;
            else if (key == "vty0") in.view.ty0 = (uint32_t)v;
            else if (key == "vtx1") in.view.tx1 = (uint32_t)v;
            else if (key == "vty1") in.view.ty1 = (uint32_t)v;
            else known = false;
#define X(f) if (key == #f) { in.f = (decltype(in.f))v; known = true; }
            PLAN_IN_FIELDS(X)
#undef X
#define X(f) if (key == #f) { in.tune.f = (decltype(in.tune.f))v; known = true; }
            PLAN_TUNE_FIELDS(X)
#undef X
            if (!known) {
                std::fprintf(stderr, "view_cull_main: unknown field %s\n", key.c_str());
                return 2;
            }
            ++n;
        }
        if (n == 0) continue;
        rtp::LaunchPlan p;
        const int rc = rtp::plan_launch(in, (int)occ, (int)occ_s, &p);
        std::printf("{\"rc\":%d,\"nothing\":%d", rc, (int)p.nothing);
        if (rc == RT_SUCCESS && !p.nothing) {
            std::printf(",\"out\":{\"si\":%d", p.variant.sched);
#define X(f) std::printf(",\"" #f "\":%lld", (long long)p.f);
            PLAN_OUT_FIELDS(X)
#undef X
            std::printf("}");
        }
        std::printf("}\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && std::strcmp(argv[1], "rect") == 0) return rect_lines();
    if (argc == 2 && std::strcmp(argv[1], "plan") == 0) return plan_lines();
    std::fprintf(stderr, "usage: view_cull_main rect|plan\n");
    return 2;
}

// rt_launch_plan.cpp -- the launch plan (rt_launch_plan.hpp): the row window and tiles, the scene
// path and its LDS size, the grid, the work order, the bulk / tail split and the counter
// partitions.  Pure arithmetic: a pixel handed out twice or never starts here, so it is kept where
// a CPU test can sweep it (tests/native/plan_main.cpp).
#include "rt_launch_plan.hpp"

#include <algorithm>

#include "../../include/rt_status.h"
#include "rt_layout.hpp"
#include "rt_scene_pack.hpp"

namespace rtp {

namespace {

constexpr size_t kLdsBudget = 64 * 1024;       // per-workgroup LDS the scene path may use
#ifndef RT_STATIC_FIRST
#define RT_STATIC_FIRST 1
#endif
// per-frame launches without a bulk region: tail counters on this many partitions (a power of two, <=
// rtk::kMaxParts; step_body next_chunk_parts) -- 1080p 2-bounce frames 0.172 -> 0.165 ms with 128-pixel
// tail chunks, which on one counter took 0.231 (profiles/r06/work_handout_ab.txt)
#ifndef RT_COUNTER_PARTS
#define RT_COUNTER_PARTS 8
#endif
#ifndef RT_PF_COUNTER_SLOTS
#define RT_PF_COUNTER_SLOTS 1
#endif
// tail chunks: sized so that every `RT_TAIL_SHARE_WAVES` waves get >= 2.5 of them (1: every wave; 4:
// every workgroup, whose waves split the last one by work stealing): fewer atomics on the tail
// counter for small launches (1080p 2-bounce frames 0.282 -> 0.218 ms alone; 4K launches already
// take the largest chunk, profiles/r06/work_handout_ab.txt)
#ifndef RT_TAIL_SHARE_WAVES
#define RT_TAIL_SHARE_WAVES 4
#endif

// floor(a / b), b > 0
int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

}  // namespace

uint32_t counter_parts() { return RT_COUNTER_PARTS; }

int resolve_schedule(int sched, int32_t light_bounces) {
    const bool wf = sched == rtk::kSchedWavefront && light_bounces >= 1 && light_bounces <= rtk::kWfMaxBounces;
    return wf ? rtk::kSchedWavefront : (sched == rtk::kSchedWavefront ? rtk::kSchedStep : sched);
}

int plan_shape(const PlanIn& in, LaunchPlan* out) {
    *out = LaunchPlan{};
    LaunchPlan& a = *out;
    if (in.gws == 0 || in.gws > 0xffffffffull) return RT_INVALID_GLOBAL_WORK_SIZE;
    const int si = resolve_schedule(in.sched, in.light_bounces);
    const bool wf = si == rtk::kSchedWavefront;
    const bool fused = in.fused;
    const uint32_t W = in.W, n_frames = in.n_frames;

    uint64_t g0 = std::min<uint64_t>(in.range_first, in.gws);
    uint64_t g1 = in.range_last ? std::min<uint64_t>(in.range_last, in.gws) : in.gws;
    if (g1 <= g0) {  // nothing in range
        a.nothing = true;
        return RT_SUCCESS;
    }
    a.gidBegin = g0;
    a.gidEnd = g1;
    const uint64_t row0 = g0 / W, row1 = (g1 + W - 1) / W;
    a.rowBegin = (uint32_t)row0;
    a.rowCount = (uint32_t)(row1 - row0);
    const uint32_t tile = si == rtk::kSchedTiles ? 16u : 8u;
    if (in.band_period > 1 && si == rtk::kSchedTiles) return RT_INVALID_OPERATION;
    a.tilesX = (W + tile - 1) / tile;
    uint64_t tilesY = (row1 - row0 + tile - 1) / tile;
    a.bandPeriod = in.band_period;
    a.bandPhase = in.band_phase;
    if (in.band_period > 1) {  // bands phase, phase + period, ... of the row window
        tilesY = tilesY > in.band_phase ? (tilesY - in.band_phase + in.band_period - 1) / in.band_period : 0;
        if (tilesY == 0) {
            a.nothing = true;
            return RT_SUCCESS;
        }
    }
    const uint64_t n_tiles = tilesY * a.tilesX;
    if (n_tiles * 64 > 0xfff00000ull) return RT_INVALID_GLOBAL_WORK_SIZE;
    a.nTiles = (uint32_t)n_tiles;
    a.nFrames = n_frames;
    a.visTx0 = 0u, a.visTy0 = 0u, a.visW = a.tilesX, a.visH = (uint32_t)tilesY, a.visTiles = a.nTiles;
    // The view cull: a fused step launch leaves the tiles outside in.view out of its work -- every
    // sample there is a primary miss, which the accumulation knows without the render (accum_frames_body).
    // Not with stats (the counters see every tile), not with hit buffers bound (each pixel's id and t are
    // written by its path), not with 0 bounces (a sample is then 0, not the sky constant).
    if (RT_VIEW_CULL && !in.view.all() && fused && si == rtk::kSchedStep && !in.stats && !in.hit_bound &&
        in.light_bounces > 0) {
        const uint32_t tx0 = std::min(in.view.tx0, a.tilesX), tx1 = std::min(in.view.tx1, a.tilesX);
        // tile row ty of this launch covers image rows [r, r + 8), r = rowBegin + (ty * period + phase) * 8;
        // the rectangle covers rows [8 * view.ty0, 8 * view.ty1): the bands b = ty * period + phase with
        // r + 8 > 8 * ty0 and r < 8 * ty1, then the ty among them -- an interval
        const int64_t period = std::max<uint32_t>(in.band_period, 1u), phase = in.band_phase;
        const int64_t b0 = floor_div(8 * (int64_t)in.view.ty0 - 8 - (int64_t)row0, 8) + 1;
        const int64_t b1 = floor_div(8 * (int64_t)in.view.ty1 - (int64_t)row0 + 7, 8) - 1;  // inclusive
        const int64_t ty0 = std::max<int64_t>(floor_div(b0 - phase + period - 1, period), 0);
        const int64_t ty1 = std::min<int64_t>(floor_div(b1 - phase, period), (int64_t)tilesY - 1);  // inclusive
        // (no tile of this launch in the rectangle -- a rank whose rows are all sky: it keeps all its tiles)
        if (tx0 < tx1 && ty0 <= ty1) {
            a.visTx0 = tx0, a.visW = tx1 - tx0;
            a.visTy0 = (uint32_t)ty0, a.visH = (uint32_t)(ty1 - ty0 + 1);
            a.visTiles = a.visW * a.visH;
        }
    }
    // The path kill: a step launch ends a path once its throughput is exactly zero -- exact when both
    // halves of the certificate hold (rt_path_kill.cpp).  Not with stats: the counters are the
    // reference's, every segment walked.
    a.pathKill = RT_PATH_KILL && in.tune.path_kill && si == rtk::kSchedStep && !in.stats && in.kill_scene_ok &&
                         path_kill_launch_ok(in.light_type, in.skybox_intensity, in.light_bounces)
                     ? 1u
                     : 0u;
    a.radStride = (uint32_t)g1;
    if (fused) {
        // fused frames: radiance slots indexed by global work-item id (the lane packs
        // slot * g1 + gid into 32 bits); tiles x frames work items
        // (work items stay below 2^32 - 2^20: the work-stealing ranges add a few tiles past
        // their end in 32-bit fields)
        if ((uint64_t)n_frames * g1 > 0xffffffffull || n_tiles * 64 * n_frames > 0xfff00000ull)
            return RT_INVALID_GLOBAL_WORK_SIZE;
        a.need = (size_t)n_frames * g1;
        // frame flags: a byte per (slot, work item), or a 64-bit word per (slot, tile) (flagTiles)
        a.fneed = std::max<size_t>(a.need, (size_t)n_frames * n_tiles * 8u);
        // the set's own render stream (pick_render_stream).  (With hit buffers bound the renders stay
        // in order on the main stream: each writes them.)
        a.own_stream = in.overlap && !in.hit_bound && !wf;
    }

    // LDS: octant node records (8 x 32 B per node), triangles (48 B), shading records
    // (48 B per triangle, 64 B per material); no stack
    const size_t scene_bytes = (size_t)oct_records(in.n_nodes) * 16 + (size_t)in.n_tris * 96 + (size_t)in.n_mats * 64;
    const bool lds = !in.force_global && in.oct_ok && scene_bytes <= kLdsBudget;

    // scenes too large for LDS: the step schedule may walk the octant records in HBM/L2
    // (RT_TUNE_GLOBAL_OCT) instead of the 64-B global node records
    const bool goct = !lds && (wf || si == rtk::kSchedStep) && in.oct_ok && in.tune.global_oct;
    a.nTop = lds || goct ? 0u : in.n_top;  // global path: top-of-tree node records staged in LDS
    a.nNodes = in.n_nodes;
    a.octStride = oct_stride(in.n_nodes);
    a.octB = oct_b(in.n_nodes);
    a.octRecords = oct_records(in.n_nodes);
    if (goct && RT_GOCT_GROUP && in.goct_available && in.goct_b) {
        // regrouped records, links as walk words (build_oct_nodes_grouped)
        a.regrouped = true;
        a.octStride = RT_GOCT_GROUP;
        a.octB = in.goct_b;
        a.octRecords = 2u * a.octB;
        a.nNodes = RT_GOCT_END_WORD ? rtk::kEndWalk : goct_word(in.n_nodes, RT_GOCT_GROUP);  // the END word
    }
    // (octant walk: refill at 32 free lanes under the pixel-major order, 16 before: -0.5 %,
    // profiles/r05/goct_bursts_weights.txt)
    a.refillMin = lds ? in.tune.refill_min : in.tune.refill_min_g ? in.tune.refill_min_g : goct ? 32u : 8u;
    a.shadeMin = lds ? in.tune.shade_min : in.tune.shade_min_g ? in.tune.shade_min_g : 48u;
    a.stepWeightNode = in.tune.w_node;
    a.stepWeightLeaf = in.tune.w_leaf;
    if (!lds) {
        // scenes in HBM/L2: a node step's loads cost more against a triangle step's than in LDS
        // (octant walk under the pixel-major order: 65 / 55 -- 35: +1.0 %, 45: +0.4 %, 80-130 the same;
        // profiles/r05/goct_bursts_weights.txt)
        a.stepWeightNode = in.tune.w_node_g ? in.tune.w_node_g : goct ? 65u : in.tune.w_node;
        a.stepWeightLeaf = in.tune.w_leaf_g ? in.tune.w_leaf_g : in.tune.w_leaf;
    }
    if (wf) a.nTop = std::min(a.nTop, in.tune.wf_top_limit);
    a.smem =
        wf ? (lds ? ((size_t)a.octRecords + 3 * (size_t)in.n_tris) * 16 : (size_t)a.nTop * 64) +
                 (rtk::kWfExtendThreads / 64) * rtk::kWfRingBytes
           : (lds ? scene_bytes : (size_t)a.nTop * 64) +
                 (si == rtk::kSchedStep && !fused ? 4 * rtk::kFinishWaveBytes : 0) +
                 (si == rtk::kSchedStep && lds ? 4 * (fused ? rtk::kRingWaveBytes : rtk::kRingWaveBytesPf) : 0) +
                 (si == rtk::kSchedStep ? rtk::kStealBytes : 0);
    // the step schedule's ray ring (LDS scenes) writes each tile's frame flags as one word at ring
    // fill; the other fused renders write a byte per path at its end
    a.flagTiles = fused && !wf && si == rtk::kSchedStep && lds ? 1u : fused && !wf && si == rtk::kSchedStep && goct ? 2u : 0u;

    const rtk::Walk walk = lds ? (a.octB == rtk::kOctB ? rtk::Walk::LdsB : rtk::Walk::Lds)
                               : (goct ? rtk::Walk::GlobalOct : rtk::Walk::GlobalNodes);
    a.variant = rtk::Variant{si, in.math, walk, in.stats, fused, false};

    // the chunk counters start at zero: per-frame launches clear theirs here; a fused render's
    // (its radiance set's) were cleared by the accumulation that followed the set's previous render
    // (accum_key_body), which this render already waits for -- no clearing launch in front of it
#ifdef RT_DIAG_NO_ACCUM
    const bool clear_here = true;  // (diagnostic builds without the accumulation launch)
#else
    const bool clear_here = !fused;
#endif
    // RT_PF_COUNTER_SLOTS: a per-frame step launch takes one of two counter slots in turn and zeroes
    // the other for the next one (step_body), so no clearing launch sits between consecutive renders
    // (1080p: a 4-us fill and two ~6-us dispatch gaps in a ~0.28-ms frame)
    a.pf_slots = RT_PF_COUNTER_SLOTS && !fused && si == rtk::kSchedStep && !wf;
    a.clear_counter_here = !a.pf_slots && si != rtk::kSchedTiles && !wf && clear_here;
    return RT_SUCCESS;
}

void plan_handout(const PlanIn& in, int occ, int occ_shade, LaunchPlan* out) {
    LaunchPlan& a = *out;
    const int si = a.variant.sched;
    const bool wf = a.wf(), lds = a.variant.lds(), fused = in.fused;
    const uint32_t n_frames = in.n_frames;
    const uint64_t n_tiles = a.visTiles;  // the tiles handed out (all of them unless the view cull applies)
    uint64_t grid = (uint64_t)(in.tune.max_blocks ? std::min(occ, in.tune.max_blocks) : occ) * (uint64_t)in.num_cus;
    // tiles: one workgroup per 16x16 tile at most; persistent schedules: one 8x8 tile per wave
    // (wavefront extend: 8 waves per workgroup)
    grid = std::min<uint64_t>(grid, si == rtk::kSchedTiles ? n_tiles
                                    : wf                   ? (n_tiles * n_frames + 7) / 8
                                                           : (n_tiles * n_frames + 3) / 4);
    if (grid == 0) grid = 1;
    a.grid = grid;
    {
        // bulk chunks only when every resident wave gets at least two of them; a small frame
        // (512x512: ~40 pixels per wave) is handed out 64 pixels at a time
        const uint64_t tot = n_tiles * 64u * n_frames, waves = grid * 4u;
        // fused work order (step_body) on the HBM/L2 scene path: pixel-major when F is a power of two
        // -- a pixel's frames side by side in a wave, so a step's lanes read fewer records: bunny
        // proxy 1.352 -> 1.282 ms/frame, emulated N = 8 rank 1.637 -> 1.535 ms
        // (profiles/r05/pixel_major_ab.txt); else tile-major for large launches (a tile's frames back
        // to back: -1.4 %, profiles/r01/work_order_ab.txt) and frame-major for small ones (tile-major
        // bunches a costly tile's frames into the tail); LDS scenes frame-major (the ray ring)
        // (the pixel-major order is the step schedule's: the wavefront extend launches keep the
        // big / frame-major rule their order was measured with, profiles/r02/wavefront/)
        const bool pow2 = (n_frames == 2 || n_frames == 4 || n_frames == 8) && si == rtk::kSchedStep;
        const bool big = !lds && tot >= 4096u * waves;
        a.tileMajor = n_frames < 2 ? 0u
                      : in.tune.tile_major == 2 ? (!lds && pow2 ? 2u : 1u)
                      : in.tune.tile_major == 1 ? 1u
                      : in.tune.tile_major == 0 ? 0u
                      : !lds && pow2       ? 2u
                      : big                ? 1u
                                           : 0u;
        // the bulk share stops where the tail would hold less than two bulk chunks per wave: a
        // bulk chunk (512 pixel-frames, ~0.25 ms of a wave's time at 4K) taken just before the
        // split otherwise outlasts the tail that should even the waves out -- small launches
        // (multi-GPU ranks: N = 8 renders 1/8 of the frame) get a larger tail (bulk 80 % -> ~37 %:
        // emulated N = 8 rank step, Cornell 1.112 -> 1.047 ms, bunny proxy 1.694 -> 1.629 ms;
        // profiles/r02/multigpu/n8_chunk_sweep_*.txt); full 4K launches keep 80 %
        // bulk chunks of 512 work items, 1024 in the pixel-major order (two whole tiles x 8 frames per
        // fetch: bunny proxy -0.8 %, profiles/r05/goct_bursts_weights.txt)
        const uint32_t chunk = in.tune.chunk_pixels ? in.tune.chunk_pixels : a.tileMajor == 2u ? 1024u : 512u;
        a.chunkPixels = chunk;
        uint64_t bulk = tot * in.tune.bulk_percent / 100;
        const uint64_t reserve = 2u * waves * chunk;
        bulk = std::min<uint64_t>(bulk, tot > reserve ? tot - reserve : 0u);
        a.chunkSplit = tot >= 2u * waves * chunk ? (uint32_t)(bulk / chunk * chunk) : 0u;
        // tail chunks: the largest power-of-two multiple of 64 pixels, up to tail_chunk, that still
        // gives every wave >= 2.5 of them -- few atomics on the tail counter for large launches,
        // fine-grained balance for small ones (4K fused 256, 4K per-frame / 1080p / 512^2 fused 128,
        // 512^2 per-frame 64: profiles/r02/chunk_sweep.txt)
        // (with counter partitions -- per-frame launches without a bulk region, below -- the grabs no
        // longer queue on one address, and the finer per-wave rule balances better)
        const bool parts = RT_COUNTER_PARTS > 1 && RT_STATIC_FIRST && RT_PF_COUNTER_SLOTS && !fused &&
                           si == rtk::kSchedStep && !wf && a.chunkSplit == 0u && grid >= RT_COUNTER_PARTS &&
                           tot >= 256u * waves;  // (512^2 frames, ~50 work items per wave: +5 % with them)
        const uint64_t share = (tot - a.chunkSplit) * (parts ? 1u : RT_TAIL_SHARE_WAVES) / waves;
        uint32_t tail = 64;
        while (tail * 2u <= in.tune.tail_chunk && (uint64_t)tail * 2u * 5u <= share * 2u) tail *= 2u;
        a.tailChunk = tail;
        // RT_STATIC_FIRST: a per-frame launch without a bulk region starts every wave on its own tail chunk,
        // with no atomic (step_body), and the tail counter hands out from past those chunks.  (The
        // same for the bulk region of large launches was 3-5 % slower: the waves then stay in step
        // and meet again at the counter.)
        a.tailBase = a.chunkSplit;
        if (RT_STATIC_FIRST && !fused && si == rtk::kSchedStep && !wf && a.chunkSplit == 0u) {
            a.staticFirst = 1u;
            a.tailBase = (uint32_t)std::min<uint64_t>(waves * tail, tot);
            // RT_COUNTER_PARTS: the tail counter split over that many partitions (with the per-frame
            // counter slots, whose layout holds them)
            if (parts) {
                a.nParts = RT_COUNTER_PARTS;
                a.partLen = (uint32_t)((tot / 64u + RT_COUNTER_PARTS - 1) / RT_COUNTER_PARTS * 64u);
            }
            // such launches (a 1080p frame: ~400 work items per wave) refill at 16 free lanes, not 6:
            // 1080p 2-bounce frames -2.8 % (4K fused launches lose 5 % at 16,
            // profiles/r06/work_handout_ab.txt)
            if (lds && !in.tune.refill_min_set) a.refillMin = 16u;
        }
    }

    // per-frame sky shortcut (step_body): its key costs each wave one gamma step at launch
    // start, which pays off from ~256 pixels per wave (1080p -2.7 %, 4K) and not on small frames
    // (512^2; round 6: the threshold was 1k pixels per wave before the small-launch hand-out,
    // profiles/r06/work_handout_ab.txt)
    a.use_pf_sky = !fused && si == rtk::kSchedStep &&
                   (in.tune.pf_sky == 2 || (in.tune.pf_sky == 1 && a.gidEnd - a.gidBegin >= 256u * 4u * grid));
    if (wf) {
        // queues for every (frame slot, work-item) of the launch, streams of 64-entry blocks
        const uint64_t blocks = n_tiles * n_frames;
        // streams: by default one per shade workgroup the GPU holds at once, so the shade
        // launch is a single round of workgroups (no second, partly empty round)
        const uint64_t per_cu = in.tune.wf_streams_per_cu ? in.tune.wf_streams_per_cu : (uint64_t)occ_shade;
        a.cap = (uint32_t)(blocks * 64);
        a.G = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(blocks, (uint64_t)in.num_cus * per_cu));
        a.nBlocks = (uint32_t)blocks;
        a.wfRefillMin = in.tune.wf_refill_min;
        a.grid_s = a.G;  // one workgroup per stream
    }
}

}  // namespace rtp

// rt_scene_pack.hpp -- host-side scene validation and record packing (rt_scene_pack.cpp): what
// turns a malformed scene into an error code, never a wild GPU walk.  No HIP here.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/rt_cl_types.h"
#include "rt_layout.hpp"

namespace rtp {

// leaf codes (count << 24 | first, count 1..127) start here; node indices stay below
constexpr uint32_t kLeafMin = 1u << 24;

// records per octant plane: the n nodes, the END sentinel, and one pad record when that count is
// even -- an odd plane stride (x 16 B) staggers the eight planes over the LDS banks, so lanes of
// different octants at the same node do not collide (an even stride of 40 put planes o and o+2
// on the same banks: +40 % bank-conflict cycles)
inline uint32_t oct_stride(uint32_t n) { return (n + 1) | 1u; }
// float4 offset of the B planes: rtk::kOctB for trees of at most kOctBMaxStride records per plane
// (a node step then reads B at an immediate offset from A), else right after the A planes
inline uint32_t oct_b(uint32_t n) {
    return oct_stride(n) <= rtk::kOctBMaxStride ? rtk::kOctB : 8u * oct_stride(n);
}
inline uint32_t oct_records(uint32_t n) { return oct_b(n) + 8u * oct_stride(n); }

#ifndef RT_NODE_COLLAPSE
#define RT_NODE_COLLAPSE 1  // launches without counters walk the collapsed links (collapse_oct_links)
#endif
#ifndef RT_OCTANT_CULL
#define RT_OCTANT_CULL 1  // ... and the pruned links (prune_oct_links), which contain the collapse
#endif
#ifndef RT_GATE_SKIP
#define RT_GATE_SKIP 1  // ... in the gate-skipped form of both (gate_skip_oct_links; needs RT_NODE_COLLAPSE)
#endif
// how select_gate_skips chooses the removed interior nodes: 0 the SAH programme, 1 the plain area ratio
// (RT_GATE_RATIO_PCT / 100 and above), kept for comparison (profiles/r14/removed_visits.txt)
#ifndef RT_GATE_SELECT
#define RT_GATE_SELECT 0
#endif
#ifndef RT_GATE_RATIO_PCT
#define RT_GATE_RATIO_PCT 90
#endif
#ifndef RT_GOCT_GROUP
#define RT_GOCT_GROUP 1  // node-major: bunny proxy fused 1.405 -> 1.393 ms/frame (profiles/r03/goct_layout_ab.txt)
#endif
// walk word of node i in the regrouped records (build_oct_nodes_grouped)
inline uint32_t goct_word(uint32_t i, uint32_t G) { return (i / G) * 8u * G + i % G; }

// (see rt_scene_pack.cpp for each one's contract)
int check_nodes(const rt_cl_bvh_node* nd, uint32_t n, uint32_t n_tris, int* depth_out, uint32_t* n_used);
void build_skips(const rt_cl_bvh_node* nd, uint32_t n, std::vector<uint32_t>& skips);
bool build_oct_nodes(const rt_cl_bvh_node* nd, uint32_t n, const std::vector<uint32_t>& skips,
                     std::vector<uint32_t>& out);
void build_oct_nodes_grouped(const std::vector<uint32_t>& oct, uint32_t n, uint32_t G, std::vector<uint32_t>& out,
                             uint32_t* b_ofs);
uint32_t collapse_oct_links(const std::vector<uint32_t>& oct, uint32_t n, std::vector<uint32_t>& out);
uint32_t prune_oct_links(const std::vector<uint32_t>& oct, const std::vector<uint32_t>& base, uint32_t n,
                         const uint8_t* tri_octants, std::vector<uint32_t>& out);
bool boxes_nest(const rt_cl_bvh_node* nd, uint32_t n);
void select_gate_skips(const rt_cl_bvh_node* nd, uint32_t n, std::vector<uint8_t>& removed);
uint32_t gate_skip_oct_links(const std::vector<uint32_t>& oct, uint32_t n, const std::vector<uint8_t>& removed,
                             std::vector<uint32_t>& out);
void build_global_nodes(const rt_cl_bvh_node* nd, uint32_t n, const std::vector<uint32_t>& skips,
                        uint32_t top, std::vector<uint32_t>& out, uint32_t* n_top,
                        std::vector<uint32_t>* slot_of = nullptr);
void build_refit_links(const rt_cl_bvh_node* nd, uint32_t n, const std::vector<uint32_t>& slot_of,
                       std::vector<uint32_t>& out);

// The bytes of the caller's three scene buffers (mats null: nothing is bound, as for ray queries).
struct SceneBytes {
    const uint8_t* tris = nullptr;
    size_t tris_size = 0;
    const uint8_t* nodes = nullptr;
    size_t nodes_size = 0;
    const uint8_t* mats = nullptr;
    size_t mats_size = 0;
};

// Everything the host derives from a validated scene: what rti::DeviceScene uploads and remembers.
struct HostPack {
    uint32_t n_nodes = 0, n_tris = 0, n_mats = 0;
    int depth = 0;
    uint32_t n_top = 0;   // global records staged in LDS
    bool oct_ok = false;  // every leaf fits the octant records' inline {first, count}
    uint32_t goct_b = 0;  // float4 offset of the regrouped records' B planes (0: none)
    std::vector<uint32_t> global_nodes, refit_links, oct_nodes;
    std::vector<uint32_t> goct_nodes;  // empty when the scene has none
    // the collapsed link set (collapse_oct_links) of both octant layouts: empty when it changes no link
    // word (collapsed_links 0) -- the plain records then serve as both sets
    uint32_t collapsed_links = 0;
    std::vector<uint32_t> oct_nodes_collapsed, goct_nodes_collapsed;
    // the pruned link set (prune_oct_links over the collapsed set, so it contains the collapse) of both
    // layouts, filled by pack_pruned_links: empty when the pruning changes no link word (pruned_links 0)
    // -- the collapsed records then serve
    uint32_t pruned_links = 0;
    std::vector<uint32_t> oct_nodes_pruned, goct_nodes_pruned;
    // The gate-skipped link set (gate_skip_oct_links), which contains the collapse.  nested: the tree holds
    // the certificate (boxes_nest); gate_removed: the interior nodes no link of the set leads to, one byte per
    // node (empty without the certificate); gate_links: the link words the set changes against the plain
    // one.  The records are empty where the certificate is refused and where the set is word for word the
    // collapsed one -- the collapsed records (or the plain ones) then serve.  Where they exist a launch walks
    // them in place of the collapsed set, and their own pruned form (pack_pruned_links: prune_oct_links over
    // them; gated_pruned_links words against them, records empty when 0) in place of the pruned one.
    bool nested = false;
    std::vector<uint8_t> gate_removed;
    uint32_t gate_links = 0;
    std::vector<uint32_t> oct_nodes_gated, goct_nodes_gated;
    uint32_t gated_pruned_links = 0;
    std::vector<uint32_t> oct_nodes_gated_pruned, goct_nodes_gated_pruned;
};

// Validate the scene and pack every record (top_limit: build_global_nodes' `top`).  On an error
// `out` holds nothing to be used.
int pack_scene_host(const SceneBytes& in, uint32_t top_limit, HostPack* out);
// The third record set of a scene pack_scene_host accepted: tri_octants[t] (n_tris bytes) holds for
// triangle t the octants whose every ray fails its test (rt_octant_cull.hpp: the caller evaluates the
// certificate, this file stays free of it), and its twin over the gate-skipped set where the scene has one.
// Nothing in a build with RT_OCTANT_CULL=0.
void pack_pruned_links(const uint8_t* tri_octants, HostPack* pack);

}  // namespace rtp

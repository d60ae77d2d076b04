// rt_device_scene.hpp -- the packed scene a kernel's launches read: the device records derived from
// the caller's triangle, node and material buffers, which buffers (and which of their generations)
// they were derived from, and the one rule that decides when they are stale.  Nothing is launched on a
// scene the host has not validated (rt_scene_pack.cpp): prepare() runs before every launch and every
// query, and refit() skips the validation only while nothing structural was written since the last one.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_internal.hpp"

namespace rti {

class DeviceScene {
public:
    // nodes of the global records staged in LDS (RT_TUNE_TOP_NODES; swept,
    // profiles/r01/bunny_top_nodes_sweep_2.txt).  A change renumbers the records: invalidate()
    uint32_t top_limit = 384;

    // The records are those of `tris`, `nodes` and `mats` as they are now: returns at once when they
    // already are, else validates and packs on the host, uploads, and only then remembers the buffers.
    // mats null (ray queries without a material buffer): no material is packed and no material index
    // checked; a later call with materials packs and checks again.
    int prepare(rt_context ctx, rt_mem tris, rt_mem nodes, rt_mem mats);
    // Bounds from the moved triangles on the device, into `nodes` and every record (rt_refit.hip); a
    // full prepare() first unless the scene is structurally current.  Materials stay as packed.
    int refit(rt_context ctx, rt_mem tris, rt_mem nodes, rt_mem mats);
    // the next prepare() or refit() prepares in full
    void invalidate() { for_nodes_ = nullptr; }
    void release();

    uint32_t n_nodes() const { return n_nodes_; }
    uint32_t n_tris() const { return n_tris_; }
    uint32_t n_mats() const { return n_mats_; }
    uint32_t n_top() const { return n_top_; }
    bool oct_ok() const { return oct_ok_; }  // every leaf fits the octant records' inline {first, count}
    uint32_t goct_b() const { return goct_b_; }  // the regrouped records' B planes (float4 offset)
    const float4* packed_tris() const { return packed_tris_; }
    const float4* shade_tris() const { return shade_tris_; }  // compact shading records (normals + mtlIndex)
    // compact materials, two tables of n_mats: IEEE divisions (pinned, devicelib), then the shipped policy's
    const float4* shade_mats() const { return shade_mats_; }
    const float4* oct_nodes() const { return oct_nodes_; }    // [node][octant] 2 x float4 (LDS-resident scenes)
    const float4* g_nodes() const { return g_nodes_; }        // 64-B node records, top of the tree first
    // regrouped octant records for the HBM/L2 walk (RT_GOCT_GROUP), null when this scene has none
    const float4* goct() const { return goct_b_ ? goct_nodes_ : nullptr; }
    // The collapsed link set (rtp::collapse_oct_links): the same records with the octant walk's links
    // past near children whose box is bitwise their parent's.  collapse_ok(): the set may be walked --
    // the boxes are as the host packed them.  False after a device refit, which rewrites planes and no
    // links and leaves the equality unknown, like root_bounds(), until the next full preparation; false
    // throughout in a build with RT_NODE_COLLAPSE=0.  A launch that reports traversal counters walks
    // the plain set whatever this says.  The two accessors return the plain records where the set
    // changes no link word.
    bool collapse_ok() const { return collapse_known_; }
    uint32_t collapsed_links() const { return collapsed_links_; }  // link words the set changes
    const float4* oct_nodes_collapsed() const { return has_collapsed_ ? oct_collapsed_ : oct_nodes_; }
    const float4* goct_collapsed() const { return has_collapsed_ && goct_b_ ? goct_collapsed_ : goct(); }
    // The gate-skipped link set (rtp::gate_skip_oct_links), which contains the collapse: where the scene
    // has one (its boxes nest, and it differs from the collapsed set) the two accessors above return it in
    // the collapsed set's place, and the two below its own pruned form, under the same conditions --
    // collapse_ok() and cull_ok() -- since a device refit leaves the nesting unknown like the equality.
    // gate_links(): the link words it changes against the plain set (0: no certificate, or a build with
    // RT_GATE_SKIP=0); gate_skipped(): launches that walk "the collapsed links" walk these.
    uint32_t gate_links() const { return gate_links_; }
    bool gate_skipped() const { return gate_skipped_; }
    // The pruned link set (rtp::prune_oct_links over the collapsed set): per octant, no link leads to a
    // subtree whose triangles every ray of the octant rejects (rt_octant_cull.hpp).  cull_ok(): the set
    // may be walked -- triangles and boxes are as the host saw them at the last full preparation.  False
    // after a device refit (rtRefitBVH, rtEnqueueUpdateVertices), which moves vertices without the host
    // looking, until the next full preparation; false throughout in a build with RT_OCTANT_CULL=0.  A
    // launch that reports traversal counters never walks it.  The two accessors return the collapsed
    // accessors' records where the pruning changes no link word.
    bool cull_ok() const { return cull_known_; }
    uint32_t pruned_links() const { return pruned_links_; }  // link words the pruning changes
    const float4* oct_nodes_pruned() const { return has_pruned_ ? oct_pruned_ : oct_nodes_collapsed(); }
    const float4* goct_pruned() const { return has_pruned_ && goct_b_ ? goct_pruned_ : goct_collapsed(); }
    // The root node's bounds (nodes[0]: min xyz, max xyz) as the host last saw them: read at every full
    // preparation, so a launch after a vertex or node write sees the new ones.  Null after a device
    // refit, which moves them without the host looking: such launches do without the view cull.
    const float* root_bounds() const { return root_known_ ? root_bounds_ : nullptr; }
    // The path-kill certificate's scene half (rt_path_kill.hpp) for the material table of `shipped`
    // math or the IEEE one, evaluated at every full preparation with materials.  False where it was
    // refused and where it is unknown: after a device refit, which moves vertices and normals without
    // the host looking, like root_bounds().
    bool path_kill_ok(bool shipped) const { return kill_known_ && kill_ok_[shipped ? 1 : 0]; }
    // rtDiagScenePrepares
    uint64_t full_prepares() const { return full_prepares_; }
    uint64_t refits() const { return refits_; }

private:
    // a bound buffer, or its contents, differ from what the records were packed from
    bool stale(rt_mem tris, rt_mem nodes, rt_mem mats) const {
        return for_tris_ != tris || tris_gen_ != tris->generation || for_nodes_ != nodes ||
               nodes_gen_ != nodes->generation || (mats && (for_mats_ != mats || mats_gen_ != mats->generation));
    }
    // The stricter rule of the refit, which validates nothing: the records come from these buffers and
    // no writer that may change topology or material indices has touched them since the last full
    // preparation (rt_mem_s::structural).  Positions, normals and bounds may have moved.
    bool structurally_current(rt_mem tris, rt_mem nodes) const {
        return for_tris_ == tris && for_nodes_ == nodes && tris_struct_ == tris->structural &&
               nodes_struct_ == nodes->structural;
    }
    int allocate(uint32_t n_nodes, uint32_t n_tris, uint32_t n_mats, size_t goct_words, bool collapsed, bool pruned);

    // provenance: the buffers packed from, their generations then, their structural generations at
    // the last full preparation
    rt_mem for_tris_ = nullptr, for_nodes_ = nullptr, for_mats_ = nullptr;
    uint64_t tris_gen_ = 0, nodes_gen_ = 0, mats_gen_ = 0;
    uint64_t tris_struct_ = 0, nodes_struct_ = 0;
    uint32_t n_nodes_ = 0, n_tris_ = 0, n_mats_ = 0, n_top_ = 0, goct_b_ = 0;
    bool oct_ok_ = false;
    bool root_known_ = false;
    float root_bounds_[6] = {};
    bool collapse_known_ = false;
    uint32_t collapsed_links_ = 0;
    bool cull_known_ = false;
    uint32_t pruned_links_ = 0;
    uint32_t gate_links_ = 0;
    bool gate_skipped_ = false;
    bool has_collapsed_ = false, has_pruned_ = false;  // the two pairs of copies below hold a set
    bool kill_known_ = false;
    bool kill_ok_[2] = {false, false};  // [0] the IEEE material table, [1] the shipped policy's
    uint64_t full_prepares_ = 0, refits_ = 0;
    // device records and their capacities (float4s)
    float4 *packed_tris_ = nullptr, *shade_tris_ = nullptr, *shade_mats_ = nullptr;
    float4 *oct_nodes_ = nullptr, *goct_nodes_ = nullptr, *g_nodes_ = nullptr;
    size_t packed_tris_cap_ = 0, shade_tris_cap_ = 0, shade_mats_cap_ = 0;
    size_t oct_nodes_cap_ = 0, goct_nodes_cap_ = 0, g_nodes_cap_ = 0;
    // the collapsed copies of the two octant layouts (allocated for scenes whose set changes a link), or
    // the gate-skipped ones
    float4 *oct_collapsed_ = nullptr, *goct_collapsed_ = nullptr;
    size_t oct_collapsed_cap_ = 0, goct_collapsed_cap_ = 0;
    // ... and the pruned copies of whichever they hold (for scenes whose pruning changes a link)
    float4 *oct_pruned_ = nullptr, *goct_pruned_ = nullptr;
    size_t oct_pruned_cap_ = 0, goct_pruned_cap_ = 0;
    // device refit: node -> parent, then node -> g_nodes record (n_nodes words each), uploaded by the
    // full preparation; the climb's arrival counters
    uint32_t *refit_links_ = nullptr, *refit_arrivals_ = nullptr;
    size_t refit_links_cap_ = 0, refit_arrivals_cap_ = 0;
};

}  // namespace rti

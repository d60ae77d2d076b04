// rt_scene_pack.cpp -- validation of the flattened BVH and the node records packed from it.
// Pure host code (no HIP): rti::DeviceScene (rt_device_scene.cpp) owns the device buffers and the copies.
#include "rt_scene_pack.hpp"

#include <algorithm>
#include <cstring>
#include <limits>

#include "../../include/rt_status.h"

namespace rtp {

// Validate the flattened BVH (CLBVHnode.cpp:161-183 contract) and return its depth and its
// node count.  The tree is the prefix [0, end) of the array: in the depth-first layout (first
// child = parent + 1, second child after the first child's subtree) the root's subtree ends
// after the leaf its chain of second children reaches.  Nodes past `end` are never read -- by
// the reference's walk from node 0 either -- so a buffer may be larger than the tree it holds
// (rtBuildBVH writes `count` nodes into a buffer of 2n-1).  Within the tree every node is
// checked and each one but the root must have exactly one parent; since a parent's index is
// smaller than its children's, that makes every node reachable from node 0 and the
// skip-pointer walk a finite depth-first order (a child shared by two parents would make it
// loop).
int check_nodes(const rt_cl_bvh_node* nd, uint32_t n, uint32_t n_tris, int* depth_out, uint32_t* n_used) {
    if (n == 0) return RT_INVALID_MEM_OBJECT;
    uint32_t last = 0;  // the root's chain of second children (offsets strictly increase)
    while (nd[last].nPrimitives == 0) {
        if (nd[last].offset <= last || nd[last].offset >= n) return RT_INVALID_MEM_OBJECT;
        last = nd[last].offset;
    }
    n = last + 1;
    std::vector<int> depth(n, -1);
    std::vector<uint8_t> parents(n, 0);
    depth[0] = 0;
    int max_depth = 0;
    // children have larger indices than their parent, so one forward sweep sets depths
    for (uint32_t i = 0; i < n; ++i) {
        const rt_cl_bvh_node& x = nd[i];
        if (i > 0 && parents[i] != 1) return RT_INVALID_MEM_OBJECT;  // orphan: unreachable
        if (x.nPrimitives > 0) {
            if ((uint64_t)x.offset + x.nPrimitives > n_tris) return RT_INVALID_MEM_OBJECT;
            max_depth = std::max(max_depth, depth[i]);
        } else {
            if (x.axis > 2) return RT_INVALID_MEM_OBJECT;
            const uint64_t a = (uint64_t)i + 1, b = x.offset;
            if (a >= n || b >= n || b <= a) return RT_INVALID_MEM_OBJECT;
            if (parents[a]++ != 0 || parents[b]++ != 0) return RT_INVALID_MEM_OBJECT;  // shared child
            depth[a] = depth[i] + 1;
            depth[b] = depth[i] + 1;
        }
    }
    *depth_out = max_depth;
    *n_used = n;
    // The reference's 64-entry stack (kernel_bvh.cl:181) would overflow past depth 64; the
    // stackless walk here has no such limit, so deeper trees are rendered, not rejected.
    return RT_SUCCESS;
}

// Per-octant skip pointers (see rt_kernels.hip, intersect): for octant o (bit i = the ray
// direction's sign on axis i) the reference visits an interior node's second child first
// when bit axis(n) is set (kernel_bvh.cl:200-207).  skip[n][o] is the node the reference
// pops after finishing n's subtree: near child -> far child, far child -> skip of parent.
// Children have larger indices than their parent, so one forward sweep fills the table.
void build_skips(const rt_cl_bvh_node* nd, uint32_t n, std::vector<uint32_t>& skips) {
    skips.assign((size_t)n * 8, 0xffffffffu);
    for (uint32_t i = 0; i < n; ++i) {
        if (nd[i].nPrimitives > 0) continue;
        const uint32_t first = i + 1, second = nd[i].offset;
        for (uint32_t o = 0; o < 8; ++o) {
            const bool swap = (o >> nd[i].axis) & 1u;
            const uint32_t nearc = swap ? second : first, farc = swap ? first : second;
            skips[(size_t)nearc * 8 + o] = farc;
            skips[(size_t)farc * 8 + o] = skips[(size_t)i * 8 + o];
        }
    }
}

// Octant-resolved node records for LDS-resident scenes (stored as 16 planes of float4:
// A[octant][node], then B[octant][node], each plane n + 1 records): for node i and ray
// octant o,
//   A = {near.x, near.y, near.z, far.x}, B = {far.y, far.z, hit_next, miss_next}
// where near/far are the slab planes kernel_bvh.cl:156-169 selects by the ray's signs
// (bit-exact copies of pmin/pmax), miss_next = skip[i][o] and hit_next is the near child
// (interior, < 2^24) or the leaf code count << 24 | first (count 1..127).  The reference's
// "stack empty" is record n, a sentinel every ray misses (its near planes are +inf along the
// octant's direction, so t0 = +inf) whose successors are n itself: a finished walk parks
// there, and the kernel needs no end test per step.  A node step is two b128 reads, the slab
// arithmetic and two selects.  Returns false when a leaf does not fit (> 127 primitives or
// first + count > 2^24): such a scene is rendered from the global layout instead (LDS scenes
// are small, so this takes an unusual hand-made BVH).
bool build_oct_nodes(const rt_cl_bvh_node* nd, uint32_t n, const std::vector<uint32_t>& skips,
                     std::vector<uint32_t>& out) {
    const uint32_t stride = oct_stride(n), bofs = oct_b(n);
    out.assign((size_t)oct_records(n) * 4, 0u);
    bool ok = n < kLeafMin;
    auto bits = [](float f) {
        uint32_t u;
        std::memcpy(&u, &f, 4);
        return u;
    };
    const float inf = std::numeric_limits<float>::infinity();
    for (uint32_t i = 0; i <= n; ++i) {
        uint32_t leaf = 0;
        float lo[3], hi[3];
        if (i < n) {
            const rt_cl_bvh_node& x = nd[i];
            if (x.nPrimitives > 0) {
                if (x.nPrimitives <= 127 && (uint64_t)x.offset + x.nPrimitives <= kLeafMin)
                    leaf = ((uint32_t)x.nPrimitives << 24) | x.offset;
                else
                    ok = false;
            }
            lo[0] = x.bounds.pmin.x, lo[1] = x.bounds.pmin.y, lo[2] = x.bounds.pmin.z;
            hi[0] = x.bounds.pmax.x, hi[1] = x.bounds.pmax.y, hi[2] = x.bounds.pmax.z;
        } else {
            // END sentinel: near plane +inf (octant bit clear: near = pmin) or -inf (set: near =
            // pmax), i.e. lo = +inf, hi = -inf -- (near - o) * invDir = +inf on every axis
            for (int ax = 0; ax < 3; ++ax) lo[ax] = inf, hi[ax] = -inf;
        }
        for (uint32_t o = 0; o < 8; ++o) {
            // octant-major planes A[o][node], B[o][node] (16 B each): lanes visiting different
            // nodes in the same octant hit different LDS banks
            uint32_t* ra = &out[((size_t)o * stride + i) * 4];
            uint32_t* rb = &out[((size_t)bofs + (size_t)o * stride + i) * 4];
            float nr[3], fr[3];
            for (int ax = 0; ax < 3; ++ax) {
                const bool neg = (o >> ax) & 1u;
                nr[ax] = neg ? hi[ax] : lo[ax];
                fr[ax] = neg ? lo[ax] : hi[ax];
            }
            ra[0] = bits(nr[0]);
            ra[1] = bits(nr[1]);
            ra[2] = bits(nr[2]);
            ra[3] = bits(fr[0]);
            rb[0] = bits(fr[1]);
            rb[1] = bits(fr[2]);
            if (i == n) {
                rb[2] = rb[3] = n;
                continue;
            }
            const uint32_t skip = skips[(size_t)i * 8 + o];
            rb[2] = nd[i].nPrimitives > 0 ? leaf : (((o >> nd[i].axis) & 1u) ? nd[i].offset : i + 1);
            rb[3] = skip == 0xffffffffu ? n : skip;
        }
    }
    return ok;
}

// The collapsed link set: a copy of build_oct_nodes' records `oct` (n nodes, every leaf inline: the
// caller passes records whose build returned true) that differs only in hit_next words of interior
// records, and the number of words it changes.  For node i and octant o the plain hit_next is the near
// child c.  While c is interior and its box is bitwise i's, the link moves on to c's own near child
// under o; the chain ends at the first node whose box differs, or at a leaf.
//
// Why a walk over these links computes what the plain walk computes.  A walk that follows i's hit_next
// has just passed i's box test for its ray and its current t.  Its next step is c's box test: no
// triangle is tested between the two node steps, so t is the same word, and the ray is the same ray.
// The test reads the six planes the record holds for the ray's octant; when c's six words equal i's it
// is the same arithmetic on the same operands as the test just passed -- comparisons against t and NaN
// slabs of axis-aligned rays included, whatever their outcome rule -- so it passes, every time, and the
// plain walk goes on to c's hit_next.  Going there at once leaves out a step whose result was known
// when the scene was packed, and nothing else: c's miss_next is never taken (its test cannot fail), and
// the nodes below c keep their own records, whose miss_next words already lead to c's far child and
// from there out of c's subtree.  By induction over the chain, every leaf entered, every triangle
// tested and the final {t, prim} are the plain walk's, in its order; only the visit count is smaller,
// by one per skipped node per passage.  That holds for closest-hit and any-hit walks alike, which differ
// in what a triangle step does, not in the node steps.
//   * Words are compared as uint32_t.  +0.0 and -0.0 planes differ as words and do not collapse:
//     (plane - o) * invDir may differ in sign or be NaN for one and not the other, and the argument
//     above needs the same operands, not equal values.  (Two NaN planes with the same word would
//     collapse, rightly: the same operands again.)
//   * For one octant the near/far selection is the same for i and c, so comparing the record's six
//     plane words under o is comparing pmin and pmax, all six words.
//   * A leaf is never skipped, identical box or not: on entering a leaf the kernels take the walk's
//     continuation from the visited record's miss_next, and i's is not the leaf's.  The leaf keeps its
//     own visit.
//   * The END sentinel and every word other than an interior hit_next -- A planes, the far planes in B,
//     leaf codes, miss_next -- are the plain set's, word for word.
// The equality is a property of the planes as packed: a device refit rewrites planes and no links, so
// after one only the plain set may be walked until the next full preparation (rti::DeviceScene).
uint32_t collapse_oct_links(const std::vector<uint32_t>& oct, uint32_t n, std::vector<uint32_t>& out) {
    const uint32_t stride = oct_stride(n), bofs = oct_b(n);
    out = oct;
    uint32_t changed = 0;
    for (uint32_t o = 0; o < 8; ++o) {
        const uint32_t* pa = &oct[(size_t)o * stride * 4];
        const uint32_t* pb = &oct[((size_t)bofs + (size_t)o * stride) * 4];
        auto same_box = [&](uint32_t x, uint32_t y) {
            return std::memcmp(pa + (size_t)x * 4, pa + (size_t)y * 4, 16) == 0 &&
                   std::memcmp(pb + (size_t)x * 4, pb + (size_t)y * 4, 8) == 0;
        };
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t near0 = pb[(size_t)i * 4 + 2];
            if (near0 >= kLeafMin) continue;  // i is a leaf: its code stays
            // (children have larger indices than their parent: the chain is finite)
            uint32_t c = near0;
            while (pb[(size_t)c * 4 + 2] < kLeafMin && same_box(i, c)) c = pb[(size_t)c * 4 + 2];
            if (c != near0) {
                out[((size_t)bofs + (size_t)o * stride + i) * 4 + 2] = c;
                ++changed;
            }
        }
    }
    return changed;
}

// The pruned link set: a copy of `base` -- the collapsed set, or the plain one where the collapse changes
// nothing -- in which, per octant, no link leads to a subtree whose triangles every ray of that octant
// rejects; returns the number of words it changes.  `oct` is the plain set of the same scene (n nodes,
// every leaf inline), which still shows the tree: node i's near child under o is its plain hit_next c,
// its far child is c's miss_next.  tri_octants[t] bit o: triangle t is certified for octant o
// (rt_octant_cull.hpp: every evaluation of its test on a ray of octant o rejects or is NaN).
//   * A leaf is culled under o when every triangle of it is certified for o; an interior node when both
//     children are.  (Children have larger indices: one backward sweep.)
//   * Every hit_next or miss_next word of octant o that targets a culled node x is replaced by x's own
//     miss_next, repeated while the target is culled.  miss_next words strictly advance in the octant's
//     depth-first order and END is never culled, so the chain ends.
// Why a walk over these links computes what the walk over `base` computes.  A walk that arrives at a
// culled leaf x either fails x's box test and goes to x's miss_next, or passes it, tests x's triangles --
// each test accepts nothing, by the certificate, so {t, prim, u, v} are what they were -- and goes to the
// visited record's miss_next: the same word.  A walk that arrives at a culled interior node x leaves
// through x's miss_next if the box fails; if it passes, every leaf below x is culled, t does not change,
// and every way through the subtree ends at the skip of x's subtree, which is x's miss_next again.  So the
// state after x is the state before x with the position moved to x's miss_next, whatever the ray does:
// going there at once leaves out x's box test and every triangle test below x, all of which accept
// nothing, and nothing else.  That holds for closest-hit and any-hit walks alike (an any-hit walk ends at
// an accepted test; none is removed).  By induction over the replaced words the triangle tests that
// remain are the base walk's in its order, and the final {t, prim, u, v} are its bits.
//   * The collapsed links in `base` stay valid: a collapsed hit_next i -> c stands for box tests known to
//     pass; if c is culled the argument above applies to the arrival at c.
//   * If the root is culled under o, octant o's links stay as they are (a walk must start somewhere; such
//     a scene shows that octant nothing and is not worth a special entry).
//   * Planes, leaf codes and END are base's, word for word; a partly culled leaf keeps its whole code.
// The certificate is a property of the triangles as the host saw them, and the collapse of the boxes: after
// a device refit or a vertex update only the plain set may be walked until the next full preparation.
uint32_t prune_oct_links(const std::vector<uint32_t>& oct, const std::vector<uint32_t>& base, uint32_t n,
                         const uint8_t* tri_octants, std::vector<uint32_t>& out) {
    const uint32_t stride = oct_stride(n), bofs = oct_b(n);
    out = base;
    uint32_t changed = 0;
    std::vector<uint8_t> culled(n);
    for (uint32_t o = 0; o < 8; ++o) {
        const size_t plane = ((size_t)bofs + (size_t)o * stride) * 4;
        const uint32_t* pb = &oct[plane];
        for (uint32_t i = n; i-- > 0;) {
            const uint32_t hn = pb[(size_t)i * 4 + 2];
            if (hn >= kLeafMin) {
                const uint32_t first = hn & (kLeafMin - 1), count = hn >> 24;
                bool all = true;
                for (uint32_t t = first; t < first + count; ++t) all = all && ((tri_octants[t] >> o) & 1u);
                culled[i] = all;
            } else {
                const uint32_t farc = pb[(size_t)hn * 4 + 3];  // the near child's skip: the far child
                culled[i] = culled[hn] && farc < n && culled[farc];
            }
        }
        if (culled[0]) continue;
        auto live = [&](uint32_t x) {
            while (x < n && culled[x]) x = pb[(size_t)x * 4 + 3];
            return x;
        };
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t k = 2; k < 4; ++k) {
                uint32_t& w = out[plane + (size_t)i * 4 + k];
                if (w >= kLeafMin) continue;  // a leaf code
                const uint32_t to = live(w);
                if (to != w) {
                    w = to;
                    ++changed;
                }
            }
    }
    return changed;
}

// The same octant records regrouped for the walk over HBM/L2 (RT_GOCT_GROUP = G > 0): blocks of G
// consecutive nodes, each block laid out octant-major ([block][octant][G nodes], A planes then B
// planes), so G = 1 puts the eight octants' records of a node in one 128-B line (lanes of different
// octants at the same node -- every traversal starts at the root -- read one line, not eight) and
// larger G keeps neighbouring nodes of one octant together as the octant-major layout does.  Links
// are stored as walk words (block * 8G + node in block), so the kernel's index (octant x octStride
// + word) holds with octStride = G; END = rtk::kEndWalk, a word that is neither a node nor a leaf (a
// walk that reaches it leaves the node and triangle steps at once: no sentinel loads).
void build_oct_nodes_grouped(const std::vector<uint32_t>& oct, uint32_t n, uint32_t G, std::vector<uint32_t>& out,
                             uint32_t* b_ofs) {
    const uint32_t stride = oct_stride(n), bofs = oct_b(n);
    const uint32_t na = ((n + 1 + G - 1) / G) * 8u * G;  // A records, sentinel included, whole blocks
    *b_ofs = na;
    out.assign((size_t)2 * na * 4, 0u);
    for (uint32_t i = 0; i <= n; ++i)
        for (uint32_t o = 0; o < 8; ++o) {
            const uint32_t* ra = &oct[((size_t)o * stride + i) * 4];
            const uint32_t* rb = &oct[((size_t)bofs + (size_t)o * stride + i) * 4];
            const size_t at = (size_t)goct_word(i, G) + (size_t)o * G;
            uint32_t* wa = &out[at * 4];
            uint32_t* wb = &out[((size_t)na + at) * 4];
            for (int c = 0; c < 4; ++c) wa[c] = ra[c];
            wb[0] = rb[0];
            wb[1] = rb[1];
            wb[2] = rb[2] >= kLeafMin ? rb[2] : goct_word(rb[2], G);  // leaf code as it is, else the near child
            wb[3] = rb[3] >= n && RT_GOCT_END_WORD ? rtk::kEndWalk : goct_word(rb[3], G);  // END: the non-walk word
        }
}

// Node records for scenes read from HBM/L2 (64 B = half a cache line, so one visit touches
// one line): q0 = {bmin.xyz, bmax.x}, q1 = {bmax.yz, c0, c1}, q2/q3 = skip[8].  Interior:
// c0 = first child, c1 = second child | axis << 30; leaf: c0 = first triangle,
// c1 = count | 3 << 30.  Children and skips are explicit, so the nodes can be renumbered:
// the first `top` nodes in breadth-first order (the top of the tree, visited by nearly every
// ray) come first and are staged in LDS; the rest keep their depth-first order.  The walk is
// the same tree and skip table, so visits, tests and results are unchanged.
void build_global_nodes(const rt_cl_bvh_node* nd, uint32_t n, const std::vector<uint32_t>& skips,
                        uint32_t top, std::vector<uint32_t>& out, uint32_t* n_top, std::vector<uint32_t>* slot_of) {
    std::vector<uint32_t> order, newid(n, 0xffffffffu);
    order.reserve(n);
    std::vector<uint32_t> q = {0};
    for (size_t h = 0; h < q.size() && order.size() < top; ++h) {
        const uint32_t i = q[h];
        newid[i] = (uint32_t)order.size();
        order.push_back(i);
        if (nd[i].nPrimitives == 0) {
            q.push_back(i + 1);
            q.push_back(nd[i].offset);
        }
    }
    *n_top = (uint32_t)order.size();
    for (uint32_t i = 0; i < n; ++i)
        if (newid[i] == 0xffffffffu) {
            newid[i] = (uint32_t)order.size();
            order.push_back(i);
        }
    auto map = [&](uint32_t x) { return x == 0xffffffffu ? x : newid[x]; };
    auto bits = [](float f) {
        uint32_t u;
        std::memcpy(&u, &f, 4);
        return u;
    };
    out.assign((size_t)n * 16, 0u);
    for (uint32_t p = 0; p < n; ++p) {
        const uint32_t i = order[p];
        const rt_cl_bvh_node& x = nd[i];
        uint32_t* r = &out[(size_t)p * 16];
        r[0] = bits(x.bounds.pmin.x);
        r[1] = bits(x.bounds.pmin.y);
        r[2] = bits(x.bounds.pmin.z);
        r[3] = bits(x.bounds.pmax.x);
        r[4] = bits(x.bounds.pmax.y);
        r[5] = bits(x.bounds.pmax.z);
        if (x.nPrimitives > 0) {
            r[6] = x.offset;
            r[7] = (uint32_t)x.nPrimitives | (3u << 30);
        } else {
            r[6] = map(i + 1);
            r[7] = map(x.offset) | ((uint32_t)x.axis << 30);
        }
        for (int o = 0; o < 8; ++o) r[8 + o] = map(skips[(size_t)i * 8 + o]);
    }
    if (slot_of) slot_of->swap(newid);  // node -> its record (the device refit writes planes there)
}

// What the device refit (rt_refit.hip) needs beside the validated node buffer, 2n words: node ->
// parent (interior i is the parent of i + 1 and offset; the root: 0xffffffff), then node -> record
// of the global layout (build_global_nodes' renumbering).  A parent's index is smaller than its
// children's, so a climb through these links ends at the root.
void build_refit_links(const rt_cl_bvh_node* nd, uint32_t n, const std::vector<uint32_t>& slot_of,
                       std::vector<uint32_t>& out) {
    out.assign((size_t)n * 2, 0xffffffffu);
    for (uint32_t i = 0; i < n; ++i) {
        if (nd[i].nPrimitives == 0) {
            out[i + 1] = i;
            out[nd[i].offset] = i;
        }
        out[(size_t)n + i] = slot_of[i];
    }
}

// The whole host half of a scene preparation, in the order a launch has always run it: buffer sizes,
// the tree, the material indices (only against a bound material buffer), the node-index width; then
// every packer.  The regrouped records exist for scenes whose octant records hold every leaf and whose
// walk words stay below the leaf codes.
int pack_scene_host(const SceneBytes& in, uint32_t top_limit, HostPack* out) {
    if (in.tris_size < sizeof(rt_cl_triangle) || in.nodes_size < sizeof(rt_cl_bvh_node) ||
        (in.mats && in.mats_size < sizeof(rt_cl_material)))
        return RT_INVALID_MEM_OBJECT;
    const rt_cl_triangle* tr = reinterpret_cast<const rt_cl_triangle*>(in.tris);
    const rt_cl_bvh_node* nd = reinterpret_cast<const rt_cl_bvh_node*>(in.nodes);
    HostPack& p = *out;
    p = HostPack();
    p.n_tris = (uint32_t)(in.tris_size / sizeof(rt_cl_triangle));
    p.n_mats = in.mats ? (uint32_t)(in.mats_size / sizeof(rt_cl_material)) : 0u;
    const uint32_t n_buf = (uint32_t)(in.nodes_size / sizeof(rt_cl_bvh_node));
    // (n_nodes: the tree's nodes, a prefix of the buffer)
    const int rc = check_nodes(nd, n_buf, p.n_tris, &p.depth, &p.n_nodes);
    if (rc) return rc;
    for (uint32_t i = 0; in.mats && i < p.n_tris; ++i)
        if (tr[i].mtlIndex >= p.n_mats) return RT_INVALID_MEM_OBJECT;
    const uint32_t nn = p.n_nodes;
    if (nn >= (1u << 30)) return RT_INVALID_MEM_OBJECT;  // node indices share a word with the axis
    std::vector<uint32_t> skips, slot_of;
    build_skips(nd, nn, skips);
    build_global_nodes(nd, nn, skips, top_limit, p.global_nodes, &p.n_top, &slot_of);
    build_refit_links(nd, nn, slot_of, p.refit_links);
    p.oct_ok = build_oct_nodes(nd, nn, skips, p.oct_nodes);
    if (RT_GOCT_GROUP && p.oct_ok && (uint64_t)(nn + RT_GOCT_GROUP) * 8u < kLeafMin)
        build_oct_nodes_grouped(p.oct_nodes, nn, RT_GOCT_GROUP, p.goct_nodes, &p.goct_b);
    // the collapsed link set of both layouts, kept only where it differs from the plain one
    if (RT_NODE_COLLAPSE && p.oct_ok) {
        p.collapsed_links = collapse_oct_links(p.oct_nodes, nn, p.oct_nodes_collapsed);
        if (p.collapsed_links == 0) {
            p.oct_nodes_collapsed.clear();
        } else if (!p.goct_nodes.empty()) {
            uint32_t b = 0;
            build_oct_nodes_grouped(p.oct_nodes_collapsed, nn, RT_GOCT_GROUP, p.goct_nodes_collapsed, &b);
        }
    }
    return RT_SUCCESS;
}

// The pruned set of both layouts over the collapsed one (the plain one where there is none), kept only
// where it differs from it.
void pack_pruned_links(const uint8_t* tri_octants, HostPack* pack) {
    HostPack& p = *pack;
    p.pruned_links = 0;
    p.oct_nodes_pruned.clear();
    p.goct_nodes_pruned.clear();
    if (!RT_OCTANT_CULL || !p.oct_ok || !tri_octants) return;
    const std::vector<uint32_t>& base = p.collapsed_links ? p.oct_nodes_collapsed : p.oct_nodes;
    p.pruned_links = prune_oct_links(p.oct_nodes, base, p.n_nodes, tri_octants, p.oct_nodes_pruned);
    if (p.pruned_links == 0) {
        p.oct_nodes_pruned.clear();
    } else if (!p.goct_nodes.empty()) {
        uint32_t b = 0;
        build_oct_nodes_grouped(p.oct_nodes_pruned, p.n_nodes, RT_GOCT_GROUP, p.goct_nodes_pruned, &b);
    }
}

}  // namespace rtp

// rt_scene_pack.cpp -- validation of the flattened BVH and the node records packed from it.
// Pure host code (no HIP): rti::DeviceScene (rt_device_scene.cpp) owns the device buffers and the copies.
#include "rt_scene_pack.hpp"

#include <algorithm>
#include <cmath>
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
//     miss_next in `base`, repeated while the target is culled.  miss_next words strictly advance in the
//     octant's depth-first order and END is never culled, so the chain ends.
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
//   * So do the gate-skipped links where `base` is that set (gate_skip_oct_links).  The argument about the
//     arrival at a culled node x is unaffected: it reads no box test but x's own, and "the skip of x's
//     subtree" is, in that set, the word x's own miss_next holds there -- every link out of the subtree was
//     redirected alike -- which is why the chain above follows base's miss_next and not the plain one.  Base's
//     words never target a removed node, so neither do these.
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
        const uint32_t* bb = &base[plane];  // (base's miss_next: the plain word but over the gate-skipped set)
        auto live = [&](uint32_t x) {
            while (x < n && culled[x]) x = bb[(size_t)x * 4 + 3];
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

// The certificate of the gate-skipped link set: every plane of the tree [0, n) is finite, and every node
// but the root nests in its parent plane by plane -- pmin_child >= pmin_parent and pmax_child <= pmax_parent
// on the three axes, compared as float values (+0 and -0 are equal) on the bounds the octant records are
// bitwise copies of.  A builder that forms a parent's box as the exact min / max of its children's nests by
// construction.  One node that does not and the scene has no such set: nothing is repaired.
bool boxes_nest(const rt_cl_bvh_node* nd, uint32_t n) {
    auto planes = [&](uint32_t i, float* lo, float* hi) {
        lo[0] = nd[i].bounds.pmin.x, lo[1] = nd[i].bounds.pmin.y, lo[2] = nd[i].bounds.pmin.z;
        hi[0] = nd[i].bounds.pmax.x, hi[1] = nd[i].bounds.pmax.y, hi[2] = nd[i].bounds.pmax.z;
    };
    for (uint32_t i = 0; i < n; ++i) {
        float lo[3], hi[3];
        planes(i, lo, hi);
        for (int ax = 0; ax < 3; ++ax)
            if (!std::isfinite(lo[ax]) || !std::isfinite(hi[ax])) return false;
        if (nd[i].nPrimitives > 0) continue;
        for (uint32_t c : {i + 1, nd[i].offset}) {
            float clo[3], chi[3];
            planes(c, clo, chi);
            for (int ax = 0; ax < 3; ++ax)
                if (!(clo[ax] >= lo[ax]) || !(chi[ax] <= hi[ax])) return false;
        }
    }
    return true;
}

namespace {

// a triangle test against a node visit, in VALU instructions of the shipped fused LDS-walk kernel: 52 for
// the test (profiles/r06/tuning_sweep.txt), 19 for the visit (profiles/HISTORY.md, round 13)
constexpr double kGateTriCost = 52.0 / 19.0;
// the longest run of removed nodes between a node and its gate that the programme weighs; a longer run
// (of equal-box nodes, which are removed whatever it says) is weighed as one of this length
constexpr uint32_t kGateMaxRun = 8;

double box_area(const rt_cl_bvh_node& x) {
    const double d[3] = {(double)x.bounds.pmax.x - x.bounds.pmin.x, (double)x.bounds.pmax.y - x.bounds.pmin.y,
                         (double)x.bounds.pmax.z - x.bounds.pmin.z};
    return 2.0 * (d[0] * d[1] + d[1] * d[2] + d[2] * d[0]);
}

// the share of the rays through g's box that go through i's (i nests in g): the surface-area ratio
double pass_share(const std::vector<double>& area, uint32_t i, uint32_t g) {
    return area[g] > 0.0 ? std::min(1.0, std::max(0.0, area[i] / area[g])) : 1.0;
}

// the six bound words are equal as uint32_t (the collapse's comparison: +0.0 and -0.0 differ)
bool same_bounds(const rt_cl_bvh_node& a, const rt_cl_bvh_node& b) {
    const float* x[6] = {&a.bounds.pmin.x, &a.bounds.pmin.y, &a.bounds.pmin.z, &a.bounds.pmax.x, &a.bounds.pmax.y, &a.bounds.pmax.z};
    const float* y[6] = {&b.bounds.pmin.x, &b.bounds.pmin.y, &b.bounds.pmin.z, &b.bounds.pmax.x, &b.bounds.pmax.y, &b.bounds.pmax.z};
    for (int k = 0; k < 6; ++k)
        if (std::memcmp(x[k], y[k], 4) != 0) return false;
    return true;
}

}  // namespace

// The interior nodes the gate-skipped set removes (removed[i] = 1), for a tree that holds boxes_nest; one
// set for the eight octants.  The root is kept: the ring fill's root test and its sky decision read the
// root's record.  Leaves are kept: their box test is part of the result (a leaf entered is a leaf whose
// triangles are tested), and the kernels take a leaf's continuation from the visited record.  An interior
// node whose box is bitwise its parent's is removed whatever the cost says -- its test is the collapse's,
// known to pass -- so the set contains the collapsed one.  The rest is a choice of cost alone, since the
// lemma of gate_skip_oct_links allows any of them:
//   RT_GATE_SELECT 0, the SAH programme.  With p = area(node) / area(nearest kept ancestor g), the share of
//   g's passing rays that reach into the node's box, the expected cost of a subtree under gate g is
//     kept interior      1 + p * (cost of the two children under the node)
//     removed interior   the cost of the two children under g
//     leaf               1 + p * count * kGateTriCost
//   and a node is removed where that is strictly cheaper.  Children have larger indices than their parent:
//   one backward sweep fills cost[node][distance to the gate], a forward sweep reads the choices off.
//   RT_GATE_SELECT 1, the plain ratio: a node is removed when p >= RT_GATE_RATIO_PCT / 100.
void select_gate_skips(const rt_cl_bvh_node* nd, uint32_t n, std::vector<uint8_t>& removed) {
    removed.assign(n, 0);
    if (n == 0) return;
    std::vector<uint32_t> parent(n, 0xffffffffu), depth(n, 0);
    std::vector<double> area(n);
    for (uint32_t i = 0; i < n; ++i) {
        area[i] = box_area(nd[i]);
        if (nd[i].nPrimitives > 0) continue;
        for (uint32_t c : {i + 1, nd[i].offset}) parent[c] = i, depth[c] = depth[i] + 1;
    }
    auto forced = [&](uint32_t i) { return i > 0 && nd[i].nPrimitives == 0 && same_bounds(nd[i], nd[parent[i]]); };
    auto ancestor = [&](uint32_t i, uint32_t k) {
        while (k-- > 0) i = parent[i];
        return i;
    };
    const uint32_t K = kGateMaxRun + 1;  // gate distances 1..K
    if (RT_GATE_SELECT == 1) {
        std::vector<uint32_t> gate(n, 0);  // the nearest kept ancestor
        for (uint32_t i = 1; i < n; ++i) {
            gate[i] = removed[parent[i]] ? gate[parent[i]] : parent[i];
            if (nd[i].nPrimitives == 0)
                removed[i] = forced(i) || pass_share(area, i, gate[i]) * 100.0 >= (double)RT_GATE_RATIO_PCT;
        }
        return;
    }
    std::vector<double> cost((size_t)n * (K + 1), 0.0);
    std::vector<uint8_t> skip((size_t)n * (K + 1), 0);
    for (uint32_t i = n; i-- > 0;) {
        for (uint32_t k = 1; k <= std::min(K, depth[i]); ++k) {
            const double p = pass_share(area, i, ancestor(i, k));
            double& c = cost[(size_t)i * (K + 1) + k];
            if (nd[i].nPrimitives > 0) {
                c = 1.0 + p * (double)nd[i].nPrimitives * kGateTriCost;
                continue;
            }
            const uint32_t a = i + 1, b = nd[i].offset, kk = std::min(k + 1, K);
            const double kept = 1.0 + p * (cost[(size_t)a * (K + 1) + 1] + cost[(size_t)b * (K + 1) + 1]);
            const double gone = cost[(size_t)a * (K + 1) + kk] + cost[(size_t)b * (K + 1) + kk];
            const bool s = forced(i) || (k < K && gone < kept);
            skip[(size_t)i * (K + 1) + k] = s;
            c = s ? gone : kept;
        }
    }
    std::vector<uint32_t> dist(n, 1);  // distance to the nearest kept ancestor, as the programme weighed it
    for (uint32_t i = 1; i < n; ++i) {
        const uint32_t q = parent[i];
        dist[i] = removed[q] ? std::min(dist[q] + 1, K) : 1;
        removed[i] = skip[(size_t)i * (K + 1) + dist[i]];
    }
}

// The gate-skipped link set: a copy of the plain records `oct` (n nodes, every leaf inline) in which, per
// octant o, every hit_next and miss_next word that targets a removed interior node c (select_gate_skips)
// is replaced by c's near child under o -- c's plain hit_next -- repeated while the target is removed;
// returns the number of words it changes.  (Children have larger indices: the chain is finite and ends at
// a kept node, which may be a leaf.)  The tree must hold boxes_nest.
//
// Why a walk over these links computes what the plain walk computes.  The lemma: for a ray of octant o and
// a node c with a descendant x, if x's box test passes at some t' <= t then c's passes at t.  The node step
// (oct_step, oct_step_w and oct_step_g of rt_kernels_body.hpp are one arithmetic, and the three math
// policies differ only in the reciprocal `inv` they formed once per ray) computes per axis a near term
// fl(fl(near - o_k) * inv_k) and a far term fl(fl(far - o_k) * inv_k) on the planes the record holds for o,
// t0 = max(0, near terms), t1 = min(t, far terms), and passes when t1 >= t0.
//   * Under o, the near plane is pmin where inv_k >= 0 and pmax where inv_k < 0 (the octant bit is
//     `inv_k < 0`, so d_k = -0 with inv_k = -inf counts as negative and d_k = +0 as positive).  Nesting moves
//     x's near plane along the ray against c's and x's far plane against it: fl(b - o_k) is monotone in b,
//     and fl(y * inv_k) is monotone in y with the direction inv_k's sign gives, so x's near term >= c's and
//     x's far term <= c's, whatever inv_k's value -- an exact quotient, a hardware reciprocal an ulp off, or
//     an infinity.  min(t, .) is monotone in t.  Hence t0(c) <= t0(x) <= t1(x) <= t1(c).
//   * NaN.  __builtin_fmaxf / fminf return the other operand when one is NaN, so a NaN term constrains
//     nothing, and `t1 >= t0` is false on a NaN.  t0 is never NaN (it starts from 0).  With finite planes a
//     term is NaN when inv_k is NaN (then it is for c and x alike) or as 0 * inf: plane == o_k on an axis
//     with d_k = +-0.  If x's term is NaN and c's is not, c's plane lies on the side nesting allows: its
//     near term is -inf and its far term +inf, which constrain nothing either.  If c's term is NaN and
//     x's is not, c is the less strict of the two.  A NaN t with every far term NaN fails x and c alike; x
//     passing needs a far term that is a number, and c's term on that axis is no smaller (a NaN there would
//     put x's far plane behind the origin: far term -inf, and x fails).
//   * +0 and -0 planes: fl(b - o_k) differs for them only in the sign of a zero, which max, min and >= do not
//     see and which gives NaN for both against an infinite inv_k.  The certificate compares values.
// Equivalently: c fails implies every node below c fails, at the same t.  Now take a word redirected from c
// to c's near child a.  If c's test would have passed, the plain walk goes to a: the same position, one
// visit less.  If it would have failed, the plain walk goes to c's miss_next with t untouched; the walk over
// these links visits a, which fails, goes on to a's miss_next -- c's far child b, or b's near child where b
// is removed -- and so on: every kept node below c is visited at most once, fails (kept leaves have their
// own box test, and it fails), no triangle is tested, t does not change, and the last miss_next of the
// subtree is the word c's own miss_next is in this set.  Either way the state after c's subtree is the plain
// walk's.  By induction over the redirected words every leaf entered, every triangle tested and the final
// {t, prim, u, v} are the plain walk's, in its order, for closest-hit and any-hit walks alike (they differ in
// what a triangle step does, and t only shrinks, which the lemma allows).  Only the visits differ: one less
// per passage of a passing removed node, up to the subtree's kept nodes more per passage of a failing one,
// which is what select_gate_skips weighs.
//   * The collapse is the case of a removed node with its parent's planes; every collapsed word is on the
//     chain followed here, so a word of this set differs from the collapsed set's only where that one still
//     targets a removed node.
//   * Planes, leaf codes and END are the plain set's, word for word.  The root's record stays; so does every
//     removed node's, which no link leads to.
// Like the collapse, the certificate is a property of the planes as packed: after a device refit only the
// plain set may be walked until the next full preparation (rti::DeviceScene).
uint32_t gate_skip_oct_links(const std::vector<uint32_t>& oct, uint32_t n, const std::vector<uint8_t>& removed,
                             std::vector<uint32_t>& out) {
    const uint32_t stride = oct_stride(n), bofs = oct_b(n);
    out = oct;
    uint32_t changed = 0;
    for (uint32_t o = 0; o < 8; ++o) {
        const size_t plane = ((size_t)bofs + (size_t)o * stride) * 4;
        const uint32_t* pb = &oct[plane];
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t k = 2; k < 4; ++k) {
                uint32_t& w = out[plane + (size_t)i * 4 + k];
                if (w >= n) continue;  // a leaf code, or END
                uint32_t to = w;
                while (removed[to]) to = pb[(size_t)to * 4 + 2];  // (a removed node is interior: a node index)
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
    // the gate-skipped link set of both layouts, for trees that hold its certificate; kept only where it
    // differs from the collapsed one
    if (RT_GATE_SKIP && RT_NODE_COLLAPSE && p.oct_ok && (p.nested = boxes_nest(nd, nn))) {
        select_gate_skips(nd, nn, p.gate_removed);
        p.gate_links = gate_skip_oct_links(p.oct_nodes, nn, p.gate_removed, p.oct_nodes_gated);
        if (p.oct_nodes_gated == (p.collapsed_links ? p.oct_nodes_collapsed : p.oct_nodes)) {
            p.oct_nodes_gated.clear();
        } else if (!p.goct_nodes.empty()) {
            uint32_t b = 0;
            build_oct_nodes_grouped(p.oct_nodes_gated, nn, RT_GOCT_GROUP, p.goct_nodes_gated, &b);
        }
    }
    return RT_SUCCESS;
}

// The pruned set of both layouts over the collapsed one (the plain one where there is none), kept only
// where it differs from it; and, for a scene with a gate-skipped set, the pruned set over that one.
void pack_pruned_links(const uint8_t* tri_octants, HostPack* pack) {
    HostPack& p = *pack;
    p.pruned_links = 0;
    p.oct_nodes_pruned.clear();
    p.goct_nodes_pruned.clear();
    p.gated_pruned_links = 0;
    p.oct_nodes_gated_pruned.clear();
    p.goct_nodes_gated_pruned.clear();
    if (!RT_OCTANT_CULL || !p.oct_ok || !tri_octants) return;
    const std::vector<uint32_t>& base = p.collapsed_links ? p.oct_nodes_collapsed : p.oct_nodes;
    p.pruned_links = prune_oct_links(p.oct_nodes, base, p.n_nodes, tri_octants, p.oct_nodes_pruned);
    if (p.pruned_links == 0) {
        p.oct_nodes_pruned.clear();
    } else if (!p.goct_nodes.empty()) {
        uint32_t b = 0;
        build_oct_nodes_grouped(p.oct_nodes_pruned, p.n_nodes, RT_GOCT_GROUP, p.goct_nodes_pruned, &b);
    }
    // ... and the pruned set over the gate-skipped one, where the scene has that
    if (p.oct_nodes_gated.empty()) return;
    p.gated_pruned_links = prune_oct_links(p.oct_nodes, p.oct_nodes_gated, p.n_nodes, tri_octants, p.oct_nodes_gated_pruned);
    if (p.gated_pruned_links == 0) {
        p.oct_nodes_gated_pruned.clear();
    } else if (!p.goct_nodes.empty()) {
        uint32_t b = 0;
        build_oct_nodes_grouped(p.oct_nodes_gated_pruned, p.n_nodes, RT_GOCT_GROUP, p.goct_nodes_gated_pruned, &b);
    }
}

}  // namespace rtp

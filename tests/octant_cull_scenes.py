"""Hand-built triangles and trees for the octant-cull tests (test_octant_cull.py, test_octant_cull_gpu.py),
written down so that the tests know every index, and the rule of csrc/rt_scene_pack.cpp (prune_oct_links)
restated over the node array for the expected links.

A quad(p, e1, e2) is the two triangles (p, p + e1, p + e1 + e2), (p, p + e1 + e2, p + e2): both have the
geometric normal e1 x e2.  RayTriangle rejects det < 1e-8 and det = -d . (e1 x e2), so a quad is culled for
the rays that travel along its normal: for an axis-plane quad with normal +z those are the four octants whose
z bit is clear (bit k of an octant = the direction's component k is negative or -0)."""
import numpy as np

from clrt import _native as N
from clrt import scene as S

import node_collapse_scenes as NC
import stress_scenes as SS

C = np.float32(SS.CENTER)


def tri(p1, p2, p3, mtl=0):
    t = np.zeros(1, N.TRIANGLE_DTYPE)
    p = [np.float32(x) for x in (p1, p2, p3)]
    with np.errstate(all="ignore"):
        n = np.cross((p[1] - p[0]).astype(np.float64), (p[2] - p[0]).astype(np.float64))
        l = np.sqrt((n * n).sum())
        n = np.float32(n / l) if np.isfinite(l) and l > 0 else np.float32([0.0, 0.0, 1.0])
    for v, q in zip(("v1", "v2", "v3"), p):
        t[v]["position"][0, :3] = q
        t[v]["normal"][0, :3] = n
    t["mtlIndex"] = mtl
    return t


def quad(p, e1, e2, mtl=0):
    p, e1, e2 = (np.float32(x) for x in (p, e1, e2))
    return np.concatenate([tri(p, p + e1, p + e1 + e2, mtl), tri(p, p + e1 + e2, p + e2, mtl)])


def octants(bit, value):
    """The mask of the four octants whose bit `bit` is `value`."""
    return sum(1 << o for o in range(8) if ((o >> bit) & 1) == value)


ROT = (np.float32(np.cos(0.3)), np.float32(np.sin(0.3)))  # the rotated box's side direction (ax, ay)


def room_scene():
    """A room of axis-plane quads around SS.CENTER with slanted triangles and the side of a box rotated
    about z in its middle; returns (Scene, leaf name -> node index, leaf name -> expected triangle mask).
         0 root, axis 2: first 1, second 6
         1 axis 0: first leaf F (floor, normal +z), second 3
         3 axis 1: first leaf W1 (wall x = -4, normal -x: it faces outwards), second leaf G (slanted + rotated: never culled)
         6 axis 0: first 7, second leaf C (ceiling, normal -z)
         7 axis 1: first leaf W2 (wall x = +4, normal -x), second leaf B (wall y = +4, normal -y)
       Node 7 is culled where the x and y bits are both set, node 6 where all three are.  The walls stop one
       unit short of a neighbour so that no child has its parent's box (nothing collapses); leaf G is partly
       certified (the rotated quad's second triangle), which changes nothing: only whole leaves are culled."""
    lo, hi = C - 4, C + 4
    rng = np.random.default_rng(41)
    mats = SS.soup_materials(rng)
    F = quad(lo, (8, 0, 0), (0, 8, 0), 1)
    W1 = quad(lo, (0, 0, 7), (0, 8, 0), 2)
    ax, ay = ROT
    G = np.concatenate([
        tri(C + (-2, -1, -3), C + (2, -1.5, -2), C + (0.5, 2, -2.5), 4),
        tri(C + (-1, 1, 0), C + (1.5, 0.5, 1), C + (0, -2, 2), 5),
        tri(C + (2, 2, -1), C + (-2, 2.5, 0.5), C + (0, 0.5, 3), 0),   # emissive
        quad(C + (-1, -1, -4), (2 * ax, 2 * ay, 0), (0, 0, 3), 6),      # a vertical face rotated about z
    ])
    W2 = quad((hi[0], lo[1] + 1, lo[2] + 1), (0, 0, 7), (0, 7, 0), 3)
    B = quad((lo[0], hi[1], lo[2] + 1), (8, 0, 0), (0, 0, 7), 7)
    Cq = quad((lo[0], lo[1], hi[2]), (0, 8, 0), (8, 0, 0), 8)  # the ceiling; material 8 is emissive
    parts = [("F", F), ("W1", W1), ("G", G), ("W2", W2), ("B", B), ("C", Cq)]
    tris = np.concatenate([p for _, p in parts])
    rng_ = {}
    at = 0
    for name, p in parts:
        rng_[name] = (at, at + len(p))
        at += len(p)
    leaf = lambda name: ("leaf", *rng_[name], None)
    n3 = ("node", 1, leaf("W1"), leaf("G"), None)
    n1 = ("node", 0, leaf("F"), n3, None)
    n7 = ("node", 1, leaf("W2"), leaf("B"), None)
    n6 = ("node", 0, n7, leaf("C"), None)
    nodes = NC.build_tree(tris, ("node", 2, n1, n6, None))
    names = {"n0": 0, "n1": 1, "F": 2, "n3": 3, "W1": 4, "G": 5, "n6": 6, "n7": 7, "W2": 8, "B": 9, "C": 10}
    assert len(nodes) == 11 and int(nodes[0]["offset"]) == 6 and int(nodes[1]["offset"]) == 3
    masks = {"F": octants(2, 0), "C": octants(2, 1), "W1": octants(0, 1), "W2": octants(0, 1), "B": octants(1, 1)}
    return S.Scene(tris, nodes, mats, 8), names, masks, rng_


def corner_scene():
    """Three quads with normals +x, +y, +z: octant 0 culls every triangle (its links stay as they are).
         0 root, axis 0: first leaf X, second 2;   2 axis 1: first leaf Y, second leaf Z"""
    lo = C - 2
    rng = np.random.default_rng(42)
    mats = SS.soup_materials(rng)
    X = quad(lo, (0, 4, 0), (0, 0, 4), 1)
    Y = quad(lo, (0, 0, 4), (4, 0, 0), 2)
    Z = quad(lo, (4, 0, 0), (0, 4, 0), 3)
    tris = np.concatenate([X, Y, Z])
    nodes = NC.build_tree(tris, ("node", 0, ("leaf", 0, 2, None), ("node", 1, ("leaf", 2, 4, None), ("leaf", 4, 6, None), None), None))
    return S.Scene(tris, nodes, mats, 2)


# ---- the rule, restated over the node array ---------------------------------------------------

def skip_table(nodes, n):
    """{(i, o): the node the walk goes to after i's subtree (n: the end)}"""
    out = {(0, o): n for o in range(8)}
    for i in range(n):
        if nodes[i]["nPrimitives"] > 0:
            continue
        first, second = i + 1, int(nodes[i]["offset"])
        for o in range(8):
            near, far = (second, first) if (o >> int(nodes[i]["axis"])) & 1 else (first, second)
            out[near, o] = far
            out[far, o] = out[i, o]
    return out


def culled_nodes(nodes, n, masks):
    """{(i, o): every triangle below node i is certified for octant o} (masks: one byte per triangle)"""
    out = {}
    for i in reversed(range(n)):
        for o in range(8):
            if nodes[i]["nPrimitives"] > 0:
                lo = int(nodes[i]["offset"])
                out[i, o] = all((int(masks[t]) >> o) & 1 for t in range(lo, lo + int(nodes[i]["nPrimitives"])))
            else:
                out[i, o] = out[i + 1, o] and out[int(nodes[i]["offset"]), o]
    return out


def expected_pruned(nodes, n, masks):
    """{(i, o): (hit_next, miss_next)} of the pruned set: the collapsed links (NC.expected_links) and the
    skips, each moved on past culled nodes; an octant that culls the root keeps the collapsed links."""
    base = NC.expected_links(nodes, n)
    skip = skip_table(nodes, n)
    cull = culled_nodes(nodes, n, masks)

    def live(x, o):
        while x < n and cull[x, o]:
            x = skip[x, o]
        return x

    out = {}
    for (i, o), (_, hit) in base.items():
        if cull[0, o]:
            out[i, o] = (hit, skip[i, o])
        else:
            out[i, o] = (hit if hit >= NC.LEAF_MIN else live(hit, o), live(skip[i, o], o))
    return out

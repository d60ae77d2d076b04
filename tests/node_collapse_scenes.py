"""Hand-built trees for the node-collapse tests (test_node_collapse.py, test_node_collapse_gpu.py):
chains of interior nodes that carry their parent's box, written down node by node so that the tests
know every index, and the rule of csrc/rt_scene_pack.cpp (collapse_oct_links) restated over the node
array for the expected links.

A tree is a nested spec: ("leaf", lo, hi, box) or ("node", axis, first, second, box), box being None
(the exact bounds of the triangles below), "parent" (the parent's box, word for word) or a function of
the parent's box.  Nodes are emitted depth first, the first child right after its parent, as
CLLinearBVHNode arrays are."""
import numpy as np

from clrt import _native as N
from clrt import scene as S

import stress_scenes as SS

LEAF_MIN = 1 << 24


def _tight(tris, spec):
    if spec[0] == "leaf":
        return SS._bounds(tris, spec[1], spec[2])
    a, b = _tight(tris, spec[2]), _tight(tris, spec[3])
    return np.minimum(a[0], b[0]), np.maximum(a[1], b[1])


def build_tree(tris, spec):
    """The node array of `spec` over `tris` (no garbage tail)."""
    nodes = []

    def emit(s, parent_box):
        how = s[-1]
        if how is None:
            box = _tight(tris, s)
        elif how == "parent":
            box = parent_box
        else:
            box = how(parent_box)
        box = (np.array(box[0], np.float32), np.array(box[1], np.float32))
        r = np.zeros((), N.NODE_DTYPE)
        r["bmin"][:3], r["bmax"][:3] = box
        me = len(nodes)
        nodes.append(r)
        if s[0] == "leaf":
            r["offset"], r["nPrimitives"] = s[1], s[2] - s[1]
        else:
            r["axis"] = s[1]
            emit(s[2], box)
            r["offset"] = len(nodes)
            emit(s[3], box)
        return me

    emit(spec, None)
    out = np.zeros(len(nodes), N.NODE_DTYPE)
    for i, r in enumerate(nodes):
        out[i] = r
    return out


def chain_spec(links, n_tris):
    """A chain of len(links) + 1 interior nodes with one box, from the root along `links` ("f": the
    next one is the first child, "s": the second), every off-chain sibling a one-triangle leaf; the
    chain's last node has a leaf of the remaining triangles and, as its second child, an interior node
    with its own (tight) box over two one-triangle leaves.  Triangle ranges are handed out in emission (depth-first) order."""
    counter = [0]

    def leaf(k=1):
        lo = counter[0]
        counter[0] += k
        return ("leaf", lo, lo + k, None)

    def end():
        a = leaf()
        return ("node", 1, a, leaf(), None)

    def chain(rest, top):
        box = None if top else "parent"
        axis = len(rest) % 3
        if not rest:
            # (the "f" links' sibling leaves are emitted after this subtree: one triangle each stays for them)
            a = leaf(n_tris - counter[0] - links.count("f") - 2)
            return ("node", axis, a, end(), box)
        if rest[0] == "f":
            first = chain(rest[1:], False)
            return ("node", axis, first, leaf(), box)
        sib = leaf()
        return ("node", axis, sib, chain(rest[1:], False), box)

    spec = chain(links, True)
    assert counter[0] == n_tris, (counter[0], n_tris)
    return spec


def chain_nodes(nodes, links):
    """Indices of the chain's interior nodes in the emitted array, root first."""
    idx = [0]
    for c in links:
        i = idx[-1]
        idx.append(i + 1 if c == "f" else int(nodes[i]["offset"]))
    return idx


def chain_scene(links, n_tris=24, seed=31):
    tris, mats = SS.soup(seed, n_tris)
    nodes = build_tree(tris, chain_spec(links, n_tris))
    chain = chain_nodes(nodes, links)
    below = int(nodes[chain[-1]]["offset"])
    assert not np.array_equal(_box_words(nodes, below), _box_words(nodes, 0))
    return S.Scene(tris, nodes, mats, n_tris)


def _neg_zero_z(box):
    lo = np.array(box[0], np.float32)
    lo[2] = np.float32(-0.0)
    return lo, box[1]


def _zero_floor(tris, lo, hi):
    """The tight box of triangles [lo, hi) with its lower z plane moved down to +0.0."""
    def f(_parent):
        bmin, bmax = SS._bounds(tris, lo, hi)
        assert bmin[2] > 0.0
        bmin = bmin.copy()
        bmin[2] = np.float32(0.0)
        return bmin, bmax
    return f


MIXED_TRIS = 40


def mixed_scene(seed=32):
    """One tree with every case, renderable (a soup with materials):
         0 root, axis 0: first 1, second leaf A
         1 box of 0, axis 2: first leaf B, second 3          (0 -> 1 along a first-child link)
         3 box of 0, axis 1: first 4, second leaf E          (1 -> 3 along a second-child link)
         4 box of 0, axis 1: first leaf C (box of 0: a leaf with its parent's box), second 6
         6 own box with bmin.z = +0.0, axis 0: first 7, second leaf H
         7 box of 6 but bmin.z = -0.0, axis 2: first leaf F, second leaf G   (must not collapse)
       Returns (Scene, names -> node index)."""
    tris, mats = SS.soup(seed, MIXED_TRIS)
    T = MIXED_TRIS
    # depth-first triangle ranges: B, C, F, G, H, E, A
    rB, rC, rF, rG, rH, rE, rA = (0, 3), (3, 7), (7, 12), (12, 20), (20, 27), (27, 33), (33, T)
    n7 = ("node", 2, ("leaf", *rF, None), ("leaf", *rG, None), _neg_zero_z)
    n6 = ("node", 0, n7, ("leaf", *rH, None), _zero_floor(tris, rF[0], rH[1]))
    n4 = ("node", 1, ("leaf", *rC, "parent"), n6, "parent")
    n3 = ("node", 1, n4, ("leaf", *rE, None), "parent")
    n1 = ("node", 2, ("leaf", *rB, None), n3, "parent")
    n0 = ("node", 0, n1, ("leaf", *rA, None), None)
    nodes = build_tree(tris, n0)
    names = {"n0": 0, "n1": 1, "B": 2, "n3": 3, "n4": 4, "C": 5, "n6": 6, "n7": 7, "F": 8, "G": 9, "H": 10, "E": 11,
             "A": 12}
    assert len(nodes) == 13 and int(nodes[1]["offset"]) == 3 and int(nodes[0]["offset"]) == 12
    return S.Scene(tris, nodes, mats, 8), names


def single_leaf_scene(seed=33):
    tris, mats = SS.soup(seed, 20)  # (the soup's first eight picks are zero-area triangles)
    return S.Scene(tris, build_tree(tris, ("leaf", 0, 20, None)), mats, 20)


# ---- the rule, restated over the node array ---------------------------------------------------

def _box_words(nodes, i):
    return np.concatenate([nodes["bmin"][i, :3], nodes["bmax"][i, :3]]).view(np.uint32)


def near_child(nodes, i, o):
    return int(nodes[i]["offset"]) if (o >> int(nodes[i]["axis"])) & 1 else i + 1


def leaf_code(nodes, i):
    return (int(nodes[i]["nPrimitives"]) << 24) | int(nodes[i]["offset"])


def expected_links(nodes, n):
    """{(i, o): (plain hit_next, collapsed hit_next)} for every node of the tree [0, n)."""
    out = {}
    for i in range(n):
        for o in range(8):
            if nodes[i]["nPrimitives"] > 0:
                out[i, o] = (leaf_code(nodes, i),) * 2
                continue
            c0 = c = near_child(nodes, i, o)
            while nodes[c]["nPrimitives"] == 0 and np.array_equal(_box_words(nodes, c), _box_words(nodes, i)):
                c = near_child(nodes, c, o)
            out[i, o] = (c0, c)
    return out

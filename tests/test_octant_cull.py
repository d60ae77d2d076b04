"""CPU: the octant-cull certificate (csrc/rt_octant_cull.cpp) and the pruned link set of the octant records
(csrc/rt_scene_pack.cpp, prune_oct_links), driven through the stand-alone tests/native/octant_cull_main.cpp
built with g++ -fsanitize=address,undefined (host code, no preload).

* the certificate against brute force: for every certified (triangle, octant) pair, det in fp32 with and
  without fma contraction, in both association orders, over a lattice of the octant's directions with +-0
  components, single-axis directions, components of 1e-30 and of denormal size; no evaluation reaches 1e-8.
* hand-built triangles: an axis-plane quad is certified in exactly its 4 octants; a vertical quad rotated about
  z, a triangle under the 2^-18 margin, a non-finite and an out-of-range triangle are refused.
* Cornell: the certified pairs and the pruned link words, counted once and written here.
* the pruned links of hand-built trees (octant_cull_scenes.py) against the rule restated over the node array.
* a replay walker (in the driver) over plain, collapsed and pruned links: the pruned walk's tested-triangle
  sequence is the plain walk's without the tests of wholly certified leaves (partly certified leaves are not
  shrunk; in the corner scene, whose leaves are all or nothing, these are exactly the certified tests), no
  removed test was accepted by the plain walk, and {t, prim, u, v} are bit-equal."""
import os
import subprocess

import numpy as np
import pytest

import node_collapse_scenes as NC
import octant_cull_scenes as OC
import stress_scenes as SS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "mini-opencl-raytracer_amd", "csrc")

# Cornell, counted once with the driver.  Its box is not aligned with the coordinate axes, so most triangles
# are certified in one or two octants, not four; 15 are refused.  Some leaves are partly certified: they stay.
CORNELL = {"tris": 72, "pairs": 80, "refused": 15, "pruned_links": 25}


def _compile(tmp, name, *defs):
    exe = str(tmp / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *defs, "-o", exe,
                    os.path.join(REPO, "tests", "native", "octant_cull_main.cpp"),
                    os.path.join(CSRC, "rt_octant_cull.cpp"), os.path.join(CSRC, "rt_scene_pack.cpp")],
                   check=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def tools(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("octant_cull")
    return {"on": _compile(tmp, "octant_cull_main"), "off": _compile(tmp, "octant_cull_off", "-DRT_OCTANT_CULL=0")}


def _run(exe, *args):
    p = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    f = p.stdout.split()
    return {k: int(v) for k, v in zip(f[::2], f[1::2])}


def _masks(exe, tmp_path, tris, tag):
    """-> (one certificate mask per triangle, the brute-force report)"""
    path = tmp_path / f"{tag}.tris"
    np.ascontiguousarray(tris).tofile(path)
    r = _run(exe, "cert", path, tmp_path / f"{tag}.mask")
    m = np.fromfile(tmp_path / f"{tag}.mask", np.uint8)
    assert len(m) == len(tris) == r["tris"] and r["pairs"] == sum(bin(int(x)).count("1") for x in m)
    return m, r


# ---- the certificate ------------------------------------------------------------------------------------

def test_axis_plane_quads_are_certified_in_exactly_four_octants(tools, tmp_path):
    sc, _, want, rng = OC.room_scene()
    m, r = _masks(tools["on"], tmp_path, sc.triangles, "room")
    for name, mask in want.items():
        lo, hi = rng[name]
        assert [int(x) for x in m[lo:hi]] == [mask] * (hi - lo), name
        assert bin(mask).count("1") == 4
    assert r["violations"] == 0 and r["evals"] > 100000 and r["max_det_e12"] <= 0


def test_rotated_vertical_quad_is_refused_where_the_dz_pair_must_cancel(tools, tmp_path):
    """The first triangle of the quad has e1 = (ax, ay, 0), e2 = (ax, ay, h): a.z = e1.y e2.x and b.z = e1.x e2.y
    are non-zero and equal, c.z = 0 only because they cancel, so no octant can be certified.  The second has
    e1 = (ax, ay, h), e2 = (0, 0, h), whose z products are exactly zero: it needs no cancellation and is certified
    in the two octants that oppose its normal in x and y."""
    ax, ay = OC.ROT
    q = OC.quad(OC.C, (2 * ax, 2 * ay, 0), (0, 0, 3))
    m, r = _masks(tools["on"], tmp_path, q, "rot")
    assert int(m[0]) == 0
    # the normal is (ay, -ax, 0) * 6: culled for d.x >= 0 and d.y <= 0, either sign of d.z
    assert int(m[1]) == (1 << 2) | (1 << 6)
    assert r["violations"] == 0


def test_margin_nonfinite_and_range(tools, tmp_path):
    o = OC.C
    k = 2.0 ** -19
    tris = np.concatenate([
        # e1 = (1, 1, 0), e2 = (1, 1 + k, 0): a.z = 1, b.z = 1 + k, |c.z| = k = 2^-19 < 2^-18 (|a.z| + |b.z|)
        OC.tri((0, 0, 0), (1, 1, 0), (1, 1 + k, 0)),
        # the same shape with 8 k = 2^-16: above the margin, an axis-plane triangle certified in its 4 octants
        OC.tri((0, 0, 0), (1, 1, 0), (1, 1 + 8 * k, 0)),
        OC.tri(o, o + np.float32([1, 0, 0]), o + np.float32([0, np.nan, 0])),
        OC.tri(o, o + np.float32([1, 0, 0]), o + np.float32([0, np.inf, 0])),
        OC.tri((0, 0, 0), (2.0 ** 20 * 1.5, 0, 0), (0, 1, 0)),
        OC.tri((0, 0, 0), (2.0 ** 20, 0, 0), (0, 1, 0)),      # on the bound: in range
        OC.tri(o, o, o),                                      # a point: det is 0 for every ray
    ])
    m, r = _masks(tools["on"], tmp_path, tris, "edge")
    assert [int(x) for x in m] == [0, OC.octants(2, 0), 0, 0, 0, OC.octants(2, 0), 255]
    assert r["violations"] == 0


def test_soup_pairs_hold_by_brute_force(tools, tmp_path):
    """Random triangles (zero-area ones, duplicates, non-finite vertices among them): whatever is certified
    holds; a general triangle is certified in at most one octant."""
    tris, _ = SS.soup(12, 200, nonfinite=True)
    m, r = _masks(tools["on"], tmp_path, tris, "soup")
    assert r["violations"] == 0 and r["pairs"] > 50
    pos = np.stack([tris[v]["position"][:, :3] for v in ("v1", "v2", "v3")], axis=1)
    assert not m[~np.isfinite(pos).all(axis=(1, 2))].any()
    assert not m[(np.abs(pos) > 2.0 ** 20).any(axis=(1, 2))].any()


def test_cornell_counts(tools, tmp_path, cornell):
    m, r = _masks(tools["on"], tmp_path, cornell.triangles, "cornell")
    print(r, [int(x) for x in m])
    assert r["violations"] == 0 and r["max_det_e12"] <= 0
    assert r["tris"] == CORNELL["tris"] and r["pairs"] == CORNELL["pairs"]
    assert int((m == 0).sum()) == CORNELL["refused"]


# ---- the pruned links -----------------------------------------------------------------------------------

def _files(tmp_path, scene, tag):
    nodes, tris = tmp_path / f"{tag}.nodes", tmp_path / f"{tag}.tris"
    np.ascontiguousarray(scene.nodes).tofile(nodes)
    np.ascontiguousarray(scene.triangles).tofile(tris)
    return nodes, tris


class Packed:
    def __init__(self, exe, tmp_path, scene, tag):
        nodes, tris = _files(tmp_path, scene, tag)
        self.info = _run(exe, "pack", nodes, tris, tmp_path / tag)
        self.n = self.info["n"]
        self.stride = (self.n + 1) | 1
        self.bofs = 512 if self.stride <= 64 else 8 * self.stride
        rd = lambda ext, t=np.uint32: np.fromfile(tmp_path / f"{tag}.{ext}", t)
        self.oct, self.octc, self.octp, self.goct, self.goctp = rd("oct"), rd("octc"), rd("octp"), rd("goct"), rd("goctp")
        self.mask = rd("mask", np.uint8)
        self.base = self.octc if self.octc.size else self.oct

    def links(self, recs):
        at = lambda i, o, k: int(recs[(self.bofs + o * self.stride + i) * 4 + k])
        return {(i, o): (at(i, o, 2), at(i, o, 3)) for i in range(self.n) for o in range(8)}


def _check_pruned(pk, nodes):
    """The pruned set of one packed scene against the restated rule; returns the changed words' count."""
    want = OC.expected_pruned(nodes, pk.n, pk.mask)
    base = pk.links(pk.base)
    changed = sum((a[0] != b[0]) + (a[1] != b[1]) for a, b in ((want[k], base[k]) for k in want))
    assert pk.info["pruned"] == changed
    if not changed:
        assert pk.octp.size == 0 and pk.goctp.size == 0
        return 0
    assert pk.links(pk.octp) == want
    # every word that is not a link of a node record is the base set's
    assert pk.octp.shape == pk.base.shape and int((pk.octp != pk.base).sum()) == changed
    # the regrouped set: the same links as walk words
    G = pk.info["group"]
    word = lambda i: (i // G) * 8 * G + i % G
    end = lambda w: w if w < pk.n else None
    for (i, o), (hit, miss) in want.items():
        at = (pk.info["goct_b"] + word(i) + o * G) * 4
        assert int(pk.goctp[at + 2]) == (hit if hit >= NC.LEAF_MIN else word(hit))
        if end(miss) is not None:
            assert int(pk.goctp[at + 3]) == word(miss)
    return changed


def test_room_links_by_rule_and_by_hand(tools, tmp_path):
    sc, at, _, _ = OC.room_scene()
    pk = Packed(tools["on"], tmp_path, sc, "room")
    assert pk.info["oct_ok"] == 1 and pk.info["links"] == 0
    assert _check_pruned(pk, sc.nodes) > 0
    got, plain = pk.links(pk.octp), pk.links(pk.oct)
    END = pk.n
    # octant 0 (all components positive): the floor F is culled, n1's near child
    assert plain[at["n1"], 0][0] == at["F"] and got[at["n1"], 0][0] == at["n3"]   # a culled leaf as near child
    assert got[at["n3"], 0] == plain[at["n3"], 0]
    # octant 1 (x negative): n1's near child is n3, whose near child W1 is culled; its far child is the culled floor
    assert plain[at["n3"], 1] == (at["W1"], at["F"]) and got[at["n3"], 1] == (at["G"], at["n6"])
    assert plain[at["G"], 1][1] == at["F"] and got[at["G"], 1][1] == at["n6"]     # a culled leaf as far child
    # octant 3 (x, y negative): after G come W1 and F, both culled: two in a row; n7 = {W2, B} is a culled
    # interior subtree, the far child of n6
    assert plain[at["G"], 3][1] == at["W1"] and plain[at["W1"], 3][1] == at["F"] and plain[at["F"], 3][1] == at["n6"]
    assert got[at["G"], 3][1] == at["n6"]
    assert plain[at["n6"], 3][0] == at["C"]                                       # axis 0, x set: the second child first
    assert plain[at["C"], 3][1] == at["n7"] and got[at["C"], 3][1] == END
    # octant 7: n6 = {n7, C} is culled as a whole; the root's near child is n6 (z set): the link moves on to n1
    assert plain[0, 7][0] == at["n6"] and got[0, 7][0] == at["n1"]
    # leaf codes never change
    for (i, o), (hit, _) in plain.items():
        if hit >= NC.LEAF_MIN:
            assert got[i, o][0] == hit


def test_corner_octant_with_everything_culled_keeps_its_links(tools, tmp_path):
    sc = OC.corner_scene()
    pk = Packed(tools["on"], tmp_path, sc, "corner")
    assert all(int(x) & 1 for x in pk.mask)
    assert _check_pruned(pk, sc.nodes) > 0
    got, base = pk.links(pk.octp), pk.links(pk.base)
    for i in range(pk.n):
        assert got[i, 0] == base[i, 0]
    assert not any(got[i, 7] != base[i, 7] for i in range(pk.n))   # octant 7 culls nothing: unchanged too
    assert any(got[i, 1] != base[i, 1] for i in range(pk.n))


def test_soup_tree_and_mixed_tree_follow_the_rule(tools, tmp_path):
    """Trees over random triangles (leaves partly certified: they stay) and the node-collapse tree, whose
    pruned set is built over collapsed links."""
    for tag, sc in (("mixed", NC.mixed_scene()[0]), ("ff", NC.chain_scene("ff"))):
        pk = Packed(tools["on"], tmp_path, sc, tag)
        assert pk.info["links"] > 0
        _check_pruned(pk, sc.nodes)


def test_cornell_links(tools, tmp_path, cornell):
    pk = Packed(tools["on"], tmp_path, cornell, "cornell")
    assert pk.n == 39 and pk.info["links"] == 20 and pk.info["pairs"] == CORNELL["pairs"]
    assert _check_pruned(pk, cornell.nodes) == CORNELL["pruned_links"] == pk.info["pruned"]
    # the collapsed set is word for word what it was
    off = Packed(tools["off"], tmp_path, cornell, "cornell_off")
    assert np.array_equal(off.octc, pk.octc) and np.array_equal(off.oct, pk.oct) and np.array_equal(off.goct, pk.goct)


def test_off_switch(tools, tmp_path, cornell):
    pk = Packed(tools["off"], tmp_path, cornell, "off")
    assert pk.info["pruned"] == 0 and pk.octp.size == 0 and pk.goctp.size == 0 and pk.info["links"] == 20


# ---- the replay walker ------------------------------------------------------------------------------------

def _rays(scene, seed, n_random=1500):
    """origin, direction x 6 float32, all 8 octants: random unit directions from inside and outside the root
    box, and axis-aligned directions with exact +0 / -0 components."""
    rng = np.random.default_rng(seed)
    lo, hi = scene.nodes["bmin"][0, :3], scene.nodes["bmax"][0, :3]
    ext = hi - lo
    out = []
    d = rng.normal(size=(n_random, 3))
    out.append(np.hstack([rng.uniform(lo, hi, (n_random, 3)), d / np.linalg.norm(d, axis=1, keepdims=True)]))
    o = rng.uniform(lo - 2 * ext, hi + 2 * ext, (n_random, 3))
    d = rng.uniform(lo, hi, (n_random, 3)) - o
    out.append(np.hstack([o, d / np.linalg.norm(d, axis=1, keepdims=True)]))
    for ax in range(3):
        for s in (1.0, -1.0):
            for z in (0.0, -0.0):
                d = np.full(3, z)
                d[ax] = s
                k = 40
                out.append(np.hstack([rng.uniform(lo - ext, hi + ext, (k, 3)), np.tile(d, (k, 1))]))
                out.append(np.hstack([rng.uniform(lo, hi, (k, 3)), np.tile(d, (k, 1))]))
    return np.ascontiguousarray(np.vstack(out), np.float32)


def _scenes(cornell):
    return {"cornell": cornell, "room": OC.room_scene()[0], "corner": OC.corner_scene(), "mixed": NC.mixed_scene()[0]}


@pytest.mark.parametrize("name", ["cornell", "room", "corner", "mixed"])
def test_replay_walks_agree(tools, tmp_path, cornell, name):
    sc = _scenes(cornell)[name]
    nodes, tris = _files(tmp_path, sc, name)
    rays = _rays(sc, 9)
    assert 3000 < len(rays) < 10000
    rays.tofile(tmp_path / "rays")
    r = _run(tools["on"], "walk", nodes, tris, tmp_path / "rays")
    print(name, r)
    assert r["rays"] == len(rays) and r["octants"] == 255
    assert r["mismatches"] == 0 and r["removed_accepts"] == 0
    assert r["tests_plain"] - r["tests_pruned"] == r["removed_tests"]
    assert r["hits"] > 0 and r["visits_pruned"] <= r["visits_collapsed"] <= r["visits_plain"]
    if name != "mixed":
        assert r["removed_tests"] > 0 and r["visits_pruned"] < r["visits_collapsed"]
    if name == "corner":  # all-or-nothing leaves: exactly the certified tests are gone
        assert r["certified_left"] == 0
    off = _run(tools["off"], "walk", nodes, tris, tmp_path / "rays")
    assert off["visits_pruned"] == off["visits_collapsed"] == r["visits_collapsed"] and off["mismatches"] == 0
    assert off["tests_pruned"] == r["tests_plain"]


def test_units_are_free_of_hip():
    for name in ("rt_octant_cull.cpp", "rt_octant_cull.hpp"):
        with open(os.path.join(CSRC, name)) as f:
            assert "#include <hip" not in f.read(), name

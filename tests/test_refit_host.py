"""CPU: the host refit (rtsRefitBounds, clrt.scene.refit) -- the CPU statement of the bounds rule the
device refit (rtRefitBVH) is compared with.

* unchanged geometry: the host SAH builder's bounds are what the rule gives (Cornell to the bit, the
  bunny proxy as floats);
* displaced geometry: bounds == a numpy fold, everything that is not a bound stays;
* hand-built trees (random axis flags, a chain, a 140-triangle leaf, garbage behind the tree), a
  one-leaf tree;
* malformed trees are an error code and nothing is written;
* the same cases, plus soups with overflowing / infinite / NaN vertices, through a stand-alone program
  built with -fsanitize=address,undefined.
"""
import os
import subprocess

import numpy as np
import pytest

import refit_ref as R
import stress_scenes as SS
from clrt import _native as N
from clrt import scene as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREES = R.tree_scenes()


def _bounds(nodes, end):
    return nodes["bmin"][:end, :3], nodes["bmax"][:end, :3]


def _check_refit(scene, tris):
    """refit of `scene`'s tree over `tris`: bounds == the numpy fold, the rest untouched."""
    out = S.refit(S.Scene(tris, scene.nodes, scene.materials, scene.max_prims_in_node)).nodes
    _, end = SS.tree_depth(scene.nodes)
    lo, hi = R.fold_bounds(tris, scene.nodes)
    glo, ghi = _bounds(out, end)
    assert np.array_equal(glo, lo) and np.array_equal(ghi, hi)
    R.assert_only_bounds_changed(scene.nodes, out)
    for f in ("offset", "nPrimitives", "axis", "pad"):
        assert np.array_equal(out[f], scene.nodes[f])
    return out


def test_unchanged_cornell_is_bit_identical(cornell):
    out = S.refit(cornell)
    assert out.nodes.tobytes() == cornell.nodes.tobytes()
    assert out.triangles is cornell.triangles and out.nodes is not cornell.nodes


def test_unchanged_proxy_is_value_identical():
    import clrt.proxy as P
    proxy = P.bunny_proxy()
    out = S.refit(proxy).nodes
    assert np.array_equal(out["bmin"][:, :3], proxy.nodes["bmin"][:, :3])
    assert np.array_equal(out["bmax"][:, :3], proxy.nodes["bmax"][:, :3])
    R.assert_only_bounds_changed(proxy.nodes, out)


def test_displaced_cornell(cornell):
    moved = R.displaced(cornell.triangles, 5)
    out = _check_refit(cornell, moved)
    assert (out["bmin"][:, :3] != cornell.nodes["bmin"][:, :3]).any()


@pytest.mark.parametrize("tree", list(TREES))
def test_trees(tree):
    scene = TREES[tree]()
    _check_refit(scene, scene.triangles)               # (hand-built bounds skip non-finite vertices only)
    out = _check_refit(scene, R.displaced(scene.triangles, 7))
    _, end = SS.tree_depth(scene.nodes)
    assert len(scene.nodes) > end                      # garbage records behind the tree: byte-identical
    assert out[end:].tobytes() == scene.nodes[end:].tobytes()


def _malformed(cornell):
    """name -> (triangle count, nodes): each breaks one rule of the tree contract."""
    nt = cornell.n_triangles
    a = cornell.nodes.copy()
    a["offset"][0] = 1                                 # second child <= first child
    b = cornell.nodes.copy()
    leaf = int(np.flatnonzero(b["nPrimitives"] > 0)[-1])
    b["offset"][leaf] = nt                             # leaf range beyond n_tris
    return {"second_child": (nt, a), "leaf_range": (nt, b)}


@pytest.mark.parametrize("case", ["second_child", "leaf_range"])
def test_malformed_tree_is_an_error_and_writes_nothing(cornell, case):
    nt, nodes = _malformed(cornell)[case]
    before = nodes.tobytes()
    tris = np.ascontiguousarray(cornell.triangles)
    rc = N.scene_lib().rtsRefitBounds(tris.ctypes.data, nt, nodes.ctypes.data, len(nodes))
    assert rc != 0
    assert nodes.tobytes() == before
    with pytest.raises(N.RTError):
        S.refit(S.Scene(cornell.triangles, nodes, cornell.materials))


def test_null_and_empty_arguments(cornell):
    lib = N.scene_lib()
    tris = np.ascontiguousarray(cornell.triangles)
    assert lib.rtsRefitBounds(tris.ctypes.data, len(tris), None, 0) != 0
    nodes = cornell.nodes.copy()
    assert lib.rtsRefitBounds(None, len(tris), nodes.ctypes.data, len(nodes)) != 0


# ---- the same under AddressSanitizer + UBSan: a stand-alone program, nothing loaded into Python ----
@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("refit_san") / "refit_sanitize_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                    os.path.join(REPO, "tests", "native", "refit_sanitize_main.cpp"),
                    os.path.join(REPO, "mini-opencl-raytracer_amd", "host", "scene.cpp")],
                   check=True, timeout=600)
    return exe


def _run_sanitized(exe, tmp_path, tris, nodes):
    tp, np_, op = (str(tmp_path / n) for n in ("t.bin", "n.bin", "o.bin"))
    np.ascontiguousarray(tris).tofile(tp)
    np.ascontiguousarray(nodes).tofile(np_)
    p = subprocess.run([exe, tp, np_, op], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-4000:]
    return int(p.stdout.strip()), np.fromfile(op, N.NODE_DTYPE)


def test_sanitized_refit(sanitized, tmp_path, cornell):
    cases = {"cornell": (cornell, cornell.triangles), "cornell_moved": (cornell, R.displaced(cornell.triangles, 5))}
    for name, make in TREES.items():
        scene = make()
        cases[name] = (scene, R.displaced(scene.triangles, 7))
    for tree in ("rt7", "chain", "big"):
        scene = SS.soup_scene(12, tree, nonfinite=True)
        cases[tree + "_nonfinite"] = (scene, scene.triangles)
    for name, (scene, tris) in cases.items():
        rc, out = _run_sanitized(sanitized, tmp_path, tris, scene.nodes)
        assert rc == 0, name
        want = S.refit(S.Scene(tris, scene.nodes, scene.materials)).nodes
        assert out.tobytes() == want.tobytes(), name
        _, end = SS.tree_depth(scene.nodes)
        lo, hi = R.fold_bounds(tris, scene.nodes)
        # (== on floats: an all-NaN axis folds to the empty box +inf / -inf in both)
        assert np.array_equal(out["bmin"][:end, :3], lo) and np.array_equal(out["bmax"][:end, :3], hi), name
    for name, (nt, nodes) in _malformed(cornell).items():
        rc, out = _run_sanitized(sanitized, tmp_path, cornell.triangles, nodes)
        assert rc != 0, name
        assert out.tobytes() == nodes.tobytes(), name

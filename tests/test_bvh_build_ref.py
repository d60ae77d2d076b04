"""CPU: the numpy restatement of the device BVH builders (bvh_build_ref.py) and its cases.

The GPU tests (test_device_bvh.py) ask the builder for the reference's bytes, so the reference itself
is held here to what rt_hip.h documents -- a valid depth-first tree, leaves <= max_prims, the bounds
rule of rtRefitBVH on every plane of every node -- and the cases to the conditions that make them
worth comparing (ties, forced rounds, both orientations, every axis and leaf size, unclipped windows).
"""
import numpy as np
import pytest

import bvh_build_ref as R
from clrt import _native as N
from clrt import scene as S
from test_scene import _check_bvh

INPUTS = sorted({name for name, _ in R.CASES}, key=[name for name, _ in R.CASES].index)
SOUPS = [c for c in R.CASES if c[0].startswith("soup")]


def _scene(case, method):
    tris, nodes, _ = R.reference(case[0], case[1], method)
    return S.Scene(tris, nodes, np.zeros(6, N.MATERIAL_DTYPE), case[1])


def _rows(tris):
    return sorted(bytes(r) for r in np.ascontiguousarray(tris).view(np.uint8).reshape(len(tris), -1))


def test_case_list_covers_the_size_edges():
    """Block edge 256, window edge 2 * 32 + 1, the m > 64 force rule, 64 * 256 grid stride, one-leaf inputs."""
    sizes = {int(name[4:]) for name, _ in SOUPS}
    assert sizes == {2, 3, 5, 33, 64, 65, 66, 255, 256, 257, 1025, 4097, 16385}
    for name in INPUTS:
        want = {1, 2, 4, 8} if name == "soup257" else {1, 4}
        assert {mp for nm, mp in R.CASES if nm == name} == want
    assert {"cornell", "identical", "coplanar_grid", "one_point", "nonfinite"} <= set(INPUTS)
    assert [len(R.case_triangles(n)) for n in ("cornell", "identical", "coplanar_grid", "one_point", "nonfinite")] \
        == [72, 2000, 20000, 500, 202]


@pytest.mark.parametrize("name", INPUTS)
def test_no_case_holds_a_negative_zero(name):
    p = R.positions(R.case_triangles(name))
    assert not ((p == 0) & np.signbit(p)).any()


def test_clamp_is_rtBuildBVHEx_s():
    assert [R.clamp_max_prims(v) for v in (0, 1, 4, 65535, 65536, 100000, 0xFFFFFFFF)] == [1, 1, 4, 65535, 65535, 65535, 65535]


def test_one_point_centroids_are_equal_and_triangles_differ():
    t = R.case_triangles("one_point")
    c = R.centroids(R.positions(t))
    assert (c.view(np.uint32) == c[0].view(np.uint32)).all()
    assert len(set(_rows(t))) == len(t)
    assert not R.morton_codes(R.positions(t)).any()


def test_nonfinite_holds_an_all_nan_axis_and_an_all_inf_vertex():
    p = R.positions(R.case_triangles("nonfinite"))
    assert np.isnan(p[:, :, 1]).all(axis=1).any()
    assert np.isposinf(p).all(axis=2).any()
    lo, hi = R.tri_boxes(p)
    assert not np.isnan(lo).any() and not np.isnan(hi).any()


@pytest.mark.parametrize("method", R.METHODS)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_reference_tree(case, method):
    src = R.case_triangles(case[0])
    sc = _scene(case, method)
    n = len(src)
    if R.finite_input(case[0]):
        _check_bvh(sc)
    assert N.validate_bvh(sc.nodes, n) >= 0
    leaf = sc.nodes["nPrimitives"] > 0
    assert sc.nodes["nPrimitives"].max() <= case[1]
    assert int(sc.nodes["nPrimitives"].sum()) == n
    assert len(sc.nodes) <= 2 * n - 1 and (case[1] != 1 or len(sc.nodes) == 2 * n - 1)
    assert _rows(sc.triangles) == _rows(src)
    assert (sc.nodes["axis"] <= 2).all() and not sc.nodes["axis"][leaf].any()
    assert not sc.nodes["pad"].any()
    assert not sc.nodes["bmin"][:, 3].view(np.uint32).any() and not sc.nodes["bmax"][:, 3].view(np.uint32).any()
    # the documented bounds rule, all six planes of every node, bit for bit (the all-NaN axis included)
    assert R.first_difference(sc.nodes, S.refit(sc).nodes) is None


@pytest.mark.parametrize("method", R.METHODS)
def test_max_prims_clamp_in_the_reference(method):
    t = R.identical(300)
    cache = {}
    zero, one = (R.build(t, mp, method, cache)[1] for mp in (0, 1))
    assert zero.tobytes() == one.tobytes() and len(zero) == 599
    assert len(R.build(t, 100000, method, cache)[1]) == 1


# ---- input conditions: a case that misses one is changed, never the condition --------------------
def _stats(name, mp, method):
    return R.reference(name, mp, method)[2]


@pytest.mark.parametrize("name", ["cornell", "identical", "one_point"])
def test_equal_morton_codes_exist(name):
    assert _stats(name, 4, "lbvh")["equal_code_pairs"] >= 1


def test_forced_rounds_on_identical_and_none_on_the_soups():
    st = _stats("identical", 4, "ploc")
    assert st["forced_rounds"] >= 1 and st["rounds"] > st["forced_rounds"]
    for name, mp in SOUPS:
        assert _stats(name, mp, "ploc")["forced_rounds"] == 0, name


def test_orient_swaps_and_keeps():
    for name in ("soup257", "soup4097", "cornell", "one_point", "nonfinite"):
        st = _stats(name, 4, "ploc")
        assert st["swaps"] >= 1 and st["non_swaps"] >= 1, name


@pytest.mark.parametrize("method", R.METHODS)
def test_every_axis_occurs_over_the_soups(method):
    hist = np.sum([_stats(name, mp, method)["axis_hist"] for name, mp in SOUPS], axis=0)
    assert (hist > 0).all(), hist


@pytest.mark.parametrize("method", R.METHODS)
def test_every_leaf_size_occurs_at_max_prims_4(method):
    hist = np.zeros(5, np.int64)
    for name, mp in R.CASES:
        if mp == 4:
            h = _stats(name, mp, method)["leaf_size_hist"]
            hist[:len(h)] += h
    assert (hist[1:] > 0).all(), hist


@pytest.mark.parametrize("n", [65, 66])
def test_windows_clipped_on_neither_side(n):
    assert _stats(f"soup{n}", 4, "ploc")["unclipped_windows"] >= n - 2 * R.PLOC_RADIUS >= 1
    assert _stats("soup64", 4, "ploc")["unclipped_windows"] == 0

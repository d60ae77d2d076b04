"""Shared pieces of the refit tests (test_refit_host.py, test_refit_gpu.py): the bounds rule as a
numpy fold, the displacement recipe, and the scenes neither stress_scenes nor the fixtures hold."""
import functools

import numpy as np

import stress_scenes as SS
from clrt import _native as N
from clrt import scene as S

VERTS = ("v1", "v2", "v3")


def positions(tris):
    """(n, 3, 3) float32: triangle, vertex, xyz."""
    return np.stack([tris[v]["position"][:, :3] for v in VERTS], axis=1).astype(np.float32)


def fold_bounds(tris, nodes):
    """The bounds rule: (lo, hi) of shape (tree nodes, 3) -- a leaf's box is the fmin / fmax fold
    (NaN ignored) over its triangles' vertices, an interior box that of its two children."""
    _, end = SS.tree_depth(nodes)
    p = positions(tris)
    lo = np.full((end, 3), np.inf, np.float32)
    hi = np.full((end, 3), -np.inf, np.float32)
    for i in range(end - 1, -1, -1):
        off, cnt = int(nodes["offset"][i]), int(nodes["nPrimitives"][i])
        if cnt > 0:
            q = p[off:off + cnt].reshape(-1, 3)
            lo[i] = np.fmin.reduce(q, axis=0, initial=np.float32(np.inf))
            hi[i] = np.fmax.reduce(q, axis=0, initial=np.float32(-np.inf))
        else:
            lo[i] = np.fmin(lo[i + 1], lo[off])
            hi[i] = np.fmax(hi[i + 1], hi[off])
    return lo, hi


def displaced(tris, seed, sigma=0.5):
    """A copy of `tris` with every vertex coordinate moved by a seeded normal(0, sigma)."""
    rng = np.random.default_rng(seed)
    out = tris.copy()
    for v in VERTS:
        out[v]["position"][:, :3] += rng.normal(0.0, sigma, (len(tris), 3)).astype(np.float32)
    return out


def tri_points(a):
    """(n, 3, 3) -> n N.TRI_POINTS_DTYPE records (w slots filled with a marker the update must ignore)."""
    a = np.asarray(a, np.float32).reshape(-1, 3, 3)
    out = np.zeros(len(a), N.TRI_POINTS_DTYPE)
    for i, f in enumerate(("p1", "p2", "p3")):
        out[f][:, :3] = a[:, i]
        out[f][:, 3] = 12345.0
    return out


def non_bounds_view(nodes):
    """The bytes of node records a refit must keep: the w slots and bytes 32..47."""
    raw = np.ascontiguousarray(nodes).view(np.uint8).reshape(-1, 48)
    return np.concatenate([raw[:, 12:16], raw[:, 28:32], raw[:, 32:48]], axis=1)


def assert_only_bounds_changed(before, after):
    _, end = SS.tree_depth(before)
    assert np.array_equal(non_bounds_view(before), non_bounds_view(after))
    assert np.ascontiguousarray(before[end:]).tobytes() == np.ascontiguousarray(after[end:]).tobytes()


@functools.lru_cache(maxsize=None)
def one_leaf_scene():
    """The root is a leaf of five triangles (no climb), two garbage records behind it."""
    tris, mats = SS.soup(12, 5)
    nodes = np.zeros(3, N.NODE_DTYPE)
    lo, hi = SS._bounds(tris, 0, 5)
    nodes["bmin"][0, :3], nodes["bmax"][0, :3] = lo, hi
    nodes["bmin"][0, 3], nodes["bmax"][0, 3] = 7.0, -7.0  # w slots: kept
    nodes["offset"][0], nodes["nPrimitives"][0] = 0, 5
    nodes["offset"][1:] = 0xDEADBEEF
    nodes["bmin"][1:, :3] = 3.5
    return S.Scene(tris, nodes, mats, 5)


@functools.lru_cache(maxsize=None)
def big_soup_scene():
    """6,000 triangles under the host SAH tree: read from HBM/L2, several workgroups climb one tree."""
    tris, mats = SS.soup(21, 6000)
    return S.build_bvh(tris, mats, 4)


# name -> scene factory: the trees every bounds test walks
def tree_scenes():
    out = {t: functools.partial(SS.soup_scene, 12, t) for t in ("rt1", "rt7", "rt127", "chain", "big")}
    out["one_leaf"] = one_leaf_scene
    return out

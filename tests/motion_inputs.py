"""Seeded inputs of the motion tests (CPU: test_motion_plan.py, GPU: test_motion_gpu.py), made once and shared,
never modified.

The scene is the Cornell fixture (tests/golden/cornell.rtscene, 72 triangles); its short box is the 24 triangles of
material 5, which lie scattered in [8, 68) of the triangle order, so a move of that range has moved and unmoved
triangles inside it.

The motion variants run on test_temporal_gpu's wall-and-slab views with motion records made here: every covered
pixel's record holds the world point its depth gives, displaced by a motion of its surface since the previous time
-- the slab came from 0.8 to the right, the wall slid 1.0 from the left -- and its normal; uncovered pixels and
about 3 % of the covered ones are misses (prim -1); about 3 % carry a tilted previous normal that fails the normal
test.  Depths along the wall do not change under either displacement, so history is kept wherever the displaced
point is seen in the previous view on the same surface.
"""
import functools
import struct

import numpy as np

import motion_ref as ref
import temporal_ref
from clrt import _native as N
from reproject_samples_inputs import seeded_stats
from test_temporal_gpu import PAIRS, PREV, SIZES, synthetic as temporal_synthetic

F = np.float32
NAN_BYTE = 0xFF
SHORT_BOX_MATERIAL = 5
BOX_RANGE = (8, 60)            # first_tri, n_tris: the short box's triangles and the ones between them
BOX_SHIFT = (-1.5, 0.5, 0.0)   # the end-to-end move
SLAB_CAME_FROM, WALL_CAME_FROM = (0.8, 0.0, 0.0), (-1.0, 0.0, 0.0)


@functools.lru_cache(maxsize=None)
def scene():
    import clrt
    return clrt.scene.cornell()


def short_box(tris):
    return tris["mtlIndex"] == SHORT_BOX_MATERIAL


@functools.lru_cache(maxsize=None)
def moved_scene(shift=BOX_SHIFT):
    """(positions, normals) of every triangle after the short box was translated by `shift`: (72, 3, 3) each."""
    tris = scene().triangles
    pos, nrm = ref.vertices(tris, "position"), ref.vertices(tris, "normal")
    pos = pos.copy()
    pos[short_box(tris)] += np.asarray(shift, F)
    pos.setflags(write=False)
    nrm.setflags(write=False)
    return pos, nrm


def float_classes():
    tiny, big = F(1e-45), F(3.4028235e38)
    classes = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, tiny, -tiny, big, -big, 1e-38, -20.0], F)
    return np.concatenate([classes, np.array([0x7F800001, 0xFFC12345], np.uint32).view(F)])


@functools.lru_cache(maxsize=None)
def seeded_hits(n, n_scene=72):
    """n RAY_HIT_DTYPE records: prims mostly inside the scene, some just outside, negative or extreme; barycentrics
    mostly inside the triangle, a fifth of them from reproject_samples_inputs.non_finite_inputs' class list."""
    rng = np.random.default_rng(7000 + n)
    hits = np.zeros(n, N.RAY_HIT_DTYPE)
    hits["prim"] = rng.integers(0, n_scene, n)
    odd = rng.random(n) < 0.25
    hits["prim"][odd] = rng.choice(np.array([-1, -2, n_scene, n_scene + 1, 2 ** 31 - 1, -2 ** 31, 1 << 24, -72], np.int64),
                                   int(odd.sum())).astype(np.int32)
    u = rng.random(n).astype(F)
    hits["u"], hits["v"] = u, (rng.random(n).astype(F) * (F(1) - u))
    hits["t"] = (rng.random(n) * 30).astype(F)
    for name in ("u", "v"):
        at = rng.random(n) < 0.2
        hits[name][at] = rng.choice(float_classes(), int(at.sum()))
    if n == 1:
        hits["prim"], hits["u"], hits["v"] = 9, 0.25, 0.5
    hits.setflags(write=False)
    return hits


def pack_hits(tris, first_tri, n_tris, prev_pos, prev_nrm, hits):
    """The input file of `motion_main hit`."""
    head = struct.pack("<5I", len(tris), first_tri, n_tris, int(prev_nrm is not None and n_tris > 0), len(hits))
    parts = [np.ascontiguousarray(tris).tobytes()]
    if n_tris:
        parts.append(np.ascontiguousarray(prev_pos[:n_tris]).tobytes())
        if prev_nrm is not None:
            parts.append(np.ascontiguousarray(prev_nrm[:n_tris]).tobytes())
    return head + b"".join(parts) + np.ascontiguousarray(hits).tobytes()


@functools.lru_cache(maxsize=None)
def motion_records(w, h, pair):
    """MOTION records of the current view of test_temporal_gpu.synthetic(w, h, pair); read-only."""
    _, cf, _, _, view = temporal_synthetic(w, h, pair)
    pos, front, up = (np.asarray(v, F) for v in view)
    rng = np.random.default_rng(2000 * w + h)
    u = temporal_ref.centre_rays(w, h, front, up)
    X = pos + u * cf["depth"][..., None]
    on_slab = cf["depth"] < F(0.9) * (F(20) - pos[1]) / np.maximum(u[..., 1], F(1e-6))
    m = np.zeros((h, w), ref.MOTION)
    m["prev_point"] = X + np.where(on_slab[..., None], np.asarray(SLAB_CAME_FROM, F), np.asarray(WALL_CAME_FROM, F))
    covered = cf["coverage"] > 0
    m["prim"] = np.where(covered, rng.integers(0, 72, (h, w)), -1)
    m["prev_normal"][..., 1] = -1
    m["flags"] = on_slab
    if w * h > 1:
        m["prim"][(rng.random((h, w)) < 0.03)] = -1
        tilt = rng.random((h, w)) < 0.03
        m["prev_normal"][tilt] = np.array([0.8, -0.6, 0.0], F)
    m["prev_point"][m["prim"] < 0] = 0
    m["prev_normal"][m["prim"] < 0] = 0
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def temporal_reference(w, h, pair):
    import test_temporal_gpu as T
    cur, cf, hist, hf, view = temporal_synthetic(w, h, pair)
    out, info = ref.temporal(cur, cf, hist, hf, motion_records(w, h, pair), w, h, view, PREV, **T.DEFAULTS, details=True)
    out.setflags(write=False)
    return out, info


@functools.lru_cache(maxsize=None)
def stats_synthetic(w, h):
    st = seeded_stats(w, h, np.random.default_rng(3000 * w + h))
    if w * h == 1:
        st["n"] = 5.0
    st.setflags(write=False)
    return st


@functools.lru_cache(maxsize=None)
def reproject_reference(w, h, pair):
    from reproject_samples_inputs import DEFAULTS
    _, cf, _, hf, view = temporal_synthetic(w, h, pair)
    out, info = ref.reproject(stats_synthetic(w, h), hf, cf, motion_records(w, h, pair), w, h, view, PREV, **DEFAULTS,
                              details=True)
    out.setflags(write=False)
    return out, info


def non_finite_motion(w=61, h=7, pair="shift"):
    """motion_records(w, h, pair) with a fifth of the previous points and a tenth of the previous normals of any
    class, component by component."""
    m = np.array(motion_records(w, h, pair))
    rng = np.random.default_rng(77)
    for name, share in (("prev_point", 0.2), ("prev_normal", 0.1)):
        at = rng.random((h, w, 3)) < share
        m[name][at] = rng.choice(float_classes(), int(at.sum()))
    return m


def pack_project(w, h, cur_view, prev_view, depth_tolerance, normal_threshold, motion, hist_features):
    """The input file of `motion_main project`."""
    views = [float(c) for v in (cur_view, prev_view) for part in v for c in part]
    head = struct.pack("<2I18f2f", w, h, *views, depth_tolerance, normal_threshold)
    return head + np.ascontiguousarray(motion).tobytes() + np.ascontiguousarray(hist_features).tobytes()


PROJECT_OUT = np.dtype([("ok", np.uint32), ("x0", np.int32), ("y0", np.int32), ("tx", F), ("ty", F), ("de", F),
                        ("inside", np.uint8, (4,)), ("on", np.uint8, (4,))])

__all__ = ["BOX_RANGE", "BOX_SHIFT", "NAN_BYTE", "PAIRS", "PREV", "SIZES", "float_classes", "motion_records",
           "moved_scene", "non_finite_motion", "pack_hits", "pack_project", "reproject_reference", "scene",
           "seeded_hits", "short_box", "stats_synthetic", "temporal_reference"]

"""Seeded synthetic inputs of the sample-reprojection tests (CPU: test_reproject_samples_plan.py, GPU:
test_reproject_samples_gpu.py), made once per size and camera pair and shared, never modified.

The scene, the camera pairs and the sizes are test_temporal_gpu.py's: a wall at y = 20 and a nearer slab, about
20 % of the pixels uncovered, about 5 % of the covered ones with coverage 0.75 and a shortened normal.  The history
statistics: n drawn from 0 .. 8, so that n = 0 (the tap does not count), n = 1 (the single-sample rule) and n >= 2
all occur; sums, means and m2_y finite and non-negative; the reserved words set, so that a copy of them would show.
"""
import functools
import struct

import numpy as np

import reproject_samples_ref as ref
from test_temporal_gpu import PAIRS, PREV, SIZES, scene_features

F = np.float32
DEFAULTS = dict(max_history=16.0, depth_tolerance=0.05, normal_threshold=0.9)
VARIANTS = {"defaults": {}, "cap": {"max_history": 3.0}, "depth_exact": {"depth_tolerance": 0.0},
            "any_normal": {"normal_threshold": -1.0}}
NAN_BYTE = 0xFF


def seeded_stats(w, h, rng):
    st = np.zeros((h, w), ref.STATS)
    n = rng.integers(0, 9, (h, w)).astype(F)
    st["n"] = n
    st["sum"] = (rng.random((h, w, 3)) * 2).astype(F) * n[..., None]
    st["mean_y"] = (rng.random((h, w)) * 2).astype(F)
    st["m2_y"] = (rng.random((h, w)) * 3).astype(F) * n
    st["reserved"] = 0xDEADBEEF
    return st


@functools.lru_cache(maxsize=None)
def synthetic(w, h, pair):
    """(hist_stats, hist_features, cur_features, cur view); read-only."""
    rng = np.random.default_rng(1000 * w + h)
    hs = seeded_stats(w, h, rng)
    if w * h == 1:
        hs["n"] = 5.0
    hf = scene_features(w, h, PREV, rng, uncover=w * h > 1)
    cf = scene_features(w, h, PAIRS[pair], rng, uncover=w * h > 1)
    for a in (hs, hf, cf):
        a.setflags(write=False)
    return hs, hf, cf, PAIRS[pair]


def params(variant):
    return {**DEFAULTS, **VARIANTS[variant]}


@functools.lru_cache(maxsize=None)
def reference(w, h, pair, variant="defaults"):
    hs, hf, cf, view = synthetic(w, h, pair)
    out, info = ref.reproject(hs, hf, cf, w, h, view, PREV, **params(variant), details=True)
    out.setflags(write=False)
    return out, info


def non_finite_inputs():
    """61 x 7, "shift", with non-finite values only where the definition selects them away: depths of both views
    of any class; NaN coverages; statistics of 0xFF bytes on taps whose features cannot count, and a NaN n (with
    NaN and infinite fields beside it) on some that could."""
    w, h = 61, 7
    hs, hf, cf, view = (np.array(a) if isinstance(a, np.ndarray) else a for a in synthetic(w, h, "shift"))
    rng = np.random.default_rng(99)
    tiny, big = F(1e-45), F(3.4028235e38)
    classes = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, tiny, -tiny, big, -big, 1e-38, -20.0], F)
    classes = np.concatenate([classes, np.array([0x7F800001, 0xFFC12345], np.uint32).view(F)])
    for a in (cf["depth"], hf["depth"]):
        at = rng.random((h, w)) < 0.2
        a[at] = rng.choice(classes, int(at.sum()))
    for a in (cf["coverage"], hf["coverage"]):
        a[rng.random((h, w)) < 0.05] = np.nan
    dead = ~(hf["coverage"] > 0)
    hs.view(np.uint8).reshape(h, w, 32)[dead & (rng.random((h, w)) < 0.7)] = NAN_BYTE
    nan_n = ~dead & (rng.random((h, w)) < 0.1)
    hs["n"][nan_n] = np.nan
    hs["sum"][nan_n] = np.array([np.inf, np.nan, -np.inf], F)
    hs["mean_y"][nan_n], hs["m2_y"][nan_n] = np.nan, -np.inf
    return w, h, hs, hf, cf, view, dead, nan_n


def pack(w, h, cur_view, prev_view, prm, hs, hf, cf):
    """The input file of `reproject_samples_plan_main merge`."""
    views = [float(c) for v in (cur_view, prev_view) for part in v for c in part]
    head = struct.pack("<2I18f3f", w, h, *views, prm["max_history"], prm["depth_tolerance"], prm["normal_threshold"])
    return head + b"".join(np.ascontiguousarray(a).tobytes() for a in (hs, hf, cf))


__all__ = ["DEFAULTS", "NAN_BYTE", "PAIRS", "PREV", "SIZES", "VARIANTS", "non_finite_inputs", "pack", "params",
           "reference", "seeded_stats", "synthetic"]

"""GPU: the step schedule's traversal decision (step_body, rt_kernels_body.hpp) at the smallest
shapes where its tests can go wrong.  The decision keeps its wave-uniform flags (`exhausted`, `dry`,
`chunk_tail`) in scalar registers, decides "refill is due" once per outer iteration instead of at
every traversal step, and classifies the lanes (node, leaf, END) once per decision, the END lanes
of the last decision being the shading predicate.  None of that may move a node visit, a triangle
test, a shading round or an RNG draw, so every case here is compared bit for bit (radiance, primary
hit ids and t) and counter for counter (rays, node visits, triangle tests, hits) against the CPU
oracle in pinned math -- as one fused launch and as per-frame launches, with and without the
per-frame sky key, in the timed kernels and in their counting variants -- and in shipped math the
fused launch against the same frames issued as per-frame launches.

The shapes:
  8x8, 24x16 (1 and 3 fused frames)  the work counter runs dry inside the first refill: `exhausted`
                                     is set with idle lanes left
  70x9                               a width that is no multiple of 8: tiles with fewer than 64 valid
                                     lanes, and a tile row of which one pixel row exists
  64x64, lightBounces 0 and 1        0: every popped lane is DONE, the traversal loop must end at its
                                     first test; 1: every path is done after one shading round
  64x64, refill_min / shade_min at   the refill and the shade gate fire in every or in no outer
  the ends of their ranges           iteration (the ranges are those of tuning_table.KNOBS)
  128x128 bunny proxy                the same body with the HBM/L2 octant walk's template arguments,
                                     and with those of the plain global walk (global_oct 0)
"""
import numpy as np
import pytest

from clrt import _native as N
from hip_helpers import HipRenderer, rgb
from tuning_table import KNOBS

pytestmark = pytest.mark.gpu
COUNTERS = ("rays", "node_visits", "tri_tests", "hits")
_RANGE = {name: (lo, hi) for name, _, lo, hi, _ in KNOBS}

# id: (scene, W, H, fused frames, lightBounces, tuning)
CASES = {
    "8x8-f1": ("cornell", 8, 8, 1, 9, {}),
    "8x8-f3": ("cornell", 8, 8, 3, 9, {}),
    "24x16-f1": ("cornell", 24, 16, 1, 9, {}),
    "24x16-f3": ("cornell", 24, 16, 3, 9, {}),
    "70x9": ("cornell", 70, 9, 2, 9, {}),
    "bounces0": ("cornell", 64, 64, 2, 0, {}),
    "bounces1": ("cornell", 64, 64, 2, 1, {}),
    "refill-lo": ("cornell", 64, 64, 2, 9, {"refill_min": _RANGE["refill_min"][0]}),
    "refill-hi": ("cornell", 64, 64, 2, 9, {"refill_min": _RANGE["refill_min"][1]}),
    "shade-lo": ("cornell", 64, 64, 2, 9, {"shade_min": _RANGE["shade_min"][0]}),
    "shade-hi": ("cornell", 64, 64, 2, 9, {"shade_min": _RANGE["shade_min"][1]}),
    "bunny-octant": ("bunny", 128, 128, 2, 9, {}),
    "bunny-global": ("bunny", 128, 128, 2, 9, {"global_oct": 0}),
}

_scenes = {}
_refs = {}


def _scene(name, cornell):
    if name == "cornell":
        return cornell
    if name not in _scenes:
        from clrt import proxy
        _scenes[name] = proxy.bunny_proxy()
    return _scenes[name]


def _reference(case, cornell, oracle_mod):
    """Frames 1..F of the case from the CPU oracle, computed once: (result, last frame's primary
    hit ids and t, the counters summed over the frames)."""
    if case not in _refs:
        scene, W, H, F, lb, _ = CASES[case]
        res = np.zeros((W * H, 4), np.float32)
        counts = dict.fromkeys(COUNTERS, 0)
        ids = t = None
        for f in range(1, F + 1):
            res, ids, t, c = oracle_mod.render(_scene(scene, cornell), W, H, frame_count=f, light_bounces=lb,
                                               result=res, want_hits=True, threads=16)
            for key in COUNTERS:
                counts[key] += c[key]
        for a in (res, ids, t):
            a.setflags(write=False)
        _refs[case] = (res, ids, t, counts)
    return _refs[case]


def _render(case, cornell, math, fused, stats, sky=None):
    scene, W, H, F, lb, tuning = CASES[case]
    r = HipRenderer(_scene(scene, cornell), W, H, math=math, hits=True, stats=stats)
    r.ctx.WriteBuffer(r.hit_bufs[0], np.full(W * H, -2, np.int32))  # "never written"
    r.k.set_tuning("perframe_defer", 0)  # per-frame launches render into the output themselves
    if sky is not None:
        r.k.set_tuning("perframe_sky", sky)
    for name, value in tuning.items():
        r.k.set_tuning(name, value)
    if fused:
        r.frame(1, light_bounces=lb, n_frames=F)
    else:
        for f in range(1, F + 1):
            r.frame(f, light_bounces=lb)
    out = (r.result(), r.hits(), r.k.stats() if stats else None, r.k.scene_in_lds())
    r.close()
    assert out[3] == (scene == "cornell")
    return out


def _bits(a, b, what):
    a = np.ascontiguousarray(a).view(np.uint32).ravel()
    b = np.ascontiguousarray(b).view(np.uint32).ravel()
    diff = np.flatnonzero(a != b)
    assert diff.size == 0, f"{what}: {diff.size} words differ, first at {diff[:8]}"


def _check_oracle(got, ref, what):
    res, ids, t, counts = ref
    _bits(rgb(got[0]), rgb(res), f"{what}: radiance")
    assert np.array_equal(got[1][0], ids), f"{what}: {(got[1][0] != ids).sum()} primary hit ids differ"
    _bits(got[1][1], t, f"{what}: hit t")
    if got[2] is not None:
        for key in COUNTERS:
            assert got[2][key] == counts[key], f"{what}: {key} {got[2][key]} != {counts[key]}"


@pytest.mark.parametrize("case", list(CASES))
def test_fused_pinned_equals_oracle(cornell, oracle_mod, case):
    ref = _reference(case, cornell, oracle_mod)
    for stats in (False, True):
        _check_oracle(_render(case, cornell, N.MATH_PINNED, True, stats), ref, f"fused, stats {stats}")


@pytest.mark.parametrize("case", list(CASES))
def test_per_frame_pinned_equals_oracle(cornell, oracle_mod, case):
    """Per-frame launches: paths end through the finish queue (sky key off) or, for primary misses
    whose stored value follows the key chain, through the sky key (perframe_sky 2: always)."""
    ref = _reference(case, cornell, oracle_mod)
    for sky in (0, 2):
        for stats in (False, True):
            _check_oracle(_render(case, cornell, N.MATH_PINNED, False, stats, sky), ref,
                          f"per-frame, sky key {sky}, stats {stats}")


@pytest.mark.parametrize("case", list(CASES))
def test_fused_shipped_equals_per_frame(cornell, case):
    a = _render(case, cornell, N.MATH_SHIPPED, True, True)
    assert (a[1][0] >= -1).all()  # every pixel's primary hit was written (-1: a miss)
    for sky in (0, 2):
        b = _render(case, cornell, N.MATH_SHIPPED, False, True, sky)
        _bits(a[0], b[0], f"sky key {sky}: output")
        assert np.array_equal(a[1][0], b[1][0]), f"sky key {sky}: primary hit ids"
        _bits(a[1][1], b[1][1], f"sky key {sky}: hit t")
        for key in COUNTERS:
            assert a[2][key] == b[2][key], f"sky key {sky}: {key}"
    # the timed kernels (no counters) against their counting variants
    c = _render(case, cornell, N.MATH_SHIPPED, True, False)
    _bits(a[0], c[0], "timed fused kernel: output")
    assert np.array_equal(a[1][0], c[1][0])
    _bits(a[1][1], c[1][1], "timed fused kernel: hit t")

"""GPU: the step schedule's refill (step_body, rt_kernels_body.hpp) at the smallest shapes where its
pop can go wrong.  On launches with the camera-ray ring the refill is a scalar loop that fills the
empty ring, followed by one straight-line predicated pop, repeated by a loop with a single exit; the
order in which ring slots go to lanes, the hand-out of tiles and the thresholds are what they were.
None of that may move a node visit, a triangle test, a shading round or an RNG draw, so every case
here is compared bit for bit (radiance, primary hit ids and t) and counter for counter (rays, node
visits, triangle tests, hits) against the CPU oracle in pinned math -- as one fused launch and as
per-frame launches, with and without the per-frame sky key, in the timed kernels and in their
counting variants -- and in shipped math the fused launch against the same frames issued as
per-frame launches.

The shapes (those tests/test_step_decision.py does not hold):
  16x8, 1 and 3 fused frames, a     tile 0 has no primary hit and tile 1 has some (asserted from the
  camera turned off the box         oracle's hit ids): a fill that leaves the ring empty must be followed
                                    by another fill before any pop.  With hit buffers bound (no view
                                    cull) and without (the fused launch culls tile 0)
  64x8, refill_min at the ends of   lowest: pops of one or two lanes walk the ring's head through a tile;
  its range                         highest: a pop takes a whole tile and drains the ring exactly
  40x24, 8 fused frames, hit        lightBounces 0: the pop's own DONE branch writes the last frame's hit
  buffers, lightBounces 0 and 9     ids; 9: the shading writes them
  24x8, the middle 100 work items   invalid lanes are compacted at the fill: the ring holds fewer than 64
                                    entries while more lanes are idle -- two pops in one refill round
  the 64x8 and 24x8 shapes again    every primary ray hits: a tile's ring fill holds all its valid lanes (64;
  from a camera inside the box      at most 34 in the work range), so the pops named above do happen
  256x64 and 250x64, 8 fused        the shapes above give every wave one tile at most.  Here a wave takes
  frames, camera inside the box,    several, so at the lowest refill_min a tile's ring is popped in pieces
  one workgroup per CU              (asserted: more pop iterations than ring fills), at the highest every pop
                                    drains its fill (asserted: as many), and in 250x64's last tile column a
                                    fill of 16 entries meets 64 idle lanes: two fills and pops in one round
                                    (asserted: more pops than fills, which only such a round can cause)
  64x64 bunny proxy, 2 and 8        the ringless refill with the HBM/L2 octant walk's template
  fused frames                      arguments, and with those of the plain global walk (global_oct 0)
"""
import numpy as np
import pytest

from clrt import _native as N
from hip_helpers import DEFAULT_CAMERA, HipRenderer, rgb
from tuning_table import KNOBS

pytestmark = pytest.mark.gpu
COUNTERS = ("rays", "node_visits", "tri_tests", "hits")
_RANGE = {name: (lo, hi) for name, _, lo, hi, _ in KNOBS}
# the default camera turned to the left: the box fills the right half of a 16x8 image, and no ray of
# the left 8x8 tile comes within two pixel columns of it (found with the CPU oracle)
OFF_BOX = ((0.0, -25.0, 8.5), (-0.65, 1.0, 0.0), (0.0, 0.0, 1.0))
# a camera inside the box: every primary ray hits, so no lane is decided as sky at the fill and a tile puts all
# its valid lanes into the ring (the default camera sees the box in a tenth of these small images' pixels, and
# most of their ring fills hold a few entries or none)
INSIDE = ((0.0, 0.0, 8.5), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
NEVER = -2  # the hit-id buffer's content before a launch: "never written"


class Case:
    def __init__(self, scene, W, H, frames, bounces=9, tuning=None, camera=DEFAULT_CAMERA, hits=True, work=None,
                 pops=None):
        self.scene, self.W, self.H, self.frames, self.bounces = scene, W, H, frames, bounces
        self.tuning, self.camera, self.hits = tuning or {}, camera, hits
        self.pops = pops  # what the fused counting run's pop iterations must be against its ring fills
        self.work = work or (0, W * H)  # work items [first, last)

    def ref_key(self):
        return (self.scene, self.W, self.H, self.frames, self.bounces, self.camera, self.work)


CASES = {
    "empty-fill-f1": Case("cornell", 16, 8, 1, camera=OFF_BOX),
    "empty-fill-f3": Case("cornell", 16, 8, 3, camera=OFF_BOX),
    "empty-fill-f1-cull": Case("cornell", 16, 8, 1, camera=OFF_BOX, hits=False),
    "empty-fill-f3-cull": Case("cornell", 16, 8, 3, camera=OFF_BOX, hits=False),
    "pop-small": Case("cornell", 64, 8, 2, tuning={"refill_min": _RANGE["refill_min"][0]}),
    "pop-tile": Case("cornell", 64, 8, 2, tuning={"refill_min": _RANGE["refill_min"][1]}),
    "pop-small-inside": Case("cornell", 64, 8, 2, tuning={"refill_min": _RANGE["refill_min"][0]}, camera=INSIDE),
    "pop-tile-inside": Case("cornell", 64, 8, 2, tuning={"refill_min": _RANGE["refill_min"][1]}, camera=INSIDE),
    # more tiles than waves (max_blocks 1: one workgroup per CU; 2048 (tile, frame) fills), every ray a hit
    "pop-small-waves": Case("cornell", 256, 64, 8, camera=INSIDE, pops="more",
                            tuning={"refill_min": _RANGE["refill_min"][0], "max_blocks": 1}),
    "pop-tile-waves": Case("cornell", 256, 64, 8, camera=INSIDE, pops="equal",
                           tuning={"refill_min": _RANGE["refill_min"][1], "max_blocks": 1}),
    "partial-tiles-waves": Case("cornell", 250, 64, 8, camera=INSIDE, pops="more",
                                tuning={"refill_min": _RANGE["refill_min"][1], "max_blocks": 1}),
    "done-at-pop": Case("cornell", 40, 24, 8, bounces=0),
    "done-at-shade": Case("cornell", 40, 24, 8, bounces=9),
    "range-middle": Case("cornell", 24, 8, 2, work=(46, 146)),
    "range-middle-inside": Case("cornell", 24, 8, 2, work=(46, 146), camera=INSIDE),
    "bunny-octant-f2": Case("bunny", 64, 64, 2),
    "bunny-octant-f8": Case("bunny", 64, 64, 8),
    "bunny-global-f2": Case("bunny", 64, 64, 2, tuning={"global_oct": 0}),
    "bunny-global-f8": Case("bunny", 64, 64, 8, tuning={"global_oct": 0}),
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
    """Frames 1..F of the case from the CPU oracle, computed once per distinct shape: (result, last
    frame's primary hit ids and t, the counters summed over the frames).  Outside the work range the
    result is 0 and the hit ids are NEVER."""
    c = CASES[case]
    if c.ref_key() not in _refs:
        res = np.zeros((c.W * c.H, 4), np.float32)
        counts = dict.fromkeys(COUNTERS, 0)
        ids = t = None
        for f in range(1, c.frames + 1):
            res, ids, t, n = oracle_mod.render(_scene(c.scene, cornell), c.W, c.H, frame_count=f,
                                               light_bounces=c.bounces, camera=c.camera, result=res,
                                               first=c.work[0], last=c.work[1], want_hits=True, threads=16)
            for key in COUNTERS:
                counts[key] += n[key]
        inside = np.zeros(c.W * c.H, bool)
        inside[c.work[0]:c.work[1]] = True
        ids = np.where(inside, ids, NEVER).astype(np.int32)
        t = np.where(inside, t, np.float32(0.0)).astype(np.float32)
        if c.camera is OFF_BOX:  # what the shape is for
            hit = (ids >= 0).reshape(c.H, c.W)
            assert not hit[:, :8].any() and hit[:, 8:].any()
        for a in (res, ids, t):
            a.setflags(write=False)
        _refs[c.ref_key()] = (res, ids, t, counts)
    return _refs[c.ref_key()]


def _render(case, cornell, math, fused, stats, sky=None):
    """(output, (hit ids, t) or None, counters or None) of the case's frames."""
    c = CASES[case]
    n = c.W * c.H
    r = HipRenderer(_scene(c.scene, cornell), c.W, c.H, math=math, hits=c.hits, stats=stats)
    r.ctx.WriteBuffer(r.out, np.zeros((n, 4), np.float32))
    if c.hits:
        r.ctx.WriteBuffer(r.hit_bufs[0], np.full(n, NEVER, np.int32))
        r.ctx.WriteBuffer(r.hit_bufs[1], np.zeros(n, np.float32))
    r.k.set_tuning("perframe_defer", 0)  # per-frame launches render into the output themselves
    if sky is not None:
        r.k.set_tuning("perframe_sky", sky)
    for name, value in c.tuning.items():
        r.k.set_tuning(name, value)
    kw = dict(light_bounces=c.bounces, camera=c.camera, work_range=c.work if c.work != (0, n) else None)
    if fused:
        r.frame(1, n_frames=c.frames, **kw)
    else:
        for f in range(1, c.frames + 1):
            r.frame(f, **kw)
    out = (r.result(), r.hits() if c.hits else None, r.k.stats() if stats else None, r.k.scene_in_lds())
    r.close()
    assert out[3] == (c.scene == "cornell")
    return out[:3]


def _bits(a, b, what):
    a = np.ascontiguousarray(a).view(np.uint32).ravel()
    b = np.ascontiguousarray(b).view(np.uint32).ravel()
    diff = np.flatnonzero(a != b)
    assert diff.size == 0, f"{what}: {diff.size} words differ, first at {diff[:8]}"


def _check_oracle(got, ref, what):
    res, ids, t, counts = ref
    _bits(rgb(got[0]), rgb(res), f"{what}: radiance")
    if got[1] is not None:
        assert np.array_equal(got[1][0], ids), f"{what}: {(got[1][0] != ids).sum()} primary hit ids differ"
        _bits(got[1][1], t, f"{what}: hit t")
    if got[2] is not None:
        for key in COUNTERS:
            assert got[2][key] == counts[key], f"{what}: {key} {got[2][key]} != {counts[key]}"


@pytest.mark.parametrize("case", list(CASES))
def test_fused_pinned_equals_oracle(cornell, oracle_mod, case):
    ref = _reference(case, cornell, oracle_mod)
    for stats in (False, True):
        got = _render(case, cornell, N.MATH_PINNED, True, stats)
        _check_oracle(got, ref, f"fused, stats {stats}")
    c = CASES[case]
    if c.pops:
        # Every (tile, frame) has valid lanes and every ray hits, so each is one ring fill with entries, and
        # each such fill is drained by one pop iteration or more.  refill_min 64: a refill round starts with
        # 64 idle lanes, so every pop takes its whole fill -- as many pops as fills.  refill_min 1 with more
        # tiles than waves: a wave refills while its other lanes still walk, so some fill is popped in pieces
        # -- were every fill drained by a single pop, the counts would be equal.  250x64 at refill_min 64:
        # a pop can leave entries in the ring only if it was not the first pop of its round (the first meets
        # 64 idle lanes), so more pops than fills means a round that filled and popped twice -- which a fill
        # from the last tile column (16 valid lanes) followed by another tile forces.
        fills = ((c.W + 7) // 8) * ((c.H + 7) // 8) * c.frames
        pops = got[2]["sched"]["refill_pops"]
        print(f"{case}: ring fills {fills}, pop iterations {pops}, refill rounds {got[2]['sched']['refill_rounds']}")
        assert pops > fills if c.pops == "more" else pops == fills, (pops, fills)


@pytest.mark.parametrize("case", list(CASES))
def test_per_frame_pinned_equals_oracle(cornell, oracle_mod, case):
    """Per-frame launches: paths end through the finish queue (sky key off) or, for primary misses
    whose stored value follows the key chain, through the sky key (perframe_sky 2: always)."""
    ref = _reference(case, cornell, oracle_mod)
    for sky in (0, 2):
        for stats in (False, True):
            _check_oracle(_render(case, cornell, N.MATH_PINNED, False, stats, sky), ref,
                          f"per-frame, sky key {sky}, stats {stats}")


def _same(a, b, what):
    _bits(a[0], b[0], f"{what}: output")
    if a[1] is not None:
        assert np.array_equal(a[1][0], b[1][0]), f"{what}: primary hit ids"
        _bits(a[1][1], b[1][1], f"{what}: hit t")
    if a[2] is not None and b[2] is not None:
        for key in COUNTERS:
            assert a[2][key] == b[2][key], f"{what}: {key}"


@pytest.mark.parametrize("case", list(CASES))
def test_fused_shipped_equals_per_frame(cornell, case):
    c = CASES[case]
    a = _render(case, cornell, N.MATH_SHIPPED, True, True)
    if c.hits:  # every pixel's primary hit in the work range was written (-1: a miss), no other
        assert (a[1][0][c.work[0]:c.work[1]] >= -1).all()
        assert (np.delete(a[1][0], np.s_[c.work[0]:c.work[1]]) == NEVER).all()
    for sky in (0, 2):
        _same(a, _render(case, cornell, N.MATH_SHIPPED, False, True, sky), f"sky key {sky}")
    # the timed kernels (no counters) against their counting variants
    _same(a, _render(case, cornell, N.MATH_SHIPPED, True, False), "timed fused kernel")

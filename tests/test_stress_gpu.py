"""GPU: the HIP kernels on the stress fixtures (stress_scenes.py) -- tilted GGX lobes in every
alpha regime, axis-aligned rays with +0 / -0 components, degenerate camera bases, a camera inside
a triangle soup (hits behind the origin), zero-area / duplicate / non-finite triangles, smooth,
zero and huge vertex normals, and hand-built trees (random axis flags, leaves of 1..127 and more,
a 59-deep chain of second children, garbage records past the tree's end).

test_stress_cpu.py shows, without a GPU, that the x86-64 build of the reference kernel equals the
oracle on every one of these inputs and that the inputs reach what they are meant to reach.  Here:
  A. pinned math == the oracle: radiance bits, primary ids, primary t bits, the four counters;
  B. every scene layout x schedule x launch shape on a subset: pinned == the oracle, shipped and
     devicelib == their own default path;
  C. shipped / devicelib == the reference kernel run live through OpenCL (skipped without it);
  D. the non-finite soup, on its own.
Nothing is compared under a tolerance.
"""
import numpy as np
import pytest

import stress_scenes as SS
from clrt import _native as N
from hip_helpers import HipRenderer, rgb
from ref_compare import bits_differ

pytestmark = pytest.mark.gpu

MODES = {"shipped": (N.MATH_SHIPPED, "shipped"), "devicelib": (N.MATH_DEVICELIB, "strict")}
# scene layouts: LDS; the octant records read from HBM/L2; the 64-B global node records with no
# and with a few (fewer than the tree has) top-of-tree nodes staged in LDS
LAYOUTS = {
    "lds": (False, {}),
    "global_oct": (True, {}),
    "global_top0": (True, {"global_oct": 0, "top_nodes": 0, "wf_top_nodes": 0}),
    "global_top5": (True, {"global_oct": 0, "top_nodes": 5, "wf_top_nodes": 5}),
}
SCHEDS = {"tiles": N.SCHED_TILES, "step": N.SCHED_STEP, "wavefront": N.SCHED_WAVEFRONT}


def _open_ref(variant):
    import clref
    ok, why = clref.available()
    if not ok:
        pytest.skip(why)
    try:
        return clref.ReferenceKernel(variant)
    except RuntimeError as e:
        pytest.skip(f"no OpenCL GPU device for the reference: {e}")


@pytest.fixture(scope="module")
def refs():
    opened = {}

    def get(variant):
        if variant not in opened:
            opened[variant] = _open_ref(variant)
        return opened[variant]

    yield get
    for r in opened.values():
        r.close()


@pytest.fixture(scope="module")
def sweeps(cornell):
    return SS.material_sweeps(cornell)


class _Pool:
    """Renderers kept open and reused: every run starts at frame 0 (which overwrites the output
    buffer), sets its schedule and resets the counters, so runs on one renderer are independent.
    Scenes that differ only in their materials share a renderer; the materials are written into
    the bound buffer before each run (the library re-packs them, test_gpu_state.py)."""

    def __init__(self):
        self.open = {}

    def get(self, key, scene, W, H, math, layout):
        k = (key, W, H, math, layout)
        if k not in self.open:
            force_global, tuning = LAYOUTS[layout]
            r = HipRenderer(scene, W, H, math=math, hits=True, stats=True, force_global=force_global)
            for name, value in tuning.items():
                r.k.set_tuning(name, value)
            self.open[k] = r
        return self.open[k]

    def close(self):
        for r in self.open.values():
            r.close()
        self.open = {}


@pytest.fixture(scope="module")
def cornell_pool():
    p = _Pool()
    yield p
    p.close()


@pytest.fixture
def pool():
    p = _Pool()
    yield p
    p.close()


def _hip(pool, key, scene, W, H, camera, light_type, bounces, frames, math=N.MATH_PINNED, layout="lds",
         sched=N.SCHED_STEP, fused=False):
    assert frames[0] == 0
    r = pool.get(key, scene, W, H, math, layout)
    r.ctx.WriteBuffer(r.bufs[2], scene.materials)
    r.k.set_schedule(sched)
    r.k.reset_stats()
    kw = dict(light_bounces=bounces, light_type=light_type, camera=camera)
    if fused:
        r.frame(frames[0], n_frames=len(frames), **kw)
    else:
        for f in frames:
            r.frame(f, **kw)
    out = rgb(r.result())
    ids, t = r.hits()
    st = r.k.stats()
    return out, ids, t, {k: st[k] for k in SS.COUNTERS}


def _assert_same(got, want, what):
    out, ids, t, st = got
    w_out, w_ids, w_t, w_st = want
    nd = bits_differ(out, rgb(w_out) if w_out.shape[1] == 4 else w_out)
    assert nd == 0, f"{what}: {nd} radiance words differ"
    assert np.array_equal(ids, w_ids), f"{what}: {(ids != w_ids).sum()} primary hit ids differ"
    assert bits_differ(t, w_t) == 0, f"{what}: primary t differs"
    if w_st is not None:
        assert st == w_st, f"{what}: counters {st} != {w_st}"


def _sweep_args(sweeps, name):
    R = SS.SWEEP_RUN
    return (sweeps[name], R["W"], R["H"], SS.DEFAULT, SS.sweep_light_type(list(sweeps).index(name)), R["bounces"],
            R["frames"])


def _camera_args(sweeps, cam):
    R = SS.SWEEP_RUN
    return (sweeps["mixed"], R["W"], R["H"], SS.CAMERAS[cam], 0, R["bounces"], R["frames"])


def _soup_args(case, cam, nonfinite=False):
    R = SS.SOUP_RUN
    return (SS.soup_scene(*case, nonfinite=nonfinite), R["W"], R["H"], SS.SOUP_CAMERAS[cam], 0, R["bounces"],
            R["frames"])


SWEEP_NAMES = [SS.sweep_name(v) for v in SS.SWEEP_VALUES] + ["mixed"]


# ---- A. pinned math against the oracle ----------------------------------------------------------
@pytest.mark.parametrize("name", SWEEP_NAMES)
def test_sweep_pinned_equals_oracle(oracle_mod, cornell_pool, sweeps, name):
    args = _sweep_args(sweeps, name)
    _assert_same(_hip(cornell_pool, "cornell", *args), SS.oracle_run(oracle_mod, ("sweep", name), *args), name)


@pytest.mark.parametrize("cam", list(SS.CAMERAS))
def test_cameras_pinned_equals_oracle(oracle_mod, cornell_pool, sweeps, cam):
    args = _camera_args(sweeps, cam)
    _assert_same(_hip(cornell_pool, "cornell", *args), SS.oracle_run(oracle_mod, ("camera", cam), *args), cam)


@pytest.mark.parametrize("case", SS.soup_cases(), ids=SS.case_id)
def test_soups_pinned_equals_oracle(oracle_mod, pool, case):
    """tri_accept's branch-free accept on zero-area triangles (det == 0, inv_det = inf, u = 0 * inf),
    duplicates and hits behind the origin; the octant walk on trees the builder would never make.
    The soup whose tree holds a leaf of more than 127 triangles renders from the global records."""
    for cam in SS.SOUP_CAMERAS:
        args = _soup_args(case, cam)
        _assert_same(_hip(pool, case, *args), SS.oracle_run(oracle_mod, ("soup", case, cam, False), *args),
                     f"{SS.case_id(case)} {cam}")


def test_big_leaf_soup_leaves_lds(oracle_mod):
    sc = SS.soup_scene(SS.SOUP_SEEDS[0], "big")
    r = HipRenderer(sc, 16, 16)
    r.frame(1, light_bounces=1)
    in_lds = r.k.scene_in_lds()
    r.close()
    assert not in_lds
    r = HipRenderer(SS.soup_scene(SS.SOUP_SEEDS[0], "rt127"), 16, 16)
    r.frame(1, light_bounces=1)
    in_lds = r.k.scene_in_lds()
    r.close()
    assert in_lds


# ---- B. every scene path and schedule --------------------------------------------------------------
def _path_scene(sweeps, which):
    """(oracle key, renderer key, run arguments), three frames from frame 0"""
    if which == "mixed":
        return ("sweep", "mixed"), "cornell", _sweep_args(sweeps, "mixed")
    case = SS.PATH_SOUPS[which]
    return ("soup", case, "inside", "f012"), case, _soup_args(case, "inside")[:6] + (SS.PATH_FRAMES,)


PATH_SCENES = ["mixed"] + list(SS.PATH_SOUPS)


@pytest.mark.parametrize("which", PATH_SCENES)
def test_paths_pinned_equal_oracle(oracle_mod, cornell_pool, pool, sweeps, which):
    okey, rkey, args = _path_scene(sweeps, which)
    want = SS.oracle_run(oracle_mod, okey, *args)
    p = cornell_pool if rkey == "cornell" else pool
    for layout in LAYOUTS:
        for sched in SCHEDS:
            for fused in (False, True):
                got = _hip(p, rkey, *args, layout=layout, sched=SCHEDS[sched], fused=fused)
                _assert_same(got, want, f"{which} {layout} {sched} {'fused' if fused else 'perframe'}")


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("which", PATH_SCENES)
def test_paths_equal_default_path(cornell_pool, pool, sweeps, which, mode):
    """Shipped and devicelib: every layout, schedule and launch shape leaves the bits of the default
    path (LDS, step schedule, per-frame launches) -- no reference runtime needed."""
    math = MODES[mode][0]
    _, rkey, args = _path_scene(sweeps, which)
    p = cornell_pool if rkey == "cornell" else pool
    want = _hip(p, rkey, *args, math=math)
    for layout in LAYOUTS:
        for sched in SCHEDS:
            for fused in (False, True):
                if (layout, sched, fused) == ("lds", "step", False):
                    continue
                got = _hip(p, rkey, *args, math=math, layout=layout, sched=SCHEDS[sched], fused=fused)
                _assert_same(got, want, f"{which} {layout} {sched} {'fused' if fused else 'perframe'}")


# ---- C. shipped and devicelib against the live reference kernel ----------------------------------
def _check_live(ref, pool, rkey, math, args, what, layouts=("lds", "global_oct")):
    scene, W, H, camera, lt, lb, frames = args
    want = ref.render(scene, W, H, frames=frames, light_bounces=lb, light_type=lt, camera=camera)[:, :3]
    ids_r, t_r = ref.primary_hits(scene, W, H, frame=frames[-1], camera=camera)
    for layout in layouts:
        _assert_same(_hip(pool, rkey, *args, math=math, layout=layout), (want, ids_r, t_r, None),
                     f"{what} {layout}")


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", SWEEP_NAMES)
def test_sweep_equals_live_reference(refs, cornell_pool, sweeps, name, mode):
    """The shipped build's fast pow / sincos / rcp / div at operands Cornell's own materials never
    produce: exponents in (0, 1), at +-2^23 and negative, a finite D, a tilted half vector."""
    math, variant = MODES[mode]
    _check_live(refs(variant), cornell_pool, "cornell", math, _sweep_args(sweeps, name), name)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("cam", list(SS.CAMERAS))
def test_cameras_equal_live_reference(refs, cornell_pool, sweeps, cam, mode):
    math, variant = MODES[mode]
    _check_live(refs(variant), cornell_pool, "cornell", math, _camera_args(sweeps, cam), cam)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("tree", ["sah4", "rt7"])
@pytest.mark.parametrize("seed", SS.SOUP_SEEDS)
def test_soups_equal_live_reference(refs, pool, seed, tree, mode):
    math, variant = MODES[mode]
    for cam in SS.SOUP_CAMERAS:
        _check_live(refs(variant), pool, (seed, tree), math, _soup_args((seed, tree), cam), f"s{seed}-{tree} {cam}")


# ---- D. non-finite vertices -------------------------------------------------------------------------
@pytest.mark.parametrize("tree", ["sah4", "rt7"])
def test_nonfinite_soup(oracle_mod, pool, tree):
    """Three vertices at 1e30 (products overflow), one NaN and one +inf coordinate.

    Why this cannot hang: a walk's length does not depend on float values.  In step_body a walking
    lane's word `cur` changes only through oct_step / oct_step_w / oct_step_g (and node_visit on the
    global node records), which return the record's hit_next when `t1 >= t0` and its miss_next
    otherwise -- a NaN compares false and takes miss_next like any miss.  Both successors are fixed
    per (node, octant) by build_skips / build_oct_nodes: the near child, the far child after the near
    one's subtree, or the parent's successor, i.e. a later position in that octant's depth-first
    order of a tree check_nodes has validated, or END.  The octant (r.sgn) is three bits whatever
    the direction holds.  A leaf step tests a count of triangles read from the leaf code, then
    continues at the leaf's miss_next; tri_accept only chooses whether to keep {t, prim}, and prim
    is always an index the leaf produced.  The bounce loop is bounded by lightBounces.  So every
    path ends after at most lightBounces walks of at most (nodes + triangles) steps each, and no
    address is formed from a float.  The final max(radiance, 0) clears NaN (OpenCL fmax), so the
    image is finite; the oracle and the x86-64 reference agree on it (test_stress_cpu.py)."""
    case = (SS.SOUP_SEEDS[0], tree)
    for cam in SS.SOUP_CAMERAS:
        args = _soup_args(case, cam, nonfinite=True)
        want = SS.oracle_run(oracle_mod, ("soup", case, cam, True), *args)
        assert np.isfinite(want[0]).all()
        for layout in ("lds", "global_oct", "global_top5"):
            _assert_same(_hip(pool, case, *args, layout=layout), want, f"nonfinite {tree} {cam} {layout}")
        for math, _ in MODES.values():
            a = _hip(pool, case, *args, math=math)
            b = _hip(pool, case, *args, math=math, layout="global_oct", sched=N.SCHED_WAVEFRONT, fused=True)
            _assert_same(b, a, f"nonfinite {tree} {cam} math {math}")
            assert np.isfinite(a[0]).all()

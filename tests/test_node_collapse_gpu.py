"""GPU: launches walk the collapsed link set of the octant records (csrc/rt_scene_pack.cpp,
collapse_oct_links) and compute what the plain set computes.

Scenes: Cornell (20 collapsed link words) and the hand-built tree of node_collapse_scenes.mixed_scene
(chains of four nodes with one box along first- and second-child links, a leaf with its parent's box, a
-0.0 / +0.0 pair).  Sizes: 64x64, and 250x64 so that a wave gets several tiles.  Nine bounces.

The reference for pinned math is the CPU oracle, bit for bit: radiance, primary ids and t.  The CPU oracle
has no shipped arithmetic; for shipped math the reference is the same launch with stats on, which walks the
plain records -- the records and kernels of every launch before the collapse -- and must agree bit for bit
(its counters are pinned to the oracle's by the stats tests here and in test_benched_path.py)."""
import numpy as np
import pytest

from clrt import _native as N
from clrt import scene as S
from hip_helpers import DEFAULT_CAMERA, HipRenderer, rgb

import node_collapse_scenes as NC
import refit_ref as R
import stress_scenes as SS

pytestmark = pytest.mark.gpu

FRAMES = tuple(range(8))
BOUNCES = 9
SIZES = {"64x64": (64, 64), "250x64": (250, 64)}
SCHEDS = {"step": N.SCHED_STEP, "tiles": N.SCHED_TILES, "wavefront": N.SCHED_WAVEFRONT}


def _scene(cornell, name):
    """-> (scene, camera, collapsed link words)"""
    if name == "cornell":
        return cornell, DEFAULT_CAMERA, 20
    sc = NC.mixed_scene()[0]
    want = NC.expected_links(sc.nodes, len(sc.nodes))
    return sc, SS.CAMERAS["inside"], sum(1 for a, b in want.values() if a != b)


def _render(scene, W, H, camera, math=N.MATH_PINNED, fused=True, stats=False, force_global=False, sched=N.SCHED_STEP):
    """FRAMES -> (radiance words, hit ids, hit t bits, rtKernelGetNodeCollapse, rt_stats, scene in LDS)"""
    r = HipRenderer(scene, W, H, math=math, hits=True, stats=stats, force_global=force_global, sched=sched)
    try:
        if fused:
            r.frame(FRAMES[0], light_bounces=BOUNCES, camera=camera, n_frames=len(FRAMES))
        else:
            r.k.set_tuning("perframe_defer", 0)
            for f in FRAMES:
                r.frame(f, light_bounces=BOUNCES, camera=camera)
        img = rgb(r.result()).view(np.uint32)
        ids, t = r.hits()
        return img, ids, t.view(np.uint32), r.k.node_collapse(), r.k.stats(), r.k.scene_in_lds()
    finally:
        r.close()


def _oracle(oracle_mod, name, scene, W, H, camera):
    res, ids, t, counts = SS.oracle_run(oracle_mod, ("node_collapse", name, W, H), scene, W, H, camera, 0, BOUNCES, FRAMES)
    return rgb(res).view(np.uint32), ids, t.view(np.uint32), counts


def _same(got, want, what):
    for a, b, part in zip(got[:3], want[:3], ("radiance words", "hit ids", "hit t")):
        assert np.array_equal(a, b), f"{(a != b).sum()} {part} differ from {what}"


@pytest.mark.parametrize("math", [N.MATH_PINNED, N.MATH_SHIPPED], ids=["pinned", "shipped"])
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "perframe"])
@pytest.mark.parametrize("size", list(SIZES))
@pytest.mark.parametrize("name", ["cornell", "mixed"])
def test_collapsed_launch_equals_reference(cornell, oracle_mod, name, size, fused, math):
    scene, cam, links = _scene(cornell, name)
    W, H = SIZES[size]
    got = _render(scene, W, H, cam, math=math, fused=fused)
    assert got[3] == {"collapsed_links": links, "scene_collapsible": True, "launch_collapsed": True}
    assert got[5] and links > 0
    if math == N.MATH_PINNED:
        _same(got, _oracle(oracle_mod, name, scene, W, H, cam), "the oracle")
    else:
        plain = _render(scene, W, H, cam, math=math, fused=fused, stats=True)
        assert not plain[3]["launch_collapsed"]
        _same(got, plain, "the launch over the plain records")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "perframe"])
@pytest.mark.parametrize("name", ["cornell", "mixed"])
def test_stats_launch_walks_the_plain_set(cornell, oracle_mod, name, fused):
    scene, cam, links = _scene(cornell, name)
    W, H = SIZES["64x64"]
    counted = _render(scene, W, H, cam, fused=fused, stats=True)
    plain = _render(scene, W, H, cam, fused=fused)
    want = _oracle(oracle_mod, name, scene, W, H, cam)
    _same(counted, plain, "the launch without stats")
    assert {k: counted[4][k] for k in SS.COUNTERS} == want[3]
    assert counted[3] == {"collapsed_links": links, "scene_collapsible": True, "launch_collapsed": False}
    assert plain[3]["launch_collapsed"]


@pytest.mark.parametrize("sched", ["tiles", "wavefront"])
def test_tile_and_wavefront_schedules(cornell, oracle_mod, sched):
    scene, cam, _ = _scene(cornell, "mixed")
    W, H = SIZES["64x64"]
    got = _render(scene, W, H, cam, fused=sched == "wavefront", sched=SCHEDS[sched])
    assert got[3]["launch_collapsed"] and got[5]
    _same(got, _oracle(oracle_mod, "mixed", scene, W, H, cam), "the oracle")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "perframe"])
@pytest.mark.parametrize("name", ["cornell", "mixed"])
def test_hbm_walk_of_the_regrouped_records(cornell, oracle_mod, name, fused):
    """rtKernelForceGlobalScene puts the step schedule on the octant walk over HBM/L2 (the regrouped records),
    as the existing tests do with Cornell."""
    scene, cam, links = _scene(cornell, name)
    W, H = SIZES["64x64"]
    got = _render(scene, W, H, cam, fused=fused, force_global=True)
    assert not got[5]
    assert got[3] == {"collapsed_links": links, "scene_collapsible": True, "launch_collapsed": True}
    _same(got, _oracle(oracle_mod, name, scene, W, H, cam), "the oracle")
    counted = _render(scene, W, H, cam, fused=fused, force_global=True, stats=True)
    assert not counted[3]["launch_collapsed"] and not counted[5]
    assert {k: counted[4][k] for k in SS.COUNTERS} == _oracle(oracle_mod, name, scene, W, H, cam)[3]


def test_global_node_records_are_not_collapsed(cornell, oracle_mod):
    """The 64-byte node layout chooses its near child at run time: no collapsed set is walked there."""
    scene, cam, _ = _scene(cornell, "mixed")
    W, H = SIZES["64x64"]
    r = HipRenderer(scene, W, H, hits=True, force_global=True)
    try:
        r.k.set_tuning("global_oct", 0)
        r.frame(FRAMES[0], light_bounces=BOUNCES, camera=cam, n_frames=len(FRAMES))
        ids, t = r.hits()
        got = rgb(r.result()).view(np.uint32), ids, t.view(np.uint32)
        info = r.k.node_collapse()
    finally:
        r.close()
    assert info["scene_collapsible"] and not info["launch_collapsed"]
    _same(got, _oracle(oracle_mod, "mixed", scene, W, H, cam), "the oracle")


def test_refit_withdraws_the_collapse_until_the_next_full_preparation(oracle_mod):
    """A device refit rewrites planes and no links.  In the hand-built tree nodes 1, 3 and 4 carry the root's
    box; after a triangle of the root's other child (leaf A) has moved outwards, the refit gives the root a
    larger box and node 1 its own smaller one.  The launches after it walk the plain records and equal the
    oracle on the read-back arrays; a full preparation brings the collapsed set back."""
    scene, at = NC.mixed_scene()
    cam = SS.CAMERAS["inside"]
    W, H = SIZES["64x64"]
    links = sum(1 for a, b in NC.expected_links(scene.nodes, len(scene.nodes)).values() if a != b)
    leaf_a = int(scene.nodes[at["A"]]["offset"])
    moved = R.positions(scene.triangles[leaf_a:leaf_a + 1]) + np.float32([20.0, 0.0, 0.0])
    r = HipRenderer(scene, W, H, hits=True)
    extra = []
    try:
        rw = N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR
        for b in r.bufs[:2]:
            b.release()
        r.bufs[0] = r.ctx.create_buffer(rw, scene.triangles.nbytes, scene.triangles)
        r.bufs[1] = r.ctx.create_buffer(rw, scene.nodes.nbytes, scene.nodes)
        r.k.set_buffer(N.BUFFER_SCENE, r.bufs[0])
        r.k.set_buffer(N.BUFFER_NODE, r.bufs[1])
        recs = R.tri_points(moved)
        extra.append(r.ctx.create_buffer(rw, recs.nbytes, recs))

        def frames():
            r.ctx.WriteBuffer(r.out, np.zeros((r.n, 4), np.float32))
            r.frame(FRAMES[0], light_bounces=BOUNCES, camera=cam, n_frames=len(FRAMES))
            ids, t = r.hits()
            return rgb(r.result()).view(np.uint32), ids, t.view(np.uint32), r.k.node_collapse()

        first = frames()
        assert first[3] == {"collapsed_links": links, "scene_collapsible": True, "launch_collapsed": True}
        _same(first, _oracle(oracle_mod, "mixed", scene, W, H, cam), "the oracle")

        r.ctx.UpdateVertices(r.bufs[0], leaf_a, 1, extra[0])
        r.ctx.RefitBVH(r.k)
        after = frames()
        assert not after[3]["scene_collapsible"] and not after[3]["launch_collapsed"]
        t_now, n_now = np.empty_like(scene.triangles), np.empty_like(scene.nodes)
        r.ctx.ReadBuffer(r.bufs[0], t_now, blocking=True)
        r.ctx.ReadBuffer(r.bufs[1], n_now, blocking=True)
        assert np.array_equal(R.positions(t_now[leaf_a:leaf_a + 1]), moved)
        # the child's box is now inside its parent's, no longer equal to it
        assert n_now["bmax"][at["n1"], 0] < n_now["bmax"][at["n0"], 0]
        assert n_now["bmax"][at["n0"], 0] > scene.nodes["bmax"][at["n0"], 0]
        now = S.Scene(t_now, n_now, scene.materials, scene.max_prims_in_node)
        _same(after, _oracle(oracle_mod, "mixed_moved", now, W, H, cam), "the oracle on the moved geometry")
        assert r.k.scene_prepares() == (1, 1)

        # a host write of both buffers: the next launch prepares in full, from the original arrays
        r.ctx.WriteBuffer(r.bufs[0], np.ascontiguousarray(scene.triangles), blocking=True)
        r.ctx.WriteBuffer(r.bufs[1], np.ascontiguousarray(scene.nodes), blocking=True)
        again = frames()
        assert again[3] == {"collapsed_links": links, "scene_collapsible": True, "launch_collapsed": True}
        assert r.k.scene_prepares() == (2, 1)
        _same(again, first, "the first launch")
    finally:
        for b in extra:
            b.release()
        r.close()


def _octant_rays(scene, per_octant=96, seed=5):
    """Rays in all eight octants: origins around the scene, every sign pattern of the direction."""
    rng = np.random.default_rng(seed)
    lo, hi = scene.nodes["bmin"][0, :3], scene.nodes["bmax"][0, :3]
    ext = hi - lo
    o, d = [], []
    for octant in range(8):
        sign = np.float32([-1.0 if (octant >> ax) & 1 else 1.0 for ax in range(3)])
        o.append(rng.uniform(lo - 0.25 * ext, hi + 0.25 * ext, (per_octant, 3)))
        d.append(np.abs(rng.standard_normal((per_octant, 3))) * sign + sign * 1e-3)
    rays = np.zeros(8 * per_octant, N.RAY_DTYPE)
    rays["origin"], rays["dir"] = np.float32(np.vstack(o)), np.float32(np.vstack(d))
    rays["tmin"], rays["tmax"] = -np.inf, 100000.0
    return rays


@pytest.fixture(scope="module")
def octant_reference(oracle_mod):
    from ray_query_ref import SceneWalker
    scene = NC.mixed_scene()[0]
    rays = _octant_rays(scene)
    w = SceneWalker(scene)
    ref = {"closest": w.walk_rays(rays), "any": w.walk_rays(rays, any_hit=True)}
    hit = ref["closest"][0] >= 0
    octant = (rays["dir"][:, 0] < 0) * 1 + (rays["dir"][:, 1] < 0) * 2 + (rays["dir"][:, 2] < 0) * 4
    assert sorted(set(octant.tolist())) == list(range(8))
    assert all(hit[octant == o].any() for o in range(8)), "every octant needs hits"
    return scene, rays, ref


@pytest.mark.parametrize("force_global", [False, True], ids=["lds", "hbm"])
def test_intersect_rays_in_every_octant(octant_reference, force_global):
    from test_ray_query import Rig, check_against
    scene, rays, ref = octant_reference
    for stats in (False, True):
        g = Rig(scene, force_global=force_global, stats=stats)
        try:
            for mode in ("closest", "any"):
                g.k.reset_stats()
                hits = g.query(rays, any_hit=mode == "any")
                assert g.k.scene_in_lds() == (not force_global)
                check_against(hits, ref[mode], rays, f"{mode} stats={stats}")
                info = g.k.node_collapse()
                assert info["scene_collapsible"] and info["launch_collapsed"] == (not stats)
                if stats:
                    st = g.k.stats()
                    assert (st["rays"], st["node_visits"], st["tri_tests"], st["hits"]) == \
                        (len(rays), ref[mode][2], ref[mode][3], int((ref[mode][0] >= 0).sum())), (mode, st)
        finally:
            g.close()

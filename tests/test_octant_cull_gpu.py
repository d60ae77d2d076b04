"""GPU: launches walk the pruned link set of the octant records (csrc/rt_scene_pack.cpp, prune_oct_links;
the certificate: csrc/rt_octant_cull.cpp) and compute what the plain set computes.

Cases (octant_cull_gpu_cases.py): Cornell at 128x72 from a camera inside the box, Cornell at 64x64 from the
bench camera, and the hand-built room of octant_cull_scenes.py (culled leaves as near and far children, two in a
row, a culled interior subtree) at 64x64.  Nine bounces, frames 0..7.

Pinned math is compared with the CPU oracle bit for bit: radiance, primary ids and t.  The oracle has no shipped
arithmetic; shipped math is compared, bit for bit, with the same launches of the library built with
RT_OCTANT_CULL=0 from the same sources (lib/librt_hip_nocull.so, rendered once in a process of its own) and
with the launch with stats on, which walks the plain records."""
import os
import subprocess
import sys

import numpy as np
import pytest

from clrt import _native as N
from clrt import scene as S
from hip_helpers import HipRenderer, rgb

import node_collapse_scenes as NC
import octant_cull_gpu_cases as GC
import octant_cull_scenes as OC
import refit_ref as R
import stress_scenes as SS

pytestmark = pytest.mark.gpu

SCHEDS = {"step": N.SCHED_STEP, "tiles": N.SCHED_TILES, "wavefront": N.SCHED_WAVEFRONT}
CORNELL_PRUNED = 25  # test_octant_cull.py counts them against the rule


def _room_pruned():
    sc, at, masks, rng = OC.room_scene()
    m = np.zeros(len(sc.triangles), np.uint8)   # leaf G is never wholly certified: its bits do not matter
    for name, mask in masks.items():
        m[rng[name][0]:rng[name][1]] = mask
    want = OC.expected_pruned(sc.nodes, len(sc.nodes), m)
    base = NC.expected_links(sc.nodes, len(sc.nodes))
    skip = OC.skip_table(sc.nodes, len(sc.nodes))
    return sum((w[0] != base[k][1]) + (w[1] != skip[k]) for k, w in want.items())


def _pruned(case):
    return CORNELL_PRUNED if GC.CASES[case][0] == "cornell" else _room_pruned()


def _info(case, walked=True, certified=True):
    return {"pruned_links": _pruned(case), "contracted_links": 0, "scene_certified": certified, "launch_pruned": walked}


def _oracle(oracle_mod, case):
    name, W, H, cam = GC.CASES[case]
    res, ids, t, counts = SS.oracle_run(oracle_mod, ("octant_cull", case), GC.scene(name), W, H, cam, 0, GC.BOUNCES, GC.FRAMES)
    return rgb(res).view(np.uint32), ids, t.view(np.uint32), counts


def _same(got, want, what):
    for a, b, part in zip(got[:3], want[:3], ("radiance words", "hit ids", "hit t")):
        assert np.array_equal(a, b), f"{(a != b).sum()} {part} differ from {what}"


@pytest.fixture(scope="module")
def nocull(tmp_path_factory):
    """The shipped renders of every case on the RT_OCTANT_CULL=0 build, in one child process."""
    lib = os.path.join(N.LIB_DIR, "librt_hip_nocull.so")
    assert os.path.exists(lib), "librt_hip_nocull.so is not built (run __graft_entry__.build())"
    out = tmp_path_factory.mktemp("nocull") / "ref.npz"
    env = dict(os.environ, RT_HIP_LIB=lib)
    p = subprocess.run([sys.executable, os.path.join(os.path.dirname(__file__), "octant_cull_nocull_render.py"), str(out)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    return np.load(out)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "perframe"])
@pytest.mark.parametrize("case", list(GC.CASES))
def test_pinned_equals_the_oracle(oracle_mod, case, fused):
    got = GC.render(case, fused=fused)
    assert got[3] == _info(case) and got[3]["pruned_links"] > 0 and got[6]
    assert got[4]["launch_collapsed"]        # the pruned set contains the collapse
    _same(got, _oracle(oracle_mod, case), "the oracle")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "perframe"])
@pytest.mark.parametrize("case", list(GC.CASES))
def test_shipped_equals_the_build_without_the_cull(nocull, case, fused):
    got = GC.render(case, math=N.MATH_SHIPPED, fused=fused)
    assert got[3] == _info(case)
    key = f"{case}-{'fused' if fused else 'perframe'}"
    _same(got, (nocull[key + "-img"], nocull[key + "-ids"], nocull[key + "-t"]), "the RT_OCTANT_CULL=0 build")
    plain = GC.render(case, math=N.MATH_SHIPPED, fused=fused, stats=True)
    assert not plain[3]["launch_pruned"]
    _same(got, plain, "the launch over the plain records")


@pytest.mark.parametrize("sched", ["tiles", "wavefront"])
@pytest.mark.parametrize("case", ["cornell-inside", "room"])
def test_tile_and_wavefront_schedules(oracle_mod, case, sched):
    got = GC.render(case, fused=sched == "wavefront", sched=SCHEDS[sched])
    assert got[3] == _info(case) and got[6]
    _same(got, _oracle(oracle_mod, case), "the oracle")


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "perframe"])
@pytest.mark.parametrize("case", ["cornell-inside", "room"])
def test_hbm_walk_of_the_regrouped_records(oracle_mod, case, fused):
    got = GC.render(case, fused=fused, force_global=True)
    assert not got[6] and got[3] == _info(case)
    _same(got, _oracle(oracle_mod, case), "the oracle")


@pytest.mark.parametrize("force_global", [False, True], ids=["lds", "hbm"])
@pytest.mark.parametrize("case", ["cornell-bench", "room"])
def test_stats_launches_count_the_reference_walk(oracle_mod, case, force_global):
    counted = GC.render(case, stats=True, force_global=force_global)
    want = _oracle(oracle_mod, case)
    _same(counted, want, "the oracle")
    assert {k: counted[5][k] for k in SS.COUNTERS} == want[3]
    assert counted[3] == _info(case, walked=False) and not counted[4]["launch_collapsed"]


def test_global_node_records_are_not_pruned(oracle_mod):
    got = GC.render("room", force_global=True, tune=(("global_oct", 0),))
    assert got[3]["scene_certified"] and not got[3]["launch_pruned"] and not got[6]
    _same(got, _oracle(oracle_mod, "room"), "the oracle")


# ---- ray queries and path tracing over caller rays ------------------------------------------------------

def _octant_rays(scene, per_octant=96, seed=5):
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
def query_reference(oracle_mod):
    from ray_query_ref import SceneWalker
    out = {}
    for name in ("cornell", "room"):
        scene = GC.scene(name)
        rays = _octant_rays(scene)
        w = SceneWalker(scene)
        ref = {"closest": w.walk_rays(rays), "any": w.walk_rays(rays, any_hit=True)}
        hit = ref["closest"][0] >= 0
        octant = (rays["dir"][:, 0] < 0) * 1 + (rays["dir"][:, 1] < 0) * 2 + (rays["dir"][:, 2] < 0) * 4
        assert all(hit[octant == o].any() for o in range(8)), "every octant needs hits"
        out[name] = (scene, rays, ref)
    return out


@pytest.mark.parametrize("force_global", [False, True], ids=["lds", "hbm"])
@pytest.mark.parametrize("name", ["cornell", "room"])
def test_intersect_rays_in_every_octant(query_reference, name, force_global):
    from test_ray_query import Rig, check_against
    scene, rays, ref = query_reference[name]
    for stats in (False, True):
        g = Rig(scene, force_global=force_global, stats=stats)
        try:
            for mode in ("closest", "any"):
                g.k.reset_stats()
                hits = g.query(rays, any_hit=mode == "any")
                assert g.k.scene_in_lds() == (not force_global)
                check_against(hits, ref[mode], rays, f"{mode} stats={stats}")
                info = g.k.octant_cull()
                assert info["scene_certified"] and info["launch_pruned"] == (not stats) and info["pruned_links"] > 0
                if stats:
                    st = g.k.stats()
                    assert (st["rays"], st["node_visits"], st["tri_tests"], st["hits"]) == \
                        (len(rays), ref[mode][2], ref[mode][3], int((ref[mode][0] >= 0).sum())), (mode, st)
        finally:
            g.close()


@pytest.fixture(scope="module")
def path_reference(oracle_mod):
    import path_ref
    scene = GC.scene("room")
    rays = _octant_rays(scene, per_octant=24)
    seeds = np.random.default_rng(8).integers(0, 2 ** 32, len(rays), dtype=np.uint32)
    (res,) = path_ref.trace_rays_pool([(scene, rays, seeds, (GC.BOUNCES,), 0, 1.0)], procs=1)
    assert (res[GC.BOUNCES]["prim"] >= 0).sum() > 50
    return scene, rays, seeds, res[GC.BOUNCES]


@pytest.mark.parametrize("force_global", [False, True], ids=["lds", "hbm"])
def test_trace_paths(path_reference, force_global):
    from test_trace_paths import TraceRig, check, result_bits
    scene, rays, seeds, ref = path_reference
    g = TraceRig(scene, force_global=force_global)
    try:
        g.lights(GC.BOUNCES, 0)
        res = g.trace(rays, seeds)
        check(res, ref, "pinned paths")
        assert g.k.octant_cull()["launch_pruned"]
        g.k.set_math_mode(N.MATH_SHIPPED)
        shipped = g.trace(rays, seeds)
        assert g.k.octant_cull()["launch_pruned"]
    finally:
        g.close()
    g = TraceRig(scene, math=N.MATH_SHIPPED, force_global=force_global, stats=True)
    try:
        g.lights(GC.BOUNCES, 0)
        plain = g.trace(rays, seeds)
        assert not g.k.octant_cull()["launch_pruned"]
    finally:
        g.close()
    assert np.array_equal(result_bits(shipped), result_bits(plain))


# ---- moving geometry ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("refit", [True, False], ids=["refit", "update-only"])
def test_moved_vertices_withdraw_the_pruned_set(oracle_mod, refit):
    """The floor of the room is turned over on the device (its vertices in the other winding: the same plane,
    the opposite face), so octants that culled it must now hit it.  After rtEnqueueUpdateVertices + rtRefitBVH
    the certificate is unknown and the plain records are walked; after the update alone the next launch prepares
    in full from the moved triangles and walks a pruned set made for them.  Either way the result equals the
    oracle on the read-back arrays; a host write of the original arrays brings the first set back."""
    scene, at, _, rng = OC.room_scene()
    name, W, H, cam = GC.CASES["room"]
    lo, hi = rng["F"]
    pos = R.positions(scene.triangles[lo:hi])
    moved = np.ascontiguousarray(pos[:, [0, 2, 1], :])       # v2 <-> v3
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
            r.frame(GC.FRAMES[0], light_bounces=GC.BOUNCES, camera=cam, n_frames=len(GC.FRAMES))
            ids, t = r.hits()
            return rgb(r.result()).view(np.uint32), ids, t.view(np.uint32), r.k.octant_cull()

        first = frames()
        assert first[3] == _info("room")
        _same(first, _oracle(oracle_mod, "room"), "the oracle")

        r.ctx.UpdateVertices(r.bufs[0], lo, hi - lo, extra[0])
        if refit:
            r.ctx.RefitBVH(r.k)
        after = frames()
        t_now, n_now = np.empty_like(scene.triangles), np.empty_like(scene.nodes)
        r.ctx.ReadBuffer(r.bufs[0], t_now, blocking=True)
        r.ctx.ReadBuffer(r.bufs[1], n_now, blocking=True)
        assert np.array_equal(R.positions(t_now[lo:hi]), moved)
        now = S.Scene(t_now, n_now, scene.materials, scene.max_prims_in_node)
        key = ("octant_cull", "room-moved")
        res, ids, t, _ = SS.oracle_run(oracle_mod, key, now, W, H, cam, 0, GC.BOUNCES, GC.FRAMES)
        _same(after, (rgb(res).view(np.uint32), ids, t.view(np.uint32)), "the oracle on the moved geometry")
        assert not np.array_equal(after[0], first[0])
        if refit:
            assert not after[3]["scene_certified"] and not after[3]["launch_pruned"]
            assert r.k.scene_prepares() == (1, 1)
        else:
            assert after[3]["scene_certified"] and after[3]["launch_pruned"]
            assert r.k.scene_prepares() == (2, 0)

        r.ctx.WriteBuffer(r.bufs[0], np.ascontiguousarray(scene.triangles), blocking=True)
        r.ctx.WriteBuffer(r.bufs[1], np.ascontiguousarray(scene.nodes), blocking=True)
        again = frames()
        assert again[3] == _info("room")
        _same(again, first, "the first launch")
    finally:
        for b in extra:
            b.release()
        r.close()

"""GPU: launches walk the gate-skipped link set of the octant records (csrc/rt_scene_pack.cpp,
gate_skip_oct_links) and compute what the plain set computes.

Cornell (LDS walk; 13 of its 19 interior nodes removed) and the bunny proxy (the HBM/L2 walk of the regrouped
records; about 10,000 removed) at 64x64, 2 fused frames, 4 bounces, in the three math modes, fused and per
frame: the image, the primary ids and t of a normal launch are the bits of the same launch with stats on,
which walks the plain records.  Ray queries, closest-hit and any-hit, over 4,096 rays -- random, axis-aligned
with +-0 components, origins on box planes and corners, inside and far outside, half with a short tmax -- agree
bit for bit between the two.  After rtRefitBVH a launch walks the plain set."""
import numpy as np
import pytest

from clrt import _native as N
from hip_helpers import DEFAULT_CAMERA, HipRenderer, rgb

pytestmark = pytest.mark.gpu

W = H = 64
FRAMES = (0, 1)
BOUNCES = 4
MATHS = {"pinned": N.MATH_PINNED, "devicelib": N.MATH_DEVICELIB, "shipped": N.MATH_SHIPPED}


@pytest.fixture(scope="module")
def scenes(cornell):
    import clrt.proxy as P
    return {"cornell": cornell, "bunny": P.bunny_proxy()}


def _render(scene, math, fused, stats):
    r = HipRenderer(scene, W, H, math=math, hits=True, stats=stats)
    try:
        if fused:
            r.frame(FRAMES[0], light_bounces=BOUNCES, camera=DEFAULT_CAMERA, n_frames=len(FRAMES))
        else:
            r.k.set_tuning("perframe_defer", 0)
            for f in FRAMES:
                r.frame(f, light_bounces=BOUNCES, camera=DEFAULT_CAMERA)
        img = rgb(r.result()).view(np.uint32)
        ids, t = r.hits()
        return img, ids, t.view(np.uint32), r.k.gate_skip(), r.k.node_collapse(), r.k.scene_in_lds()
    finally:
        r.close()


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "perframe"])
@pytest.mark.parametrize("math", list(MATHS))
@pytest.mark.parametrize("name", ["cornell", "bunny"])
def test_launch_equals_the_stats_launch_over_the_plain_links(scenes, name, math, fused):
    got = _render(scenes[name], MATHS[math], fused, stats=False)
    plain = _render(scenes[name], MATHS[math], fused, stats=True)
    assert got[3]["gate_links"] > got[4]["collapsed_links"] > 0
    assert got[3]["scene_nested"] and got[3]["launch_gate_skipped"] and got[4]["launch_collapsed"]
    assert plain[3]["scene_nested"] and not plain[3]["launch_gate_skipped"] and not plain[4]["launch_collapsed"]
    assert got[5] == (name == "cornell")
    assert (got[1] >= 0).sum() > 500
    for a, b, part in zip(got[:3], plain[:3], ("radiance words", "hit ids", "hit t")):
        assert a.tobytes() == b.tobytes(), f"{(a != b).sum()} {part} differ from the launch over the plain records"


def _rays(scene, n=4096, seed=21):
    rng = np.random.default_rng(seed)
    nodes = scene.nodes
    lo, hi = nodes["bmin"][0, :3], nodes["bmax"][0, :3]
    ext = hi - lo
    planes = np.concatenate([nodes["bmin"][:, :3], nodes["bmax"][:, :3]])
    planes = planes[np.isfinite(planes).all(axis=1) & (planes >= lo).all(axis=1) & (planes <= hi).all(axis=1)]
    k = n // 8
    o, d = [], []
    o.append(rng.uniform(lo, hi, (2 * k, 3))), d.append(rng.standard_normal((2 * k, 3)))          # inside
    a = rng.uniform(lo - 2 * ext, hi + 2 * ext, (k, 3))                                             # around
    o.append(a), d.append(rng.uniform(lo, hi, (k, 3)) - a)
    a = rng.uniform(lo, hi, (k, 3)) + rng.choice([-1.0, 1.0], (k, 3)) * 1000.0 * ext                # far outside
    o.append(a), d.append(rng.uniform(lo, hi, (k, 3)) - a)
    c = planes[rng.integers(0, len(planes), k)]                                                     # box corners
    o.append(c), d.append(rng.standard_normal((k, 3)))
    axes = np.zeros((3 * k, 3))
    axes[np.arange(3 * k), rng.integers(0, 3, 3 * k)] = rng.choice([-1.0, 1.0], 3 * k)
    axes = np.where(axes == 0.0, rng.choice([0.0, -0.0], (3 * k, 3)), axes)                         # +-0 components
    p = planes[rng.integers(0, len(planes), 3 * k)]
    mix = np.where(rng.random((3 * k, 3)) < 0.5, p, rng.uniform(lo - 0.5 * ext, hi + 0.5 * ext, (3 * k, 3)))
    o.append(mix), d.append(axes)
    rays = np.zeros(n, N.RAY_DTYPE)
    rays["origin"], rays["dir"] = np.float32(np.vstack(o)), np.float32(np.vstack(d))
    length = np.maximum(np.linalg.norm(rays["dir"][:, :3].astype(np.float64), axis=1), 1e-6)
    short = rng.uniform(0.05, 1.5, n) * float(np.linalg.norm(ext)) / length
    rays["tmin"], rays["tmax"] = -np.inf, np.where(rng.random(n) < 0.5, 100000.0, short)
    return rays


@pytest.mark.parametrize("math", ["pinned", "shipped"])
@pytest.mark.parametrize("name", ["cornell", "bunny"])
def test_ray_queries_agree_between_the_link_sets(scenes, name, math):
    from test_ray_query import Rig
    scene = scenes[name]
    rays = _rays(scene)
    assert len(rays) == 4096
    got = {}
    for stats in (False, True):
        g = Rig(scene, math=MATHS[math], stats=stats)
        try:
            for mode in ("closest", "any"):
                got[stats, mode] = g.query(rays, any_hit=mode == "any")
                info = g.k.gate_skip()
                assert info["scene_nested"] and info["launch_gate_skipped"] == (not stats)
        finally:
            g.close()
    for mode in ("closest", "any"):
        a, b = got[False, mode], got[True, mode]
        assert a.tobytes() == b.tobytes(), f"{name} {mode}: hit records differ between the link sets"
        hit = a["prim"] >= 0
        print(name, math, mode, "hits", int(hit.sum()), "of", len(rays))
        assert hit.sum() > 400


def test_refit_withdraws_the_gate_skip_until_the_next_full_preparation(cornell):
    r = HipRenderer(cornell, W, H, hits=True)
    try:
        rw = N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR
        for b in r.bufs[:2]:
            b.release()
        r.bufs[0] = r.ctx.create_buffer(rw, cornell.triangles.nbytes, cornell.triangles)
        r.bufs[1] = r.ctx.create_buffer(rw, cornell.nodes.nbytes, cornell.nodes)
        r.k.set_buffer(N.BUFFER_SCENE, r.bufs[0])
        r.k.set_buffer(N.BUFFER_NODE, r.bufs[1])

        def frames():
            r.ctx.WriteBuffer(r.out, np.zeros((r.n, 4), np.float32))
            r.frame(FRAMES[0], light_bounces=BOUNCES, n_frames=len(FRAMES))
            return rgb(r.result()).view(np.uint32), r.k.gate_skip(), r.k.node_collapse()

        first = frames()
        assert first[1]["scene_nested"] and first[1]["launch_gate_skipped"] and first[1]["gate_links"] > 20
        r.ctx.RefitBVH(r.k)
        after = frames()
        assert not after[1]["scene_nested"] and not after[1]["launch_gate_skipped"]
        assert not after[2]["scene_collapsible"] and not after[2]["launch_collapsed"]
        assert r.k.scene_prepares() == (1, 1)
        # a host write of both buffers: the next launch prepares in full, and the set is back
        r.ctx.WriteBuffer(r.bufs[0], np.ascontiguousarray(cornell.triangles), blocking=True)
        r.ctx.WriteBuffer(r.bufs[1], np.ascontiguousarray(cornell.nodes), blocking=True)
        again = frames()
        assert again[1] == first[1] and r.k.scene_prepares() == (2, 1)
        assert np.array_equal(again[0], first[0])
    finally:
        r.close()

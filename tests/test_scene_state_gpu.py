"""GPU: the packed device scene's state across rebinding, rejected trees and repacks.

A kernel's packed scene is derived from its bound buffers and remembered with their handles and
generations.  Each case drives one kernel through a sequence that makes that memory stale in another
way -- other buffers bound, a buffer rewritten with a tree the validation refuses, a tuning that
renumbers the global records -- and compares every render and query bit for bit with a fresh kernel on a
fresh context that was given only the final scene.  64 x 36 frames, 2 bounces, pinned math.
"""
import numpy as np
import pytest

import refit_ref as R
import stress_scenes as SS
from clrt import _native as N
from clrt import scene as S
from hip_helpers import HipRenderer

pytestmark = pytest.mark.gpu

W, H, BOUNCES = 64, 36, 2
N_RAYS = 256
INVALID_MEM_OBJECT, INVALID_OPERATION = -38, -59


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def query_rays(scene):
    rng = np.random.default_rng(5)
    p = R.positions(scene.triangles).reshape(-1, 3)
    rays = np.zeros(N_RAYS, N.RAY_DTYPE)
    rays["origin"] = rng.uniform(p.min(axis=0), p.max(axis=0), (N_RAYS, 3)).astype(np.float32)
    rays["dir"] = rng.standard_normal((N_RAYS, 3)).astype(np.float32)
    rays["tmin"], rays["tmax"] = -np.inf, 100000.0
    return rays


class Rig(HipRenderer):
    """HipRenderer whose scene buffers are read-write and can be rebound (bind) or rewritten."""

    def __init__(self, scene, **kw):
        super().__init__(scene, W, H, **kw)
        self.extra = []
        self.bound = {}
        self.bind(scene)

    def bind(self, scene):
        """`scene` from buffers of its own, created at its first binding and kept (binding it again
        binds the same handles, with their generations as they are)."""
        if id(scene) not in self.bound:
            rw = N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR
            self.bound[id(scene)] = [self.ctx.create_buffer(rw, a.nbytes, a)
                                     for a in (scene.triangles, scene.nodes, scene.materials)]
            self.extra += self.bound[id(scene)]
        self.tris, self.nodes, self.mats = self.bound[id(scene)]
        for slot, b in zip((N.BUFFER_SCENE, N.BUFFER_NODE, N.BUFFER_MATERIAL), (self.tris, self.nodes, self.mats)):
            self.k.set_buffer(slot, b)

    def render(self):
        """Frames 1-2 into a cleared output."""
        self.ctx.WriteBuffer(self.out, np.zeros((self.n, 4), np.float32))
        for f in (1, 2):
            self.frame(f, light_bounces=BOUNCES)
        return self.result()

    def query_status(self, rays):
        """(status of rtEnqueueIntersectRays, the hit buffer read back): the buffer starts as 0xff bytes."""
        rb = self.ctx.create_buffer(N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR, rays.nbytes, rays)
        fill = np.full(len(rays) * 16, 0xFF, np.uint8)
        hb = self.ctx.create_buffer(N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR, fill.nbytes, fill)
        self.extra += [rb, hb]
        rc = self.ctx._lib.rtEnqueueIntersectRays(self.ctx.handle, self.k.handle, rb.handle, 0, len(rays),
                                                  N.QUERY_CLOSEST, hb.handle)
        hits = np.empty(len(rays), N.RAY_HIT_DTYPE)
        self.ctx.ReadBuffer(hb, hits, blocking=True)
        return rc, hits

    def query(self, rays):
        rc, hits = self.query_status(rays)
        assert rc == 0
        return hits

    def launches(self):
        return self.k.stats()["launches"]

    def close(self):
        self.ctx.Finish()
        for b in self.extra:
            b.release()
        super().close()


@pytest.fixture
def rigs():
    made = []

    def make(*a, **kw):
        made.append(Rig(*a, **kw))
        return made[-1]

    yield make
    for r in made:
        r.close()


_fresh = {}


def fresh(scene, force_global, global_oct=None, rays=None):
    """(image, hits or None) of a fresh kernel on a fresh context given `scene`; computed once per
    scene and setting and shared, read-only."""
    key = (scene.triangles.tobytes(), scene.nodes.tobytes(), force_global, global_oct, rays is not None)
    if key not in _fresh:
        r = Rig(scene, force_global=force_global)
        try:
            if global_oct is not None:
                r.k.set_tuning("global_oct", global_oct)
            img = r.render()
            hits = r.query(rays) if rays is not None else None
            assert r.k.scene_prepares() == (1, 0)
        finally:
            r.close()
        for a in (img, hits):
            if a is not None:
                a.setflags(write=False)
        _fresh[key] = (img, hits)
    return _fresh[key]


def same_hits(a, b):
    return a.tobytes() == b.tobytes()


# ---- (a) rebinding chain -------------------------------------------------------------------------
@pytest.mark.parametrize("force_global", [False, True], ids=["lds", "force_global"])
def test_rebinding_chain(cornell, rigs, force_global):
    big = SS.soup_scene(12, "big")  # a 140-triangle leaf: no octant records, the global records
    rays = query_rays(cornell)
    r = rigs(cornell, force_global=force_global)
    for step, scene in enumerate((cornell, big, cornell)):
        r.bind(scene)
        img = r.render()
        assert r.k.scene_prepares() == (step + 1, 0)
        if scene is cornell:
            want, want_hits = fresh(cornell, force_global, rays=rays)
            assert r.k.scene_in_lds() == (not force_global)
            assert same_hits(r.query(rays), want_hits), step
        else:
            want, _ = fresh(big, force_global)
            assert not r.k.scene_in_lds()
            before = r.launches()
            rc, hits = r.query_status(rays)
            assert rc == INVALID_OPERATION
            assert hits.tobytes() == b"\xff" * hits.nbytes and r.launches() == before
        assert np.array_equal(bits(img), bits(want)), step
        assert r.k.scene_prepares() == (step + 1, 0)


# ---- (b) a malformed tree, and recovery ----------------------------------------------------------
def test_malformed_tree_is_refused_then_recovers(cornell, rigs):
    rays = query_rays(cornell)
    r = rigs(cornell)
    lib, ctx, k = r.ctx._lib, r.ctx.handle, r.k.handle
    first = r.render()
    want, want_hits = fresh(cornell, False, rays=rays)
    assert np.array_equal(bits(first), bits(want))
    assert r.k.scene_prepares() == (1, 0)
    broken = cornell.nodes.copy()
    broken["offset"][0] = 0                 # second child <= parent
    r.ctx.WriteBuffer(r.nodes, broken)
    launches = r.launches()
    with pytest.raises(N.RTError) as err:
        r.frame(3, light_bounces=BOUNCES)
    assert err.value.code == INVALID_MEM_OBJECT
    rc, hits = r.query_status(rays)
    assert rc == INVALID_MEM_OBJECT and hits.tobytes() == b"\xff" * hits.nbytes
    assert lib.rtRefitBVH(ctx, k) == INVALID_MEM_OBJECT
    # nothing was launched: no launch counted, the image and both scene arrays as they were
    assert r.launches() == launches
    assert np.array_equal(bits(r.result()), bits(first))
    t, n = np.empty_like(cornell.triangles), np.empty_like(broken)
    r.ctx.ReadBuffer(r.tris, t, blocking=True)
    r.ctx.ReadBuffer(r.nodes, n, blocking=True)
    assert t.tobytes() == cornell.triangles.tobytes() and n.tobytes() == broken.tobytes()
    assert r.k.scene_prepares() == (1, 0)
    # the good tree back: the first render again, after exactly one more full preparation
    r.ctx.WriteBuffer(r.nodes, cornell.nodes)
    again = r.render()
    assert np.array_equal(bits(again), bits(first))
    assert r.k.scene_prepares() == (2, 0)
    assert same_hits(r.query(rays), want_hits)
    assert r.k.scene_prepares() == (2, 0)


# ---- (c) a changed top-node count repacks --------------------------------------------------------
@pytest.mark.parametrize("global_oct", [0, 1], ids=["global_records", "global_octants"])
def test_top_nodes_repack_then_refit(cornell, rigs, global_oct):
    r = rigs(cornell, force_global=True)
    r.k.set_tuning("global_oct", global_oct)
    want, _ = fresh(cornell, True, global_oct)
    before = r.render()
    assert np.array_equal(bits(before), bits(want))
    assert r.k.scene_prepares() == (1, 0)
    r.k.set_tuning("top_nodes", 16)
    assert r.k.scene_prepares() == (1, 0)   # the repack waits for the next launch
    after = r.render()
    assert not r.k.scene_in_lds()
    assert np.array_equal(bits(after), bits(before))
    assert r.k.scene_prepares() == (2, 0)

    def move(seed):
        recs = R.tri_points(R.positions(R.displaced(cornell.triangles, seed)))
        pb = r.ctx.create_buffer(N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR, recs.nbytes, recs)
        r.extra.append(pb)
        r.ctx.UpdateVertices(r.tris, 0, len(recs), pb)
        r.ctx.RefitBVH(r.k)

    def final_scene():
        t, n = np.empty_like(cornell.triangles), np.empty_like(cornell.nodes)
        r.ctx.ReadBuffer(r.tris, t, blocking=True)
        r.ctx.ReadBuffer(r.nodes, n, blocking=True)
        return S.Scene(t, n, cornell.materials, cornell.max_prims_in_node)

    move(7)                                 # the repacked scene is current: the device path
    assert r.k.scene_prepares() == (2, 1)
    moved = r.render()
    assert r.k.scene_prepares() == (2, 1)
    assert not np.array_equal(bits(moved), bits(before))
    assert np.array_equal(bits(moved), bits(fresh(final_scene(), True, global_oct)[0]))
    # a change with no launch before the refit: the refit itself prepares in full first
    r.k.set_tuning("top_nodes", 384)
    move(8)
    assert r.k.scene_prepares() == (3, 2)
    moved = r.render()
    assert r.k.scene_prepares() == (3, 2)
    assert np.array_equal(bits(moved), bits(fresh(final_scene(), True, global_oct)[0]))

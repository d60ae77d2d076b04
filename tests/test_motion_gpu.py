"""GPU: motion records (rtEnqueueExtractVertices, rtEnqueueHitMotion, rtEnqueueFrameMotion), the motion variants of the
two reprojections, and Raytracer.move_vertices(keep_previous=True) / temporal(motion=True) on the Cornell fixture.

The reference is tests/motion_ref.py, the numpy float32 restatement of the definitions (checked on the CPU in
test_motion_plan.py, where a stand-alone program compiled from the kernels' own math texts gives its bytes).
rtEnqueueFrameMotion is compared with the composition of public calls it fuses -- the numpy centre rays uploaded,
rtEnqueueIntersectRays (closest), rtEnqueueHitMotion -- byte for byte in every math mode, and in pinned math with the
oracle's walk.  Sizes (w x h): 1 x 1, a single lane; 5 x 3, a partial 64-ray unit; 61 x 7, fewer units than waves;
131 x 77, partial 64 x 4 tiles.  Records that hold a NaN an operation produced are compared with
motion_ref.same_motion (IEEE leaves its sign and payload open); everything else byte for byte.
"""
import ctypes

import numpy as np
import pytest

import motion_inputs as I
import motion_ref as ref
import reproject_samples_inputs as RI
import reproject_samples_ref
import temporal_ref
import test_temporal_gpu as T
from clrt import _native as N
from hip_helpers import DEFAULT_CAMERA
from test_motion_plan import prev_records
from test_reproject_samples_plan import same_records

pytestmark = pytest.mark.gpu

F = np.float32
MODES = {"pinned": N.MATH_PINNED, "devicelib": N.MATH_DEVICELIB, "shipped": N.MATH_SHIPPED}


class Rig(T.Device):
    """A context and a kernel with the Cornell fixture bound (triangles and nodes writable), every slot set."""

    def __init__(self, w=61, h=7, camera=DEFAULT_CAMERA):
        super().__init__()
        s = I.scene()
        self.tris, self.nodes, self.mats = (self.buffer(a.nbytes, a) for a in (s.triangles, s.nodes, s.materials))
        self.out = self.buffer(max(w * h, 1) * 16)
        k = self.k
        for slot, b in ((N.BUFFER_OUT, self.out), (N.BUFFER_SCENE, self.tris), (N.BUFFER_NODE, self.nodes),
                        (N.BUFFER_MATERIAL, self.mats)):
            k.set_buffer(slot, b)
        k.set_uint(N.FRAME_COUNT, 1)
        k.set_uint(N.FRAME_SEED, 12345)
        k.set_int(N.LIGHT_BOUNCES, 2)
        k.set_int(N.LIGHT_TYPE, 0)
        k.set_float(N.SKYBOX_INTENSITY, 1.0)
        k.set_math_mode(N.MATH_PINNED)        # (the tests that change the mode put this one back)
        self.view(w, h, camera)

    def view(self, w, h, camera=DEFAULT_CAMERA):
        self.w, self.h, self.camera = w, h, camera
        self.k.set_int(N.WIDTH, w)
        self.k.set_int(N.HEIGHT, h)
        for slot, v in zip((N.CAMERA_POS, N.CAMERA_FRONT, N.CAMERA_UP), camera):
            self.k.set_float3(slot, v)

    def prev(self, first_tri, n_tris, normals=True):
        """Buffers of prev_records(first_tri, n_tris) (None for an empty range) and the records themselves."""
        pp, pn = prev_records(first_tri, n_tris)
        if n_tris == 0:
            return None, None, None, None
        return self.buffer(pp.nbytes, pp), self.buffer(pn.nbytes, pn) if normals else None, pp, pn if normals else None

    def composed(self, n, pb, nb, first_tri, n_tris):
        """The public calls FrameMotion fuses, for pixels 0 .. n - 1: (records, hits, rays)."""
        rays = ref.centre_rays(self.w, self.h, self.camera, n)
        rb, hb, mb = self.buffer(rays.nbytes, rays), self.buffer(n * 16), self.buffer(n * 32)
        self.ctx.IntersectRays(self.k, rb, hb, n)
        self.ctx.HitMotion(self.k, hb, 0, n, mb, pb, nb, first_tri, n_tris)
        return self.read(mb, n, ref.MOTION), self.read(hb, n, N.RAY_HIT_DTYPE), rays


@pytest.fixture(scope="module")
def rig():
    r = Rig()
    yield r
    r.close()


@pytest.fixture(scope="module")
def dev():
    d = T.Device()
    yield d
    d.close()


# ---- rtEnqueueExtractVertices ---------------------------------------------------------------------------
@pytest.mark.parametrize("first,n,normals", [(0, 72, True), (3, 7, False), (8, 60, True), (71, 1, True)])
def test_extract_vertices_equals_the_numpy_slice(rig, first, n, normals):
    tris = I.scene().triangles
    tail = 3
    fill = np.full((n + tail) * 48, I.NAN_BYTE, np.uint8)
    pb, nb = rig.buffer(fill.nbytes, fill), rig.buffer(fill.nbytes, fill) if normals else None
    rig.ctx.ExtractVertices(rig.tris, first, n, pb, nb)
    for b, field in ((pb, "position"), (nb, "normal")):
        if b is None:
            continue
        got = rig.read(b, n + tail, N.TRI_POINTS_DTYPE)
        assert got[:n].tobytes() == ref.tri_points(ref.vertices(tris, field)[first:first + n]).tobytes(), field
        assert (got[n:].view(np.uint8) == I.NAN_BYTE).all()                    # records past n_tris stay
    # extract, then update with the same data: the triangle array keeps its bytes
    rig.ctx.UpdateVertices(rig.tris, first, n, pb, nb)
    assert rig.read(rig.tris, len(tris), N.TRIANGLE_DTYPE).tobytes() == tris.tobytes()


# ---- rtEnqueueHitMotion -----------------------------------------------------------------------------------
@pytest.mark.parametrize("first_tri,n_tris,normals", [(0, 0, False), (3, 7, False), (3, 7, True), (0, 72, True)])
@pytest.mark.parametrize("n", [1, 5, 257])
def test_hit_motion_equals_the_restatement(rig, n, first_tri, n_tris, normals):
    first, pad = 5, 3
    hits = np.zeros(first + n + pad, N.RAY_HIT_DTYPE)
    hits[first:first + n] = I.seeded_hits(n)
    hits["prim"][:first], hits["prim"][first + n:] = 1, 2                      # (valid hits outside the range)
    pb, nb, pp, pn = rig.prev(first_tri, n_tris, normals)
    hb = rig.buffer(hits.nbytes, hits)
    mb = rig.buffer(hits.size * 32, np.full(hits.size * 32, I.NAN_BYTE, np.uint8))
    rig.ctx.HitMotion(rig.k, hb, first, n, mb, pb, nb, first_tri, n_tris)
    got = rig.read(mb, hits.size, ref.MOTION)
    want = ref.hit_motion(hits[first:first + n], I.scene().triangles, pp, pn, first_tri, n_tris)
    ref.same_motion(got[first:first + n], want, f"n {n}, moved [{first_tri}, +{n_tris}), normals {normals}")
    outside = np.concatenate([got[:first], got[first + n:]])
    assert (outside.view(np.uint8) == I.NAN_BYTE).all()                        # slots outside the range stay
    assert rig.read(hb, hits.size, N.RAY_HIT_DTYPE).tobytes() == hits.tobytes()
    if n == 257:
        assert (want["prim"] < 0).any() and np.isnan(want["prev_point"]).any()
        assert (want["flags"] == 1).any() == (n_tris > 0)


# ---- rtEnqueueFrameMotion -----------------------------------------------------------------------------------
def frame_motion(rig, n, pb, nb, first_tri, n_tris, tail=4):
    mb = rig.buffer((n + tail) * 32, np.full((n + tail) * 32, I.NAN_BYTE, np.uint8))
    rig.ctx.FrameMotion(rig.k, n, mb, pb, nb, first_tri, n_tris)
    got = rig.read(mb, n + tail, ref.MOTION)
    assert (got[n:].view(np.uint8) == I.NAN_BYTE).all()                        # the tail past the image stays
    return got[:n]


@pytest.mark.parametrize("mode", sorted(MODES))
def test_frame_motion_equals_the_composed_calls(rig, mode):
    rig.k.set_math_mode(MODES[mode])
    pb, nb, pp, pn = rig.prev(*I.BOX_RANGE)
    try:
        for force_global in (False, True):
            rig.k.force_global_scene(force_global)
            for w, h in T.SIZES:
                for camera in (DEFAULT_CAMERA, T.PAIRS["yaw"]) if (w, h) == (131, 77) else (DEFAULT_CAMERA,):
                    rig.view(w, h, camera)
                    want, hits, _ = rig.composed(w * h, pb, nb, *I.BOX_RANGE)
                    got = frame_motion(rig, w * h, pb, nb, *I.BOX_RANGE)
                    assert rig.k.scene_in_lds() == (not force_global)
                    assert got.tobytes() == want.tobytes(), (mode, force_global, w, h)
                    if (w, h) == (131, 77):
                        assert (got["prim"] < 0).any() and (got["flags"] == 1).any()
                        assert ((got["flags"] == 0) & (got["prim"] >= 0)).any()
        # nothing moved, no buffers: the current points
        rig.view(61, 7)
        want, _, _ = rig.composed(61 * 7, None, None, 0, 0)
        assert frame_motion(rig, 61 * 7, None, None, 0, 0).tobytes() == want.tobytes()
        # a work size that is not the image's
        want, _, _ = rig.composed(100, pb, nb, *I.BOX_RANGE)
        assert frame_motion(rig, 100, pb, nb, *I.BOX_RANGE).tobytes() == want.tobytes()
    finally:
        rig.k.force_global_scene(False)
        rig.k.set_math_mode(N.MATH_PINNED)
        rig.view(61, 7)


def test_frame_motion_equals_the_oracle_walk_in_pinned_math(rig, oracle_mod):
    """The oracle's walk of the numpy centre rays gives the prim; the barycentrics are the query's, whose prim was
    checked against the oracle's; the restatement makes the record."""
    from ray_query_ref import SceneWalker
    walker = SceneWalker(I.scene())
    pb, nb, pp, pn = rig.prev(*I.BOX_RANGE)
    rig.k.set_math_mode(N.MATH_PINNED)
    try:
        for w, h in T.SIZES:
            rig.view(w, h)
            got = frame_motion(rig, w * h, pb, nb, *I.BOX_RANGE)
            _, hits, rays = rig.composed(w * h, pb, nb, *I.BOX_RANGE)
            pick = np.arange(0, w * h, 7 if w * h > 1000 else 1)
            prim, t, _, _ = walker.walk_rays(rays[pick])
            assert np.array_equal(prim, hits["prim"][pick]) and t.tobytes() == hits["t"][pick].tobytes()
            walked = hits[pick].copy()
            walked["prim"], walked["t"] = prim, t
            want = ref.hit_motion(walked, I.scene().triangles, pp, pn, *I.BOX_RANGE)
            assert got[pick].tobytes() == want.tobytes(), (w, h)
    finally:
        rig.view(61, 7)


def test_frame_motion_counts_what_the_query_counts(rig):
    rig.view(131, 77)
    n = 131 * 77
    keys = ("rays", "node_visits", "tri_tests", "hits")
    rig.k.set_stats(True)
    try:
        counts = []
        for fused in (False, True):
            rig.k.reset_stats()
            if fused:
                frame_motion(rig, n, None, None, 0, 0)
            else:
                rays = ref.centre_rays(131, 77, DEFAULT_CAMERA)
                rb, hb = rig.buffer(rays.nbytes, rays), rig.buffer(n * 16)
                rig.ctx.IntersectRays(rig.k, rb, hb, n)
                rig.ctx.Finish()
            s = rig.k.stats()
            counts.append([s[key] for key in keys])
        assert counts[0] == counts[1] and counts[0][0] == n and 0 < counts[0][3] < n, counts
    finally:
        rig.k.set_stats(False)
        rig.view(61, 7)


def test_frame_motion_sees_moved_geometry_without_a_full_preparation(cornell):
    """Raytracer.move_vertices(keep_previous=True), then motion(): the records are the restatement's on the moved
    scene with the kept vertices, the short box's pixels point back by the shift, nothing was prepared in full."""
    import clrt
    W, H = 61, 7
    rt = clrt.Raytracer(W, H)
    rt.Init()
    try:
        rt.upload_scene(cornell)
        tris = I.scene().triangles
        before = rt.motion()
        assert (before["flags"] == 0).all() and (before["prim"] >= 0).any()
        full, refits = rt.kernel.scene_prepares()
        pos, _ = I.moved_scene()
        first, n = I.BOX_RANGE
        rt.move_vertices(pos[first:first + n], first=first, keep_previous=True)
        got = rt.motion()
        assert rt.kernel.scene_prepares() == (full, refits + 1)
        # the composition on the device's own (moved) scene, and the restatement on the host's copy of it
        moved = tris.copy()
        for i, v in enumerate(("v1", "v2", "v3")):
            moved[v]["position"][:, :3] = pos[:, i]
        rays = ref.centre_rays(W, H, (rt.camera.position, rt.camera.front, rt.camera.up))
        hits = rt.cast(rays["origin"], rays["dir"])
        keep_p, keep_n = ref.tri_points(ref.vertices(tris, "position")), ref.tri_points(ref.vertices(tris, "normal"))
        want = ref.hit_motion(hits, moved, keep_p, keep_n, 0, len(tris))
        assert got.reshape(-1).tobytes() == want.tobytes()
        assert rt.kernel.scene_prepares() == (full, refits + 1)
        box = I.short_box(tris)[np.where(got["prim"] >= 0, got["prim"], 0)] & (got["prim"] >= 0)
        assert box.any() and (got["flags"][got["prim"] >= 0] == 1).all()     # the whole array was kept: all "moved"
        t = hits["t"].reshape(H, W)
        d = rays["dir"].reshape(H, W, 3).astype(np.float64)
        cur = rays["origin"].reshape(H, W, 3) + d / np.linalg.norm(d, axis=-1, keepdims=True) * t[..., None]
        back = got["prev_point"].astype(np.float64) - cur
        assert np.abs(back[box] + np.asarray(I.BOX_SHIFT)).max() < 1e-3
        still = (got["prim"] >= 0) & ~box
        assert np.abs(back[still]).max() < 1e-3
    finally:
        rt.release()


# ---- the motion variants of both reprojections ------------------------------------------------------------
def run_temporal(dev, w, h, pair, motion, out=None):
    cur, cf, hist, hf, view = T.synthetic(w, h, pair)
    bufs = [dev.buffer(a.nbytes, a) for a in (cur, cf, hist, hf)]
    mb = dev.buffer(motion.nbytes, motion) if motion is not None else None
    ob = out if out is not None else dev.buffer(cur.nbytes)
    dev.ctx.TemporalAccumulate(dev.k, *bufs, w, h, ob, view, T.PREV, **T.DEFAULTS, motion=mb)
    return dev.read(ob, (h, w, 4), F), bufs + [mb], ob


def run_reproject(dev, w, h, pair, motion, out=None):
    _, cf, _, hf, view = T.synthetic(w, h, pair)
    hs = I.stats_synthetic(w, h)
    bufs = [dev.buffer(a.nbytes, a) for a in (hs, hf, cf)]
    mb = dev.buffer(motion.nbytes, motion) if motion is not None else None
    ob = out if out is not None else dev.buffer(hs.nbytes)
    dev.ctx.ReprojectSamples(dev.k, *bufs, w, h, ob, view, T.PREV, **RI.DEFAULTS, motion=mb)
    return dev.read(ob, (h, w), ref.STATS), bufs + [mb], ob


def null_motion_calls(dev, w, h, pair):
    """Both Motion entry points with motion NULL, through the library's symbols."""
    cur, cf, hist, hf, view = T.synthetic(w, h, pair)
    hs = I.stats_synthetic(w, h)
    lib, ctx, k = dev.ctx._lib, dev.ctx.handle, dev.k.handle

    def vw(v):
        return N.VIEW(*((ctypes.c_float * 3)(*part) for part in v))
    b = {name: dev.buffer(a.nbytes, a) for name, a in (("cur", cur), ("cf", cf), ("hist", hist), ("hf", hf), ("hs", hs))}
    ot, orp = dev.buffer(cur.nbytes), dev.buffer(hs.nbytes)
    d = T.DEFAULTS
    tp = N.TEMPORAL_PARAMS(vw(view), vw(T.PREV), d["cur_frames"], d["history_frames"], d["max_history"],
                           d["depth_tolerance"], d["normal_threshold"])
    assert lib.rtEnqueueTemporalAccumulateMotion(ctx, k, b["cur"].handle, b["cf"].handle, b["hist"].handle, b["hf"].handle,
                                                 None, w, h, ctypes.byref(tp), ot.handle) == 0
    r = RI.DEFAULTS
    rp = N.REPROJECT_PARAMS(vw(view), vw(T.PREV), r["max_history"], r["depth_tolerance"], r["normal_threshold"])
    assert lib.rtEnqueueReprojectSamplesMotion(ctx, k, b["hs"].handle, b["hf"].handle, b["cf"].handle, None, w, h,
                                               ctypes.byref(rp), orp.handle) == 0
    return dev.read(ot, (h, w, 4), F), dev.read(orp, (h, w), ref.STATS)


@pytest.mark.parametrize("pair", ["same", "shift", "yaw"])
@pytest.mark.parametrize("w,h", T.SIZES)
def test_motion_variants_equal_the_restatement(dev, w, h, pair):
    m = I.motion_records(w, h, pair)
    got, *_ = run_temporal(dev, w, h, pair, m)
    T.same_bytes(got, I.temporal_reference(w, h, pair)[0], f"temporal, {w}x{h}, {pair}")
    got, *_ = run_reproject(dev, w, h, pair, m)
    same_records(got, I.reproject_reference(w, h, pair)[0], f"samples, {w}x{h}, {pair}")
    # motion NULL: the existing calls' bytes
    gt, gr = null_motion_calls(dev, w, h, pair)
    T.same_bytes(gt, T.reference(w, h, pair)[0], f"temporal without motion, {w}x{h}, {pair}")
    _, cf, _, hf, view = T.synthetic(w, h, pair)
    want = reproject_samples_ref.reproject(I.stats_synthetic(w, h), hf, cf, w, h, view, T.PREV, **RI.DEFAULTS)
    same_records(gr, want, f"samples without motion, {w}x{h}, {pair}")


@pytest.mark.parametrize("mode", sorted(MODES))
def test_motion_variants_in_every_math_mode(dev, mode):
    dev.k.set_math_mode(MODES[mode])
    try:
        for (w, h), pair in (((131, 77), "yaw"), ((61, 7), "shift")):
            m = I.motion_records(w, h, pair)
            T.same_bytes(run_temporal(dev, w, h, pair, m)[0], I.temporal_reference(w, h, pair)[0], f"{mode}, {pair}")
            same_records(run_reproject(dev, w, h, pair, m)[0], I.reproject_reference(w, h, pair)[0], f"{mode}, {pair}")
    finally:
        dev.k.set_math_mode(N.MATH_PINNED)


def test_non_finite_motion_rows_equal_the_restatement(dev):
    w, h, pair = 61, 7, "shift"
    m = I.non_finite_motion(w, h, pair)
    cur, cf, hist, hf, view = T.synthetic(w, h, pair)
    assert not np.isfinite(m["prev_point"]).all() and not np.isfinite(m["prev_normal"]).all()
    want, info = ref.temporal(cur, cf, hist, hf, m, w, h, view, T.PREV, **T.DEFAULTS, details=True)
    assert info["history"].any() and not info["history"].all() and np.isfinite(want).all()
    T.same_bytes(run_temporal(dev, w, h, pair, m)[0], want, "non-finite motion rows, temporal")
    want = ref.reproject(I.stats_synthetic(w, h), hf, cf, m, w, h, view, T.PREV, **RI.DEFAULTS)
    same_records(run_reproject(dev, w, h, pair, m)[0], want, "non-finite motion rows, samples")


def test_motion_variants_leave_inputs_and_tail_and_repeat(dev):
    w, h, pair = 131, 77, "shift"
    m = I.motion_records(w, h, pair)
    cur, cf, hist, hf, _ = T.synthetic(w, h, pair)
    hs = I.stats_synthetic(w, h)
    for run, nbytes, inputs in ((run_temporal, cur.nbytes, (cur, cf, hist, hf, m)), (run_reproject, hs.nbytes, (hs, hf, cf, m))):
        tail = 4096
        ob = dev.buffer(nbytes + tail, np.full(nbytes + tail, I.NAN_BYTE, np.uint8))
        _, bufs, _ = run(dev, w, h, pair, m, out=ob)
        raw = dev.read(ob, nbytes + tail, np.uint8)
        assert (raw[nbytes:] == I.NAN_BYTE).all() and not (raw[:nbytes] == I.NAN_BYTE).all()
        for b, a in zip(bufs, inputs):
            assert dev.read(b, a.shape, a.dtype).tobytes() == a.tobytes()
        run(dev, w, h, pair, m, out=ob)
        assert dev.read(ob, nbytes + tail, np.uint8).tobytes() == raw.tobytes()


# ---- ordering, timing, errors -----------------------------------------------------------------------------
def test_each_call_is_ordered_between_a_write_and_a_read_and_behind_queued_frames():
    """Per call: queued frames, WriteBuffer(input), the call, ReadBuffer(output) without a Finish in between, against
    the same steps with a Finish after each on fresh buffers -- and against the restatement."""
    w, h = 61, 7
    n = w * h
    tris = I.scene().triangles
    hits = I.seeded_hits(257)
    pair = "shift"
    cur, cf, hist, hf, view = T.synthetic(w, h, pair)
    m = I.motion_records(w, h, pair)
    hs = I.stats_synthetic(w, h)
    results = {}
    for finish in (False, True):
        rig = Rig(w, h)
        rig.k.set_tuning("perframe_batch", 4)                      # per-frame launches are held back and coalesced
        try:
            def sync():
                if finish:
                    rig.ctx.Finish()

            def frames():
                for f in (1, 2):
                    rig.k.set_uint(N.FRAME_COUNT, f)
                    rig.ctx.ExecuteKernel(rig.k, n)
                sync()

            def read(buf, shape, dtype):
                out = np.empty(shape, dtype)
                rig.ctx.ReadBuffer(buf, out, blocking=False)
                rig.ctx.Finish()
                return out
            got = {}
            pp, pn = prev_records(3, 7)
            # HitMotion: the hits written just before
            hb, mb = rig.buffer(hits.nbytes, np.zeros_like(hits)), rig.buffer(hits.size * 32)
            rig.ctx.Finish()
            frames()
            rig.ctx.WriteBuffer(hb, hits, blocking=False)
            sync()
            rig.ctx.HitMotion(rig.k, hb, 0, hits.size, mb)
            sync()
            got["hit"] = read(mb, hits.size, ref.MOTION)
            # FrameMotion: the kept vertices written just before
            kb, fb = rig.buffer(pp.nbytes, np.zeros_like(pp)), rig.buffer(n * 32)
            rig.ctx.Finish()
            frames()
            rig.ctx.WriteBuffer(kb, pn, blocking=False)
            sync()
            rig.ctx.FrameMotion(rig.k, n, fb, kb, None, 3, 7)
            sync()
            got["frame"] = read(fb, n, ref.MOTION)
            got["frame_want"] = rig.composed(n, rig.buffer(pn.nbytes, pn), None, 3, 7)[0]
            # the two variants: the motion records written just before
            bufs = [rig.buffer(a.nbytes, a) for a in (cur, cf, hist, hf, hs)]
            for name in ("temporal", "samples"):
                rb = rig.buffer(m.nbytes, np.zeros_like(m))
                ob = rig.buffer(cur.nbytes if name == "temporal" else hs.nbytes)
                rig.ctx.Finish()
                frames()
                rig.ctx.WriteBuffer(rb, m, blocking=False)
                sync()
                if name == "temporal":
                    rig.ctx.TemporalAccumulate(rig.k, *bufs[:4], w, h, ob, view, T.PREV, **T.DEFAULTS, motion=rb)
                    sync()
                    got[name] = read(ob, (h, w, 4), F)
                else:
                    rig.ctx.ReprojectSamples(rig.k, bufs[4], bufs[3], bufs[1], w, h, ob, view, T.PREV, **RI.DEFAULTS, motion=rb)
                    sync()
                    got[name] = read(ob, (h, w), ref.STATS)
            # ExtractVertices, last (the scene changes): after an update that is still in the queue
            upd = rig.buffer(pp.nbytes)
            eb = rig.buffer(pp.nbytes, np.zeros_like(pp))
            rig.ctx.Finish()
            frames()
            rig.ctx.WriteBuffer(upd, pp, blocking=False)
            sync()
            rig.ctx.UpdateVertices(rig.tris, 3, 7, upd)
            sync()
            rig.ctx.ExtractVertices(rig.tris, 3, 7, eb)
            sync()
            got["extract"] = read(eb, 7, N.TRI_POINTS_DTYPE)
            results[finish] = got
        finally:
            rig.close()
    for name in results[False]:
        assert results[False][name].tobytes() == results[True][name].tobytes(), name
    got = results[False]
    assert got["extract"].tobytes() == prev_records(3, 7)[0].tobytes()
    ref.same_motion(got["hit"], ref.hit_motion(hits, tris), "behind a queued write")
    assert got["frame"].tobytes() == got["frame_want"].tobytes()
    T.same_bytes(got["temporal"], I.temporal_reference(w, h, pair)[0], "behind a queued write")
    same_records(got["samples"], I.reproject_reference(w, h, pair)[0], "behind a queued write")


def test_timing_counts_each_call_as_one_launch(rig):
    w, h, pair = 61, 7, "shift"
    n = w * h
    cur, cf, hist, hf, view = T.synthetic(w, h, pair)
    m, hs = I.motion_records(w, h, pair), I.stats_synthetic(w, h)
    b = [rig.buffer(a.nbytes, a) for a in (cur, cf, hist, hf, hs, m)]
    hits = I.seeded_hits(257)
    hb, mb, fb = rig.buffer(hits.nbytes, hits), rig.buffer(hits.size * 32), rig.buffer(n * 32)
    ot, osb = rig.buffer(cur.nbytes), rig.buffer(hs.nbytes)
    frame_motion(rig, n, None, None, 0, 0)                                     # (the scene is prepared)
    calls = (lambda: rig.ctx.HitMotion(rig.k, hb, 0, hits.size, mb),
             lambda: rig.ctx.FrameMotion(rig.k, n, fb),
             lambda: rig.ctx.TemporalAccumulate(rig.k, *b[:4], w, h, ot, view, T.PREV, **T.DEFAULTS, motion=b[5]),
             lambda: rig.ctx.ReprojectSamples(rig.k, b[4], b[3], b[1], w, h, osb, view, T.PREV, **RI.DEFAULTS, motion=b[5]))
    rig.k.set_timing(True)
    try:
        for i, call in enumerate(calls):
            rig.k.reset_stats()
            before = rig.k.stats()
            call()
            rig.ctx.Finish()
            after = rig.k.stats()
            assert after["launches"] == before["launches"] + 1 and after["kernel_ms"] > before["kernel_ms"], i
    finally:
        rig.k.set_timing(False)


def test_errors_launch_nothing(rig):
    w, h, pair = 61, 7, "shift"
    n = w * h
    other = T.Device()
    try:
        lib, ctx, k = rig.ctx._lib, rig.ctx.handle, rig.k.handle
        hits = I.seeded_hits(257)
        pp, pn = prev_records(3, 7)
        hb, pb, nb = rig.buffer(hits.nbytes, hits), rig.buffer(pp.nbytes, pp), rig.buffer(pn.nbytes, pn)
        sentinel = np.full(max(n, hits.size) * 32, I.NAN_BYTE, np.uint8)
        mb = rig.buffer(sentinel.nbytes, sentinel)
        small, foreign = rig.buffer(7 * 48 - 16), other.buffer(sentinel.nbytes)
        bare = other.k.handle
        H = lambda buf: buf.handle if buf is not None else None   # noqa: E731

        def extract(t, first, cnt, p, nn, c=ctx):
            return lib.rtEnqueueExtractVertices(c, H(t), first, cnt, H(p), H(nn))

        def hit(kk, hh, first, cnt, p, nn, ft, nt, out):
            return lib.rtEnqueueHitMotion(ctx, kk, H(hh), first, cnt, H(p), H(nn), ft, nt, H(out))

        def frame(kk, cnt, p, nn, ft, nt, out):
            return lib.rtEnqueueFrameMotion(ctx, kk, cnt, H(p), H(nn), ft, nt, H(out))

        rig.k.set_timing(True)
        rig.k.reset_stats()
        before = rig.read(rig.tris, 72, N.TRIANGLE_DTYPE).tobytes()
        # rtEnqueueExtractVertices: rtEnqueueUpdateVertices' rows in its order
        assert extract(rig.tris, 3, 7, pb, nb, c=None) == -34
        assert extract(None, 3, 7, pb, nb) == -38 and extract(rig.tris, 3, 7, None, nb) == -38
        assert extract(rig.tris, 3, 7, pb, foreign) == -38 and extract(foreign, 3, 7, pb, nb) == -38
        assert extract(rig.tris, 3, 7, rig.tris, None) == -38 and extract(rig.tris, 3, 7, pb, rig.tris) == -38
        assert extract(rig.tris, 3, 7, pb, pb) == -38
        assert extract(rig.tris, 70, 3, pb, nb) == -61 and extract(rig.tris, 73, 0, pb, nb) == -61
        assert extract(rig.tris, 3, 7, small, nb) == -61 and extract(rig.tris, 3, 7, pb, small) == -61
        assert extract(rig.tris, 70, 3, rig.tris, nb) == -38                              # ... before the sizes
        assert extract(rig.tris, 3, 0, pb, nb) == 0
        # rtEnqueueHitMotion
        assert hit(None, hb, 0, 257, pb, nb, 3, 7, mb) == -48 and hit(bare, hb, 0, 257, pb, nb, 3, 7, mb) == -48
        assert hit(k, None, 0, 257, pb, nb, 3, 7, mb) == -38 and hit(k, foreign, 0, 257, pb, nb, 3, 7, mb) == -38
        assert hit(k, hb, 2 ** 31, 1, pb, nb, 3, 7, mb) == -30
        assert hit(k, hb, 0, 257, pb, nb, 3, 7, None) == -38 and hit(k, hb, 0, 257, pb, nb, 3, 7, foreign) == -38
        assert hit(k, hb, 0, 257, pb, nb, 3, 7, hb) == -38
        assert hit(k, hb, 0, 257, None, nb, 3, 7, mb) == -38 and hit(k, hb, 0, 257, foreign, nb, 3, 7, mb) == -38
        assert hit(k, hb, 0, 257, pb, foreign, 3, 7, mb) == -38 and hit(k, hb, 0, 257, mb, nb, 3, 7, mb) == -38
        assert hit(k, hb, 1, 257, pb, nb, 3, 7, mb) == -61 and hit(k, hb, 0, 257, small, nb, 3, 7, mb) == -61
        assert hit(k, hb, 0, 257, pb, small, 3, 7, mb) == -61 and hit(k, hb, 0, 257, pb, nb, 3, 8, mb) == -61
        assert hit(k, hb, 0, 257, pb, nb, 70, 3, mb) == -61                                # beyond the scene
        assert hit(bare, hb, 0, 257, pb, nb, 3, 7, mb) == -48
        assert hit(k, hb, 0, 0, pb, nb, 3, 7, mb) == 0
        # rtEnqueueFrameMotion
        assert frame(None, n, pb, nb, 3, 7, mb) == -48 and frame(k, n, pb, nb, 3, 7, None) == -38
        assert frame(k, n, pb, nb, 3, 7, foreign) == -38
        assert frame(k, 0, pb, nb, 3, 7, mb) == -63 and frame(k, 2 ** 31 + 1, pb, nb, 3, 7, mb) == -63
        assert frame(k, sentinel.nbytes // 32 + 1, pb, nb, 3, 7, mb) == -61
        assert frame(k, n, None, nb, 3, 7, mb) == -38 and frame(k, n, mb, nb, 3, 7, mb) == -38
        assert frame(k, n, pb, small, 3, 7, mb) == -61 and frame(k, n, pb, nb, 70, 3, mb) == -61
        # the motion buffer of the two variants
        cur, cf, hist, hf, view = T.synthetic(w, h, pair)
        hs = I.stats_synthetic(w, h)
        b = [rig.buffer(a.nbytes, a) for a in (cur, cf, hist, hf, hs)]
        ot, osb = rig.buffer(cur.nbytes, sentinel[:cur.nbytes]), rig.buffer(hs.nbytes, sentinel[:hs.nbytes])
        short_m = rig.buffer(n * 32 - 32)
        import clrt
        for bad in (foreign, short_m, ot):
            with pytest.raises(clrt.RTError) as e:
                rig.ctx.TemporalAccumulate(rig.k, *b[:4], w, h, ot, view, T.PREV, **T.DEFAULTS, motion=bad)
            assert e.value.code == (-61 if bad is short_m else -38)
        for bad in (foreign, short_m, osb):
            with pytest.raises(clrt.RTError) as e:
                rig.ctx.ReprojectSamples(rig.k, b[4], b[3], b[1], w, h, osb, view, T.PREV, **RI.DEFAULTS, motion=bad)
            assert e.value.code == (-61 if bad is short_m else -38)
        # a kernel without a scene: the queries' row
        free = T.Device()
        try:
            fm, fh = free.buffer(n * 32), free.buffer(hits.nbytes, hits)
            assert lib.rtEnqueueHitMotion(free.ctx.handle, free.k.handle, fh.handle, 0, 257, None, None, 0, 0, fm.handle) == -52
            assert lib.rtEnqueueFrameMotion(free.ctx.handle, free.k.handle, n, None, None, 0, 0, fm.handle) == -52
        finally:
            free.close()
        rig.ctx.Finish()
        assert rig.k.stats()["launches"] == 0
        assert (rig.read(mb, sentinel.nbytes, np.uint8) == I.NAN_BYTE).all()              # nothing was launched
        assert (rig.read(ot, cur.nbytes, np.uint8) == I.NAN_BYTE).all() and (rig.read(osb, hs.nbytes, np.uint8) == I.NAN_BYTE).all()
        assert rig.read(pb, 7, N.TRI_POINTS_DTYPE).tobytes() == pp.tobytes()
        assert rig.read(rig.tris, 72, N.TRIANGLE_DTYPE).tobytes() == before
        # the kernel that saw every error still works
        assert hit(k, hb, 0, 257, pb, nb, 3, 7, mb) == 0
        ref.same_motion(rig.read(mb, 257, ref.MOTION), ref.hit_motion(hits, I.scene().triangles, pp, pn, 3, 7), "after the errors")
        assert rig.k.stats()["launches"] == 1
    finally:
        rig.k.set_timing(False)
        other.close()


# ---- the whole pipeline ---------------------------------------------------------------------------------
def test_temporal_with_motion_keeps_the_history_of_a_moved_box(cornell):
    """Cornell at 64 x 48: eight frames, temporal(); the short box translated with move_vertices(keep_previous=True);
    two new frames, temporal(motion=True).  The result equals a host replay of the same calls through the
    restatements on the read-back buffers; the moved box's pixels whose history tap passes keep their history
    (w > n_frames); and the camera-only definition on the same buffers either finds no history for those pixels or
    reads it at the pixel itself, a surface point at least the shift's component across the ray away from where the
    pixel's surface point was.  Measured on an MI355X: see the printed line."""
    import clrt
    W, H, n_old, n_new = 64, 48, 8, 2
    rt = clrt.Raytracer(W, H)
    rt.Init()
    try:
        rt.upload_scene(cornell)
        tris = I.scene().triangles
        for _ in range(n_old):
            rt.RenderFrame()
        first_out = rt.temporal()
        assert (first_out[..., 3] == n_old).all()
        pos, _ = I.moved_scene()
        first, n = I.BOX_RANGE
        rt.move_vertices(pos[first:first + n], first=first, keep_previous=True)
        rt.frame_count = 1
        for _ in range(n_new):
            rt.RenderFrame()
        got = rt.temporal(motion=True)
        assert rt._motion["used"] == {"temporal"}
        now, prev = rt._temporal_at, 1 - rt._temporal_at

        def read(buf, shape, dtype):
            out = np.empty(shape, dtype)
            rt.ctx.ReadBuffer(buf, out, blocking=True)
            return out
        cur = read(rt.output, (H, W, 4), F)
        cf, hf = (read(rt._temporal_feat[i], (H, W), N.PIXEL_FEATURES_DTYPE) for i in (now, prev))
        hist = read(rt._temporal_img[prev], (H, W, 4), F)
        m = read(rt._motion["records"], (H, W), ref.MOTION)
        assert hist.tobytes() == first_out.tobytes()
        view = (rt.camera.position, rt.camera.front, rt.camera.up)
        prm = dict(cur_frames=float(n_new), history_frames=0.0, max_history=32.0, depth_tolerance=0.05, normal_threshold=0.9)
        want, info = ref.temporal(cur, cf, hist, hf, m, W, H, view, view, **prm, details=True)
        T.same_bytes(got, want, "temporal(motion=True) against the host replay")
        # the records themselves: the restatement over the kept vertices and the device's closest hits
        rays = ref.centre_rays(W, H, view)
        hits = rt.cast(rays["origin"], rays["dir"])
        moved = tris.copy()
        for i, v in enumerate(("v1", "v2", "v3")):
            moved[v]["position"][:, :3] = pos[:, i]
        keep_p, keep_n = ref.tri_points(ref.vertices(tris, "position")), ref.tri_points(ref.vertices(tris, "normal"))
        assert m.reshape(-1).tobytes() == ref.hit_motion(hits, moved, keep_p, keep_n, 0, len(tris)).tobytes()
        # the moved box keeps its history
        box = (m["prim"] >= 0) & I.short_box(tris)[np.where(m["prim"] >= 0, m["prim"], 0)]
        kept = box & info["history"]
        assert box.sum() > 100 and kept.sum() > box.sum() // 2, (int(box.sum()), int(kept.sum()))
        assert (got[..., 3][kept] > n_new).all() and (got[..., 3][box & ~info["history"]] == n_new).all()
        # ... which the camera-only definition loses or takes from another surface point
        _, plain = temporal_ref.temporal(cur, cf, hist, hf, W, H, view, view, **prm, details=True)
        d = rays["dir"].reshape(H, W, 3).astype(np.float64)
        u = d / np.linalg.norm(d, axis=-1, keepdims=True)
        shift = np.asarray(I.BOX_SHIFT, np.float64)
        across = np.linalg.norm(shift - (u @ shift)[..., None] * u, axis=-1)      # the shift's component across the ray
        seen_then = np.asarray(view[0], np.float64) + u * hf["depth"][..., None].astype(np.float64)
        apart = np.linalg.norm(seen_then - m["prev_point"].astype(np.float64), axis=-1)
        ghost = kept & plain["history"]
        assert (~plain["history"][kept] | (apart[kept] >= 0.5 * across[kept])).all()
        assert across[kept].min() > 0.5 and (kept & ~plain["history"]).any()
        print(f"temporal(motion=True): {int(box.sum())} box pixels, {int(kept.sum())} keep history; camera-only loses "
              f"{int((kept & ~plain['history']).sum())} of them and ghosts {int(ghost.sum())}")
        # a second call without a move in between: nothing is kept to use, the records say where things are now
        again = rt.temporal(motion=True)
        m2 = read(rt._motion["records"], (H, W), ref.MOTION)
        assert (m2["flags"] == 0).all() and np.isfinite(again).all()
    finally:
        rt.release()


def test_reproject_samples_motion_carries_the_statistics_of_a_moved_box(cornell):
    """Cornell at 64 x 48: a few adaptive rounds; the short box translated with move_vertices(keep_previous=True), which
    also takes the history features; reproject_samples_motion().  The statistics equal a host replay through the
    restatement on the read-back buffers, the history features are the ones from before the move, pixels of the moved
    box carry statistics, and the plain call on the same buffers carries for those pixels what the pixel itself
    showed before the move."""
    import clrt
    W, H = 64, 48
    rt = clrt.Raytracer(W, H)
    rt.Init()
    try:
        rt.upload_scene(cornell)
        tris = I.scene().triangles
        rt.render_adaptive(4, threshold=0.2, floor_y=0.01, min_samples=2, max_samples=6, radius=1)
        old = rt.sample_stats()
        feat_before = rt.features(4)
        pos, _ = I.moved_scene()
        first, n = I.BOX_RANGE
        rt.move_vertices(pos[first:first + n], first=first, keep_previous=True)
        assert rt._motion["feat"] == 4
        rt.reproject_samples_motion(rt.camera)
        assert rt._motion["used"] == {"samples"}
        got = rt.sample_stats()

        def read(buf, dtype):
            out = np.empty((H, W), dtype)
            rt.ctx.ReadBuffer(buf, out, blocking=True)
            return out
        hf, cf = (read(b, N.PIXEL_FEATURES_DTYPE) for b in rt._reproject_feat)
        m = read(rt._motion["records"], ref.MOTION)
        assert hf.tobytes() == feat_before.tobytes() and cf.tobytes() != hf.tobytes()
        assert read(rt._adaptive_buffers()["spare"], ref.STATS).tobytes() == old.tobytes()
        view = (rt.camera.position, rt.camera.front, rt.camera.up)
        want, info = ref.reproject(old, hf, cf, m, W, H, view, view, 16.0, 0.05, 0.9, details=True)
        same_records(got, want, "reproject_samples_motion against the host replay")
        box = (m["prim"] >= 0) & I.short_box(tris)[np.where(m["prim"] >= 0, m["prim"], 0)]
        kept = box & info["carried"]
        assert box.sum() > 100 and kept.sum() > box.sum() // 2, (int(box.sum()), int(kept.sum()))
        assert (got["n"][kept] >= 1).all() and (got["n"][box & ~info["carried"]] == 0).all()
        # the camera did not move: the plain definition reads each pixel's own history, whatever it showed then
        plain, pinfo = reproject_samples_ref.reproject(old, hf, cf, W, H, view, view, 16.0, 0.05, 0.9, details=True)
        assert (kept & ~pinfo["carried"]).any() and (plain[kept].tobytes() != want[kept].tobytes())
    finally:
        rt.release()


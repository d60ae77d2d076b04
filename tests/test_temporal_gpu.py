"""GPU: temporal reprojection (rtEnqueueTemporalAccumulate, Raytracer.temporal).

The reference is tests/temporal_ref.py, the numpy float32 restatement of the definition (checked on the CPU
in test_temporal_plan.py): the device's bytes must equal its bytes.

Inputs are seeded and synthetic, made once per size and camera pair and shared (never modified).  The scene
is a wall at y = 20 and a nearer slab at y = 12 for |x| < 3, |z - 8| < 3; a view's features hold the depth
along each of its centre rays, the normal (0, -1, 0), and about 20 % of the pixels uncovered at random.
The prescribed normals are the same everywhere, so no tap would ever fail the normal test; as in real
feature buffers (a mean over frames to which a miss adds nothing, not normalised again) about 5 % of the
covered pixels therefore have coverage 0.75 and the normal (0, -0.75, 0): a tap between two of them has
the dot product 0.5625 < 0.9.  Colours are random in [0, 2), history sample counts 1 .. 8.  The previous
camera is the reference default; the current one is the same, shifted to (0.37, -25, 8.6), yawed by
0.2 rad, moved forward to y = -20, or facing away (yaw 3.0).  The sizes (w x h): 1 x 1; 5 x 3, smaller than
a wave row; 61 x 7, a partial row of lanes and a partial tile of rows; 131 x 77, several workgroups with
partial edges.

Non-finite inputs: defined behaviour, every class the CPU sweep covers.  IEEE leaves the sign and payload
of a NaN that an operation produces open (x86 and gfx950 differ), so non-finite values are placed where
the definition selects them away or copies them -- depths of both views, history sample counts, history
colours of taps that do not count, current colours of pixels without history -- and not where they would
flow through the blend's arithmetic into an output.
"""
import ctypes
import functools

import numpy as np
import pytest

import temporal_ref
from clrt import _native as N

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = [(1, 1), (5, 3), (61, 7), (131, 77)]
PREV = ((0.0, -25.0, 8.5), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))


def yawed(pos, yaw):
    return (tuple(pos), (float(F(np.sin(yaw))), float(F(np.cos(yaw))), 0.0), (0.0, 0.0, 1.0))


PAIRS = {"same": PREV, "shift": yawed((0.37, -25.0, 8.6), 0.0), "yaw": yawed((0.0, -25.0, 8.5), 0.2),
         "forward": yawed((0.0, -20.0, 8.5), 0.0), "away": yawed((0.0, -25.0, 8.5), 3.0)}
DEFAULTS = dict(cur_frames=2.0, history_frames=0.0, max_history=32.0, depth_tolerance=0.05, normal_threshold=0.9)
VARIANTS = {"defaults": {}, "history_frames": {"history_frames": 5.0}, "ema": {"max_history": 3.0},
            "depth_exact": {"depth_tolerance": 0.0}, "any_normal": {"normal_threshold": -1.0},
            "one_frame": {"cur_frames": 1.0}}
NAN_BYTE = 0xFF


def scene_features(w, h, view, rng, uncover=True):
    """The wall-and-slab scene seen from `view`: depth along the centre rays, normal (0, -1, 0)."""
    pos, front, up = (np.asarray(v, F) for v in view)
    u = temporal_ref.centre_rays(w, h, front, up)
    with np.errstate(all="ignore"):
        t_wall, t_slab = (F(20) - pos[1]) / u[..., 1], (F(12) - pos[1]) / u[..., 1]
        x = pos + u * t_slab[..., None]
        on_slab = (np.abs(x[..., 0]) < 3) & (np.abs(x[..., 2] - 8) < 3) & (t_slab > 0)
        t = np.where(on_slab, t_slab, t_wall).astype(F)
        covered = (t > 0) & np.isfinite(t)
    f = np.zeros((h, w), N.PIXEL_FEATURES_DTYPE)
    f["albedo"] = 0.5
    cov = covered.astype(F)
    if uncover:
        cov[rng.random((h, w)) < 0.2] = 0
        cov[(rng.random((h, w)) < 0.05) & (cov > 0)] = 0.75
    f["depth"] = np.where(covered, t, 0)
    f["coverage"] = cov
    f["normal"][..., 1] = -cov
    return f


@functools.lru_cache(maxsize=None)
def synthetic(w, h, pair):
    """(cur, cur_features, hist, hist_features, cur view); read-only."""
    rng = np.random.default_rng(1000 * w + h)
    hist = (rng.random((h, w, 4)) * 2).astype(F)
    hist[..., 3] = rng.integers(1, 9, (h, w))
    cur = (rng.random((h, w, 4)) * 2).astype(F)
    hf = scene_features(w, h, PREV, rng, uncover=w * h > 1)
    cf = scene_features(w, h, PAIRS[pair], rng, uncover=w * h > 1)
    for a in (cur, cf, hist, hf):
        a.setflags(write=False)
    return cur, cf, hist, hf, PAIRS[pair]


def params(variant):
    return {**DEFAULTS, **VARIANTS[variant]}


@functools.lru_cache(maxsize=None)
def reference(w, h, pair, variant="defaults", history=True):
    cur, cf, hist, hf, view = synthetic(w, h, pair)
    out, info = temporal_ref.temporal(cur, cf, hist if history else None, hf if history else None, w, h, view, PREV,
                                      **params(variant), details=True)
    out.setflags(write=False)
    return out, info


class Device:
    """A context and a kernel with nothing bound (the reprojection needs no scene), and buffers on demand."""

    def __init__(self):
        import clrt
        self.ctx = clrt.CLContext(0)
        self.k = clrt.CLKernel(self.ctx, "KernelEntry")
        self._bufs = []

    def buffer(self, nbytes, host=None):
        if host is None:
            b = self.ctx.create_buffer(N.MEM_READ_WRITE, nbytes)
        else:
            b = self.ctx.create_buffer(N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR, nbytes, np.ascontiguousarray(host))
        self._bufs.append(b)
        return b

    def read(self, buf, shape, dtype):
        out = np.empty(shape, dtype)
        self.ctx.ReadBuffer(buf, out, blocking=True)
        return out

    def run(self, w, h, arrays, view, prm, out=None, history=True):
        cur, cf, hist, hf = arrays
        bufs = [self.buffer(a.nbytes, a) for a in (cur, cf, hist, hf)]
        ob = out if out is not None else self.buffer(cur.nbytes)
        self.ctx.TemporalAccumulate(self.k, bufs[0], bufs[1], bufs[2] if history else None, bufs[3] if history else None,
                                    w, h, ob, view, PREV, **prm)
        return self.read(ob, (h, w, 4), np.float32), bufs, ob

    def close(self):
        self.ctx.Finish()
        for b in self._bufs:
            b.release()
        self.k.release()
        self.ctx.release()


@pytest.fixture(scope="module")
def dev():
    d = Device()
    yield d
    d.close()


def same_bytes(got, want, what):
    a = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 4)
    b = np.ascontiguousarray(want).view(np.uint32).reshape(-1, 4)
    bad = np.flatnonzero((a != b).any(axis=1))
    assert bad.size == 0, (f"{what}: {bad.size} of {len(a)} pixels differ, first {bad[:4]}: "
                           f"{np.ascontiguousarray(got).reshape(-1, 4)[bad[:2]]} vs "
                           f"{np.ascontiguousarray(want).reshape(-1, 4)[bad[:2]]}")


def share(w, h, pair):
    """Of the current view's covered pixels, the share that keeps history (on the reference)."""
    covered = synthetic(w, h, pair)[1]["coverage"] > 0
    return reference(w, h, pair)[1]["history"][covered].mean() if covered.any() else None


def full_share(w, h, pair):
    """The same on the fully covered scene, before pixels are uncovered at random."""
    rng = np.random.default_rng(1)
    hist = np.ones((h, w, 4), F)
    hf, cf = scene_features(w, h, PREV, rng, uncover=False), scene_features(w, h, PAIRS[pair], rng, uncover=False)
    _, info = temporal_ref.temporal(hist, cf, hist, hf, w, h, PAIRS[pair], PREV, **DEFAULTS, details=True)
    covered = cf["coverage"] > 0
    return info["history"][covered].mean() if covered.any() else None


# ---- 1: bytes equal to the restatement -----------------------------------------------------------
def test_inputs_are_not_trivial():
    """Before anything is compared, on the reference: history is kept and lost, taps are counted in part, and
    each of the four tests rules some tap out."""
    w, h = 131, 77
    assert 0.5 < share(w, h, "yaw") < 0.95
    # the fully covered scene keeps all its history under the three small moves, at every size; under the yaw
    # the pixels that come into view have none (0.8, 0.74, 0.80 of the covered ones keep it; none at 1 x 1)
    for ww, hh in SIZES:
        for pair in ("same", "shift", "forward"):
            assert full_share(ww, hh, pair) == 1.0, (ww, hh, pair)
        assert full_share(ww, hh, "away") is None
    assert [round(float(full_share(ww, hh, "yaw")), 2) for ww, hh in SIZES] == [0.0, 0.8, 0.74, 0.8]
    # with a fifth of the pixels uncovered a lone tap is often missing: less history, but most of it stays
    assert 0.5 < share(w, h, "same") < share(w, h, "shift") < 1.0
    assert not (synthetic(w, h, "away")[1]["coverage"] > 0).any() and not reference(w, h, "away")[1]["history"].any()
    for pair in ("same", "shift", "yaw", "forward"):
        out, info = reference(w, h, pair)
        cur = synthetic(w, h, pair)[0]
        assert ((info["counted"] >= 1) & (info["counted"] <= 3)).any(), pair
        assert (info["counted"] == 4).any(), pair
        assert (out[..., :3][info["history"]] != cur[..., :3][info["history"]]).any()
        assert len(np.unique(out[..., 3])) > 4                     # fractional sample counts
    _, info = reference(w, h, "shift")
    for reason in ("outside", "coverage", "depth", "normal"):
        assert info["rejected"][reason] > 0, (reason, info["rejected"])
    assert reference(w, h, "yaw")[1]["rejected"]["outside"] > 0
    # the variants change the answer
    base = reference(w, h, "shift")[0]
    for variant in VARIANTS:
        if variant != "defaults":
            assert (reference(w, h, "shift", variant)[0] != base).any(), variant
    assert (reference(w, h, "shift", "ema")[0][..., 3] == 3.0).any()


@pytest.mark.parametrize("pair", sorted(PAIRS))
@pytest.mark.parametrize("w,h", SIZES)
def test_bytes_equal_the_restatement(dev, w, h, pair):
    got, *_ = dev.run(w, h, synthetic(w, h, pair)[:4], PAIRS[pair], params("defaults"))
    same_bytes(got, reference(w, h, pair)[0], f"{w}x{h}, {pair}")


@pytest.mark.parametrize("variant", [v for v in sorted(VARIANTS) if v != "defaults"])
@pytest.mark.parametrize("pair", ["shift", "yaw"])
def test_parameter_variants_equal_the_restatement(dev, pair, variant):
    w, h = 131, 77
    got, *_ = dev.run(w, h, synthetic(w, h, pair)[:4], PAIRS[pair], params(variant))
    same_bytes(got, reference(w, h, pair, variant)[0], f"{pair}, {variant}")


# ---- 2: buffers ----------------------------------------------------------------------------------
def test_inputs_untouched_tail_untouched_repeatable_and_without_history(dev):
    w, h = 131, 77
    arrays = synthetic(w, h, "shift")[:4]
    nbytes, tail = arrays[0].nbytes, 4096
    ob = dev.buffer(nbytes + tail, np.full(nbytes + tail, NAN_BYTE, np.uint8))
    for history in (True, False):
        got, bufs, _ = dev.run(w, h, arrays, PAIRS["shift"], params("defaults"), out=ob, history=history)
        want = reference(w, h, "shift", "defaults", history)[0]
        same_bytes(got, want, f"oversized out, history {history}")
        if not history:
            assert np.array_equal(got[..., :3], arrays[0][..., :3]) and (got[..., 3] == 2.0).all()
        raw = dev.read(ob, nbytes + tail, np.uint8)
        assert (raw[nbytes:] == NAN_BYTE).all()
        for b, a in zip(bufs, arrays):
            assert dev.read(b, a.shape, a.dtype).tobytes() == a.tobytes()
        # the same call again, into the same buffer
        dev.ctx.TemporalAccumulate(dev.k, bufs[0], bufs[1], bufs[2] if history else None, bufs[3] if history else None,
                                   w, h, ob, PAIRS["shift"], PREV, **params("defaults"))
        assert dev.read(ob, nbytes + tail, np.uint8).tobytes() == raw.tobytes()
    # inputs may alias one another: the current image as its own history, at the same camera
    cur, cf = arrays[0], arrays[1]
    cb, fb, o2 = dev.buffer(cur.nbytes, cur), dev.buffer(cf.nbytes, cf), dev.buffer(cur.nbytes)
    dev.ctx.TemporalAccumulate(dev.k, cb, fb, cb, fb, w, h, o2, PAIRS["shift"], PAIRS["shift"], **params("history_frames"))
    want = temporal_ref.temporal(cur, cf, cur, cf, w, h, PAIRS["shift"], PAIRS["shift"], **params("history_frames"))
    same_bytes(dev.read(o2, (h, w, 4), np.float32), want, "aliased inputs")


# ---- 3: non-finite rows (defined behaviour; after the finite ones) ---------------------------------
def non_finite_inputs():
    w, h = 61, 7
    cur, cf, hist, hf, view = (np.array(a) if isinstance(a, np.ndarray) else a for a in synthetic(w, h, "shift"))
    rng = np.random.default_rng(99)
    tiny, big = F(1e-45), F(3.4028235e38)
    classes = np.array([np.inf, -np.inf, np.nan, 0.0, -0.0, tiny, -tiny, big, -big, 1e-38, -20.0], F)
    nan_payload = np.array([0x7F800001, 0xFFC12345], np.uint32).view(F)
    classes = np.concatenate([classes, nan_payload])
    # depths of both views, and history sample counts: any class anywhere
    for a in (cf["depth"], hf["depth"], hist[..., 3]):
        at = rng.random((h, w)) < 0.2
        a[at] = rng.choice(classes, int(at.sum()))
    # history colours where the tap cannot count (uncovered, or a sample count below one)
    dead = (hf["coverage"] <= 0) | ~(hist[..., 3] >= 1)
    at = dead & (rng.random((h, w)) < 0.7)
    hist[..., :3][at] = rng.choice(classes, (int(at.sum()), 3))
    return w, h, cur, cf, hist, hf, view, dead


def test_non_finite_rows_equal_the_restatement(dev):
    w, h, cur, cf, hist, hf, view, dead = non_finite_inputs()
    assert dead.any() and not np.isfinite(hist[..., :3][dead]).all()
    prm = params("defaults")
    # current colours of pixels that take the no-history row are copied: any class (found on the reference)
    _, info = temporal_ref.temporal(cur, cf, hist, hf, w, h, view, PREV, **prm, details=True)
    lone = ~info["history"]
    assert lone.any() and info["history"].any()
    cur[..., :3][lone] = np.array([np.inf, np.nan, -np.inf], F)
    cur[..., 3] = F(np.nan)
    want, info = temporal_ref.temporal(cur, cf, hist, hf, w, h, view, PREV, **prm, details=True)
    assert np.array_equal(info["history"], ~lone)
    assert np.isfinite(want[info["history"]]).all()            # nothing non-finite came through the arithmetic
    assert info["rejected"]["count"] > 0 and info["rejected"]["depth"] > 0
    got, *_ = dev.run(w, h, (cur, cf, hist, hf), view, prm)
    same_bytes(got, want, "non-finite depths, counts and unused colours")


# ---- 4: ordering ---------------------------------------------------------------------------------
def test_temporal_is_ordered_behind_queued_frames_and_features(cornell):
    from test_ray_query import Rig
    W, H = 128, 72
    hist = synthetic(131, 77, "same")[2][:H, :W].copy()
    results = []
    for finish in (False, True):
        g = Rig(cornell, W=W, H=H, perframe_batch=None)   # (the library default: frames coalesce)
        try:
            fb, ob = g.buffer(W * H * 32), g.buffer(W * H * 16)
            for f in range(1, 5):
                g.r.frame(f, light_bounces=2)
                if finish:
                    g.ctx.Finish()
            g.k.set_uint(N.FRAME_COUNT, 1)
            g.ctx.FrameFeatures(g.k, W * H, 4, fb)
            if finish:
                g.ctx.Finish()
            hb = g.buffer(hist.nbytes, hist)
            # the image's own features as the history's: every covered pixel reprojects onto itself
            g.ctx.TemporalAccumulate(g.k, g.r.out, fb, hb, fb, W, H, ob, PREV, PREV, 4.0, 0.0, 32.0, 0.05, 0.9)
            results.append((g.read(ob, (H, W, 4), np.float32), g.r.result().reshape(H, W, 4),
                            g.read(fb, (H, W), N.PIXEL_FEATURES_DTYPE)))
        finally:
            g.close()
    (a, img_a, feat_a), (b, img_b, feat_b) = results
    assert img_a[..., :3].any() and img_a.tobytes() == img_b.tobytes() and feat_a.tobytes() == feat_b.tobytes()
    assert a.tobytes() == b.tobytes()
    want, info = temporal_ref.temporal(img_a, feat_a, hist, feat_a, W, H, PREV, PREV, 4.0, 0.0, 32.0, 0.05, 0.9,
                                       details=True)
    assert info["history"].mean() > 0.3
    same_bytes(a, want, "behind four queued frames and their features")


# ---- 5: timing and errors ------------------------------------------------------------------------
def test_timing_counts_the_call_as_one_launch(dev):
    w, h = 131, 77
    dev.k.set_timing(True)
    try:
        dev.k.reset_stats()
        before = dev.k.stats()
        got, *_ = dev.run(w, h, synthetic(w, h, "yaw")[:4], PAIRS["yaw"], params("defaults"))
        after = dev.k.stats()
        assert after["launches"] == before["launches"] + 1 and after["kernel_ms"] > before["kernel_ms"]
        same_bytes(got, reference(w, h, "yaw")[0], "with timing on")
    finally:
        dev.k.set_timing(False)


def test_errors_launch_nothing(dev):
    import clrt
    w, h = 61, 7
    cur, cf, hist, hf, view = synthetic(w, h, "shift")
    other = Device()
    try:
        lib, ctx, k = dev.ctx._lib, dev.ctx.handle, dev.k.handle
        cb, fb, hb, gb = (dev.buffer(a.nbytes, a) for a in (cur, cf, hist, hf))
        sentinel = np.full(cur.nbytes, NAN_BYTE, np.uint8)
        ob = dev.buffer(sentinel.nbytes, sentinel)
        small = dev.buffer(cur.nbytes - 16)
        foreign = other.buffer(cf.nbytes)

        def vw(v):
            return N.VIEW(*((ctypes.c_float * 3)(*part) for part in v))

        def prm(**kw):
            p = {**DEFAULTS, "cur": view, "prev": PREV, **kw}
            return N.TEMPORAL_PARAMS(vw(p["cur"]), vw(p["prev"]), p["cur_frames"], p["history_frames"], p["max_history"],
                                     p["depth_tolerance"], p["normal_threshold"])

        def rc(kernel, c, f, hi, hfe, ww, hh, p, o):
            hd = [b.handle if b else None for b in (c, f, hi, hfe, o)]
            return lib.rtEnqueueTemporalAccumulate(ctx, kernel, hd[0], hd[1], hd[2], hd[3], ww, hh,
                                                   None if p is None else ctypes.byref(p), hd[4])

        ok = prm()
        nan, inf = float("nan"), float("inf")
        dev.k.set_timing(True)
        dev.k.reset_stats()
        assert rc(None, cb, fb, hb, gb, w, h, ok, ob) == -48 and rc(other.k.handle, cb, fb, hb, gb, w, h, ok, ob) == -48
        assert rc(k, cb, fb, hb, gb, w, h, None, ob) == -30
        assert rc(k, cb, fb, hb, gb, 0, h, ok, ob) == -30 and rc(k, cb, fb, hb, gb, w, 0, ok, ob) == -30
        assert rc(k, cb, fb, hb, gb, 65536, 32769, ok, ob) == -30
        bad_view = ((0.0, nan, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
        assert rc(k, cb, fb, hb, gb, w, h, prm(cur=bad_view), ob) == -30
        assert rc(k, cb, fb, hb, gb, w, h, prm(prev=(PREV[0], (0.0, inf, 0.0), PREV[2])), ob) == -30
        for key, values in (("cur_frames", (nan, 0.5, 2.0 ** 21)), ("history_frames", (-1.0, inf, nan, 0.5, 2.0 ** 21)),
                            ("max_history", (nan, 1.0, 2.0 ** 21)), ("depth_tolerance", (nan, -0.1, 1.5)),
                            ("normal_threshold", (nan, -1.5, 1.5))):
            for bad in values:
                assert rc(k, cb, fb, hb, gb, w, h, prm(**{key: bad}), ob) == -30, (key, bad)
        assert rc(k, None, None, None, gb, w, h, prm(cur_frames=0.0), None) == -30      # ... checked before the buffers
        assert rc(k, cb, fb, hb, None, w, h, ok, ob) == -38 and rc(k, cb, fb, None, gb, w, h, ok, ob) == -38
        assert rc(k, None, fb, hb, gb, w, h, ok, ob) == -38 and rc(k, cb, None, hb, gb, w, h, ok, ob) == -38
        assert rc(k, cb, fb, hb, gb, w, h, ok, None) == -38 and rc(k, cb, fb, hb, foreign, w, h, ok, ob) == -38
        for same in (cb, fb, hb, gb):
            assert rc(k, cb, fb, hb, gb, w, h, ok, same) == -38                            # out is an input
        assert rc(k, cb, fb, hb, gb, w + 1, h, ok, cb) == -38                              # ... checked before the sizes
        assert rc(k, cb, fb, hb, gb, w, h, ok, small) == -61 and rc(k, small, fb, hb, gb, w, h, ok, ob) == -61
        assert rc(k, cb, small, hb, gb, w, h, ok, ob) == -61 and rc(k, cb, fb, small, gb, w, h, ok, ob) == -61
        assert rc(k, cb, fb, hb, small, w, h, ok, ob) == -61 and rc(k, cb, fb, hb, gb, w, h + 1, ok, ob) == -61
        assert dev.k.stats()["launches"] == 0
        assert (dev.read(ob, cur.nbytes, np.uint8) == NAN_BYTE).all()                      # nothing was launched
        with pytest.raises(clrt.RTError):
            dev.ctx.TemporalAccumulate(dev.k, cb, fb, hb, gb, w, h, cb, view, PREV)
        # the kernel that saw every error still works
        assert rc(k, cb, fb, hb, gb, w, h, ok, ob) == 0
        same_bytes(dev.read(ob, (h, w, 4), np.float32), reference(w, h, "shift")[0], "after the errors")
        assert dev.k.stats()["launches"] == 1
    finally:
        dev.k.set_timing(False)
        other.close()


# ---- 6: the whole pipeline -----------------------------------------------------------------------
@pytest.mark.parametrize("math_name", ["pinned", "shipped"])
def test_raytracer_temporal_equals_the_restatement_and_lowers_the_error(cornell, math_name):
    """8 frames and temporal(), the camera moved by (0.37, 0, 0.1), 8 new frames and temporal() again: the device's
    bytes equal temporal_ref's on the read-back inputs, and the error against 256 frames at the new camera falls.
    Measured on an MI355X: mse 0.05323 -> 0.03047, ratio 0.5725 in pinned and in shipped math, 0.90 of the covered
    pixels keeping history."""
    import clrt
    W, H, FRAMES, LONG = 128, 72, 8, 256
    rt = clrt.Raytracer(W, H)
    rt.Init()
    try:
        rt.upload_scene(cornell)
        rt.kernel.set_math_mode({"pinned": N.MATH_PINNED, "shipped": N.MATH_SHIPPED}[math_name])
        assert rt.light_bounces == 9

        def inputs():
            """The accumulation buffer and the features of frames 1 .. 8 at the current camera, read back."""
            img = np.empty((H, W, 4), np.float32)
            rt.ctx.ReadBuffer(rt.output, img, blocking=True)
            at, rt.frame_count = rt.frame_count, 1
            feat = rt.features(FRAMES)
            rt.frame_count = at
            return img, feat

        for _ in range(FRAMES):
            rt.RenderFrame()
        first = rt.temporal()
        assert first.shape == (H, W, 4) and first.dtype == np.float32 and rt.frame_count == FRAMES + 1
        img0, feat0 = inputs()
        view0 = (rt.camera.position, rt.camera.front, rt.camera.up)
        assert img0.tobytes() == rt.pixels.reshape(H, W, 4).tobytes()                    # BUFFER_OUT is left alone
        same_bytes(first, temporal_ref.temporal(img0, feat0, None, None, W, H, view0, view0, 8.0), "first call")
        assert (first[..., 3] == 8.0).all() and np.array_equal(first[..., :3], img0[..., :3])

        # the camera moves: the reference starts over with frame 1
        p = rt.camera.position
        rt.camera = clrt.renderer.Camera(position=(p[0] + 0.37, p[1], p[2] + 0.1))
        rt.frame_count = 1
        for _ in range(FRAMES):
            rt.RenderFrame()
        second = rt.temporal()
        assert rt.frame_count == FRAMES + 1
        img1, feat1 = inputs()
        view1 = (rt.camera.position, rt.camera.front, rt.camera.up)
        want, info = temporal_ref.temporal(img1, feat1, first, feat0, W, H, view1, view0, 8.0, 0.0, 32.0, 0.05, 0.9,
                                           details=True)
        covered = feat1["coverage"] > 0
        assert 0.3 < covered.mean() and info["history"][covered].mean() > 0.5
        same_bytes(second, want, f"Raytracer.temporal after a move, {math_name}")
        assert (second[..., 3][info["history"]] > 8.0).all() and (second[..., 3] <= 32.0).all()

        # reset_history: the next call starts from the image alone
        rt.reset_history()
        third = rt.temporal(FRAMES, max_history=16.0)
        assert (third[..., 3] == 8.0).all() and np.array_equal(third[..., :3], img1[..., :3])

        # quality: against 256 frames at the new camera, over covered pixels
        rt.set_uniforms()
        rt.ctx.ExecuteKernelFrames(rt.kernel, W * H, LONG - FRAMES)
        out = np.empty((H, W, 4), np.float32)
        rt.ctx.ReadBuffer(rt.output, out, blocking=True)
        truth = out[..., :3].astype(np.float64)
        assert (out[..., :3] != img1[..., :3]).any()
        mse_raw = ((img1[..., :3] - truth) ** 2)[covered].mean()
        mse_temporal = ((second[..., :3] - truth) ** 2)[covered].mean()
        ratio = mse_temporal / mse_raw
        print(f"temporal {math_name}: mse {mse_raw:.6g} -> {mse_temporal:.6g}, ratio {ratio:.4f}, "
              f"history share {info['history'][covered].mean():.3f}")
        assert ratio < RATIO_BOUND, ratio
    finally:
        rt.release()


# The midpoint between the measured ratio, 0.5725, and 1 (the denoiser's precedent: measured 0.384, asserted < 0.75).
RATIO_BOUND = 0.786

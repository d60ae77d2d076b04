"""GPU: reprojection of the adaptive sample statistics (rtEnqueueReprojectSamples, Raytracer.reproject_samples).

The reference is tests/reproject_samples_ref.py, the numpy float32 restatement of the definition (checked on the CPU
in test_reproject_samples_plan.py, where a stand-alone program compiled from the kernel's own math texts gives its
bytes): the device's bytes must equal its bytes, in every math mode of the kernel object.

Inputs are reproject_samples_inputs.py's: seeded, synthetic, made once per size and camera pair and shared.  The
sizes (w x h): 1 x 1; 5 x 3, smaller than a wave row; 61 x 7, a partial row of lanes and a partial tile of rows;
131 x 77, several workgroups with partial edges.  Non-finite values are placed only where the definition selects
them away (IEEE leaves the sign and payload of a NaN that an operation produces open).
"""
import ctypes

import numpy as np
import pytest

import adaptive_ref
import reproject_samples_inputs as I
import reproject_samples_ref as ref
from clrt import _native as N
from test_reproject_samples_plan import same_records
from test_temporal_gpu import Device

pytestmark = pytest.mark.gpu

F = np.float32
MODES = {"pinned": N.MATH_PINNED, "devicelib": N.MATH_DEVICELIB, "shipped": N.MATH_SHIPPED}


@pytest.fixture(scope="module")
def dev():
    d = Device()
    yield d
    d.close()


def run(dev, w, h, arrays, view, prm, out=None):
    hs, hf, cf = arrays
    bufs = [dev.buffer(a.nbytes, a) for a in (hs, hf, cf)]
    ob = out if out is not None else dev.buffer(hs.nbytes)
    dev.ctx.ReprojectSamples(dev.k, bufs[0], bufs[1], bufs[2], w, h, ob, view, I.PREV, **prm)
    return dev.read(ob, (h, w), ref.STATS), bufs, ob


# ---- 1: bytes equal to the restatement -----------------------------------------------------------
@pytest.mark.parametrize("pair", sorted(I.PAIRS))
@pytest.mark.parametrize("w,h", I.SIZES)
def test_bytes_equal_the_restatement(dev, w, h, pair):
    got, *_ = run(dev, w, h, I.synthetic(w, h, pair)[:3], I.PAIRS[pair], I.params("defaults"))
    same_records(got, I.reference(w, h, pair)[0], f"{w}x{h}, {pair}")


@pytest.mark.parametrize("variant", [v for v in sorted(I.VARIANTS) if v != "defaults"])
@pytest.mark.parametrize("pair", ["shift", "yaw"])
def test_parameter_variants_equal_the_restatement(dev, pair, variant):
    w, h = 131, 77
    got, *_ = run(dev, w, h, I.synthetic(w, h, pair)[:3], I.PAIRS[pair], I.params(variant))
    same_records(got, I.reference(w, h, pair, variant)[0], f"{pair}, {variant}")


@pytest.mark.parametrize("mode", sorted(MODES))
def test_every_math_mode_gives_the_same_bytes(dev, mode):
    dev.k.set_math_mode(MODES[mode])
    try:
        for (w, h), pair in (((131, 77), "shift"), ((131, 77), "yaw"), ((61, 7), "forward"), ((5, 3), "same")):
            got, *_ = run(dev, w, h, I.synthetic(w, h, pair)[:3], I.PAIRS[pair], I.params("defaults"))
            same_records(got, I.reference(w, h, pair)[0], f"{mode}, {w}x{h}, {pair}")
    finally:
        dev.k.set_math_mode(N.MATH_PINNED)


def test_the_reference_reaches_both_outcomes():
    """Asserted on the restatement: on 131 x 77, "shift" and "yaw" carry some covered pixels and lose others."""
    for pair in ("shift", "yaw"):
        covered = I.synthetic(131, 77, pair)[2]["coverage"] > 0
        carried = int(I.reference(131, 77, pair)[1]["carried"].sum())
        assert 0 < carried < int(covered.sum()), (pair, carried, int(covered.sum()))


# ---- 2: buffers ----------------------------------------------------------------------------------
def test_inputs_untouched_tail_untouched_repeatable_and_aliased_inputs(dev):
    w, h = 131, 77
    arrays = I.synthetic(w, h, "shift")[:3]
    nbytes, tail = arrays[0].nbytes, 4096
    ob = dev.buffer(nbytes + tail, np.full(nbytes + tail, I.NAN_BYTE, np.uint8))
    got, bufs, _ = run(dev, w, h, arrays, I.PAIRS["shift"], I.params("defaults"), out=ob)
    same_records(got, I.reference(w, h, "shift")[0], "oversized out_stats")
    raw = dev.read(ob, nbytes + tail, np.uint8)
    assert (raw[nbytes:] == I.NAN_BYTE).all()
    for b, a in zip(bufs, arrays):
        assert dev.read(b, a.shape, a.dtype).tobytes() == a.tobytes()
    # the same call again, into the same buffer
    dev.ctx.ReprojectSamples(dev.k, bufs[0], bufs[1], bufs[2], w, h, ob, I.PAIRS["shift"], I.PREV, **I.params("defaults"))
    assert dev.read(ob, nbytes + tail, np.uint8).tobytes() == raw.tobytes()
    # inputs may alias one another: one feature buffer for both views, at one camera
    hs, hf = arrays[0], arrays[1]
    o2 = dev.buffer(nbytes)
    dev.ctx.ReprojectSamples(dev.k, bufs[0], bufs[1], bufs[1], w, h, o2, I.PREV, I.PREV, **I.params("cap"))
    want = ref.reproject(hs, hf, hf, w, h, I.PREV, I.PREV, **I.params("cap"))
    same_records(dev.read(o2, (h, w), ref.STATS), want, "aliased feature buffers")


# ---- 3: non-finite rows (defined behaviour; after the finite ones) ---------------------------------
def test_non_finite_rows_equal_the_restatement(dev):
    w, h, hs, hf, cf, view, dead, nan_n = I.non_finite_inputs()
    assert dead.any() and nan_n.any() and np.isnan(hs["n"][dead]).any()
    assert not np.isfinite(cf["depth"]).all() and not np.isfinite(hf["depth"]).all() and np.isnan(cf["coverage"]).any()
    want, info = ref.reproject(hs, hf, cf, w, h, view, I.PREV, **I.DEFAULTS, details=True)
    assert info["carried"].any() and not info["carried"].all() and info["rejected"]["count"] > 0
    for name in ("sum", "n", "mean_y", "m2_y"):
        assert np.isfinite(want[name]).all(), name          # nothing non-finite came through the arithmetic
    got, *_ = run(dev, w, h, (hs, hf, cf), view, I.DEFAULTS)
    same_records(got, want, "non-finite depths, coverages and unused statistics")


# ---- 4: ordering ---------------------------------------------------------------------------------
def test_ordered_between_a_write_and_a_read(dev):
    """WriteBuffer(hist_stats), ReprojectSamples, ReadBuffer(out_stats) without a Finish in between, against the same
    steps with a Finish after each on fresh buffers."""
    w, h = 131, 77
    hs, hf, cf, view = I.synthetic(w, h, "shift")
    results = []
    for finish in (False, True):
        hb = dev.buffer(hs.nbytes, np.zeros_like(hs))
        fb, cb, ob = dev.buffer(hf.nbytes, hf), dev.buffer(cf.nbytes, cf), dev.buffer(hs.nbytes, np.zeros_like(hs))
        dev.ctx.Finish()
        dev.ctx.WriteBuffer(hb, hs, blocking=False)
        if finish:
            dev.ctx.Finish()
        dev.ctx.ReprojectSamples(dev.k, hb, fb, cb, w, h, ob, view, I.PREV, **I.DEFAULTS)
        if finish:
            dev.ctx.Finish()
        out = np.empty((h, w), ref.STATS)
        dev.ctx.ReadBuffer(ob, out, blocking=False)
        dev.ctx.Finish()
        results.append(out)
    assert results[0].tobytes() == results[1].tobytes()
    same_records(results[0], I.reference(w, h, "shift")[0], "behind a queued write")


def test_ordered_before_accumulation_and_selection(dev):
    """ReprojectSamples, AccumulateSamples into out_stats, SelectPixels on it, without a Finish in between, against
    the same steps with a Finish after each on fresh buffers -- and against the restatements."""
    w, h = 131, 77
    hs, hf, cf, view = I.synthetic(w, h, "yaw")
    rng = np.random.default_rng(5)
    samples = np.zeros(w * h, adaptive_ref.RESULT)
    samples["radiance"] = (rng.random((w * h, 3)) * 2).astype(F)
    # (a wide threshold: the seeded statistics are noisy, and the selection is to take some pixels and leave others)
    sel = dict(threshold=0.7, floor_y=0.01, min_samples=2, max_samples=64, radius=1)
    results = []
    for finish in (False, True):
        hb, fb, cb = (dev.buffer(a.nbytes, a) for a in (hs, hf, cf))
        ob, rb = dev.buffer(hs.nbytes, np.zeros_like(hs)), dev.buffer(samples.nbytes, samples)
        ib = dev.buffer(w * h * 4, np.full(w * h, 0xFFFFFFFF, np.uint32))
        sb = dev.buffer(16, np.zeros(4, np.uint32))
        dev.ctx.Finish()
        dev.ctx.ReprojectSamples(dev.k, hb, fb, cb, w, h, ob, view, I.PREV, **I.DEFAULTS)
        if finish:
            dev.ctx.Finish()
        dev.ctx.AccumulateSamples(dev.k, None, rb, w * h, w * h, ob)
        if finish:
            dev.ctx.Finish()
        dev.ctx.SelectPixels(dev.k, ob, w, h, ib, sb, **sel)
        if finish:
            dev.ctx.Finish()
        results.append((dev.read(ob, (h, w), ref.STATS), dev.read(ib, w * h, np.uint32), dev.read(sb, 4, np.uint32)))
    for a, b in zip(*results):
        assert a.tobytes() == b.tobytes()
    stats, ids, res = results[0]
    want = adaptive_ref.accumulate(I.reference(w, h, "yaw")[0].reshape(-1), None, samples, 0, w * h, w * h)
    same_records(stats, want, "reprojected, then one sample each")
    want_ids, hot = adaptive_ref.select(want, w, h, **sel)
    assert 0 < len(want_ids) < w * h and list(res[:2]) == [len(want_ids), hot]
    assert np.array_equal(ids[:len(want_ids)], want_ids) and (ids[len(want_ids):] == 0xFFFFFFFF).all()


# ---- 5: timing and errors ------------------------------------------------------------------------
def test_timing_counts_the_call_as_one_launch(dev):
    w, h = 131, 77
    dev.k.set_timing(True)
    try:
        dev.k.reset_stats()
        before = dev.k.stats()
        got, *_ = run(dev, w, h, I.synthetic(w, h, "yaw")[:3], I.PAIRS["yaw"], I.params("defaults"))
        after = dev.k.stats()
        assert after["launches"] == before["launches"] + 1 and after["kernel_ms"] > before["kernel_ms"]
        same_records(got, I.reference(w, h, "yaw")[0], "with timing on")
    finally:
        dev.k.set_timing(False)


def test_errors_launch_nothing(dev):
    import clrt
    w, h = 61, 7
    hs, hf, cf, view = I.synthetic(w, h, "shift")
    other = Device()
    try:
        lib, ctx, k = dev.ctx._lib, dev.ctx.handle, dev.k.handle
        hb, fb, cb = (dev.buffer(a.nbytes, a) for a in (hs, hf, cf))
        sentinel = np.full(hs.nbytes, I.NAN_BYTE, np.uint8)
        ob = dev.buffer(sentinel.nbytes, sentinel)
        small = dev.buffer(hs.nbytes - 32)
        foreign = other.buffer(hs.nbytes)

        def vw(v):
            return N.VIEW(*((ctypes.c_float * 3)(*part) for part in v))

        def prm(**kw):
            p = {**I.DEFAULTS, "cur": view, "prev": I.PREV, **kw}
            return N.REPROJECT_PARAMS(vw(p["cur"]), vw(p["prev"]), p["max_history"], p["depth_tolerance"],
                                      p["normal_threshold"])

        def rc(kernel, s, g, f, ww, hh, p, o):
            hd = [b.handle if b else None for b in (s, g, f, o)]
            return lib.rtEnqueueReprojectSamples(ctx, kernel, hd[0], hd[1], hd[2], ww, hh,
                                                 None if p is None else ctypes.byref(p), hd[3])

        ok = prm()
        nan, inf = float("nan"), float("inf")
        dev.k.set_timing(True)
        dev.k.reset_stats()
        assert rc(None, hb, fb, cb, w, h, ok, ob) == -48 and rc(other.k.handle, hb, fb, cb, w, h, ok, ob) == -48
        assert rc(k, hb, fb, cb, w, h, None, ob) == -30
        assert rc(k, hb, fb, cb, 0, h, ok, ob) == -30 and rc(k, hb, fb, cb, w, 0, ok, ob) == -30
        assert rc(k, hb, fb, cb, 65536, 32769, ok, ob) == -30
        assert rc(k, hb, fb, cb, w, h, prm(cur=((0.0, nan, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))), ob) == -30
        assert rc(k, hb, fb, cb, w, h, prm(prev=(I.PREV[0], (0.0, inf, 0.0), I.PREV[2])), ob) == -30
        for key, values in (("max_history", (nan, inf, 0.0, 0.5, 3.5, -4.0, 2.0 ** 20 + 1)),
                            ("depth_tolerance", (nan, -0.1, 1.5)), ("normal_threshold", (nan, -1.5, 1.5))):
            for bad in values:
                assert rc(k, hb, fb, cb, w, h, prm(**{key: bad}), ob) == -30, (key, bad)
        assert rc(k, None, None, None, w, h, prm(max_history=0.0), None) == -30         # ... checked before the buffers
        assert rc(k, None, fb, cb, w, h, ok, ob) == -38 and rc(k, hb, None, cb, w, h, ok, ob) == -38
        assert rc(k, hb, fb, None, w, h, ok, ob) == -38 and rc(k, hb, fb, cb, w, h, ok, None) == -38
        for at in range(4):
            handles = [hb, fb, cb, ob]
            handles[at] = foreign
            assert rc(k, *handles[:3], w, h, ok, handles[3]) == -38, at                    # another context's buffer
        for same in (hb, fb, cb):
            assert rc(k, hb, fb, cb, w, h, ok, same) == -38                                # out_stats is an input
        assert rc(k, hb, fb, cb, w + 1, h, ok, hb) == -38                                  # ... checked before the sizes
        assert rc(k, small, fb, cb, w, h, ok, ob) == -61 and rc(k, hb, small, cb, w, h, ok, ob) == -61
        assert rc(k, hb, fb, small, w, h, ok, ob) == -61 and rc(k, hb, fb, cb, w, h, ok, small) == -61
        assert rc(k, hb, fb, cb, w, h + 1, ok, ob) == -61
        assert dev.k.stats()["launches"] == 0
        assert (dev.read(ob, hs.nbytes, np.uint8) == I.NAN_BYTE).all()                     # nothing was launched
        with pytest.raises(clrt.RTError):
            dev.ctx.ReprojectSamples(dev.k, hb, fb, cb, w, h, hb, view, I.PREV)
        # the kernel that saw every error still works
        assert rc(k, hb, fb, cb, w, h, ok, ob) == 0
        same_records(dev.read(ob, (h, w), ref.STATS), I.reference(w, h, "shift")[0], "after the errors")
        assert dev.k.stats()["launches"] == 1
    finally:
        dev.k.set_timing(False)
        other.close()


# ---- 6: the whole pipeline -----------------------------------------------------------------------
def test_raytracer_reproject_samples_keeps_what_the_move_leaves(cornell):
    """A few adaptive rounds on the Cornell box, the camera moved by (0.37, 0, 0.1), reproject_samples(): the
    statistics equal the restatement's on the read-back inputs, the next selection is adaptive_ref's on them and
    smaller than the one after reset_samples(), which is the whole frame, and the disocclusions have no samples.
    Measured on an MI355X: 0.524 of the pixels carried, 1517 of 3072 selected after the move."""
    import clrt
    W, H = 64, 48
    adaptive = dict(threshold=0.2, floor_y=0.01, min_samples=2, max_samples=6, radius=1)
    rt = clrt.Raytracer(W, H)
    rt.Init()
    try:
        rt.upload_scene(cornell)
        _, info = rt.render_adaptive(6, **adaptive)
        assert info["rounds"] >= 2 and rt.frame_count == 1
        old = rt.sample_stats()
        assert (old["n"] >= 2).all()
        prev = rt.camera
        feat0 = rt.features(4)
        p = prev.position
        rt.camera = clrt.renderer.Camera(position=(p[0] + 0.37, p[1], p[2] + 0.1))
        feat1 = rt.features(4)
        sample_frame = rt._sample_frame
        rt.reproject_samples(prev)
        assert rt.frame_count == 1 and rt._sample_frame == sample_frame and rt.camera.position[0] == p[0] + 0.37
        got = rt.sample_stats()
        view0, view1 = ((c.position, c.front, c.up) for c in (prev, rt.camera))
        want, details = ref.reproject(old, feat0, feat1, W, H, view1, view0, 16.0, 0.05, 0.9, details=True)
        same_records(got, want, "Raytracer.reproject_samples after a move")
        covered = feat1["coverage"] > 0
        assert details["carried"][covered].mean() > 0.5 and (got["n"] == 0).any() and (got["n"] <= 6).all()
        assert (got["n"][covered] == 0).any()                      # disocclusions among the covered pixels
        assert rt.features(4).tobytes() == feat1.tobytes()         # the camera's uniforms are the new camera's again

        picked = []

        def on_sample(rnd, frame, n, buffers):
            ids = np.empty(n, np.uint32)
            rt.ctx.ReadBuffer(buffers["ids"], ids, blocking=True)
            picked.append((frame, ids))

        _, info = rt.render_adaptive(1, on_sample=on_sample, **adaptive)
        want_ids, hot = adaptive_ref.select(want, W, H, **adaptive)
        assert (info["selected"], info["hot"]) == (len(want_ids), hot) and len(picked) == 1
        assert picked[0][0] == sample_frame and np.array_equal(picked[0][1], want_ids)   # fresh seeds: the frames go on
        assert set(np.flatnonzero(got["n"].reshape(-1) == 0)) <= set(want_ids.tolist())

        rt.reset_samples()
        _, info_reset = rt.render_adaptive(1, **adaptive)
        assert info_reset["selected"] == W * H and 0 < len(want_ids) < W * H
        print(f"reproject_samples: {details['carried'].mean():.3f} of the pixels carried, "
              f"{len(want_ids)} of {W * H} selected after the move")
    finally:
        rt.release()

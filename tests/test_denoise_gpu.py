"""GPU: the feature-guided a-trous denoiser (rtEnqueueDenoise, Raytracer.denoise).

The reference is tests/denoise_ref.py, the numpy float32 restatement of the filter's definition (checked on
the CPU in test_denoise_plan.py): the device's bytes must equal its bytes.

Inputs are seeded and synthetic, made once per size and shared (never modified): colours in [0, 2), albedo
from {0.25, 0.5, 0.75} in 4 x 4 blocks, normals jittered around +z, depth 20 .. 22, about 20 % of the pixels
uncovered.  The sizes (w x h): 1 x 1; 5 x 3, smaller than one tile; 61 x 7, a partial tile; 131 x 77, three
tiles across with partial ones at both edges and several rows per residue class at step 16; 40 x 200, many
tiles down one column; at 5 x 3 and 61 x 7 the later steps are larger than the image.
"""
import ctypes
import functools

import numpy as np
import pytest

import denoise_ref
from clrt import _native as N

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 3), (61, 7), (131, 77), (40, 200)]
DEFAULTS = (4.0, 0.5, 0.1, 0.25)
ALONE = {"color": (4.0, 0, 0, 0), "normal": (0, 0.5, 0, 0), "depth": (0, 0, 0.1, 0), "albedo": (0, 0, 0, 0.25)}
NAN_BYTE = 0xFF


@functools.lru_cache(maxsize=None)
def synthetic(w, h):
    """(image (h, w, 4) float32, features (h, w) N.PIXEL_FEATURES_DTYPE); read-only."""
    rng = np.random.default_rng(1000 * w + h)
    img = (rng.random((h, w, 4)) * 2).astype(np.float32)
    f = np.zeros((h, w), N.PIXEL_FEATURES_DTYPE)
    blocks = rng.choice(np.float32([0.25, 0.5, 0.75]), ((h + 3) // 4, (w + 3) // 4, 3))
    f["albedo"] = np.repeat(np.repeat(blocks, 4, axis=0), 4, axis=1)[:h, :w]
    n = np.concatenate([rng.normal(0, 0.15, (h, w, 2)), np.ones((h, w, 1))], axis=2)
    f["normal"] = (n / np.linalg.norm(n, axis=2, keepdims=True)).astype(np.float32)
    f["depth"] = rng.uniform(20, 22, (h, w)).astype(np.float32)
    cov = rng.integers(1, 9, (h, w)).astype(np.float32) / np.float32(8)
    cov[rng.random((h, w)) < 0.2] = 0
    if w * h == 1:
        cov[:] = 1
    f["coverage"] = cov
    img.setflags(write=False)
    f.setflags(write=False)
    return img, f


@functools.lru_cache(maxsize=None)
def reference(w, h, iterations, sigmas=DEFAULTS):
    img, f = synthetic(w, h)
    out = denoise_ref.denoise(img, f, w, h, iterations, *sigmas)
    out.setflags(write=False)
    return out


class Device:
    """A context and a kernel with nothing bound (the denoiser needs no scene), and buffers on demand."""

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

    def denoise(self, w, h, iterations, sigmas=DEFAULTS, out=None):
        img, f = synthetic(w, h)
        ib, fb = self.buffer(img.nbytes, img), self.buffer(f.nbytes, f)
        ob = out if out is not None else self.buffer(img.nbytes)
        self.ctx.Denoise(self.k, ib, fb, w, h, ob, iterations, *sigmas)
        return self.read(ob, (h, w, 4), np.float32), ib, fb, ob

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


# ---- 1: bytes equal to the restatement -----------------------------------------------------------
@pytest.mark.parametrize("w,h", [s for s in SIZES if s != (1, 1)])
def test_inputs_are_not_trivial(w, h):
    """Before anything is compared: the filter does something on these inputs, and its weights matter."""
    img, f = synthetic(w, h)
    covered = f["coverage"] != 0
    assert 0.1 < 1 - covered.mean() < 0.35 or w * h < 100
    one, five = reference(w, h, 1), reference(w, h, 5)
    changed = (one[..., :3] != img[..., :3]).any(axis=2)
    assert changed[covered].mean() >= 0.25 and not changed[~covered].any()
    assert (one != five).any()
    blur = reference(w, h, 1, (0.0, 0.0, 0.0, 0.0))
    frac = ((one[..., :3] != blur[..., :3]).any(axis=2) & changed)[covered]
    assert frac.mean() >= 0.25 or w * h < 100 and frac.any()     # fractional weights: neither input nor plain blur
    assert np.array_equal(one[..., 3], img[..., 3]) and np.array_equal(five[..., 3], img[..., 3])


@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("w,h", SIZES)
def test_bytes_equal_the_restatement(dev, w, h, iterations):
    got, *_ = dev.denoise(w, h, iterations)
    same_bytes(got, reference(w, h, iterations), f"{w}x{h}, {iterations} iterations")


@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("term", sorted(ALONE))
def test_each_term_alone_equals_the_restatement(dev, term, iterations):
    w, h = 131, 77
    want = reference(w, h, iterations, ALONE[term])
    assert (want != reference(w, h, iterations, (0.0, 0.0, 0.0, 0.0))).any()      # the term does something
    assert (want != reference(w, h, iterations)).any()
    got, *_ = dev.denoise(w, h, iterations, ALONE[term])
    same_bytes(got, want, f"{term} alone, {iterations} iterations")


def test_no_term_at_all_is_the_plain_blur(dev):
    got, *_ = dev.denoise(131, 77, 3, (0.0, 0.0, 0.0, 0.0))
    same_bytes(got, reference(131, 77, 3, (0.0, 0.0, 0.0, 0.0)), "every sigma 0")


# ---- 2: buffers and scratch ----------------------------------------------------------------------
def test_inputs_untouched_tail_untouched_and_repeatable(dev):
    w, h = 131, 77
    img, f = synthetic(w, h)
    tail = 4096
    ob = dev.buffer(img.nbytes + tail, np.full(img.nbytes + tail, NAN_BYTE, np.uint8))
    for iterations in (1, 4):
        got, ib, fb, _ = dev.denoise(w, h, iterations, out=ob)
        same_bytes(got, reference(w, h, iterations), f"oversized out, {iterations} iterations")
        raw = dev.read(ob, img.nbytes + tail, np.uint8)
        assert (raw[img.nbytes:] == NAN_BYTE).all()
        assert dev.read(ib, img.shape, np.float32).tobytes() == img.tobytes()
        assert dev.read(fb, f.shape, f.dtype).tobytes() == f.tobytes()
        # the same call again, into the same buffer
        dev.ctx.Denoise(dev.k, ib, fb, w, h, ob, iterations, *DEFAULTS)
        assert dev.read(ob, img.nbytes + tail, np.uint8).tobytes() == raw.tobytes()


def test_scratch_is_reused_by_a_smaller_call():
    d = Device()                          # a kernel of its own: its scratch starts empty
    try:
        for w, h in ((61, 7), (131, 77), (5, 3), (40, 200), (131, 77)):    # grow, grow, reuse, reuse, reuse
            got, *_ = d.denoise(w, h, 5)
            same_bytes(got, reference(w, h, 5), f"{w}x{h} after the calls before it")
    finally:
        d.close()


# ---- 3: the whole pipeline -----------------------------------------------------------------------
@pytest.mark.parametrize("math_name", ["pinned", "shipped"])
def test_raytracer_denoise_equals_the_restatement_and_lowers_the_error(cornell, math_name):
    import clrt
    W, H, FRAMES, LONG = 128, 72, 8, 256
    rt = clrt.Raytracer(W, H)
    rt.Init()
    try:
        rt.upload_scene(cornell)
        rt.kernel.set_math_mode({"pinned": N.MATH_PINNED, "shipped": N.MATH_SHIPPED}[math_name])
        assert rt.light_bounces == 9
        for _ in range(FRAMES):
            rt.RenderFrame()
        noisy = rt.pixels.reshape(H, W, 4).copy()
        den = rt.denoise()
        assert den.shape == (H, W, 4) and den.dtype == np.float32 and rt.frame_count == FRAMES + 1
        # the accumulation buffer is untouched, and the guides are those of frames 1 .. 8
        out = np.empty((H, W, 4), np.float32)
        rt.ctx.ReadBuffer(rt.output, out, blocking=True)
        assert out.tobytes() == noisy.tobytes()
        at, rt.frame_count = rt.frame_count, 1
        feat = rt.features(FRAMES)
        rt.frame_count = at
        covered = feat["coverage"] != 0
        assert 0.3 < covered.mean() and (feat["coverage"][covered] <= 1).all()
        same_bytes(den, denoise_ref.denoise(noisy, feat, W, H), f"Raytracer.denoise, {math_name}")
        same_bytes(rt.denoise(FRAMES, 2, 1.0, 0.0, 0.2, 0.5), denoise_ref.denoise(noisy, feat, W, H, 2, 1.0, 0.0, 0.2, 0.5),
                   "other parameters")
        # the progressive render goes on from where it was: frames 9 .. 256 into the same buffer
        rt.set_uniforms()
        rt.ctx.ExecuteKernelFrames(rt.kernel, W * H, LONG - FRAMES)
        rt.ctx.ReadBuffer(rt.output, out, blocking=True)
        truth = out[..., :3].astype(np.float64)
        assert (out[..., :3] != noisy[..., :3]).any()
        mse_noisy = ((noisy[..., :3] - truth) ** 2)[covered].mean()
        mse_den = ((den[..., :3] - truth) ** 2)[covered].mean()
        ratio = mse_den / mse_noisy
        print(f"denoise {math_name}: mse {mse_noisy:.6g} -> {mse_den:.6g}, ratio {ratio:.4f}")
        assert ratio < 0.75, ratio
    finally:
        rt.release()


# ---- 4: ordering ---------------------------------------------------------------------------------
def test_denoise_is_ordered_behind_queued_frames_and_features(cornell):
    from test_ray_query import Rig
    W, H = 128, 72
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
            g.ctx.Denoise(g.k, g.r.out, fb, W, H, ob, 3)
            results.append((g.read(ob, (H, W, 4), np.float32), g.r.result().reshape(H, W, 4),
                            g.read(fb, (H, W), N.PIXEL_FEATURES_DTYPE)))
        finally:
            g.close()
    (a, img_a, feat_a), (b, img_b, feat_b) = results
    assert img_a[..., :3].any() and img_a.tobytes() == img_b.tobytes() and feat_a.tobytes() == feat_b.tobytes()
    assert a.tobytes() == b.tobytes()
    same_bytes(a, denoise_ref.denoise(img_a, feat_a, W, H, 3), "behind four queued frames and their features")


# ---- 5: timing and errors ------------------------------------------------------------------------
def test_timing_counts_the_call_as_one_launch(dev):
    w, h = 131, 77
    dev.k.set_timing(True)
    try:
        dev.k.reset_stats()
        before = dev.k.stats()
        got, *_ = dev.denoise(w, h, 5)
        after = dev.k.stats()
        assert after["launches"] == before["launches"] + 1 and after["kernel_ms"] > before["kernel_ms"]
        same_bytes(got, reference(w, h, 5), "with timing on")
    finally:
        dev.k.set_timing(False)


def test_errors_launch_nothing(dev):
    import clrt
    w, h = 61, 7
    img, f = synthetic(w, h)
    other = Device()
    try:
        lib, ctx, k = dev.ctx._lib, dev.ctx.handle, dev.k.handle
        ib, fb = dev.buffer(img.nbytes, img), dev.buffer(f.nbytes, f)
        sentinel = np.full(img.nbytes, NAN_BYTE, np.uint8)
        ob = dev.buffer(sentinel.nbytes, sentinel)
        small = dev.buffer(img.nbytes - 16)
        foreign = other.buffer(img.nbytes)

        def rc(kernel, i, fe, ww, hh, params, o):
            p = None if params is None else ctypes.byref(N.DENOISE_PARAMS(*params))
            return lib.rtEnqueueDenoise(ctx, kernel, i.handle if i else None, fe.handle if fe else None, ww, hh, p,
                                        o.handle if o else None)

        ok = (3,) + DEFAULTS
        dev.k.set_timing(True)
        dev.k.reset_stats()
        assert rc(None, ib, fb, w, h, ok, ob) == -48 and rc(other.k.handle, ib, fb, w, h, ok, ob) == -48
        assert rc(k, ib, fb, w, h, None, ob) == -30
        assert rc(k, ib, fb, w, h, (0,) + DEFAULTS, ob) == -30 and rc(k, ib, fb, w, h, (6,) + DEFAULTS, ob) == -30
        for bad in (-1.0, float("nan"), float("inf"), 2.0 ** -21, 2.0 ** 21):
            for slot in range(4):
                s = list(DEFAULTS)
                s[slot] = bad
                assert rc(k, ib, fb, w, h, (3, *s), ob) == -30, (bad, slot)
        assert rc(k, ib, fb, 0, h, ok, ob) == -30 and rc(k, ib, fb, w, 0, ok, ob) == -30
        assert rc(k, ib, fb, 65536, 32769, ok, ob) == -30
        assert rc(k, None, None, w, h, (0,) + DEFAULTS, None) == -30            # ... checked before the buffers
        assert rc(k, None, fb, w, h, ok, ob) == -38 and rc(k, ib, None, w, h, ok, ob) == -38
        assert rc(k, ib, fb, w, h, ok, None) == -38 and rc(k, ib, fb, w, h, ok, foreign) == -38
        assert rc(k, ib, fb, w, h, ok, ib) == -38 and rc(k, ib, fb, w, h, ok, fb) == -38   # out is an input
        assert rc(k, ib, fb, w + 1, h, ok, ib) == -38                           # ... checked before the sizes
        assert rc(k, ib, fb, w, h, ok, small) == -61 and rc(k, small, fb, w, h, ok, ob) == -61
        assert rc(k, ib, small, w, h, ok, ob) == -61 and rc(k, ib, fb, w, h + 1, ok, ob) == -61
        assert dev.k.stats()["launches"] == 0
        assert (dev.read(ob, img.nbytes, np.uint8) == NAN_BYTE).all()            # nothing was launched
        with pytest.raises(clrt.RTError):
            dev.ctx.Denoise(dev.k, ib, fb, w, h, ib)
        # the kernel that saw every error still works
        assert rc(k, ib, fb, w, h, ok, ob) == 0
        same_bytes(dev.read(ob, (h, w, 4), np.float32), reference(w, h, 3), "after the errors")
        assert dev.k.stats()["launches"] == 1
    finally:
        dev.k.set_timing(False)
        other.close()

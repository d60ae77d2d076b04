"""GPU: the variance-guided denoiser over the adaptive sample statistics (rtEnqueueDenoiseSamples,
Raytracer.denoise_adaptive).

The reference is tests/denoise_samples_ref.py, the numpy float32 restatement of the filter's definition (checked
on the CPU in test_denoise_samples_plan.py, also against the text the kernel compiles): the device's bytes must
equal its bytes, `out` and `variance` alike.

Inputs are denoise_samples_ref.synthetic's: seeded, made once per size and shared (never modified) -- sample
counts from {0, 1, 2, 5, 40, 3000}, about 20 % of the pixels uncovered, about 3 % of the records with a negative
or a NaN m2_y.  The sizes (w x h): 1 x 1; 5 x 3, smaller than one tile; 61 x 7, a partial tile; 131 x 77, three
tiles across with partial ones at both edges and several rows per residue class at step 16; 40 x 200, many
tiles down one column, more rows than a step-16 class tile.

A record whose m2_y is NaN never counts; its variance is carried, so the variance plane holds a NaN there.  IEEE
leaves a NaN's payload open, so there the comparison asks for a NaN; every other compared word is finite and
must be the reference's word.
"""
import ctypes
import functools

import numpy as np
import pytest

import denoise_samples_ref as R
from clrt import _native as N

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 3), (61, 7), (131, 77), (40, 200)]
DEFAULTS = (4.0, 0.5, 0.1, 0.25)
EPSILON = 1e-4
ALONE = {"luminance": (4.0, 0, 0, 0), "normal": (0, 0.5, 0, 0), "depth": (0, 0, 0.1, 0), "albedo": (0, 0, 0, 0.25)}
NONE = (0.0, 0.0, 0.0, 0.0)
ENCODINGS = {"linear": R.LINEAR, "gamma": R.GAMMA}
NAN_BYTE = 0xFF


@functools.lru_cache(maxsize=None)
def cells(w, h, iterations, sigmas=DEFAULTS):
    """The last iteration's {r, g, b, v} of the reference: computed once, shared by the encodings."""
    st, f = R.synthetic(w, h)
    c = R.filtered_cells(st, f, w, h, iterations, *sigmas, epsilon=EPSILON)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(w, h, iterations, sigmas=DEFAULTS, encoding=R.GAMMA):
    out, var = R.output(cells(w, h, iterations, sigmas), R.synthetic(w, h)[0], encoding)
    out.setflags(write=False)
    var.setflags(write=False)
    return out, var


class Device:
    """A context and a kernel with nothing bound (the denoiser needs no scene), and buffers on demand."""

    def __init__(self):
        import clrt
        self.ctx = clrt.CLContext(0)
        self.k = clrt.CLKernel(self.ctx, "KernelEntry")
        self._bufs, self._inputs = [], {}

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

    def inputs(self, w, h):
        """the synthetic statistics and features of a size on the device: uploaded once, only ever read"""
        if (w, h) not in self._inputs:
            st, f = R.synthetic(w, h)
            self._inputs[w, h] = (self.buffer(st.nbytes, st), self.buffer(f.nbytes, f))
        return self._inputs[w, h]

    def denoise(self, w, h, iterations, sigmas=DEFAULTS, encoding=R.GAMMA, out=None, variance=True):
        """(out (h, w, 4), variance (h, w) or None, the four buffers)"""
        sb, fb = self.inputs(w, h)
        ob = out if out is not None else self.buffer(w * h * 16)
        vb = None if variance is False else variance if variance is not True else self.buffer(w * h * 4)
        self.ctx.DenoiseSamples(self.k, sb, fb, w, h, ob, vb, iterations, *sigmas, EPSILON, encoding)
        var = self.read(vb, (h, w), np.float32) if vb is not None else None
        return self.read(ob, (h, w, 4), np.float32), var, (sb, fb, ob, vb)

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
    """Word for word; where the reference holds a NaN (see the module's text) the device must hold one."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaNs elsewhere"
    a, b = got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} words differ, first {got[~nan][bad[:4]]} vs {want[~nan][bad[:4]]}"


def check(got, var, w, h, iterations, sigmas, encoding, what):
    want, wvar = reference(w, h, iterations, sigmas, encoding)
    same_bytes(got, want, what + ": out")
    if var is not None:
        same_bytes(var, wvar, what + ": variance")


def near(mask, reach=2):
    """pixels with a pixel of `mask` among their 25 taps at step 1"""
    h, w = mask.shape
    p = np.pad(mask, reach)
    out = np.zeros((h, w), bool)
    for dy in range(2 * reach + 1):
        for dx in range(2 * reach + 1):
            out |= p[dy:dy + h, dx:dx + w]
    return out


# ---- 1: bytes equal to the restatement -----------------------------------------------------------
@pytest.mark.parametrize("w,h", [s for s in SIZES if s[0] * s[1] >= 400])
def test_inputs_are_not_trivial(w, h):
    """Before anything is compared, on the reference alone: the filter does something on these inputs, the
    luminance term matters, every counting rule rejects taps of ordinary centres, and what is compared is finite."""
    st, f = R.synthetic(w, h)
    c0 = R.stats_cells(st)
    counts = R.counting(c0, f["coverage"])
    assert 0.5 < counts.mean() < 0.9 and set(np.unique(st["n"])) == set(R.COUNTS)
    assert 0.1 < (f["coverage"] == 0).mean() < 0.3
    one, five = cells(w, h, 1), cells(w, h, 5)
    changed = (one[..., :3] != c0[..., :3]).any(axis=2)
    assert changed[counts].mean() > 0.5 and not changed[~counts].any()
    assert (one[counts] != five[counts]).any()
    plain = cells(w, h, 1, (0.0,) + DEFAULTS[1:])
    assert (one[..., :3] != plain[..., :3]).any(axis=2)[counts].mean() > 0.1      # the luminance term
    with np.errstate(invalid="ignore"):
        v = c0[..., 3]
        rejected = {"coverage": (f["coverage"] == 0) & (st["n"] >= 1) & (v >= 0),
                    "n < 1": (f["coverage"] != 0) & ~(st["n"] >= 1),
                    "negative variance": (f["coverage"] != 0) & (v < 0) & (st["n"] >= 2),
                    "NaN variance": (f["coverage"] != 0) & np.isnan(v)}
    for rule, mask in rejected.items():
        assert (near(mask) & counts).any(), rule
    for iterations in range(1, 6):
        for enc in ENCODINGS.values():
            out, var = reference(w, h, iterations, DEFAULTS, enc)
            assert np.isfinite(out).all() and np.isfinite(var[counts]).all()
            assert np.array_equal(np.isnan(var), np.isnan(v))       # carried by the records that hold one
            assert not np.isinf(var).any()


@pytest.mark.parametrize("encoding", sorted(ENCODINGS))
@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("w,h", SIZES)
def test_bytes_equal_the_restatement(dev, w, h, iterations, encoding):
    got, var, _ = dev.denoise(w, h, iterations, DEFAULTS, ENCODINGS[encoding])
    check(got, var, w, h, iterations, DEFAULTS, ENCODINGS[encoding], f"{w}x{h}, {iterations} iterations, {encoding}")


@pytest.mark.parametrize("iterations", [1, 3, 5])
@pytest.mark.parametrize("term", sorted(ALONE))
def test_each_term_alone_equals_the_restatement(dev, term, iterations):
    w, h = 131, 77
    want = cells(w, h, iterations, ALONE[term])
    assert (want != cells(w, h, iterations, NONE)).any() and (want != cells(w, h, iterations)).any()   # it does something
    got, var, _ = dev.denoise(w, h, iterations, ALONE[term], R.LINEAR)
    check(got, var, w, h, iterations, ALONE[term], R.LINEAR, f"{term} alone, {iterations} iterations")


def test_no_term_at_all_is_the_plain_blur(dev):
    got, var, _ = dev.denoise(131, 77, 3, NONE, R.LINEAR)
    check(got, var, 131, 77, 3, NONE, R.LINEAR, "every sigma 0")


@pytest.mark.parametrize("iterations", [1, 4])
def test_without_a_variance_buffer(dev, iterations):
    got, var, _ = dev.denoise(131, 77, iterations, variance=False)
    assert var is None
    check(got, None, 131, 77, iterations, DEFAULTS, R.GAMMA, "variance NULL")


# ---- 2: buffers and scratch ----------------------------------------------------------------------
def test_inputs_untouched_tails_untouched_and_repeatable(dev):
    w, h = 131, 77
    st, f = R.synthetic(w, h)
    px, tail = w * h, 4096
    ob = dev.buffer(px * 16 + tail, np.full(px * 16 + tail, NAN_BYTE, np.uint8))
    vb = dev.buffer(px * 4 + tail, np.full(px * 4 + tail, NAN_BYTE, np.uint8))
    for iterations in (1, 4):
        got, var, (sb, fb, _, _) = dev.denoise(w, h, iterations, out=ob, variance=vb)
        check(got, var, w, h, iterations, DEFAULTS, R.GAMMA, f"oversized buffers, {iterations} iterations")
        raw, vraw = dev.read(ob, px * 16 + tail, np.uint8), dev.read(vb, px * 4 + tail, np.uint8)
        assert (raw[px * 16:] == NAN_BYTE).all() and (vraw[px * 4:] == NAN_BYTE).all()
        assert dev.read(sb, st.shape, st.dtype).tobytes() == st.tobytes()
        assert dev.read(fb, f.shape, f.dtype).tobytes() == f.tobytes()
        # the same call again, into the same buffers
        dev.ctx.DenoiseSamples(dev.k, sb, fb, w, h, ob, vb, iterations, *DEFAULTS, EPSILON, R.GAMMA)
        assert dev.read(ob, px * 16 + tail, np.uint8).tobytes() == raw.tobytes()
        assert dev.read(vb, px * 4 + tail, np.uint8).tobytes() == vraw.tobytes()


def test_scratch_is_reused_after_a_larger_call_and_shared_with_the_image_filter():
    import denoise_ref
    d = Device()                          # a kernel of its own: its scratch starts empty
    try:
        for w, h in ((61, 7), (131, 77), (5, 3), (40, 200), (131, 77)):    # grow, grow, reuse, reuse, reuse
            got, var, (_, fb, ob, _) = d.denoise(w, h, 5)
            check(got, var, w, h, 5, DEFAULTS, R.GAMMA, f"{w}x{h} after the calls before it")
        # rtEnqueueDenoise ping-pongs through the same block: each still gives its own bytes after the other
        w, h = 131, 77
        img = d.read(ob, (h, w, 4), np.float32)
        ib, o2 = d.buffer(img.nbytes, img), d.buffer(img.nbytes)
        d.ctx.Denoise(d.k, ib, fb, w, h, o2, 4)
        want = denoise_ref.denoise(img, R.synthetic(w, h)[1], w, h, 4)
        assert d.read(o2, (h, w, 4), np.float32).tobytes() == want.tobytes()
        got, var, _ = d.denoise(w, h, 4)
        check(got, var, w, h, 4, DEFAULTS, R.GAMMA, "after rtEnqueueDenoise")
    finally:
        d.close()


# ---- 3: ordering ---------------------------------------------------------------------------------
def test_ordered_behind_coalesced_frames_and_a_queued_accumulation(cornell):
    """Per-frame launches that coalesce, then rtEnqueueAccumulateSamples of one more sample a pixel into the
    statistics, then the filter, with nothing waited for in between -- against the same calls with a Finish after
    each, and against the reference fed the statistics read back."""
    from test_ray_query import Rig
    W, H = 64, 36
    px = W * H
    st, f = R.synthetic(W, H)
    rng = np.random.default_rng(5)
    res = np.zeros(px, N.PATH_RESULT_DTYPE)
    res["radiance"] = (rng.random((px, 3)) * 2).astype(np.float32)
    results = []
    for finish in (False, True):
        g = Rig(cornell, W=W, H=H, perframe_batch=None)   # (the library default: frames coalesce)
        try:
            sb, fb, rb = g.buffer(st.nbytes, st), g.buffer(f.nbytes, f), g.buffer(res.nbytes, res)
            ob, vb = g.buffer(px * 16), g.buffer(px * 4)
            for frame in range(1, 4):
                g.r.frame(frame, light_bounces=2)
                if finish:
                    g.ctx.Finish()
            g.ctx.AccumulateSamples(g.k, None, rb, px, px, sb)
            if finish:
                g.ctx.Finish()
            g.ctx.DenoiseSamples(g.k, sb, fb, W, H, ob, vb, 3, *DEFAULTS, EPSILON, R.GAMMA)
            results.append((g.read(ob, (H, W, 4), np.float32), g.read(vb, (H, W), np.float32),
                            g.read(sb, (H, W), N.PIXEL_STATS_DTYPE), g.r.result().tobytes()))
        finally:
            g.close()
    (a, va, sa, ia), (b, vb_, sb_, ib) = results
    assert ia == ib and sa.tobytes() == sb_.tobytes() and sa.tobytes() != st.tobytes()
    assert np.array_equal(sa["n"], st["n"] + 1)
    assert a.tobytes() == b.tobytes() and va.tobytes() == vb_.tobytes()
    want, wvar = R.denoise_samples(sa, f, W, H, 3, *DEFAULTS, epsilon=EPSILON)
    same_bytes(a, want, "behind three queued frames and an accumulation: out")
    same_bytes(va, wvar, "behind three queued frames and an accumulation: variance")
    stale, _ = R.denoise_samples(st, f, W, H, 3, *DEFAULTS, epsilon=EPSILON)
    assert (stale != want).any()                           # ... which the statistics before the accumulation do not give


# ---- 4: timing and errors ------------------------------------------------------------------------
def test_timing_counts_the_call_as_one_launch(dev):
    w, h = 131, 77
    dev.k.set_timing(True)
    try:
        dev.k.reset_stats()
        before = dev.k.stats()
        got, var, _ = dev.denoise(w, h, 5)
        after = dev.k.stats()
        assert after["launches"] == before["launches"] + 1 and after["kernel_ms"] > before["kernel_ms"]
        check(got, var, w, h, 5, DEFAULTS, R.GAMMA, "with timing on")
    finally:
        dev.k.set_timing(False)


def test_errors_launch_nothing(dev):
    import clrt
    w, h = 61, 7
    px = w * h
    other = Device()
    try:
        lib, ctx, k = dev.ctx._lib, dev.ctx.handle, dev.k.handle
        sb, fb = dev.inputs(w, h)
        ob = dev.buffer(px * 16, np.full(px * 16, NAN_BYTE, np.uint8))
        vb = dev.buffer(px * 4, np.full(px * 4, NAN_BYTE, np.uint8))
        small32, small16, small4 = dev.buffer(px * 32 - 32), dev.buffer(px * 16 - 16), dev.buffer(px * 4 - 4)
        foreign = other.buffer(px * 32)

        def rc(kernel, s, fe, ww, hh, params, o, v):
            p = None if params is None else ctypes.byref(N.DENOISE_SAMPLES_PARAMS(*params))
            return lib.rtEnqueueDenoiseSamples(ctx, kernel, s.handle if s else None, fe.handle if fe else None, ww, hh, p,
                                               o.handle if o else None, v.handle if v else None)

        def params(iterations=3, sigmas=DEFAULTS, epsilon=EPSILON, encoding=R.GAMMA):
            return (iterations, *sigmas, epsilon, encoding)

        ok = params()
        dev.k.set_timing(True)
        dev.k.reset_stats()
        assert rc(None, sb, fb, w, h, ok, ob, vb) == -48 and rc(other.k.handle, sb, fb, w, h, ok, ob, vb) == -48
        # RT_INVALID_VALUE
        assert rc(k, sb, fb, w, h, None, ob, vb) == -30
        assert rc(k, sb, fb, w, h, params(0), ob, vb) == -30 and rc(k, sb, fb, w, h, params(6), ob, vb) == -30
        for bad in (-1.0, float("nan"), float("inf"), 2.0 ** -21, 2.0 ** 21):
            for slot in range(4):
                s = list(DEFAULTS)
                s[slot] = bad
                assert rc(k, sb, fb, w, h, params(sigmas=s), ob, vb) == -30, (bad, slot)
        for bad in (0.0, -1e-4, float("nan"), float("inf"), 2.0 ** -41, 2.0 ** 21):
            assert rc(k, sb, fb, w, h, params(epsilon=bad), ob, vb) == -30, bad
        assert rc(k, sb, fb, w, h, params(encoding=2), ob, vb) == -30
        assert rc(k, sb, fb, w, h, params(encoding=-1), ob, vb) == -30
        assert rc(k, sb, fb, 0, h, ok, ob, vb) == -30 and rc(k, sb, fb, w, 0, ok, ob, vb) == -30
        assert rc(k, sb, fb, 65536, 32769, ok, ob, vb) == -30
        assert rc(k, None, None, w, h, params(0), None, foreign) == -30          # ... checked before the buffers
        assert rc(k, None, None, w, h, params(epsilon=0.0), None, None) == -30
        # RT_INVALID_MEM_OBJECT
        assert rc(k, None, fb, w, h, ok, ob, vb) == -38 and rc(k, sb, None, w, h, ok, ob, vb) == -38
        assert rc(k, sb, fb, w, h, ok, None, vb) == -38
        assert rc(k, foreign, fb, w, h, ok, ob, vb) == -38 and rc(k, sb, foreign, w, h, ok, ob, vb) == -38
        assert rc(k, sb, fb, w, h, ok, foreign, vb) == -38 and rc(k, sb, fb, w, h, ok, ob, foreign) == -38
        assert rc(k, sb, fb, w, h, ok, sb, vb) == -38 and rc(k, sb, fb, w, h, ok, fb, vb) == -38     # out is an input
        assert rc(k, sb, fb, w, h, ok, ob, sb) == -38 and rc(k, sb, fb, w, h, ok, ob, fb) == -38     # variance is
        assert rc(k, sb, fb, w, h, ok, ob, ob) == -38                                                # ... or is out
        assert rc(k, sb, fb, w + 1, h, ok, sb, vb) == -38                        # ... checked before the sizes
        # RT_INVALID_BUFFER_SIZE
        assert rc(k, small32, fb, w, h, ok, ob, vb) == -61 and rc(k, sb, small32, w, h, ok, ob, vb) == -61
        assert rc(k, sb, fb, w, h, ok, small16, vb) == -61 and rc(k, sb, fb, w, h, ok, ob, small4) == -61
        assert rc(k, sb, fb, w, h + 1, ok, ob, vb) == -61 and rc(k, sb, fb, w, h + 1, ok, ob, None) == -61
        assert dev.k.stats()["launches"] == 0
        assert (dev.read(ob, px * 16, np.uint8) == NAN_BYTE).all()              # nothing was launched
        assert (dev.read(vb, px * 4, np.uint8) == NAN_BYTE).all()
        with pytest.raises(clrt.RTError):
            dev.ctx.DenoiseSamples(dev.k, sb, fb, w, h, sb)
        # the kernel that saw every error still works
        assert rc(k, sb, fb, w, h, ok, ob, vb) == 0
        check(dev.read(ob, (h, w, 4), np.float32), dev.read(vb, (h, w), np.float32), w, h, 3, DEFAULTS, R.GAMMA,
              "after the errors")
        assert dev.k.stats()["launches"] == 1
    finally:
        dev.k.set_timing(False)
        other.close()


# ---- 5: the whole pipeline -----------------------------------------------------------------------
# measured on an MI355X, pinned and shipped math alike: 0.3185 of the unfiltered error at the defaults (3
# iterations, sigma_luminance 8); the bound is the midpoint between that and 1
QUALITY_BOUND = 0.659


@pytest.mark.parametrize("math_name", ["pinned", "shipped"])
def test_denoise_adaptive_equals_the_restatement_and_lowers_the_error(cornell, math_name):
    """Cornell 128 x 72, 9 bounces: a few adaptive rounds from 4 samples a pixel, filtered, against 256 uniform
    samples a pixel taken at other sample frames; mean squared error in gamma space over the covered pixels."""
    import clrt
    W, H, ROUNDS, LONG = 128, 72, 6, 256
    rt = clrt.Raytracer(W, H)
    rt.Init()
    try:
        rt.upload_scene(cornell)
        rt.kernel.set_math_mode({"pinned": N.MATH_PINNED, "shipped": N.MATH_SHIPPED}[math_name])
        assert rt.light_bounces == 9
        rt.frame_count = 7
        noisy, info = rt.render_adaptive(ROUNDS, samples_per_round=4, min_samples=4, max_samples=32)
        frames = info["rounds"] * 4
        stats = rt.sample_stats()
        assert info["rounds"] >= 2 and stats["n"].min() == 4 and stats["n"].max() > 4      # the counts differ
        den, var = rt.denoise_adaptive(variance=True)
        assert den.shape == (H, W, 4) and den.dtype == np.float32 and var.shape == (H, W) and rt.frame_count == 7
        # the statistics are untouched, and the guides are those of the sample frames taken
        assert rt.sample_stats().tobytes() == stats.tobytes()
        at, rt.frame_count = rt.frame_count, 1
        feat = rt.features(frames)
        rt.frame_count = at
        covered = feat["coverage"] != 0
        assert 0.3 < covered.mean() and (feat["coverage"][covered] <= 1).all()
        want, wvar = R.denoise_samples(stats, feat, W, H)
        same_bytes(den, want, f"Raytracer.denoise_adaptive, {math_name}: out")
        same_bytes(var, wvar, f"Raytracer.denoise_adaptive, {math_name}: variance")
        assert np.array_equal(den[..., 3], stats["n"]) and np.isfinite(var).all()
        lin = rt.denoise_adaptive(frames, 2, 8.0, 0.0, 0.2, 0.5, 1e-3, "linear")
        same_bytes(lin, R.denoise_samples(stats, feat, W, H, 2, 8.0, 0.0, 0.2, 0.5, 1e-3, R.LINEAR)[0], "other parameters")
        # the truth: 256 samples a pixel at sample frames no sample above was taken at
        rt.reset_samples()
        rt._sample_frame = 4097
        truth, tinfo = rt.render_adaptive(4, samples_per_round=LONG // 4, min_samples=LONG, max_samples=LONG)
        assert tinfo["paths"] == LONG * W * H and (truth[..., 3] == LONG).all()
        truth = truth[..., :3].astype(np.float64)
        mse_noisy = ((noisy[..., :3] - truth) ** 2)[covered].mean()
        mse_den = ((den[..., :3] - truth) ** 2)[covered].mean()
        ratio = mse_den / mse_noisy
        print(f"denoise_adaptive {math_name}: mse {mse_noisy:.6g} -> {mse_den:.6g}, ratio {ratio:.4f}")
        assert ratio < QUALITY_BOUND, ratio
    finally:
        rt.release()

"""GPU: rtEnqueueSamplePixels -- one fused launch per adaptive sample -- against the three calls it replaces.

Every comparison is byte equality of the whole statistics buffer, two guard records past n_pixels included, with the
composed rtEnqueueCameraPathsFor -> rtEnqueueTracePaths (RT_TRACE_LINEAR, the seeds given) ->
rtEnqueueAccumulateSamples run on a copy of the same prior statistics.  The composed path is itself pinned to
tests/adaptive_ref.py and the oracle by test_adaptive_gpu.py and test_trace_paths.py.
"""
import ctypes

import numpy as np
import pytest

import adaptive_ref as R
from clrt import _native as N
from test_adaptive_gpu import AdaptRig, random_stats, raytracer
from test_ray_query import MATHS

pytestmark = pytest.mark.gpu

GUARD = 2          # statistics records past n_pixels: they keep their bytes
FIRST = 3


@pytest.fixture
def rigs():
    made = []

    def make(*a, **kw):
        made.append(AdaptRig(*a, **kw))
        return made[-1]

    yield make
    for g in made:
        g.close()


@pytest.fixture(scope="module")
def proxy():
    import clrt.proxy as P
    return P.bunny_proxy()


def make_ids(rng, px):
    """FIRST guard ids, a shuffled 80 % of the pixels with about 5 % replaced by ids out of range, five guard ids:
    the guards name pixels of the image that the range leaves out, so touching one would show."""
    tail = 5
    if px == 1:
        body = np.array([0, 1, 0xFFFFFFFF, 2, 0x80000000], np.uint32)
        guards = [0] * (FIRST + tail)          # (the one pixel: a guard read as a record would count twice)
    else:
        perm = rng.permutation(px).astype(np.uint32)
        n = max(1, int(px * 0.8))
        body = perm[:n].copy()
        guards = (perm[n:].tolist() * (FIRST + tail))[:FIRST + tail]
        out = np.flatnonzero(rng.random(n) < 0.05)
        body[out] = rng.choice(np.array([px, px + 1, px + 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], np.uint32), len(out))
        body[n // 2], body[n // 3], body[n // 5] = 0xFFFFFFFF, px, 0x80000000
    ids = np.concatenate([np.array(guards[:FIRST], np.uint32), body, np.array(guards[FIRST:], np.uint32)])
    return ids, len(body)


def composed(g, ib, n, px, sb, first=FIRST):
    """The reference: the three calls over records [first, first + n) of `ib`, into `sb`."""
    if n == 0:
        return
    m = first + n
    rb, sd, ob = g.buffer(m * 32), g.buffer(m * 4), g.buffer(m * 16)
    g.ctx.CameraPathsFor(g.k, ib, n, rb, sd, first=first)
    g.ctx.TracePaths(g.k, rb, ob, n, seeds=sd, first=first, encoding=N.TRACE_LINEAR)
    g.ctx.AccumulateSamples(g.k, ib, ob, n, px, sb, first=first)


def set_frame(g, frame, bounces=2, light_type=0):
    g.r.frame(frame, light_bounces=1)      # every slot, the camera's among them (one small render)
    g.lights(bounces, light_type)
    g.k.set_uint(N.FRAME_COUNT, frame)


def both(g, W, H, seed, bounces=2, light_type=0, frame=5):
    """(fused, composed, prior) statistics for the image size's id list."""
    px = W * H
    rng = np.random.default_rng(seed)
    st = random_stats(rng, px + GUARD)
    ids, n = make_ids(rng, px)
    set_frame(g, frame, bounces, light_type)
    ib = g.buffer(ids.nbytes, ids)
    s1, s2 = g.buffer(st.nbytes, st), g.buffer(st.nbytes, st)
    g.ctx.SamplePixels(g.k, ib, n, px, s1, first=FIRST)
    composed(g, ib, n, px, s2)
    got, want = g.read(s1, px + GUARD, R.STATS), g.read(s2, px + GUARD, R.STATS)
    assert g.read(ib, len(ids), np.uint32).tobytes() == ids.tobytes()        # ids is only read
    return got, want, st, ids[FIRST:FIRST + n]


def check(got, want, st, body, px):
    assert got.tobytes() == want.tobytes()
    assert want[px:].tobytes() == st[px:].tobytes()
    inside = body[body < px]
    assert (want["n"][inside] == st["n"][inside] + 1).all() and want.tobytes() != st.tobytes()
    untouched = np.setdiff1d(np.arange(px), inside)
    assert want[untouched].tobytes() == st[untouched].tobytes()
    assert px == 1 or ((body >= px).sum() >= 3 and len(untouched) > 0)


# ---- 1: shapes ------------------------------------------------------------------------------------
SIZES = [(1, 1), (61, 7), (131, 77)]      # 61 x 7: 341 records, five full units and one of 21; 131 x 77: 127 units
SIZE_IDS = [f"{w}x{h}" for w, h in SIZES]


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("config", ["lds", "global", "proxy"])
@pytest.mark.parametrize("math_name", list(MATHS))
def test_fused_sample_equals_the_three_calls(cornell, proxy, rigs, math_name, config, size):
    W, H = size
    scene = proxy if config == "proxy" else cornell
    g = rigs(scene, math=MATHS[math_name], force_global=config == "global", W=W, H=H)
    got, want, st, body = both(g, W, H, seed=W * H + len(config))
    check(got, want, st, body, W * H)
    assert g.k.scene_in_lds() == (config == "lds")


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("bounces", [0, 1, 9])
def test_bounce_counts_on_pinned_cornell(cornell, rigs, bounces, size):
    W, H = size
    g = rigs(cornell, math=N.MATH_PINNED, W=W, H=H)
    got, want, st, body = both(g, W, H, seed=31 * W + bounces, bounces=bounces)
    check(got, want, st, body, W * H)
    if bounces == 0:       # a zero sample: the counts move, the sums do not
        inside = body[body < W * H]
        assert want["sum"][inside].tobytes() == st["sum"][inside].tobytes()


@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("light_type", [0, 1, 2])
def test_light_types_on_pinned_cornell(cornell, rigs, light_type, size):
    W, H = size
    g = rigs(cornell, math=N.MATH_PINNED, W=W, H=H)
    got, want, st, body = both(g, W, H, seed=17 * W + light_type, light_type=light_type)
    check(got, want, st, body, W * H)


# ---- 2: a wave taking more than one unit -------------------------------------------------------------
def device_cus(g):
    """the compute units of the context's device, from the HIP runtime the library runs on"""
    dev, cus = ctypes.c_int(), ctypes.c_int()
    assert g.ctx._lib.rtContextGetDevice(g.ctx.handle, ctypes.byref(dev)) == 0
    hip = ctypes.CDLL("libamdhip64.so")
    assert hip.hipDeviceGetAttribute(ctypes.byref(cus), 63, dev) == 0     # hipDeviceAttributeMultiprocessorCount
    return cus.value


def test_a_wave_takes_more_than_one_unit(cornell, rigs):
    sizes = [(320, 240), (640, 480), (1280, 720)]
    g = rigs(cornell, math=N.MATH_SHIPPED, W=sizes[0][0], H=sizes[0][1])
    g.k.set_tuning("max_blocks", 1)
    assert g.k.get_tuning("max_blocks") == 1
    waves = 1 * device_cus(g) * 4           # one workgroup of four waves per compute unit
    W, H = next(s for s in sizes if (s[0] * s[1] + 63) // 64 > waves)
    if (W, H) != sizes[0]:
        g = rigs(cornell, math=N.MATH_SHIPPED, W=W, H=H)
        g.k.set_tuning("max_blocks", 1)
    px = W * H
    assert (px + 63) // 64 > waves
    rng = np.random.default_rng(px)
    st = random_stats(rng, px + GUARD)
    ids = np.arange(px, dtype=np.uint32)
    set_frame(g, 3)
    ib, s1, s2 = g.buffer(ids.nbytes, ids), g.buffer(st.nbytes, st), g.buffer(st.nbytes, st)
    g.ctx.SamplePixels(g.k, ib, px, px, s1)
    composed(g, ib, px, px, s2, first=0)
    got, want = g.read(s1, px + GUARD, R.STATS), g.read(s2, px + GUARD, R.STATS)
    assert got.tobytes() == want.tobytes()
    assert (want["n"][:px] == st["n"][:px] + 1).all() and want[px:].tobytes() == st[px:].tobytes()


# ---- 3: the device count ----------------------------------------------------------------------------
def test_the_count_is_read_on_the_device_and_clamped(cornell, rigs):
    W, H = 61, 7
    px = W * H
    g = rigs(cornell, math=N.MATH_SHIPPED, W=W, H=H)
    rng = np.random.default_rng(9)
    st = random_stats(rng, px + GUARD)
    ids, n = make_ids(rng, px)
    assert n > 65
    set_frame(g, 2)
    ib = g.buffer(ids.nbytes, ids)

    def run(nn, count=None):
        sb = g.buffer(st.nbytes, st)
        cb = None if count is None else g.buffer(16, np.array([count, 0xFFFFFFFF, 7, 0xDEADBEEF], np.uint32))
        g.ctx.SamplePixels(g.k, ib, nn, px, sb, count=cb, first=FIRST)
        out = g.read(sb, px + GUARD, R.STATS)
        if cb is not None:
            assert g.read(cb, 4, np.uint32).tolist() == [count, 0xFFFFFFFF, 7, 0xDEADBEEF]      # only read
        return out

    assert run(n, 0).tobytes() == st.tobytes()
    full = run(n)
    for c in (1, 63, 64, 65, n, n + 1000):
        m = min(c, n)
        got = run(n, c)
        assert got.tobytes() == (full if m == n else run(m)).tobytes(), c
        later = ids[FIRST + m:FIRST + n]
        later = np.setdiff1d(later[later < px], ids[FIRST:FIRST + m])
        assert got[later].tobytes() == st[later].tobytes(), c              # the records past m keep their bytes
        assert m == n or len(later) > 0
    assert full.tobytes() != st.tobytes() and run(1).tobytes() != st.tobytes()


def test_a_select_result_used_directly_equals_the_round_with_a_read(cornell, rigs):
    W, H = 61, 7
    px = W * H
    g = rigs(cornell, math=N.MATH_SHIPPED, W=W, H=H)
    rng = np.random.default_rng(4)
    st = random_stats(rng, px + GUARD)
    st["reserved"][px:] = 0
    params = dict(threshold=0.05, floor_y=0.01, min_samples=4, max_samples=32, radius=1)
    set_frame(g, 6)
    fill = np.full(px, 0xA5A5A5A5, np.uint32)
    # the queued round: nothing is read between the select and the sample
    s1, i1, r1 = g.buffer(st.nbytes, st), g.buffer(fill.nbytes, fill), g.buffer(16)
    g.ctx.SelectPixels(g.k, s1, W, H, i1, r1, **params)
    g.ctx.SamplePixels(g.k, i1, px, px, s1, count=r1)
    got = g.read(s1, px + GUARD, R.STATS)
    # the composed round, with the read
    s2, i2, r2 = g.buffer(st.nbytes, st), g.buffer(fill.nbytes, fill), g.buffer(16)
    sel = int(g.select(s2, W, H, i2, r2, **params)[0])
    assert 0 < sel < px
    composed(g, i2, sel, px, s2, first=0)
    want = g.read(s2, px + GUARD, R.STATS)
    assert got.tobytes() == want.tobytes() and want.tobytes() != st.tobytes()
    assert int((want["n"] != st["n"]).sum()) == sel


# ---- 4: skipped samples -----------------------------------------------------------------------------
def test_samples_that_overflow_are_skipped_as_the_accumulate_skips_them(cornell, rigs):
    import copy
    scene = copy.copy(cornell)
    scene.materials = cornell.materials.copy()
    lit = np.flatnonzero(scene.materials["emission"][:, :3].max(axis=1) > 0)
    assert len(lit) >= 1
    scene.materials["emission"][lit, :3] = np.float32(3.0e37)          # emission * 50 overflows fp32
    with np.errstate(over="ignore"):
        assert not np.isfinite(np.float32(3.0e37) * np.float32(50.0))
    # (the CPU oracle's render of this scene, camera and frame has 15 non-finite pixels of the 2,304)
    W, H = 64, 36
    px = W * H
    g = rigs(scene, math=N.MATH_PINNED, W=W, H=H)
    got, want, st, body = both(g, W, H, seed=77, bounces=9)
    inside = body[body < px]
    kept = want["n"][inside] == st["n"][inside]
    assert kept.any() and (~kept).any()         # some selected pixels kept their n, some did not
    assert want[inside[kept]].tobytes() == st[inside[kept]].tobytes()
    assert got.tobytes() == want.tobytes()


# ---- 5: end to end ----------------------------------------------------------------------------------
def adaptive_run(scene, fused, sync_every=1, rounds=40, per_round=1, move=False, **params):
    import clrt
    W, H = 64, 36
    rt = raytracer(scene, W, H, N.MATH_SHIPPED, 2)
    try:
        out = []
        image, info = rt.render_adaptive(rounds, samples_per_round=per_round, fused=fused, sync_every=sync_every, **params)
        out.append((image.tobytes(), rt.sample_stats().tobytes(), info, rt._sample_frame, rt.frame_count))
        if move:
            prev = rt.camera
            p = prev.position
            rt.camera = clrt.renderer.Camera(position=(p[0] + 0.37, p[1], p[2] + 0.1))
            rt.reproject_samples(prev)
            image, info = rt.render_adaptive(rounds, samples_per_round=per_round, fused=fused, sync_every=sync_every, **params)
            out.append((image.tobytes(), rt.sample_stats().tobytes(), info, rt._sample_frame, rt.frame_count))
        return out
    finally:
        rt.release()


PARAMS = dict(threshold=0.05, floor_y=0.01, min_samples=4, max_samples=32, radius=1)
_plain = {}


def plain_run(scene, key, **kw):
    """the fused=False runs, computed once and shared"""
    if key not in _plain:
        _plain[key] = adaptive_run(scene, False, **kw)
    return _plain[key]


@pytest.mark.parametrize("sync_every", [1, 4, 64])
def test_render_adaptive_fused_equals_the_composed_rounds(cornell, sync_every):
    want = plain_run(cornell, "move", move=True, **PARAMS)
    got = adaptive_run(cornell, True, sync_every, move=True, **PARAMS)
    assert len(want) == len(got) == 2
    for w, f in zip(want, got):
        assert f[2] == w[2] and f[3:] == w[3:]           # info, the sample-frame counter, frame_count
        assert f[1] == w[1] and f[0] == w[0]             # statistics and image bytes
    assert 4 < want[0][2]["rounds"] < 40 and want[0][2]["selected"] == 0      # (the run ended by itself)
    assert want[1][2]["rounds"] > 0


@pytest.mark.parametrize("sync_every", [1, 3])
def test_two_samples_per_round_and_a_run_that_hits_its_round_limit(cornell, sync_every):
    want = plain_run(cornell, "two", rounds=3, per_round=2, **PARAMS)
    got = adaptive_run(cornell, True, sync_every, rounds=3, per_round=2, **PARAMS)
    assert got == want
    assert want[0][2]["rounds"] == 3 and want[0][2]["selected"] > 0 and want[0][3] == 1 + 6


def test_three_fused_rounds_sum_the_traces_of_sample_frames_1_2_3(cornell):
    W, H = 32, 18
    rt = raytracer(cornell, W, H, N.MATH_PINNED, 2)
    try:
        rt.frame_count = 9
        seen = []
        image, info = rt.render_adaptive(10, min_samples=3, max_samples=3, fused=True, sync_every=4,
                                         on_sample=lambda rnd, frame, n, b: seen.append((rnd, frame, n, b["results"])))
        assert info == {"rounds": 3, "paths": 3 * W * H, "selected": 0, "hot": info["hot"]}
        assert rt.frame_count == 9 and rt._sample_frame == 4
        assert seen == [(r, r + 1, None, None) for r in range(4)]     # (the fourth was enqueued before the wait)
        st = rt.sample_stats()
        assert (st["n"] == 3).all()
        total = np.zeros((W * H, 3), np.float32)
        for f in (1, 2, 3):
            rt.frame_count = f
            rays, seeds = rt.camera_paths()
            rad, _ = rt.trace(rays["origin"], rays["dir"], seeds=seeds)
            total = total + rad
        assert st["sum"].reshape(-1, 3).tobytes() == total.tobytes() and total.any()
        assert image.tobytes() == R.resolve(st).reshape(H, W, 4).tobytes()
    finally:
        rt.release()


# ---- 6: the queue -----------------------------------------------------------------------------------
def test_a_queued_session_equals_a_blocking_replay(cornell, rigs):
    """Fused frames, a coalescible run of per-frame launches, select -> SamplePixels with the device count ->
    resolve -> denoise on one context with one non-blocking read at the end, against a fresh context that waits
    after every step."""
    W, H = 64, 36
    px = W * H
    outs = []
    for blocking in (False, True):
        g = rigs(cornell, math=N.MATH_PINNED, W=W, H=H, perframe_batch=None)   # (the default: frames coalesce)
        st0 = np.zeros(px, R.STATS)
        st0["n"][::3] = 8.0                 # a third of the pixels are done (and cold): the count matters
        st0["mean_y"][::3] = 0.5
        stats, ids, res = g.buffer(px * 32, st0), g.buffer(px * 4, np.zeros(px, np.uint32)), g.buffer(16)
        img, feat, den = g.buffer(px * 16), g.buffer(px * 32), g.buffer(px * 16)

        def step(fn, *a, **kw):
            fn(*a, **kw)
            if blocking:
                g.ctx.Finish()

        step(g.r.frame, 1, light_bounces=2, n_frames=4)
        for f in (5, 6, 7):
            step(g.r.frame, f, light_bounces=2)
        step(g.ctx.SelectPixels, g.k, stats, W, H, ids, res, min_samples=1, max_samples=8, radius=0)
        g.k.set_uint(N.FRAME_COUNT, 3)
        step(g.ctx.SamplePixels, g.k, ids, px, px, stats, count=res)
        step(g.ctx.ResolveSamples, g.k, stats, W, H, img)
        g.k.set_uint(N.FRAME_COUNT, 3)
        step(g.ctx.FrameFeatures, g.k, px, 1, feat)
        step(g.ctx.Denoise, g.k, img, feat, W, H, den)
        d = np.empty(px * 4, np.float32)
        g.ctx.ReadBuffer(den, d, blocking=blocking)
        g.ctx.Finish()
        outs.append((g.r.result().tobytes(), g.read(stats, px, R.STATS), d.tobytes(), g.read(res, 4, np.uint32).tolist()))
    sel = px - len(range(0, px, 3))
    assert outs[0][3] == outs[1][3] == [sel, 0, 0, 0]
    assert outs[0][0] == outs[1][0] and outs[0][2] == outs[1][2]
    assert outs[0][1].tobytes() == outs[1][1].tobytes()
    n = outs[0][1]["n"].reshape(-1)
    assert (n[::3] == 8).all() and (np.delete(n, np.arange(0, px, 3)) == 1).all()
    assert outs[0][1]["sum"].any() and np.frombuffer(outs[0][2], np.float32).any()


def test_a_round_after_a_refit_sees_the_moved_geometry(cornell):
    from test_refit_gpu import Mover, new_positions
    W, H = 64, 8
    px = W * H

    def one_round(m):
        m.k.set_int(N.LIGHT_BOUNCES, 2), m.k.set_int(N.LIGHT_TYPE, 0), m.k.set_float(N.SKYBOX_INTENSITY, 1.0)
        m.k.set_uint(N.FRAME_COUNT, 1)
        cam = ((0.0, -25.0, 8.5), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
        for slot, v in zip((N.CAMERA_POS, N.CAMERA_FRONT, N.CAMERA_UP), cam):
            m.k.set_float3(slot, v)
        mk = m.ctx.create_buffer
        bufs = [mk(N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR, px * 32, np.zeros(px, R.STATS)), mk(N.MEM_READ_WRITE, px * 4),
                mk(N.MEM_READ_WRITE, 16)]
        stats, ids, res = bufs
        m.ctx.SelectPixels(m.k, stats, W, H, ids, res, min_samples=1, max_samples=8)
        m.ctx.SamplePixels(m.k, ids, px, px, stats, count=res)
        out = np.empty(px, R.STATS)
        m.ctx.ReadBuffer(stats, out, blocking=True)
        for b in bufs:
            b.release()
        return out

    m = Mover(cornell, W, H)
    try:
        before = one_round(m)
        assert m.k.scene_prepares() == (1, 0)
        m.move(new_positions(cornell))
        after = one_round(m)
        assert m.k.scene_prepares() == (1, 1)      # no second full preparation
        moved = m.read_scene()
    finally:
        m.close()
    c = Mover(moved, W, H)
    try:
        want = one_round(c)
    finally:
        c.close()
    assert (after["n"] == 1).all()
    assert after.tobytes() == want.tobytes() and after.tobytes() != before.tobytes()


@pytest.mark.parametrize("config", ["lds", "global"])
def test_counters_equal_the_traces_over_the_records_in_range(cornell, rigs, config):
    W, H = 61, 7
    px = W * H
    g = rigs(cornell, math=N.MATH_PINNED, force_global=config == "global", stats=True, W=W, H=H)
    rng = np.random.default_rng(12)
    st = random_stats(rng, px + GUARD)
    ids, n = make_ids(rng, px)
    body = ids[FIRST:FIRST + n]
    inside = np.ascontiguousarray(body[body < px])
    assert 0 < len(inside) < n
    set_frame(g, 4)
    keys = ("rays", "node_visits", "tri_tests", "hits")
    ib, sb = g.buffer(ids.nbytes, ids), g.buffer(st.nbytes, st)
    g.ctx.Finish()
    g.k.reset_stats()
    g.ctx.SamplePixels(g.k, ib, n, px, sb, first=FIRST)
    g.ctx.Finish()
    fused = g.k.stats()
    # the trace over the in-range records alone
    jb = g.buffer(inside.nbytes, inside)
    rb, sd, ob = g.buffer(len(inside) * 32), g.buffer(len(inside) * 4), g.buffer(len(inside) * 16)
    g.ctx.CameraPathsFor(g.k, jb, len(inside), rb, sd)
    g.ctx.Finish()
    g.k.reset_stats()
    g.ctx.TracePaths(g.k, rb, ob, len(inside), seeds=sd, encoding=N.TRACE_LINEAR)
    g.ctx.Finish()
    trace = g.k.stats()
    assert [fused[k] for k in keys] == [trace[k] for k in keys]
    assert trace["rays"] >= len(inside) and trace["node_visits"] > 0 and trace["tri_tests"] > 0 and trace["hits"] > 0
    assert fused["launches"] == 1 == trace["launches"]


# ---- 7: errors through the real ABI ----------------------------------------------------------------
def test_errors_launch_nothing(cornell, rigs):
    import clrt
    W, H = 61, 7
    px = W * H
    g = rigs(cornell, W=W, H=H)
    other = rigs(cornell, W=W, H=H)
    g.k.set_timing(True)
    lib, ctx, k = g.ctx._lib, g.ctx.handle, g.k.handle
    rng = np.random.default_rng(2)
    st = random_stats(rng, px)
    stats, ids = g.buffer(st.nbytes, st), g.buffer(px * 4, np.arange(px, dtype=np.uint32))
    count, small = g.buffer(16, np.array([px, 0, 0, 0], np.uint32)), g.buffer(8, np.array([px, 0], np.uint32))
    short_stats = g.buffer(st.nbytes - 32)
    foreign = other.buffer(px * 32)
    h = lambda b: b.handle if b is not None else None   # noqa: E731
    smp = lambda kk, i, c, first, n, npx, s: lib.rtEnqueueSamplePixels(ctx, kk, h(i), h(c), first, n, npx, h(s))   # noqa: E731
    set_frame(g, 1)

    def kernel_with(skip=(), zero=None):
        """a kernel with every slot of g.k's but `skip` (and `zero` set to 0)"""
        b = clrt.CLKernel(g.ctx, "KernelEntry")
        b.set_math_mode(N.MATH_PINNED)
        ints = {N.WIDTH: W, N.HEIGHT: H, N.LIGHT_BOUNCES: 2, N.LIGHT_TYPE: 0}
        if zero is not None:
            ints[zero] = 0
        for slot, buf in ((N.BUFFER_OUT, g.r.out), (N.BUFFER_SCENE, g.r.bufs[0]), (N.BUFFER_NODE, g.r.bufs[1]),
                          (N.BUFFER_MATERIAL, g.r.bufs[2])):
            if slot not in skip:
                b.set_buffer(slot, buf)
        for slot, v in ints.items():
            if slot not in skip:
                b.set_int(slot, v)
        if N.FRAME_COUNT not in skip:
            b.set_uint(N.FRAME_COUNT, 1)
        if N.SKYBOX_INTENSITY not in skip:
            b.set_float(N.SKYBOX_INTENSITY, 1.0)
        for slot, v in zip((N.CAMERA_POS, N.CAMERA_FRONT, N.CAMERA_UP), ((0.0, -25.0, 8.5), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))):
            if slot not in skip:
                b.set_float3(slot, v)
        return b

    partial = {name: kernel_with(**kw) for name, kw in {
        "no_width": dict(skip=(N.WIDTH,)), "no_height": dict(skip=(N.HEIGHT,)), "no_frame": dict(skip=(N.FRAME_COUNT,)),
        "no_pos": dict(skip=(N.CAMERA_POS,)), "no_front": dict(skip=(N.CAMERA_FRONT,)), "no_up": dict(skip=(N.CAMERA_UP,)),
        "width_zero": dict(zero=N.WIDTH), "height_zero": dict(zero=N.HEIGHT),
        "no_scene": dict(skip=(N.BUFFER_SCENE,)), "no_nodes": dict(skip=(N.BUFFER_NODE,)),
        "no_materials": dict(skip=(N.BUFFER_MATERIAL,)), "no_bounces": dict(skip=(N.LIGHT_BOUNCES,)),
        "no_light_type": dict(skip=(N.LIGHT_TYPE,)), "no_skybox": dict(skip=(N.SKYBOX_INTENSITY,))}.items()}
    launches = g.k.stats()["launches"]
    rows = [
        # 1. RT_INVALID_VALUE
        (smp(k, ids, count, 1 << 31, 1, px, stats), -30), (smp(k, ids, count, 0, (1 << 31) + 1, px, stats), -30),
        (smp(k, ids, count, 0, px, 0, stats), -30), (smp(k, ids, count, 0, px, (1 << 31) + 1, stats), -30),
        (smp(k, None, count, 0, px, 0, None), -30),                                     # ... before the buffers
        # 2. RT_INVALID_MEM_OBJECT
        (smp(k, None, count, 0, px, px, stats), -38), (smp(k, ids, count, 0, px, px, None), -38),
        (smp(k, foreign, count, 0, px, px, stats), -38), (smp(k, ids, count, 0, px, px, foreign), -38),
        (smp(k, ids, foreign, 0, px, px, stats), -38),
        (smp(k, ids, count, 0, px, px, ids), -38), (smp(k, ids, stats, 0, px, px, stats), -38),
        (smp(k, ids, ids, 0, px, px, stats), -38),
        (smp(k, ids, ids, 1, px, px, stats), -38),                                      # ... before the sizes
        # 3. RT_INVALID_BUFFER_SIZE
        (smp(k, ids, count, 1, px, px, stats), -61), (smp(k, ids, small, 0, px, px, stats), -61),
        (smp(k, ids, count, 0, px, px, short_stats), -61), (smp(k, ids, count, 0, px, px + 1, stats), -61),
        (smp(partial["no_width"].handle, ids, small, 0, px, px, stats), -61),           # ... before the slots
        (smp(k, ids, count, 0, 0, px + 1, stats), -61),                                 # ... before the empty range
        # 4. RT_INVALID_KERNEL_ARGS
        *[(smp(b.handle, ids, count, 0, px, px, stats), -52) for b in partial.values()],
        (smp(partial["no_scene"].handle, ids, count, 0, 0, px, stats), -52),            # ... before the empty range
        # 5. n == 0
        (smp(k, ids, count, 0, 0, px, stats), 0), (smp(k, ids, None, px, 0, px, stats), 0),
    ]
    assert [r[0] for r in rows] == [r[1] for r in rows]
    s = g.k.stats()
    assert s["launches"] == launches and all(b.stats()["launches"] == 0 for b in partial.values())
    assert all(b.scene_prepares() == (0, 0) for b in partial.values())                 # nothing was prepared
    assert g.read(stats, px, R.STATS).tobytes() == st.tobytes()
    # and the kernel that saw every error still works: one launch, which adds to kernel_ms
    ms = s["kernel_ms"]
    assert smp(k, ids, count, 0, px, px, stats) == 0
    s = g.k.stats()
    assert s["launches"] == launches + 1 and s["kernel_ms"] > ms
    assert (g.read(stats, px, R.STATS)["n"] == st["n"] + 1).all()
    for b in partial.values():
        b.release()


def test_a_leaf_of_more_than_127_triangles_is_refused_after_the_preparation(rigs):
    """Row 6: a scene the octant walk cannot hold is RT_INVALID_OPERATION, as rtEnqueueTracePaths refuses it, and an
    empty range on the same kernel is RT_SUCCESS before anything is prepared."""
    import stress_scenes as SS
    scene = SS.soup_scene(12, "big")
    W, H = 8, 4
    px = W * H
    g = rigs(scene, W=W, H=H)
    for slot, v in zip((N.CAMERA_POS, N.CAMERA_FRONT, N.CAMERA_UP), ((0.0, -25.0, 8.5), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))):
        g.k.set_float3(slot, v)
    g.k.set_uint(N.FRAME_COUNT, 1)
    g.lights(2)
    st = np.zeros(px, R.STATS)
    stats, ids = g.buffer(st.nbytes, st), g.buffer(px * 4, np.arange(px, dtype=np.uint32))
    lib, ctx, k = g.ctx._lib, g.ctx.handle, g.k.handle
    assert lib.rtEnqueueSamplePixels(ctx, k, ids.handle, None, 0, 0, px, stats.handle) == 0
    assert g.k.scene_prepares() == (0, 0)
    assert lib.rtEnqueueSamplePixels(ctx, k, ids.handle, None, 0, px, px, stats.handle) == -59
    assert g.k.stats()["launches"] == 0 and g.read(stats, px, R.STATS).tobytes() == st.tobytes()

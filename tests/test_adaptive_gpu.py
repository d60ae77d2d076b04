"""GPU: adaptive sampling -- rtEnqueueAccumulateSamples, rtEnqueueSelectPixels, rtEnqueueCameraPathsFor and
rtEnqueueResolveSamples against the numpy restatement tests/adaptive_ref.py, byte for byte; the rounds end to end
against Raytracer.trace (itself pinned to the oracle) and against a host replay of the device's own trace results;
their ordering on the queue; and the error rows through the real ABI.
"""
import ctypes

import numpy as np
import pytest

import adaptive_ref as R
from clrt import _native as N
from test_ray_query import MATHS, Rig, bits

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5


class AdaptRig(Rig):
    def lights(self, bounces=2, light_type=0, skybox=1.0):
        self.k.set_int(N.LIGHT_BOUNCES, bounces)
        self.k.set_int(N.LIGHT_TYPE, light_type)
        self.k.set_float(N.SKYBOX_INTENSITY, skybox)

    def select(self, stats_buf, W, H, ids_buf, res_buf, **params):
        self.ctx.SelectPixels(self.k, stats_buf, W, H, ids_buf, res_buf, **params)
        return self.read(res_buf, 4, np.uint32)


@pytest.fixture
def rigs():
    made = []

    def make(*a, **kw):
        made.append(AdaptRig(*a, **kw))
        return made[-1]

    yield make
    for g in made:
        g.close()


def random_stats(rng, n, zero_share=0.2):
    """Prior statistics: n from 0 to 40, some records all zero, reserved words random."""
    st = np.zeros(n, R.STATS)
    st["n"] = rng.integers(0, 41, n)
    st["mean_y"] = rng.random(n).astype(np.float32) * 2
    st["m2_y"] = (rng.random(n) * st["n"] * 0.05).astype(np.float32)
    st["sum"] = rng.random((n, 3)).astype(np.float32) * st["n"][:, None]
    st["reserved"] = rng.integers(0, 2 ** 32, (n, 2), dtype=np.uint32)
    st[rng.random(n) < zero_share] = np.zeros(1, R.STATS)[0]
    return st


def random_results(rng, m, bad_share=0.05):
    r = np.zeros(m, R.RESULT)
    r["radiance"] = (rng.random((m, 3)) ** 3 * 4).astype(np.float32)
    r["prim"] = rng.integers(-1, 30, m)
    bad = np.flatnonzero(rng.random(m) < bad_share)
    r["radiance"][bad, rng.integers(0, 3, len(bad))] = rng.choice([np.inf, -np.inf, np.nan], len(bad))
    return r, len(bad)


# ---- accumulate ---------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(1, 1), (61, 7), (131, 77)], ids=["1x1", "61x7", "131x77"])
def test_accumulate_equals_the_restatement(cornell, rigs, size):
    W, H = size
    px = W * H
    rng = np.random.default_rng(100 + px)
    g = rigs(cornell)
    # two records past the image follow the statistics: they must keep their bytes
    st = random_stats(rng, px + 2)
    first, tail = 3, 5
    # a random subset of the pixels in random order; about 5 % out of range, 0xFFFFFFFF among them; guard
    # records on both sides name pixels of the image that the range does not: touching one would show
    perm = rng.permutation(px).astype(np.uint32)
    n = max(1, int(px * 0.8)) if px > 1 else 1
    body = perm[:n].copy()
    guards = (perm[n:].tolist() * (first + tail))[:first + tail] if px > n else [0] * (first + tail)
    if px == 1:
        body = np.array([0, 1, 0xFFFFFFFF, 2], np.uint32)       # the one pixel, and three ids out of range
        n = len(body)
        guards = [0] * (first + tail)
    else:
        out = np.flatnonzero(rng.random(n) < 0.05)
        body[out] = rng.choice(np.array([px, px + 1, px + 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], np.uint32), len(out))
        body[n // 2] = 0xFFFFFFFF
    ids = np.concatenate([np.array(guards[:first], np.uint32), body, np.array(guards[first:], np.uint32)])
    m = max(len(ids), px + 7)        # results: the ids' records, and past the image for the run without ids
    res1, bad1 = random_results(rng, m)
    res2, _ = random_results(rng, m)
    assert px == 1 or (bad1 > 0 and (body >= px).sum() > 1)
    sb = g.buffer(st.nbytes, st)
    ib, r1, r2 = g.buffer(ids.nbytes, ids), g.buffer(res1.nbytes, res1), g.buffer(res2.nbytes, res2)
    g.ctx.AccumulateSamples(g.k, ib, r1, n, px, sb, first=first)
    got1 = g.read(sb, px + 2, R.STATS)
    want1 = R.accumulate(st, ids, res1, first, n, px)
    assert got1.tobytes() == want1.tobytes()
    assert want1.tobytes() != st.tobytes()
    # two calls in a row: the restatement applied twice
    g.ctx.AccumulateSamples(g.k, ib, r2, n, px, sb, first=first)
    assert g.read(sb, px + 2, R.STATS).tobytes() == R.accumulate(want1, ids, res2, first, n, px).tobytes()
    # ids == NULL: record i is pixel i, and records from n_pixels on are skipped
    sb = g.buffer(st.nbytes, st)
    f0 = 3 if px > 8 else 0
    cnt = m - f0
    g.ctx.AccumulateSamples(g.k, None, r1, cnt, px, sb, first=f0)
    want = R.accumulate(st, None, res1, f0, cnt, px)
    assert g.read(sb, px + 2, R.STATS).tobytes() == want.tobytes()
    assert want[:f0].tobytes() == st[:f0].tobytes() and want[px:].tobytes() == st[px:].tobytes()
    assert f0 + cnt > px    # (the range ran past the image)


# ---- select -------------------------------------------------------------------------------------
def cold(px, n=8.0):
    st = np.zeros(px, R.STATS)
    st["n"], st["mean_y"] = n, 0.5
    return st


SELECT_SIZES = [(1, 1), (5, 3), (61, 7), (131, 77), (2049, 1), (1024, 320)]


@pytest.mark.parametrize("radius", [0, 1, 2])
@pytest.mark.parametrize("size", SELECT_SIZES, ids=[f"{w}x{h}" for w, h in SELECT_SIZES])
def test_select_equals_the_restatement(cornell, rigs, size, radius):
    """1024 x 320 = 327,680 pixels are 320 blocks of rtp::kSelectBlockPixels = 1024 (256 threads, 4 pixels each),
    more than the rtp::kScanThreads = 256 block counts the single scanning workgroup takes per pass: the scan
    runs a second pass with a carry (rt_adaptive_plan.hpp; the CPU test pins scan_passes > 1 for this size).
    2049 x 1 is two full blocks and a one-pixel third."""
    W, H = size
    px = W * H
    rng = np.random.default_rng(7 * px + radius)
    g = rigs(cornell)
    params = dict(threshold=0.05, floor_y=0.01, min_samples=4, max_samples=64, radius=radius)
    cases = {}
    cases["none"] = cold(px)
    cases["all"] = cold(px, 2.0)
    corners = sorted({0, W - 1, px - W, px - 1})
    for c in corners:   # exactly one pixel selected: the others sit at max_samples, whatever their window holds
        st = cold(px, 64.0)
        st["n"][c], st["m2_y"][c] = 8.0, 100.0
        cases[f"corner{c}"] = st
    st = cold(px)
    st["m2_y"][corners] = 100.0                      # ... and the corners' dilation into pixels that may be selected
    cases["corners_dilated"] = st
    st = cold(px)
    st["n"] = rng.choice(np.array([3, 4, 5, 8, 63, 64, 65], np.float32), px)   # just below / at min, at / past max
    st["m2_y"][rng.random(px) < 0.3] = 100.0
    st["mean_y"] = rng.random(px).astype(np.float32)
    cases["random"] = st
    fill = np.full(px, SENTINEL, np.uint32)
    for name, st in cases.items():
        sb, ib = g.buffer(st.nbytes, st), g.buffer(fill.nbytes, fill)
        rb = g.buffer(16, np.full(4, 0xDEADBEEF, np.uint32))
        res = g.select(sb, W, H, ib, rb, **params)
        ids, hot = R.select(st, W, H, **params)
        want = fill.copy()
        want[:len(ids)] = ids
        assert res.tolist() == [len(ids), hot, 0, 0], (name, res, len(ids), hot)
        assert g.read(ib, px, np.uint32).tobytes() == want.tobytes(), name
        assert g.read(sb, px, R.STATS).tobytes() == st.tobytes(), name      # stats is only read
        if name == "none":
            assert len(ids) == 0
        elif name == "all":
            assert len(ids) == px
        elif name.startswith("corner") and name != "corners_dilated":
            assert ids.tolist() == [int(name[6:])] and hot == 1
        elif name == "random" and px > 64:
            assert 0 < len(ids) < px and hot > 0
        for b in (sb, ib, rb):
            b.release()
            g._bufs.remove(b)


# ---- camera paths for a list of work-items -------------------------------------------------------
@pytest.mark.parametrize("size", [(64, 36), (61, 7)], ids=["64x36", "61x7"])
@pytest.mark.parametrize("math_name", list(MATHS))
def test_camera_paths_for_equal_the_full_calls_rows(cornell, rigs, math_name, size):
    W, H = size
    px = W * H
    big = 3 * px                     # ids past width * height: the full call with a larger global_work_size
    rng = np.random.default_rng(px)
    g = rigs(cornell, math=MATHS[math_name], W=W, H=H)
    g.r.frame(7, light_bounces=1)    # sets FRAME_COUNT 7 and the camera slots
    full_r, full_s = g.buffer(big * 32), g.buffer(big * 4)
    g.ctx.CameraPaths(g.k, big, full_r, full_s)
    rays = g.read(full_r, big * 8, np.uint32).reshape(big, 8)
    seeds = g.read(full_s, big, np.uint32)
    first, n, tail = 5, px + 37, 3
    ids = rng.integers(0, px, first + n + tail).astype(np.uint32)       # out of order, with duplicates
    ids[first + 1], ids[first + 2] = ids[first], ids[first]
    past = rng.choice(np.arange(first, first + n), n // 8, replace=False)
    ids[past] = rng.integers(px, big, len(past))
    ids[first + 3], ids[first + n - 1] = big - 1, px
    m = len(ids)
    ib = g.buffer(ids.nbytes, ids)
    rb, sb = g.buffer(m * 32, np.full(m * 8, SENTINEL, np.uint32)), g.buffer(m * 4, np.full(m, SENTINEL, np.uint32))
    g.ctx.CameraPathsFor(g.k, ib, n, rb, sb, first=first)
    want_r = np.full((m, 8), SENTINEL, np.uint32)
    want_s = np.full(m, SENTINEL, np.uint32)
    want_r[first:first + n], want_s[first:first + n] = rays[ids[first:first + n]], seeds[ids[first:first + n]]
    assert g.read(rb, m * 8, np.uint32).tobytes() == want_r.tobytes()
    assert g.read(sb, m, np.uint32).tobytes() == want_s.tobytes()
    assert (ids[first:first + n] >= px).sum() >= n // 8


# ---- resolve ------------------------------------------------------------------------------------
_resolve_refs = {}


def resolve_case(size):
    if size not in _resolve_refs:
        px = size[0] * size[1]
        rng = np.random.default_rng(px)
        st = random_stats(rng, px)
        st["n"][st["n"] == 0] = 0
        some = np.flatnonzero(st["n"] == 0)[::2]
        st["sum"][some] = 3.0            # a pixel with n == 0 is sixteen zero bytes whatever its sums hold
        _resolve_refs[size] = (st, R.resolve(st))
    return _resolve_refs[size]


@pytest.mark.parametrize("size", [(5, 3), (131, 77)], ids=["5x3", "131x77"])
@pytest.mark.parametrize("math_name", list(MATHS))
def test_resolve_equals_the_restatement_in_every_math_mode(cornell, rigs, math_name, size):
    W, H = size
    px = W * H
    st, want = resolve_case(size)
    assert (st["n"] == 0).any() and (st["n"] > 0).any()
    g = rigs(cornell, math=MATHS[math_name])
    sb = g.buffer(st.nbytes, st)
    ob = g.buffer((px + 3) * 16, np.full((px + 3) * 4, SENTINEL, np.uint32))
    g.ctx.ResolveSamples(g.k, sb, W, H, ob)
    got = g.read(ob, (px + 3) * 4, np.uint32).reshape(px + 3, 4)
    assert got[:px].tobytes() == want.tobytes()
    assert (got[px:] == SENTINEL).all()          # the bytes past the image are kept
    assert (got[:px][st["n"] == 0] == 0).all()


# ---- end to end ------------------------------------------------------------------------------------
def raytracer(scene, W, H, math, bounces):
    import clrt
    rt = clrt.Raytracer(W, H)
    rt.Init()
    rt.upload_scene(scene)
    rt.kernel.set_math_mode(math)
    rt.light_bounces = bounces
    return rt


def test_three_rounds_sum_the_traces_of_sample_frames_1_2_3(cornell):
    W, H = 32, 18
    rt = raytracer(cornell, W, H, N.MATH_PINNED, 2)
    try:
        rt.frame_count = 9
        image, info = rt.render_adaptive(10, min_samples=3, max_samples=3)
        assert info == {"rounds": 3, "paths": 3 * W * H, "selected": 0, "hot": info["hot"]}
        assert rt.frame_count == 9
        st = rt.sample_stats()
        assert (st["n"] == 3).all()
        total = np.zeros((W * H, 3), np.float32)
        for f in (1, 2, 3):
            rt.frame_count = f
            rays, seeds = rt.camera_paths()
            rad, _ = rt.trace(rays["origin"], rays["dir"], seeds=seeds)
            total = total + rad
        assert st["sum"].reshape(-1, 3).tobytes() == total.tobytes()
        assert total.any()
        # the fourth select has nothing left
        _, info = rt.render_adaptive(1, min_samples=3, max_samples=3)
        assert info["rounds"] == 0 and info["selected"] == 0 and info["paths"] == 0
        assert image.tobytes() == R.resolve(st).reshape(H, W, 4).tobytes()
        rt.reset_samples()
        assert rt.sample_stats().tobytes() == bytes(32 * W * H)
    finally:
        rt.release()


def test_adaptive_rounds_equal_a_host_replay_and_leave_the_sky_at_four_samples(cornell, oracle_mod):
    """Cornell at 64 x 36 from the default camera, 2 bounces, shipped math.  The loop runs live; the host replays it
    with the numpy select and accumulate from the device's own trace results."""
    W, H = 64, 36
    px = W * H
    params = dict(threshold=0.05, floor_y=0.01, min_samples=4, max_samples=32, radius=1)

    def all_miss_3x3(hit):
        """pixels whose whole 3 x 3 neighbourhood (inside the image) never hit"""
        h = np.pad(hit.reshape(H, W), 1)
        near = np.zeros((H, W), bool)
        for dy in range(3):
            for dx in range(3):
                near |= h[dy:dy + H, dx:dx + W]
        return ~near.reshape(-1)

    # on the CPU first: this camera and size give both kinds of pixel (the oracle's primary hit ids of the four
    # sample frames every pixel takes)
    hit = np.zeros(px, bool)
    for f in (1, 2, 3, 4):
        _, ids, _, _ = oracle_mod.render(cornell, W, H, frame_count=f, light_bounces=1, want_hits=True, threads=8)
        hit |= ids.reshape(-1) >= 0
    assert all_miss_3x3(hit).sum() >= 100 and hit.sum() >= 100

    rt = raytracer(cornell, W, H, N.MATH_SHIPPED, 2)
    try:
        log = []

        def on_sample(rnd, frame, n, b):
            ids = np.empty(n, np.uint32)
            res = np.empty(n, N.PATH_RESULT_DTYPE)
            rt.ctx.ReadBuffer(b["ids"], ids, blocking=True)
            rt.ctx.ReadBuffer(b["results"], res, blocking=True)
            log.append((rnd, frame, ids, res))

        image, info = rt.render_adaptive(40, on_sample=on_sample, **params)
        got = rt.sample_stats().reshape(-1)
    finally:
        rt.release()
    st = np.zeros(px, R.STATS)
    hit = np.zeros(px, bool)
    assert [e[1] for e in log] == list(range(1, len(log) + 1)) and len(log) == info["rounds"]
    for rnd, frame, ids, res in log:
        want_ids, _ = R.select(st, W, H, **params)
        assert ids.tobytes() == want_ids.tobytes(), rnd
        st = R.accumulate(st, ids, res.view(R.RESULT), 0, len(ids), px)
        hit[ids[res["prim"] >= 0]] = True
    last_ids, last_hot = R.select(st, W, H, **params)
    assert (len(last_ids), last_hot) == (info["selected"], info["hot"])
    assert got.tobytes() == st.tobytes()
    assert image.tobytes() == R.resolve(st).reshape(H, W, 4).tobytes()
    sky = all_miss_3x3(hit)
    assert sky.sum() >= 1 and (st["n"][sky] == 4).all()      # the sky term is a constant: m2 is exactly 0
    assert (st["m2_y"][sky] == 0).all()
    assert (st["n"] > 4).any()
    assert st["n"].min() >= 4 and st["n"].max() <= 32
    assert info["paths"] == int(st["n"].sum()) == sum(len(e[2]) for e in log)


# ---- ordering -----------------------------------------------------------------------------------
def test_a_queued_session_equals_a_blocking_replay(cornell, rigs):
    """A fused launch, a coalescible run of per-frame launches, then select -> camera paths -> trace -> accumulate ->
    resolve -> denoise of the resolved image on one context with one non-blocking read at the end, against a fresh
    context that waits after every step."""
    W, H = 64, 36
    px = W * H
    outs = []
    for blocking in (False, True):
        g = rigs(cornell, math=N.MATH_PINNED, W=W, H=H, perframe_batch=None)   # (the default: frames coalesce)
        stats, ids, res = g.buffer(px * 32, np.zeros(px, R.STATS)), g.buffer(px * 4), g.buffer(16)
        rb, sb, ob = g.buffer(px * 32), g.buffer(px * 4), g.buffer(px * 16)
        img, feat, den = g.buffer(px * 16), g.buffer(px * 32), g.buffer(px * 16)

        def step(fn, *a, **kw):
            fn(*a, **kw)
            if blocking:
                g.ctx.Finish()

        step(g.r.frame, 1, light_bounces=2, n_frames=4)
        for f in (5, 6, 7):
            step(g.r.frame, f, light_bounces=2)
        # (zero statistics and min_samples 1: every pixel is selected, so the session needs no read of `result`)
        step(g.ctx.SelectPixels, g.k, stats, W, H, ids, res, min_samples=1, max_samples=8)
        g.k.set_uint(N.FRAME_COUNT, 3)
        step(g.ctx.CameraPathsFor, g.k, ids, px, rb, sb)
        step(g.ctx.TracePaths, g.k, rb, ob, px, seeds=sb)
        step(g.ctx.AccumulateSamples, g.k, ids, ob, px, px, stats)
        step(g.ctx.ResolveSamples, g.k, stats, W, H, img)
        g.k.set_uint(N.FRAME_COUNT, 3)
        step(g.ctx.FrameFeatures, g.k, px, 1, feat)
        step(g.ctx.Denoise, g.k, img, feat, W, H, den)
        d = np.empty(px * 4, np.float32)
        g.ctx.ReadBuffer(den, d, blocking=blocking)
        g.ctx.Finish()
        outs.append((g.r.result().tobytes(), g.read(stats, px, R.STATS), d.tobytes(), g.read(res, 4, np.uint32).tolist()))
    assert outs[0][3] == outs[1][3] == [px, 0, 0, 0]
    assert outs[0][0] == outs[1][0] and outs[0][2] == outs[1][2]
    assert outs[0][1].tobytes() == outs[1][1].tobytes()
    assert (outs[0][1]["n"] == 1).all() and outs[0][1]["sum"].any() and np.frombuffer(outs[0][2], np.float32).any()


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
        flags = N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR
        bufs = [mk(flags, px * 32, np.zeros(px, R.STATS)), mk(N.MEM_READ_WRITE, px * 4), mk(N.MEM_READ_WRITE, 16),
                mk(N.MEM_READ_WRITE, px * 32), mk(N.MEM_READ_WRITE, px * 4), mk(N.MEM_READ_WRITE, px * 16)]
        stats, ids, res, rb, sb, ob = bufs
        m.ctx.SelectPixels(m.k, stats, W, H, ids, res, min_samples=1, max_samples=8)
        m.ctx.CameraPathsFor(m.k, ids, px, rb, sb)
        m.ctx.TracePaths(m.k, rb, ob, px, seeds=sb)
        m.ctx.AccumulateSamples(m.k, ids, ob, px, px, stats)
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


# ---- errors through the real ABI ---------------------------------------------------------------
def test_errors_launch_nothing(cornell, rigs):
    import clrt
    W, H = 61, 7
    px = W * H
    g = rigs(cornell, W=W, H=H)
    other = rigs(cornell, W=W, H=H)
    g.k.set_timing(True)
    lib, ctx, k = g.ctx._lib, g.ctx.handle, g.k.handle
    st = np.zeros(px, R.STATS)
    stats, ids, res = g.buffer(st.nbytes, st), g.buffer(px * 4, np.arange(px, dtype=np.uint32)), g.buffer(16)
    results, rays, seeds, out = g.buffer(px * 16, np.ones(px * 4, np.float32)), g.buffer(px * 32), g.buffer(px * 4), g.buffer(px * 16)
    small = g.buffer(8)
    foreign = other.buffer(px * 32)
    par = N.ADAPTIVE_PARAMS(0.05, 0.01, 4, 64, 1)
    h = lambda b: b.handle if b is not None else None   # noqa: E731
    launches = g.k.stats()["launches"]

    acc = lambda i, r, first, n, npx, s: lib.rtEnqueueAccumulateSamples(ctx, k, h(i), h(r), first, n, npx, h(s))   # noqa: E731
    sel = lambda s, w, hh, p, i, r: lib.rtEnqueueSelectPixels(ctx, k, h(s), w, hh, ctypes.byref(p) if p else None, h(i), h(r))   # noqa: E731
    cpf = lambda kk, i, first, n, r, s: lib.rtEnqueueCameraPathsFor(ctx, kk, h(i), first, n, h(r), h(s))   # noqa: E731
    rsv = lambda s, w, hh, o: lib.rtEnqueueResolveSamples(ctx, k, h(s), w, hh, h(o))   # noqa: E731
    bare = clrt.CLKernel(g.ctx, "KernelEntry")
    g.r.frame(1, light_bounces=1)      # sets every slot of g.k (one launch)
    launches = g.k.stats()["launches"]
    rows = [
        (acc(ids, results, 1 << 31, 1, px, stats), -30), (acc(ids, results, 0, px, 0, stats), -30),
        (acc(ids, None, 0, px, 0, None), -30),                                  # ... before the buffers
        (acc(ids, None, 0, px, px, stats), -38), (acc(foreign, results, 0, px, px, stats), -38),
        (acc(ids, results, 0, px, px, results), -38), (acc(ids, results, 0, px, px, ids), -38),
        (acc(ids, results, 1, px, px, stats), -61), (acc(ids, results, 0, px, px + 1, stats), -61),
        (acc(ids, results, 0, 0, px + 1, stats), -61),                          # ... before the empty range
        (acc(ids, results, 0, 0, px, stats), 0),
        (sel(stats, W, H, None, ids, res), -30), (sel(stats, W, H, N.ADAPTIVE_PARAMS(0.05, 0.01, 4, 64, 3), ids, res), -30),
        (sel(stats, W, H, N.ADAPTIVE_PARAMS(float("nan"), 0.01, 4, 64, 1), ids, res), -30),
        (sel(stats, 0, H, par, ids, res), -30), (sel(stats, 65536, 32769, par, ids, res), -30),
        (sel(None, W, H, par, ids, res), -38), (sel(stats, W, H, par, ids, ids), -38),
        (sel(stats, W, H, par, stats, res), -38), (sel(foreign, W, H, par, ids, res), -38),
        (sel(stats, W, H + 1, par, ids, res), -61), (sel(stats, W, H, par, ids, small), -61),
        (sel(stats, W, H, par, small, res), -61),
        (cpf(bare.handle, ids, 0, px, rays, seeds), -52),                       # slots unset
        (cpf(k, ids, 1 << 31, 1, rays, seeds), -30),
        (cpf(k, ids, 0, px, None, seeds), -38), (cpf(k, ids, 0, px, rays, rays), -38),
        (cpf(k, ids, 0, px, ids, seeds), -38), (cpf(k, foreign, 0, px, rays, seeds), -38),
        (cpf(k, ids, 1, px, rays, seeds), -61), (cpf(k, ids, 0, 3, rays, small), -61),
        (cpf(k, ids, 0, 0, rays, seeds), 0),
        (rsv(stats, 0, H, out), -30), (rsv(stats, 65536, 32769, out), -30),
        (rsv(stats, W, H, None), -38), (rsv(stats, W, H, stats), -38), (rsv(foreign, W, H, out), -38),
        (rsv(stats, W, H + 1, out), -61), (rsv(stats, W, H, small), -61),
    ]
    assert [r[0] for r in rows] == [r[1] for r in rows]
    s = g.k.stats()
    assert s["launches"] == launches and bare.stats()["launches"] == 0
    assert g.read(stats, px, R.STATS).tobytes() == st.tobytes()
    # and the kernel that saw every error still works: each call is one launch and adds to kernel_ms
    ms = s["kernel_ms"]
    assert acc(ids, results, 0, px, px, stats) == 0 and sel(stats, W, H, par, ids, res) == 0
    assert cpf(k, ids, 0, px, rays, seeds) == 0 and rsv(stats, W, H, out) == 0
    s = g.k.stats()
    assert s["launches"] == launches + 4 and s["kernel_ms"] > ms
    assert (g.read(stats, px, R.STATS)["n"] == 1).all() and g.read(res, 4, np.uint32).tolist() == [px, 0, 0, 0]
    bare.release()

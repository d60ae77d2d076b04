"""GPU: path tracing over caller rays (rtEnqueueTracePaths, rtEnqueueCameraPaths).

The reference for arbitrary rays and seeds is tests/path_ref.py, a replay of the oracle's Render
pinned to the oracle by tests/test_path_ref.py; the render path -- bit-exact with the live reference in
every math mode -- is the reference for the camera's paths.

The inputs (checked with the replay alone on the CPU): Cornell, 512 random_rays plus the 32x18 camera
paths of frame 1 -- 1,088 records; the bunny proxy and soup_scene(12, "rt7"), 192 random rays each.  The
fixture asserts, before anything is compared, at least 100 first-segment misses and at least 100 paths
of three or more rounds in the Cornell set.
"""
import ctypes
import os

import numpy as np
import pytest

from clrt import _native as N
from test_ray_query import MATHS, Rig, bits, degenerate_rays, make_rays, random_rays, scene_box

pytestmark = pytest.mark.gpu

INF = float("inf")
BOUNCES, LIGHTS = (1, 2, 9), (0, 1, 2)
SEED_BASES = (12345, 0xFFFFFF00)   # the second wraps past 2^32 inside the 1,088 records
COUNTERS = ("rays", "node_visits", "tri_tests", "hits")
CW, CH = 32, 18


def result_bits(res):
    return np.ascontiguousarray(res).view(np.uint32).reshape(-1, 4)


def want_bits(ref):
    return np.concatenate([bits(ref["radiance"]), ref["prim"].view(np.uint32)[:, None]], axis=1)


# ---- the device side ----------------------------------------------------------------------------
class TraceRig(Rig):
    def lights(self, bounces=9, light_type=0, skybox=1.0):
        self.k.set_int(N.LIGHT_BOUNCES, bounces)
        self.k.set_int(N.LIGHT_TYPE, light_type)
        self.k.set_float(N.SKYBOX_INTENSITY, skybox)

    def trace(self, rays, seeds=None, seed_base=0, encoding=N.TRACE_LINEAR):
        rb = self.buffer(rays.nbytes, rays)
        sb = None if seeds is None else self.buffer(4 * len(rays), np.ascontiguousarray(seeds, np.uint32))
        ob = self.buffer(len(rays) * 16)
        self.ctx.TracePaths(self.k, rb, ob, len(rays), seeds=sb, seed_base=seed_base, encoding=encoding)
        return self.read(ob, len(rays), N.PATH_RESULT_DTYPE)

    def counters(self):
        st = self.k.stats()
        return tuple(st[c] for c in COUNTERS)


@pytest.fixture
def rigs():
    made = []

    def make(*a, **kw):
        made.append(TraceRig(*a, **kw))
        return made[-1]

    yield make
    for g in made:
        g.close()


# ---- references, computed once and shared (never modified) --------------------------------------
@pytest.fixture(scope="module")
def proxy():
    import clrt.proxy as P
    return P.bunny_proxy()


@pytest.fixture(scope="module")
def soup():
    import stress_scenes as SS
    return SS.soup_scene(12, "rt7")


@pytest.fixture(scope="module")
def refs(cornell, proxy, soup, oracle_mod):
    """Per input set: rays, seeds and the replay's results per (variant, bounces)."""
    import path_ref
    cam_rays, cam_seeds = path_ref.camera_paths(CW, CH, 1)
    rays = np.concatenate([random_rays(cornell, 512), cam_rays])
    seeds = np.concatenate([np.random.default_rng(5).integers(0, 2 ** 32, 512, dtype=np.uint32), cam_seeds])
    n = len(rays)
    windowed = rays.copy()
    windowed["tmin"], windowed["tmax"] = 0.0, 5.0
    sets = {"cornell": (cornell, rays, seeds)}
    jobs, keys = [], []
    for lt in LIGHTS:
        jobs.append((cornell, rays, seeds, BOUNCES, lt, 1.0)), keys.append(("cornell", f"light{lt}"))
    for base in SEED_BASES:
        based = ((base + np.arange(n, dtype=np.uint64)) & 0xffffffff).astype(np.uint32)
        jobs.append((cornell, rays, based, (9,), 0, 1.0)), keys.append(("cornell", f"base{base}"))
    jobs.append((cornell, windowed, seeds, (2, 9), 1, 1.0)), keys.append(("cornell", "window"))
    for name, scene in (("proxy", proxy), ("soup", soup)):
        r = random_rays(scene, 192)
        s = np.random.default_rng(6).integers(0, 2 ** 32, 192, dtype=np.uint32)
        sets[name] = (scene, r, s)
        jobs.append((scene, r, s, BOUNCES, 0, 1.0)), keys.append((name, "light0"))
        jobs.append((scene, r, s, (9,), 2, 0.25)), keys.append((name, "light2"))
    done = path_ref.trace_rays_pool(jobs, procs=min(16, os.cpu_count() or 1))
    out = {name: {"scene": sc, "rays": r, "seeds": s, "windowed": windowed if name == "cornell" else None}
           for name, (sc, r, s) in sets.items()}
    for (name, variant), res in zip(keys, done):
        out[name][variant] = res
    full = out["cornell"]["light0"][9]
    assert (full["prim"] < 0).sum() >= 100, "first-segment misses in the Cornell set"
    assert (full["rounds"] >= 3).sum() >= 100, "paths of three or more rounds in the Cornell set"
    assert (out["cornell"]["window"][9]["prim"] != out["cornell"]["light1"][9]["prim"]).sum() >= 50
    for name in ("proxy", "soup"):
        p = out[name]["light0"][9]["prim"]
        assert (p >= 0).any() and (p < 0).any()
    return out


def check(res, ref, what):
    got, want = result_bits(res), want_bits(ref)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} records differ, first {bad[:4]}: {res[bad[:4]]} vs " \
                          f"{ref['radiance'][bad[:4]]} {ref['prim'][bad[:4]]}"


# ---- 1: pinned parity with the replay -----------------------------------------------------------
@pytest.mark.parametrize("force_global", [False, True], ids=["lds", "global"])
def test_pinned_equals_replay_on_cornell(refs, rigs, force_global):
    c = refs["cornell"]
    g = rigs(c["scene"], force_global=force_global, stats=True)
    for lt in LIGHTS:
        for b in BOUNCES:
            g.lights(b, lt)
            g.k.reset_stats()
            res = g.trace(c["rays"], c["seeds"])
            assert g.k.scene_in_lds() == (not force_global)
            check(res, c[f"light{lt}"][b], f"light {lt} bounces {b}")
            assert g.counters() == c[f"light{lt}"][b]["counts"], (lt, b)
    g.lights(9, 0)
    for base in SEED_BASES:
        g.k.reset_stats()
        check(g.trace(c["rays"], seed_base=base), c[f"base{base}"][9], f"seed_base {base}")
        assert g.counters() == c[f"base{base}"][9]["counts"]
    # (seed_base is ignored when seeds are given)
    check(g.trace(c["rays"], c["seeds"], seed_base=777), c["light0"][9], "seeds over seed_base")
    for b in (2, 9):
        g.lights(b, 1)
        g.k.reset_stats()
        check(g.trace(c["windowed"], c["seeds"]), c["window"][b], f"[0, 5] window, bounces {b}")
        assert g.counters() == c["window"][b]["counts"]


@pytest.mark.parametrize("name", ["proxy", "soup"])
def test_pinned_equals_replay_on_other_scenes(refs, rigs, name):
    c = refs[name]
    g = rigs(c["scene"], stats=True)
    for b in BOUNCES:
        g.lights(b, 0)
        g.k.reset_stats()
        check(g.trace(c["rays"], c["seeds"]), c["light0"][b], f"{name} bounces {b}")
        assert g.counters() == c["light0"][b]["counts"]
    if name == "proxy":
        assert not g.k.scene_in_lds()
    g.lights(9, 2, 0.25)
    check(g.trace(c["rays"], c["seeds"]), c["light2"][9], f"{name} light 2, skybox 0.25")


# ---- 2: every math mode is tied to the render ---------------------------------------------------
@pytest.mark.parametrize("size", [(64, 36), (61, 7)], ids=["64x36", "61x7"])
@pytest.mark.parametrize("math_name", list(MATHS))
def test_camera_paths_continue_the_render(cornell, rigs, math_name, size):
    import path_ref
    W, H = size
    n = W * H
    g = rigs(cornell, math=MATHS[math_name], W=W, H=H, hits=True)

    def paths(frame, encoding):
        """the render of `frame`, then the trace over its camera paths"""
        g.ctx.WriteBuffer(g.r.out, np.zeros((n, 4), np.float32))
        g.r.frame(frame, light_bounces=9)
        image, (ids, _) = g.r.result(), g.r.hits()
        rb, sb, ob = g.buffer(n * 32), g.buffer(n * 4), g.buffer(n * 16)
        g.ctx.CameraPaths(g.k, n, rb, sb)
        g.ctx.TracePaths(g.k, rb, ob, n, seeds=sb, encoding=encoding)
        return image, ids, g.read(rb, n, N.RAY_DTYPE), g.read(sb, n, np.uint32), g.read(ob, n, N.PATH_RESULT_DTYPE)

    image, ids, rays, seeds, res = paths(0, N.TRACE_FRAME0)
    assert (ids >= 0).sum() >= 32 and (ids < 0).sum() >= 32   # (61x7 is a wide strip: 37 of 427 pixels hit)
    assert (bits(res["radiance"]) == bits(image[:, :3])).all()
    assert (res["prim"] == ids).all()
    # the records are rtEnqueueCameraRays' bytes, the seeds the double hash
    _, cam = g.camera_rays(n)
    assert cam.tobytes() == rays.tobytes()
    gid = np.arange(n, dtype=np.uint32)
    with np.errstate(over="ignore"):
        assert (seeds == path_ref.hash_u32(path_ref.hash_u32(gid + np.uint32(12345)))).all()   # frame_hash(0)
    if math_name == "pinned":
        _, _, _, _, lin = paths(0, N.TRACE_LINEAR)
        assert (lin["prim"] == ids).all()
        assert (bits(N.pinned_math("pow", lin["radiance"], np.float32(0.45454545))) == bits(res["radiance"])).all()
        image1, ids1, _, _, lin1 = paths(1, N.TRACE_LINEAR)
        assert (lin1["prim"] == ids1).all()
        assert (bits(N.pinned_math("pow", lin1["radiance"], np.float32(0.454545))) == bits(image1[:, :3])).all()


def test_camera_paths_continue_the_render_outside_lds(cornell, rigs):
    W, H = 64, 36
    n = W * H
    g = rigs(cornell, math=N.MATH_SHIPPED, force_global=True, W=W, H=H, hits=True)
    g.r.frame(0, light_bounces=9)
    image, (ids, _) = g.r.result(), g.r.hits()
    rb, sb, ob = g.buffer(n * 32), g.buffer(n * 4), g.buffer(n * 16)
    g.ctx.CameraPaths(g.k, n, rb, sb)
    g.ctx.TracePaths(g.k, rb, ob, n, seeds=sb, encoding=N.TRACE_FRAME0)
    res = g.read(ob, n, N.PATH_RESULT_DTYPE)
    assert not g.k.scene_in_lds()
    assert (bits(res["radiance"]) == bits(image[:, :3])).all() and (res["prim"] == ids).all()


# ---- 3: shapes where the kernel can go wrong ----------------------------------------------------
def test_ranges_keep_the_other_slots(refs, rigs):
    c = refs["cornell"]
    ref = want_bits(c["light0"][9])
    g = rigs(c["scene"])
    g.lights(9, 0)
    m = len(c["rays"])
    rb, sb = g.buffer(c["rays"].nbytes, c["rays"]), g.buffer(4 * m, c["seeds"])
    fill = np.full((m, 4), 0xFFFFFFFF, np.uint32)
    for first, n in ((0, 1), (0, 63), (0, 64), (0, 65), (3, 427), (1023, 65)):
        ob = g.buffer(fill.nbytes, fill)
        g.ctx.TracePaths(g.k, rb, ob, n, seeds=sb, first=first)
        out = g.read(ob, m * 4, np.uint32).reshape(m, 4)
        expect = fill.copy()
        expect[first:first + n] = ref[first:first + n]
        assert (out == expect).all(), (first, n)
    # the seed of record i is seed_base + i with the absolute index
    base = want_bits(c[f"base{SEED_BASES[1]}"][9])
    ob = g.buffer(fill.nbytes, fill)
    g.ctx.TracePaths(g.k, rb, ob, 427, seed_base=SEED_BASES[1], first=3)
    out = g.read(ob, m * 4, np.uint32).reshape(m, 4)
    assert (out[3:430] == base[3:430]).all() and (out[:3] == 0xFFFFFFFF).all() and (out[430:] == 0xFFFFFFFF).all()


def test_zero_bounces_and_miss_only_input(cornell, refs, rigs):
    c = refs["cornell"]
    g = rigs(cornell, stats=True)
    g.lights(0, 0)
    for enc in (N.TRACE_LINEAR, N.TRACE_FRAME0):
        res = g.trace(c["rays"][:130], c["seeds"][:130], encoding=enc)
        assert (bits(res["radiance"]) == 0).all() and (res["prim"] == -1).all()
    assert g.counters() == (0, 0, 0, 0)
    # rays that leave the scene's box at once: exactly the sky term in all three channels
    lo, hi = scene_box(cornell)
    rng = np.random.default_rng(3)
    d = np.abs(rng.standard_normal((200, 3))).astype(np.float32) + np.float32(0.1)
    rays = make_rays(np.tile(hi + np.float32(1.0), (200, 1)).astype(np.float32), d)
    for skybox in (1.0, 0.7):
        g.lights(9, 0, skybox)
        g.k.reset_stats()
        res = g.trace(rays, seed_base=1)
        s = np.float32(0.5) * np.float32(skybox)
        assert (res["prim"] == -1).all() and (bits(res["radiance"]) == bits(s)).all()
        assert g.counters()[0] == 200 and g.counters()[3] == 0


@pytest.mark.parametrize("force_global", [False, True], ids=["lds", "global"])
def test_degenerate_rays_end_with_the_querys_prim(cornell, rigs, force_global):
    rays = degenerate_rays(cornell)
    g = rigs(cornell, force_global=force_global)
    g.lights(9, 1)
    hits = g.query(rays)
    res = g.trace(rays, seed_base=99)
    assert (res["prim"] == hits["prim"]).all()
    assert (hits["prim"] >= 0).any() and (hits["prim"] < 0).any()
    inverted = rays["tmin"] > rays["tmax"]
    s = np.float32(0.5)
    assert inverted.any() and (bits(res["radiance"][inverted]) == bits(s)).all()


# ---- 4: queue behaviour ---------------------------------------------------------------------------
def test_trace_is_ordered_with_coalesced_frames(refs, rigs):
    c = refs["cornell"]
    images = []
    for with_trace in (False, True):
        g = rigs(c["scene"], W=128, H=72, perframe_batch=None)  # (the library default: frames coalesce)
        rb, sb = g.buffer(c["rays"].nbytes, c["rays"]), g.buffer(4 * len(c["rays"]), c["seeds"])
        ob = g.buffer(16 * len(c["rays"]))
        g.r.frame(1, light_bounces=9)
        g.r.frame(2, light_bounces=9)
        if with_trace:
            g.ctx.TracePaths(g.k, rb, ob, len(c["rays"]), seeds=sb)
        g.r.frame(3, light_bounces=9)
        g.r.frame(4, light_bounces=9)
        images.append(g.r.result())
        if with_trace:
            check(g.read(ob, len(c["rays"]), N.PATH_RESULT_DTYPE), c["light0"][9], "trace between queued frames")
    assert images[0][:, :3].any()
    assert images[0].tobytes() == images[1].tobytes()


def test_trace_after_a_refit_equals_a_cold_start(cornell, refs):
    from test_refit_gpu import Mover, new_positions
    c = refs["cornell"]
    rays, seeds = c["rays"][:512], c["seeds"][:512]

    def trace(r):
        r.k.set_int(N.LIGHT_BOUNCES, 9), r.k.set_int(N.LIGHT_TYPE, 0), r.k.set_float(N.SKYBOX_INTENSITY, 1.0)
        flags = N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR
        rb, sb = r.ctx.create_buffer(flags, rays.nbytes, rays), r.ctx.create_buffer(flags, seeds.nbytes, seeds)
        ob = r.ctx.create_buffer(N.MEM_READ_WRITE, 16 * len(rays))
        r.ctx.TracePaths(r.k, rb, ob, len(rays), seeds=sb)
        out = np.empty(len(rays), N.PATH_RESULT_DTYPE)
        r.ctx.ReadBuffer(ob, out, blocking=True)
        for b in (rb, sb, ob):
            b.release()
        return out

    m = Mover(cornell, 64, 8)
    try:
        before = trace(m)
        check(before, {k: v[:512] for k, v in c["light0"][9].items() if k != "counts"}, "before the move")
        assert m.k.scene_prepares() == (1, 0)
        m.move(new_positions(cornell))
        after = trace(m)
        assert m.k.scene_prepares() == (1, 1)
        moved = m.read_scene()
    finally:
        m.close()
    cold = Mover(moved, 64, 8)
    try:
        want = trace(cold)
        assert cold.k.scene_prepares() == (1, 0)
    finally:
        cold.close()
    assert result_bits(after).tobytes() == result_bits(want).tobytes()
    assert result_bits(after).tobytes() != result_bits(before).tobytes()


def test_errors_launch_nothing(cornell, refs, rigs):
    import clrt
    import stress_scenes as SS
    c = refs["cornell"]
    rays, seeds = c["rays"], c["seeds"]
    n = len(rays)
    g = rigs(cornell)
    g.lights(9, 0)
    other = rigs(cornell)
    rb, sb = g.buffer(rays.nbytes, rays), g.buffer(4 * n, seeds)
    fill = np.full(n * 4, 0x7fc12345, np.uint32)
    ob = g.buffer(fill.nbytes, fill)
    small_r, small_s, small_o = g.buffer(32 * 100), g.buffer(4 * 100), g.buffer(16 * 100)
    foreign = other.buffer(fill.nbytes, fill)
    lib, ctx, k = g.ctx._lib, g.ctx.handle, g.k.handle
    lin = N.TRACE_PARAMS(0, N.TRACE_LINEAR)

    def rc(kernel, r, s, first, count, params, o):
        return lib.rtEnqueueTracePaths(ctx, kernel, r.handle if r else None, s.handle if s else None, first, count,
                                       ctypes.byref(params) if params else None, o.handle if o else None)

    launches = g.k.stats()["launches"]
    bare = clrt.CLKernel(g.ctx, "KernelEntry")
    rows = [
        (rc(k, rb, sb, 0, n, None, ob), -30),                                   # params NULL
        (rc(k, None, sb, 0, n, None, None), -30),                               # ... before the buffers
        (rc(k, rb, sb, 0, n, N.TRACE_PARAMS(0, 2), ob), -30),                   # encoding
        (rc(k, rb, sb, 0, n, N.TRACE_PARAMS(0, -1), ob), -30),
        (rc(k, rb, sb, 1 << 31, 1, lin, ob), -30),                              # first + n > 2^31
        (rc(k, rb, sb, 5, (1 << 64) - 3, lin, ob), -30),                        # (a sum that would wrap)
        (rc(k, None, sb, 0, n, lin, ob), -38), (rc(k, rb, sb, 0, n, lin, None), -38),
        (rc(k, foreign, sb, 0, n, lin, ob), -38), (rc(k, rb, sb, 0, n, lin, foreign), -38),
        (rc(k, rb, foreign, 0, n, lin, ob), -38),                               # seeds of another context
        (rc(k, rb, sb, 0, n, lin, rb), -38), (rc(k, rb, sb, 0, n, lin, sb), -38),   # out is an input
        (rc(k, rb, sb, 0, n + 1, lin, rb), -38),                                # ... before the sizes
        (rc(k, small_r, sb, 0, 101, lin, ob), -61), (rc(k, rb, small_s, 0, 101, lin, ob), -61),
        (rc(k, rb, sb, 0, 101, lin, small_o), -61), (rc(k, rb, sb, 1, n, lin, ob), -61),
        (rc(k, rb, None, 0, 101, lin, small_o), -61),
        (rc(bare.handle, rb, sb, 0, n + 1, lin, ob), -61),                      # ... before the slots
        (rc(bare.handle, rb, sb, 0, n, lin, ob), -52),                          # scene, node, material unbound
    ]
    bare.set_buffer(N.BUFFER_SCENE, g.r.bufs[0])
    bare.set_buffer(N.BUFFER_NODE, g.r.bufs[1])
    rows.append((rc(bare.handle, rb, sb, 0, n, lin, ob), -52))                  # material unbound
    bare.set_buffer(N.BUFFER_MATERIAL, g.r.bufs[2])
    rows.append((rc(bare.handle, rb, sb, 0, n, lin, ob), -52))                  # light slots unset
    bare.set_int(N.LIGHT_BOUNCES, 9)
    bare.set_int(N.LIGHT_TYPE, 0)
    rows.append((rc(bare.handle, rb, sb, 0, 0, lin, ob), -52))                  # SKYBOX_INTENSITY unset, n == 0
    bare.set_float(N.SKYBOX_INTENSITY, 1.0)
    # a leaf of more than 127 triangles has no octant records: refused, not walked -- n == 0 included
    big = SS.soup_scene(12, "big")
    tb, nb = g.buffer(big.triangles.nbytes, big.triangles), g.buffer(big.nodes.nbytes, big.nodes)
    mb = g.buffer(big.materials.nbytes, big.materials)
    bare.set_buffer(N.BUFFER_SCENE, tb), bare.set_buffer(N.BUFFER_NODE, nb), bare.set_buffer(N.BUFFER_MATERIAL, mb)
    rows += [(rc(bare.handle, rb, sb, 0, n, lin, ob), -59), (rc(bare.handle, rb, sb, 0, 0, lin, ob), -59)]
    rows.append((rc(k, rb, sb, 0, 0, lin, ob), 0))                              # n == 0: no launch
    assert [r[0] for r in rows] == [r[1] for r in rows]
    assert g.k.stats()["launches"] == launches and bare.stats()["launches"] == 0
    assert (g.read(ob, n * 4, np.uint32) == fill).all()
    # camera paths: rtEnqueueCameraRays' errors and the seeds'
    cp = lib.rtEnqueueCameraPaths
    assert cp(ctx, k, 16, rb.handle, sb.handle) == -52                          # FRAME_COUNT / camera slots unset
    g.r.frame(1, light_bounces=1)
    assert cp(ctx, k, 0, rb.handle, sb.handle) == -63
    assert cp(ctx, k, n + 1, rb.handle, sb.handle) == -61 and cp(ctx, k, 101, rb.handle, small_s.handle) == -61
    assert cp(ctx, k, 16, rb.handle, None) == -38 and cp(ctx, k, 16, rb.handle, rb.handle) == -38
    assert cp(ctx, k, 16, rb.handle, foreign.handle) == -38
    # and the kernel that saw every error still works
    g.lights(9, 0)
    assert rc(k, rb, sb, 0, n, lin, ob) == 0
    check(g.read(ob, n, N.PATH_RESULT_DTYPE), c["light0"][9], "after the errors")
    assert g.k.stats()["launches"] == launches + 2
    bare.release()


# ---- 5: the Raytracer surface -------------------------------------------------------------------
def test_raytracer_trace_equals_low_level_path(cornell, refs):
    import clrt
    c = refs["cornell"]
    rt = clrt.Raytracer(CW, CH)
    rt.Init()
    try:
        rt.upload_scene(cornell)
        rt.kernel.set_math_mode(N.MATH_PINNED)
        rad, prim = rt.trace(c["rays"]["origin"], c["rays"]["dir"], seeds=c["seeds"])
        want = c["light0"][9]
        assert rad.dtype == np.float32 and rad.shape == (len(c["rays"]), 3) and prim.dtype == np.int32
        assert (bits(rad) == bits(want["radiance"])).all() and (prim == want["prim"]).all()
        rad, prim = rt.trace(c["rays"]["origin"], c["rays"]["dir"], seed_base=SEED_BASES[0])
        assert (bits(rad) == bits(c[f"base{SEED_BASES[0]}"][9]["radiance"])).all()
        rt.light_type = 1
        rad, prim = rt.trace(c["rays"]["origin"], c["rays"]["dir"], seeds=c["seeds"], tmin=0.0, tmax=5.0)
        assert (bits(rad) == bits(c["window"][9]["radiance"])).all() and (prim == c["window"][9]["prim"]).all()
        rt.light_type = 0
        rays, seeds = rt.camera_paths()   # frame_count 1: the fixture's camera records
        assert rays.tobytes() == c["rays"][512:].tobytes() and (seeds == c["seeds"][512:]).all()
        # frame 0 through the high-level calls equals RenderFrame's image
        rt.frame_count = 0
        rays, seeds = rt.camera_paths()
        rad, _ = rt.trace(rays["origin"], rays["dir"], seeds=seeds, encoding="frame0")
        rt.RenderFrame()
        assert (bits(rad) == bits(rt.pixels[:, :3])).all()
        assert rt.trace(np.zeros((0, 3)), np.zeros((0, 3)))[0].shape == (0, 3)
        with pytest.raises(ValueError):
            rt.trace(np.zeros((2, 3)), np.zeros((2, 3)), encoding="srgb")
    finally:
        rt.release()

"""GPU: shadow rays for the analytic light (rtKernelSetShadowRays) in rtEnqueueTracePaths and
rtEnqueueSamplePixels.

The reference for pinned math is tests/shadow_path_ref.py -- path_ref's replay of Render with the one change
rt_hip.h defines at kernel_bvh.cl:378 -- which test_shadow_path_ref.py pins to the plain replay and so to the
oracle.  The other math modes are tied to the library's own public calls: the closest-hit query, the surface
records and the any-hit query say per path whether the one shadow ray of a one-bounce path is occluded.

Inputs of the replay comparisons: the 32x18 camera paths of frame 1 plus 256 random rays, on Cornell (both scene
paths) and on soup_scene(12, "rt7") (zero-area and duplicate triangles).
"""
import os

import numpy as np
import pytest

from clrt import _native as N
from test_ray_query import MATHS, bits, make_rays, random_rays
from test_trace_paths import COUNTERS, TraceRig, check, result_bits

pytestmark = pytest.mark.gpu

BOUNCES, LIGHTS = (1, 3, 9), (0, 1, 2)
CW, CH = 32, 18
SEED_BASE = 0xFFFFFF00            # wraps past 2^32 inside the 832 records
LIGHT_L = (0.5, -0.4, 0.1)        # -lightDirection
SHORT_BOX_MATERIAL, BOX_SHIFT = 5, (-1.5, 0.5, 0.0)


@pytest.fixture
def rigs():
    made = []

    def make(*a, shadows=True, **kw):
        made.append(TraceRig(*a, **kw))
        made[-1].k.set_shadow_rays(shadows)
        return made[-1]

    yield make
    for g in made:
        g.close()


def floor_scene():
    """One floor quad at z = 0 in both windings (four triangles, every normal up) under an open sky: lit by the
    directional light, with nothing between it and the light."""
    import clrt.scene as S
    quad = np.float32([[-8, -8, 0], [8, -8, 0], [8, 8, 0], [-8, 8, 0]])
    tris = np.zeros(4, N.TRIANGLE_DTYPE)
    for i, (a, b, c) in enumerate(((0, 1, 2), (0, 2, 3), (0, 2, 1), (0, 3, 2))):
        for v, j in zip(("v1", "v2", "v3"), (a, b, c)):
            tris[v]["position"][i, :3] = quad[j]
            tris[v]["normal"][i, :3] = (0.0, 0.0, 1.0)
    mats = np.zeros(1, N.MATERIAL_DTYPE)
    mats["diffuse"][:, :3], mats["specular"][:, :3] = (0.7, 0.6, 0.5), (0.3, 0.3, 0.3)
    mats["roughness"], mats["ior"] = 0.5, 1.0
    return S.build_bvh(tris, mats, 4)


def floor_rays(n, seed=21):
    """n rays from above onto the floor's inner part"""
    rng = np.random.default_rng(seed)
    org = np.column_stack([rng.uniform(-6, 6, n), rng.uniform(-6, 6, n), rng.uniform(2, 9, n)]).astype(np.float32)
    d = np.column_stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), -np.ones(n)]).astype(np.float32)
    return make_rays(org, d)


# ---- references, computed once and shared (never modified) --------------------------------------
@pytest.fixture(scope="module")
def soup():
    import stress_scenes as SS
    return SS.soup_scene(12, "rt7")


@pytest.fixture(scope="module")
def floor():
    return floor_scene()


@pytest.fixture(scope="module")
def refs(cornell, soup, floor, oracle_mod):
    import path_ref
    import shadow_path_ref
    cam_rays, cam_seeds = path_ref.camera_paths(CW, CH, 1)
    out, jobs, keys = {}, [], []
    for name, scene in (("cornell", cornell), ("soup", soup)):
        rays = np.concatenate([cam_rays, random_rays(scene, 256, seed=11)])
        seeds = np.concatenate([cam_seeds, np.random.default_rng(5).integers(0, 2 ** 32, 256, dtype=np.uint32)])
        out[name] = {"scene": scene, "rays": rays, "seeds": seeds}
        for lt in LIGHTS if name == "cornell" else (0, 2):
            jobs.append((scene, rays, seeds, BOUNCES, lt, 1.0)), keys.append((name, f"light{lt}"))
    c = out["cornell"]
    n = len(c["rays"])
    based = ((SEED_BASE + np.arange(n, dtype=np.uint64)) & 0xffffffff).astype(np.uint32)
    jobs.append((cornell, c["rays"], based, (9,), 0, 1.0)), keys.append(("cornell", "base"))
    windowed = c["rays"].copy()
    windowed["tmin"], windowed["tmax"] = 0.0, 5.0
    c["windowed"] = windowed
    jobs.append((cornell, windowed, c["seeds"], (3,), 1, 1.0)), keys.append(("cornell", "window"))
    jobs.append((cornell, c["rays"], c["seeds"], (3,), 0, 1.0, False)), keys.append(("cornell", "off"))
    # the edge shapes: 64 rays onto the lit floor, and one of them among 63 that miss the scene
    # (of 200 candidates, the first 65 whose first bounce goes on and so casts a shadow ray)
    pool, pseeds = floor_rays(200), np.arange(100, 300, dtype=np.uint32)
    first = shadow_path_ref.ShadowPathTracer(floor).trace_rays(pool, pseeds, (1,), 0)[1]
    asks = np.flatnonzero(first["cast"] == 1)[:65]
    assert len(asks) == 65
    onto, fseeds = pool[asks], pseeds[asks]
    away = onto.copy()
    away["dir"][:, 2] = 1.0
    away[37] = onto[37]
    out["floor"] = {"scene": floor, "rays": onto, "one": away[:64], "seeds": fseeds}
    jobs.append((floor, onto, fseeds, (1, 9), 0, 1.0)), keys.append(("floor", "all"))
    jobs.append((floor, away[:64], fseeds[:64], (1, 9), 0, 1.0)), keys.append(("floor", "single"))
    done = shadow_path_ref.trace_rays_pool(jobs, procs=min(16, os.cpu_count() or 1))
    for (name, variant), res in zip(keys, done):
        out[name][variant] = res
    # before anything is compared: the inputs exercise both outcomes, and the shadow rays change results
    for lt in LIGHTS:
        cast, occluded = c[f"light{lt}"][3]["shadow"]
        assert occluded >= 30 and cast - occluded >= 30, (lt, cast, occluded)
    assert (bits(c["light0"][3]["radiance"]) != bits(c["off"][3]["radiance"])).any(axis=1).sum() >= 100
    assert out["soup"]["light0"][9]["shadow"][0] >= 30
    assert (out["floor"]["all"][1]["cast"] == 1).all() and out["floor"]["all"][9]["shadow"][1] == 0
    assert out["floor"]["single"][1]["cast"].tolist() == [int(i == 37) for i in range(64)]
    return out


def check_counted(g, res, ref, what):
    check(res, ref, what)
    assert g.counters() == ref["counts"], (what, g.counters(), ref["counts"])


# ---- 1: pinned math against the replay, bit for bit ---------------------------------------------
@pytest.mark.parametrize("force_global", [False, True], ids=["lds", "global"])
def test_pinned_equals_the_replay_on_cornell(refs, rigs, force_global):
    c = refs["cornell"]
    g = rigs(c["scene"], force_global=force_global, stats=True)
    for lt in LIGHTS:
        for b in BOUNCES:
            g.lights(b, lt)
            g.k.reset_stats()
            res = g.trace(c["rays"], c["seeds"])
            assert g.k.scene_in_lds() == (not force_global)
            check_counted(g, res, c[f"light{lt}"][b], f"light {lt} bounces {b}")
    g.lights(9, 0)
    g.k.reset_stats()
    check_counted(g, g.trace(c["rays"], seed_base=SEED_BASE), c["base"][9], "seed_base")
    g.lights(3, 1)
    g.k.reset_stats()
    check_counted(g, g.trace(c["windowed"], c["seeds"]), c["window"][3], "[0, 5] first-segment window")


def test_pinned_equals_the_replay_on_a_stress_soup(refs, rigs):
    c = refs["soup"]
    g = rigs(c["scene"], stats=True)
    for lt in (0, 2):
        for b in BOUNCES:
            g.lights(b, lt)
            g.k.reset_stats()
            check_counted(g, g.trace(c["rays"], c["seeds"]), c[f"light{lt}"][b], f"soup light {lt} bounces {b}")


def test_shadows_follow_a_refit(cornell, refs, oracle_mod):
    """The short box translated with rtEnqueueUpdateVertices + rtRefitBVH: the replay on the moved arrays."""
    import refit_ref
    import shadow_path_ref
    from test_refit_gpu import Mover
    c = refs["cornell"]
    rays, seeds = c["rays"][:CW * CH], c["seeds"][:CW * CH]

    def trace(m):
        m.k.set_int(N.LIGHT_BOUNCES, 3), m.k.set_int(N.LIGHT_TYPE, 0), m.k.set_float(N.SKYBOX_INTENSITY, 1.0)
        flags = N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR
        rb, sb = m.ctx.create_buffer(flags, rays.nbytes, rays), m.ctx.create_buffer(flags, seeds.nbytes, seeds)
        ob = m.ctx.create_buffer(N.MEM_READ_WRITE, 16 * len(rays))
        m.k.reset_stats()
        m.ctx.TracePaths(m.k, rb, ob, len(rays), seeds=sb)
        out = np.empty(len(rays), N.PATH_RESULT_DTYPE)
        m.ctx.ReadBuffer(ob, out, blocking=True)
        for b in (rb, sb, ob):
            b.release()
        return out, m.counters()

    pts = refit_ref.positions(cornell.triangles).copy()
    pts[cornell.triangles["mtlIndex"] == SHORT_BOX_MATERIAL] += np.float32(BOX_SHIFT)
    m = Mover(cornell, 64, 8, stats=True)
    try:
        m.k.set_shadow_rays(True)
        before, _ = trace(m)
        check(before, {k: v[:CW * CH] for k, v in c["light0"][3].items() if k in ("radiance", "prim")}, "before the move")
        m.move(pts)
        after, counts = trace(m)
        assert m.k.scene_prepares() == (1, 1)
        moved = m.read_scene()
    finally:
        m.close()
    want = shadow_path_ref.ShadowPathTracer(moved).trace_rays(rays, seeds, (3,), 0)[3]
    check(after, want, "after the move")
    assert counts == want["counts"]
    assert result_bits(after).tobytes() != result_bits(before).tobytes()
    assert want["shadow"][1] >= 30


# ---- 2: every math mode, through public calls only ----------------------------------------------
@pytest.mark.parametrize("math_name", list(MATHS))
def test_one_bounce_paths_agree_with_the_any_hit_query(cornell, rigs, math_name):
    W, H = 64, 36
    n = W * H
    g = rigs(cornell, math=MATHS[math_name], W=W, H=H)
    g.r.frame(1, light_bounces=1)          # every slot, the camera's among them (one small render)
    g.lights(1, 0)
    rb, sb, ob, hb, fb = g.buffer(n * 32), g.buffer(n * 4), g.buffer(n * 16), g.buffer(n * 16), g.buffer(n * 64)
    g.ctx.CameraPaths(g.k, n, rb, sb)
    g.ctx.TracePaths(g.k, rb, ob, n, seeds=sb)
    on = g.read(ob, n, N.PATH_RESULT_DTYPE)
    g.k.set_shadow_rays(False)
    g.ctx.TracePaths(g.k, rb, ob, n, seeds=sb)
    off = g.read(ob, n, N.PATH_RESULT_DTYPE)
    g.ctx.IntersectRays(g.k, rb, hb, n, N.QUERY_CLOSEST)
    g.ctx.HitSurfaces(g.k, rb, hb, fb, n)
    hits, surf = g.read(hb, n, N.RAY_HIT_DTYPE), g.read(fb, n, N.SURFACE_DTYPE)
    assert (hits["prim"] == on["prim"]).all() and (hits["prim"] == off["prim"]).all()
    shadow = make_rays(surf["position"], np.tile(np.float32(LIGHT_L), (n, 1)), 0.01, 100000.0)
    occluded = (g.query(shadow, any_hit=True)["prim"] >= 0) & (hits["prim"] >= 0)
    same = (bits(on["radiance"]) == bits(off["radiance"])).all(axis=1)
    assert same[~occluded].all()
    emission = cornell.materials["emission"][surf["material"] % len(cornell.materials), :3]
    E = (emission * np.float32(50.0)).astype(np.float32)
    differ = ~same
    assert (bits(on["radiance"][differ]) == bits(E[differ])).all()
    assert differ.sum() >= 100, differ.sum()


# ---- 3: off is off --------------------------------------------------------------------------------
@pytest.mark.parametrize("math_name", list(MATHS))
def test_off_after_on_is_a_fresh_kernel(refs, rigs, math_name):
    c = refs["cornell"]
    fresh = rigs(c["scene"], math=MATHS[math_name], stats=True, shadows=False)
    g = rigs(c["scene"], math=MATHS[math_name], stats=True)
    for r in (fresh, g):
        r.lights(9, 0)
    shadowed = g.trace(c["rays"], c["seeds"])
    g.k.set_shadow_rays(False)
    g.k.reset_stats()
    got, want = g.trace(c["rays"], c["seeds"]), fresh.trace(c["rays"], c["seeds"])
    assert result_bits(got).tobytes() == result_bits(want).tobytes()
    assert g.counters() == fresh.counters()
    assert result_bits(shadowed).tobytes() != result_bits(want).tobytes()
    if math_name == "pinned":
        off = refs["cornell"]
        g.lights(3, 0)
        check(g.trace(c["rays"], c["seeds"]), off["off"][3], "off equals the plain replay")


def test_fused_frames_do_not_read_the_setting(cornell, rigs):
    images = []
    for shadows in (False, True):
        g = rigs(cornell, math=N.MATH_SHIPPED, W=64, H=36, shadows=shadows)
        g.r.frame(1, light_bounces=9, n_frames=4)
        images.append(g.r.result())
    assert images[0][:, :3].any() and images[0].tobytes() == images[1].tobytes()


# ---- 4: nothing to occlude --------------------------------------------------------------------------
@pytest.mark.parametrize("math_name", list(MATHS))
def test_an_open_floor_keeps_every_bit(refs, rigs, math_name):
    f = refs["floor"]
    g = rigs(f["scene"], math=MATHS[math_name], stats=True)
    g.lights(9, 0)
    on, with_shadows = g.trace(f["rays"], f["seeds"]), g.counters()
    g.k.set_shadow_rays(False)
    g.k.reset_stats()
    off, without = g.trace(f["rays"], f["seeds"]), g.counters()
    assert result_bits(on).tobytes() == result_bits(off).tobytes()
    assert (on["prim"] >= 0).all() and on["radiance"].any()
    assert with_shadows[3] == without[3] and with_shadows[0] > without[0]
    if math_name == "pinned":
        cast, occluded = f["all"][9]["shadow"]
        assert occluded == 0 and with_shadows[0] - without[0] == cast and with_shadows == f["all"][9]["counts"]


# ---- 5: the fused sampler ---------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(61, 7), (64, 36)], ids=["61x7", "64x36"])
@pytest.mark.parametrize("math_name", list(MATHS))
def test_fused_sample_equals_the_three_calls_with_shadows(cornell, math_name, size):
    """(the 61 x 7 strip sees the scene in 37 pixels: the count of changed pixels is asserted at 64 x 36)"""
    import adaptive_ref as R
    from test_adaptive_gpu import AdaptRig
    from test_sample_pixels_gpu import FIRST, GUARD, both, composed, make_ids
    W, H = size
    px = W * H
    g = AdaptRig(cornell, math=MATHS[math_name], W=W, H=H)
    try:
        g.k.set_shadow_rays(True)
        got, want, st, body = both(g, W, H, seed=px, bounces=9)         # a host count
        assert got.tobytes() == want.tobytes() and want.tobytes() != st.tobytes()
        ids, n = make_ids(np.random.default_rng(px), px)                # a device count below n
        m = n - 70
        ib, cb = g.buffer(ids.nbytes, ids), g.buffer(16, np.array([m, 0, 0, 0], np.uint32))
        s1, s2 = g.buffer(st.nbytes, st), g.buffer(st.nbytes, st)
        g.ctx.SamplePixels(g.k, ib, n, px, s1, count=cb, first=FIRST)
        composed(g, ib, m, px, s2)
        fused = g.read(s1, px + GUARD, R.STATS)
        assert fused.tobytes() == g.read(s2, px + GUARD, R.STATS).tobytes() and fused.tobytes() != got.tobytes()
        if math_name == "pinned" and size == (64, 36):
            g.k.set_shadow_rays(False)
            plain, _, _, _ = both(g, W, H, seed=px, bounces=9)
            assert (got["sum"].view(np.uint32) != plain["sum"].view(np.uint32)).any(axis=1).sum() >= 30
    finally:
        g.close()


# ---- 6: edge shapes of the new phase ----------------------------------------------------------------
def test_one_record_and_a_partial_second_unit(refs, rigs):
    c = refs["cornell"]
    want = np.concatenate([bits(c["light0"][9]["radiance"]), c["light0"][9]["prim"].view(np.uint32)[:, None]], axis=1)
    g = rigs(c["scene"])
    g.lights(9, 0)
    m = len(c["rays"])
    rb, sb = g.buffer(c["rays"].nbytes, c["rays"]), g.buffer(4 * m, c["seeds"])
    fill = np.full((m, 4), 0xFFFFFFFF, np.uint32)
    for first, n in ((200, 1), (200, 65)):
        ob = g.buffer(fill.nbytes, fill)
        g.ctx.TracePaths(g.k, rb, ob, n, seeds=sb, first=first)
        expect = fill.copy()
        expect[first:first + n] = want[first:first + n]
        assert (g.read(ob, m * 4, np.uint32).reshape(m, 4) == expect).all(), (first, n)


@pytest.mark.parametrize("bounces", [1, 9])
def test_one_lane_and_all_lanes_of_a_wave_ask(refs, rigs, bounces):
    """LIGHT_BOUNCES 1: the shadow ray is the last thing a path does."""
    f = refs["floor"]
    g = rigs(f["scene"], stats=True)
    g.lights(bounces, 0)
    check_counted(g, g.trace(f["one"], f["seeds"][:64]), f["single"][bounces], "one lane of 64 asks")
    g.k.reset_stats()
    check_counted(g, g.trace(f["rays"], f["seeds"]), f["all"][bounces], "all lanes ask, and a 65th record")


def test_non_finite_shadow_rays_end(cornell, rigs):
    """Hits so far away that the point light's L overflows: the launch only has to end, with the query's prims."""
    rng = np.random.default_rng(4)
    d = rng.standard_normal((96, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    centre = np.float32([0.0, 0.0, 5.0])
    far = np.repeat(np.float32([1e18, 1e30, 3e38]), 32)[:, None]
    rays = make_rays((centre - d * far).astype(np.float32), d)
    g = rigs(cornell)
    hits = g.query(rays)
    for lt in (1, 2):
        g.lights(9, lt)
        res = g.trace(rays, seed_base=3)
        assert (res["prim"] == hits["prim"]).all()


# ---- 7: errors and getters ----------------------------------------------------------------------------
def test_errors_and_getters(cornell, rigs):
    import ctypes

    import clrt
    g = rigs(cornell, shadows=False)
    lib, k = g.ctx._lib, g.k.handle
    v = ctypes.c_int(-7)
    assert lib.rtKernelGetShadowRays(k, ctypes.byref(v)) == 0 and v.value == 0      # the default
    assert lib.rtKernelSetShadowRays(k, 1) == 0
    assert lib.rtKernelSetShadowRays(k, 2) == -30 and lib.rtKernelSetShadowRays(k, -1) == -30
    assert lib.rtKernelGetShadowRays(k, ctypes.byref(v)) == 0 and v.value == 1      # (an error keeps the value)
    assert lib.rtKernelGetShadowRays(k, None) == -30
    invalid_kernel = lib.rtKernelSetMathMode(None, N.MATH_PINNED)
    assert invalid_kernel != 0
    assert lib.rtKernelSetShadowRays(None, 1) == invalid_kernel
    assert lib.rtKernelGetShadowRays(None, ctypes.byref(v)) == invalid_kernel
    assert lib.rtKernelSetShadowRays(k, 0) == 0 and g.k.get_shadow_rays() is False
    g.k.set_shadow_rays(True)
    assert g.k.get_shadow_rays() is True
    rt = clrt.Raytracer(CW, CH)
    assert rt.shadow_rays is False
    rt.shadow_rays = True                  # before Init: applied when the kernel exists
    rt.Init()
    try:
        assert rt.shadow_rays is True and rt.kernel.get_shadow_rays() is True
        rt.shadow_rays = False
        assert rt.shadow_rays is False and rt.kernel.get_shadow_rays() is False
    finally:
        rt.release()


def test_raytracer_trace_follows_the_property(cornell, refs):
    import clrt
    c = refs["cornell"]
    rt = clrt.Raytracer(CW, CH)
    rt.Init()
    try:
        rt.upload_scene(cornell)
        rt.kernel.set_math_mode(N.MATH_PINNED)
        rt.light_bounces = 3
        rt.shadow_rays = True
        rad, prim = rt.trace(c["rays"]["origin"], c["rays"]["dir"], seeds=c["seeds"])
        assert (bits(rad) == bits(c["light0"][3]["radiance"])).all() and (prim == c["light0"][3]["prim"]).all()
        rt.shadow_rays = False
        rad, _ = rt.trace(c["rays"]["origin"], c["rays"]["dir"], seeds=c["seeds"])
        assert (bits(rad) == bits(c["off"][3]["radiance"])).all()
    finally:
        rt.release()

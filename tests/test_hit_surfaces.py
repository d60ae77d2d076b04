"""GPU: surface records of ray hits (rtEnqueueHitSurfaces) and first-hit feature buffers
(rtEnqueueFrameFeatures).

The reference for pinned math is tests/surface_ref.py, a numpy float32 restatement of the reference's hit
record (checked on the CPU in test_surface_plan.py); the other two math modes are held to it by bounds
measured on these inputs (MEASURED below); the feature buffers are held, bit for bit, to the
fold of the public per-frame calls and to the render path's primary hits.

Inputs, made once per module with pinned math and shared (never modified): per scene 2,048 random rays
(test_ray_query.random_rays) and their closest hits from rtEnqueueIntersectRays; Cornell also gets the
64x36 frame of camera rays, which brings the misses.  The fixture asserts at least 100 hits per set and at
least 100 misses in the camera frame before anything is compared.
"""
import numpy as np
import pytest

import surface_ref
from clrt import _native as N
from test_ray_query import MATHS, Rig, random_rays
from test_surface_plan import assert_known_answer, known_answer_case

pytestmark = pytest.mark.gpu

W, H = 64, 36
ODD = (61, 7)  # 427 work-items: a partial last workgroup
NAN_BYTE = 0xFF

# Largest difference from the pinned restatement per mode and field over the three input sets, as measured
# on an MI355X: normal and geo_normal by largest absolute component difference, position and
# texcoord by absolute difference over max(1, |origin|inf + |t|).  The tests assert 8x these: a guard
# against a wrong formula, not an accuracy claim.
MEASURED = {
    "devicelib": {"normal": 1.1920928955078125e-07, "geo_normal": 1.7881393432617188e-07,
                  "position": 1.3344801856048422e-07, "texcoord": 0.0},
    "shipped": {"normal": 1.7881393432617188e-07, "geo_normal": 1.7881393432617188e-07,
                "position": 1.2250571473846042e-07, "texcoord": 1.2417640002682211e-08},
}


def set_camera(k, frame_count):
    from hip_helpers import DEFAULT_CAMERA
    k.set_uint(N.FRAME_COUNT, frame_count)
    k.set_float3(N.CAMERA_POS, DEFAULT_CAMERA[0])
    k.set_float3(N.CAMERA_FRONT, DEFAULT_CAMERA[1])
    k.set_float3(N.CAMERA_UP, DEFAULT_CAMERA[2])


def surfaces_of(g, rays, hits, first=0, n=None):
    """rtEnqueueHitSurfaces over host arrays: the surface records read back."""
    rb = g.buffer(rays.nbytes, rays)
    hb = g.buffer(hits.nbytes, hits)
    sb = g.buffer(len(rays) * 64)
    g.ctx.HitSurfaces(g.k, rb, hb, sb, len(rays) if n is None else n, first)
    return g.read(sb, len(rays), N.SURFACE_DTYPE)


def same_bytes(got, want, what):
    a = np.ascontiguousarray(got).view(np.uint32).reshape(len(got), -1)
    b = np.ascontiguousarray(want).view(np.uint32).reshape(len(want), -1)
    bad = np.flatnonzero((a != b).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} of {len(got)} records differ, first {bad[:4]}: {got[bad[:2]]} vs {want[bad[:2]]}"


# ---- inputs and the pinned reference, once -------------------------------------------------------
@pytest.fixture(scope="module")
def proxy():
    import clrt.proxy as P
    return P.bunny_proxy()


@pytest.fixture(scope="module")
def soup():
    import stress_scenes as SS
    return SS.soup_scene(12, "rt7")


@pytest.fixture(scope="module")
def inputs(cornell, proxy, soup):
    """name -> (scene, rays, hits, reference surfaces)."""
    out = {}
    for name, scene in (("cornell", cornell), ("proxy", proxy), ("soup", soup)):
        g = Rig(scene, W=W, H=H)
        try:
            rays = random_rays(scene)
            if name == "cornell":
                set_camera(g.k, 1)
                _, cam = g.camera_rays(W * H)
                rays = np.concatenate([rays, cam])
            hits = g.query(rays)
        finally:
            g.close()
        hit = hits["prim"] >= 0
        assert hit.sum() >= 100, (name, int(hit.sum()))
        if name == "cornell":
            cam_hit = hit[2048:]
            assert (~cam_hit).sum() >= 100 and cam_hit.sum() >= 100, (int(cam_hit.sum()), cam_hit.size)
        out[name] = (scene, rays, hits, surface_ref.surfaces(scene.triangles, rays, hits))
    # the soup brings zero normals, zero-area triangles and real material indices into the hits
    _, _, hits, ref = out["soup"]
    hit = hits["prim"] >= 0
    assert (~ref["normal"][hit].any(axis=1)).any()
    assert len(set(ref["material"][hit].tolist())) >= 4
    _, _, hits, ref = out["proxy"]
    assert len({tuple(x) for x in ref["texcoord"][hits["prim"] >= 0].tolist()}) >= 50   # real uvs
    return out


@pytest.fixture
def rig_factory():
    rigs = []

    def make(*a, **kw):
        rigs.append(Rig(*a, **kw))
        return rigs[-1]

    yield make
    for g in rigs:
        g.close()


# ---- 1: pinned equals the restatement, all 64 bytes ----------------------------------------------
@pytest.mark.parametrize("force_global", [False, True], ids=["lds", "global"])
@pytest.mark.parametrize("name", ["cornell", "proxy", "soup"])
def test_pinned_equals_restatement(inputs, rig_factory, name, force_global):
    scene, rays, hits, ref = inputs[name]
    g = rig_factory(scene, force_global=force_global, W=W, H=H)
    rb = g.buffer(rays.nbytes, rays)
    hb = g.buffer(len(rays) * 16)
    sb = g.buffer(len(rays) * 64)
    g.ctx.IntersectRays(g.k, rb, hb, len(rays))
    g.ctx.HitSurfaces(g.k, rb, hb, sb, len(rays))        # hits in, surfaces out: nothing leaves the device
    same_bytes(g.read(hb, len(rays), N.RAY_HIT_DTYPE), hits, f"{name} hits")
    if name == "cornell":
        assert g.k.scene_in_lds() == (not force_global)
    elif name == "proxy" or force_global:
        assert not g.k.scene_in_lds()
    same_bytes(g.read(sb, len(rays), N.SURFACE_DTYPE), ref, name)


def test_synthetic_hits_on_every_soup_triangle(soup, rig_factory):
    """Nothing is intersected again, so hit records can name triangles no ray would hit: every triangle of
    the soup -- the zero-area ones (culled by the walk) and the exact duplicates included -- at fixed
    barycentrics.  A zero-area triangle whose cross product is exactly zero gives the zero geo_normal."""
    n = len(soup.triangles)
    rng = np.random.default_rng(3)
    rays = random_rays(soup, n, seed=9)
    hits = np.zeros(n, N.RAY_HIT_DTYPE)
    hits["prim"] = np.arange(n)
    hits["t"] = rng.uniform(-2, 30, n).astype(np.float32)
    hits["u"] = rng.uniform(0, 0.5, n).astype(np.float32)
    hits["v"] = rng.uniform(0, 0.5, n).astype(np.float32)
    ref = surface_ref.surfaces(soup.triangles, rays, hits)
    flat = (soup.triangles["v3"]["position"] == soup.triangles["v2"]["position"]).all(axis=1)
    assert flat.sum() >= 8 and not ref["geo_normal"][flat].any() and ref["geo_normal"][~flat].any(axis=1).all()
    assert (~ref["normal"].any(axis=1)).sum() >= 20          # the normals of scale 0
    g = rig_factory(soup, W=W, H=H)
    same_bytes(surfaces_of(g, rays, hits), ref, "every soup triangle")


# ---- 2: known answer in all three math modes -----------------------------------------------------
@pytest.mark.parametrize("math_name", list(MATHS))
def test_known_answer(rig_factory, math_name):
    """Exact in all three modes: recorded on an MI355X, the hardware rsq path of devicelib and shipped
    returns rsqrt(1) = 1, rsqrt(16) = 1/4 and rsqrt(64) = 1/8 exactly, so they are held to pinned's answer."""
    scene, rays, hits, exact = known_answer_case()
    g = rig_factory(scene, math=MATHS[math_name])
    got_hits = g.query(rays)
    same_bytes(got_hits, hits, f"{math_name} hits")
    surf = surfaces_of(g, rays, got_hits)
    inexact = [(i, s) for i, (s, e) in enumerate(zip(surf, exact)) if e and
               tuple(map(float, s["normal"])) + tuple(map(float, s["geo_normal"])) !=
               tuple(map(float, e[5])) + tuple(map(float, e[6]))]
    print(math_name, "inexact normals:", inexact[:4])
    assert_known_answer(surf, exact, math_name)


# ---- 3: devicelib and shipped against the pinned restatement -------------------------------------
def differences(got, ref, rays):
    """field -> the largest difference as the module docstring defines it; the exact fields asserted."""
    for f in ("prim", "t", "material", "reserved"):
        assert got[f].tobytes() == ref[f].tobytes(), f
    hit = ref["prim"] >= 0
    assert not got[~hit].view(np.uint32).reshape(-1, 16)[:, [0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14, 15]].any()
    g64 = {f: got[f][hit].astype(np.float64) for f in ("normal", "geo_normal", "position", "texcoord")}
    r64 = {f: ref[f][hit].astype(np.float64) for f in g64}
    scale = np.maximum(1.0, np.abs(rays["origin"][hit]).max(axis=1).astype(np.float64) + np.abs(ref["t"][hit]))
    out = {}
    for f in g64:
        assert np.isfinite(g64[f]).all() == np.isfinite(r64[f]).all(), f
        d = np.abs(g64[f] - r64[f])
        d[~np.isfinite(r64[f])] = 0.0
        if f in ("position", "texcoord"):
            d = d / scale[:, None]
        out[f] = float(d.max())
    return out


@pytest.mark.parametrize("math_name", ["devicelib", "shipped"])
def test_other_modes_stay_near_pinned(inputs, rig_factory, math_name):
    worst = {}
    for name, (scene, rays, hits, ref) in inputs.items():
        g = rig_factory(scene, math=MATHS[math_name], W=W, H=H)
        d = differences(surfaces_of(g, rays, hits), ref, rays)
        print(math_name, name, d)
        for f, v in d.items():
            worst[f] = max(worst.get(f, 0.0), v)
    print(math_name, "worst", worst)
    for f, v in worst.items():
        assert v <= 8 * MEASURED[math_name][f], (math_name, f, v, MEASURED[math_name][f])


# ---- 4: features equal the fold of the public per-frame calls ------------------------------------
def per_frame(g, n, frames, set_frame=True):
    """frame -> (hits, surfaces) through rtEnqueueCameraRays, rtEnqueueIntersectRays, rtEnqueueHitSurfaces
    (set_frame False: at the FRAME_COUNT the kernel holds)."""
    rb, hb, sb = g.buffer(n * 32), g.buffer(n * 16), g.buffer(n * 64)
    out = {}
    for f in frames:
        if set_frame:
            set_camera(g.k, f)
        g.ctx.CameraRays(g.k, n, rb)
        g.ctx.IntersectRays(g.k, rb, hb, n)
        g.ctx.HitSurfaces(g.k, rb, hb, sb, n)
        out[f] = (g.read(hb, n, N.RAY_HIT_DTYPE), g.read(sb, n, N.SURFACE_DTYPE))
    return out


def features_of(g, n, f0, n_frames):
    fb = g.buffer(n * 32, np.full(n * 32, NAN_BYTE, np.uint8))   # NaN bytes: the buffer is never read
    set_camera(g.k, f0)
    g.ctx.FrameFeatures(g.k, n, n_frames, fb)
    return g.read(fb, n, N.PIXEL_FEATURES_DTYPE)


@pytest.mark.parametrize("size", [(W, H), ODD], ids=["64x36", "61x7"])
@pytest.mark.parametrize("scene_name", ["cornell", "proxy"])
@pytest.mark.parametrize("math_name", list(MATHS))
def test_features_equal_fold_of_per_frame_calls(cornell, proxy, rig_factory, math_name, scene_name, size):
    scene = cornell if scene_name == "cornell" else proxy
    n = size[0] * size[1]
    g = rig_factory(scene, math=MATHS[math_name], W=size[0], H=size[1])
    frames = per_frame(g, n, range(0, 13))
    for f0 in (0, 5):
        for nf in (1, 3, 8):
            got = features_of(g, n, f0, nf)
            want = surface_ref.fold_features([frames[f0 + i] for i in range(nf)], scene.materials, nf)
            same_bytes(got, want, f"{math_name} {scene_name} {size} f0={f0} n={nf}")
            assert 0 < (got["coverage"] > 0).sum() and (got["coverage"] == 0).sum() > 0
    # the FRAME_COUNT slot is unchanged: the kernel still generates frame 5's rays
    same_bytes(per_frame(g, n, [5], set_frame=False)[5][0], frames[5][0], "FRAME_COUNT after the features")


def test_features_frame_count_wraps(cornell, rig_factory):
    n = ODD[0] * ODD[1]
    g = rig_factory(cornell, W=ODD[0], H=ODD[1])
    order = (0xFFFFFFFE, 0xFFFFFFFF, 0)
    frames = per_frame(g, n, order)
    got = features_of(g, n, order[0], 3)
    same_bytes(got, surface_ref.fold_features([frames[f] for f in order], cornell.materials, 3), "wrap")


# ---- 5: features tie to the render path ----------------------------------------------------------
@pytest.mark.parametrize("scene_name,nf", [("cornell", 8), ("proxy", 3)])
@pytest.mark.parametrize("math_name", list(MATHS))
def test_features_tie_to_render_path(cornell, proxy, rig_factory, math_name, scene_name, nf):
    scene = cornell if scene_name == "cornell" else proxy
    n, f0 = W * H, 2
    g = rig_factory(scene, math=MATHS[math_name], W=W, H=H, hits=True)
    count = np.zeros(n, np.float32)
    depth = np.zeros(n, np.float32)
    for f in range(f0, f0 + nf):
        g.r.frame(f, light_bounces=1)                    # one launch per frame, primary hits bound
        ids, t = g.r.hits()
        hit = ids >= 0
        count[hit] = count[hit] + np.float32(1)
        depth[hit] = depth[hit] + t[hit]
    got = features_of(g, n, f0, nf)
    inv = np.float32(1) / np.float32(nf)
    assert (count == nf).any() and (count == 0).any() and ((count > 0) & (count < nf)).any()
    assert np.rint(got["coverage"].astype(np.float64) * nf).tolist() == count.tolist()
    assert got["coverage"].tobytes() == (count * inv).tobytes()
    assert got["depth"].tobytes() == (depth * inv).tobytes()


# ---- 6: out-of-range prim ------------------------------------------------------------------------
def test_out_of_range_prim_is_a_miss(inputs, rig_factory):
    scene, rays, hits, ref = inputs["cornell"]
    n_tris = len(scene.triangles)
    edited = hits.copy()
    victims = np.flatnonzero(hits["prim"] >= 0)[[3, 40, 41, 90, 300]]
    edited["prim"][victims] = [-2, n_tris, 0x7FFFFFFF, -0x80000000, n_tris + 1]
    g = rig_factory(scene, W=W, H=H)
    got = surfaces_of(g, rays, edited)
    want = ref.copy()
    for f in ("position", "normal", "geo_normal", "texcoord"):
        want[f][victims] = 0
    want["prim"][victims] = -1
    want["material"][victims] = 0xFFFFFFFF
    same_bytes(got, want, "edited prims")                          # the victims' neighbours are unchanged
    same_bytes(got, surface_ref.surfaces(scene.triangles, rays, edited), "restatement of the edited hits")
    assert (got["t"][victims] == hits["t"][victims]).all()
    last = np.flatnonzero(hits["prim"] == n_tris - 1)
    assert last.size and (got["prim"][last] == n_tris - 1).all()   # the last triangle is still a hit


# ---- 7: after a refit ----------------------------------------------------------------------------
def test_surfaces_after_refit(cornell):
    import clrt
    rays = random_rays(cornell)
    rng = np.random.default_rng(5)
    tris = cornell.triangles.copy()
    pos = np.stack([tris[v]["position"][:, :3] for v in ("v1", "v2", "v3")], axis=1)
    nrm = np.stack([tris[v]["normal"][:, :3] for v in ("v1", "v2", "v3")], axis=1)
    new_pos = (pos * np.float32(1.125) + rng.normal(0, 0.05, pos.shape)).astype(np.float32)
    new_nrm = (nrm * np.float32(3.0) + rng.normal(0, 0.3, nrm.shape)).astype(np.float32)
    for i, v in enumerate(("v1", "v2", "v3")):
        tris[v]["position"][:, :3] = new_pos[:, i]
        tris[v]["normal"][:, :3] = new_nrm[:, i]
    rt = clrt.Raytracer(64, 8)
    rt.Init()
    try:
        rt.kernel.set_math_mode(N.MATH_PINNED)
        rt.upload_scene(cornell)
        hits0, surf0 = rt.surfaces(rays["origin"], rays["dir"])
        same_bytes(surf0, surface_ref.surfaces(cornell.triangles, rays, hits0), "before the move")
        full, refits = rt.kernel.scene_prepares()
        rt.move_vertices(new_pos, new_nrm)
        hits, surf = rt.surfaces(rays["origin"], rays["dir"])
        assert rt.kernel.scene_prepares() == (full, refits + 1)
        assert (hits["prim"] >= 0).sum() >= 100 and hits.tobytes() != hits0.tobytes()
        same_bytes(surf, surface_ref.surfaces(tris, rays, hits), "after the move")
    finally:
        rt.release()


# ---- 8: errors -----------------------------------------------------------------------------------
def test_errors_and_untouched_slots(inputs, cornell, rig_factory):
    import clrt
    import stress_scenes as SS
    scene, rays, hits, ref = inputs["cornell"]
    rays, hits, ref = rays[:2048], hits[:2048], ref[:2048]
    n = len(rays)
    g = rig_factory(scene, W=W, H=H)
    other = rig_factory(scene, W=W, H=H)
    lib, ctx, k = g.ctx._lib, g.ctx.handle, g.k.handle
    rb, hb = g.buffer(rays.nbytes, rays), g.buffer(hits.nbytes, hits)
    sentinel = np.full(n * 16, 0x7FC12345, np.uint32)
    sb = g.buffer(sentinel.nbytes, sentinel)
    small = g.buffer(64 * 100)
    foreign = other.buffer(n * 64)

    def rc(kernel, r, h, first, cnt, s):
        return lib.rtEnqueueHitSurfaces(ctx, kernel, r.handle, h.handle, first, cnt,
                                        s.handle if s is not None else None)

    g.k.set_timing(True)
    g.k.reset_stats()
    assert rc(k, rb, hb, 1 << 31, 1, sb) == -30                       # first + n > 2^31
    assert rc(k, rb, hb, 5, (1 << 64) - 3, sb) == -30                 # (a sum that would wrap)
    assert rc(k, rb, hb, 1 << 31, 1, None) == -30                     # ... checked before the output
    assert rc(k, rb, hb, 0, n, rb) == -38 and rc(k, rb, hb, 0, n, hb) == -38   # surfaces is an input
    assert rc(k, rb, hb, 0, n, foreign) == -38 and rc(k, rb, hb, 0, n, None) == -38
    assert rc(k, rb, rb, 0, n, sb) == -38                             # rays == hits
    assert rc(k, rb, hb, 0, 101, small) == -61                        # beyond the surfaces
    assert rc(k, rb, hb, 1, n, sb) == -61                             # beyond rays / hits
    assert rc(k, rb, small, 0, 401, sb) == -61                        # beyond a short hit buffer (6,400 B)
    bare = clrt.CLKernel(g.ctx, "KernelEntry")
    assert rc(bare.handle, rb, hb, 0, n, sb) == -52                   # no scene / node buffer
    assert rc(bare.handle, rb, hb, 0, 0, sb) == -52                   # ... checked before n == 0
    assert rc(bare.handle, rb, hb, 0, 101, small) == -61              # ... and after the sizes
    bare.set_buffer(N.BUFFER_SCENE, g.r.bufs[0])
    assert rc(bare.handle, rb, hb, 0, n, sb) == -52
    assert rc(k, rb, hb, 0, 0, sb) == 0 and rc(k, rb, hb, 7, 0, sb) == 0   # n == 0: no launch
    assert g.k.stats()["launches"] == 0
    assert (g.read(sb, n * 16, np.uint32) == sentinel).all()          # nothing was launched so far

    # frame features
    def fc(kernel, gws, nf, f):
        return lib.rtEnqueueFrameFeatures(ctx, kernel, gws, nf, f.handle if f is not None else None)

    fb = g.buffer(W * H * 32, np.full(W * H * 32, NAN_BYTE, np.uint8))
    set_camera(g.k, 1)
    assert fc(k, W * H, 0, fb) == -30 and fc(k, W * H, 4097, fb) == -30
    assert fc(k, 0, 1, fb) == -63 and fc(k, 1 << 32, 1, fb) == -63
    assert fc(k, W * H + 1, 1, fb) == -61
    assert fc(k, W * H, 1, None) == -38 and fc(k, W * H, 1, foreign) == -38
    assert fc(bare.handle, W * H, 1, fb) == -52                       # no WIDTH / camera / node / material
    bare.set_buffer(N.BUFFER_NODE, g.r.bufs[1])
    bare.set_int(N.WIDTH, W)
    bare.set_int(N.HEIGHT, H)
    set_camera(bare, 1)
    assert fc(bare.handle, W * H, 1, fb) == -52                       # the material slot alone is unbound
    bare.set_buffer(N.BUFFER_MATERIAL, g.r.bufs[2])
    bare.set_int(N.WIDTH, 0)
    assert fc(bare.handle, W * H, 1, fb) == -52                       # WIDTH zero
    bare.set_int(N.WIDTH, W)
    big = SS.soup_scene(12, "big")                                    # a leaf of more than 127 triangles
    tb, nb = g.buffer(big.triangles.nbytes, big.triangles), g.buffer(big.nodes.nbytes, big.nodes)
    mb = g.buffer(big.materials.nbytes, big.materials)
    bare.set_buffer(N.BUFFER_SCENE, tb)
    bare.set_buffer(N.BUFFER_NODE, nb)
    bare.set_buffer(N.BUFFER_MATERIAL, mb)
    assert fc(bare.handle, W * H, 1, fb) == -59
    assert (g.read(fb, W * H * 32, np.uint8) == NAN_BYTE).all()       # nothing was launched
    assert g.k.stats()["launches"] == 0
    with pytest.raises(clrt.RTError):
        g.ctx.HitSurfaces(g.k, rb, hb, rb, n)
    with pytest.raises(clrt.RTError):
        g.ctx.FrameFeatures(g.k, W * H, 0, fb)

    # a range inside the buffers: the other slots keep the sentinel; timing counts the launch
    for first, cnt in ((0, 1), (1, 255), (255, 257), (1000, 1048)):
        sb2 = g.buffer(sentinel.nbytes, sentinel)
        before = g.k.stats()
        assert rc(k, rb, hb, first, cnt, sb2) == 0
        got = g.read(sb2, n * 16, np.uint32).reshape(n, 16)
        want = sentinel.reshape(n, 16).copy()
        want[first:first + cnt] = ref[first:first + cnt].view(np.uint32).reshape(-1, 16)
        assert (got == want).all(), (first, cnt)
        after = g.k.stats()
        assert after["launches"] == before["launches"] + 1 and after["kernel_ms"] > before["kernel_ms"]
    # a kernel without a material buffer answers; the kernel that saw every error still works
    bare.release()
    bare = clrt.CLKernel(g.ctx, "KernelEntry")
    bare.set_buffer(N.BUFFER_SCENE, g.r.bufs[0])
    bare.set_buffer(N.BUFFER_NODE, g.r.bufs[1])
    bare.set_math_mode(N.MATH_PINNED)
    assert rc(bare.handle, rb, hb, 0, n, sb) == 0
    same_bytes(g.read(sb, n, N.SURFACE_DTYPE), ref, "kernel without materials")
    bare.release()
    assert rc(k, rb, hb, 0, n, sb) == 0
    same_bytes(g.read(sb, n, N.SURFACE_DTYPE), ref, "after the errors")


def test_surfaces_are_ordered_behind_coalesced_frames(inputs, rig_factory):
    scene, rays, hits, ref = inputs["cornell"]
    images = []
    for with_surfaces in (False, True):
        g = rig_factory(scene, W=128, H=72, perframe_batch=None)   # (the library default: frames coalesce)
        rb, hb, sb = g.buffer(rays.nbytes, rays), g.buffer(hits.nbytes, hits), g.buffer(len(rays) * 64)
        for f in range(1, 5):
            g.r.frame(f, light_bounces=2)
        if with_surfaces:
            g.ctx.HitSurfaces(g.k, rb, hb, sb, len(rays))
        images.append(g.r.result())
        if with_surfaces:
            same_bytes(g.read(sb, len(rays), N.SURFACE_DTYPE), ref, "behind four queued frames")
    assert images[0][:, :3].any() and images[0].tobytes() == images[1].tobytes()


# ---- 9: the Raytracer surface --------------------------------------------------------------------
def test_raytracer_surfaces_and_features_equal_low_level_path(inputs, cornell):
    import clrt
    _, rays, hits, ref = inputs["cornell"]
    rt = clrt.Raytracer(61, 7)
    rt.Init()
    try:
        rt.upload_scene(cornell)
        rt.kernel.set_math_mode(N.MATH_PINNED)
        got_hits, got = rt.surfaces(rays["origin"], rays["dir"])
        assert got_hits.dtype == N.RAY_HIT_DTYPE and got.dtype == N.SURFACE_DTYPE
        same_bytes(got_hits, hits, "Raytracer.surfaces hits")
        same_bytes(got, ref, "Raytracer.surfaces")
        part_hits, part = rt.surfaces(rays["origin"][:100], rays["dir"][:100])    # the kept buffers, reused
        same_bytes(part, ref[:100], "a shorter call")
        empty = rt.surfaces(np.zeros((0, 3)), np.zeros((0, 3)))
        assert len(empty[0]) == 0 and len(empty[1]) == 0
        same_bytes(rt.cast(rays["origin"], rays["dir"]), hits, "cast is unchanged")
        rt.frame_count = 5
        feat = rt.features(3)
        assert feat.shape == (7, 61) and feat.dtype == N.PIXEL_FEATURES_DTYPE and rt.frame_count == 5
        n = 61 * 7
        fb = rt.ctx.create_buffer(N.MEM_READ_WRITE, n * 32)
        rt.ctx.FrameFeatures(rt.kernel, n, 3, fb)
        low = np.empty(n, N.PIXEL_FEATURES_DTYPE)
        rt.ctx.ReadBuffer(fb, low, blocking=True)
        fb.release()
        same_bytes(feat.reshape(-1), low, "Raytracer.features")
        assert (feat["coverage"] > 0).any() and (rt.features()["coverage"] <= 1).all()
    finally:
        rt.release()

"""GPU: batched ray queries over caller rays (rtEnqueueIntersectRays, rtEnqueueCameraRays).

The reference for arbitrary rays is tests/ray_query_ref.py, a replay of the oracle's stack walk
through the oracle's own probes; the render path -- bit-exact with the live reference in every math
mode -- is the reference for the camera's rays.

The random ray set (RAYS: 2,048 rays from default_rng(7), origins uniform in the scene's bounding
box, directions standard normal and not unit length) was checked with the helper alone on the CPU.
On Cornell: hit share 0.845 unbounded and 0.402 with [tmin, tmax] = [0, 5]; 27 closest hits with a
negative t; any-hit prim differs from closest prim for 610 of 2,048 rays.  The tests assert those
input conditions before they compare anything.
"""
from fractions import Fraction

import numpy as np
import pytest

from clrt import _native as N

pytestmark = pytest.mark.gpu

INF = float("inf")
N_RAYS = 2048
MATHS = {"pinned": N.MATH_PINNED, "devicelib": N.MATH_DEVICELIB, "shipped": N.MATH_SHIPPED}


# ---- rays ---------------------------------------------------------------------------------------
def scene_box(scene):
    p = np.concatenate([scene.triangles[v]["position"][:, :3] for v in ("v1", "v2", "v3")])
    return p.min(axis=0), p.max(axis=0)


def make_rays(origins, dirs, tmin=-INF, tmax=100000.0):
    r = np.zeros(len(origins), N.RAY_DTYPE)
    r["origin"], r["dir"] = origins, dirs
    r["tmin"], r["tmax"] = tmin, tmax
    return r


def random_rays(scene, n=N_RAYS, tmin=-INF, tmax=100000.0, seed=7):
    rng = np.random.default_rng(seed)
    lo, hi = scene_box(scene)
    origins = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    dirs = rng.standard_normal((n, 3)).astype(np.float32)
    return make_rays(origins, dirs, tmin, tmax)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the device side ----------------------------------------------------------------------------
class Rig:
    """A HipRenderer (context, kernel, bound scene) plus ray and hit buffers made on demand."""

    def __init__(self, scene, math=N.MATH_PINNED, force_global=False, stats=False, W=64, H=8, hits=False,
                 perframe_batch=1):
        from hip_helpers import HipRenderer
        self.r = HipRenderer(scene, W, H, math=math, force_global=force_global, stats=stats, hits=hits,
                             perframe_batch=perframe_batch)
        self.ctx, self.k = self.r.ctx, self.r.k
        self._bufs = []

    def buffer(self, nbytes, host=None):
        if host is None:
            b = self.ctx.create_buffer(N.MEM_READ_WRITE, nbytes)
        else:
            b = self.ctx.create_buffer(N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR, nbytes, host)
        self._bufs.append(b)
        return b

    def read(self, buf, n, dtype):
        out = np.empty(n, dtype)
        self.ctx.ReadBuffer(buf, out, blocking=True)
        return out

    def query(self, rays, any_hit=False):
        rb = self.buffer(rays.nbytes, rays)
        hb = self.buffer(len(rays) * 16)
        self.ctx.IntersectRays(self.k, rb, hb, len(rays), N.QUERY_ANY if any_hit else N.QUERY_CLOSEST)
        return self.read(hb, len(rays), N.RAY_HIT_DTYPE)

    def camera_rays(self, n):
        rb = self.buffer(n * 32)
        self.ctx.CameraRays(self.k, n, rb)
        return rb, self.read(rb, n, N.RAY_DTYPE)

    def close(self):
        self.ctx.Finish()
        for b in self._bufs:
            b.release()
        self.r.close()


@pytest.fixture
def rig_factory():
    rigs = []

    def make(*a, **kw):
        rigs.append(Rig(*a, **kw))
        return rigs[-1]

    yield make
    for g in rigs:
        g.close()


# ---- references, computed once and shared (never modified) --------------------------------------
@pytest.fixture(scope="module")
def proxy():
    import clrt.proxy as P
    return P.bunny_proxy()


@pytest.fixture(scope="module")
def walkers(cornell, proxy, oracle_mod):
    from ray_query_ref import SceneWalker
    return {"cornell": SceneWalker(cornell), "proxy": SceneWalker(proxy)}


@pytest.fixture(scope="module")
def cornell_ref(cornell, walkers):
    """rays and the helper's (prim, t, visits, tests) per (range, mode) on Cornell, with the input
    conditions the comparisons rest on."""
    w = walkers["cornell"]
    out = {}
    for name, (tmin, tmax) in {"unbounded": (-INF, 100000.0), "ranged": (0.0, 5.0)}.items():
        rays = random_rays(cornell, tmin=tmin, tmax=tmax)
        out[name] = {"rays": rays, "closest": w.walk_rays(rays), "any": w.walk_rays(rays, any_hit=True)}
    pc, tc = out["unbounded"]["closest"][:2]
    pa = out["unbounded"]["any"][0]
    assert 0.2 <= (pc >= 0).mean() <= 0.95 and 0.2 <= (out["ranged"]["closest"][0] >= 0).mean() <= 0.95
    assert ((pc >= 0) & (tc < 0)).sum() >= 1          # Intersect's negative-t hits are in the set
    assert (pa != pc).mean() >= 0.10                  # any-hit is not closest-hit in disguise
    return out


def check_against(hits, ref, rays, what):
    prim, t = ref[0], ref[1]
    bad = np.flatnonzero(hits["prim"] != prim)
    assert bad.size == 0, f"{what}: {bad.size} prims differ, first ray {bad[:5]}: {hits['prim'][bad[:5]]} vs {prim[bad[:5]]}"
    bad = np.flatnonzero(bits(hits["t"]) != bits(t))
    assert bad.size == 0, f"{what}: {bad.size} t differ in bits, first ray {bad[:5]}: {hits['t'][bad[:5]]} vs {t[bad[:5]]}"
    miss = hits["prim"] < 0
    assert (bits(hits["t"][miss]) == bits(rays["tmax"][miss])).all(), f"{what}: a miss must keep tmax"
    assert not hits["u"][miss].any() and not hits["v"][miss].any(), f"{what}: a miss has u = v = 0"


# ---- 1, 2: pinned math equals the oracle walk ---------------------------------------------------
@pytest.mark.parametrize("force_global", [False, True], ids=["lds", "global"])
def test_pinned_equals_oracle_walk_on_cornell(cornell, cornell_ref, rig_factory, force_global):
    g = rig_factory(cornell, force_global=force_global, stats=True)
    for rng_name, ref in cornell_ref.items():
        for mode in ("closest", "any"):
            g.k.reset_stats()
            hits = g.query(ref["rays"], any_hit=mode == "any")
            assert g.k.scene_in_lds() == (not force_global)
            check_against(hits, ref[mode], ref["rays"], f"{rng_name} {mode}")
            st = g.k.stats()
            assert (st["rays"], st["node_visits"], st["tri_tests"], st["hits"]) == \
                (N_RAYS, ref[mode][2], ref[mode][3], int((ref[mode][0] >= 0).sum())), (rng_name, mode, st)
    # the any-hit flag is closest-hit's
    assert ((cornell_ref["unbounded"]["any"][0] >= 0) == (cornell_ref["unbounded"]["closest"][0] >= 0)).all()


def test_pinned_equals_oracle_walk_on_proxy(proxy, walkers, rig_factory):
    """512 camera rays (64x8) and 512 random ones on the bunny proxy, which does not fit in LDS."""
    g = rig_factory(proxy, W=64, H=8)
    g.r.frame(1, light_bounces=1)  # (sets FRAME_COUNT and the camera slots)
    _, cam = g.camera_rays(512)
    rays = np.concatenate([cam, random_rays(proxy, 512)])
    ref_c = walkers["proxy"].walk_rays(rays)
    ref_a = walkers["proxy"].walk_rays(rays, any_hit=True)
    assert (ref_c[0][:512] >= 0).any() and (ref_c[0][512:] >= 0).any()
    check_against(g.query(rays), ref_c, rays, "proxy closest")
    assert not g.k.scene_in_lds()
    check_against(g.query(rays, any_hit=True), ref_a, rays, "proxy any")


# ---- 3: degenerate rays -------------------------------------------------------------------------
def degenerate_rays(scene):
    lo, hi = scene_box(scene)
    c = ((lo + hi) / 2).astype(np.float32)
    vertex = scene.triangles["v1"]["position"][0, :3]
    o, d, tmin, tmax = [], [], [], []

    def add(org, dr, a=-INF, b=100000.0):
        o.append(org), d.append(dr), tmin.append(a), tmax.append(b)

    add(c, (0.0, 0.0, 0.0))                                   # the zero direction
    for axis in range(3):                                     # each axis direction, +0.0 / -0.0 elsewhere
        for s in (1.0, -1.0):
            for z in (0.0, -0.0):
                dr = [z, z, z]
                dr[axis] = s
                add(c + np.float32([0.25, -0.5, 0.125]), dr)
    add(c, (6e-31, 6e-31, 5e-31))                             # length 1e-30: the squared length underflows
    add(c, (-6e29, 6e29, -5e29))                              # length 1e30: it overflows
    add(c, (3e-31, 0.0, 0.0))
    rng = np.random.default_rng(11)
    for _ in range(4):                                        # from exactly a wall vertex
        add(vertex, rng.standard_normal(3).astype(np.float32))
    add(vertex, c - vertex)
    for _ in range(4):
        dr = rng.standard_normal(3).astype(np.float32)
        add(c, dr, -INF, 0.0)                                 # tmax = 0
        add(c, dr, 5.0, 1.0)                                  # tmin > tmax: always a miss with t == tmax
        add(c, dr, 2.0, 100000.0)                             # a lower bound that discards near hits
        add(c, dr, -INF, INF)
    return make_rays(np.float32(o), np.float32(d), np.float32(tmin), np.float32(tmax))


@pytest.mark.parametrize("force_global", [False, True], ids=["lds", "global"])
def test_degenerate_rays_equal_oracle_walk(cornell, walkers, rig_factory, force_global):
    rays = degenerate_rays(cornell)
    g = rig_factory(cornell, force_global=force_global)
    for any_hit in (False, True):
        ref = walkers["cornell"].walk_rays(rays, any_hit=any_hit)
        hits = g.query(rays, any_hit=any_hit)
        check_against(hits, ref, rays, f"degenerate any={any_hit}")
        inverted = rays["tmin"] > rays["tmax"]
        assert inverted.any() and (hits["prim"][inverted] == -1).all()
    assert (ref[0] >= 0).any() and (ref[0] < 0).any()


# ---- 4: barycentrics, known answer --------------------------------------------------------------
def leaf_scene():
    """One hand-built leaf: right triangles with small-integer vertices and legs 2 and 4, so that
    det = +-8 for rays along (0, 0, -1) and every operation of RayTriangle is exact in fp32."""
    from clrt import scene as S
    verts = [((0, 0, 0), (2, 0, 0), (0, 4, 0)),     # det +8, plane z = 0
             ((1, 1, 1), (1, 5, 1), (-1, 1, 1)),    # det +8, plane z = 1, overlaps the first
             ((0, 0, 2), (0, 4, 2), (2, 0, 2)),     # det -8: culled, though it covers the first
             ((4, 0, 3), (6, 0, 3), (4, 4, 3))]     # det +8, apart from the others
    t = np.zeros(len(verts), N.TRIANGLE_DTYPE)
    for i, tri in enumerate(verts):
        for name, p in zip(("v1", "v2", "v3"), tri):
            t[name]["position"][i, :3] = p
            t[name]["normal"][i, :3] = (0, 0, 1)
    nodes = np.zeros(1, N.NODE_DTYPE)
    nodes["bmin"][0, :3], nodes["bmax"][0, :3] = (-1, 0, 0), (6, 5, 3)
    nodes["offset"], nodes["nPrimitives"] = 0, len(verts)
    mats = np.zeros(1, N.MATERIAL_DTYPE)
    mats["diffuse"][:, :3], mats["roughness"], mats["ior"] = 0.5, 1.0, 1.0
    return S.Scene(t, nodes, mats, len(verts)), verts


def exact_hit(verts, ox, oy, oz):
    """RayTriangle + the closest-hit rule in exact rationals for direction (0, 0, -1)."""
    def sub(a, b): return tuple(x - y for x, y in zip(a, b))
    def dot(a, b): return sum(x * y for x, y in zip(a, b))
    def cross(a, b): return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
    o = tuple(Fraction(x) for x in (ox, oy, oz))
    d = (Fraction(0), Fraction(0), Fraction(-1))
    best = (-1, Fraction(100000), Fraction(0), Fraction(0))
    for i, (p1, p2, p3) in enumerate(verts):
        p1, p2, p3 = (tuple(Fraction(c) for c in p) for p in (p1, p2, p3))
        e1, e2 = sub(p2, p1), sub(p3, p1)
        pvec = cross(d, e2)
        det = dot(e1, pvec)
        if det < Fraction(1, 10**8):
            continue
        tvec = sub(o, p1)
        u = dot(tvec, pvec) / det
        qvec = cross(tvec, e1)
        v = dot(d, qvec) / det
        t = dot(e2, qvec) / det
        if u < 0 or u > 1 or v < 0 or u + v > 1 or not t < best[1]:
            continue
        best = (i, t, u, v)
    return best


@pytest.mark.parametrize("math_name", list(MATHS))
def test_barycentrics_known_answer(rig_factory, math_name):
    """t, u, v equal the exact rationals bit for bit in all three math modes: the shipped policy's
    2.5-ulp division and its normalize were recorded on an MI355X to be exact on these operands
    (1 / 8, rsqrt(1)) as well, so shipped is held to the same answer as pinned and devicelib."""
    scene, verts = leaf_scene()
    pts = [(x, y) for x in (-0.5, 0.0, 0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 4.5, 5.0, 5.75)
           for y in (0.0, 0.5, 1.0, 1.5, 2.0, 2.25, 3.0, 4.0, 4.5)]
    rays = make_rays(np.float32([(x, y, 5.0) for x, y in pts]), np.float32([(0.0, 0.0, -1.0)] * len(pts)))
    want = [exact_hit(verts, x, y, 5.0) for x, y in pts]
    prims = {w[0] for w in want}
    assert prims == {-1, 0, 1, 3}, prims                     # the culled triangle 2 is never the answer
    assert any(w[0] >= 0 and w[2] + w[3] == 1 for w in want) and any(w[0] >= 0 and w[2] == 0 for w in want)
    g = rig_factory(scene, math=MATHS[math_name])
    for force in (False, True):
        g.k.force_global_scene(force)
        hits = g.query(rays)
        got = [(int(h["prim"]), float(h["t"]), float(h["u"]), float(h["v"])) for h in hits]
        print(math_name, "global" if force else "lds", "inexact:",
              [(p, a, b) for p, a, b in zip(pts, got, want) if a[0] >= 0 and a != tuple(map(float, b))][:6])
        assert [a[0] for a in got] == [w[0] for w in want]
        assert [a for a, w in zip(got, want) if w[0] >= 0] == [tuple(map(float, w)) for w in want if w[0] >= 0]
        assert all(a == (-1, 100000.0, 0.0, 0.0) for a, w in zip(got, want) if w[0] < 0)


# ---- 5: every math mode is tied to the render path ----------------------------------------------
_walk_cache = {}


@pytest.mark.parametrize("frame_count", [1, 7])
@pytest.mark.parametrize("config", ["cornell-lds", "cornell-global", "proxy"])
@pytest.mark.parametrize("math_name", list(MATHS))
def test_query_of_camera_rays_equals_render_path(cornell, proxy, walkers, oracle_mod, rig_factory, math_name, config,
                                                 frame_count):
    W, H = 320, 180
    n = W * H
    scene_name = config.split("-")[0]
    scene = cornell if scene_name == "cornell" else proxy
    g = rig_factory(scene, math=MATHS[math_name], force_global=config == "cornell-global", W=W, H=H, hits=True)
    g.r.frame(frame_count, light_bounces=1)
    ids, t = g.r.hits()
    rb, rays = g.camera_rays(n)
    hb = g.buffer(n * 16)
    g.ctx.IntersectRays(g.k, rb, hb, n)
    hits = g.read(hb, n, N.RAY_HIT_DTYPE)
    assert g.k.scene_in_lds() == (config == "cornell-lds")
    assert 0.1 < (ids >= 0).mean() < 1.0
    assert (hits["prim"] == ids).all(), int((hits["prim"] != ids).sum())
    hit = ids >= 0
    assert (bits(hits["t"])[hit] == bits(t)[hit]).all()
    g.ctx.IntersectRays(g.k, rb, hb, n, N.QUERY_ANY)
    any_hits = g.read(hb, n, N.RAY_HIT_DTYPE)
    assert ((any_hits["prim"] >= 0) == hit).all()
    # the records themselves: origin = camPos, the full range
    from hip_helpers import DEFAULT_CAMERA
    assert (rays["origin"] == np.float32(DEFAULT_CAMERA[0])).all()
    assert (rays["tmin"] == -INF).all() and (rays["tmax"] == 100000.0).all()
    if math_name == "pinned":
        # three ways: the oracle's render of the same frame, and the helper's walk of the records
        _, oids, ot, _ = oracle_mod.render(scene, W, H, frame_count=frame_count, light_bounces=1, want_hits=True)
        assert (hits["prim"] == oids.ravel()).all()
        assert (bits(hits["t"])[hit] == bits(ot.ravel())[hit]).all()
        key = (scene_name, frame_count)
        if key not in _walk_cache:
            _walk_cache[key] = (rays.tobytes(), walkers[scene_name].walk_rays(rays))
        assert _walk_cache[key][0] == rays.tobytes()
        check_against(hits, _walk_cache[key][1], rays, "helper walk of the camera rays")


# ---- 6: hand-out at scale -----------------------------------------------------------------------
def test_handout_at_scale_and_ranges(cornell, cornell_ref, rig_factory):
    base = cornell_ref["unbounded"]["rays"]
    g = rig_factory(cornell)
    want = g.query(base)
    check_against(want, cornell_ref["unbounded"]["closest"], base, "source rays")
    n_big = (1 << 20) + 37
    big = np.tile(base, n_big // N_RAYS + 1)[:n_big]
    got = g.query(big)
    assert (got.view(np.uint32) == np.tile(want, n_big // N_RAYS + 1)[:n_big].view(np.uint32)).all()
    got_any = g.query(big, any_hit=True)
    want_any = g.query(base, any_hit=True)
    assert (got_any.view(np.uint32) == np.tile(want_any, n_big // N_RAYS + 1)[:n_big].view(np.uint32)).all()

    # small ranges at offsets: only [first, first + n) is written
    m = 4097 + 65 + 7
    src = np.tile(base, 3)[:m]
    full = np.tile(want, 3)[:m]
    rb = g.buffer(src.nbytes, src)
    sentinel = np.zeros(m, N.RAY_HIT_DTYPE)
    sentinel["prim"], sentinel["t"], sentinel["u"], sentinel["v"] = -7, 123.0, 4.0, 5.0
    for n in (1, 63, 64, 65):
        for first in (0, 1, 4097):
            hb = g.buffer(sentinel.nbytes, sentinel)
            g.ctx.IntersectRays(g.k, rb, hb, n, N.QUERY_CLOSEST, first)
            out = g.read(hb, m, N.RAY_HIT_DTYPE)
            expect = sentinel.copy()
            expect[first:first + n] = full[first:first + n]
            assert (out.view(np.uint32) == expect.view(np.uint32)).all(), (n, first)
    # two disjoint ranges back to back into one hit buffer, one read
    hb = g.buffer(sentinel.nbytes, sentinel)
    g.ctx.IntersectRays(g.k, rb, hb, 1000, N.QUERY_CLOSEST, 5)
    g.ctx.IntersectRays(g.k, rb, hb, 2000, N.QUERY_CLOSEST, 2100)
    out = g.read(hb, m, N.RAY_HIT_DTYPE)
    expect = sentinel.copy()
    expect[5:1005], expect[2100:4100] = full[5:1005], full[2100:4100]
    assert (out.view(np.uint32) == expect.view(np.uint32)).all()


# ---- 7: ordering with the render queue ----------------------------------------------------------
def test_query_is_ordered_with_coalesced_frames(cornell, cornell_ref, rig_factory):
    rays = cornell_ref["unbounded"]["rays"]
    images = []
    for with_query in (False, True):
        g = rig_factory(cornell, W=128, H=72, perframe_batch=None)  # (the library default: frames coalesce)
        rb = g.buffer(rays.nbytes, rays)
        hb = g.buffer(len(rays) * 16)
        for f in range(1, 5):
            g.r.frame(f, light_bounces=2)
        if with_query:
            g.ctx.IntersectRays(g.k, rb, hb, len(rays))
        images.append(g.r.result())
        if with_query:
            check_against(g.read(hb, len(rays), N.RAY_HIT_DTYPE), cornell_ref["unbounded"]["closest"], rays,
                          "query behind four queued frames")
    assert images[0][:, :3].any()
    assert images[0].tobytes() == images[1].tobytes()


# ---- 8: errors ----------------------------------------------------------------------------------
def test_errors(cornell, cornell_ref, rig_factory):
    import clrt
    from clrt import RTError
    import stress_scenes as SS
    rays = cornell_ref["unbounded"]["rays"]
    g = rig_factory(cornell)
    rb = g.buffer(rays.nbytes, rays)
    sentinel = np.full(N_RAYS * 4, 0x7fc12345, np.uint32)
    hb = g.buffer(sentinel.nbytes, sentinel)
    small = g.buffer(16 * 100)
    lib, ctx, k = g.ctx._lib, g.ctx.handle, g.k.handle

    def rc(kernel, rays_b, first, n, mode, hits_b):
        return lib.rtEnqueueIntersectRays(ctx, kernel, rays_b.handle, first, n, mode, hits_b.handle)

    assert rc(k, rb, 0, 0, N.QUERY_CLOSEST, hb) == 0                       # n_rays == 0: no launch
    assert rc(k, rb, 0, N_RAYS, 2, hb) == -30 and rc(k, rb, 0, N_RAYS, -1, hb) == -30   # mode
    assert rc(k, rb, 1, N_RAYS, N.QUERY_ANY, hb) == -61                    # beyond the ray buffer
    assert rc(k, rb, 0, 101, N.QUERY_CLOSEST, small) == -61                # beyond the hit buffer
    assert rc(k, rb, 1 << 31, 1, N.QUERY_CLOSEST, hb) == -30               # first + n > 2^31
    assert rc(k, rb, 5, (1 << 64) - 3, N.QUERY_CLOSEST, hb) == -30         # (a sum that would wrap)
    assert rc(k, rb, 0, N_RAYS, N.QUERY_CLOSEST, rb) == -38                # one buffer for both
    bare = clrt.CLKernel(g.ctx, "KernelEntry")
    assert rc(bare.handle, rb, 0, N_RAYS, N.QUERY_CLOSEST, hb) == -52      # no scene / node buffer
    bare.set_buffer(N.BUFFER_SCENE, g.r.bufs[0])
    assert rc(bare.handle, rb, 0, N_RAYS, N.QUERY_CLOSEST, hb) == -52
    # a malformed tree is refused as a render refuses it
    bad_nodes = cornell.nodes.copy()
    leaf = int(np.flatnonzero(bad_nodes["nPrimitives"] > 0)[0])
    bad_nodes["offset"][leaf] = len(cornell.triangles)
    bad = g.buffer(bad_nodes.nbytes, bad_nodes)
    bare.set_buffer(N.BUFFER_NODE, bad)
    assert rc(bare.handle, rb, 0, N_RAYS, N.QUERY_CLOSEST, hb) == -38
    # a leaf of more than 127 triangles has no octant records: refused, not walked
    big = SS.soup_scene(12, "big")
    tb = g.buffer(big.triangles.nbytes, big.triangles)
    nb = g.buffer(big.nodes.nbytes, big.nodes)
    bare.set_buffer(N.BUFFER_SCENE, tb)
    bare.set_buffer(N.BUFFER_NODE, nb)
    assert rc(bare.handle, rb, 0, N_RAYS, N.QUERY_CLOSEST, hb) == -59
    # camera rays
    assert lib.rtEnqueueCameraRays(ctx, bare.handle, 16, rb.handle) == -52  # no WIDTH / camera slots
    g.r.frame(1, light_bounces=1)
    assert lib.rtEnqueueCameraRays(ctx, k, 0, rb.handle) == -63
    assert lib.rtEnqueueCameraRays(ctx, k, N_RAYS + 1, rb.handle) == -61
    with pytest.raises(RTError):
        g.ctx.IntersectRays(g.k, rb, hb, N_RAYS, 7)
    # nothing was launched: the hit buffer still holds the pre-fill
    assert (g.read(hb, N_RAYS * 4, np.uint32) == sentinel).all()
    # a material buffer is not needed: the scene and node buffers alone answer the query
    bare.set_buffer(N.BUFFER_SCENE, g.r.bufs[0])
    bare.set_buffer(N.BUFFER_NODE, g.r.bufs[1])
    bare.set_math_mode(N.MATH_PINNED)
    assert rc(bare.handle, rb, 0, N_RAYS, N.QUERY_CLOSEST, hb) == 0
    check_against(g.read(hb, N_RAYS, N.RAY_HIT_DTYPE), cornell_ref["unbounded"]["closest"], rays, "bare kernel")
    # and the kernel that saw every error still works
    assert rc(k, rb, 0, N_RAYS, N.QUERY_ANY, hb) == 0
    check_against(g.read(hb, N_RAYS, N.RAY_HIT_DTYPE), cornell_ref["unbounded"]["any"], rays, "after the errors")
    bare.release()


# ---- 9: the Raytracer surface -------------------------------------------------------------------
def test_raytracer_cast_equals_low_level_path(cornell, cornell_ref):
    import clrt
    rays = cornell_ref["unbounded"]["rays"]
    rt = clrt.Raytracer(64, 8)
    rt.Init()
    try:
        rt.upload_scene(cornell)
        rt.kernel.set_math_mode(N.MATH_PINNED)
        for mode, any_hit in (("closest", False), ("any", True)):
            hits = rt.cast(rays["origin"], rays["dir"], any_hit=any_hit)
            assert hits.dtype == N.RAY_HIT_DTYPE
            check_against(hits, cornell_ref["unbounded"][mode], rays, f"cast {mode}")
        ranged = cornell_ref["ranged"]
        hits = rt.cast(ranged["rays"]["origin"][:100], ranged["rays"]["dir"][:100], tmin=0.0, tmax=5.0)
        check_against(hits, tuple(a[:100] for a in ranged["closest"][:2]), ranged["rays"][:100], "cast ranged")
        assert len(rt.cast(np.zeros((0, 3)), np.zeros((0, 3)))) == 0
    finally:
        rt.release()

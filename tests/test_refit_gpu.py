"""GPU: vertex updates and the device-side BVH refit (rtEnqueueUpdateVertices, rtRefitBVH).

The node and triangle buffers are read back after a refit ("read-back arrays") and everything is
checked against them: the bounds against the host refit (clrt.scene.refit), renders and queries
against the CPU oracle on a Scene made of the read-back arrays, and -- bit for bit -- against a cold
start (a fresh context given the read-back arrays, i.e. the full host-side preparation), which pins
every derived node layout the refit rewrites against the host packers.
"""
import numpy as np
import pytest

import refit_ref as R
import stress_scenes as SS
from clrt import _native as N
from clrt import scene as S
from hip_helpers import HipRenderer, rgb

pytestmark = pytest.mark.gpu

W, H, BOUNCES = 64, 48, 3
COUNTERS = ("rays", "node_visits", "tri_tests", "hits")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class Mover(HipRenderer):
    """HipRenderer whose triangle and node buffers are read-write, plus move() = UpdateVertices +
    RefitBVH and the read-back of both arrays."""

    def __init__(self, scene, width=W, height=H, global_oct=None, **kw):
        super().__init__(scene, width, height, **kw)
        self.scene = scene
        rw = N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR
        for b in self.bufs[:2]:
            b.release()
        self.bufs[0] = self.ctx.create_buffer(rw, scene.triangles.nbytes, scene.triangles)
        self.bufs[1] = self.ctx.create_buffer(rw, scene.nodes.nbytes, scene.nodes)
        self.k.set_buffer(N.BUFFER_SCENE, self.bufs[0])
        self.k.set_buffer(N.BUFFER_NODE, self.bufs[1])
        if global_oct is not None:
            self.k.set_tuning("global_oct", global_oct)
        self.staged = []

    def stage(self, pts):
        """A device buffer of rt_tri_points records (creating one waits on the queue: stage first)."""
        recs = R.tri_points(pts)
        b = self.ctx.create_buffer(N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR, recs.nbytes, recs)
        self.staged.append(b)
        return b, len(recs)

    def move_staged(self, pos, normals=None, first=0):
        self.ctx.UpdateVertices(self.bufs[0], first, pos[1], pos[0], normals[0] if normals else None)
        self.ctx.RefitBVH(self.k)

    def move(self, positions, normals=None, first=0):
        self.move_staged(self.stage(positions), self.stage(normals) if normals is not None else None, first)

    def arrays(self):
        t = np.empty_like(self.scene.triangles)
        n = np.empty_like(self.scene.nodes)
        self.ctx.ReadBuffer(self.bufs[0], t, blocking=True)
        self.ctx.ReadBuffer(self.bufs[1], n, blocking=True)
        return t, n

    def read_scene(self):
        t, n = self.arrays()
        return S.Scene(t, n, self.scene.materials, self.scene.max_prims_in_node)

    def clear_output(self):
        self.ctx.WriteBuffer(self.out, np.zeros((self.n, 4), np.float32))

    def counters(self):
        st = self.k.stats()
        return tuple(st[c] for c in COUNTERS)

    def close(self):
        self.ctx.Finish()
        for b in self.staged:
            b.release()
        super().close()


@pytest.fixture
def movers():
    made = []

    def make(*a, **kw):
        made.append(Mover(*a, **kw))
        return made[-1]

    yield make
    for m in made:
        m.close()


def frames(r, first=1, count=2):
    for f in range(first, first + count):
        r.frame(f, light_bounces=BOUNCES)


def cold_start(scene, first=1, count=2, global_oct=None, stats=True, **kw):
    """The same frames from a fresh context given `scene`: the full preparation path."""
    r = HipRenderer(scene, W, H, stats=stats, **kw)
    if global_oct is not None:
        r.k.set_tuning("global_oct", global_oct)
    frames(r, first, count)
    out = r.result()
    st = tuple(r.k.stats()[c] for c in COUNTERS) if stats else None
    r.close()
    return out, st


def new_positions(scene, seed=7):
    """The displacement recipe of every test here: each vertex moved by normal(0, 0.5)."""
    return R.positions(R.displaced(scene.triangles, seed))


def expected_triangles(scene, pts, first=0, normals=None):
    want = scene.triangles.copy()
    pts = np.asarray(pts, np.float32).reshape(-1, 3, 3)
    for i, v in enumerate(R.VERTS):
        want[v]["position"][first:first + len(pts), :3] = pts[:, i]
        if normals is not None:
            want[v]["normal"][first:first + len(pts), :3] = np.asarray(normals, np.float32).reshape(-1, 3, 3)[:, i]
    return want


def check_arrays(scene, tris, nodes, want_tris):
    """Read-back arrays: triangles changed only where written; bounds == the host refit of the
    read-back triangles; every other node byte and the records past the tree's end unchanged."""
    assert tris.tobytes() == want_tris.tobytes()
    host = S.refit(S.Scene(tris, scene.nodes, scene.materials)).nodes
    _, end = SS.tree_depth(scene.nodes)
    assert np.array_equal(nodes["bmin"][:end, :3], host["bmin"][:end, :3])
    assert np.array_equal(nodes["bmax"][:end, :3], host["bmax"][:end, :3])
    R.assert_only_bounds_changed(scene.nodes, nodes)


def grew(old, new):
    """At least one new bound lies outside the old box."""
    _, end = SS.tree_depth(old)
    return bool((new["bmin"][:end, :3] < old["bmin"][:end, :3]).any() or
                (new["bmax"][:end, :3] > old["bmax"][:end, :3]).any())


def scene_of(name, cornell):
    if name == "cornell":
        return cornell
    if name == "soup6000":
        return R.big_soup_scene()
    return R.tree_scenes()[name]()


# ---- 1. bounds and untouched bytes ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["cornell", "rt1", "rt7", "rt127", "chain", "big", "one_leaf", "soup6000"])
def test_bounds_and_untouched_bytes(cornell, movers, name):
    scene = scene_of(name, cornell)
    m = movers(scene)
    pts = new_positions(scene)
    m.move(pts)
    tris, nodes = m.arrays()
    check_arrays(scene, tris, nodes, expected_triangles(scene, pts))
    assert grew(scene.nodes, nodes)
    assert m.k.scene_prepares() == (1, 1)


# ---- 2, 3. renders after a move: the oracle, and a cold start ------------------------------------
CONFIGS = {
    "cornell_lds": ("cornell", dict()),
    "cornell_global": ("cornell", dict(force_global=True)),
    "cornell_global_records": ("cornell", dict(force_global=True, global_oct=0)),
    "big": ("big", dict()),
    "soup6000": ("soup6000", dict()),
    "cornell_wavefront": ("cornell", dict(sched=N.SCHED_WAVEFRONT)),
}
_moved = {}


def moved_render(cfg, cornell):
    """Frames 1-2 after every vertex moved, rendered once per configuration and shared:
    (image, counters, read-back Scene, scene in LDS)."""
    if cfg not in _moved:
        name, kw = CONFIGS[cfg]
        scene = scene_of(name, cornell)
        m = Mover(scene, stats=True, **kw)
        try:
            frames(m)                       # the old geometry is packed and rendered first
            m.ctx.Finish()
            m.clear_output()
            m.k.reset_stats()
            m.move(new_positions(scene))
            frames(m)
            out, st, back, lds = m.result(), m.counters(), m.read_scene(), m.k.scene_in_lds()
            assert m.k.scene_prepares() == (1, 1)
        finally:
            m.close()
        assert grew(scene.nodes, back.nodes), "old boxes would still be right"
        for a in (out, back.triangles, back.nodes):
            a.setflags(write=False)
        _moved[cfg] = (out, st, back, lds)
    return _moved[cfg]


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_render_after_move_equals_oracle(cornell, oracle_mod, cfg):
    out, st, back, lds = moved_render(cfg, cornell)
    where = {"cornell_lds": True, "cornell_global": False, "cornell_global_records": False, "soup6000": False}
    assert cfg not in where or lds == where[cfg]
    res = np.zeros((W * H, 4), np.float32)
    counts = dict.fromkeys(COUNTERS, 0)
    for f in (1, 2):
        res, _, _, c = oracle_mod.render(back, W, H, frame_count=f, light_bounces=BOUNCES, result=res, threads=16)
        for key in COUNTERS:
            counts[key] += c[key]
    assert np.array_equal(bits(rgb(out)), bits(rgb(res)))
    assert st == tuple(counts[c] for c in COUNTERS)


@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_render_after_move_equals_cold_start(cornell, cfg):
    out, st, back, _ = moved_render(cfg, cornell)
    want, wst = cold_start(back, **CONFIGS[cfg][1])
    assert np.array_equal(bits(out), bits(want))
    assert st == wst


@pytest.mark.parametrize("math", ["devicelib", "shipped"])
def test_cold_start_bits_in_other_math_modes(cornell, movers, math):
    mode = {"devicelib": N.MATH_DEVICELIB, "shipped": N.MATH_SHIPPED}[math]
    m = movers(cornell, math=mode)
    frames(m)
    m.clear_output()
    m.move(new_positions(cornell))
    frames(m)
    out, back = m.result(), m.read_scene()
    want, _ = cold_start(back, math=mode, stats=False)
    assert np.array_equal(bits(out), bits(want))


# ---- 4. repeated and partial updates -------------------------------------------------------------
def test_three_moves_without_host_waits(cornell, movers):
    m = movers(cornell)
    staged = [m.stage(new_positions(cornell, seed)) for seed in (1, 2, 3)]
    for i, pos in enumerate(staged):
        m.clear_output()
        m.move_staged(pos)                  # update, refit and launch back to back
        frames(m)
        out, back = m.result(), m.read_scene()
        want, _ = cold_start(back, stats=False)
        assert np.array_equal(bits(out), bits(want)), i
        check_arrays(cornell, back.triangles, back.nodes,
                     expected_triangles(cornell, new_positions(cornell, i + 1)))
    assert m.k.scene_prepares() == (1, 3)


def test_partial_updates(movers):
    scene = SS.soup_scene(12, "rt7")
    m = movers(scene)
    nt = scene.n_triangles
    leaves = np.flatnonzero(scene.nodes["nPrimitives"][:SS.tree_depth(scene.nodes)[1]] > 1)
    leaf = int(leaves[len(leaves) // 2])
    lo, cnt = int(scene.nodes["offset"][leaf]), int(scene.nodes["nPrimitives"][leaf])
    moved = new_positions(scene, 11)
    want = scene.triangles
    for first, n in ((lo, cnt), (nt - 1, 1), (0, 1)):
        m.move(moved[first:first + n], first=first)
        tris, nodes = m.arrays()
        want = expected_triangles(S.Scene(want, scene.nodes, scene.materials), moved[first:first + n], first)
        check_arrays(scene, tris, nodes, want)
    frames(m)
    out = m.result()
    cold, _ = cold_start(m.read_scene(), stats=False)
    assert np.array_equal(bits(out), bits(cold))


def test_normals_update_changes_shading_not_bounds(cornell, oracle_mod, movers):
    m = movers(cornell)
    frames(m)
    before = m.result()
    rng = np.random.default_rng(3)
    normals = rng.normal(0.0, 1.0, (cornell.n_triangles, 3, 3)).astype(np.float32)
    pts = R.positions(cornell.triangles)
    m.clear_output()
    m.move(pts, normals)
    frames(m)
    out, back = m.result(), m.read_scene()
    assert back.triangles.tobytes() == expected_triangles(cornell, pts, 0, normals).tobytes()
    assert np.array_equal(back.nodes["bmin"], cornell.nodes["bmin"])
    assert np.array_equal(back.nodes["bmax"], cornell.nodes["bmax"])
    assert not np.array_equal(bits(out), bits(before))
    res = np.zeros((W * H, 4), np.float32)
    for f in (1, 2):
        res, _, _, _ = oracle_mod.render(back, W, H, frame_count=f, light_bounces=BOUNCES, result=res, threads=16)
    assert np.array_equal(bits(rgb(out)), bits(rgb(res)))


# ---- 5. queue order ------------------------------------------------------------------------------
def _sequence(m, pos, fused, finish):
    def step(fn, *a, **kw):
        fn(*a, **kw)
        if finish:
            m.ctx.Finish()

    if fused:
        step(m.frame, 1, light_bounces=BOUNCES, n_frames=4)
        step(m.move_staged, pos)
        step(m.frame, 5, light_bounces=BOUNCES, n_frames=4)
    else:
        step(m.frame, 1, light_bounces=BOUNCES)
        step(m.frame, 2, light_bounces=BOUNCES)
        step(m.move_staged, pos)
        step(m.frame, 3, light_bounces=BOUNCES)
        step(m.frame, 4, light_bounces=BOUNCES)
    return m.result()


@pytest.mark.parametrize("fused", [False, True], ids=["coalesced_perframe", "fused_frames"])
def test_move_is_ordered_with_queued_frames(cornell, movers, fused):
    outs = []
    for finish in (False, True):
        m = movers(cornell, perframe_batch=None)   # the library's default: frames coalesce
        pos = m.stage(new_positions(cornell))
        outs.append(_sequence(m, pos, fused, finish))
    assert np.array_equal(bits(outs[0]), bits(outs[1]))
    # and the move took effect between the frames: not what the unmoved scene gives
    m = movers(cornell, perframe_batch=None)
    if fused:
        m.frame(1, light_bounces=BOUNCES, n_frames=8)
    else:
        frames(m, 1, 4)
    assert not np.array_equal(bits(outs[0]), bits(m.result()))


# ---- 6. queries ----------------------------------------------------------------------------------
N_RAYS = 2048
_query_ref = {}


def query_rays(scene):
    rng = np.random.default_rng(7)
    p = R.positions(scene.triangles).reshape(-1, 3)
    rays = np.zeros(N_RAYS, N.RAY_DTYPE)
    rays["origin"] = rng.uniform(p.min(axis=0), p.max(axis=0), (N_RAYS, 3)).astype(np.float32)
    rays["dir"] = rng.standard_normal((N_RAYS, 3)).astype(np.float32)
    rays["tmin"], rays["tmax"] = -np.inf, 100000.0
    return rays


def query_reference(back, rays):
    """SceneWalker on the read-back arrays, once per mode (the arrays are the same for every rig: same
    scene, same displacement)."""
    from ray_query_ref import SceneWalker
    key = (back.triangles.tobytes(), back.nodes.tobytes())
    if _query_ref.get("key") != key:
        w = SceneWalker(back)
        _query_ref.update(key=key, closest=w.walk_rays(rays), any=w.walk_rays(rays, any_hit=True))
    return _query_ref


def run_query(m, rays, any_hit):
    rb = m.ctx.create_buffer(N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR, rays.nbytes, rays)
    hb = m.ctx.create_buffer(N.MEM_READ_WRITE, len(rays) * 16)
    m.staged += [rb, hb]
    m.ctx.IntersectRays(m.k, rb, hb, len(rays), N.QUERY_ANY if any_hit else N.QUERY_CLOSEST)
    hits = np.empty(len(rays), N.RAY_HIT_DTYPE)
    m.ctx.ReadBuffer(hb, hits, blocking=True)
    return hits


@pytest.mark.parametrize("force_global", [False, True], ids=["lds", "global"])
def test_queries_after_move_equal_oracle_walk(cornell, oracle_mod, movers, force_global):
    m = movers(cornell, force_global=force_global, stats=True)
    rays = query_rays(cornell)
    run_query(m, rays, False)               # the old geometry is packed and queried first
    m.move(new_positions(cornell))
    back = m.read_scene()
    ref = query_reference(back, rays)
    for mode in ("closest", "any"):
        m.k.reset_stats()
        hits = run_query(m, rays, mode == "any")
        assert m.k.scene_in_lds() == (not force_global)
        prim, t, visits, tests = ref[mode]
        assert np.array_equal(hits["prim"], prim), mode
        assert np.array_equal(bits(hits["t"]), bits(t)), mode
        st = m.k.stats()
        assert (st["rays"], st["node_visits"], st["tri_tests"], st["hits"]) == \
            (N_RAYS, visits, tests, int((prim >= 0).sum())), mode
    assert m.k.scene_prepares() == (1, 1)


def test_query_only_kernel_without_materials_refits(cornell, oracle_mod):
    import clrt
    ctx = clrt.CLContext(0)
    k = clrt.CLKernel(ctx, "KernelEntry")
    rw = N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR
    tb = ctx.create_buffer(rw, cornell.triangles.nbytes, cornell.triangles)
    nb = ctx.create_buffer(rw, cornell.nodes.nbytes, cornell.nodes)
    k.set_buffer(N.BUFFER_SCENE, tb)
    k.set_buffer(N.BUFFER_NODE, nb)
    k.set_math_mode(N.MATH_PINNED)
    rays = query_rays(cornell)
    recs = R.tri_points(new_positions(cornell))
    pb = ctx.create_buffer(rw, recs.nbytes, recs)
    rb = ctx.create_buffer(rw, rays.nbytes, rays)
    hb = ctx.create_buffer(N.MEM_READ_WRITE, N_RAYS * 16)
    try:
        ctx.UpdateVertices(tb, 0, len(recs), pb)
        ctx.RefitBVH(k)                     # never prepared, no material bound: the full leg, then the refit
        assert k.scene_prepares() == (1, 1)
        ctx.IntersectRays(k, rb, hb, N_RAYS)
        hits = np.empty(N_RAYS, N.RAY_HIT_DTYPE)
        ctx.ReadBuffer(hb, hits, blocking=True)
        t, n = np.empty_like(cornell.triangles), np.empty_like(cornell.nodes)
        ctx.ReadBuffer(tb, t, blocking=True)
        ctx.ReadBuffer(nb, n, blocking=True)
        prim, tt, _, _ = query_reference(S.Scene(t, n, cornell.materials), rays)["closest"]
        assert np.array_equal(hits["prim"], prim) and np.array_equal(bits(hits["t"]), bits(tt))
        assert k.scene_prepares() == (1, 1)
    finally:
        ctx.Finish()
        for b in (tb, nb, pb, rb, hb):
            b.release()
        k.release()
        ctx.release()


def test_raytracer_move_vertices_and_cast(cornell, oracle_mod):
    import clrt
    rt = clrt.Raytracer(W, H)
    rt.Init()
    try:
        rt.kernel.set_math_mode(N.MATH_PINNED)
        rt.upload_scene(cornell)
        rays = query_rays(cornell)
        rt.cast(rays["origin"], rays["dir"])
        rt.move_vertices(new_positions(cornell))
        hits = rt.cast(rays["origin"], rays["dir"])
        t, n = np.empty_like(cornell.triangles), np.empty_like(cornell.nodes)
        rt.ctx.ReadBuffer(rt._scene_bufs[0], t, blocking=True)
        rt.ctx.ReadBuffer(rt._scene_bufs[1], n, blocking=True)
        prim, tt, _, _ = query_reference(S.Scene(t, n, cornell.materials), rays)["closest"]
        assert np.array_equal(hits["prim"], prim) and np.array_equal(bits(hits["t"]), bits(tt))
        assert rt.kernel.scene_prepares() == (1, 1)
    finally:
        rt.release()


# ---- 7. no host round trip -----------------------------------------------------------------------
def test_scene_prepares_counts_and_shared_buffers(cornell, movers):
    import clrt
    m = movers(cornell)
    frames(m, 1, 1)
    m.result()
    assert m.k.scene_prepares() == (1, 0)
    for i in range(1, 4):
        m.move(new_positions(cornell, i))
        frames(m, 1, 1)
        m.result()
        assert m.k.scene_prepares() == (1, i)
    # a host write into the triangle buffer may have changed anything: the next refit prepares in full
    moved = R.displaced(cornell.triangles, 9)
    m.ctx.WriteBuffer(m.bufs[0], moved)
    m.ctx.RefitBVH(m.k)
    assert m.k.scene_prepares() == (2, 4)
    m.clear_output()
    frames(m)
    out, back = m.result(), m.read_scene()
    assert m.k.scene_prepares() == (2, 4)
    assert back.triangles.tobytes() == moved.tobytes()
    want, _ = cold_start(back, stats=False)
    assert np.array_equal(bits(out), bits(want))
    # a second kernel bound to the same buffers sees a changed generation and prepares in full
    k2 = clrt.CLKernel(m.ctx, "KernelEntry")
    out2 = m.ctx.create_buffer(N.MEM_WRITE_ONLY, W * H * 16)
    m.staged.append(out2)
    try:
        for slot, b in ((N.BUFFER_OUT, out2), (N.BUFFER_SCENE, m.bufs[0]), (N.BUFFER_NODE, m.bufs[1]),
                        (N.BUFFER_MATERIAL, m.bufs[2])):
            k2.set_buffer(slot, b)
        k2.set_int(N.WIDTH, W)
        k2.set_int(N.HEIGHT, H)
        k2.set_math_mode(N.MATH_PINNED)
        k2.set_tuning("perframe_batch", 1)
        main_k, main_out = m.k, m.out
        m.k, m.out = k2, out2
        frames(m)
        got2 = m.result()
        m.move(new_positions(cornell, 10))  # k2 refits: m's own kernel prepares in full at its next launch
        m.k, m.out = main_k, main_out
        assert np.array_equal(bits(got2), bits(want))
        assert k2.scene_prepares() == (1, 1)
        m.clear_output()
        frames(m)
        out3 = m.result()
        assert m.k.scene_prepares() == (3, 4)
        want3, _ = cold_start(m.read_scene(), stats=False)
        assert np.array_equal(bits(out3), bits(want3))
    finally:
        m.ctx.Finish()
        k2.release()


# ---- 8. non-finite input -------------------------------------------------------------------------
def test_nonfinite_vertices(oracle_mod, movers):
    scene = SS.soup_scene(12, "rt7")
    bad = SS.soup_scene(12, "rt7", nonfinite=True)
    pts = R.positions(bad.triangles)
    assert np.isnan(pts).any() and np.isinf(pts).any() and (np.abs(pts[np.isfinite(pts)]) > 1e29).any()
    m = movers(scene)
    frames(m)
    m.clear_output()
    m.move(pts)
    frames(m)
    out, back = m.result(), m.read_scene()
    assert back.triangles.tobytes() == bad.triangles.tobytes()
    check_arrays(scene, back.triangles, back.nodes, bad.triangles)
    res = np.zeros((W * H, 4), np.float32)
    for f in (1, 2):
        res, _, _, _ = oracle_mod.render(back, W, H, frame_count=f, light_bounces=BOUNCES, result=res, threads=16)
    assert np.array_equal(bits(rgb(out)), bits(rgb(res)))


# ---- 9. errors -----------------------------------------------------------------------------------
def test_errors_launch_nothing(cornell, movers):
    import clrt
    m = movers(cornell)
    lib, ctx = m.ctx._lib, m.ctx.handle
    nt = cornell.n_triangles
    pos, _ = m.stage(new_positions(cornell))
    small, _ = m.stage(new_positions(cornell)[:nt - 1])
    other = clrt.CLContext(0)
    foreign = other.create_buffer(N.MEM_READ_WRITE, nt * 48)
    k_unbound = clrt.CLKernel(m.ctx, "KernelEntry")
    tb = m.bufs[0].handle

    def update(tris, first, n, p, nrm):
        return lib.rtEnqueueUpdateVertices(ctx, tris, first, n, p, nrm)

    try:
        assert lib.rtRefitBVH(ctx, k_unbound.handle) == -52                 # scene / node slot unbound
        k_unbound.set_buffer(N.BUFFER_SCENE, m.bufs[0])
        assert lib.rtRefitBVH(ctx, k_unbound.handle) == -52
        assert update(tb, 0, nt, foreign.handle, None) == -38              # another context's buffer
        assert update(tb, 0, nt, pos.handle, foreign.handle) == -38
        assert update(foreign.handle, 0, nt, pos.handle, None) == -38
        assert update(tb, 0, nt, None, None) == -38                        # NULL buffers
        assert update(None, 0, nt, pos.handle, None) == -38
        assert update(tb, 1, nt, pos.handle, None) == -61                  # first + n beyond tris
        assert update(tb, nt + 1, 0, pos.handle, None) == -61
        assert update(tb, 2 ** 63, 2 ** 63, pos.handle, None) == -61
        assert update(tb, 0, nt, small.handle, None) == -61                # positions / normals < 48 n
        assert update(tb, 0, nt, pos.handle, small.handle) == -61
        assert update(tb, 0, nt, tb, None) == -38                          # positions / normals are tris
        assert update(tb, 0, nt, pos.handle, tb) == -38
        assert update(tb, 0, 0, pos.handle, None) == 0                     # nothing to do
        t, n = m.arrays()
        assert t.tobytes() == cornell.triangles.tobytes() and n.tobytes() == cornell.nodes.tobytes()
        # a malformed tree met by the full-preparation leg
        broken = cornell.nodes.copy()
        broken["offset"][0] = 1
        m.ctx.WriteBuffer(m.bufs[1], broken)
        assert lib.rtRefitBVH(ctx, m.k.handle) == -38
        t, n = m.arrays()
        assert t.tobytes() == cornell.triangles.tobytes() and n.tobytes() == broken.tobytes()
        assert m.k.scene_prepares() == (0, 0)
        m.ctx.WriteBuffer(m.bufs[1], cornell.nodes)
        m.ctx.RefitBVH(m.k)
        assert m.k.scene_prepares() == (1, 1)
    finally:
        m.ctx.Finish()
        k_unbound.release()
        foreign.release()
        other.release()

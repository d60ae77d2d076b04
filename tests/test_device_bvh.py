"""GPU: device-side BVH build (rtBuildBVH).

The device builder writes the reference's node contract (CLBVHnode.cpp:161-183) but a
different tree than the host SAH build (host/scene.cpp, the reference's algorithm), so:
  * structure: depth-first layout, leaves partition the (permuted) triangle array, bounds
    contain their children and triangles, leaf sizes <= maxPrimitivesInNode;
  * parity is per geometry: rendering the device-built arrays is bit-exact with the CPU
    oracle rendering the same arrays (pinned math), and close to the SAH-built scene's image
    (the Cornell OBJ holds every face twice, so ties may pick the other copy);
  * the builder's output is fully determined, so it equals the numpy restatement of both builders
    (bvh_build_ref.py) byte for byte on every case of bvh_build_ref.CASES, two builds of one input
    give the same bytes, and the built buffers go through bind, move, refit, rebuild and query.
"""
import time

import numpy as np
import pytest

from clrt import _native as N
from clrt import scene as S
from hip_helpers import HipRenderer, rgb
from ref_compare import rel_err
from test_scene import _check_bvh

pytestmark = pytest.mark.gpu


def _file_order_cornell():
    z = np.load(S.CORNELL_NPZ, allow_pickle=False)
    return z["triangles"].view(N.TRIANGLE_DTYPE), z["materials"].view(N.MATERIAL_DTYPE)


def _same_multiset(a, b):
    key = lambda x: sorted(bytes(r) for r in x.view(np.uint8).reshape(x.shape[0], -1))
    return key(a) == key(b)


METHODS = ["ploc", "lbvh"]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("max_prims", [1, 2, 4, 8])
def test_device_bvh_structure(max_prims, method):
    tris, mats = _file_order_cornell()
    sc = S.build_bvh_device(tris, mats, max_prims, method=method)
    _check_bvh(sc)
    leaf = sc.nodes["nPrimitives"]
    assert leaf.max() <= max_prims
    assert sc.nodes.shape[0] <= 2 * tris.shape[0] - 1
    assert _same_multiset(sc.triangles, tris)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("n", [1, 3])
def test_device_bvh_single_leaf(n, method):
    tris, mats = _file_order_cornell()
    sc = S.build_bvh_device(tris[:n], mats, 4, method=method)
    # n <= max_prims: one leaf, for both builders (PLOC collapses every subtree of <= max_prims
    # triangles; only an RT_PLOC_SAH_LEAVES build, off by default, lets the SAH keep it split)
    assert sc.nodes.shape[0] == 1 and sc.nodes[0]["nPrimitives"] == n
    assert sc.nodes["nPrimitives"].sum() == n
    _check_bvh(sc)


@pytest.mark.parametrize("method", METHODS)
def test_device_bvh_render_bit_exact_vs_oracle(oracle_mod, method):
    tris, mats = _file_order_cornell()
    sc = S.build_bvh_device(tris, mats, 4, method=method)
    W, H = 160, 90
    r = HipRenderer(sc, W, H, stats=True)
    for f in (1, 2):
        r.frame(f, light_bounces=9)
    got = r.result()
    st = r.k.stats()
    r.close()
    want = np.zeros((W * H, 4), np.float32)
    counts = {"node_visits": 0, "tri_tests": 0}
    for f in (1, 2):
        want, _, _, c = oracle_mod.render(sc, W, H, frame_count=f, light_bounces=9, result=want, threads=16)
        for k in counts:
            counts[k] += c[k]
    a, b = rgb(got), rgb(want)
    assert (a.view(np.uint32) == b.view(np.uint32)).all()
    assert (st["node_visits"], st["tri_tests"]) == (counts["node_visits"], counts["tri_tests"])


@pytest.mark.parametrize("method", METHODS)
def test_device_bvh_bunny_matches_sah_image(method):
    """70k-triangle proxy: the device tree renders the same geometry as the SAH tree."""
    from clrt import proxy
    host = proxy.bunny_proxy()
    raw = S.load_obj(proxy.os.path.join(proxy.GEN_DIR, "bunny_proxy.obj"), build=False)
    t0 = time.perf_counter()
    dev = S.build_bvh_device(raw.triangles, raw.materials, 4, method=method)
    build_s = time.perf_counter() - t0
    _check_bvh(dev)
    assert _same_multiset(dev.triangles, host.triangles)
    W, H = 256, 144
    imgs = []
    for sc in (host, dev):
        r = HipRenderer(sc, W, H, math=N.MATH_DEVICELIB, hits=True)
        r.frame(1, light_bounces=1)
        imgs.append((rgb(r.result()), r.hits()[0], None))
        r.close()
    (a, ida, _), (b, idb, _) = imgs

    def face_keys(sc):  # geometric identity of a triangle (the loader's two copies share it)
        pos = np.stack([sc.triangles[v]["position"][:, :3] for v in ("v1", "v2", "v3")], axis=1)
        return [tuple(sorted(map(tuple, q.tolist()))) for q in pos]

    kh, kd = face_keys(host), face_keys(dev)
    fa = [kh[i] if i >= 0 else None for i in ida.ravel()]
    fb = [kd[i] if i >= 0 else None for i in idb.ravel()]
    agree = np.mean([x == y for x, y in zip(fa, fb)])
    assert agree > 0.999, agree                      # the same face is hit
    rel = rel_err(a, b).max(axis=-1)
    assert (rel > 1e-4).mean() < 0.005               # radiance: last-bit differences from ties
    same = (a.view(np.uint32) == b.view(np.uint32)).all(axis=-1).mean()
    print(f"device {method} build of {raw.triangles.shape[0]} triangles: {build_s * 1e3:.1f} ms incl. transfers; "
          f"same face {agree:.5f}; {same:.4f} of pixels bit-identical to the SAH tree's image")


@pytest.mark.parametrize("method", [N.BVH_PLOC, N.BVH_LBVH])
@pytest.mark.parametrize("max_prims", [1, 4])
def test_device_bvh_buffers_bind_to_kernel_entry_as_they_are(oracle_mod, max_prims, method):
    """rt_hip.h's flow for rtBuildBVH: the triangle and node buffers it wrote are bound to
    KernelEntry directly -- the node buffer keeps its 2n-1 records (the tree is the first
    `count`, the rest unused) -- and the render equals the oracle's on the tree read back."""
    import clrt
    tris, mats = _file_order_cornell()
    n = tris.shape[0]
    W, H = 128, 96
    ctx = clrt.CLContext(0)
    tb = ctx.create_buffer(N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR, tris.nbytes, tris)
    nb = ctx.create_buffer(N.MEM_READ_WRITE, (2 * n - 1) * N.NODE_DTYPE.itemsize)
    mb = ctx.create_buffer(N.MEM_READ_ONLY | N.MEM_COPY_HOST_PTR, mats.nbytes, mats)
    count = ctx.BuildBVH(tb, n, max_prims, nb, method)
    assert (max_prims == 1) == (count == 2 * n - 1)
    out = ctx.create_buffer(N.MEM_WRITE_ONLY, W * H * 16)
    k = clrt.CLKernel(ctx)
    for slot, b in ((N.BUFFER_OUT, out), (N.BUFFER_SCENE, tb), (N.BUFFER_NODE, nb), (N.BUFFER_MATERIAL, mb)):
        k.set_buffer(slot, b)
    k.set_math_mode(N.MATH_PINNED)
    k.set_int(N.WIDTH, W)
    k.set_int(N.HEIGHT, H)
    k.set_int(N.LIGHT_BOUNCES, 4)
    k.set_int(N.LIGHT_TYPE, 0)
    k.set_float(N.SKYBOX_INTENSITY, 1.0)
    k.set_uint(N.FRAME_SEED, 0)
    for slot, v in zip((N.CAMERA_POS, N.CAMERA_FRONT, N.CAMERA_UP), ((0.0, -25.0, 8.5), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))):
        k.set_float3(slot, v)
    k.set_uint(N.FRAME_COUNT, 1)
    ctx.ExecuteKernel(k, W * H)
    got = np.zeros((W * H, 4), np.float32)
    ctx.ReadBuffer(out, got, blocking=True)
    t_dev = np.empty_like(tris)
    n_dev = np.empty(count, N.NODE_DTYPE)
    ctx.ReadBuffer(tb, t_dev, blocking=True)
    ctx.ReadBuffer(nb, n_dev, n_dev.nbytes, blocking=True)
    for b in (tb, nb, mb, out):
        b.release()
    k.release()
    ctx.release()
    sc = S.Scene(t_dev, n_dev, mats, max_prims)
    want, _, _, _ = oracle_mod.render(sc, W, H, frame_count=1, light_bounces=4, threads=16)
    assert (rgb(got).view(np.uint32) == rgb(want).view(np.uint32)).all()


def _sah_cost(sc):
    """Surface-area-heuristic cost of a depth-first node array (interior 1, triangle test 1 per
    triangle), relative to the root box: the expected work of a random ray that hits the root."""
    lo, hi = sc.nodes["bmin"][:, :3].astype(np.float64), sc.nodes["bmax"][:, :3].astype(np.float64)
    d = np.maximum(hi - lo, 0.0)
    area = 2.0 * (d[:, 0] * d[:, 1] + d[:, 1] * d[:, 2] + d[:, 2] * d[:, 0])
    cnt = sc.nodes["nPrimitives"].astype(np.float64)
    return float(np.sum(area * np.where(cnt > 0, cnt, 1.0)) / area[0])


def test_device_bvh_ploc_tree_beats_lbvh():
    """PLOC clusters by surface area: on the 70k-triangle proxy its tree's SAH cost is well below
    the linear BVH's and within reach of the host SAH build (the reference's algorithm)."""
    from clrt import proxy
    host = proxy.bunny_proxy()
    raw = S.load_obj(proxy.os.path.join(proxy.GEN_DIR, "bunny_proxy.obj"), build=False)
    c = {m: _sah_cost(S.build_bvh_device(raw.triangles, raw.materials, 4, method=m)) for m in METHODS}
    c["host_sah"] = _sah_cost(host)
    print("SAH cost:", {k: round(v, 2) for k, v in c.items()})
    assert c["ploc"] < 0.9 * c["lbvh"], c
    assert c["ploc"] < 1.3 * c["host_sah"], c


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("case", ["identical", "coplanar_grid", "random_soup"])
def test_device_bvh_degenerate_and_large_inputs(oracle_mod, method, case):
    """Inputs that stress the builders: 2,000 copies of one triangle (every Morton code and every
    PLOC cost ties: the pairing fallback), a flat grid of 20,000 triangles in one plane (zero-volume
    boxes), and a 150,000-triangle random soup.  The tree keeps the node contract and a render of it
    is bit-exact with the oracle rendering the same arrays."""
    tris, mats = _file_order_cornell()
    rng = np.random.default_rng(7)
    if case == "identical":
        out = np.repeat(tris[10:11], 2000)
    elif case == "coplanar_grid":
        g = 100
        xs, ys = np.meshgrid(np.linspace(-5, 5, g + 1)[:-1], np.linspace(-5, 5, g + 1)[:-1])
        out = np.repeat(tris[:1], 2 * g * g)
        d = 10.0 / g
        for k, (dx0, dy0, dx1, dy1, dx2, dy2) in enumerate(((0, 0, d, 0, 0, d), (d, 0, d, d, 0, d))):
            sl = out[k::2]
            sl["v1"]["position"][:, 0], sl["v1"]["position"][:, 1] = xs.ravel() + dx0, ys.ravel() + dy0
            sl["v2"]["position"][:, 0], sl["v2"]["position"][:, 1] = xs.ravel() + dx1, ys.ravel() + dy1
            sl["v3"]["position"][:, 0], sl["v3"]["position"][:, 1] = xs.ravel() + dx2, ys.ravel() + dy2
            for v in ("v1", "v2", "v3"):
                sl[v]["position"][:, 2] = 0.0
            out[k::2] = sl
    else:
        out = np.repeat(tris[:1], 150_000)
        c = rng.uniform(-6, 6, (out.shape[0], 3)).astype(np.float32) + np.float32([0, 0, 6])
        for v in ("v1", "v2", "v3"):
            out[v]["position"][:, :3] = c + rng.normal(0, 0.15, (out.shape[0], 3)).astype(np.float32)
    out["mtlIndex"] = 1
    sc = S.build_bvh_device(out, mats, 4, method=method)
    _check_bvh(sc)
    assert sc.nodes["nPrimitives"].max() <= 4
    assert _same_multiset(sc.triangles, out)
    W, H = 64, 48
    r = HipRenderer(sc, W, H)
    r.frame(1, light_bounces=3)
    got = r.result()
    r.close()
    want, _, _, _ = oracle_mod.render(sc, W, H, frame_count=1, light_bounces=3,
                                      result=np.zeros((W * H, 4), np.float32), threads=16)
    assert (rgb(got).view(np.uint32) == rgb(want).view(np.uint32)).all()


# ---- the builders against their numpy restatement (bvh_build_ref.py) -----------------------------
import bvh_build_ref as B  # noqa: E402
import refit_ref  # noqa: E402
import stress_scenes as SS  # noqa: E402

CODES = {"ploc": N.BVH_PLOC, "lbvh": N.BVH_LBVH}
FILL = 0xA5  # the byte unused buffer space is filled with


def _assert_build_equals(tris, nodes, want_tris, want_nodes):
    """Byte equality of a build's output with the reference's, naming the first difference."""
    diff = B.first_difference(nodes, want_nodes)
    assert diff is None, diff
    a = np.ascontiguousarray(tris).view(np.uint8).reshape(len(tris), -1)
    b = np.ascontiguousarray(want_tris).view(np.uint8).reshape(len(want_tris), -1)
    bad = np.flatnonzero((a != b).any(axis=1))
    assert bad.size == 0, f"triangle {int(bad[0])} of {len(a)} is not the reference's ({bad.size} differ)"


def _build_raw(ctx, tris, max_prims, method, extra_tris=0, extra_nodes=0):
    """rtBuildBVHEx into buffers with room for `extra` records behind n triangles and 2n-1 nodes, the
    nodes and the extra room pre-filled with FILL: (count, triangle bytes, node bytes) read back."""
    n = len(tris)
    traw = np.full((n + extra_tris) * 256, FILL, np.uint8)
    traw[:n * 256] = np.ascontiguousarray(tris).view(np.uint8).reshape(-1)
    nraw = np.full((2 * n - 1 + extra_nodes) * 48, FILL, np.uint8)
    rw = N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR
    tb, nb = ctx.create_buffer(rw, traw.nbytes, traw), ctx.create_buffer(rw, nraw.nbytes, nraw)
    try:
        count = ctx.BuildBVH(tb, n, max_prims, nb, CODES[method])
        ctx.ReadBuffer(tb, traw, blocking=True)
        ctx.ReadBuffer(nb, nraw, blocking=True)
    finally:
        tb.release()
        nb.release()
    return count, traw, nraw


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("case", B.CASES, ids=B.case_id)
def test_device_bvh_equals_reference_bytes(case, method):
    """The builder's output is fully determined (one rounding per fp32 operation, a stable sort, a
    topology-only PLOC): triangles, node count and every node byte equal the numpy restatement's."""
    want_t, want_n, _ = B.reference(case[0], case[1], method)
    sc = S.build_bvh_device(B.case_triangles(case[0]), _file_order_cornell()[1], case[1], method=method)
    assert sc.nodes.shape[0] == want_n.shape[0]
    _assert_build_equals(sc.triangles, sc.nodes, want_t, want_n)


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("scene", ["soup150k", "bunny"])
def test_device_bvh_two_builds_give_identical_bytes(scene, method):
    """No reference: a climb that read a sibling's box or size before it was published, or an output
    that depended on the order merges were numbered in, would differ from run to run."""
    if scene == "bunny":
        from clrt import proxy
        proxy.bunny_proxy()
        tris = S.load_obj(proxy.os.path.join(proxy.GEN_DIR, "bunny_proxy.obj"), build=False).triangles
    else:
        tris = B.random_soup(150_000, 7)
    mats = _file_order_cornell()[1]
    a, b = (S.build_bvh_device(tris, mats, 4, method=method) for _ in range(2))
    assert a.nodes.shape == b.nodes.shape
    _assert_build_equals(a.triangles, a.nodes, b.triangles, b.nodes)


@pytest.mark.parametrize("method", METHODS)
def test_device_bvh_max_prims_clamp(method):
    """max_prims_in_node 0 builds as 1 and anything above 65535 as 65535 (nPrimitives has 16 bits):
    70,000 copies of one triangle never wrap a leaf's count."""
    tris, mats = B.identical(70_000), _file_order_cornell()[1]
    cache = {}
    built = {mp: S.build_bvh_device(tris, mats, mp, method=method) for mp in (100_000, 0, 1)}
    for mp in (100_000, 0):
        want_t, want_n, _ = B.build(tris, mp, method, cache)
        _assert_build_equals(built[mp].triangles, built[mp].nodes, want_t, want_n)
    big = built[100_000].nodes
    assert 0 < big["nPrimitives"].max() <= 65535 and int(big["nPrimitives"].astype(np.int64).sum()) == 70_000
    assert built[0].nodes.tobytes() == built[1].nodes.tobytes()
    assert built[0].triangles.tobytes() == built[1].triangles.tobytes()
    assert len(built[0].nodes) == 2 * 70_000 - 1


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("max_prims", [1, 4])
def test_device_bvh_writes_nothing_past_its_output(max_prims, method):
    """Triangles past n_tris and every node record from *n_nodes to the buffer's end keep their bytes."""
    import clrt
    tris = B.case_triangles("soup257")
    n = len(tris)
    ctx = clrt.CLContext(0)
    try:
        count, traw, nraw = _build_raw(ctx, tris, max_prims, method, extra_tris=2, extra_nodes=3)
    finally:
        ctx.release()
    want_t, want_n, _ = B.reference("soup257", max_prims, method)
    assert count == len(want_n) and (max_prims != 1 or count == 2 * n - 1)
    _assert_build_equals(traw[:n * 256].view(N.TRIANGLE_DTYPE), nraw[:count * 48].view(N.NODE_DTYPE), want_t, want_n)
    assert (traw[n * 256:] == FILL).all() and traw[n * 256:].size == 2 * 256
    assert (nraw[count * 48:] == FILL).all() and nraw[count * 48:].size == (2 * n - 1 + 3 - count) * 48


def test_device_bvh_errors_leave_the_buffers_alone():
    import ctypes

    import clrt
    tris, _ = _file_order_cornell()
    n = len(tris)
    ctx, other = clrt.CLContext(0), clrt.CLContext(0)
    rw = N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR
    nfill = np.full((2 * n - 1) * 48, FILL, np.uint8)
    tb = ctx.create_buffer(rw, tris.nbytes, tris)
    nb = ctx.create_buffer(rw, nfill.nbytes, nfill)
    short_t = ctx.create_buffer(rw, tris.nbytes - 1, tris)
    short_n = ctx.create_buffer(rw, nfill.nbytes - 1, nfill)
    foreign = other.create_buffer(rw, nfill.nbytes, nfill)
    lib, h = ctx._lib, ctx.handle
    cnt = ctypes.c_size_t(12345)
    out = ctypes.byref(cnt)

    def build(t, n_tris, method, nd, n_nodes=out, max_prims=4):
        rc = lib.rtBuildBVHEx(h, t, n_tris, max_prims, method, nd, n_nodes)
        got_t, got_n = np.empty_like(tris), np.empty_like(nfill)
        ctx.ReadBuffer(tb, got_t, blocking=True)
        ctx.ReadBuffer(nb, got_n, blocking=True)
        assert got_t.tobytes() == tris.tobytes() and got_n.tobytes() == nfill.tobytes(), "an error wrote"
        assert cnt.value == 12345
        return rc

    try:
        for method in (-1, 2, 7):
            assert build(tb.handle, n, method, nb.handle) == -30               # not a method
        assert build(tb.handle, 0, N.BVH_PLOC, nb.handle) == -30               # no triangles
        assert build(tb.handle, 2 ** 30, N.BVH_PLOC, nb.handle) == -30         # n_tris >= 2^30
        assert build(tb.handle, 2 ** 40, N.BVH_LBVH, nb.handle) == -30
        assert build(tb.handle, n, N.BVH_PLOC, nb.handle, None) == -30         # NULL n_nodes
        assert build(None, n, N.BVH_PLOC, nb.handle) == -38                    # NULL buffers
        assert build(tb.handle, n, N.BVH_LBVH, None) == -38
        assert build(foreign.handle, n, N.BVH_PLOC, nb.handle) == -38          # another context's buffer
        assert build(tb.handle, n, N.BVH_PLOC, foreign.handle) == -38
        for method in CODES.values():
            assert build(tb.handle, n, method, tb.handle) == -38               # tris == nodes
        assert build(short_t.handle, n, N.BVH_PLOC, nb.handle) == -61          # triangle buffer < n * 256
        assert build(tb.handle, n + 1, N.BVH_PLOC, nb.handle) == -61
        assert build(tb.handle, n, N.BVH_LBVH, short_n.handle) == -61          # node buffer < (2n - 1) * 48
        # a build after all of them succeeds
        count = ctx.BuildBVH(tb, n, 4, nb, N.BVH_PLOC)
        want_t, want_n, _ = B.reference("cornell", 4, "ploc")
        got_t, got_n = np.empty_like(tris), np.empty(count, N.NODE_DTYPE)
        ctx.ReadBuffer(tb, got_t, blocking=True)
        ctx.ReadBuffer(nb, got_n, got_n.nbytes, blocking=True)
        _assert_build_equals(got_t, got_n, want_t, want_n)
    finally:
        for b in (tb, nb, short_t, short_n, foreign):
            b.release()
        ctx.release()
        other.release()


# ---- build -> bind -> move -> refit -> rebuild in place -> query ----------------------------------
LIFE_W, LIFE_H, LIFE_BOUNCES = 64, 48, 3


def _life_input(name):
    return _file_order_cornell() if name == "cornell" else SS.soup(21, 6000)


def _life_rig(name, max_prims, method, **kw):
    """A kernel bound to read-write buffers that rtBuildBVHEx filled (the node buffer keeps its 2n-1
    records, those past the tree filled with FILL): (rig, node count)."""
    from test_refit_gpu import Mover
    tris, mats = _life_input(name)
    nodes = np.full((2 * len(tris) - 1) * 48, FILL, np.uint8).view(N.NODE_DTYPE)
    m = Mover(S.Scene(tris, nodes, mats, max_prims), LIFE_W, LIFE_H, **kw)
    try:
        count = m.ctx.BuildBVH(m.bufs[0], len(tris), max_prims, m.bufs[1], CODES[method])
    except Exception:
        m.close()
        raise
    return m, count


def _oracle_frames(oracle_mod, steps):
    """Frames accumulated into one image over (scene, frame) steps: (image, counters)."""
    res = np.zeros((LIFE_W * LIFE_H, 4), np.float32)
    counts = dict.fromkeys(SS.COUNTERS, 0)
    for sc, f in steps:
        res, _, _, c = oracle_mod.render(sc, LIFE_W, LIFE_H, frame_count=f, light_bounces=LIFE_BOUNCES,
                                         result=res, threads=16)
        for key in SS.COUNTERS:
            counts[key] += c[key]
    return res, tuple(counts[c] for c in SS.COUNTERS)


def _same_image(got, want):
    return np.array_equal(rgb(got).view(np.uint32), rgb(want).view(np.uint32))


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", ["cornell", "soup6000"])
def test_device_bvh_lifecycle(oracle_mod, name, method):
    """The built buffers through everything added since the builder: bound as they are, moved and
    refitted on the device, rebuilt in place while bound, rendered and queried."""
    from test_ray_query import random_rays
    from test_refit_gpu import cold_start, frames, run_query
    from ray_query_ref import SceneWalker
    tris, mats = _life_input(name)
    m, count = _life_rig(name, 4, method, stats=True)
    try:
        # 1. bound as built
        frames(m)
        out, st = m.result(), m.counters()
        assert m.k.scene_in_lds() == (name == "cornell")
        t1, n1 = m.arrays()
        want_t, want_n, _ = B.build(tris, 4, method)
        assert count == len(want_n)
        _assert_build_equals(t1, n1[:count], want_t, want_n)
        assert (n1[count:].view(np.uint8) == FILL).all()
        built = S.Scene(t1, n1[:count], mats, 4)
        want, wst = _oracle_frames(oracle_mod, [(built, 1), (built, 2)])
        assert _same_image(out, want) and st == wst
        # 2. every vertex moves, the tree is refitted on the device
        m.clear_output()
        m.k.reset_stats()
        m.move(refit_ref.positions(refit_ref.displaced(t1, 7)))
        assert m.k.scene_prepares() == (1, 1)
        frames(m)
        out, st = m.result(), m.counters()
        assert m.k.scene_prepares() == (1, 1)
        t2, n2 = m.arrays()
        assert t2.tobytes() == refit_ref.displaced(t1, 7).tobytes()
        moved = S.Scene(t2, n2[:count], mats, 4)
        diff = B.first_difference(n2[:count], S.refit(S.Scene(t2, n1[:count], mats, 4)).nodes)
        assert diff is None, diff
        assert n2[count:].tobytes() == n1[count:].tobytes()
        want, wst = _oracle_frames(oracle_mod, [(moved, 1), (moved, 2)])
        assert _same_image(out, want) and st == wst
        cold, cst = cold_start(moved)
        assert np.array_equal(out.view(np.uint32), cold.view(np.uint32)) and st == cst
        # 3. rebuilt in place on the bound buffers
        m.clear_output()
        m.k.reset_stats()
        count3 = m.ctx.BuildBVH(m.bufs[0], len(tris), 4, m.bufs[1], CODES[method])
        t3, n3 = m.arrays()
        want_t, want_n, _ = B.build(t2, 4, method)
        assert count3 == len(want_n)
        _assert_build_equals(t3, n3[:count3], want_t, want_n)
        assert n3[count3:].tobytes() == n2[count3:].tobytes()
        m.frame(1, light_bounces=LIFE_BOUNCES)
        assert m.k.scene_prepares() == (2, 1)
        m.frame(2, light_bounces=LIFE_BOUNCES)
        out, st = m.result(), m.counters()
        rebuilt = S.Scene(t3, n3[:count3], mats, 4)
        want, wst = _oracle_frames(oracle_mod, [(rebuilt, 1), (rebuilt, 2)])
        assert _same_image(out, want) and st == wst
        rays = random_rays(rebuilt, 2048)
        walker = SceneWalker(rebuilt)
        for any_hit in (False, True):
            hits = run_query(m, rays, any_hit)
            prim, t, _, _ = walker.walk_rays(rays, any_hit=any_hit)
            assert np.array_equal(hits["prim"], prim), any_hit
            assert np.array_equal(hits["t"].view(np.uint32), t.view(np.uint32)), any_hit
        assert m.k.scene_prepares() == (2, 1)
    finally:
        m.close()


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", ["cornell", "soup6000"])
def test_device_bvh_rebuild_is_ordered_with_queued_frames(oracle_mod, name, method):
    """Coalesced frames queued before a rebuild render the old tree, those after it the new one,
    with or without host waits in between."""
    tris, mats = _life_input(name)
    outs = []
    for finish in (False, True, None):       # None: no rebuild, four frames on the refitted old tree
        m, count = _life_rig(name, 4, method, perframe_batch=None)
        try:
            t1, _ = m.arrays()
            pos = m.stage(refit_ref.positions(refit_ref.displaced(t1, 7)))
            m.move_staged(pos)
            t2, n2 = m.arrays()
            counts = []
            steps = [lambda f=f: m.frame(f, light_bounces=LIFE_BOUNCES) for f in (1, 2, 3, 4)]
            if finish is not None:
                steps.insert(2, lambda: counts.append(
                    m.ctx.BuildBVH(m.bufs[0], len(tris), 4, m.bufs[1], CODES[method])))
            for step in steps:
                step()
                if finish:
                    m.ctx.Finish()
            outs.append(m.result())
            if finish is False:
                t3, n3 = m.arrays()
                old, new = S.Scene(t2, n2[:count], mats, 4), S.Scene(t3, n3[:counts[0]], mats, 4)
        finally:
            m.close()
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert not np.array_equal(outs[0].view(np.uint32), outs[2].view(np.uint32))
    want, _ = _oracle_frames(oracle_mod, [(old, 1), (old, 2), (new, 3), (new, 4)])
    assert _same_image(outs[0], want)

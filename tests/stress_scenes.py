"""Seeded stress fixtures for the parity tests (test_stress_cpu.py, test_stress_gpu.py).

Everything is generated with numpy from fixed seeds; nothing is stored as data.  The fixtures
reach the parts of the hot path that the Cornell box and the bunny proxy leave cold:
  * material_sweeps: GGX lobes with a half vector tilted off the normal -- every regime of
    alpha = 2/roughness^2 - 2 (kernel_bvh.cl:275) and of the exponent 1/(alpha + 1);
  * CAMERAS: axis-aligned rays with exact +0 / -0 direction components (the octant comes from
    invDir < 0, kernel_bvh.cl:42-55; the slab test meets 0 * inf), degenerate bases, a camera
    inside the scene and one in a scene plane;
  * soup: triangle soups with zero-area and duplicate triangles, smooth / zero / tiny / huge
    vertex normals, and optionally overflowing, infinite and NaN vertices;
  * random_tree: hand-built CLLinearBVHNode arrays whose `axis` flags, split positions and
    leaf sizes are unrelated to the geometry, with garbage records past the tree's end.
"""
import functools

import numpy as np

from clrt import _native as N
from clrt import scene as S

SQRT2 = np.sqrt(np.float32(2))
# No fp32 roughness makes alpha exactly -1: r * r == 2 has no fp32 solution (fp32(sqrt 2) squares
# to 2 - 2^-23, its successor to 2 + 2^-22), and 2 / x rounds to 1 for x == 2 only.  The two
# neighbours bracket the pole of 1/(alpha + 1): alpha = -1 + 2^-23 and -1 - 2^-23, exponents
# +2^23 and -2^23 -- the largest finite ones the lobe can see.
SWEEP_VALUES = [0.05, 0.3, 0.5, 0.9, 1.0, 1.2, float(SQRT2), float(np.nextafter(SQRT2, np.float32(2))), 1.5, 2.0,
                5.0, -0.5, 1e-20, 1e20, float("inf"), float("nan")]
MIXED_ROUGHNESS = [0.2, 0.45, 0.7, 0.0, 1.1, 1.35]

CENTER = (0.0, 0.0, 8.5)
DEFAULT = ((0.0, -25.0, 8.5), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
CAMERAS = {
    "up0": ((0.0, -25.0, 8.5), (0.0, 1.0, 0.0), (0.0, 0.0, 0.0)),
    "up0_negzero": ((0.0, -25.0, 8.5), (-0.0, 1.0, -0.0), (0.0, 0.0, 0.0)),
    "axis_x": ((-30.0, 0.0, 8.5), (1.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
    "axis_negz": ((0.5, 0.5, 40.0), (-0.0, -0.0, -1.0), (0.0, 0.0, 0.0)),
    "front0": ((0.0, -25.0, 8.5), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0)),
    "all0": ((0.0, 0.0, 8.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),
    "up_parallel": ((0.0, -25.0, 8.5), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0)),
    "inside": ((0.0, 0.0, 8.5), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)),
    "on_plane": ((0.0, -25.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)),
}


def alpha32(roughness):
    """alpha as material_record (rt_kernels_body.hpp) forms it, in fp32: 2 / (r * r) - 2."""
    with np.errstate(all="ignore"):
        r = np.float32(roughness)
        return np.float32(np.float32(2.0) / np.float32(r * r)) - np.float32(2.0)


def alpha_regime(roughness):
    a = alpha32(roughness)
    if np.isnan(a):
        return "nan"
    if np.isposinf(a):
        return "+inf"
    if a > 0:
        return "finite>0"
    if a == 0:
        return "==0"
    if a > -1 + 2.0 ** -22:
        return "(-1,0)"
    if abs(np.float64(a) + 1.0) <= 2.0 ** -23:
        return "pole-" if a < -1 else "pole"
    return "<-1"


REGIMES = ("+inf", "finite>0", "==0", "(-1,0)", "pole", "pole-", "<-1", "nan")


def sweep_name(v):
    return "r_" + repr(float(v)).replace("-", "m").replace(".", "p").replace("+", "")


def material_sweeps(cornell):
    """{name: Scene}: Cornell's geometry and tree; every material's roughness at one value of
    SWEEP_VALUES with specular 0.5 (several Cornell materials have Ks = 0, which would hide the
    specular lobe), plus "mixed": a different roughness per material, a coloured specular
    above 0.5 and emission on a second material."""
    out = {}
    for v in SWEEP_VALUES:
        m = cornell.materials.copy()
        m["roughness"] = np.float32(v)
        m["specular"][:, :3] = 0.5
        out[sweep_name(v)] = S.Scene(cornell.triangles, cornell.nodes, m, cornell.max_prims_in_node)
    m = cornell.materials.copy()
    k = m.shape[0]
    m["roughness"] = np.resize(np.float32(MIXED_ROUGHNESS), k)
    m["specular"][:, :3] = np.resize(np.float32([[0.9, 0.5, 0.2], [0.3, 1.2, 0.6], [0.5, 0.5, 0.5]]), (k, 3))
    dark = np.flatnonzero(~(m["emission"][:, :3] > 0).any(axis=1))
    m["emission"][dark[0], :3] = (0.2, 1.5, 0.4)
    out["mixed"] = S.Scene(cornell.triangles, cornell.nodes, m, cornell.max_prims_in_node)
    return out


def sweep_light_type(i):
    """Light types 0, 1 and 2 spread over the sweep (index in material_sweeps order)."""
    return i % 3


def soup_materials(rng, k=12):
    m = np.zeros(k, N.MATERIAL_DTYPE)
    rough = [0.0, 0.3, 0.6, 0.9, 1.0, 1.2, float(SQRT2), 1.5, 3.0, -0.5, float(np.nextafter(SQRT2, np.float32(2))), 0.45]
    m["roughness"] = np.resize(np.float32(rough), k)
    m["diffuse"][:, :3] = rng.uniform(0.1, 0.9, (k, 3)).astype(np.float32)
    m["specular"][:, :3] = rng.uniform(0.0, 1.5, (k, 3)).astype(np.float32)
    m["emission"][::4, :3] = rng.uniform(0.5, 3.0, (len(m[::4]), 3)).astype(np.float32)
    m["ior"] = 1.0
    return m


def soup(seed, n=200, nonfinite=False):
    """(triangles, materials) in generation order (no tree): see the module docstring."""
    rng = np.random.default_rng(seed)
    t = np.zeros(n, N.TRIANGLE_DTYPE)
    c = rng.uniform(-4.0, 4.0, (n, 3)).astype(np.float32) + np.float32(CENTER)
    scale = rng.choice(np.float32([0.0, 1.0, 1e-3, 50.0]), n)
    for v in ("v1", "v2", "v3"):
        t[v]["position"][:, :3] = c + rng.normal(0.0, 1.6, (n, 3)).astype(np.float32)
        t[v]["normal"][:, :3] = rng.normal(0.0, 1.0, (n, 3)).astype(np.float32) * scale[:, None]
    pick = rng.permutation(n)
    for i in pick[:8]:                               # zero area: det == 0, inv_det = inf
        t["v3"]["position"][i] = t["v2"]["position"][i]
    mats = soup_materials(rng)
    t["mtlIndex"] = rng.integers(0, mats.shape[0], n)
    for i, j in zip(pick[8:16], pick[16:24]):        # exact duplicates of other triangles
        t[i] = t[j]
    if nonfinite:
        for i in pick[24:27]:                        # products overflow
            t["v1"]["position"][i, :3] *= np.float32(1e30)
        t["v2"]["position"][pick[27], 1] = np.nan
        t["v3"]["position"][pick[28], 2] = np.inf
    return t, mats


def _bounds(tris, lo, hi):
    p = np.concatenate([tris[v]["position"][lo:hi, :3] for v in ("v1", "v2", "v3")]).astype(np.float32)
    ok = np.isfinite(p)
    bmin = np.where(ok, p, np.float32(np.inf)).min(axis=0)
    bmax = np.where(ok, p, np.float32(-np.inf)).max(axis=0)
    none = ~ok.any(axis=0)
    bmin[none] = 0.0
    bmax[none] = 0.0
    return bmin, bmax


def random_tree(tris, rng, max_leaf, chain=False, first_leaf=0):
    """A depth-first CLLinearBVHNode array over `tris` in their given order: random split
    positions, a random axis flag per interior node, a subtree of <= max_leaf triangles made
    a leaf with probability 1/2; bounds = the exact min/max of the finite vertex coordinates.
    chain: split off one triangle at a time (a chain of second children len(tris) - 1 deep).
    first_leaf > 0: the root's first child is one leaf of that many triangles.  Five records
    of garbage follow the tree (check_nodes: records past the tree's end are never read)."""
    nodes = []

    def emit(lo, hi, leaf):
        bmin, bmax = _bounds(tris, lo, hi)
        r = np.zeros((), N.NODE_DTYPE)
        r["bmin"][:3], r["bmax"][:3] = bmin, bmax
        if leaf:
            r["offset"], r["nPrimitives"] = lo, hi - lo
        else:
            r["axis"] = rng.integers(0, 3)
        nodes.append(r)
        return len(nodes) - 1

    def build(lo, hi, force_leaf=False, root=False):
        n = hi - lo
        if force_leaf or n == 1 or (not chain and not (root and first_leaf) and n <= max_leaf and rng.random() < 0.5):
            emit(lo, hi, True)
            return
        me = emit(lo, hi, False)
        if root and first_leaf:
            k = lo + first_leaf
        else:
            k = lo + 1 if chain else int(rng.integers(lo + 1, hi))
        build(lo, k, force_leaf=chain or (root and first_leaf > 0))
        nodes[me]["offset"] = len(nodes)
        build(k, hi)

    build(0, tris.shape[0], root=True)
    out = np.zeros(len(nodes) + 5, N.NODE_DTYPE)
    for i, r in enumerate(nodes):
        out[i] = r
    tail = out[len(nodes):]
    tail["offset"] = 0xDEADBEEF
    tail["nPrimitives"] = [0, 3, 0, 65535, 0]
    tail["axis"] = [7, 0, 2, 255, 1]
    tail["bmin"][:, :3] = rng.normal(0.0, 100.0, (5, 3)).astype(np.float32)
    tail["bmax"][:, :3] = rng.normal(0.0, 100.0, (5, 3)).astype(np.float32)
    return out


def tree_depth(nodes):
    """(depth, node count) of the tree that starts at node 0 (the garbage tail excluded)."""
    depth, end, stack = 0, 0, [(0, 0)]
    while stack:
        i, d = stack.pop()
        end = max(end, i + 1)
        if nodes[i]["nPrimitives"] > 0:
            depth = max(depth, d)
        else:
            stack.append((i + 1, d + 1))
            stack.append((int(nodes[i]["offset"]), d + 1))
    return depth, end


# name -> (soup seed, triangle count, tree kind, tree argument)
SOUP_TREES = {
    "sah1": ("sah", 1), "sah4": ("sah", 4), "rt1": ("random", 1), "rt7": ("random", 7),
    "rt127": ("random", 127), "chain": ("chain", 1), "big": ("big", 140),
}
SOUP_SEEDS = (12, 13)
# the chain holds 60 triangles (the reference's 64-entry stack): its own seeds, picked like
# SOUP_SEEDS so that the coverage floors of test_stress_cpu.py hold
CHAIN_SEEDS = {12: 120, 13: 257}
CHAIN_TRIS = 60


@functools.lru_cache(maxsize=None)
def soup_scene(seed, tree, nonfinite=False):
    """One soup under one of SOUP_TREES.  Hand-built trees keep the generation order (their
    nodes are `tree nodes + 5 garbage records`); the SAH build permutes the triangles.  Built
    once and shared: callers do not modify the arrays."""
    kind, arg = SOUP_TREES[tree]
    if kind == "chain":
        tris, mats = soup(CHAIN_SEEDS[seed], CHAIN_TRIS, nonfinite=nonfinite)
    else:
        tris, mats = soup(seed, 200, nonfinite=nonfinite)
    if kind == "sah":
        return S.build_bvh(tris, mats, arg)
    rng = np.random.default_rng(1000 * seed + arg)
    if kind == "chain":
        nodes = random_tree(tris, rng, 1, chain=True)
    elif kind == "big":  # one leaf too large for the LDS leaf code (> 127): the global-record path
        nodes = random_tree(tris, rng, 7, first_leaf=arg)
    else:
        nodes = random_tree(tris, rng, arg)
    return S.Scene(tris, nodes, mats, max(arg, 1))


def soup_cases():
    return [(seed, tree) for seed in SOUP_SEEDS for tree in SOUP_TREES]


def case_id(case):
    return f"s{case[0]}-{case[1]}"


# the soup/tree pairs rendered through every layout, schedule and launch shape (camera `inside`,
# three frames from frame 0)
PATH_SOUPS = {"s12-rt127": (SOUP_SEEDS[0], "rt127"), "s13-chain": (SOUP_SEEDS[1], "chain")}
PATH_FRAMES = (0, 1, 2)

SOUP_CAMERAS = {"inside": CAMERAS["inside"], "default": DEFAULT, "up0_negzero": CAMERAS["up0_negzero"]}


def packed_camera_bits(cam):
    """The 3 x 16 bytes CLKernel.set_float3 hands to rtSetKernelArg for (pos, front, up),
    captured from the call itself (no library needed)."""
    from clrt.device import CLKernel

    class Probe(CLKernel):
        def __init__(self):
            self.sent = []

        def SetArgument(self, index, data):
            self.sent.append(bytes(data))
            return True

    p = Probe()
    for slot, v in zip((N.CAMERA_POS, N.CAMERA_FRONT, N.CAMERA_UP), cam):
        p.set_float3(slot, v)
    return [np.frombuffer(b, np.uint32) for b in p.sent]


# ---- shared reference renders -------------------------------------------------------------
SWEEP_RUN = dict(W=96, H=64, bounces=6, frames=(0, 1, 2))
SOUP_RUN = dict(W=64, H=48, bounces=9, frames=(0, 1))
COUNTERS = ("rays", "node_visits", "tri_tests", "hits")
_oracle_cache = {}


def oracle_run(oracle, key, scene, W, H, camera, light_type, bounces, frames):
    """The CPU oracle over `frames` into one buffer, computed once per `key` and shared (the
    returned arrays are read-only): radiance, the last frame's primary ids and t, the
    counters summed over the frames."""
    if key not in _oracle_cache:
        res = np.zeros((W * H, 4), np.float32)
        counts = dict.fromkeys(COUNTERS, 0)
        for f in frames:
            res, ids, t, c = oracle.render(scene, W, H, frame_count=f, light_bounces=bounces,
                                           light_type=light_type, camera=camera, result=res,
                                           want_hits=True, threads=16)
            for k in COUNTERS:
                counts[k] += c[k]
        for a in (res, ids, t):
            a.setflags(write=False)
        _oracle_cache[key] = (res, ids, t, counts)
    return _oracle_cache[key]

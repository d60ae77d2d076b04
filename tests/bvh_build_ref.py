"""The device BVH builders (csrc/rt_bvh.hip, rtBuildBVHEx) restated in numpy, and the cases the
builder tests share (test_bvh_build_ref.py on the CPU, test_device_bvh.py on the GPU).

rt_bvh.hip is compiled without contraction or fast math and with correctly rounded division, its sort
is stable and its output depends only on the merge topology, so its bytes are fully determined by the
input.  build() computes the same bytes: every fp32 operation is one numpy float32 operation in the
builder's association, fminf / fmaxf are np.fmin / np.fmax (a NaN operand is dropped).

The two topologies are written from their definitions rather than from the kernels' searches:
  * lbvh: over the 64-bit keys (Morton code << 32 | sorted position) a range splits at the highest
    bit in which its first and last key differ (no Karras direction / length search);
  * ploc: one sequential loop of rounds (no atomics, no arrival counters, no scan); the merges of a
    round are numbered by position, which the output does not depend on.
A zero bound's sign is not specified by rt_hip.h, so no case holds a -0.0 coordinate.
"""
import bisect
import functools

import numpy as np

import stress_scenes as SS
from clrt import _native as N
from clrt import scene as S

F = np.float32
VERTS = ("v1", "v2", "v3")
PLOC_RADIUS = 32          # RT_PLOC_RADIUS
METHODS = ("ploc", "lbvh")
INF = F(np.inf)


def clamp_max_prims(max_prims):
    """rtBuildBVHEx: 0 -> 1, above 65535 -> 65535 (nPrimitives has 16 bits)."""
    return max(1, min(int(max_prims), 65535))


def positions(tris):
    """(n, 3, 3) float32: triangle, vertex, xyz."""
    return np.stack([tris[v]["position"][:, :3] for v in VERTS], axis=1).astype(F)


def centroids(p):
    return ((p[:, 0] + p[:, 1]) + p[:, 2]) * F(1.0 / 3.0)


def _expand_bits(q):
    """10 bits -> every third bit."""
    out = np.zeros(q.shape, np.uint32)
    for b in range(10):
        out |= ((q >> np.uint32(b)) & np.uint32(1)) << np.uint32(3 * b)
    return out


def morton_codes(p):
    """30-bit codes of the centroids within their NaN-dropping bounds, x most significant."""
    c = centroids(p)
    lo = np.fmin.reduce(c, axis=0, initial=INF)
    hi = np.fmax.reduce(c, axis=0, initial=-INF)
    code = np.zeros(len(p), np.uint32)
    for k in range(3):
        ext = hi[k] - lo[k]
        u = (c[:, k] - lo[k]) / ext if ext > 0 else np.zeros(len(p), F)
        u = np.fmin(np.fmax(u, F(0)), F(1))
        q = np.fmin(u * F(1024), F(1023)).astype(np.uint32)
        code |= _expand_bits(q) << np.uint32(2 - k)
    return code


def tri_boxes(p):
    """The bounds rule (rtRefitBVH): the fold over the three vertices starts from +inf / -inf."""
    lo = np.fmin(np.fmin(np.fmin(INF, p[:, 0]), p[:, 1]), p[:, 2])
    hi = np.fmax(np.fmax(np.fmax(-INF, p[:, 0]), p[:, 1]), p[:, 2])
    return lo, hi


def box_area(lo, hi):
    d = hi - lo
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return F(2) * ((dx * dy + dy * dz) + dz * dx)


def _pick_axis(d):
    """The builder's >= chain over three values (a NaN loses every comparison)."""
    return np.where((d[..., 0] >= d[..., 1]) & (d[..., 0] >= d[..., 2]), 0,
                    np.where(d[..., 1] >= d[..., 2], 1, 2)).astype(np.uint8)


def child_axis(alo, ahi, blo, bhi):
    """The axis along which two boxes' centres (as lo + hi) lie furthest apart."""
    return _pick_axis(np.abs((blo + bhi) - (alo + ahi)))


# ---- lbvh ----------------------------------------------------------------------------------------
def _lbvh(codes, mp):
    """Preorder (first triangle, leaf count or 0, second child, depth) of the radix tree."""
    n = len(codes)
    keys = ((codes.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)).tolist()
    first, count, second, depth = [], [], [], []
    stack = [(0, n - 1, 0, -1)]
    while stack:
        lo, hi, d, waiting = stack.pop()
        i = len(first)
        if waiting >= 0:
            second[waiting] = i
        first.append(lo), depth.append(d), second.append(0)
        if hi - lo + 1 <= mp:
            count.append(hi - lo + 1)
            continue
        count.append(0)
        bit = (keys[lo] ^ keys[hi]).bit_length() - 1
        s = bisect.bisect_left(keys, ((keys[lo] >> bit) | 1) << bit, lo, hi + 1)  # first key with `bit` set
        stack.append((s, hi, d + 1, i))
        stack.append((lo, s - 1, d + 1, -1))
    return tuple(np.array(a, np.int64) for a in (first, count, second, depth))


def _range_bounds(first, count, second, depth, tlo, thi):
    """Leaf boxes fold their triangles (the leaves partition the array in order), interior boxes
    their two children, deepest level first."""
    k = len(first)
    lo, hi = np.empty((k, 3), F), np.empty((k, 3), F)
    leaf = count > 0
    lo[leaf] = np.fmin.reduceat(tlo, first[leaf], axis=0)
    hi[leaf] = np.fmax.reduceat(thi, first[leaf], axis=0)
    for d in range(int(depth.max()), -1, -1):
        i = np.flatnonzero(~leaf & (depth == d))
        lo[i] = np.fmin(lo[i + 1], lo[second[i]])
        hi[i] = np.fmax(hi[i + 1], hi[second[i]])
    return lo, hi


# ---- ploc ----------------------------------------------------------------------------------------
def _nearest(lo, hi):
    """Per cluster the neighbour within PLOC_RADIUS positions with the least union area: strict <
    in ascending position, so ties go to the lowest; nothing below +inf -> i - 1 (1 for i == 0)."""
    m, R = len(lo), PLOC_RADIUS
    cost = np.full((m, 2 * R), INF, F)   # columns: positions i-R .. i-1, i+1 .. i+R
    for d in range(1, min(R, m - 1) + 1):
        a = box_area(np.fmin(lo[:-d], lo[d:]), np.fmax(hi[:-d], hi[d:]))
        a = np.where(np.isnan(a), INF, a)
        cost[:m - d, R + d - 1] = a
        cost[d:, R - d] = a
    i = np.arange(m)
    col = cost.argmin(axis=1)            # the first of equal minima
    j = np.where(col < R, i - R + col, i + 1 + col - R)
    return np.where(cost.min(axis=1) < INF, j, np.where(i == 0, 1, i - 1))


def _ploc_merges(tlo, thi):
    """Cluster bottom-up.  Nodes 0 .. n-1 are the sorted triangles, n .. 2n-2 the merges."""
    n = len(tlo)
    blo, bhi = np.empty((2 * n - 1, 3), F), np.empty((2 * n - 1, 3), F)
    blo[:n], bhi[:n] = tlo, thi
    cnt = np.ones(2 * n - 1, np.int64)
    left, right = np.zeros(n - 1, np.int64), np.zeros(n - 1, np.int64)
    clus, nxt, force = np.arange(n), n, False
    st = {"rounds": 0, "forced_rounds": 0, "unclipped_windows": 0}
    while len(clus) > 1:
        m = len(clus)
        st["rounds"] += 1
        if force:
            st["forced_rounds"] += 1
            i = np.arange(0, m - 1, 2)
            j = i + 1
        else:
            st["unclipped_windows"] += max(0, m - 2 * PLOC_RADIUS)
            nn = _nearest(blo[clus], bhi[clus])
            pos = np.arange(m)
            i = pos[(nn[nn] == pos) & (pos < nn)]
            j = nn[i]
        ids = nxt + np.arange(len(i))
        a, b = clus[i], clus[j]
        left[ids - n], right[ids - n] = a, b
        blo[ids], bhi[ids] = np.fmin(blo[a], blo[b]), np.fmax(bhi[a], bhi[b])
        cnt[ids] = cnt[a] + cnt[b]
        keep = np.ones(m, bool)
        keep[j] = False                  # the lower position keeps the new cluster
        clus = clus.copy()
        clus[i] = ids
        clus = clus[keep]
        m_new, nxt = len(clus), nxt + len(i)
        force = m_new == m or (m > 64 and (((m - m_new) * 64) & 0xFFFFFFFF) < m)
    # orient every merge along child_axis: the first child is the lower one
    ax = child_axis(blo[left], bhi[left], blo[right], bhi[right])
    r = np.arange(n - 1)
    swap = (blo[left] + bhi[left])[r, ax] > (blo[right] + bhi[right])[r, ax]
    left, right = np.where(swap, right, left), np.where(swap, left, right)
    st["swaps"], st["non_swaps"] = int(swap.sum()), int((~swap).sum())
    return {"root": int(clus[0]), "left": left, "right": right, "cnt": cnt, "lo": blo, "hi": bhi, "stats": st}


def _ploc_emit(tree, n, mp):
    """Depth-first over the oriented tree: a subtree of <= mp triangles is one leaf whose triangles
    keep the depth-first order of the full tree."""
    left, right, cnt = tree["left"].tolist(), tree["right"].tolist(), tree["cnt"].tolist()
    node, first, count, second, order = [], [], [], [], []
    stack = [(tree["root"], -1)]
    while stack:
        t, waiting = stack.pop()
        i = len(node)
        if waiting >= 0:
            second[waiting] = i
        node.append(t), first.append(len(order)), second.append(0)
        if cnt[t] > mp:
            count.append(0)
            stack.append((right[t - n], i))
            stack.append((left[t - n], -1))
            continue
        count.append(cnt[t])
        inner = [t]
        while inner:
            c = inner.pop()
            if c < n:
                order.append(c)
            else:
                inner.append(right[c - n]), inner.append(left[c - n])
    return tuple(np.array(a, np.int64) for a in (node, first, count, second, order))


# ---- build ---------------------------------------------------------------------------------------
def _histogram(values, size):
    return np.bincount(np.asarray(values, np.int64), minlength=size).tolist()


def build(triangles, max_prims, method, _cache=None):
    """(triangles in leaf order, depth-first NODE_DTYPE records, stats) as rtBuildBVHEx writes them
    for `method` in {"lbvh", "ploc"}.  `_cache`: a dict that callers building the same triangles
    more than once pass along (the Morton order and the PLOC merges do not depend on max_prims)."""
    assert method in METHODS
    tris = np.ascontiguousarray(triangles, dtype=N.TRIANGLE_DTYPE)
    n, mp = len(tris), clamp_max_prims(max_prims)
    cache = {} if _cache is None else _cache
    with np.errstate(all="ignore"):
        if "order" not in cache:
            p = positions(tris)
            codes = morton_codes(p)
            cache["order"] = np.argsort(codes, kind="stable")
            cache["codes"] = codes[cache["order"]]
            cache["boxes"] = tuple(b[cache["order"]] for b in tri_boxes(p))
        order, codes, (tlo, thi) = cache["order"], cache["codes"], cache["boxes"]
        stats = {"equal_code_pairs": int((codes[1:] == codes[:-1]).sum())}
        if method == "lbvh":
            first, count, second, depth = _lbvh(codes, mp)
            lo, hi = _range_bounds(first, count, second, depth, tlo, thi)
            tri_order = order
            axis = _pick_axis(hi - lo)
        else:
            if "ploc" not in cache:
                cache["ploc"] = _ploc_merges(tlo, thi)
            tree = cache["ploc"]
            stats.update(tree["stats"])
            node, first, count, second, leaf_order = _ploc_emit(tree, n, mp)
            lo, hi = tree["lo"][node], tree["hi"][node]
            tri_order = order[leaf_order]
            inner = np.flatnonzero(count == 0)
            a, b = node[inner + 1], node[second[inner]]
            axis = np.zeros(len(node), np.uint8)
            axis[inner] = child_axis(tree["lo"][a], tree["hi"][a], tree["lo"][b], tree["hi"][b])
    leaf = count > 0
    nodes = np.zeros(len(first), N.NODE_DTYPE)
    nodes["bmin"][:, :3], nodes["bmax"][:, :3] = lo, hi
    nodes["offset"] = np.where(leaf, first, second)
    nodes["nPrimitives"] = count
    nodes["axis"] = np.where(leaf, 0, axis)
    stats["axis_hist"] = _histogram(nodes["axis"][~leaf], 3)
    stats["leaf_size_hist"] = _histogram(count[leaf], int(count.max()) + 1)
    return tris[tri_order], nodes, stats


# ---- cases ---------------------------------------------------------------------------------------
def cornell_file_order():
    z = np.load(S.CORNELL_NPZ, allow_pickle=False)
    return z["triangles"].view(N.TRIANGLE_DTYPE), z["materials"].view(N.MATERIAL_DTYPE)


def random_soup(n, seed):
    """test_device_bvh.py's random soup: centres uniform in a 12-unit cube, vertices 0.15 around them."""
    rng = np.random.default_rng(seed)
    out = np.repeat(cornell_file_order()[0][:1], n)
    c = rng.uniform(-6, 6, (n, 3)).astype(F) + F([0, 0, 6])
    for v in VERTS:
        out[v]["position"][:, :3] = c + rng.normal(0, 0.15, (n, 3)).astype(F)
    out["mtlIndex"] = 1
    return out


def coplanar_grid(g=100):
    """test_device_bvh.py's flat grid: 2 * g * g triangles in the plane z = 0."""
    xs, ys = np.meshgrid(np.linspace(-5, 5, g + 1)[:-1], np.linspace(-5, 5, g + 1)[:-1])
    out = np.repeat(cornell_file_order()[0][:1], 2 * g * g)
    d = 10.0 / g
    for k, (dx0, dy0, dx1, dy1, dx2, dy2) in enumerate(((0, 0, d, 0, 0, d), (d, 0, d, d, 0, d))):
        sl = out[k::2]
        for v, dx, dy in (("v1", dx0, dy0), ("v2", dx1, dy1), ("v3", dx2, dy2)):
            sl[v]["position"][:, 0], sl[v]["position"][:, 1] = xs.ravel() + dx, ys.ravel() + dy
            sl[v]["position"][:, 2] = 0.0
        out[k::2] = sl
    out["mtlIndex"] = 1
    return out


def identical(n):
    out = np.repeat(cornell_file_order()[0][10:11], n)
    out["mtlIndex"] = 1
    return out


def one_point(n=500):
    """Different triangles (a, -a, P) with one centroid: a + -a is exactly +0 and 0 + P is P, so every
    centroid is fl(P / 3), every centroid extent 0 and every Morton code 0."""
    rng = np.random.default_rng(5)
    out = np.repeat(cornell_file_order()[0][:1], n)
    a = rng.uniform(0.25, 4.0, (n, 3)).astype(F) * rng.choice(F([-1, 1]), (n, 3))
    out["v1"]["position"][:, :3] = a
    out["v2"]["position"][:, :3] = -a
    out["v3"]["position"][:, :3] = F([1.0, 2.0, 3.0])
    out["mtlIndex"] = 1
    return out


def nonfinite():
    """stress_scenes' non-finite soup, one triangle NaN on y in all three vertices (its y bounds stay
    +inf / -inf under the bounds rule) and one with an all-inf vertex."""
    t = SS.soup(12, 200, nonfinite=True)[0]
    out = np.concatenate([t, t[:2]])
    for v in VERTS:
        out[v]["position"][200, 1] = np.nan
    out["v1"]["position"][201, :3] = np.inf
    return out


SOUP_SIZES = (2, 3, 5, 33, 64, 65, 66, 255, 256, 257, 1025, 4097, 16385)
NAMED = {"cornell": lambda: cornell_file_order()[0].copy(), "identical": lambda: identical(2000),
         "coplanar_grid": coplanar_grid, "one_point": one_point, "nonfinite": nonfinite}


def finite_input(name):
    """Whether every coordinate of the input is finite (test_scene._check_bvh applies)."""
    return name != "nonfinite"


# (input name, max_prims): the one list the CPU and the GPU tests walk
CASES = [(f"soup{n}", mp) for n in SOUP_SIZES for mp in ((1, 2, 4, 8) if n == 257 else (1, 4))]
CASES += [(name, mp) for name in NAMED for mp in (1, 4)]


def case_id(case):
    return f"{case[0]}-mp{case[1]}"


@functools.lru_cache(maxsize=None)
def case_triangles(name):
    """The input of a case, generated once (read-only)."""
    t = random_soup(int(name[4:]), 100 + int(name[4:])) if name.startswith("soup") else NAMED[name]()
    t.setflags(write=False)
    return t


_shared = {}


@functools.lru_cache(maxsize=None)
def reference(name, max_prims, method):
    """build() of a case, computed once and shared (read-only arrays)."""
    tris, nodes, stats = build(case_triangles(name), max_prims, method, _shared.setdefault(name, {}))
    tris.setflags(write=False), nodes.setflags(write=False)
    return tris, nodes, stats


def first_difference(got, want):
    """None when two node arrays are equal byte for byte, else a description of the first record and
    field that differ (bounds and padding compared as bits)."""
    if got.shape != want.shape:
        return f"{got.shape[0]} nodes, expected {want.shape[0]}"
    a = np.ascontiguousarray(got).view(np.uint8).reshape(-1, 48)
    b = np.ascontiguousarray(want).view(np.uint8).reshape(-1, 48)
    bad = np.flatnonzero((a != b).any(axis=1))
    if bad.size == 0:
        return None
    i = int(bad[0])
    for f in N.NODE_DTYPE.names:
        if np.ascontiguousarray(got[f][i]).tobytes() != np.ascontiguousarray(want[f][i]).tobytes():
            return f"node {i} of {len(want)}, field {f}: {got[f][i]!r}, expected {want[f][i]!r} ({bad.size} records differ)"
    return f"node {i}: bytes differ outside the named fields"

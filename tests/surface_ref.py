"""The surface record of a ray hit (rt_surface, rt_hip.h) restated in numpy float32 for pinned math.

Written from the reference's hit record (kernel_bvh.cl:42-55 InitRay, :109-110 the edges, :144-147 pos,
normal and uv) and include/rt_pinned_math.h, not from the device code: every + - * / and sqrt below is
one correctly rounded fp32 operation on float32 arrays, which is what the pinned policy is --
dot = (x x' + y y') + z z', cross.x = a.y b.z - a.z b.y, rsqrt = 1 / sqrt(d) as two operations, and
normalize with its guards (zero vector kept; a squared length below 2^-126 rescaled by 2^86, an
infinite one by 2^-66, and a still infinite one reduced to the signs of its infinite components).
Sums of three products associate as the reference spells them: u n2 + v n3 first, then + w n1 (fp32
addition commutes, so n1 w + (n2 u + n3 v) is the same bits).
"""
import numpy as np

from clrt import _native as N

F = np.float32
MISS_MATERIAL = 0xFFFFFFFF


def _f(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a


def dot(a, b):
    a, b = _f(a), _f(b)
    return _f((a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2])


def cross(a, b):
    a, b = _f(a), _f(b)
    return _f(np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                        a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                        a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1))


def normalize(v):
    """normalize of rt_pinned_math.h, row-wise over an (n, 3) float32 array."""
    v = _f(v).copy()
    with np.errstate(all="ignore"):
        zero = (v == 0).all(axis=-1)
        d = dot(v, v)
        small = d < F(2.0 ** -126)
        big = np.isinf(d) & ~small
        vs = _f(v * F(2.0 ** 86))
        vb = _f(v * F(2.0 ** -66))
        db = dot(vb, vb)
        still = big & np.isinf(db)
        vi = _f(np.copysign(np.where(np.isinf(vb), F(1), F(0)), vb).astype(np.float32))
        v = np.where(small[..., None], vs, np.where(still[..., None], vi, np.where(big[..., None], vb, v)))
        v = _f(v.astype(np.float32))
        d = np.where(small | big, dot(v, v), d)
        r = _f(F(1) / np.sqrt(_f(d)))
        out = _f(v * r[..., None])
    return np.where(zero[..., None], _f(np.asarray(v)), out)


def weighted(a1, a2, a3, u, v):
    """(1 - u - v) a1 + u a2 + v a3 as kernel_bvh.cl:146-147 associates it."""
    w = _f((F(1) - u) - v)
    with np.errstate(all="ignore"):
        return _f(a1 * w[..., None] + (a2 * u[..., None] + a3 * v[..., None]))


def surfaces(triangles, rays, hits):
    """rt_surface records for `hits` (N.RAY_HIT_DTYPE) of `rays` (N.RAY_DTYPE) on `triangles`
    (N.TRIANGLE_DTYPE, BVH leaf order), pinned math."""
    n_tris = len(triangles)
    out = np.zeros(len(hits), N.SURFACE_DTYPE)
    prim = hits["prim"]
    hit = (prim >= 0) & (prim < n_tris)
    out["t"] = hits["t"]
    out["prim"] = np.where(hit, prim, -1)
    out["material"] = MISS_MATERIAL
    if not hit.any():
        return out
    tri = triangles[prim[hit]]
    u, v, t = _f(hits["u"][hit]), _f(hits["v"][hit]), _f(hits["t"][hit])
    with np.errstate(all="ignore"):
        d = normalize(rays["dir"][hit])
        out["position"][hit] = _f(d * t[:, None] + _f(rays["origin"][hit]))
        out["normal"][hit] = normalize(weighted(tri["v1"]["normal"][:, :3], tri["v2"]["normal"][:, :3],
                                                tri["v3"]["normal"][:, :3], u, v))
        out["texcoord"][hit] = weighted(tri["v1"]["uv"][:, :2], tri["v2"]["uv"][:, :2], tri["v3"]["uv"][:, :2], u, v)
        p1 = tri["v1"]["position"][:, :3]
        e1 = _f(tri["v2"]["position"][:, :3] - p1)
        e2 = _f(tri["v3"]["position"][:, :3] - p1)
        out["geo_normal"][hit] = normalize(cross(e1, e2))
    out["material"][hit] = tri["mtlIndex"]
    return out


def fold_features(frames, materials, n_frames):
    """rt_pixel_features from per-frame (hits, surfaces) pairs in frame order: four float32 sums per
    work-item from +0, one addition per hit, then one multiplication by float32(1) / float32(n)."""
    n = len(frames[0][0])
    out = np.zeros(n, N.PIXEL_FEATURES_DTYPE)
    for hits, surf in frames:
        hit = surf["prim"] >= 0
        kd = materials["diffuse"][surf["material"][hit], :3]
        with np.errstate(all="ignore"):
            out["albedo"][hit] = _f(out["albedo"][hit] + kd)
            out["normal"][hit] = _f(out["normal"][hit] + surf["normal"][hit])
            out["depth"][hit] = _f(out["depth"][hit] + surf["t"][hit])
            out["coverage"][hit] = _f(out["coverage"][hit] + F(1))
    inv = F(1) / F(n_frames)
    for f in ("albedo", "normal", "depth", "coverage"):
        out[f] = _f(out[f] * inv)
    return out

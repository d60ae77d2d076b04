"""The motion records and the motion variants of the two reprojections (include/rt_hip.h), restated in numpy
float32 from their definitions: every operation is one correctly rounded fp32 operation in the documented order, so
the device's bytes can be compared with this file's.  Nothing here knows how the device maps records to lanes.

    hit_motion      rtEnqueueHitMotion: miss, moved, vertices, point, normal, record
    centre_rays     rtEnqueueFrameMotion's ray per pixel: origin, dir = (right * sx + up * sy) + front (not
                    normalised), tmin = -inf, tmax = 100000
    temporal        rtEnqueueTemporalAccumulateMotion \\ steps 1, 2 and 5 changed as rt_hip.h says, the rest
    reproject       rtEnqueueReprojectSamplesMotion   / restated once (taps) for both

IEEE leaves the sign and the payload of a NaN that an operation produces open (x86 and gfx950 differ), so
same_motion() takes any NaN for any NaN in the float words of a record; every other word must be equal.
"""
import numpy as np

from clrt import _native as N
from reproject_samples_ref import STATS
from temporal_ref import A, F, MIN_WEIGHT, cross, dot3, view

MOTION = N.PIXEL_MOTION_DTYPE
REASONS = ("outside", "coverage", "depth", "normal", "count")


def vertices(tris, field):
    """(n, 3, 3): triangle, vertex, xyz of `field` ("position" / "normal") of TRIANGLE_DTYPE records."""
    return np.stack([tris[v][field][:, :3] for v in ("v1", "v2", "v3")], axis=1).astype(F)


def tri_points(a):
    """(n, 3, 3) -> n TRI_POINTS_DTYPE records, w slots 0 (what rtEnqueueExtractVertices writes)."""
    out = np.zeros(len(a), N.TRI_POINTS_DTYPE)
    for i, f in enumerate(("p1", "p2", "p3")):
        out[f][:, :3] = a[:, i]
    return out


def points_array(recs):
    return np.stack([recs[f][:, :3] for f in ("p1", "p2", "p3")], axis=1)


def hit_motion(hits, tris, prev_positions=None, prev_normals=None, first_tri=0, n_tris=0):
    """`hits`: RAY_HIT_DTYPE records; `tris`: the scene's TRIANGLE_DTYPE records; prev_*: TRI_POINTS_DTYPE records
    of triangles [first_tri, first_tri + n_tris) or None.  Returns as many MOTION records."""
    hits = np.asarray(hits)
    n_scene = len(tris)
    out = np.zeros(hits.shape, MOTION)
    prim = hits["prim"].astype(np.int64)
    hit = hits["prim"].view(np.uint32).astype(np.uint64) < n_scene          # negative ones are large unsigned ones
    moved = hit & ((prim - first_tri).astype(np.uint64) < np.uint64(n_tris)) if n_tris else np.zeros(hits.shape, bool)
    safe = np.where(hit, prim, 0)
    P, Nn = vertices(tris, "position")[safe], vertices(tris, "normal")[safe]
    if n_tris:
        local = np.where(moved, prim - first_tri, 0)
        P = np.where(moved[..., None, None], points_array(prev_positions)[local], P)
        if prev_normals is not None:
            Nn = np.where(moved[..., None, None], points_array(prev_normals)[local], Nn)
    u, v = hits["u"][..., None], hits["v"][..., None]
    with np.errstate(all="ignore"):
        w = (F(1) - u) - v
        point = P[..., 0, :] * w + (P[..., 1, :] * u + P[..., 2, :] * v)
        nn = Nn[..., 0, :] * w + (Nn[..., 1, :] * u + Nn[..., 2, :] * v)
        l2 = dot3(nn, nn)
        normal = np.where((l2 > 0)[..., None], nn * (F(1) / np.sqrt(l2))[..., None], F(0))
    out["prev_point"] = np.where(hit[..., None], point, F(0))
    out["prev_normal"] = np.where(hit[..., None], normal, F(0))
    out["prim"] = np.where(hit, hits["prim"], -1)
    out["flags"] = moved.astype(np.uint32)
    return out


def centre_rays(width, height, cam, n=None):
    """The rt_ray records of pixels gid = 0 .. n - 1 (default width * height), x = gid % W, y = gid / W."""
    pos, front, up = view(*cam)
    n = width * height if n is None else n
    gid = np.arange(n, dtype=np.int64)
    W, H = F(width), F(height)
    inv_w, inv_h, asp = F(1) / W, F(1) / H, W / H
    x, y = (gid % width).astype(F), (gid // width).astype(F)
    sx = ((F(2) * ((x + F(0.5)) * inv_w) - F(1)) * A) * asp
    sy = (F(2) * ((y + F(0.5)) * inv_h) - F(1)) * A
    right = cross(front, up)
    rays = np.zeros(n, N.RAY_DTYPE)
    rays["origin"] = pos
    rays["dir"] = (right * sx[:, None] + up * sy[:, None]) + front
    rays["tmin"], rays["tmax"] = -np.inf, 100000.0
    return rays


def same_motion(got, want, what):
    """Bytes equal; in the six float words any NaN stands for any NaN."""
    a = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 8)
    b = np.ascontiguousarray(want).view(np.uint32).reshape(-1, 8)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    fa, fb = a.view(F), b.view(F)
    both_nan = np.isnan(fa) & np.isnan(fb)
    both_nan[:, [3, 7]] = False                                # prim and flags are integers
    bad = np.flatnonzero(((a != b) & ~both_nan).any(axis=1))
    assert bad.size == 0, (f"{what}: {bad.size} of {len(a)} records differ, first {bad[:4]}: "
                           f"{np.ascontiguousarray(got).reshape(-1)[bad[:2]]} vs "
                           f"{np.ascontiguousarray(want).reshape(-1)[bad[:2]]}")


def project_point(X, width, height, prev_view):
    """Steps 3 and 4 for the (H, W, 3) points X of any bit pattern: a dict of ok, x0, y0 (int64, 0 where not ok),
    tx, ty, de."""
    ppos, pfront, pup = view(*prev_view)
    W, H = F(width), F(height)
    with np.errstate(all="ignore"):
        v = np.asarray(X, F) - ppos
        zf = dot3(v, pfront)
        ok = zf > 0
        a, b = dot3(v, cross(pfront, pup)) / zf, dot3(v, pup) / zf
        asp = W / H
        ia, ib = F(1) / (A * asp), F(1) / A
        fx = ((a * ia + F(1)) * F(0.5)) * W - F(0.5)
        fy = ((b * ib + F(1)) * F(0.5)) * H - F(0.5)
        de = np.sqrt(dot3(v, v))
        ok = ok & (fx > F(-1)) & (fx < W) & (fy > F(-1)) & (fy < H)
        fx, fy = np.where(ok, fx, F(0)), np.where(ok, fy, F(0))            # (only these become integers)
        x0f, y0f = np.floor(fx), np.floor(fy)
    return {"ok": ok, "x0": x0f.astype(np.int64), "y0": y0f.astype(np.int64), "tx": fx - x0f, "ty": fy - y0f, "de": de}


def taps(centre_ok, centre_normal, pr, hfeat, width, height, depth_tolerance, normal_threshold):
    """Step 5's tap loop up to the feature tests, j outer and i inner: yields (i, j, qy, qx, on, bw, counts_so_far)
    where `on` is the four feature tests (inside, coverage, depth, normal) under the centre's mask."""
    h, w = height, width
    dtol, nthr = F(depth_tolerance), F(normal_threshold)
    ok = centre_ok & pr["ok"]
    with np.errstate(all="ignore"):
        tol = dtol * pr["de"]
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = pr["x0"] + i, pr["y0"] + j
                inside = ok & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                qx, qy = np.where(inside, qx, 0), np.where(inside, qy, 0)
                g = hfeat[qy, qx]
                tests = (inside, g["coverage"] > 0, np.abs(g["depth"] - pr["de"]) <= tol,
                         dot3(centre_normal, g["normal"]) >= nthr)
                bw = (pr["tx"] if i else F(1) - pr["tx"]) * (pr["ty"] if j else F(1) - pr["ty"])
                yield i, j, qy, qx, ok, tests, bw


def _count(info, ok, tests):
    counts = ok
    for name, t in zip(REASONS, tests):
        info["rejected"][name] += int((counts & ~t).sum())
        counts = counts & t
    info["counted"] += counts
    return counts


def temporal(cur, cur_features, hist, hist_features, motion, width, height, cur_view, prev_view, cur_frames=1.0,
             history_frames=0.0, max_history=32.0, depth_tolerance=0.05, normal_threshold=0.9, details=False):
    """rtEnqueueTemporalAccumulateMotion with `motion` given (MOTION records of the current view); the arguments and
    the result are temporal_ref.temporal's."""
    import temporal_ref
    if not temporal_ref.params_ok(cur_view, prev_view, cur_frames, history_frames, max_history, depth_tolerance,
                                  normal_threshold):
        raise ValueError("bad parameters")
    h, w = height, width
    c = np.array(cur, F).reshape(h, w, 4)
    cf, hf, mh = F(cur_frames), F(history_frames), F(max_history)
    out = c.copy()
    out[..., 3] = cf
    info = {"history": np.zeros((h, w), bool), "counted": np.zeros((h, w), np.int64),
            "rejected": dict.fromkeys(REASONS, 0)}
    if hist is None:
        return (out, info) if details else out
    f = np.asarray(cur_features).reshape(h, w)
    m = np.asarray(motion).reshape(h, w)
    hc = np.asarray(hist, F).reshape(h, w, 4)
    hfeat = np.asarray(hist_features).reshape(h, w)
    pr = project_point(m["prev_point"], w, h, prev_view)                     # 2, 3, 4
    centre = (f["coverage"] > 0) & (m["prim"] >= 0)                         # 1
    sw, sn = np.zeros((h, w), F), np.zeros((h, w), F)
    s = [np.zeros((h, w), F) for _ in range(3)]
    with np.errstate(all="ignore"):
        for i, j, qy, qx, ok, tests, bw in taps(centre, m["prev_normal"], pr, hfeat, w, h, depth_tolerance,
                                                normal_threshold):           # 5
            hq = hc[qy, qx]
            nq = np.full((h, w), hf, F) if hf != 0 else hq[..., 3]
            counts = _count(info, ok, tests + (nq >= F(1),))
            sw = np.where(counts, sw + bw, sw)
            for ch in range(3):
                s[ch] = np.where(counts, s[ch] + bw * hq[..., ch], s[ch])
            sn = np.where(counts, sn + bw * nq, sn)
        has = sw >= MIN_WEIGHT                                               # 6
        n = np.fmin(sn / sw + cf, mh)
        alpha = cf / n
        for ch in range(3):
            hh = s[ch] / sw
            out[..., ch] = np.where(has, hh + (c[..., ch] - hh) * alpha, c[..., ch])
        out[..., 3] = np.where(has, n, cf)
    info["history"] = has
    info["projection"] = pr
    return (out, info) if details else out


def reproject(hist_stats, hist_features, cur_features, motion, width, height, cur_view, prev_view, max_history=16.0,
              depth_tolerance=0.05, normal_threshold=0.9, details=False):
    """rtEnqueueReprojectSamplesMotion with `motion` given; the arguments and the result are
    reproject_samples_ref.reproject's."""
    import reproject_samples_ref
    if not reproject_samples_ref.params_ok(cur_view, prev_view, max_history, depth_tolerance, normal_threshold):
        raise ValueError("bad parameters")
    h, w = height, width
    f = np.asarray(cur_features).reshape(h, w)
    m = np.asarray(motion).reshape(h, w)
    hs = np.asarray(hist_stats).reshape(h, w)
    hfeat = np.asarray(hist_features).reshape(h, w)
    mh = F(max_history)
    info = {"counted": np.zeros((h, w), np.int64), "rejected": dict.fromkeys(REASONS, 0)}
    out = np.zeros((h, w), STATS)
    pr = project_point(m["prev_point"], w, h, prev_view)
    centre = (f["coverage"] > 0) & (m["prim"] >= 0)
    zero = np.zeros((h, w), F)
    sw, sy, ss, sn = zero, zero, zero, zero
    sm = [zero, zero, zero]
    with np.errstate(all="ignore"):
        for i, j, qy, qx, ok, tests, bw in taps(centre, m["prev_normal"], pr, hfeat, w, h, depth_tolerance,
                                                normal_threshold):
            st = hs[qy, qx]
            n = st["n"]
            counts = _count(info, ok, tests + (n >= F(1),))
            sv = np.where(n >= F(2), st["m2_y"] / (n - F(1)), st["mean_y"] * st["mean_y"])
            sw = np.where(counts, sw + bw, sw)
            for ch in range(3):
                sm[ch] = np.where(counts, sm[ch] + bw * (st["sum"][..., ch] / n), sm[ch])
            sy = np.where(counts, sy + bw * st["mean_y"], sy)
            ss = np.where(counts, ss + bw * sv, ss)
            sn = np.where(counts, sn + bw * n, sn)
        has = sw >= MIN_WEIGHT
        n2 = np.fmin(np.floor(sn / sw), mh)
        for ch in range(3):
            out["sum"][..., ch] = np.where(has, (sm[ch] / sw) * n2, F(0))
        out["n"] = np.where(has, n2, F(0))
        out["mean_y"] = np.where(has, sy / sw, F(0))
        out["m2_y"] = np.where(has & (n2 >= F(2)), (ss / sw) * (n2 - F(1)), F(0))
    info["carried"] = has
    info["projection"] = pr
    return (out, info) if details else out

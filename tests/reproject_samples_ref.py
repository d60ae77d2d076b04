"""The reprojection of the adaptive sample statistics, rtEnqueueReprojectSamples (include/rt_hip.h),
restated in numpy float32 from its definition: every operation is one correctly rounded fp32 operation in
the documented order, so the device's bytes can be compared with this file's.  Nothing here knows how the
device maps pixels to lanes.  Pixels that a step rules out are carried along under a mask and selected away
with np.where; a float becomes an integer only for pixels that passed the range test of step 4.

    1 nothing carried unless coverage > 0                     -> 32 zero bytes
    2 X = cur.pos + u * depth, u the unit centre ray of the pixel (temporal_ref.centre_rays)
    3 v = X - prev.pos, zf = dot3(v, prev.front) > 0; fx, fy the pixel coordinates in the previous view
    4 -1 < fx < W and -1 < fy < H; x0 = floor(fx), tx = fx - x0
    5 four taps, j outer, i inner; a tap counts when inside, covered, depth within tolerance of |v|,
      normals alike, s.n >= 1; m = sum / n, sv = n >= 2 ? m2_y / (n - 1) : mean_y * mean_y; sums of bw,
      bw * m, bw * mean_y, bw * sv, bw * n over the taps that count
    6 sw >= 2^-6; n' = fmin(floor(sn / sw), max_history), sum = (sm / sw) * n', mean_y = sy / sw,
      m2_y = n' >= 2 ? (ss / sw) * (n' - 1) : 0
"""
import numpy as np

import temporal_ref
from temporal_ref import A, F, MIN_WEIGHT, cross, dot3, view

STATS = np.dtype([("sum", np.float32, (3,)), ("n", np.float32), ("mean_y", np.float32), ("m2_y", np.float32),
                  ("reserved", np.uint32, (2,))])
MAX_HISTORY = 2.0 ** 20
REASONS = ("outside", "coverage", "depth", "normal", "count")


def params_ok(cur_view, prev_view, max_history, depth_tolerance, normal_threshold):
    vals = [F(c) for v in (cur_view, prev_view) for part in v for c in part]
    mh, dt, nt = F(max_history), F(depth_tolerance), F(normal_threshold)
    return bool(all(np.isfinite(v) for v in vals) and np.isfinite(mh) and 1 <= mh <= MAX_HISTORY and
                np.floor(mh) == mh and np.isfinite(dt) and 0 <= dt <= 1 and np.isfinite(nt) and -1 <= nt <= 1)


def reproject(hist_stats, hist_features, cur_features, width, height, cur_view, prev_view, max_history=16.0,
              depth_tolerance=0.05, normal_threshold=0.9, details=False):
    """`hist_stats`: width * height records of STATS' layout; the features: as many records with the fields
    albedo, depth, normal, coverage; a view: (pos, front, up).  Returns the (height, width) STATS result; with
    details=True also a dict: `carried` (H, W) the pixels that keep statistics, `counted` (H, W) their number of
    counted taps, `rejected` {reason: taps first ruled out by it}, in the order of REASONS, `fetched` the number of
    taps whose features passed, the only ones whose statistics matter."""
    if not params_ok(cur_view, prev_view, max_history, depth_tolerance, normal_threshold):
        raise ValueError("bad parameters")
    h, w = height, width
    f = np.asarray(cur_features).reshape(h, w)
    hs = np.asarray(hist_stats).reshape(h, w)
    hfeat = np.asarray(hist_features).reshape(h, w)
    mh, dtol, nthr = F(max_history), F(depth_tolerance), F(normal_threshold)
    cpos, cfront, cup = view(*cur_view)
    ppos, pfront, pup = view(*prev_view)
    W, H = F(w), F(h)
    info = {"counted": np.zeros((h, w), np.int64), "rejected": dict.fromkeys(REASONS, 0), "fetched": 0}
    out = np.zeros((h, w), STATS)
    with np.errstate(all="ignore"):
        ok = f["coverage"] > 0                                             # 1
        u = temporal_ref.centre_rays(w, h, cfront, cup)                    # 2
        X = cpos + u * f["depth"][..., None]
        v = X - ppos                                                       # 3
        zf = dot3(v, pfront)
        ok = ok & (zf > 0)
        a, b = dot3(v, cross(pfront, pup)) / zf, dot3(v, pup) / zf
        asp = W / H
        ia, ib = F(1) / (A * asp), F(1) / A
        fx = ((a * ia + F(1)) * F(0.5)) * W - F(0.5)
        fy = ((b * ib + F(1)) * F(0.5)) * H - F(0.5)
        de = np.sqrt(dot3(v, v))
        ok = ok & (fx > F(-1)) & (fx < W) & (fy > F(-1)) & (fy < H)        # 4
        fx, fy = np.where(ok, fx, F(0)), np.where(ok, fy, F(0))            # (only these become integers)
        x0f, y0f = np.floor(fx), np.floor(fy)
        tx, ty = fx - x0f, fy - y0f
        x0, y0 = x0f.astype(np.int64), y0f.astype(np.int64)
        zero = np.zeros((h, w), F)                                         # 5
        sw, sy, ss, sn = zero, zero, zero, zero
        sm = [zero, zero, zero]
        tol = dtol * de
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j
                inside = ok & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                qx, qy = np.where(inside, qx, 0), np.where(inside, qy, 0)
                g, s = hfeat[qy, qx], hs[qy, qx]
                n = s["n"]
                tests = (inside, g["coverage"] > 0, np.abs(g["depth"] - de) <= tol,
                         dot3(f["normal"], g["normal"]) >= nthr, n >= F(1))
                counts = ok
                for name, t in zip(REASONS, tests):
                    if name == "count":
                        info["fetched"] += int(counts.sum())
                    info["rejected"][name] += int((counts & ~t).sum())
                    counts = counts & t
                sv = np.where(n >= F(2), s["m2_y"] / (n - F(1)), s["mean_y"] * s["mean_y"])
                bw = (tx if i else F(1) - tx) * (ty if j else F(1) - ty)
                sw = np.where(counts, sw + bw, sw)
                for ch in range(3):
                    sm[ch] = np.where(counts, sm[ch] + bw * (s["sum"][..., ch] / n), sm[ch])
                sy = np.where(counts, sy + bw * s["mean_y"], sy)
                ss = np.where(counts, ss + bw * sv, ss)
                sn = np.where(counts, sn + bw * n, sn)
                info["counted"] += counts
        has = sw >= MIN_WEIGHT                                             # 6
        n2 = np.fmin(np.floor(sn / sw), mh)
        for ch in range(3):
            out["sum"][..., ch] = np.where(has, (sm[ch] / sw) * n2, F(0))
        out["n"] = np.where(has, n2, F(0))
        out["mean_y"] = np.where(has, sy / sw, F(0))
        out["m2_y"] = np.where(has & (n2 >= F(2)), (ss / sw) * (n2 - F(1)), F(0))
    info["carried"] = has
    return (out, info) if details else out

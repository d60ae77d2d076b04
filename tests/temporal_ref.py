"""The temporal reprojection of rtEnqueueTemporalAccumulate (include/rt_hip.h), restated in numpy float32
from its definition: every operation is one correctly rounded fp32 operation in the documented order,
so the device's bytes can be compared with this file's.  Nothing here knows how the device maps pixels
to lanes.  Pixels that a step rules out are carried along under a mask and selected away with np.where;
a float becomes an integer only for pixels that passed the range test of step 4.

    1 no history: hist None, or !(coverage > 0)            -> {c.rgb, cur_frames}
    2 X = cur.pos + u * depth, u the unit centre ray of the pixel
    3 v = X - prev.pos, zf = dot3(v, prev.front) > 0; fx, fy the pixel coordinates in the previous view
    4 -1 < fx < W and -1 < fy < H; x0 = floor(fx), tx = fx - x0
    5 four taps, j outer, i inner; a tap counts when inside, covered, depth within tolerance of |v|,
      normals alike, n_q >= 1; sums of bw, bw * rgb, bw * n_q over the taps that count
    6 sw >= 2^-6; h = s / sw, n = fmin(hn + cur_frames, max_history), out = h + (c - h) * (cur_frames / n)
"""
import numpy as np

F = np.float32
A = F(float.fromhex("0x1.a82408p-2"))
MIN_WEIGHT = F(2.0 ** -6)
MAX_FRAMES = 2.0 ** 20
REASONS = ("outside", "coverage", "depth", "normal", "count")


def dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], F)


def view(pos, front, up):
    return tuple(np.asarray(v, F) for v in (pos, front, up))


def centre_rays(width, height, front, up):
    """Step 2's unit direction u of every pixel, (H, W, 3)."""
    W, H = F(width), F(height)
    inv_w, inv_h, asp = F(1) / W, F(1) / H, W / H
    x = np.arange(width, dtype=np.int64).astype(F)[None, :]
    y = np.arange(height, dtype=np.int64).astype(F)[:, None]
    sx = np.broadcast_to(((F(2) * ((x + F(0.5)) * inv_w) - F(1)) * A) * asp, (height, width))
    sy = np.broadcast_to((F(2) * ((y + F(0.5)) * inv_h) - F(1)) * A, (height, width))
    right = cross(front, up)
    d = (right * sx[..., None] + np.asarray(up, F) * sy[..., None]) + np.asarray(front, F)
    return d * (F(1) / np.sqrt(dot3(d, d)))[..., None]


def params_ok(cur_view, prev_view, cur_frames, history_frames, max_history, depth_tolerance, normal_threshold):
    vals = [F(c) for v in (cur_view, prev_view) for part in v for c in part]
    cf, hf, mh, dt, nt = F(cur_frames), F(history_frames), F(max_history), F(depth_tolerance), F(normal_threshold)
    return bool(all(np.isfinite(v) for v in vals) and np.isfinite(cf) and 1 <= cf <= MAX_FRAMES and
                (hf == 0 or (np.isfinite(hf) and 1 <= hf <= MAX_FRAMES)) and
                np.isfinite(mh) and cf <= mh <= MAX_FRAMES and np.isfinite(dt) and 0 <= dt <= 1 and
                np.isfinite(nt) and -1 <= nt <= 1)


def temporal(cur, cur_features, hist, hist_features, width, height, cur_view, prev_view, cur_frames=1.0,
             history_frames=0.0, max_history=32.0, depth_tolerance=0.05, normal_threshold=0.9, details=False):
    """`cur`, `hist`: width * height slots {r, g, b, w} float32 (`hist` and `hist_features` None: no
    history); the features: as many records with the fields albedo, depth, normal, coverage; a view:
    (pos, front, up).  Returns the (height, width, 4) float32 result; with details=True also a dict:
    `history` (H, W) the pixels that blend, `counted` (H, W) their number of counted taps, `rejected`
    {reason: taps first ruled out by it}, in the order outside, coverage, depth, normal, count."""
    if not params_ok(cur_view, prev_view, cur_frames, history_frames, max_history, depth_tolerance, normal_threshold):
        raise ValueError("bad parameters")
    if (hist is None) != (hist_features is None):
        raise ValueError("hist and hist_features go together")
    h, w = height, width
    c = np.array(cur, F).reshape(h, w, 4)
    cf, hf, mh = F(cur_frames), F(history_frames), F(max_history)
    dtol, nthr = F(depth_tolerance), F(normal_threshold)
    out = c.copy()
    out[..., 3] = cf
    info = {"history": np.zeros((h, w), bool), "counted": np.zeros((h, w), np.int64),
            "rejected": dict.fromkeys(REASONS, 0)}
    if hist is None:
        return (out, info) if details else out
    f = np.asarray(cur_features).reshape(h, w)
    hc = np.asarray(hist, F).reshape(h, w, 4)
    hfeat = np.asarray(hist_features).reshape(h, w)
    cpos, cfront, cup = view(*cur_view)
    ppos, pfront, pup = view(*prev_view)
    W, H = F(w), F(h)
    with np.errstate(all="ignore"):
        ok = f["coverage"] > 0                                             # 1
        u = centre_rays(w, h, cfront, cup)                                 # 2
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
        sw, sn = np.zeros((h, w), F), np.zeros((h, w), F)                  # 5
        s = [np.zeros((h, w), F) for _ in range(3)]
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j
                inside = ok & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                qx, qy = np.where(inside, qx, 0), np.where(inside, qy, 0)
                fq, hq = hfeat[qy, qx], hc[qy, qx]
                nq = np.full((h, w), hf, F) if hf != 0 else hq[..., 3]
                tests = (inside, fq["coverage"] > 0, np.abs(fq["depth"] - de) <= dtol * de,
                         dot3(f["normal"], fq["normal"]) >= nthr, nq >= F(1))
                counts = ok
                for name, t in zip(REASONS, tests):
                    info["rejected"][name] += int((counts & ~t).sum())
                    counts = counts & t
                bw = (tx if i else F(1) - tx) * (ty if j else F(1) - ty)
                sw = np.where(counts, sw + bw, sw)
                for ch in range(3):
                    s[ch] = np.where(counts, s[ch] + bw * hq[..., ch], s[ch])
                sn = np.where(counts, sn + bw * nq, sn)
                info["counted"] += counts
        has = sw >= MIN_WEIGHT                                             # 6
        n = np.fmin(sn / sw + cf, mh)
        alpha = cf / n
        for ch in range(3):
            hh = s[ch] / sw
            out[..., ch] = np.where(has, hh + (c[..., ch] - hh) * alpha, c[..., ch])
        out[..., 3] = np.where(has, n, cf)
    info["history"] = has
    return (out, info) if details else out

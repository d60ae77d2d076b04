"""A numpy float32 restatement of the four adaptive-sampling definitions of include/rt_hip.h
(rtEnqueueAccumulateSamples, rtEnqueueSelectPixels, rtEnqueueCameraPathsFor's indexing, rtEnqueueResolveSamples):
one np.float32 operation per operation of the header, in its order, so nothing is contracted and every division
is the IEEE one.  pm_pow comes through the oracle library's oracle_pow.  The GPU tests compare bytes with it.
"""
import numpy as np

F = np.float32
FLT_MAX = np.finfo(np.float32).max
STATS = np.dtype([("sum", np.float32, (3,)), ("n", np.float32), ("mean_y", np.float32), ("m2_y", np.float32),
                  ("reserved", np.uint32, (2,))])
RESULT = np.dtype([("radiance", np.float32, (3,)), ("prim", np.int32)])
assert STATS.itemsize == 32 and RESULT.itemsize == 16


def luminance(s):
    s = np.asarray(s, np.float32)
    return (F(0.2126) * s[..., 0] + F(0.7152) * s[..., 1]) + F(0.0722) * s[..., 2]


def accumulate(stats, ids, results, first, n, n_pixels):
    """stats after rtEnqueueAccumulateSamples over records [first, first + n); `stats` (flat STATS array) is not
    modified.  The ids of the range must be distinct where they are in range."""
    out = np.array(stats, STATS, copy=True).reshape(-1)
    idx = (np.arange(first, first + n, dtype=np.uint32) if ids is None
           else np.asarray(ids, np.uint32)[first:first + n])
    s = np.asarray(results, RESULT)["radiance"][first:first + n]
    with np.errstate(all="ignore"):
        ok = (idx < np.uint64(n_pixels)) & (np.abs(s) <= FLT_MAX).all(axis=1)
        p = idx[ok].astype(np.int64)
        assert len(np.unique(p)) == len(p), "the restatement takes distinct ids"
        s = s[ok]
        y = luminance(s)
        n0, mean0, m20 = out["n"][p], out["mean_y"][p], out["m2_y"][p]
        n1 = n0 + F(1.0)
        d = y - mean0
        mean1 = mean0 + d / n1
        m21 = m20 + d * (y - mean1)
        out["sum"][p] = out["sum"][p] + s
    out["n"][p], out["mean_y"][p], out["m2_y"][p] = n1, mean1, m21
    return out


def hot_flags(stats, threshold, floor_y):
    st = np.asarray(stats, STATS)
    n, mean, m2 = st["n"], st["mean_y"], st["m2_y"]
    with np.errstate(all="ignore"):
        v = (m2 / (n - F(1.0))) / n
        b = F(threshold) * (mean + F(floor_y))
        return (n >= F(2.0)) & (v > b * b)


def select(stats, width, height, threshold=0.05, floor_y=0.01, min_samples=4, max_samples=64, radius=1):
    """(ids, hot count): rtEnqueueSelectPixels' ascending list and the second word of its result."""
    st = np.asarray(stats, STATS).reshape(height, width)
    hot = hot_flags(st, threshold, floor_y)
    near = np.zeros_like(hot)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            ys, yd = slice(max(dy, 0), height + min(dy, 0)), slice(max(-dy, 0), height + min(-dy, 0))
            xs, xd = slice(max(dx, 0), width + min(dx, 0)), slice(max(-dx, 0), width + min(-dx, 0))
            near[yd, xd] |= hot[ys, xs]
    n = st["n"]
    with np.errstate(invalid="ignore"):
        always = n < F(min_samples)
        never = ~always & (n >= F(max_samples))
    sel = always | (~always & ~never & near)
    return np.flatnonzero(sel.reshape(-1)).astype(np.uint32), int(hot.sum())


_pow = None


def gamma(x):
    """pm_pow(x, 0.45454545f) element-wise, through the oracle library."""
    global _pow
    if _pow is None:
        import oracle
        _pow = oracle.lib().oracle_pow
    x = np.asarray(x, np.float32)
    e = float(F(0.45454545))
    return np.array([_pow(float(v), e) for v in x.reshape(-1)], np.float32).reshape(x.shape)


def resolve(stats):
    """rtEnqueueResolveSamples' image, (pixels, 4) float32."""
    st = np.asarray(stats, STATS).reshape(-1)
    out = np.zeros((len(st), 4), np.float32)
    with np.errstate(all="ignore"):
        nz = ~(st["n"] == F(0.0))
        out[nz, :3] = gamma(st["sum"][nz] / st["n"][nz, None])
    out[nz, 3] = st["n"][nz]
    return out

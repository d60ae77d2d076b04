"""The variance-guided a-trous denoiser of rtEnqueueDenoiseSamples (include/rt_hip.h), restated in numpy
float32 from its definition: every operation is one correctly rounded fp32 operation in the documented
order, so the device's bytes can be compared with this file's.  Nothing here knows how the device tiles.

    iteration 0 reads c = sum / n and v = n >= 2 ? (m2_y / (n - 1)) / n : mean_y^2 (n < 1: c = 0, v = -1)
    a pixel counts when coverage != 0 and v >= 0; a centre that does not count keeps {r, g, b, v}
    tol = sigma_luminance * sqrt(gv) + epsilon, gv the {1/4, 1/2, 1/4}^2 mean of v over the counting inner 3 x 3
    w = ((((k e(|l_p - l_q| / tol)) e(x_n)) e(x_z)) e(x_a)), a term with sigma 0 left out
    rgb = s_rgb / sw, v' = s_v / (sw sw) with s_v += (w w) v_q
    out = {enc(rgb), n}, variance = v'; a pixel with n < 1 gets zeros
"""
import numpy as np

from denoise_ref import H5, MAX_ITERATIONS, dot3, edge, inv_sq, shifted, sigma_ok

F = np.float32
G3 = [F(0.25), F(0.5), F(0.25)]
EPSILON_MIN, EPSILON_MAX = 2.0 ** -40, 2.0 ** 20
LINEAR, GAMMA = 0, 1
STATS = np.dtype([("sum", np.float32, (3,)), ("n", np.float32), ("mean_y", np.float32), ("m2_y", np.float32),
                  ("reserved", np.uint32, (2,))])


def luminance(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def epsilon_ok(e) -> bool:
    e = F(e)
    return bool(np.isfinite(e) and EPSILON_MIN <= e <= EPSILON_MAX)


def stats_cells(stats):
    """The {r, g, b, v} input of iteration 0 from an array of STATS records (one more axis of 4)."""
    st = np.asarray(stats, STATS)
    n, mean, m2 = st["n"], st["mean_y"], st["m2_y"]
    cells = np.zeros(st.shape + (4,), np.float32)
    with np.errstate(all="ignore"):
        has = n >= F(1)
        v = np.where(n >= F(2), (m2 / (n - F(1))) / n, mean * mean)
        cells[..., :3] = np.where(has[..., None], st["sum"] / n[..., None], F(0))
        cells[..., 3] = np.where(has, v, F(-1))
    return cells


def counting(cells, coverage):
    with np.errstate(invalid="ignore"):
        return (coverage != 0) & (cells[..., 3] >= F(0))


def tolerance(cells, counts, step, sigma_luminance, epsilon):
    """sigma_luminance * sqrt(gv) + epsilon per pixel (meaningful where the centre counts)."""
    h, w = counts.shape
    sg, sv = np.zeros((h, w), np.float32), np.zeros((h, w), np.float32)
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            ox, oy = step * dx, step * dy
            vq, inside = shifted(cells[..., 3], ox, oy)
            ok = inside & shifted(counts, ox, oy)[0]
            g = G3[dy + 1] * G3[dx + 1]
            sg = np.where(ok, sg + g, sg)
            sv = np.where(ok, sv + g * vq, sv)
    return F(sigma_luminance) * np.sqrt(sv / sg) + F(epsilon)


def iteration(cells, albedo, depth, normal, coverage, step, sigma_luminance, epsilon, inv_n, inv_z, inv_a):
    """One iteration over (H, W, 4) cells {r, g, b, v} and (H, W[, 3]) guides, all float32."""
    h, w = cells.shape[:2]
    counts = counting(cells, coverage)
    on_l = F(sigma_luminance) != 0
    tol = tolerance(cells, counts, step, sigma_luminance, epsilon)
    lum = luminance(cells)
    rz = F(1) / np.maximum(np.abs(depth), F(2.0 ** -64))
    sums = [np.zeros((h, w), np.float32) for _ in range(5)]  # w, r, g, b, v
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            ox, oy = step * dx, step * dy
            cq, inside = shifted(cells, ox, oy)
            ok = inside & shifted(counts, ox, oy)[0]
            wgt = np.full((h, w), H5[dy + 2] * H5[dx + 2], np.float32)
            if on_l:
                wgt = wgt * edge(np.abs(lum - shifted(lum, ox, oy)[0]) / tol)
            if inv_n is not None:
                wgt = wgt * edge(dot3(normal - shifted(normal, ox, oy)[0]) * inv_n)
            if inv_z is not None:
                d = (depth - shifted(depth, ox, oy)[0]) * rz
                wgt = wgt * edge((d * d) * inv_z)
            if inv_a is not None:
                wgt = wgt * edge(dot3(albedo - shifted(albedo, ox, oy)[0]) * inv_a)
            sums[0] = np.where(ok, sums[0] + wgt, sums[0])
            for c in range(3):
                sums[1 + c] = np.where(ok, sums[1 + c] + wgt * cq[..., c], sums[1 + c])
            sums[4] = np.where(ok, sums[4] + (wgt * wgt) * cq[..., 3], sums[4])
    out = cells.copy()
    for c in range(3):
        out[..., c] = np.where(counts, sums[1 + c] / sums[0], cells[..., c])
    out[..., 3] = np.where(counts, sums[4] / (sums[0] * sums[0]), cells[..., 3])
    return out


def filtered_cells(stats, features, width, height, iterations=3, sigma_luminance=8.0, sigma_normal=0.5,
                   sigma_depth=0.1, sigma_albedo=0.25, epsilon=1e-4):
    """The {r, g, b, v} image after the last iteration, (height, width, 4) float32, before the output rule."""
    if not 1 <= iterations <= MAX_ITERATIONS:
        raise ValueError("iterations outside 1..5")
    for s in (sigma_luminance, sigma_normal, sigma_depth, sigma_albedo):
        if not sigma_ok(s):
            raise ValueError("bad sigma")
    if not epsilon_ok(epsilon):
        raise ValueError("bad epsilon")
    cells = stats_cells(np.asarray(stats, STATS).reshape(height, width))
    f = np.asarray(features).reshape(height, width)
    albedo = np.ascontiguousarray(f["albedo"], np.float32)
    normal = np.ascontiguousarray(f["normal"], np.float32)
    depth = np.ascontiguousarray(f["depth"], np.float32)
    coverage = np.ascontiguousarray(f["coverage"], np.float32)
    inv_n, inv_z, inv_a = inv_sq(sigma_normal), inv_sq(sigma_depth), inv_sq(sigma_albedo)
    with np.errstate(all="ignore"):
        for i in range(iterations):
            cells = iteration(cells, albedo, depth, normal, coverage, 1 << i, sigma_luminance, epsilon, inv_n, inv_z,
                              inv_a)
    return cells


def output(cells, stats, encoding=GAMMA):
    """(out (H, W, 4), variance (H, W)) from the last iteration's cells: {enc(rgb), n} and v, zeros where n < 1."""
    if encoding not in (LINEAR, GAMMA):
        raise ValueError("bad encoding")
    h, w = cells.shape[:2]
    n = np.asarray(stats, STATS).reshape(h, w)["n"]
    with np.errstate(invalid="ignore"):
        has = n >= F(1)
    out = np.zeros((h, w, 4), np.float32)
    var = np.zeros((h, w), np.float32)
    rgb = cells[..., :3][has]
    if encoding == GAMMA:
        import adaptive_ref
        rgb = adaptive_ref.gamma(rgb)
    out[has, :3] = rgb
    out[has, 3] = n[has]
    var[has] = cells[..., 3][has]
    return out, var


FEATURES = np.dtype([("albedo", np.float32, (3,)), ("depth", np.float32), ("normal", np.float32, (3,)),
                     ("coverage", np.float32)])
COUNTS = np.float32([0, 1, 2, 5, 40, 3000])


def synthetic(w, h):
    """Seeded inputs the tests share (read-only): (stats (h, w) STATS, features (h, w) FEATURES).  A scene of
    4 x 4 albedo blocks under a left-to-right ramp, sampled with noise of standard deviation 0.3 a sample:
    counts from COUNTS, sums, means and moments as n samples would leave them (a single sample has m2_y = 0),
    about 20 % of the pixels uncovered, and about 3 % of the records with two or more samples given a
    negative or a NaN m2_y -- statistics no accumulation leaves, which must never enter a sum."""
    rng = np.random.default_rng(7000 * w + h)
    f = np.zeros((h, w), FEATURES)
    blocks = rng.choice(np.float32([0.25, 0.5, 0.75]), ((h + 3) // 4, (w + 3) // 4, 3))
    f["albedo"] = np.repeat(np.repeat(blocks, 4, axis=0), 4, axis=1)[:h, :w]
    nrm = np.concatenate([rng.normal(0, 0.15, (h, w, 2)), np.ones((h, w, 1))], axis=2)
    f["normal"] = (nrm / np.linalg.norm(nrm, axis=2, keepdims=True)).astype(np.float32)
    f["depth"] = rng.uniform(20, 22, (h, w)).astype(np.float32)
    cov = rng.integers(1, 9, (h, w)).astype(np.float32) / F(8)
    cov[rng.random((h, w)) < 0.2] = 0
    n = rng.choice(COUNTS, (h, w), p=[0.08, 0.17, 0.2, 0.25, 0.2, 0.1]).astype(np.float32)
    if w * h == 1:
        cov[:], n[:] = 1, 5
    f["coverage"] = cov
    truth = f["albedo"] * (F(0.5) + np.linspace(0, 1, w, dtype=np.float32))[None, :, None]
    sigma = F(0.3)
    with np.errstate(all="ignore"):
        mean = np.maximum(truth + (rng.normal(0, 1, (h, w, 3)) * sigma / np.sqrt(np.maximum(n, 1))[..., None]), 0)
    mean = mean.astype(np.float32)
    st = np.zeros((h, w), STATS)
    has = n >= 1
    st["n"] = n
    st["sum"] = np.where(has[..., None], mean * n[..., None], 0).astype(np.float32)
    st["mean_y"] = np.where(has, luminance(mean), 0).astype(np.float32)
    spread = (sigma * sigma * F(0.3)) * rng.chisquare(np.maximum(n - 1, 1)).astype(np.float32)
    st["m2_y"] = np.where(n >= 2, spread, 0).astype(np.float32)
    bad = (n >= 2) & (rng.random((h, w)) < 0.03)
    st["m2_y"][bad] = np.where(rng.random(int(bad.sum())) < 0.5, F(-0.5), F(np.nan))
    st["reserved"] = rng.integers(0, 2 ** 32, (h, w, 2), dtype=np.uint32)
    st.setflags(write=False)
    f.setflags(write=False)
    return st, f


def denoise_samples(stats, features, width, height, iterations=3, sigma_luminance=8.0, sigma_normal=0.5,
                    sigma_depth=0.1, sigma_albedo=0.25, epsilon=1e-4, encoding=GAMMA):
    """`stats`: width * height STATS records; `features`: as many records with the fields albedo, depth,
    normal, coverage (rt_pixel_features).  Returns (out (height, width, 4), variance (height, width))."""
    if encoding not in (LINEAR, GAMMA):
        raise ValueError("bad encoding")
    cells = filtered_cells(stats, features, width, height, iterations, sigma_luminance, sigma_normal, sigma_depth,
                           sigma_albedo, epsilon)
    return output(cells, stats, encoding)

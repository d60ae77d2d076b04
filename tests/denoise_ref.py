"""The feature-guided a-trous denoiser of rtEnqueueDenoise (include/rt_hip.h), restated in numpy float32
from its definition: every operation is one correctly rounded fp32 operation in the documented order,
so the device's bytes can be compared with this file's.  Nothing here knows how the device tiles.

    iteration i (step s = 2^i) reads the previous iteration's output, iteration 0 the image
    taps q = p + s (dx, dy), dy outer, dx inner, -2 .. 2; k = h[dy + 2] h[dx + 2], h = {1/16, 1/4, 3/8, 1/4, 1/16}
    a tap outside the image or with coverage_q == 0 adds nothing; a centre with coverage_p == 0 is copied
    dot3(a) = (a.x a.x + a.y a.y) + a.z a.z;  e(x) = m m, m = max(0, 1 - x)
    w = (((k e(x_c)) e(x_n)) e(x_z)) e(x_a), a term with sigma 0 left out
    rgb = sum_rgb / sum_w; the w slot is the image's
"""
import numpy as np

F = np.float32
H5 = [F(1) / F(16), F(1) / F(4), F(3) / F(8), F(1) / F(4), F(1) / F(16)]
MAX_ITERATIONS = 5
SIGMA_MIN, SIGMA_MAX = 2.0 ** -20, 2.0 ** 20


def sigma_ok(s) -> bool:
    s = F(s)
    return bool(s == 0 or (np.isfinite(s) and SIGMA_MIN <= s <= SIGMA_MAX))


def inv_sq(sigma):
    """1.0f / (sigma * sigma) in fp32; None for a disabled term (sigma == 0)."""
    s = F(sigma)
    if s == 0:
        return None
    return F(1) / (s * s)


def inv_color(sigma_color, i):
    """The colour term's constant of iteration i: the tolerance is ldexpf(sigma_color, -i)."""
    return inv_sq(np.ldexp(F(sigma_color), -i).astype(np.float32))


def shifted(a, ox, oy):
    """b[y, x] = a[y + oy, x + ox] where that lies inside the image (zeros elsewhere), and the mask of
    those pixels.  Any shift is allowed, also one larger than the image."""
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    valid = np.zeros((h, w), bool)
    y0, y1 = max(0, -oy), min(h, h - oy)
    x0, x1 = max(0, -ox), min(w, w - ox)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + oy:y1 + oy, x0 + ox:x1 + ox]
        valid[y0:y1, x0:x1] = True
    return out, valid


def dot3(a):
    return (a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]


def edge(x):
    m = np.maximum(F(0), F(1) - x)
    return m * m


def iteration(colour, albedo, depth, normal, coverage, step, inv_c, inv_n, inv_z, inv_a):
    """One iteration over (H, W, 4) colours and (H, W[, 3]) guides, all float32."""
    h, w = colour.shape[:2]
    covered = coverage != 0
    rz = F(1) / np.maximum(np.abs(depth), F(2.0 ** -64))
    sums = [np.zeros((h, w), np.float32) for _ in range(4)]  # w, r, g, b
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            ox, oy = step * dx, step * dy
            cq, inside = shifted(colour, ox, oy)
            ok = inside & (shifted(coverage, ox, oy)[0] != 0)
            wgt = np.full((h, w), H5[dy + 2] * H5[dx + 2], np.float32)
            if inv_c is not None:
                wgt = wgt * edge(dot3(colour[..., :3] - cq[..., :3]) * inv_c)
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
    out = colour.copy()
    for c in range(3):
        out[..., c] = np.where(covered, sums[1 + c] / sums[0], colour[..., c])
    return out


def denoise(image, features, width, height, iterations=3, sigma_color=4.0, sigma_normal=0.5, sigma_depth=0.1,
            sigma_albedo=0.25):
    """`image`: width * height slots {r, g, b, w} float32; `features`: as many records with the fields
    albedo, depth, normal, coverage (rt_pixel_features).  Returns the (height, width, 4) float32 result."""
    if not 1 <= iterations <= MAX_ITERATIONS:
        raise ValueError("iterations outside 1..5")
    for s in (sigma_color, sigma_normal, sigma_depth, sigma_albedo):
        if not sigma_ok(s):
            raise ValueError("bad sigma")
    colour = np.array(image, np.float32).reshape(height, width, 4)
    f = np.asarray(features).reshape(height, width)
    albedo = np.ascontiguousarray(f["albedo"], np.float32)
    normal = np.ascontiguousarray(f["normal"], np.float32)
    depth = np.ascontiguousarray(f["depth"], np.float32)
    coverage = np.ascontiguousarray(f["coverage"], np.float32)
    inv_n, inv_z, inv_a = inv_sq(sigma_normal), inv_sq(sigma_depth), inv_sq(sigma_albedo)
    with np.errstate(all="ignore"):
        for i in range(iterations):
            colour = iteration(colour, albedo, depth, normal, coverage, 1 << i, inv_color(sigma_color, i), inv_n,
                               inv_z, inv_a)
    return colour

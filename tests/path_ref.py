"""Reference for path tracing over arbitrary rays and seeds: a Python replay of the oracle's Render
(o_render, oracle/rt_oracle.c:314-344 = Render, kernel_bvh.cl:349-384).

Every Intersect goes through ray_query_ref.SceneWalker.walk -- the oracle's own box and triangle probes
-- with the raw direction the oracle hands to InitRay (the record's `dir` for the first segment, `wi`
afterwards), the first one with the record's [tmin, tmax].  pow, sin, cos, the RNG and max are the
oracle's exported probes (oracle_pow / oracle_sin / oracle_cos / oracle_rand / oracle_max); every other
operation is one np.float32 operation in rt_oracle.c's order (np.sqrt and `/` on np.float32 are
correctly rounded, as pm_sqrt and the C division are), the point light's attenuation its
double-precision quotient.

Render with LIGHT_BOUNCES = b is the first b rounds of Render with more: one replay therefore answers
every bounce count asked for (`bounces` may be a tuple).
"""
import ctypes
import math

import numpy as np

import oracle
from ray_query_ref import SceneWalker

F = np.float32
ZERO, ONE, TWO, FOUR, HALF = F(0.0), F(1.0), F(2.0), F(4.0), F(0.5)
TWO_PI, INV_PI = F(6.28318530718), F(0.31830988618)
MAX_DIST = 100000.0


# ---- float3 algebra of rt_oracle.c:47-79 on tuples of np.float32 --------------------------------
def v3(a):
    return (F(a[0]), F(a[1]), F(a[2]))


def vadd(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def vsub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def vmul(a, b):
    return (a[0] * b[0], a[1] * b[1], a[2] * b[2])


def vscale(a, s):
    return (a[0] * s, a[1] * s, a[2] * s)


def vneg(a):
    return (-a[0], -a[1], -a[2])


def vdot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def vcross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _rsqrt(d):
    return ONE / np.sqrt(d)


def vnormalize(v):
    if v[0] == 0.0 and v[1] == 0.0 and v[2] == 0.0:
        return v
    d = vdot(v, v)
    if d < F(2.0 ** -126):
        v = vscale(v, F(2.0 ** 86))
        d = vdot(v, v)
    elif np.isinf(d):
        v = vscale(v, F(2.0 ** -66))
        d = vdot(v, v)
        if np.isinf(d):
            v = tuple(np.copysign(ONE if np.isinf(c) else ZERO, c) for c in v)
            d = vdot(v, v)
    return vscale(v, _rsqrt(d))


class PathTracer:
    """o_render over one scene (its arrays are kept alive by the walker)."""

    def __init__(self, scene):
        self.walker = SceneWalker(scene)
        tris = self.walker.tris
        self._pos = [tris[v]["position"][:, :3].copy() for v in ("v1", "v2", "v3")]
        self._nrm = [tris[v]["normal"][:, :3].copy() for v in ("v1", "v2", "v3")]
        self._mtl = tris["mtlIndex"].tolist()
        mats = np.ascontiguousarray(scene.materials)
        self._mats = [(v3(m["diffuse"]), v3(m["specular"]), v3(m["emission"]), F(m["roughness"])) for m in mats]
        L = oracle.lib()
        self._pow, self._sin, self._cos, self._max, self._rand = \
            L.oracle_pow, L.oracle_sin, L.oracle_cos, L.oracle_max, L.oracle_rand

    # ---- probes as np.float32 -> np.float32 ------------------------------------------------------
    def pow(self, x, y):
        return F(self._pow(float(x), float(y)))

    def max(self, x, y):
        return F(self._max(float(x), float(y)))

    def rand(self, seed):
        return F(self._rand(ctypes.byref(seed)))

    def _frame(self, n):
        axis = (ZERO, ONE, ZERO) if np.abs(n[0]) > F(0.001) else (ONE, ZERO, ZERO)
        t = vnormalize(vcross(axis, n))
        return vcross(n, t), t

    def _lobe(self, n, phi, sinT, c):
        """normalize((s cos(phi)) sinT + (t sin(phi)) sinT + n c), rt_oracle.c:146-151, :254-259"""
        s, t = self._frame(n)
        a = vscale(vscale(s, F(self._cos(float(phi)))), sinT)
        b = vscale(vscale(t, F(self._sin(float(phi)))), sinT)
        return vnormalize(vadd(vadd(a, b), vscale(n, c)))

    def _sample_brdf(self, wo, n, mat, seed):
        """-> (f, wi, pdf), rt_oracle.c:263-287"""
        diffuse, specular, _, roughness = mat
        if self.rand(seed) > HALF:
            alpha = TWO / (roughness * roughness) - TWO
            phi = TWO_PI * self.rand(seed)
            self.rand(seed)  # `xi`, drawn and unused
            r = self.rand(seed)
            cosT = self.pow(r, ONE / (alpha + ONE))
            sinT = np.sqrt(self.max(ZERO, ONE - cosT * cosT))
            wh = self._lobe(n, phi, sinT, cosT)
            wi = vadd(vneg(wo), vscale(wh, TWO * vdot(wo, wh)))
            if vdot(wi, n) * vdot(wo, n) < F(0.000001):
                return (ZERO, ZERO, ZERO), wi, ZERO
            a2 = alpha * alpha
            q = cosT * cosT * (a2 - ONE) + ONE
            D = a2 * INV_PI / (q * q)
            pdf = D * cosT / (FOUR * self.max(vdot(wo, wh), ZERO))
            denom = FOUR * self.max(vdot(wi, n), ZERO) * self.max(vdot(wo, n), ZERO) + F(0.001)
            return vscale(specular, D / denom), wi, pdf
        phi = TWO_PI * self.rand(seed)
        s2 = self.rand(seed)
        wi = self._lobe(n, phi, np.sqrt(s2), np.sqrt(ONE - s2))
        return vscale(diffuse, INV_PI), wi, vdot(wi, n) * INV_PI

    def _light_pixel(self, org, d, t, normal, light_type):
        """rt_oracle.c:290-311"""
        light_pos, light_dir = v3((0.0, -10.0, 16.0)), v3((-0.5, 0.4, -0.1))
        intensity, attn = ONE, ONE
        if light_type <= 0:
            ndotl = self.max(vdot(normal, vneg(light_dir)), ZERO)
        else:
            X = vadd(org, vscale(d, t))
            L = vsub(light_pos, X)
            ndotl = self.max(vdot(normal, L), ZERO)
            if light_type == 1:
                intensity = F(16.0)
                eye = vsub(L, X)
                dist = np.sqrt(vdot(eye, eye))
                attn = F(1.0 / np.float64(F(0.8) * (dist * dist)))
        return attn * intensity * ndotl

    def _hit(self, org, d, prim, t):
        """The hit record o_ray_triangle forms at its last acceptance (rt_oracle.c:157-183): position and
        normal, from the barycentrics recomputed with its operations."""
        p1, p2, p3 = (v3(p[prim]) for p in self._pos)
        e1, e2 = vsub(p2, p1), vsub(p3, p1)
        pvec = vcross(d, e2)
        inv_det = ONE / vdot(e1, pvec)
        tvec = vsub(org, p1)
        u = vdot(tvec, pvec) * inv_det
        qvec = vcross(tvec, e1)
        v = vdot(d, qvec) * inv_det
        assert (vdot(e2, qvec) * inv_det).tobytes() == t.tobytes(), "the replay's t is the probe's"
        w = ONE - u - v
        n1, n2, n3 = (v3(n[prim]) for n in self._nrm)
        normal = vnormalize(vadd(vadd(vscale(n2, u), vscale(n3, v)), vscale(n1, w)))
        return vadd(org, vscale(d, t)), normal

    def trace(self, origin, direction, seed, bounces, light_type=0, skybox=1.0, tmin=-math.inf, tmax=MAX_DIST):
        """One record.  `bounces`: an int, or a tuple of ints.  -> (radiance 3 x np.float32 after
        max(., 0), first prim, rays, visits, tests, hits), or a dict of those per bounce count."""
        wanted = (bounces,) if isinstance(bounces, int) else tuple(bounces)
        out = {}
        seed = ctypes.c_uint32(int(seed) & 0xffffffff)
        org, raw = v3(origin), v3(direction)
        radiance, beta = (ZERO, ZERO, ZERO), (ONE, ONE, ONE)
        prim0, rays, visits, tests, hits = -1, 0, 0, 0, 0
        sky = HALF * F(skybox)
        lo, hi = tmin, tmax

        def snapshot(b):
            out[b] = (tuple(self.max(c, ZERO) for c in radiance), prim0, rays, visits, tests, hits)

        if 0 in wanted:
            snapshot(0)
        with np.errstate(all="ignore"):
            done = False
            for i in range(max(wanted)):
                if not done:
                    d = vnormalize(raw)  # o_init_ray: the ray the shading sees
                    prim, t, nv, nt = self.walker.walk([float(c) for c in org], [float(c) for c in raw], lo, hi)
                    lo, hi = -math.inf, MAX_DIST
                    rays, visits, tests = rays + 1, visits + nv, tests + nt
                    if i == 0:
                        prim0 = prim
                    if prim < 0:
                        radiance = vadd(radiance, vmul(beta, (sky, sky, sky)))
                        done = True
                    else:
                        hits += 1
                        pos, normal = self._hit(org, d, prim, F(t))
                        mat = self._mats[self._mtl[prim]]
                        radiance = vadd(radiance, vscale(vmul(beta, mat[2]), F(50.0)))
                        f, wi, pdf = self._sample_brdf(vneg(d), normal, mat, seed)
                        if pdf <= 0.0 or pdf != pdf:
                            done = True
                        else:
                            mul = vscale(f, vdot(wi, normal))
                            mul = (mul[0] / pdf, mul[1] / pdf, mul[2] / pdf)
                            beta = vmul(beta, mul)
                            lp = self._light_pixel(org, d, F(t), normal, light_type)
                            radiance = vadd(radiance, vmul(vmul((lp, lp, lp), mat[0]), beta))
                            org, raw = vadd(pos, vscale(wi, F(0.01))), wi
                if i + 1 in wanted:
                    snapshot(i + 1)
        return out[bounces] if isinstance(bounces, int) else out

    def trace_rays(self, rays, seeds, bounces, light_type=0, skybox=1.0):
        """N.RAY_DTYPE records and uint32 seeds -> per bounce count b of the tuple `bounces`:
        {"radiance": float32[n, 3], "prim": int32[n], "counts": (rays, visits, tests, hits) summed,
        "rounds": int32[n] Intersects of each path}."""
        n = len(rays)
        res = {b: {"radiance": np.zeros((n, 3), np.float32), "prim": np.full(n, -1, np.int32),
                   "rounds": np.zeros(n, np.int32), "counts": [0, 0, 0, 0]} for b in bounces}
        org, dr = rays["origin"], rays["dir"]
        tmin, tmax = rays["tmin"].tolist(), rays["tmax"].tolist()
        for i in range(n):
            per = self.trace(org[i], dr[i], seeds[i], tuple(bounces), light_type, skybox, tmin[i], tmax[i])
            for b, (rad, prim, *cnt) in per.items():
                r = res[b]
                r["radiance"][i], r["prim"][i], r["rounds"][i] = rad, prim, cnt[0]
                for k in range(4):
                    r["counts"][k] += cnt[k]
        for r in res.values():
            r["counts"] = tuple(r["counts"])
        return res


# ---- CreateRay in numpy (rt_oracle.c:347-359), for the camera's records and post-CreateRay seeds ---
def hash_u32(v):
    v = np.asarray(v, np.uint32).copy()
    v ^= v >> np.uint32(16)
    v *= np.uint32(0x7feb352d)
    v ^= v >> np.uint32(15)
    v *= np.uint32(0x846ca68b)
    v ^= v >> np.uint32(16)
    return v


def camera_paths(W, H, frame_count, camera=((0.0, -25.0, 8.5), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))):
    """-> (N.RAY_DTYPE records as rtEnqueueCameraRays writes them, uint32 seeds after CreateRay's draws)"""
    from clrt import _native as N
    gid = np.arange(W * H, dtype=np.uint32)
    with np.errstate(over="ignore"):
        s1 = hash_u32(gid + np.uint32((1103515245 * frame_count + 12345) & 0xffffffff))
        s2 = hash_u32(s1)
    r1 = s1.astype(np.float32) / F(4294967296.0)
    r2 = s2.astype(np.float32) / F(4294967296.0)
    invW, invH, aspect = ONE / F(W), ONE / F(H), F(W) / F(H)
    angle = F(oracle.lib().oracle_tan(float(HALF * (F(45.0) * F(3.1415) / F(180.0)))))
    x = (gid % np.uint32(W)).astype(np.float32) + r1 - HALF
    y = (gid // np.uint32(W)).astype(np.float32) + r2 - HALF
    x = (TWO * ((x + HALF) * invW) - ONE) * angle * aspect
    y = -(ONE - TWO * ((y + HALF) * invH)) * angle
    pos, front, up = (v3(c) for c in camera)
    side = vcross(front, up)
    rays = np.zeros(W * H, N.RAY_DTYPE)
    rays["origin"], rays["tmin"], rays["tmax"] = pos, -np.inf, MAX_DIST
    for i in range(W * H):
        rays["dir"][i] = vnormalize(vadd(vadd(vscale(side, x[i]), vscale(up, y[i])), front))
    return rays, s2


# ---- a pool of worker processes (started fresh: they never inherit a GPU context) --------------------
def _pool_job(args):
    tris, nodes, mats, rays, seeds, bounces, light_type, skybox = args
    import types
    oracle.build()
    scene = types.SimpleNamespace(triangles=tris, nodes=nodes, materials=mats)
    return PathTracer(scene).trace_rays(rays, seeds, bounces, light_type, skybox)


def trace_rays_pool(jobs, procs=16):
    """jobs: a list of (scene, rays, seeds, bounces tuple, light_type, skybox) -> their trace_rays results,
    each job split over the pool's processes (at most 16)."""
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    procs = max(1, min(16, procs))
    parts, where = [], []
    for j, (scene, rays, seeds, bounces, light_type, skybox) in enumerate(jobs):
        tris, nodes, mats = (np.ascontiguousarray(a) for a in (scene.triangles, scene.nodes, scene.materials))
        step = max(16, -(-len(rays) // procs))
        for lo in range(0, len(rays), step):
            parts.append((tris, nodes, mats, rays[lo:lo + step], np.asarray(seeds)[lo:lo + step], tuple(bounces),
                          light_type, skybox))
            where.append(j)
    with ProcessPoolExecutor(procs, mp_context=mp.get_context("spawn")) as ex:
        done = list(ex.map(_pool_job, parts))
    out = []
    for j, job in enumerate(jobs):
        mine = [d for d, w in zip(done, where) if w == j]
        merged = {}
        for b in job[3]:
            merged[b] = {"radiance": np.concatenate([m[b]["radiance"] for m in mine]),
                         "prim": np.concatenate([m[b]["prim"] for m in mine]),
                         "rounds": np.concatenate([m[b]["rounds"] for m in mine]),
                         "counts": tuple(sum(m[b]["counts"][k] for m in mine) for k in range(4))}
        out.append(merged)
    return out

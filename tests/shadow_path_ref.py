"""Reference for path tracing with shadow rays (rtKernelSetShadowRays): path_ref.PathTracer's replay of
Render with the one change rt_hip.h defines at kernel_bvh.cl:378.

Where Render adds lightPixel(...) * diffuse * beta and lightPixel's value lp is > 0, one shadow ray
{origin = isect.pos, tmin = 0.01, dir = L, tmax = T} is answered first by the walker's any-hit walk --
the oracle's own box and triangle probes, which run InitRay on the raw L -- and the term is added only
if that walk finds nothing.  L = -lightDirection and T = 100000 for the directional light; for the point
and the spot light L = lightPosition - X, the vector lightPixel forms, and T = sqrt(dot(L, L)).  With
!(lp > 0) the line executes as in Render and no ray is traced.  No RNG draw moves; beta, the next ray and
every later segment are Render's.  A shadow ray counts as one ray plus the visits and tests it walked.
"""
import math

import ctypes
import numpy as np

import oracle
from path_ref import (F, HALF, MAX_DIST, ONE, ZERO, PathTracer, v3, vadd, vdot, vmul, vneg, vnormalize, vscale,
                      vsub)

SHADOW_TMIN = 0.01
LIGHT_POS, LIGHT_DIR = (0.0, -10.0, 16.0), (-0.5, 0.4, -0.1)


class ShadowPathTracer(PathTracer):
    def shadow_ray(self, pos, light_type):
        """-> (L, T) of the shadow ray from the hit position `pos`"""
        if light_type <= 0:
            return vneg(v3(LIGHT_DIR)), F(MAX_DIST)
        L = vsub(v3(LIGHT_POS), pos)
        return L, np.sqrt(vdot(L, L))

    def trace(self, origin, direction, seed, bounces, light_type=0, skybox=1.0, tmin=-math.inf, tmax=MAX_DIST,
              shadows=True):
        """PathTracer.trace with two more values per result: the shadow rays traced and how many of them
        were occluded.  -> (radiance, first prim, rays, visits, tests, hits, shadow rays, occluded), or a
        dict of those per bounce count.  shadows=False is PathTracer.trace's arithmetic."""
        wanted = (bounces,) if isinstance(bounces, int) else tuple(bounces)
        out = {}
        seed = ctypes.c_uint32(int(seed) & 0xffffffff)
        org, raw = v3(origin), v3(direction)
        radiance, beta = (ZERO, ZERO, ZERO), (ONE, ONE, ONE)
        prim0, rays, visits, tests, hits, cast, occluded = -1, 0, 0, 0, 0, 0, 0
        sky = HALF * F(skybox)
        lo, hi = tmin, tmax

        def snapshot(b):
            out[b] = (tuple(self.max(c, ZERO) for c in radiance), prim0, rays, visits, tests, hits, cast, occluded)

        if 0 in wanted:
            snapshot(0)
        with np.errstate(all="ignore"):
            done = False
            for i in range(max(wanted)):
                if not done:
                    d = vnormalize(raw)
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
                            lit = True
                            if shadows and lp > 0.0:
                                L, T = self.shadow_ray(pos, light_type)
                                sp, _, nv, nt = self.walker.walk([float(c) for c in pos], [float(c) for c in L],
                                                                 SHADOW_TMIN, float(T), any_hit=True)
                                rays, visits, tests, cast = rays + 1, visits + nv, tests + nt, cast + 1
                                if sp >= 0:
                                    occluded += 1
                                    lit = False
                            if lit:
                                radiance = vadd(radiance, vmul(vmul((lp, lp, lp), mat[0]), beta))
                            org, raw = vadd(pos, vscale(wi, F(0.01))), wi
                if i + 1 in wanted:
                    snapshot(i + 1)
        return out[bounces] if isinstance(bounces, int) else out

    def trace_rays(self, rays, seeds, bounces, light_type=0, skybox=1.0, shadows=True):
        """path_ref's trace_rays with "shadow": (shadow rays, occluded) summed beside "counts", and
        "cast": int32[n] shadow rays of each path."""
        n = len(rays)
        res = {b: {"radiance": np.zeros((n, 3), np.float32), "prim": np.full(n, -1, np.int32),
                   "rounds": np.zeros(n, np.int32), "cast": np.zeros(n, np.int32), "counts": [0, 0, 0, 0],
                   "shadow": [0, 0]} for b in bounces}
        org, dr = rays["origin"], rays["dir"]
        tmin, tmax = rays["tmin"].tolist(), rays["tmax"].tolist()
        for i in range(n):
            per = self.trace(org[i], dr[i], seeds[i], tuple(bounces), light_type, skybox, tmin[i], tmax[i], shadows)
            for b, (rad, prim, *cnt) in per.items():
                r = res[b]
                r["radiance"][i], r["prim"][i], r["cast"][i] = rad, prim, cnt[4]
                r["rounds"][i] = cnt[0] - cnt[4]
                for k in range(4):
                    r["counts"][k] += cnt[k]
                r["shadow"][0] += cnt[4]
                r["shadow"][1] += cnt[5]
        for r in res.values():
            r["counts"], r["shadow"] = tuple(r["counts"]), tuple(r["shadow"])
        return res


# ---- a pool of worker processes (started fresh: they never inherit a GPU context) --------------------
def _pool_job(args):
    tris, nodes, mats, rays, seeds, bounces, light_type, skybox, shadows = args
    import types
    oracle.build()
    scene = types.SimpleNamespace(triangles=tris, nodes=nodes, materials=mats)
    return ShadowPathTracer(scene).trace_rays(rays, seeds, bounces, light_type, skybox, shadows)


def trace_rays_pool(jobs, procs=16):
    """jobs: a list of (scene, rays, seeds, bounces tuple, light_type, skybox[, shadows]) -> their
    trace_rays results, each job split over the pool's processes (at most 16)."""
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    procs = max(1, min(16, procs))
    parts, where = [], []
    for j, job in enumerate(jobs):
        scene, rays, seeds, bounces, light_type, skybox = job[:6]
        shadows = job[6] if len(job) > 6 else True
        tris, nodes, mats = (np.ascontiguousarray(a) for a in (scene.triangles, scene.nodes, scene.materials))
        step = max(16, -(-len(rays) // procs))
        for lo in range(0, len(rays), step):
            parts.append((tris, nodes, mats, rays[lo:lo + step], np.asarray(seeds)[lo:lo + step], tuple(bounces),
                          light_type, skybox, shadows))
            where.append(j)
    with ProcessPoolExecutor(procs, mp_context=mp.get_context("spawn")) as ex:
        done = list(ex.map(_pool_job, parts))
    out = []
    for j, job in enumerate(jobs):
        mine = [d for d, w in zip(done, where) if w == j]
        merged = {}
        for b in job[3]:
            merged[b] = {key: np.concatenate([m[b][key] for m in mine]) for key in ("radiance", "prim", "rounds", "cast")}
            merged[b]["counts"] = tuple(sum(m[b]["counts"][k] for m in mine) for k in range(4))
            merged[b]["shadow"] = tuple(sum(m[b]["shadow"][k] for m in mine) for k in range(2))
        out.append(merged)
    return out

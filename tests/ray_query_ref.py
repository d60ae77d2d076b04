"""Reference for ray queries over arbitrary rays: a Python replay of the oracle's stack walk
(o_intersect, oracle/rt_oracle.c:201-239 = Intersect, kernel_bvh.cl:171-219), driven entirely by
the oracle's probes oracle_ray_bounds and oracle_ray_triangle.  Both probes run InitRay on the raw
direction and take the current isect.t, so every float operation of a walk is the oracle's own.

The query's two generalisations sit on top: isect.t starts at the ray's tmax, and a probe
acceptance whose t is below tmin is discarded (isect.t keeps its value).  Any-hit stops at the
first kept acceptance.

The near child is chosen by the sign bit of the direction's axis component: 1 / -0 = -inf < 0, so
the sign bit is the reference's sign[] for every direction whose normalised components are not NaN.
(A zero component of a direction whose squared length under- or overflows in fp32 normalises to
0 * inf = NaN, for which the reference's sign is 0: such components must be +0.0 here.  NaN
direction components are not covered.)
"""
import ctypes
import math

import numpy as np

import oracle

NODE_BYTES, TRI_BYTES = 48, 256


class SceneWalker:
    """The walk over one scene's node and triangle arrays (kept alive here)."""

    def __init__(self, scene):
        self.nodes = np.ascontiguousarray(scene.nodes)
        self.tris = np.ascontiguousarray(scene.triangles)
        self._nbase = self.nodes.ctypes.data
        self._tbase = self.tris.ctypes.data
        # (offset, nPrimitives, axis) per node as Python ints
        self._meta = list(zip(self.nodes["offset"].tolist(), self.nodes["nPrimitives"].tolist(),
                              self.nodes["axis"].tolist()))
        L = oracle.lib()
        self._bounds, self._tri = L.oracle_ray_bounds, L.oracle_ray_triangle

    def walk(self, origin, direction, tmin=-math.inf, tmax=100000.0, any_hit=False):
        """-> (prim, t, visits, tests); t is a Python float holding the fp32 value (tmax on a miss)."""
        o = (ctypes.c_float * 3)(*origin)
        d = (ctypes.c_float * 3)(*direction)
        sign = [math.copysign(1.0, d[i]) < 0.0 for i in range(3)]
        t = ctypes.c_float(tmax).value
        t_out = ctypes.c_float()
        t_ref = ctypes.byref(t_out)
        prim, visits, tests = -1, 0, 0
        bounds, tri, meta, nbase, tbase = self._bounds, self._tri, self._meta, self._nbase, self._tbase
        stack, cur = [], 0
        while True:
            visits += 1
            offset, count, axis = meta[cur]
            if bounds(o, d, nbase + NODE_BYTES * cur, t):
                if count > 0:
                    for i in range(offset, offset + count):
                        tests += 1
                        if tri(o, d, tbase + TRI_BYTES * i, t, t_ref) and t_out.value >= tmin:
                            t, prim = t_out.value, i
                            if any_hit:
                                return prim, t, visits, tests
                    if not stack:
                        break
                    cur = stack.pop()
                elif sign[axis]:
                    stack.append(cur + 1)
                    cur = offset
                else:
                    stack.append(offset)
                    cur += 1
            else:
                if not stack:
                    break
                cur = stack.pop()
        return prim, t, visits, tests

    def walk_rays(self, rays, any_hit=False):
        """Walk an array of RAY_DTYPE records -> (prim int32[n], t float32[n], visits, tests) with
        the two counters summed over the rays."""
        n = len(rays)
        prim = np.empty(n, np.int32)
        t = np.empty(n, np.float32)
        visits = tests = 0
        org, dr = rays["origin"].tolist(), rays["dir"].tolist()
        tmin, tmax = rays["tmin"].tolist(), rays["tmax"].tolist()
        for i in range(n):
            prim[i], t[i], v, s = self.walk(org[i], dr[i], tmin[i], tmax[i], any_hit)
            visits += v
            tests += s
        return prim, t, visits, tests


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)

#!/usr/bin/env python3
"""Cost of moving geometry: the device path (rtEnqueueUpdateVertices + rtRefitBVH) against the only
path there was before it (rtEnqueueWriteBuffer of the whole triangle array and of host-refitted
nodes, which makes the next launch read both back, validate, pack and upload again).

For Cornell (scene in LDS) and the bunny proxy (octant records in HBM/L2), every triangle displaced:

  (a) HIP events around `--launches` back-to-back update + refit pairs (and around the updates and
      the refits alone; a refit = bounds climb + plane spread + triangle / shading repack), median of
      `--reps` repetitions;
  (b) wall clock from "the host has new positions" to "the next WxH one-frame render has finished",
      for the device path and for the old path, alternating in one process (the old path's host
      refit of the node array, clrt.scene.refit, is timed separately: a caller of the old path has
      to produce new bounds somehow);
  (c) a device-to-device copy of the triangle buffer in the same run: the rate that prices the
      refit's bytes.

  refit_bench.py [--width 640 --height 360 --launches 20 --reps 5 --math shipped] [--json FILE]
  rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python3 scripts/refit_bench.py --launches 3 --reps 1
      a short pass of the same launches for a kernel trace (the profiler slows the host: its numbers
      are kernel durations, not end-to-end times)
  refit_bench.py --summarize DIR/.../run_kernel_trace.csv
      per kernel and grid size (Cornell's grids are the small ones): update_vertices, refit_bounds,
      refit_spread and the repack (pack_tris, pack_shade), from that trace
"""
import argparse
import csv
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "mini-opencl-raytracer_amd"), os.path.join(REPO, "tests")]

MATHS = {"pinned": 0, "devicelib": 1, "shipped": 2}


class Events:
    """HIP events on the context's stream (the stream is handed out: launches are not coalesced)."""

    def __init__(self, stream):
        self.hip = ctypes.CDLL("libamdhip64.so")
        self.stream = ctypes.c_void_p(stream)
        self.a, self.b = ctypes.c_void_p(), ctypes.c_void_p()
        for e in (self.a, self.b):
            assert self.hip.hipEventCreate(ctypes.byref(e)) == 0

    def time_ms(self, fn, launches):
        assert self.hip.hipEventRecord(self.a, self.stream) == 0
        for _ in range(launches):
            fn()
        assert self.hip.hipEventRecord(self.b, self.stream) == 0
        assert self.hip.hipEventSynchronize(self.b) == 0
        ms = ctypes.c_float()
        assert self.hip.hipEventElapsedTime(ctypes.byref(ms), self.a, self.b) == 0
        return ms.value / launches


def med(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run(args):
    import numpy as np

    import clrt
    import clrt.proxy as P
    from clrt import _native as N
    from clrt import scene as S
    from hip_helpers import HipRenderer

    W, H = args.width, args.height
    out = {"width": W, "height": H, "math": args.math, "launches": args.launches, "reps": args.reps, "scenes": {}}
    for name, scene in (("cornell", clrt.scene.cornell()), ("bunny_proxy", P.bunny_proxy())):
        nt = scene.n_triangles
        r = HipRenderer(scene, W, H, math=MATHS[args.math])
        ctx, k = r.ctx, r.k
        rw = N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR
        for b in r.bufs[:2]:
            b.release()
        r.bufs[0] = ctx.create_buffer(rw, scene.triangles.nbytes, scene.triangles)
        r.bufs[1] = ctx.create_buffer(rw, scene.nodes.nbytes, scene.nodes)
        k.set_buffer(N.BUFFER_SCENE, r.bufs[0])
        k.set_buffer(N.BUFFER_NODE, r.bufs[1])
        tb, nb = r.bufs[0], r.bufs[1]
        # two displaced versions of the mesh, used in turn
        rng = np.random.default_rng(1)
        versions = []
        for _ in range(2):
            t = scene.triangles.copy()
            recs = np.zeros(nt, N.TRI_POINTS_DTYPE)
            for v, f in zip(("v1", "v2", "v3"), ("p1", "p2", "p3")):
                t[v]["position"][:, :3] += rng.normal(0.0, 0.05, (nt, 3)).astype(np.float32)
                recs[f][:, :3] = t[v]["position"][:, :3]
            t0 = time.perf_counter()
            nodes = S.refit(S.Scene(t, scene.nodes, scene.materials)).nodes
            versions.append((t, recs, nodes, (time.perf_counter() - t0) * 1e3))
        pos = ctx.create_buffer(N.MEM_READ_WRITE, nt * 48)
        spare = ctx.create_buffer(N.MEM_READ_WRITE, scene.triangles.nbytes)
        r.frame(1, light_bounces=9)
        ctx.Finish()

        # (b) geometry change -> next one-frame render finished, the two paths alternating
        def new_path(i):
            ctx.WriteBuffer(pos, versions[i % 2][1], blocking=False)
            ctx.UpdateVertices(tb, 0, nt, pos)
            ctx.RefitBVH(k)
            r.frame(1, light_bounces=9)
            ctx.Finish()

        def old_path(i):
            ctx.WriteBuffer(tb, versions[i % 2][0], blocking=False)
            ctx.WriteBuffer(nb, versions[i % 2][2], blocking=False)
            r.frame(1, light_bounces=9)
            ctx.Finish()

        def render_only(i):
            r.frame(1, light_bounces=9)
            ctx.Finish()

        wall = {"new_path": [], "old_path": [], "render_only": []}
        paths = {"new_path": new_path, "old_path": old_path, "render_only": render_only}
        for i in range(args.reps + 2):           # (the first two rounds warm up)
            for pname, fn in paths.items():
                t0 = time.perf_counter()
                fn(i)
                ms = (time.perf_counter() - t0) * 1e3
                if i >= 2:
                    wall[pname].append(ms)
        prepares = k.scene_prepares()

        # (a), (c) event timings of back-to-back launches
        ctx.WriteBuffer(pos, versions[0][1])
        ev = Events(ctx.stream())
        dst = spare.device_pointer()
        cases = {
            "update_vertices": lambda: ctx.UpdateVertices(tb, 0, nt, pos),
            "refit": lambda: ctx.RefitBVH(k),
            "update_refit_pair": lambda: (ctx.UpdateVertices(tb, 0, nt, pos), ctx.RefitBVH(k)),
            "copy_triangles": lambda: ctx.CopyToDevicePointer(tb, 0, scene.triangles.nbytes, dst),
        }
        res = {}
        ctx.RefitBVH(k)                          # (the old path ran last: this one prepares in full)
        for _ in range(args.reps):               # the cases alternate within a repetition
            for cname, fn in cases.items():
                for _ in range(3):
                    fn()
                ctx.Finish()
                res.setdefault(cname, []).append(ev.time_ms(fn, args.launches))
        ctx.Finish()
        s = {"triangles": nt, "nodes": int(len(scene.nodes)), "scene_in_lds": bool(k.scene_in_lds()),
             "prepares_after_wall_rounds": prepares, "prepares_at_end": k.scene_prepares(),
             "host_refit_ms": med([v[3] for v in versions])}
        for cname, v in res.items():
            s[cname + "_ms"] = med(v)
        for pname, v in wall.items():
            s["wall_" + pname + "_ms"] = med(v)
        # a copy reads and writes the buffer
        s["copy_gb_per_s"] = 2 * scene.triangles.nbytes / s["copy_triangles_ms"]["median"] / 1e6
        out["scenes"][name] = s
        print(json.dumps({name: s}), flush=True)
        for b in (pos, spare):
            b.release()
        r.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


def summarize(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    # the scenes run one after the other (Cornell, then the proxy): a kernel's launches split by scene
    # at the largest jump of its duration is not needed -- the grid size tells them apart
    groups = {}
    for r in rows:
        name = r["Kernel_Name"]
        for key in ("update_vertices", "refit_bounds", "refit_spread", "pack_tris", "pack_shade"):
            if key in name:
                grid = int(r["Grid_Size_X"]) if "Grid_Size_X" in r else int(r.get("Grid_Size", 0))
                groups.setdefault((key, grid), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print(f"{'kernel':<20}{'grid':>10}{'launches':>10}{'median_us':>11}{'min_us':>9}")
    for (key, grid), d in sorted(groups.items(), key=lambda kv: (kv[0][1], kv[0][0])):
        print(f"{key:<20}{grid:>10}{len(d):>10}{statistics.median(d):>11.1f}{min(d):>9.1f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=360)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--math", choices=list(MATHS), default="shipped")
    ap.add_argument("--json", help="write the results here as well")
    ap.add_argument("--summarize", metavar="CSV", help="summarise a rocprofv3 kernel trace of a short pass")
    args = ap.parse_args()
    if args.summarize:
        summarize(args.summarize)
    else:
        run(args)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Throughput of the batched ray queries (rtEnqueueIntersectRays) against the wavefront schedule's
bounce-0 extend launch -- the same traversal over the same rays without the 48 B per ray of ray
and hit traffic.

For Cornell (scene in LDS) and the bunny proxy (octant records in HBM/L2): the primary rays of a
WxH frame as rt_ray records (rtEnqueueCameraRays), then closest-hit and any-hit queries over them,
timed with HIP events around many back-to-back launches after a warm-up; a device-to-device copy of
the ray buffer in the same run gives the bandwidth that prices the 48 B per ray; one-bounce
wavefront renders of the same frame give the yardstick.

  rayquery_bench.py [--width W --height H --launches N --reps R --math shipped]
      event timings: Mrays/s per scene and mode, the copy bandwidth, the wavefront render per frame
      (extend + shade + accumulation: an upper bound of the extend launch)
  rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- python3 scripts/rayquery_bench.py --trace
      a short pass of the same launches for a kernel trace (the profiler slows the host: its
      numbers are kernel durations, not end-to-end rates)
  rayquery_bench.py --summarize DIR/.../run_kernel_trace.csv
      per scene: mean duration of query_rays (closest, any), wf_extend, wf_shade, camera_rays and
      the query / extend ratio, from that trace
"""
import argparse
import csv
import ctypes
import json
import os
import statistics
import sys

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


def run(args):
    import numpy as np

    import clrt
    import clrt.proxy as P
    from clrt import _native as N
    from hip_helpers import HipRenderer

    W, H = args.width, args.height
    n = W * H
    launches, reps = (3, 1) if args.trace else (args.launches, args.reps)
    out = {"width": W, "height": H, "rays": n, "math": args.math, "launches": launches, "reps": reps, "scenes": {}}
    for name, scene in (("cornell", clrt.scene.cornell()), ("bunny_proxy", P.bunny_proxy())):
        r = HipRenderer(scene, W, H, math=MATHS[args.math], sched=N.SCHED_WAVEFRONT)
        ctx, k = r.ctx, r.k
        rays = ctx.create_buffer(N.MEM_READ_WRITE, n * 32)
        rays2 = ctx.create_buffer(N.MEM_READ_WRITE, n * 32)
        hits = ctx.create_buffer(N.MEM_READ_WRITE, n * 16)
        r.frame(1, light_bounces=1)          # sets the slots; the wavefront render also warms up
        ctx.CameraRays(k, n, rays)
        ctx.Finish()
        ev = Events(ctx.stream())
        dst = rays2.device_pointer()
        cases = {
            "closest": lambda: ctx.IntersectRays(k, rays, hits, n, N.QUERY_CLOSEST),
            "any": lambda: ctx.IntersectRays(k, rays, hits, n, N.QUERY_ANY),
            "camera_rays": lambda: ctx.CameraRays(k, n, rays),
            "copy_rays": lambda: ctx.CopyToDevicePointer(rays, 0, n * 32, dst),
            "wavefront_frame": lambda: r.frame(1, light_bounces=1),
        }
        res = {}
        for _ in range(reps):                # the cases alternate within a repetition
            for cname, fn in cases.items():
                for _ in range(1 if args.trace else 3):
                    fn()
                ctx.Finish()
                res.setdefault(cname, []).append(ev.time_ms(fn, launches))
        ctx.Finish()
        hit = np.empty(n, N.RAY_HIT_DTYPE)
        ctx.IntersectRays(k, rays, hits, n, N.QUERY_CLOSEST)
        ctx.ReadBuffer(hits, hit, blocking=True)
        s = {"scene_in_lds": bool(k.scene_in_lds()), "hit_share": float((hit["prim"] >= 0).mean())}
        for cname, v in res.items():
            s[cname + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        for mode in ("closest", "any"):
            s[mode + "_mrays_per_s"] = n / s[mode + "_ms"]["median"] / 1e3
        # a copy reads and writes the buffer: bytes moved = 2 x 32 n
        s["copy_gb_per_s"] = 2 * 32 * n / s["copy_rays_ms"]["median"] / 1e6
        s["stream_48B_per_ray_ms"] = 48 * n / (s["copy_gb_per_s"] * 1e6)
        out["scenes"][name] = s
        print(json.dumps({name: s}), flush=True)
        for b in (rays, rays2, hits):
            b.release()
        r.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


def summarize(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    # grouped by kernel name: the LDS (Cornell) and HBM/L2 (proxy) variants of query_rays and
    # wf_extend, and the closest / any variants, are distinct template instances
    groups = {}
    for r in rows:
        name = r["Kernel_Name"]
        for key in ("query_rays", "wf_extend", "wf_shade", "camera_rays", "accum_frames"):
            if key in name:
                groups.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print(f"{'kernel':<110}{'launches':>9}{'mean_us':>10}{'min_us':>10}")
    for name, d in sorted(groups.items()):
        print(f"{name[:108]:<110}{len(d):>9}{statistics.mean(d):>10.1f}{min(d):>10.1f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--math", choices=list(MATHS), default="shipped")
    ap.add_argument("--trace", action="store_true", help="a short pass for a kernel trace")
    ap.add_argument("--json", help="write the results here as well")
    ap.add_argument("--summarize", metavar="CSV", help="summarise a rocprofv3 kernel trace of a --trace pass")
    args = ap.parse_args()
    if args.summarize:
        summarize(args.summarize)
    else:
        run(args)


if __name__ == "__main__":
    main()

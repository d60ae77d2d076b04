#!/usr/bin/env python3
"""Time of path tracing over caller rays (rtEnqueueTracePaths) against the render of the same paths
in the same build: one rtEnqueueKernel frame at FRAME_COUNT 0 with PERFRAME_DEFER 0, against a trace
(RT_TRACE_FRAME0) over that frame's rtEnqueueCameraPaths -- the same paths, plus 36 B in and 16 B out
per path that the render never streams.

For Cornell (scene in LDS) and the bunny proxy (records in HBM/L2), at WxH and 9 bounces: HIP events
around back-to-back launches after a warm-up, the cases alternating within each repetition, medians
reported; a device-to-device copy in the same run gives the rate that prices the 52 B per path; the
same number of incoherent random_rays-style paths (origins uniform in the scene's box, directions
standard normal); and the refill / shade threshold sweeps of the trace.

  trace_bench.py [--width W --height H --bounces B --launches N --reps R --math shipped] [--json FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "mini-opencl-raytracer_amd"), os.path.join(REPO, "tests")]
sys.path.insert(0, os.path.join(REPO, "scripts"))

from rayquery_bench import MATHS, Events  # noqa: E402

REFILLS = (8, 16, 32, 48, 64)
SHADES = (16, 32, 40, 48, 56, 64)


def median_of(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run(args):
    import numpy as np

    import clrt
    import clrt.proxy as P
    from clrt import _native as N
    from hip_helpers import HipRenderer

    W, H = args.width, args.height
    n = W * H
    launches, reps = args.launches, args.reps
    out = {"width": W, "height": H, "paths": n, "bounces": args.bounces, "math": args.math, "launches": launches,
           "reps": reps, "scenes": {}}
    for name, scene in (("cornell", clrt.scene.cornell()), ("bunny_proxy", P.bunny_proxy())):
        r = HipRenderer(scene, W, H, math=MATHS[args.math])
        ctx, k = r.ctx, r.k
        k.set_tuning("perframe_defer", 0)
        rays = ctx.create_buffer(N.MEM_READ_WRITE, n * 32)
        seeds = ctx.create_buffer(N.MEM_READ_WRITE, n * 4)
        res = ctx.create_buffer(N.MEM_READ_WRITE, n * 16)
        rays2 = ctx.create_buffer(N.MEM_READ_WRITE, n * 32)
        r.frame(0, light_bounces=args.bounces)   # sets the slots; warms the render up
        ctx.CameraPaths(k, n, rays, seeds)
        # incoherent paths: random_rays' recipe at this count
        rng = np.random.default_rng(7)
        pts = np.concatenate([scene.triangles[v]["position"][:, :3] for v in ("v1", "v2", "v3")])
        rnd = np.zeros(n, N.RAY_DTYPE)
        rnd["origin"] = rng.uniform(pts.min(axis=0), pts.max(axis=0), (n, 3)).astype(np.float32)
        rnd["dir"] = rng.standard_normal((n, 3)).astype(np.float32)
        rnd["tmin"], rnd["tmax"] = -np.inf, 100000.0
        rnd_rays = ctx.create_buffer(N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR, rnd.nbytes, rnd)
        ctx.Finish()
        ev = Events(ctx.stream())
        dst = rays2.device_pointer()
        cases = {
            "render_frame": lambda: r.frame(0, light_bounces=args.bounces),
            "trace_camera_paths": lambda: ctx.TracePaths(k, rays, res, n, seeds=seeds, encoding=N.TRACE_FRAME0),
            "trace_random_paths": lambda: ctx.TracePaths(k, rnd_rays, res, n, seed_base=1),
            "camera_paths": lambda: ctx.CameraPaths(k, n, rays, seeds),
            "copy_rays": lambda: ctx.CopyToDevicePointer(rays, 0, n * 32, dst),
        }
        t = {}
        for _ in range(reps):                # the cases alternate within a repetition
            for cname, fn in cases.items():
                for _ in range(2):
                    fn()
                ctx.Finish()
                t.setdefault(cname, []).append(ev.time_ms(fn, launches))
        # the trace's image is the render's
        img = np.zeros((n, 4), np.float32)
        got = np.empty(n, N.PATH_RESULT_DTYPE)
        r.frame(0, light_bounces=args.bounces)
        ctx.ReadBuffer(r.out, img, blocking=True)
        ctx.TracePaths(k, rays, res, n, seeds=seeds, encoding=N.TRACE_FRAME0)
        ctx.ReadBuffer(res, got, blocking=True)
        same = bool((np.ascontiguousarray(img[:, :3]).view(np.uint32) ==
                     np.ascontiguousarray(got["radiance"]).view(np.uint32)).all())
        s = {"scene_in_lds": bool(k.scene_in_lds()), "trace_equals_render_bits": same,
             "first_hit_share": float((got["prim"] >= 0).mean())}
        for cname, v in t.items():
            s[cname + "_ms"] = median_of(v)
        s["trace_over_render"] = s["trace_camera_paths_ms"]["median"] / s["render_frame_ms"]["median"]
        # a copy reads and writes the buffer: bytes moved = 2 x 32 n
        s["copy_gb_per_s"] = 2 * 32 * n / s["copy_rays_ms"]["median"] / 1e6
        s["stream_52B_per_path_ms"] = 52 * n / (s["copy_gb_per_s"] * 1e6)
        s["random_mpaths_per_s"] = n / s["trace_random_paths_ms"]["median"] / 1e3
        # threshold sweeps of the trace over the camera's paths, each value against the default in turn
        sweep = {"refill": {}, "shade": {}}
        for knob, values in (("trace_refill_min", REFILLS), ("trace_shade_min", SHADES)):
            default = k.get_tuning(knob)
            for _ in range(max(1, reps // 2)):
                for v in values:
                    k.set_tuning(knob, v)
                    cases["trace_camera_paths"]()
                    ctx.Finish()
                    sweep[knob.split("_")[1]].setdefault(v, []).append(ev.time_ms(cases["trace_camera_paths"], launches))
            k.set_tuning(knob, default)
        s["sweep_ms"] = {kn: {str(v): median_of(ts) for v, ts in d.items()} for kn, d in sweep.items()}
        out["scenes"][name] = s
        print(json.dumps({name: s}), flush=True)
        for b in (rays, seeds, res, rays2, rnd_rays):
            b.release()
        r.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--bounces", type=int, default=9)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--math", choices=list(MATHS), default="shipped")
    ap.add_argument("--json", help="write the results here as well")
    run(ap.parse_args())


if __name__ == "__main__":
    main()

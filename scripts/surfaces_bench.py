#!/usr/bin/env python3
"""Cost of the surface records (rtEnqueueHitSurfaces) and the feature buffers (rtEnqueueFrameFeatures).

For Cornell and the bunny proxy, on the primary hits of a WxH frame (rtEnqueueCameraRays +
rtEnqueueIntersectRays, misses included as the frame has them):

  * rtEnqueueHitSurfaces timed with HIP events around many back-to-back launches after a warm-up, median
    over the repetitions; a device-to-device copy of the ray buffer in the same run gives the bandwidth
    that prices the 112 B per record the kernel cannot avoid (32 + 16 in, 64 out); their ratio is what the
    gathers by `prim` (shading record, edges, uvs) cost on top.
  * rtEnqueueFrameFeatures over 8 frames, as ms per frame, beside the 8-frame fused render of the same
    frames (default bounces), which is the image the features accompany.  These two are timed on the host
    around a few calls and rtFinish: a fused render runs on the context's render and accumulation streams,
    which an event on the main stream does not cover.

  surfaces_bench.py [--width W --height H --launches N --reps R --math shipped --json OUT]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "mini-opencl-raytracer_amd"), os.path.join(REPO, "tests"),
                os.path.join(REPO, "scripts")]

from rayquery_bench import MATHS, Events  # noqa: E402

RECORD_BYTES = 32 + 16 + 64


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--bounces", type=int, default=9)
    ap.add_argument("--math", choices=list(MATHS), default="shipped")
    ap.add_argument("--json", help="write the results here as well")
    args = ap.parse_args()

    import numpy as np

    import clrt
    import clrt.proxy as P
    from clrt import _native as N
    from hip_helpers import HipRenderer

    W, H = args.width, args.height
    n = W * H
    out = {"width": W, "height": H, "records": n, "math": args.math, "launches": args.launches, "reps": args.reps,
           "frames": args.frames, "bounces": args.bounces, "scenes": {}}
    for name, scene in (("cornell", clrt.scene.cornell()), ("bunny_proxy", P.bunny_proxy())):
        r = HipRenderer(scene, W, H, math=MATHS[args.math])
        ctx, k = r.ctx, r.k
        rays = ctx.create_buffer(N.MEM_READ_WRITE, n * 32)
        rays2 = ctx.create_buffer(N.MEM_READ_WRITE, n * 32)
        hits = ctx.create_buffer(N.MEM_READ_WRITE, n * 16)
        surf = ctx.create_buffer(N.MEM_READ_WRITE, n * 64)
        feat = ctx.create_buffer(N.MEM_READ_WRITE, n * 32)
        r.frame(1, light_bounces=args.bounces, n_frames=args.frames)   # sets the slots and warms up
        ctx.CameraRays(k, n, rays)
        ctx.IntersectRays(k, rays, hits, n)
        ctx.Finish()
        ev = Events(ctx.stream())
        dst = rays2.device_pointer()

        def host_ms(fn, calls):
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            ctx.Finish()
            return (time.perf_counter() - t0) * 1e3 / calls

        def event_ms(fn):
            return ev.time_ms(fn, args.launches)

        cases = {
            "hit_surfaces": (lambda: ctx.HitSurfaces(k, rays, hits, surf, n), event_ms),
            "copy_rays": (lambda: ctx.CopyToDevicePointer(rays, 0, n * 32, dst), event_ms),
            "frame_features": (lambda: ctx.FrameFeatures(k, n, args.frames, feat), lambda fn: host_ms(fn, 4)),
            "fused_render": (lambda: r.frame(1, light_bounces=args.bounces, n_frames=args.frames),
                             lambda fn: host_ms(fn, 4)),
        }
        res = {}
        for _ in range(args.reps):               # the cases alternate within a repetition
            for cname, (fn, timer) in cases.items():
                fn()                             # warm-up
                ctx.Finish()
                res.setdefault(cname, []).append(timer(fn))
        ctx.Finish()
        hit = np.empty(n, N.RAY_HIT_DTYPE)
        ctx.ReadBuffer(hits, hit, blocking=True)
        s = {"hit_share": float((hit["prim"] >= 0).mean())}
        for cname, v in res.items():
            s[cname + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        # a copy reads and writes the buffer: bytes moved = 2 x 32 n
        s["copy_gb_per_s"] = 2 * 32 * n / s["copy_rays_ms"]["median"] / 1e6
        s["stream_112B_per_record_ms"] = RECORD_BYTES * n / (s["copy_gb_per_s"] * 1e6)
        s["surfaces_over_stream"] = s["hit_surfaces_ms"]["median"] / s["stream_112B_per_record_ms"]
        s["surfaces_gb_per_s"] = RECORD_BYTES * n / s["hit_surfaces_ms"]["median"] / 1e6
        s["features_ms_per_frame"] = s["frame_features_ms"]["median"] / args.frames
        s["render_ms_per_frame"] = s["fused_render_ms"]["median"] / args.frames
        s["features_over_render"] = s["features_ms_per_frame"] / s["render_ms_per_frame"]
        out["scenes"][name] = s
        print(json.dumps({name: s}), flush=True)
        for b in (rays, rays2, hits, surf, feat):
            b.release()
        r.close()
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

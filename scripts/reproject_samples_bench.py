#!/usr/bin/env python3
"""Cost of the sample-statistics reprojection (rtEnqueueReprojectSamples) at render size.

For Cornell and the bunny proxy: `--samples` adaptive samples per pixel at the reference camera become the history
statistics; the camera moves by (0.37, 0, 0.1) and Raytracer.reproject_samples() takes the features of both views.
The call that joins them is then timed into a buffer of its own with HIP events around `--launches` back-to-back
calls after a warm-up, median over the repetitions.

The yardstick is a device-to-device copy in the same run that moves the bytes an ideal pass moves: per pixel 32 B of
current features, one 32-B history statistics record and one 32-B history feature record read, 32 B written --
128 B, so a copy of 64 B per pixel (read and written) is timed beside it.  The two cases alternate within a
repetition.

  reproject_samples_bench.py [--width W --height H --launches N --reps R --samples S --math shipped --json OUT]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "mini-opencl-raytracer_amd"), os.path.join(REPO, "tests"),
                os.path.join(REPO, "scripts")]

from rayquery_bench import MATHS, Events  # noqa: E402

IDEAL_BYTES = 128         # per pixel: 32 + 32 + 32 read, 32 written


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--math", choices=list(MATHS), default="shipped")
    ap.add_argument("--json", help="write the results here as well")
    args = ap.parse_args()

    import clrt
    import clrt.proxy as P
    from clrt import _native as N

    W, H = args.width, args.height
    n = W * H
    out = {"width": W, "height": H, "pixels": n, "math": args.math, "launches": args.launches, "reps": args.reps,
           "samples": args.samples, "ideal_bytes_per_pixel": IDEAL_BYTES, "scenes": {}}
    for name, scene in (("cornell", clrt.scene.cornell()), ("bunny_proxy", P.bunny_proxy())):
        rt = clrt.Raytracer(W, H, read_back=False)
        rt.Init()
        rt.upload_scene(scene)
        rt.kernel.set_math_mode(MATHS[args.math])
        ctx, k = rt.ctx, rt.kernel
        rt.render_adaptive(args.samples, min_samples=args.samples, max_samples=args.samples)
        prev = rt.camera
        p = prev.position
        rt.camera = clrt.renderer.Camera(position=(p[0] + 0.37, p[1], p[2] + 0.1), front=prev.front, up=prev.up)
        rt.reproject_samples(prev)
        carried = rt.sample_stats()["n"] > 0
        b = rt._adaptive_buffers()
        hist, (feat_prev, feat_cur) = b["spare"], rt._reproject_feat     # (the statistics before the swap)
        res_buf = ctx.create_buffer(N.MEM_READ_WRITE, n * 32)
        a, c = (ctx.create_buffer(N.MEM_READ_WRITE, n * IDEAL_BYTES // 2) for _ in range(2))
        views = [(tuple(v.position), tuple(v.front), tuple(v.up)) for v in (rt.camera, prev)]
        ctx.Finish()
        ev = Events(ctx.stream())
        dst = c.device_pointer()
        cases = {
            "reproject": lambda: ctx.ReprojectSamples(k, hist, feat_prev, feat_cur, W, H, res_buf, views[0], views[1]),
            "copy_same_bytes": lambda: ctx.CopyToDevicePointer(a, 0, n * IDEAL_BYTES // 2, dst),
        }
        res = {}
        for _ in range(args.reps):               # the cases alternate within a repetition
            for cname, fn in cases.items():
                fn()                             # warm-up
                ctx.Finish()
                res.setdefault(cname, []).append(ev.time_ms(fn, args.launches))   # (per call)
        ctx.Finish()
        s = {"carried_share": float(carried.mean())}
        for cname, v in res.items():
            s[cname + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        tm, cm = s["reproject_ms"]["median"], s["copy_same_bytes_ms"]["median"]
        s["reproject_over_copy"] = tm / cm
        s["ideal_gb_per_s"] = IDEAL_BYTES * n / tm / 1e6
        s["copy_gb_per_s"] = IDEAL_BYTES * n / cm / 1e6
        out["scenes"][name] = s
        print(json.dumps({name: s}), flush=True)
        for buf in (res_buf, a, c):
            buf.release()
        rt.release()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fjson:
            json.dump(out, fjson, indent=1)


if __name__ == "__main__":
    main()

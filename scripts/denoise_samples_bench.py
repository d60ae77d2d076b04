#!/usr/bin/env python3
"""Cost of the variance-guided denoiser (rtEnqueueDenoiseSamples) at render size, beside the path it replaces.

For Cornell and the bunny proxy: WxH statistics of `--samples` uniform samples a pixel (camera paths, path trace,
rtEnqueueAccumulateSamples per sample frame) and the features of the same frames (rtEnqueueFrameFeatures), then,
for 1 .. 5 iterations, timed with HIP events around `--launches` back-to-back calls after a warm-up, median over
the repetitions, the cases alternating within a repetition:

  samples_N   rtEnqueueDenoiseSamples, gamma encoding, with the variance plane
  resolve_N   rtEnqueueResolveSamples + rtEnqueueDenoise at default parameters, the same iteration count
  copy_N      the yardstick: device-to-device copies in the same run of the bytes an ideal pass moves -- per pixel
              80 B for the first iteration (32 statistics + 32 features read, 16 written), 64 B for every later
              one (16 + 32 read, 16 written) and 8 B more for the last (the count read, the variance written).
              A copy of b bytes moves 2 b.

The time of step s alone is the difference between consecutive iteration counts (for the first, the whole
1-iteration call: it also holds the last iteration's encode).

  denoise_samples_bench.py [--width W --height H --launches N --reps R --samples S --math shipped --json OUT]
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

FIRST_BYTES, LATER_BYTES, LAST_EXTRA_BYTES = 80, 64, 8


def ideal_bytes(iterations):
    return FIRST_BYTES + LATER_BYTES * (iterations - 1) + LAST_EXTRA_BYTES


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--samples", type=int, default=4)
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
    out = {"width": W, "height": H, "pixels": n, "math": args.math, "launches": args.launches, "reps": args.reps,
           "samples": args.samples, "bounces": args.bounces,
           "ideal_bytes_per_pixel": {str(it): ideal_bytes(it) for it in range(1, 6)}, "scenes": {}}
    for name, scene in (("cornell", clrt.scene.cornell()), ("bunny_proxy", P.bunny_proxy())):
        r = HipRenderer(scene, W, H, math=MATHS[args.math])
        ctx, k = r.ctx, r.k
        mk = ctx.create_buffer
        r.frame(1, light_bounces=args.bounces)          # sets the slots
        stats = mk(N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR, n * 32, np.zeros(n, N.PIXEL_STATS_DTYPE))
        rays, seeds, res = mk(N.MEM_READ_WRITE, n * 32), mk(N.MEM_READ_WRITE, n * 4), mk(N.MEM_READ_WRITE, n * 16)
        feat, image, den, var = (mk(N.MEM_READ_WRITE, n * 32), mk(N.MEM_READ_WRITE, n * 16),
                                 mk(N.MEM_READ_WRITE, n * 16), mk(N.MEM_READ_WRITE, n * 4))
        copy_src, copy_dst = mk(N.MEM_READ_WRITE, n * 44), mk(N.MEM_READ_WRITE, n * 44)
        for frame in range(1, args.samples + 1):
            k.set_uint(N.FRAME_COUNT, frame)
            ctx.CameraPaths(k, n, rays, seeds)
            ctx.TracePaths(k, rays, res, n, seeds=seeds)
            ctx.AccumulateSamples(k, None, res, n, n, stats)
        k.set_uint(N.FRAME_COUNT, 1)
        ctx.FrameFeatures(k, n, args.samples, feat)
        ctx.Finish()
        ev = Events(ctx.stream())
        dst = copy_dst.device_pointer()

        def copies(it):
            ctx.CopyToDevicePointer(copy_src, 0, n * (FIRST_BYTES + LAST_EXTRA_BYTES) // 2, dst)
            for _ in range(it - 1):
                ctx.CopyToDevicePointer(copy_src, 0, n * LATER_BYTES // 2, dst)

        def resolve_denoise(it):
            ctx.ResolveSamples(k, stats, W, H, image)
            ctx.Denoise(k, image, feat, W, H, den, it)

        cases = {}
        for it in range(1, 6):
            cases[f"samples_{it}"] = lambda it=it: ctx.DenoiseSamples(k, stats, feat, W, H, den, var, it)
            cases[f"resolve_{it}"] = lambda it=it: resolve_denoise(it)
            cases[f"copy_{it}"] = lambda it=it: copies(it)
        t = {}
        for _ in range(args.reps):               # the cases alternate within a repetition
            for cname, fn in cases.items():
                fn()                             # warm-up
                ctx.Finish()
                t.setdefault(cname, []).append(ev.time_ms(fn, args.launches))
        ctx.Finish()
        f = np.empty(n, N.PIXEL_FEATURES_DTYPE)
        ctx.ReadBuffer(feat, f, blocking=True)
        s = {"covered_share": float((f["coverage"] != 0).mean()), "iterations": {}}
        prev = prev_r = 0.0
        for it in range(1, 6):
            d, rd, c = t[f"samples_{it}"], t[f"resolve_{it}"], t[f"copy_{it}"]
            dm, rm, cm = statistics.median(d), statistics.median(rd), statistics.median(c)
            s["iterations"][str(it)] = {
                "samples_ms": {"median": dm, "min": min(d), "max": max(d)},
                "resolve_denoise_ms": {"median": rm, "min": min(rd), "max": max(rd)},
                "copy_same_bytes_ms": {"median": cm, "min": min(c), "max": max(c)},
                "samples_over_copy": dm / cm,
                "samples_over_resolve_denoise": dm / rm,
                "ideal_gb_per_s": ideal_bytes(it) * n / dm / 1e6,
                "copy_gb_per_s": ideal_bytes(it) * n / cm / 1e6,
                "last_step": 1 << (it - 1),
                "last_step_ms": dm - prev,
                "resolve_denoise_last_step_ms": rm - prev_r,
            }
            prev, prev_r = dm, rm
        out["scenes"][name] = s
        print(json.dumps({name: s}), flush=True)
        for b in (stats, rays, seeds, res, feat, image, den, var, copy_src, copy_dst):
            b.release()
        r.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fjson:
            json.dump(out, fjson, indent=1)


if __name__ == "__main__":
    main()

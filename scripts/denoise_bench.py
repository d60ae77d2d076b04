#!/usr/bin/env python3
"""Cost of the denoiser (rtEnqueueDenoise) at render size.

For Cornell and the bunny proxy: a WxH image of `--frames` fused frames and the features of the same
frames (rtEnqueueFrameFeatures), then rtEnqueueDenoise for 1 .. 5 iterations, timed with HIP events around
`--launches` back-to-back calls after a warm-up, median over the repetitions.

The yardstick is a device-to-device copy in the same run that moves the bytes an ideal pass moves: per
pixel and iteration 48 B read (16 colour + 32 features) and 16 B written, 64 B -- a copy of the 32-B feature
buffer reads and writes exactly that, so `iterations` such copies are timed beside each case.  The cases
alternate within a repetition.  Beside each step stands what its tiles request: a tile of 64 columns x R rows
stages (64 + 4 s) x (R + 4) cells of 48 B (the plan's shape, rt_denoise_plan.hpp), so the reads it issues are
that many times the ideal 48 B per pixel; how much of the overlap the caches absorb is what the time shows.
The time of step s alone is the difference between consecutive iteration counts.

  denoise_bench.py [--width W --height H --launches N --reps R --frames F --math shipped --json OUT]
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

IDEAL_BYTES = 64          # per pixel and iteration: 48 read, 16 written
TILE_W = 64


ROWS = {"near": 8, "far": 4}   # the plan's defaults (--rows / --rows-far: a variant build's)


def tile_rows(step):
    return ROWS["far"] if step >= 16 else ROWS["near"]


def staged_over_ideal(step):
    """Cells a tile stages over the pixels it filters."""
    r = tile_rows(step)
    return (TILE_W + 4 * step) * (r + 4) / (TILE_W * r)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--bounces", type=int, default=9)
    ap.add_argument("--math", choices=list(MATHS), default="shipped")
    ap.add_argument("--rows", type=int, default=8, help="tile rows at steps 1 .. 8 of the library under test")
    ap.add_argument("--rows-far", type=int, default=4, help="... and at step 16")
    ap.add_argument("--json", help="write the results here as well")
    args = ap.parse_args()
    ROWS.update(near=args.rows, far=args.rows_far)

    import numpy as np

    import clrt
    import clrt.proxy as P
    from clrt import _native as N
    from hip_helpers import HipRenderer

    W, H = args.width, args.height
    n = W * H
    out = {"width": W, "height": H, "pixels": n, "math": args.math, "launches": args.launches, "reps": args.reps,
           "frames": args.frames, "bounces": args.bounces, "ideal_bytes_per_pixel_iteration": IDEAL_BYTES,
           "staged_over_ideal_reads": {str(1 << i): staged_over_ideal(1 << i) for i in range(5)}, "scenes": {}}
    for name, scene in (("cornell", clrt.scene.cornell()), ("bunny_proxy", P.bunny_proxy())):
        r = HipRenderer(scene, W, H, math=MATHS[args.math])
        ctx, k = r.ctx, r.k
        feat = ctx.create_buffer(N.MEM_READ_WRITE, n * 32)
        feat2 = ctx.create_buffer(N.MEM_READ_WRITE, n * 32)
        den = ctx.create_buffer(N.MEM_READ_WRITE, n * 16)
        r.frame(1, light_bounces=args.bounces, n_frames=args.frames)
        ctx.FrameFeatures(k, n, args.frames, feat)
        ctx.Finish()
        ev = Events(ctx.stream())
        dst = feat2.device_pointer()

        def copies(count):
            for _ in range(count):
                ctx.CopyToDevicePointer(feat, 0, n * 32, dst)

        cases = {}
        for it in range(1, 6):
            cases[f"denoise_{it}"] = lambda it=it: ctx.Denoise(k, r.out, feat, W, H, den, it)
            cases[f"copy_{it}"] = lambda it=it: copies(it)
        res = {}
        for _ in range(args.reps):               # the cases alternate within a repetition
            for cname, fn in cases.items():
                fn()                             # warm-up
                ctx.Finish()
                res.setdefault(cname, []).append(ev.time_ms(fn, args.launches))
        ctx.Finish()
        f = np.empty(n, N.PIXEL_FEATURES_DTYPE)
        ctx.ReadBuffer(feat, f, blocking=True)
        s = {"covered_share": float((f["coverage"] != 0).mean()), "iterations": {}}
        prev = 0.0
        for it in range(1, 6):
            d, c = res[f"denoise_{it}"], res[f"copy_{it}"]
            dm, cm = statistics.median(d), statistics.median(c)
            s["iterations"][str(it)] = {
                "denoise_ms": {"median": dm, "min": min(d), "max": max(d)},
                "copy_same_bytes_ms": {"median": cm, "min": min(c), "max": max(c)},
                "denoise_over_copy": dm / cm,
                "ideal_gb_per_s": IDEAL_BYTES * n * it / dm / 1e6,
                "copy_gb_per_s": IDEAL_BYTES * n * it / cm / 1e6,
                "last_step": 1 << (it - 1),
                "last_step_ms": dm - prev,
                "last_step_staged_over_ideal_reads": staged_over_ideal(1 << (it - 1)),
            }
            prev = dm
        out["scenes"][name] = s
        print(json.dumps({name: s}), flush=True)
        for b in (feat, feat2, den):
            b.release()
        r.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fjson:
            json.dump(out, fjson, indent=1)


if __name__ == "__main__":
    main()

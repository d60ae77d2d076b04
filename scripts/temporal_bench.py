#!/usr/bin/env python3
"""Cost of temporal reprojection (rtEnqueueTemporalAccumulate) at render size.

For Cornell and the bunny proxy: `--frames` fused frames and their features at the reference camera become
the history (a first call without history gives it its sample counts); the camera moves by (0.37, 0, 0.1),
the same number of frames and their features are taken there, and the call that joins the two is timed with
HIP events around `--launches` back-to-back calls after a warm-up, median over the repetitions.

The yardstick is a device-to-device copy in the same run that moves the bytes an ideal pass moves: per pixel
48 B read at the new camera (16 colour + 32 features), 48 B of history read once, 16 B written -- 112 B, so a
copy of 56 B per pixel (read and written) is timed beside it.  The two cases alternate within a repetition.
Also timed: the call without history (a 16-B read and a 16-B write per pixel).

  temporal_bench.py [--width W --height H --launches N --reps R --frames F --math shipped --json OUT]
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

IDEAL_BYTES = 112         # per pixel: 48 + 48 read, 16 written
PREV = ((0.0, -25.0, 8.5), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
CUR = ((0.37, -25.0, 8.6), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--launches", type=int, default=10)
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
    out = {"width": W, "height": H, "pixels": n, "math": args.math, "launches": args.launches, "reps": args.reps,
           "frames": args.frames, "bounces": args.bounces, "ideal_bytes_per_pixel": IDEAL_BYTES, "scenes": {}}
    for name, scene in (("cornell", clrt.scene.cornell()), ("bunny_proxy", P.bunny_proxy())):
        r = HipRenderer(scene, W, H, math=MATHS[args.math])
        ctx, k = r.ctx, r.k
        feat_prev, feat_cur = (ctx.create_buffer(N.MEM_READ_WRITE, n * 32) for _ in range(2))
        hist, res_buf = (ctx.create_buffer(N.MEM_READ_WRITE, n * 16) for _ in range(2))
        a, b = (ctx.create_buffer(N.MEM_READ_WRITE, n * IDEAL_BYTES // 2) for _ in range(2))
        nf = float(args.frames)
        # the history: the image and the features at the previous camera
        r.frame(1, light_bounces=args.bounces, n_frames=args.frames, camera=PREV)
        k.set_uint(N.FRAME_COUNT, 1)
        ctx.FrameFeatures(k, n, args.frames, feat_prev)
        ctx.TemporalAccumulate(k, r.out, feat_prev, None, None, W, H, hist, PREV, PREV, nf)
        # the current frames after the move
        r.frame(1, light_bounces=args.bounces, n_frames=args.frames, camera=CUR)
        k.set_uint(N.FRAME_COUNT, 1)
        ctx.FrameFeatures(k, n, args.frames, feat_cur)
        ctx.Finish()
        ev = Events(ctx.stream())
        dst = b.device_pointer()
        cases = {
            "temporal": lambda: ctx.TemporalAccumulate(k, r.out, feat_cur, hist, feat_prev, W, H, res_buf, CUR, PREV, nf),
            "copy_same_bytes": lambda: ctx.CopyToDevicePointer(a, 0, n * IDEAL_BYTES // 2, dst),
            "temporal_no_history": lambda: ctx.TemporalAccumulate(k, r.out, feat_cur, None, None, W, H, res_buf, CUR, CUR, nf),
        }
        res = {}
        for _ in range(args.reps):               # the cases alternate within a repetition
            for cname, fn in cases.items():
                fn()                             # warm-up
                ctx.Finish()
                res.setdefault(cname, []).append(ev.time_ms(fn, args.launches))   # (per call)
        cases["temporal"]()
        ctx.Finish()
        o = np.empty((n, 4), np.float32)
        f = np.empty(n, N.PIXEL_FEATURES_DTYPE)
        ctx.ReadBuffer(res_buf, o)
        ctx.ReadBuffer(feat_cur, f, blocking=True)
        covered = f["coverage"] > 0
        s = {"covered_share": float(covered.mean()),
             "history_share_of_covered": float((o[:, 3][covered] > nf).mean()) if covered.any() else None}
        for cname, v in res.items():
            s[cname + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        tm, cm = s["temporal_ms"]["median"], s["copy_same_bytes_ms"]["median"]
        s["temporal_over_copy"] = tm / cm
        s["ideal_gb_per_s"] = IDEAL_BYTES * n / tm / 1e6
        s["copy_gb_per_s"] = IDEAL_BYTES * n / cm / 1e6
        out["scenes"][name] = s
        print(json.dumps({name: s}), flush=True)
        for buf in (feat_prev, feat_cur, hist, res_buf, a, b):
            buf.release()
        r.close()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fjson:
            json.dump(out, fjson, indent=1)


if __name__ == "__main__":
    main()

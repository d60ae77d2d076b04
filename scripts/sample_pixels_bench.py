#!/usr/bin/env python3
"""rtEnqueueSamplePixels measured: DESIGN 5.11's break-even table and its equal-time row again, with
the fused round beside the composed one, both from the same build.

  breakeven  Cornell and the bunny proxy, 9 bounces: with a fraction 1.0, 0.5, 0.25, 0.1 of the pixels selected
             (scattered single pixels and whole rows), one composed round -- select, the blocking read of its
             result, rtEnqueueCameraPathsFor, rtEnqueueTracePaths, rtEnqueueAccumulateSamples; adaptive_bench.py's
             round unchanged -- against one fused round -- select, rtEnqueueSamplePixels with the select's result
             as its device count, no read -- beside one frame of a fused render.  HIP events around back-to-back
             rounds after a warm-up, the two rounds alternating within each repetition; medians, and every
             repetition's pair.
  quality    Cornell: 5.11's run (min_samples 4, max_samples 32, threshold 0.05, radius 1, 32 rounds) composed and
             fused (sync_every 8 and 32), the seconds of each with the final resolve and read-back, the number of
             fused-render frames that fit into the fused run's time, and the RMS errors against a 256-sample
             reference of the adaptive image and of a uniform image of that many samples per pixel.

Without --part every part runs as a fresh child process under its own time limit, one after the other, and the
first failure ends the run (the shell's `timeout ... && timeout ...`); a parent never touches the GPU.

  sample_pixels_bench.py [--width W --height H --bounces B --launches N --reps R --out DIR] [--part NAME]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "mini-opencl-raytracer_amd"), os.path.join(REPO, "tests")]
sys.path.insert(0, os.path.join(REPO, "scripts"))

PARTS = {"breakeven": 420, "quality": 300}      # seconds allowed per part
FRACTIONS = (1.0, 0.5, 0.25, 0.1)


def breakeven(args):
    import numpy as np

    import clrt
    import clrt.proxy as P
    from adaptive_bench import masks, median_of, stats_selecting
    from clrt import _native as N
    from hip_helpers import HipRenderer
    from rayquery_bench import MATHS, Events

    W, H = args.width, args.height
    px = W * H
    out = {}
    for name, scene in (("cornell", clrt.scene.cornell()), ("bunny_proxy", P.bunny_proxy())):
        r = HipRenderer(scene, W, H, math=MATHS[args.math])
        ctx, k = r.ctx, r.k
        mk = ctx.create_buffer
        ids, result = mk(N.MEM_READ_WRITE, px * 4), mk(N.MEM_READ_WRITE, 16)
        rays, seeds, res = mk(N.MEM_READ_WRITE, px * 32), mk(N.MEM_READ_WRITE, px * 4), mk(N.MEM_READ_WRITE, px * 16)
        r.frame(1, light_bounces=args.bounces, n_frames=8)     # sets the slots; warms the render up
        ctx.Finish()
        ev = Events(ctx.stream())
        got = np.zeros(1, N.SELECT_RESULT_DTYPE)
        s = {"scene_in_lds": bool(k.scene_in_lds()), "rounds": {}}
        frame = [1]

        def render():
            r.frame(frame[0], light_bounces=args.bounces, n_frames=8)
            frame[0] += 8

        walls = []
        for _ in range(args.reps):       # (wall clock, as bench.py and adaptive_bench.py time the fused render)
            render()
            ctx.Finish()
            t0 = time.perf_counter()
            for _ in range(args.launches):
                render()
            ctx.Finish()
            walls.append((time.perf_counter() - t0) * 1e3 / (8 * args.launches))
        s["render_frame_ms"] = statistics.median(walls)
        sel = dict(min_samples=1000, max_samples=1000, radius=1)
        for fraction in FRACTIONS:
            for shape, mask in masks(np, W, H, fraction).items():
                host = stats_selecting(np, N, px, mask)
                st_c = mk(N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR, px * 32, host)
                st_f = mk(N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR, px * 32, host)
                n = [0]

                def composed():
                    ctx.SelectPixels(k, st_c, W, H, ids, result, **sel)
                    ctx.ReadBuffer(result, got, blocking=True)
                    n[0] = int(got["selected"][0])
                    k.set_uint(N.FRAME_COUNT, frame[0])
                    frame[0] += 1
                    ctx.CameraPathsFor(k, ids, n[0], rays, seeds)
                    ctx.TracePaths(k, rays, res, n[0], seeds=seeds)
                    ctx.AccumulateSamples(k, ids, res, n[0], px, st_c)

                def fused():
                    ctx.SelectPixels(k, st_f, W, H, ids, result, **sel)
                    k.set_uint(N.FRAME_COUNT, frame[0])
                    frame[0] += 1
                    ctx.SamplePixels(k, ids, px, px, st_f, count=result)

                t = {"composed": [], "fused": []}
                for _ in range(args.reps):           # the two rounds alternate within a repetition
                    for case, fn in (("composed", composed), ("fused", fused)):
                        for _ in range(2):
                            fn()
                        ctx.Finish()
                        t[case].append(ev.time_ms(fn, args.launches))
                assert n[0] == int(mask.sum())
                # both statistics took the same rounds: the same counts
                a, b = np.empty(px, N.PIXEL_STATS_DTYPE), np.empty(px, N.PIXEL_STATS_DTYPE)
                ctx.ReadBuffer(st_c, a, blocking=True)
                ctx.ReadBuffer(st_f, b, blocking=True)
                assert a["n"].tobytes() == b["n"].tobytes()
                mc, mf = statistics.median(t["composed"]), statistics.median(t["fused"])
                s["rounds"][f"{fraction}_{shape}"] = {
                    "selected": n[0], "composed_ms": median_of(t["composed"]), "fused_ms": median_of(t["fused"]),
                    "pairs_ms": list(zip(t["composed"], t["fused"])),
                    "fused_faster_in_every_pair": all(f < c for c, f in zip(t["composed"], t["fused"])),
                    "saved_ms": mc - mf, "fused_over_composed": mf / mc,
                    "composed_over_render_frame": mc / s["render_frame_ms"],
                    "fused_over_render_frame": mf / s["render_frame_ms"]}
                st_c.release()
                st_f.release()
        out[name] = s
        print(json.dumps({"breakeven": {name: s}}), flush=True)
        r.close()
    return out


def quality(args):
    import numpy as np

    import clrt
    from rayquery_bench import MATHS

    W, H = args.width, args.height
    px = W * H
    rt = clrt.Raytracer(W, H)
    rt.Init()
    rt.upload_scene(clrt.scene.cornell())
    rt.kernel.set_math_mode(MATHS[args.math])
    rt.light_bounces = args.bounces
    rt.read_back = False
    params = dict(threshold=0.05, floor_y=0.01, min_samples=4, max_samples=32, radius=1)

    def rms(a, b):
        d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
        return float(np.sqrt((d * d).mean()))

    def run(first_frame, rounds, **kw):
        rt.reset_samples()
        rt._sample_frame = first_frame
        t0 = time.perf_counter()
        img, info = rt.render_adaptive(rounds, **kw)
        return img, info, time.perf_counter() - t0

    run(1, 2, min_samples=2, max_samples=2)
    run(1, 2, min_samples=2, max_samples=2, fused=True)                  # warm-up of both paths
    ref, _, _ = run(100001, args.reference, min_samples=args.reference, max_samples=args.reference, fused=True,
                    sync_every=64)                                     # sample frames no test image takes
    rows = {}
    for label, kw in (("composed", dict()), ("fused_sync8", dict(fused=True, sync_every=8)),
                      ("fused_sync32", dict(fused=True, sync_every=32))):
        secs, img, info = [], None, None
        for _ in range(args.reps):
            img, info, s = run(1, 32, **params, **kw)
            secs.append(s)
        rows[label] = {"seconds": statistics.median(secs), "seconds_all": secs, "rms": rms(img, ref), **info}
    assert rows["composed"]["paths"] == rows["fused_sync8"]["paths"] == rows["fused_sync32"]["paths"]
    # the fused render's frame, wall clock over back-to-back 8-frame launches
    def render(frames):
        rt.frame_count = 1
        rt.ctx.Finish()
        t0 = time.perf_counter()
        for _ in range(frames // 8):
            rt.set_uniforms()
            rt.ctx.ExecuteKernelFrames(rt.kernel, px, 8)
            rt.frame_count += 8
        rt.ctx.Finish()
        return (time.perf_counter() - t0) / frames

    render(8)
    frame_s = statistics.median(render(80) for _ in range(args.reps))
    out = {"pixels": px, "reference_samples": args.reference, "adaptive": rows, "render_frame_ms": frame_s * 1e3}
    for label in ("composed", "fused_sync8", "fused_sync32"):
        fit = max(1, int(rows[label]["seconds"] / frame_s))
        out[f"uniform_frames_in_{label}_time"] = fit
    fit = out["uniform_frames_in_fused_sync32_time"]
    u, u_info, _ = run(1, fit, min_samples=fit, max_samples=fit, fused=True, sync_every=64)
    u16, _, _ = run(1, 16, min_samples=16, max_samples=16, fused=True, sync_every=64)
    out["uniform_at_equal_time"] = {"samples": fit, "paths": u_info["paths"], "rms": rms(u, ref)}
    out["uniform16"] = {"rms": rms(u16, ref), "rms_by_sqrt_law_at_equal_time": rms(u16, ref) * (16 / fit) ** 0.5}
    print(json.dumps({"quality": out}), flush=True)
    rt.release()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--bounces", type=int, default=9)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reference", type=int, default=256, help="samples per pixel of the quality reference")
    ap.add_argument("--math", default="shipped")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "sample_pixels"), help="directory of the raw output")
    ap.add_argument("--part", choices=list(PARTS), help="run this part in this process")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.part:
        res = {"width": args.width, "height": args.height, "bounces": args.bounces, "math": args.math,
               "launches": args.launches, "reps": args.reps, args.part: {"breakeven": breakeven, "quality": quality}[args.part](args)}
        with open(os.path.join(args.out, f"sample_pixels_bench_{args.part}.json"), "w") as f:
            json.dump(res, f, indent=1)
        return 0
    for part, limit in PARTS.items():
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part] + [a for a in sys.argv[1:]]
        try:
            rc = subprocess.run(cmd, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            rc = 124
        if rc != 0:
            print(f"{part}: exit status {rc}; nothing further is started", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())

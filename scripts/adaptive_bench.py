#!/usr/bin/env python3
"""Adaptive sampling measured: what the four kernels cost, where an adaptive round breaks even
with a uniform frame, and what the samples buy at equal paths.

  kernels    at WxH, each of rtEnqueueAccumulateSamples, rtEnqueueSelectPixels, rtEnqueueCameraPathsFor and
             rtEnqueueResolveSamples alone: HIP events around back-to-back launches after a warm-up, the cases
             alternating within each repetition, medians; beside each the time a device-to-device copy in the
             same run needs for the bytes an ideal pass moves (accumulate 20 B in + 64 B read-modify-write per
             record, select 32 B per pixel + 4 B per selected pixel, indexed camera paths 40 B per record,
             resolve 48 B per pixel).
  breakeven  Cornell and the bunny proxy, 9 bounces: one adaptive round (select, the blocking read of its
             result, indexed camera paths, trace, accumulate) with a fraction 1.0, 0.5, 0.25, 0.1 of the pixels
             selected -- scattered single pixels and whole rows -- beside one frame of a fused render.
  quality    Cornell: RMS error against a 256-sample reference of a uniform 16-sample image and of an adaptive
             image given the same number of paths (both through the statistics, so all three are the gamma of
             a linear mean; the reference takes other sample frames), the times, and the histogram of n.  The
             render's own 16-frame image against its own 256-frame image (means of gamma-encoded frames) is
             listed beside them.

  adaptive_bench.py [--width W --height H --bounces B --launches N --reps R --parts kernels,breakeven,quality]
                    [--json FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "mini-opencl-raytracer_amd"), os.path.join(REPO, "tests")]
sys.path.insert(0, os.path.join(REPO, "scripts"))

from rayquery_bench import MATHS, Events  # noqa: E402

FRACTIONS = (1.0, 0.5, 0.25, 0.1)


def median_of(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def timed(ctx, ev, cases, launches, reps):
    t = {}
    for _ in range(reps):                # the cases alternate within a repetition
        for name, fn in cases.items():
            for _ in range(2):
                fn()
            ctx.Finish()
            t.setdefault(name, []).append(ev.time_ms(fn, launches))
    return {name: median_of(v) for name, v in t.items()}


def stats_selecting(np, N, px, mask):
    """Statistics under which rtEnqueueSelectPixels(min_samples = max_samples = 1000) selects exactly `mask`, for
    a thousand rounds: the others sit at max_samples."""
    st = np.zeros(px, N.PIXEL_STATS_DTYPE)
    st["n"] = 1000.0
    st["n"][mask] = 0.0
    return st


def masks(np, W, H, fraction):
    px = W * H
    if fraction >= 1.0:
        return {"all": np.ones(px, bool)}
    rng = np.random.default_rng(int(fraction * 1000))
    rows = np.zeros((H, W), bool)
    rows[rng.random(H) < fraction] = True
    return {"scattered": rng.random(px) < fraction, "rows": rows.reshape(-1)}


def kernels(args, out):
    import numpy as np

    import clrt
    from clrt import _native as N
    from hip_helpers import HipRenderer

    W, H = args.width, args.height
    px = W * H
    r = HipRenderer(clrt.scene.cornell(), W, H, math=MATHS[args.math])
    ctx, k = r.ctx, r.k
    r.frame(1, light_bounces=1)          # sets the slots
    rng = np.random.default_rng(3)
    res_h = np.zeros(px, N.PATH_RESULT_DTYPE)
    res_h["radiance"] = rng.random((px, 3)).astype(np.float32)
    mk = ctx.create_buffer
    host = N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR
    results = mk(host, res_h.nbytes, res_h)
    ids_all = mk(host, px * 4, np.arange(px, dtype=np.uint32))
    ids_out, result = mk(N.MEM_READ_WRITE, px * 4), mk(N.MEM_READ_WRITE, 16)
    rays, seeds, image = mk(N.MEM_READ_WRITE, px * 32), mk(N.MEM_READ_WRITE, px * 4), mk(N.MEM_READ_WRITE, px * 16)
    stats = mk(host, px * 32, np.zeros(px, N.PIXEL_STATS_DTYPE))
    quarter = rng.random(px) < 0.25
    st_all = mk(host, px * 32, stats_selecting(np, N, px, np.ones(px, bool)))
    st_quarter = mk(host, px * 32, stats_selecting(np, N, px, quarter))
    st_none = mk(host, px * 32, stats_selecting(np, N, px, np.zeros(px, bool)))
    # (hot everywhere, so that every window is read to its first hot flag only; cold everywhere reads all 25)
    hot = np.zeros(px, N.PIXEL_STATS_DTYPE)
    hot["n"], hot["mean_y"], hot["m2_y"] = 8.0, 0.5, 100.0
    st_hot = mk(host, px * 32, hot)
    cold = hot.copy()
    cold["m2_y"] = 0.0
    st_cold = mk(host, px * 32, cold)
    copy_src, copy_dst = mk(N.MEM_READ_WRITE, px * 32), mk(N.MEM_READ_WRITE, px * 32)
    dst = copy_dst.device_pointer()
    ctx.Finish()
    ev = Events(ctx.stream())
    sel = dict(min_samples=1000, max_samples=1000, radius=1)
    byw = dict(min_samples=4, max_samples=64, radius=2)
    cases = {
        "accumulate": lambda: ctx.AccumulateSamples(k, ids_all, results, px, px, stats),
        "accumulate_without_ids": lambda: ctx.AccumulateSamples(k, None, results, px, px, stats),
        "select_all": lambda: ctx.SelectPixels(k, st_all, W, H, ids_out, result, **sel),
        "select_quarter": lambda: ctx.SelectPixels(k, st_quarter, W, H, ids_out, result, **sel),
        "select_none": lambda: ctx.SelectPixels(k, st_none, W, H, ids_out, result, **sel),
        "select_windows_hot_r2": lambda: ctx.SelectPixels(k, st_hot, W, H, ids_out, result, **byw),
        "select_windows_cold_r2": lambda: ctx.SelectPixels(k, st_cold, W, H, ids_out, result, **byw),
        "camera_paths_for": lambda: ctx.CameraPathsFor(k, ids_all, px, rays, seeds),
        "resolve": lambda: ctx.ResolveSamples(k, stats, W, H, image),
        "copy_32B_per_pixel": lambda: ctx.CopyToDevicePointer(copy_src, 0, px * 32, dst),
    }
    t = timed(ctx, ev, cases, args.launches, args.reps)
    rate = 2 * 32 * px / t["copy_32B_per_pixel"]["median"] / 1e6     # GB/s; a copy reads and writes
    nq = int(quarter.sum())
    ideal = {"accumulate": 84 * px, "accumulate_without_ids": 80 * px, "select_all": 36 * px,
             "select_quarter": 32 * px + 4 * nq, "select_none": 32 * px, "select_windows_hot_r2": 36 * px,
             "select_windows_cold_r2": 32 * px, "camera_paths_for": 40 * px, "resolve": 48 * px}
    s = {"pixels": px, "copy_gb_per_s": rate, "ms": t, "ideal_bytes": ideal,
         "ideal_copy_ms": {n: b / (rate * 1e6) for n, b in ideal.items()}}
    s["ratio_to_copy"] = {n: t[n]["median"] / s["ideal_copy_ms"][n] for n in ideal}
    out["kernels"] = s
    print(json.dumps({"kernels": s}), flush=True)
    r.close()


def breakeven(args, out):
    import numpy as np

    import clrt
    import clrt.proxy as P
    from clrt import _native as N
    from hip_helpers import HipRenderer

    W, H = args.width, args.height
    px = W * H
    out["breakeven"] = {}
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

        # (fused renders run on the context's render streams, which events on its main stream do not bracket:
        # wall clock around back-to-back launches and a wait, as bench.py times them)
        walls = []
        for _ in range(args.reps):
            render()
            ctx.Finish()
            t0 = time.perf_counter()
            for _ in range(args.launches):
                render()
            ctx.Finish()
            walls.append((time.perf_counter() - t0) * 1e3 / (8 * args.launches))
        s["render_frame_ms_all"] = median_of(walls)
        s["render_frame_ms"] = s["render_frame_ms_all"]["median"]
        for fraction in FRACTIONS:
            for shape, mask in masks(np, W, H, fraction).items():
                stats = mk(N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR, px * 32, stats_selecting(np, N, px, mask))
                n = [0]

                def one_round():
                    ctx.SelectPixels(k, stats, W, H, ids, result, min_samples=1000, max_samples=1000, radius=1)
                    ctx.ReadBuffer(result, got, blocking=True)
                    n[0] = int(got["selected"][0])
                    k.set_uint(N.FRAME_COUNT, frame[0])
                    frame[0] += 1
                    ctx.CameraPathsFor(k, ids, n[0], rays, seeds)
                    ctx.TracePaths(k, rays, res, n[0], seeds=seeds)
                    ctx.AccumulateSamples(k, ids, res, n[0], px, stats)

                t = timed(ctx, ev, {"round": one_round}, args.launches, args.reps)["round"]
                assert n[0] == int(mask.sum())
                s["rounds"][f"{fraction}_{shape}"] = {"selected": n[0], "ms": t,
                                                      "over_render_frame": t["median"] / s["render_frame_ms"]}
                stats.release()
        out["breakeven"][name] = s
        print(json.dumps({"breakeven": {name: s}}), flush=True)
        r.close()


def quality(args, out):
    import numpy as np

    import clrt
    from clrt import _native as N

    W, H = args.width, args.height
    px = W * H
    rt = clrt.Raytracer(W, H)
    rt.Init()
    rt.upload_scene(clrt.scene.cornell())
    rt.kernel.set_math_mode(MATHS[args.math])
    rt.light_bounces = args.bounces
    rt.read_back = False

    def rms(a, b):
        d = a[..., :3].astype(np.float64) - b[..., :3].astype(np.float64)
        return float(np.sqrt((d * d).mean()))

    def uniform(samples, first_frame):
        rt.reset_samples()
        rt._sample_frame = first_frame
        t0 = time.perf_counter()
        img, info = rt.render_adaptive(samples, min_samples=samples, max_samples=samples)
        return img, info, time.perf_counter() - t0

    uniform(2, 1)                                    # warm-up
    ref, ref_info, _ = uniform(args.reference, 100001)   # sample frames no test image takes
    u16, u_info, u_s = uniform(16, 1)
    budget = u_info["paths"]
    rows = {}
    b = rt._adaptive_buffers()
    rb, sb, ob = rt._trace_buffers(px)
    got = np.zeros(1, N.SELECT_RESULT_DTYPE)
    for max_samples in (32, 64, 128):
        # render_adaptive's round, stopped at the budget of paths (one resolve and one read-back at the end,
        # as in the uniform run)
        rt.reset_samples()
        rt.set_uniforms()
        t0 = time.perf_counter()
        paths, rounds = 0, 0
        while paths < budget:
            rt.ctx.SelectPixels(rt.kernel, b["stats"], W, H, b["ids"], b["result"], 0.05, 0.01, 4, max_samples, 1)
            rt.ctx.ReadBuffer(b["result"], got, blocking=True)
            n = int(got["selected"][0])
            if n == 0:
                break
            rounds += 1
            rt.kernel.set_uint(N.FRAME_COUNT, rounds)
            rt.ctx.CameraPathsFor(rt.kernel, b["ids"], n, rb, sb)
            rt.ctx.TracePaths(rt.kernel, rb, ob, n, seeds=sb)
            rt.ctx.AccumulateSamples(rt.kernel, b["ids"], ob, n, px, b["stats"])
            paths += n
        rt.ctx.ResolveSamples(rt.kernel, b["stats"], W, H, b["image"])
        img = np.empty((H, W, 4), np.float32)
        rt.ctx.ReadBuffer(b["image"], img, blocking=True)
        secs = time.perf_counter() - t0
        n = rt.sample_stats()["n"].reshape(-1).astype(np.int64)
        hist = np.bincount(n)
        rows[str(max_samples)] = {"paths": paths, "rounds": rounds, "seconds": secs, "rms": rms(img, ref),
                                  "last_selected": int(got["selected"][0]), "last_hot": int(got["hot"][0]),
                                  "n_histogram": {str(i): int(c) for i, c in enumerate(hist) if c}}
    # the render's own images: running means of gamma-encoded frames
    def render(frames):
        rt.frame_count = 1
        rt.ctx.WriteBuffer(rt.output, np.zeros((px, 4), np.float32))
        rt.ctx.Finish()
        t0 = time.perf_counter()
        done = 0
        while done < frames:
            rt.set_uniforms()
            rt.ctx.ExecuteKernelFrames(rt.kernel, px, 8)
            rt.frame_count += 8
            done += 8
        img = np.empty((H, W, 4), np.float32)
        rt.ctx.ReadBuffer(rt.output, img, blocking=True)
        return img, time.perf_counter() - t0

    render(8)
    r16, r16_s = render(16)
    r256, _ = render(args.reference)
    s = {"pixels": px, "reference_samples": args.reference, "budget_paths": budget,
         "uniform16": {"paths": u_info["paths"], "seconds": u_s, "rms": rms(u16, ref)},
         "adaptive_by_max_samples": rows,
         "render16_fused": {"seconds": r16_s, "rms_to_render_reference": rms(r16, r256),
                            "rms_to_linear_reference": rms(r16, ref)}}
    out["quality"] = s
    print(json.dumps({"quality": s}), flush=True)
    rt.release()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--bounces", type=int, default=9)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reference", type=int, default=256, help="samples per pixel of the quality reference")
    ap.add_argument("--math", choices=list(MATHS), default="shipped")
    ap.add_argument("--parts", default="kernels,breakeven,quality")
    ap.add_argument("--json", help="write the results here as well")
    args = ap.parse_args()
    out = {"width": args.width, "height": args.height, "bounces": args.bounces, "math": args.math,
           "launches": args.launches, "reps": args.reps}
    for part in args.parts.split(","):
        {"kernels": kernels, "breakeven": breakeven, "quality": quality}[part](args, out)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

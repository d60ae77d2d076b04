#!/usr/bin/env python3
"""Cost of shadow rays (rtKernelSetShadowRays) in rtEnqueueTracePaths: the camera paths of Cornell (scene in
LDS) and the bunny proxy (records in HBM/L2) at WxH and 9 bounces, light types 0 and 1, traced with the setting
off and on.

Per scene and light type: HIP events around back-to-back launches after a warm-up, off and on alternating within
each repetition, medians with min and max (the run-to-run spread); then one launch each with the statistics on,
which gives the rays, node visits and triangle tests walked with and without shadow rays and the shadow rays per
path.  The time ratio on/off is reported beside the ratios of rays and of traversal steps (visits + tests).

--off-only times the setting-off trace alone, and --package DIR takes clrt and the library from another build's
package directory: together they time a build from before the setting existed in the same session.

  shadow_bench.py [--width W --height H --bounces B --launches N --reps R --math shipped] [--json FILE]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def median_of(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run(args):
    sys.path[:0] = [args.package or os.path.join(REPO, "mini-opencl-raytracer_amd"), os.path.join(REPO, "tests")]
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import numpy as np

    import clrt
    import clrt.proxy as P
    from clrt import _native as N
    from hip_helpers import HipRenderer
    from rayquery_bench import MATHS, Events

    W, H = args.width, args.height
    n = W * H
    launches, reps = args.launches, args.reps
    settings = (False,) if args.off_only else (False, True)
    out = {"width": W, "height": H, "paths": n, "bounces": args.bounces, "math": args.math, "launches": launches,
           "reps": reps, "off_only": args.off_only, "scenes": {}}
    for name, scene in (("cornell", clrt.scene.cornell()), ("bunny_proxy", P.bunny_proxy())):
        r = HipRenderer(scene, W, H, math=MATHS[args.math])
        ctx, k = r.ctx, r.k
        rays = ctx.create_buffer(N.MEM_READ_WRITE, n * 32)
        seeds = ctx.create_buffer(N.MEM_READ_WRITE, n * 4)
        res = ctx.create_buffer(N.MEM_READ_WRITE, n * 16)
        r.frame(1, light_bounces=1)          # sets the slots
        ctx.CameraPaths(k, n, rays, seeds)
        ctx.Finish()
        ev = Events(ctx.stream())
        per_light = {}
        for lt in (0, 1):
            k.set_int(N.LIGHT_BOUNCES, args.bounces)
            k.set_int(N.LIGHT_TYPE, lt)

            def trace():
                ctx.TracePaths(k, rays, res, n, seeds=seeds)

            def setting(on):
                if not args.off_only:
                    k.set_shadow_rays(on)

            t = {on: [] for on in settings}
            for _ in range(reps):            # off and on alternate within a repetition
                for on in settings:
                    setting(on)
                    for _ in range(2):
                        trace()
                    ctx.Finish()
                    t[on].append(ev.time_ms(trace, launches))
            s = {"off_ms": median_of(t[False])}
            s["off_spread"] = (s["off_ms"]["max"] - s["off_ms"]["min"]) / s["off_ms"]["median"]
            if not args.off_only:
                s["on_ms"] = median_of(t[True])
                s["on_over_off"] = s["on_ms"]["median"] / s["off_ms"]["median"]
                # one launch each with the counters on
                k.set_stats(True)
                counts = {}
                for on in settings:
                    setting(on)
                    k.reset_stats()
                    trace()
                    ctx.Finish()
                    st = k.stats()
                    counts[on] = {c: int(st[c]) for c in ("rays", "node_visits", "tri_tests", "hits")}
                k.set_stats(False)
                setting(False)
                steps = {on: counts[on]["node_visits"] + counts[on]["tri_tests"] for on in settings}
                s["counters_off"], s["counters_on"] = counts[False], counts[True]
                s["shadow_rays_per_path"] = (counts[True]["rays"] - counts[False]["rays"]) / n
                s["rays_on_over_off"] = counts[True]["rays"] / counts[False]["rays"]
                s["steps_on_over_off"] = steps[True] / steps[False]
            per_light[f"light{lt}"] = s
        out["scenes"][name] = {"scene_in_lds": bool(k.scene_in_lds()), **per_light}
        print(json.dumps({name: out["scenes"][name]}), flush=True)
        for b in (rays, seeds, res):
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
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--math", choices=["pinned", "devicelib", "shipped"], default="shipped")
    ap.add_argument("--off-only", action="store_true", help="time the setting-off trace alone")
    ap.add_argument("--package", help="package directory (clrt/ and lib/) of the build to time")
    ap.add_argument("--json", help="write the results here as well")
    run(ap.parse_args())


if __name__ == "__main__":
    main()

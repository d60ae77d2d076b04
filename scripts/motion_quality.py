#!/usr/bin/env python3
"""What motion records buy when geometry moves (Raytracer.move_vertices(keep_previous=True) with temporal(motion=True)
and reproject_samples_motion()), on the Cornell box with its short box translated by tests/motion_inputs.BOX_SHIFT.

Temporal: `--old` frames of the scene as it was and temporal(); the move; `--new` frames of the moved scene; then the
mean squared error against `--truth` frames of the moved scene, over all pixels and over the pixels that show the
short box before or after the move, for
  restart       the new frames alone
  camera_only   temporal(): the reprojection that knows the camera's motion only -- the ghosting case
  motion        temporal(motion=True)

Adaptive: render_adaptive() until nothing is selected; the move; then, one round at a time until nothing is selected
again, the paths traced and the error of the resolved image against a `--truth`-sample image of the moved scene, for
  reset         reset_samples()
  camera_only   reproject_samples(camera)
  motion        reproject_samples_motion(camera)

  motion_quality.py [--width W --height H --old 32 --new 8 --truth 256 --math pinned --json OUT]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "mini-opencl-raytracer_amd"), os.path.join(REPO, "tests"),
                os.path.join(REPO, "scripts")]

from rayquery_bench import MATHS  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--height", type=int, default=144)
    ap.add_argument("--old", type=int, default=32)
    ap.add_argument("--new", type=int, default=8)
    ap.add_argument("--truth", type=int, default=256)
    ap.add_argument("--max-rounds", type=int, default=200)
    ap.add_argument("--math", choices=list(MATHS), default="pinned")
    ap.add_argument("--json", help="write the results here as well")
    args = ap.parse_args()

    import numpy as np

    import clrt
    import motion_inputs as I

    W, H = args.width, args.height
    scene = clrt.scene.cornell()
    pos, _ = I.moved_scene()
    first, n = I.BOX_RANGE
    box_tri = I.short_box(scene.triangles)

    def fresh():
        rt = clrt.Raytracer(W, H)
        rt.Init()
        rt.upload_scene(scene)
        rt.kernel.set_math_mode(MATHS[args.math])
        return rt

    def move(rt, keep):
        rt.move_vertices(pos[first:first + n], first=first, keep_previous=keep)

    def frames(rt, count):
        rt.frame_count = 1
        for _ in range(count):
            rt.RenderFrame()
        return rt.pixels.reshape(H, W, 4).astype(np.float64)

    def on_box(rt):
        m = rt.motion()
        return (m["prim"] >= 0) & box_tri[np.where(m["prim"] >= 0, m["prim"], 0)]

    # ---- the truths, and the pixels the box covers before or after ----
    rt = fresh()
    region = on_box(rt)
    move(rt, False)
    region |= on_box(rt)
    truth = frames(rt, args.truth)[..., :3]
    truth_s, _ = rt.render_adaptive(args.truth, min_samples=args.truth, max_samples=args.truth)
    truth_s = truth_s[..., :3].astype(np.float64)
    rt.release()

    def err(img, ref):
        d = (np.asarray(img, np.float64)[..., :3] - ref) ** 2
        return {"all": float(d.mean()), "box": float(d[region].mean())}

    out = {"width": W, "height": H, "math": args.math, "old_frames": args.old, "new_frames": args.new,
           "truth_frames": args.truth, "shift": list(I.BOX_SHIFT), "box_pixels": int(region.sum()), "temporal": {},
           "adaptive": {}}

    # ---- temporal ----
    for case in ("restart", "camera_only", "motion"):
        rt = fresh()
        frames(rt, args.old)
        rt.temporal()
        move(rt, case == "motion")
        img = frames(rt, args.new)
        if case != "restart":
            img = rt.temporal(motion=case == "motion")
            out["temporal"][case + "_mean_count_on_box"] = float(img[..., 3][region].mean())
        out["temporal"][case] = err(img, truth)
        rt.release()

    # ---- adaptive ----
    def converge(rt):
        rows, paths = [], 0
        for _ in range(args.max_rounds):
            img, info = rt.render_adaptive(1)
            if info["rounds"] == 0:
                break
            paths += info["paths"]
            rows.append((paths, err(img, truth_s)))
        return rows

    for case in ("reset", "camera_only", "motion"):
        rt = fresh()
        before = converge(rt)
        move(rt, case == "motion")
        if case == "reset":
            rt.reset_samples()
        else:
            (rt.reproject_samples_motion if case == "motion" else rt.reproject_samples)(rt.camera)
        st = rt.sample_stats()
        img0, _ = rt.render_adaptive(0)
        rows = converge(rt)
        out["adaptive"][case] = {"paths_before_the_move": before[-1][0], "carried_share": float((st["n"] > 0).mean()),
                                 "carried_share_on_box": float((st["n"][region] > 0).mean()),
                                 "error_before_any_path": err(img0, truth_s) if case != "reset" else None,
                                 "paths": rows[-1][0] if rows else 0, "rounds": len(rows),
                                 "error": rows[-1][1] if rows else err(img0, truth_s)}
        rt.release()
    reset_paths = out["adaptive"]["reset"]["paths"]
    for case in ("camera_only", "motion"):
        out["adaptive"][case]["paths_over_reset"] = out["adaptive"][case]["paths"] / reset_paths
    print(json.dumps(out), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fjson:
            json.dump(out, fjson, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What carrying the adaptive statistics across a camera move buys (Raytracer.reproject_samples against
reset_samples), on the Cornell box.

render_adaptive() runs at the reference camera until nothing is selected; the camera moves by (0.37, 0, 0.1).
Then, one round at a time until nothing is selected again, once after reproject_samples(prev) and once after
reset_samples(): the paths traced, and the mean squared error of the resolved image over all pixels against a
`--truth`-sample image at the new camera, after every round.  Reported: both totals, both final errors, the error of
the reset run at the first round where it has traced at least as many paths as the reprojected run needed in all
(the comparison at equal paths; with its path count), and the share of pixels that kept statistics.

  reproject_samples_quality.py [--width W --height H --truth 256 --max-history 16 --math pinned --json OUT]
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
    ap.add_argument("--truth", type=int, default=256)
    ap.add_argument("--max-history", type=float, default=16.0)
    ap.add_argument("--max-rounds", type=int, default=200)
    ap.add_argument("--math", choices=list(MATHS), default="pinned")
    ap.add_argument("--json", help="write the results here as well")
    args = ap.parse_args()

    import numpy as np

    import clrt

    W, H = args.width, args.height
    rt = clrt.Raytracer(W, H, read_back=False)
    rt.Init()
    rt.upload_scene(clrt.scene.cornell())
    rt.kernel.set_math_mode(MATHS[args.math])
    prev = rt.camera
    p = prev.position
    moved = clrt.renderer.Camera(position=(p[0] + 0.37, p[1], p[2] + 0.1), front=prev.front, up=prev.up)

    # the truth at the new camera
    rt.camera = moved
    truth, _ = rt.render_adaptive(args.truth, min_samples=args.truth, max_samples=args.truth)
    truth = truth[..., :3].astype(np.float64)

    def mse(img):
        return float(((img[..., :3] - truth) ** 2).mean())

    def converge():
        """Rounds until nothing is selected: [(paths so far, error)], per round."""
        rows, paths = [], 0
        for _ in range(args.max_rounds):
            img, info = rt.render_adaptive(1)
            if info["rounds"] == 0:
                break
            paths += info["paths"]
            rows.append((paths, mse(img)))
        return rows

    # the history at the reference camera
    rt.camera = prev
    rt.reset_samples()
    before = converge()
    out = {"width": W, "height": H, "math": args.math, "truth_samples": args.truth, "max_history": args.max_history,
           "paths_before_the_move": before[-1][0], "rounds_before_the_move": len(before)}

    rt.camera = moved
    rt.reproject_samples(prev, max_history=args.max_history)
    st = rt.sample_stats()
    out["carried_share"] = float((st["n"] > 0).mean())
    out["mean_carried_n"] = float(st["n"][st["n"] > 0].mean())
    img0, _ = rt.render_adaptive(0)
    out["reprojected_error_before_any_path"] = mse(img0)
    rep = converge()
    rt.reset_samples()
    res = converge()
    out["reproject"] = {"paths": rep[-1][0], "rounds": len(rep), "error": rep[-1][1], "first_round_paths": rep[0][0]}
    out["reset"] = {"paths": res[-1][0], "rounds": len(res), "error": res[-1][1], "first_round_paths": res[0][0]}
    at = next((row for row in res if row[0] >= rep[-1][0]), res[-1])
    out["reset_at_equal_paths"] = {"paths": at[0], "error": at[1]}
    out["paths_ratio"] = rep[-1][0] / res[-1][0]
    out["rounds_reproject"], out["rounds_reset"] = rep, res
    print(json.dumps({k: v for k, v in out.items() if not k.startswith("rounds_re")}), flush=True)
    rt.release()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fjson:
            json.dump(out, fjson, indent=1)


if __name__ == "__main__":
    main()

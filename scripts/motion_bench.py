#!/usr/bin/env python3
"""Cost of the motion calls at render size (rtEnqueueFrameMotion and the two ...Motion reprojections).

For Cornell and the bunny proxy at `--width` x `--height`, HIP events around `--launches` back-to-back calls after a
warm-up, `--reps` repetitions in which the cases alternate; per case the median, the least and the largest.

  frame_motion          rtEnqueueFrameMotion with nothing moved (prev_* NULL, n_tris 0)
  frame_motion_kept     ... over the whole triangle array's kept vertices and normals (rtEnqueueExtractVertices)
  pair                  rtEnqueueCameraRays + rtEnqueueIntersectRays (closest): the two launches whose ray and hit
                        traffic the fused launch avoids (their kernels are the parent commit's: scripts/isa_compare.sh)
  pair_hit_motion       ... + rtEnqueueHitMotion: the composition that writes the same records
  extract               rtEnqueueExtractVertices of the whole array, with normals
  temporal, temporal_motion      rtEnqueueTemporalAccumulate against ...Motion on the same buffers
  reproject, reproject_motion    rtEnqueueReprojectSamples against ...Motion on the same buffers

The reprojections' inputs are Raytracer.temporal()'s and reproject_samples()' own buffers after a camera move of
(0.37, 0, 0.1), and the records are FrameMotion's at the new camera with nothing moved.

  motion_bench.py [--width W --height H --launches N --reps R --math shipped --json OUT]
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--math", choices=list(MATHS), default="shipped")
    ap.add_argument("--json", help="write the results here as well")
    args = ap.parse_args()

    import clrt
    import clrt.proxy as P
    from clrt import _native as N

    W, H = args.width, args.height
    n = W * H
    out = {"width": W, "height": H, "pixels": n, "math": args.math, "launches": args.launches, "reps": args.reps,
           "scenes": {}}
    for name, scene in (("cornell", clrt.scene.cornell()), ("bunny_proxy", P.bunny_proxy())):
        rt = clrt.Raytracer(W, H, read_back=False)
        rt.Init()
        rt.upload_scene(scene)
        rt.kernel.set_math_mode(MATHS[args.math])
        ctx, k = rt.ctx, rt.kernel
        nt = len(scene.triangles)
        mk = lambda size: ctx.create_buffer(N.MEM_READ_WRITE, size)   # noqa: E731
        rays, hits, motion = mk(n * 32), mk(n * 16), mk(n * 32)
        kept_p, kept_n = mk(nt * 48), mk(nt * 48)
        tris = rt._scene_bufs[0]
        ctx.ExtractVertices(tris, 0, nt, kept_p, kept_n)
        # the reprojections' buffers: a converged view, the camera moved, both passes run once
        for _ in range(2):
            rt.RenderFrame()
        rt.temporal()
        rt.render_adaptive(2, min_samples=2, max_samples=2)
        prev = rt.camera
        p = prev.position
        rt.camera = clrt.renderer.Camera(position=(p[0] + 0.37, p[1], p[2] + 0.1), front=prev.front, up=prev.up)
        rt.frame_count = 1
        rt.RenderFrame()
        rt.temporal()
        rt.reproject_samples(prev)
        rt.set_uniforms()
        ctx.FrameMotion(k, n, motion)
        views = [(tuple(v.position), tuple(v.front), tuple(v.up)) for v in (rt.camera, prev)]
        now, old = rt._temporal_at, 1 - rt._temporal_at
        t_out, s_out = mk(n * 16), mk(n * 32)
        b = rt._adaptive_buffers()
        feat_prev, feat_cur = rt._reproject_feat

        def temporal(m):
            ctx.TemporalAccumulate(k, rt.output, rt._temporal_feat[now], rt._temporal_img[old], rt._temporal_feat[old], W, H,
                                   t_out, views[0], views[1], 1.0, 0.0, 32.0, 0.05, 0.9, motion=m)

        def reproject(m):
            ctx.ReprojectSamples(k, b["spare"], feat_prev, feat_cur, W, H, s_out, views[0], views[1], motion=m)

        def pair():
            ctx.CameraRays(k, n, rays)
            ctx.IntersectRays(k, rays, hits, n)

        def pair_hit_motion():
            pair()
            ctx.HitMotion(k, hits, 0, n, motion)

        cases = {
            "pair": pair,
            "frame_motion": lambda: ctx.FrameMotion(k, n, motion),
            "pair_hit_motion": pair_hit_motion,
            "frame_motion_kept": lambda: ctx.FrameMotion(k, n, motion, kept_p, kept_n, 0, nt),
            "extract": lambda: ctx.ExtractVertices(tris, 0, nt, kept_p, kept_n),
            "temporal": lambda: temporal(None),
            "temporal_motion": lambda: temporal(motion),
            "reproject": lambda: reproject(None),
            "reproject_motion": lambda: reproject(motion),
        }
        ctx.Finish()
        ev = Events(ctx.stream())
        res = {}
        for _ in range(args.reps):               # the cases alternate within a repetition
            for cname, fn in cases.items():
                fn()                             # warm-up
                ctx.Finish()
                res.setdefault(cname, []).append(ev.time_ms(fn, args.launches))   # (per call)
        ctx.Finish()
        s = {"triangles": nt, "scene_in_lds": bool(k.scene_in_lds())}
        for cname, v in res.items():
            s[cname + "_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}
        s["frame_motion_over_pair"] = s["frame_motion_ms"]["median"] / s["pair_ms"]["median"]
        s["temporal_motion_over_plain"] = s["temporal_motion_ms"]["median"] / s["temporal_ms"]["median"]
        s["reproject_motion_over_plain"] = s["reproject_motion_ms"]["median"] / s["reproject_ms"]["median"]
        out["scenes"][name] = s
        print(json.dumps({name: s}), flush=True)
        for buf in (rays, hits, motion, kept_p, kept_n, t_out, s_out):
            buf.release()
        rt.release()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as fjson:
            json.dump(out, fjson, indent=1)


if __name__ == "__main__":
    main()

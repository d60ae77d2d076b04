"""The render cases of test_octant_cull_gpu.py, shared with octant_cull_nocull_render.py (which renders
them on the RT_OCTANT_CULL=0 library in a process of its own)."""
import numpy as np

import clrt
from clrt import _native as N
from hip_helpers import DEFAULT_CAMERA, HipRenderer, rgb

import octant_cull_scenes as OC
import stress_scenes as SS

FRAMES = tuple(range(8))
BOUNCES = 9
# scene, W, H, camera: Cornell from inside the box (all 8 octants among the camera rays' bounces and the
# primary rays' signs), Cornell from the bench camera, the hand-built room
CASES = {
    "cornell-inside": ("cornell", 128, 72, SS.CAMERAS["inside"]),
    "cornell-bench": ("cornell", 64, 64, DEFAULT_CAMERA),
    "room": ("room", 64, 64, SS.CAMERAS["inside"]),
}
_scenes = {}


def scene(name):
    if name not in _scenes:
        _scenes[name] = clrt.scene.cornell() if name == "cornell" else OC.room_scene()[0]
    return _scenes[name]


def render(case, math=N.MATH_PINNED, fused=True, stats=False, force_global=False, sched=N.SCHED_STEP, tune=()):
    """FRAMES of a case -> (radiance words, hit ids, hit t bits, rtKernelGetOctantCull, rtKernelGetNodeCollapse,
    rt_stats, scene in LDS)"""
    name, W, H, camera = CASES[case]
    r = HipRenderer(scene(name), W, H, math=math, hits=True, stats=stats, force_global=force_global, sched=sched)
    try:
        for knob, value in tune:
            r.k.set_tuning(knob, value)
        if fused:
            r.frame(FRAMES[0], light_bounces=BOUNCES, camera=camera, n_frames=len(FRAMES))
        else:
            r.k.set_tuning("perframe_defer", 0)
            for f in FRAMES:
                r.frame(f, light_bounces=BOUNCES, camera=camera)
        img = rgb(r.result()).view(np.uint32)
        ids, t = r.hits()
        return img, ids, t.view(np.uint32), r.k.octant_cull(), r.k.node_collapse(), r.k.stats(), r.k.scene_in_lds()
    finally:
        r.close()

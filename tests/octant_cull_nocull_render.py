"""The shipped-math reference of test_octant_cull_gpu.py: its render cases on the library built with
RT_OCTANT_CULL=0 (lib/librt_hip_nocull.so: the same kernel objects, no pruned link set).  A process loads one
librt_hip, so the test starts this file once with RT_HIP_LIB pointing at that library:
    RT_HIP_LIB=.../librt_hip_nocull.so python octant_cull_nocull_render.py OUT.npz"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(os.path.dirname(HERE), "mini-opencl-raytracer_amd"), HERE]

from clrt import _native as N  # noqa: E402

import octant_cull_gpu_cases as GC  # noqa: E402


def main(out):
    assert os.path.basename(N.HIP_LIB_PATH) == "librt_hip_nocull.so", N.HIP_LIB_PATH
    res = {}
    for case in GC.CASES:
        for fused in (True, False):
            img, ids, t, info = GC.render(case, math=N.MATH_SHIPPED, fused=fused)[:4]
            assert info == {"pruned_links": 0, "contracted_links": 0, "scene_certified": False, "launch_pruned": False}
            key = f"{case}-{'fused' if fused else 'perframe'}"
            res[key + "-img"], res[key + "-ids"], res[key + "-t"] = img, ids, t
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1])

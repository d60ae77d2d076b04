"""CPU: tests/shadow_path_ref.py -- path_ref's replay of Render with the shadow ray rt_hip.h defines at
kernel_bvh.cl:378 -- is pinned before any GPU test leans on it.  On Cornell at 32x18, frame counts 0 and 1,
light types 0/1/2 and 1, 3 and 9 bounces:
  * with shadows off it is PathTracer.trace bit for bit and counter for counter (which test_path_ref.py
    pins to the oracle's Render);
  * with shadows on the inputs exercise both outcomes: every light type has at least 30 occluded and at
    least 30 unoccluded shadow rays at 3 bounces, and what a shadow ray may change is only what the
    definition lets it change."""
import os

import numpy as np
import pytest

W, H = 32, 18
FRAMES, LIGHTS, BOUNCES = (0, 1), (0, 1, 2), (1, 3, 9)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def replays(cornell, oracle_mod):
    import path_ref
    import shadow_path_ref
    cams = {fc: path_ref.camera_paths(W, H, fc) for fc in FRAMES}
    keys = [(fc, lt) for fc in FRAMES for lt in LIGHTS]
    procs = min(16, os.cpu_count() or 1)
    plain = path_ref.trace_rays_pool([(cornell, cams[fc][0], cams[fc][1], BOUNCES, lt, 1.0) for fc, lt in keys], procs)
    off = shadow_path_ref.trace_rays_pool(
        [(cornell, cams[fc][0], cams[fc][1], BOUNCES, lt, 1.0, False) for fc, lt in keys], procs)
    on = shadow_path_ref.trace_rays_pool(
        [(cornell, cams[1][0], cams[1][1], BOUNCES, lt, 1.0, True) for lt in LIGHTS], procs)
    return {"plain": dict(zip(keys, plain)), "off": dict(zip(keys, off)), "on": dict(zip(LIGHTS, on))}


@pytest.mark.parametrize("bounces", BOUNCES)
@pytest.mark.parametrize("light_type", LIGHTS)
@pytest.mark.parametrize("frame_count", FRAMES)
def test_shadows_off_is_the_plain_replay(replays, frame_count, light_type, bounces):
    got, want = replays["off"][(frame_count, light_type)][bounces], replays["plain"][(frame_count, light_type)][bounces]
    assert bits(got["radiance"]).tobytes() == bits(want["radiance"]).tobytes()
    assert np.array_equal(got["prim"], want["prim"]) and np.array_equal(got["rounds"], want["rounds"])
    assert got["counts"] == want["counts"]
    assert got["shadow"] == (0, 0) and not got["cast"].any()


@pytest.mark.parametrize("light_type", LIGHTS)
def test_both_outcomes_are_exercised(replays, light_type):
    cast, occluded = replays["on"][light_type][3]["shadow"]
    assert occluded >= 30 and cast - occluded >= 30, (cast, occluded)


@pytest.mark.parametrize("bounces", BOUNCES)
@pytest.mark.parametrize("light_type", LIGHTS)
def test_a_shadow_ray_changes_only_the_lights_term(replays, light_type, bounces):
    on, off = replays["on"][light_type][bounces], replays["plain"][(1, light_type)][bounces]
    # the path is Render's: same first hit, same number of path segments, same shaded hits
    assert np.array_equal(on["prim"], off["prim"]) and np.array_equal(on["rounds"], off["rounds"])
    assert on["counts"][3] == off["counts"][3]
    # each shadow ray is one ray more, and walks at least the root
    cast, occluded = on["shadow"]
    assert on["counts"][0] == off["counts"][0] + cast
    assert on["counts"][1] >= off["counts"][1] + cast and on["counts"][2] >= off["counts"][2]
    # a path without a shadow ray keeps its bits; the light's term is never negative in this scene, so an
    # occluded one can only lose radiance
    same = on["cast"] == 0
    assert (bits(on["radiance"][same]) == bits(off["radiance"][same])).all()
    assert (on["radiance"] <= off["radiance"]).all()
    changed = (bits(on["radiance"]) != bits(off["radiance"])).any(axis=1)
    assert changed.sum() <= occluded
    if bounces == 3:
        assert changed.sum() >= 30

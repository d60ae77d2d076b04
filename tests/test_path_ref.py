"""CPU: tests/path_ref.py -- the Python replay of the oracle's Render for arbitrary rays and seeds --
is pinned to the oracle before any GPU test leans on it.  On Cornell at 32x18, frame counts 0 and 1,
light types 0/1/2 and 1, 3 and 9 bounces, the replay over the camera's rays and post-CreateRay seeds
(both computed in numpy), pushed through oracle_pow as KernelEntry stores a frame (exponent 0.45454545f
at frame 0; 0.454545f at frame 1 over a zero image, where the accumulation is pow(radiance, 0.454545f)),
must equal oracle.render's result bits, primary ids and counters."""
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
    cams = {fc: path_ref.camera_paths(W, H, fc) for fc in FRAMES}
    keys = [(fc, lt) for fc in FRAMES for lt in LIGHTS]
    jobs = [(cornell, cams[fc][0], cams[fc][1], BOUNCES, lt, 1.0) for fc, lt in keys]
    return dict(zip(keys, path_ref.trace_rays_pool(jobs, procs=min(16, os.cpu_count() or 1))))


@pytest.mark.parametrize("bounces", BOUNCES)
@pytest.mark.parametrize("light_type", LIGHTS)
@pytest.mark.parametrize("frame_count", FRAMES)
def test_replay_equals_the_oracle_render(cornell, oracle_mod, replays, frame_count, light_type, bounces):
    got = replays[(frame_count, light_type)][bounces]
    want, ids, _, counts = oracle_mod.render(cornell, W, H, frame_count=frame_count, light_bounces=bounces,
                                             light_type=light_type, want_hits=True, threads=4)
    powf = oracle_mod.lib().oracle_pow
    e = float(np.float32(0.45454545 if frame_count == 0 else 0.454545))
    stored = np.array([[powf(float(c), e) for c in px] for px in got["radiance"]], np.float32)
    assert np.array_equal(got["prim"], ids)
    bad = np.flatnonzero((bits(stored) != bits(want[:, :3])).any(axis=1))
    assert bad.size == 0, (bad[:5], stored[bad[:5]], want[bad[:5], :3])
    assert got["counts"] == (counts["rays"], counts["node_visits"], counts["tri_tests"], counts["hits"])


def test_the_numpy_camera_seeds_are_the_double_hash(oracle_mod):
    import path_ref
    L = oracle_mod.lib()
    for fc in (0, 1, 77):
        _, seeds = path_ref.camera_paths(7, 3, fc)
        want = [L.oracle_hash(L.oracle_hash((g + L.oracle_frame_hash(fc)) & 0xffffffff)) for g in range(21)]
        assert seeds.tolist() == want


def test_paths_reach_three_bounces_and_misses(replays):
    """(the inputs are not all one-round paths: the comparison above covers long ones too)"""
    r = replays[(1, 0)][9]
    assert (r["rounds"] >= 3).sum() >= 100 and (r["prim"] < 0).sum() >= 100

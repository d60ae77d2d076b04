"""CPU: the temporal reprojection's host side -- the plan (csrc/rt_temporal_plan.cpp temporal_plan: argument
checks in their documented order, the fp32 constants, the grid) and the address logic the kernel compiles
(csrc/rt_temporal_math.hpp), driven through the stand-alone tests/native/temporal_plan_main.cpp built with
plain g++ and once more with sanitizers; the numpy restatement tests/temporal_ref.py on cases whose answers
are known; and the Python surface of the entry point.  No GPU is touched.
"""
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "mini-opencl-raytracer_amd", "csrc")
SOURCES = [os.path.join(REPO, "tests", "native", "temporal_plan_main.cpp"), os.path.join(CSRC, "rt_temporal_plan.cpp")]

F = np.float32
FEATURES = np.dtype([("albedo", np.float32, (3,)), ("depth", np.float32), ("normal", np.float32, (3,)),
                     ("coverage", np.float32)])
DEFAULT = ((0.0, -25.0, 8.5), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
AWAY = ((0.0, -25.0, 8.5), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0))


def _build(out, *flags):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-o", out, *SOURCES],
                   check=True, timeout=300)
    return out


@pytest.fixture(scope="module")
def plan_main(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("tplan") / "temporal_plan_main"))


def _sweep_ok(stdout):
    m = re.search(r"sweep: (\d+) projections, (\d+) passed, (\d+) taps inside, (\d+) crossings bracketed, 0 failures",
                  stdout)
    assert m, stdout[-3000:]
    calls, passed, taps, bracketed = map(int, m.groups())
    # the sweep reaches both outcomes, taps on the image's border (fewer than four inside) and the crossings
    assert calls >= 1_000_000 and 0 < passed < calls and passed < taps < 4 * passed and bracketed >= 500, stdout


def test_projection_sweep_never_leaves_the_image(plan_main):
    p = subprocess.run([plan_main, "sweep"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:]
    _sweep_ok(p.stdout)


def test_error_rows_return_their_codes_in_order(plan_main):
    p = subprocess.run([plan_main, "errors"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "FAILED" not in p.stdout, p.stdout
    for row in ("valid", "valid_without_history", "params_null", "width_zero", "height_zero", "past_2_31",
                "product_near_2_64", "exactly_2_31", "camera_nan", "camera_infinite", "cur_frames_nan",
                "cur_frames_below_one", "cur_frames_huge", "history_frames_negative", "history_frames_infinite",
                "history_frames_nan", "history_frames_fraction", "history_frames_huge", "max_history_nan",
                "max_history_below_cur_frames", "max_history_huge", "depth_tolerance_nan", "depth_tolerance_negative",
                "depth_tolerance_above_one", "normal_threshold_nan", "normal_threshold_below", "normal_threshold_above",
                "hist_without_features", "features_without_hist", "cur_null", "cur_features_null", "out_null",
                "hist_foreign", "hist_features_foreign", "out_is_an_input", "cur_short", "cur_features_short",
                "hist_short", "hist_features_short", "out_short", "value_before_mem_object",
                "last_value_before_mem_object", "size_zero_before_buffer_size", "mem_object_before_size",
                "pairing_before_size", "constants"):
        assert re.search(rf"ok     {row}\b", p.stdout), (row, p.stdout)


def test_plan_and_projection_run_clean_under_sanitizers(tmp_path):
    """The same stand-alone program with address, undefined-behaviour and float-cast-overflow checks (host code,
    no preload): an out-of-range float -> int conversion in the projection would stop it."""
    exe = _build(str(tmp_path / "temporal_plan_san"), "-g", "-fsanitize=address,undefined,float-cast-overflow",
                 "-fno-sanitize-recover=all")
    for arg in ("sweep", "errors"):
        p = subprocess.run([exe, arg], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (arg, p.stdout[-2000:], p.stderr[-3000:])
        assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
        if arg == "sweep":
            _sweep_ok(p.stdout)


# ---- the restatement on cases with known answers ------------------------------------------------
W, H = 13, 9


def _plane(depth=45.0, coverage=1.0):
    """Features of a wall straight ahead: depth along each centre ray to the plane y = pos.y + depth."""
    import temporal_ref
    f = np.zeros((H, W), FEATURES)
    u = temporal_ref.centre_rays(W, H, DEFAULT[1], DEFAULT[2])
    f["depth"] = F(depth) / u[..., 1]
    f["albedo"], f["normal"], f["coverage"] = 0.5, (0.0, -1.0, 0.0), coverage
    return f


def _constant(rgb, w):
    img = np.empty((H, W, 4), np.float32)
    img[..., :3], img[..., 3] = rgb, w
    return img


def test_identical_cameras_over_a_plane_blend_by_sample_count():
    """History and current constant: out == h + (c - h) * alpha exactly, n = min(hn + cur_frames, max_history).
    The history's values and count are powers of two, so every bw * h is an exact scaling, the sums are
    h * sw exactly whatever the weights round to, and the quotients return h and hn themselves."""
    import temporal_ref
    f = _plane()
    cur, hist = _constant((0.3, 1.7, 0.011), 1.0), _constant((2.0, 0.25, 4.0), 4.0)
    for cur_frames, max_history in ((2.0, 32.0), (2.0, 5.0), (3.0, 8.0), (3.0, 3.0)):
        got, info = temporal_ref.temporal(cur, f, hist, f, W, H, DEFAULT, DEFAULT, cur_frames, 0.0, max_history,
                                          details=True)
        assert got.dtype == np.float32 and got.shape == (H, W, 4) and info["history"].all()
        # (at 13 x 9 a diagonal neighbour near the edge is over 5 % farther: some taps fail the depth test)
        assert (info["counted"][2:-2, 3:-3] == 4).all() and info["counted"].min() >= 1
        assert info["rejected"]["outside"] > 0
        n = min(F(4.0) + F(cur_frames), F(max_history))
        alpha = F(cur_frames) / n
        want = np.empty((H, W, 4), np.float32)
        want[..., :3] = hist[..., :3] + (cur[..., :3] - hist[..., :3]) * alpha
        want[..., 3] = n
        assert got.tobytes() == want.tobytes(), (cur_frames, max_history)


def test_previous_camera_facing_away_takes_the_no_history_row():
    import temporal_ref
    f = _plane()
    rng = np.random.default_rng(3)
    cur, hist = rng.random((H, W, 4)).astype(np.float32), rng.random((H, W, 4)).astype(np.float32) + 1
    got, info = temporal_ref.temporal(cur, f, hist, f, W, H, DEFAULT, AWAY, 3.0, details=True)
    assert not info["history"].any() and info["counted"].sum() == 0
    assert np.array_equal(got[..., :3], cur[..., :3]) and (got[..., 3] == 3.0).all()


def test_no_history_buffer_is_the_no_history_row_everywhere():
    import temporal_ref
    rng = np.random.default_rng(4)
    cur = rng.random((H, W, 4)).astype(np.float32)
    got = temporal_ref.temporal(cur, _plane(), None, None, W, H, DEFAULT, DEFAULT, 5.0)
    assert np.array_equal(got[..., :3], cur[..., :3]) and (got[..., 3] == 5.0).all()
    with pytest.raises(ValueError):
        temporal_ref.temporal(cur, _plane(), cur, None, W, H, DEFAULT, DEFAULT, 5.0)


def test_history_frames_overrides_the_w_slot():
    import temporal_ref
    f = _plane()
    cur, hist = _constant((0.5, 0.5, 0.5), 1.0), _constant((1.0, 1.0, 1.0), 0.0)   # w = 0: no tap would count
    got, info = temporal_ref.temporal(cur, f, hist, f, W, H, DEFAULT, DEFAULT, 2.0, 0.0, 32.0, details=True)
    assert not info["history"].any() and info["rejected"]["count"] > 0 and (got[..., 3] == 2.0).all()
    got, info = temporal_ref.temporal(cur, f, hist, f, W, H, DEFAULT, DEFAULT, 2.0, 16.0, 32.0, details=True)
    assert info["history"].all() and (got[..., 3] == 18.0).all()


def test_uncovered_current_pixel_is_copied_with_cur_frames():
    import temporal_ref
    cov = np.ones((H, W), np.float32)
    cov[4, 6], cov[0, 0] = 0.0, -1.0
    f = _plane(coverage=cov)
    rng = np.random.default_rng(5)
    cur, hist = rng.random((H, W, 4)).astype(np.float32), _constant((3.0, 3.0, 3.0), 8.0)
    got, info = temporal_ref.temporal(cur, f, hist, _plane(), W, H, DEFAULT, DEFAULT, 2.0, details=True)
    for y, x in ((4, 6), (0, 0)):
        assert got[y, x, :3].tobytes() == cur[y, x, :3].tobytes() and got[y, x, 3] == 2.0
        assert not info["history"][y, x]
    assert info["history"].sum() == W * H - 2


def test_history_tap_with_w_below_one_is_skipped():
    import temporal_ref
    f = _plane()
    cur, hist = _constant((0.0, 0.0, 0.0), 1.0), _constant((1.0, 1.0, 1.0), 4.0)
    hist[4, 6] = (1000.0, 1000.0, 1000.0, 0.5)       # would show in every pixel that taps it
    got, info = temporal_ref.temporal(cur, f, hist, f, W, H, DEFAULT, DEFAULT, 1.0, details=True)
    assert info["rejected"]["count"] >= 1 and info["counted"].min() < 4
    assert got[..., :3].max() < 1.0 + 1e-6
    # uncovered and non-finite history taps are selected away too, never multiplied by a zero weight
    hf = _plane()
    hf["coverage"][2, 3] = 0.0
    hist[2, 3] = (np.inf, np.nan, -np.inf, 4.0)
    got, info = temporal_ref.temporal(cur, f, hist, hf, W, H, DEFAULT, DEFAULT, 1.0, details=True)
    assert np.isfinite(got).all() and info["rejected"]["coverage"] >= 1


def test_non_finite_depths_take_the_no_history_row():
    import temporal_ref
    f = _plane()
    # (a depth near FLT_MAX at the same camera is not in this list: |v| overflows to +inf, inf <= tolerance * inf
    # holds, and the definition counts the taps -- defined, and as safe, if not useful)
    bad = [np.inf, -np.inf, np.nan, -45.0, 0.0, -0.0, -3.4e38, 1e-45]
    for i, d in enumerate(bad):
        f["depth"][1 + i // 4, 2 + i % 4] = d
    cur, hist = _constant((0.25, 0.25, 0.25), 1.0), _constant((1.0, 1.0, 1.0), 4.0)
    got, info = temporal_ref.temporal(cur, f, hist, _plane(), W, H, DEFAULT, DEFAULT, 1.0, details=True)
    for i in range(len(bad)):
        y, x = 1 + i // 4, 2 + i % 4
        assert not info["history"][y, x] and got[y, x].tolist() == [0.25, 0.25, 0.25, 1.0], (bad[i], got[y, x])
    assert info["history"].sum() == W * H - len(bad)


def test_constants_and_argument_checks():
    import temporal_ref
    assert temporal_ref.A.view(np.uint32) == 0x3ED41204
    assert temporal_ref.A == F(np.tan(np.float64(F(0.5) * (F(45.0) * F(3.1415) / F(180.0)))))
    ok = dict(cur_view=DEFAULT, prev_view=DEFAULT, cur_frames=1.0, history_frames=0.0, max_history=32.0,
              depth_tolerance=0.05, normal_threshold=0.9)
    assert temporal_ref.params_ok(**ok)
    for key, bad in (("cur_frames", 0.5), ("cur_frames", float("nan")), ("cur_frames", 2.0 ** 21),
                     ("history_frames", -1.0), ("history_frames", 0.5), ("history_frames", float("inf")),
                     ("max_history", 0.5), ("max_history", float("nan")), ("depth_tolerance", -0.1),
                     ("depth_tolerance", 1.5), ("normal_threshold", -1.5), ("normal_threshold", float("nan")),
                     ("cur_view", ((0.0, float("nan"), 0.0), (0, 1, 0), (0, 0, 1))),
                     ("prev_view", ((0.0, 0.0, 0.0), (0, float("inf"), 0), (0, 0, 1)))):
        assert not temporal_ref.params_ok(**{**ok, key: bad}), (key, bad)
    assert not temporal_ref.params_ok(**{**ok, "cur_frames": 8.0, "max_history": 4.0})


def test_native_declares_the_entry_point():
    import ctypes

    import clrt
    from clrt import _native as N
    assert "rtEnqueueTemporalAccumulate" in N.HIP_EXPORTS
    assert ctypes.sizeof(N.VIEW) == 36 and ctypes.sizeof(N.TEMPORAL_PARAMS) == 92
    assert [f[0] for f in N.TEMPORAL_PARAMS._fields_] == ["cur", "prev", "cur_frames", "history_frames", "max_history",
                                                           "depth_tolerance", "normal_threshold"]
    assert np.float32(N.TEMPORAL_TAN_HALF_FOV).view(np.uint32) == 0x3ED41204
    lib = clrt.hip_lib()  # (loading the library does not touch the GPU)
    assert len(lib.rtEnqueueTemporalAccumulate.argtypes) == 10
    assert callable(clrt.CLContext.TemporalAccumulate) and callable(clrt.Raytracer.temporal)
    assert callable(clrt.Raytracer.reset_history)


def test_header_declares_the_temporal_abi():
    with open(os.path.join(REPO, "include", "rt_hip.h")) as f:
        h = f.read()
    for needle in ("typedef struct rt_view {", "typedef struct rt_temporal_params {", "int rtEnqueueTemporalAccumulate(",
                   "gamma-encoded"):
        assert needle in h, needle
    with open(os.path.join(REPO, "include", "rt_cl_compat.hpp")) as f:
        assert "CLContext::TemporalAccumulate(" in f.read()
    # the kernel and the CPU sweep compile the same address logic
    with open(os.path.join(CSRC, "rt_temporal.hip")) as f:
        k = f.read()
    assert '#include "rt_temporal.hpp"' in k and "reproject(" in k and "tap_index(" in k

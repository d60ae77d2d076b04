"""CPU: the sample reprojection's host side -- the plan (csrc/rt_reproject_plan.cpp reproject_plan: argument checks
in their documented order, the temporal plan's constants and grid) and the texts the kernel compiles
(csrc/rt_temporal_math.hpp, csrc/rt_reproject_math.hpp), driven through the stand-alone
tests/native/reproject_samples_plan_main.cpp built with plain g++ and once more with sanitizers; the numpy
restatement tests/reproject_samples_ref.py against that program byte for byte and on cases whose answers are known;
and the Python surface of the entry point.  No GPU is touched.
"""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import reproject_samples_inputs as I
import reproject_samples_ref as ref
import temporal_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "mini-opencl-raytracer_amd", "csrc")
SOURCES = [os.path.join(REPO, "tests", "native", "reproject_samples_plan_main.cpp"),
           os.path.join(CSRC, "rt_reproject_plan.cpp"), os.path.join(CSRC, "rt_temporal_plan.cpp")]

F = np.float32
FEATURES = np.dtype([("albedo", np.float32, (3,)), ("depth", np.float32), ("normal", np.float32, (3,)),
                     ("coverage", np.float32)])
DEFAULT = ((0.0, -25.0, 8.5), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
AWAY = ((0.0, -25.0, 8.5), (0.0, -1.0, 0.0), (0.0, 0.0, 1.0))


def _build(out, *flags):
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", *flags, "-o", out,
                    *SOURCES], check=True, timeout=300)
    return out


@pytest.fixture(scope="module")
def plan_main(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("rplan") / "reproject_samples_plan_main"))


@pytest.fixture(scope="module")
def plan_san(tmp_path_factory):
    """The same stand-alone program with address, undefined-behaviour and float-cast-overflow checks (host code,
    nothing preloaded)."""
    return _build(str(tmp_path_factory.mktemp("rplan_san") / "reproject_samples_plan_san"), "-g",
                  "-fsanitize=address,undefined,float-cast-overflow", "-fno-sanitize-recover=all")


ROWS = ("valid", "params_null", "width_zero", "height_zero", "past_2_31", "product_near_2_64", "exactly_2_31",
        "camera_nan", "camera_infinite", "camera_front_infinite", "max_history_nan", "max_history_infinite",
        "max_history_zero", "max_history_below_one", "max_history_fraction", "max_history_negative", "max_history_huge",
        "max_history_one", "max_history_largest", "depth_tolerance_nan", "depth_tolerance_negative",
        "depth_tolerance_above_one", "depth_tolerance_zero", "normal_threshold_nan", "normal_threshold_below",
        "normal_threshold_above", "normal_threshold_lowest", "hist_stats_null", "hist_features_null",
        "cur_features_null", "out_null", "out_is_an_input", "hist_stats_short", "hist_features_short",
        "cur_features_short", "out_short", "value_before_mem_object", "last_value_before_mem_object",
        "size_zero_before_buffer_size", "mem_object_before_size", "foreign_before_size", "constants")


def _errors_ok(exe):
    p = subprocess.run([exe, "errors"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "FAILED" not in p.stdout, (p.stdout, p.stderr[-3000:])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    for row in ROWS:
        assert re.search(rf"ok     {row}\b", p.stdout), (row, p.stdout)


def test_error_rows_return_their_codes_in_order(plan_main):
    _errors_ok(plan_main)


def test_error_rows_run_clean_under_sanitizers(plan_san):
    _errors_ok(plan_san)


# ---- the program's bytes against the restatement's -----------------------------------------------
def _merge(exe, tmp_path, name, w, h, view, prm, hs, hf, cf):
    src, dst = tmp_path / f"{name}.in", tmp_path / f"{name}.out"
    src.write_bytes(I.pack(w, h, view, I.PREV, prm, hs, hf, cf))
    p = subprocess.run([exe, "merge", str(src), str(dst)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (name, p.stdout[-2000:], p.stderr[-3000:])
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    m = re.search(r"(\d+) carried, (\d+) statistics records fetched", p.stdout)
    return np.frombuffer(dst.read_bytes(), ref.STATS).reshape(h, w), int(m.group(1)), int(m.group(2))


def same_records(got, want, what):
    a = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 8)
    b = np.ascontiguousarray(want).view(np.uint32).reshape(-1, 8)
    bad = np.flatnonzero((a != b).any(axis=1))
    assert bad.size == 0, (f"{what}: {bad.size} of {len(a)} records differ, first {bad[:4]}: "
                           f"{np.ascontiguousarray(got).reshape(-1)[bad[:2]]} vs "
                           f"{np.ascontiguousarray(want).reshape(-1)[bad[:2]]}")


def test_inputs_are_not_trivial():
    """On the restatement alone, before anything is compared with it: statistics are carried and lost, taps are
    counted in part, every test rules some tap out, all three sample-count classes are merged, and each variant
    changes the answer."""
    w, h = 131, 77
    for pair in ("shift", "yaw"):
        out, info = I.reference(w, h, pair)
        covered = I.synthetic(w, h, pair)[2]["coverage"] > 0
        carried = int(info["carried"].sum())
        assert 0 < carried < int(covered.sum()), (pair, carried, int(covered.sum()))
        assert not info["carried"][~covered].any()
        assert ((info["counted"] >= 1) & (info["counted"] <= 3)).any() and (info["counted"] == 4).any()
        assert (out["n"][info["carried"]] >= 1).all() and (out["n"] == np.floor(out["n"])).all()
        assert (out["n"] == 1).any() and (out["n"] >= 2).any() and len(np.unique(out["n"])) > 4
        assert (out["m2_y"][out["n"] == 1] == 0).all() and (out["m2_y"][out["n"] >= 2] > 0).any()
        assert not out["reserved"].any() and out[~info["carried"]].tobytes() == bytes(32 * (w * h - carried))
    _, info = I.reference(w, h, "shift")
    for reason in ref.REASONS:
        assert info["rejected"][reason] > 0, (reason, info["rejected"])
    assert I.reference(w, h, "yaw")[1]["rejected"]["outside"] > 0
    hs = I.synthetic(w, h, "shift")[0]
    assert (hs["n"] == 0).any() and (hs["n"] == 1).any() and (hs["n"] >= 2).any()
    assert not I.reference(w, h, "away")[1]["carried"].any()
    base = I.reference(w, h, "shift")[0]
    for variant in I.VARIANTS:
        if variant != "defaults":
            assert I.reference(w, h, "shift", variant)[0].tobytes() != base.tobytes(), variant
    assert I.reference(w, h, "shift", "cap")[0]["n"].max() == 3.0 and base["n"].max() > 3.0


@pytest.mark.parametrize("pair", sorted(I.PAIRS))
def test_program_bytes_equal_the_restatement(plan_main, tmp_path, pair):
    for w, h in I.SIZES:
        hs, hf, cf, view = I.synthetic(w, h, pair)
        got, carried, _ = _merge(plan_main, tmp_path, f"{pair}_{w}x{h}", w, h, view, I.params("defaults"), hs, hf, cf)
        want, info = I.reference(w, h, pair)
        same_records(got, want, f"{w}x{h}, {pair}")
        assert carried == int(info["carried"].sum())


def test_program_bytes_equal_the_restatement_under_sanitizers(plan_san, tmp_path):
    """Every variant on the two moves that reach both outcomes, and the non-finite rows; the program fetches the
    statistics only of taps whose features passed, so fewer than four records per carried pixel."""
    w, h = 131, 77
    for pair in ("shift", "yaw"):
        for variant in I.VARIANTS:
            hs, hf, cf, view = I.synthetic(w, h, pair)
            got, carried, fetched = _merge(plan_san, tmp_path, f"{pair}_{variant}", w, h, view, I.params(variant), hs, hf, cf)
            want, info = I.reference(w, h, pair, variant)
            same_records(got, want, f"{pair}, {variant}")
            assert carried == int(info["carried"].sum()) and fetched == int(info["fetched"]) < 4 * w * h
            assert carried > 0 or variant == "depth_exact"      # (an exact depth match hardly survives a move)
    w, h, hs, hf, cf, view, dead, nan_n = I.non_finite_inputs()
    assert dead.any() and nan_n.any() and np.isnan(hs["n"][dead]).any()
    want, info = ref.reproject(hs, hf, cf, w, h, view, I.PREV, **I.DEFAULTS, details=True)
    assert info["carried"].any() and not info["carried"].all() and info["rejected"]["count"] > 0
    for name in ("sum", "n", "mean_y", "m2_y"):
        assert np.isfinite(want[name]).all(), name          # nothing non-finite came through the arithmetic
    got, _, _ = _merge(plan_san, tmp_path, "non_finite", w, h, view, I.DEFAULTS, hs, hf, cf)
    same_records(got, want, "non-finite depths, coverages and unused statistics")


# ---- the restatement on cases with known answers ------------------------------------------------
W, H = 13, 9


def _plane(depth=45.0, coverage=1.0):
    """Features of a wall straight ahead: depth along each centre ray to the plane y = pos.y + depth."""
    f = np.zeros((H, W), FEATURES)
    u = temporal_ref.centre_rays(W, H, DEFAULT[1], DEFAULT[2])
    f["depth"] = F(depth) / u[..., 1]
    f["albedo"], f["normal"], f["coverage"] = 0.5, (0.0, -1.0, 0.0), coverage
    return f


def _constant(sum_, n, mean_y, m2_y):
    st = np.zeros((H, W), ref.STATS)
    st["sum"], st["n"], st["mean_y"], st["m2_y"], st["reserved"] = sum_, n, mean_y, m2_y, 7
    return st


def _expect(out, at, sum_, n, mean_y, m2_y):
    want = np.zeros(1, ref.STATS)
    want["sum"], want["n"], want["mean_y"], want["m2_y"] = sum_, n, mean_y, m2_y
    assert at.any() and (out[at] == want[0]).all(), out[at][out[at] != want[0]][:3]


def test_same_view_over_a_plane_returns_the_statistics():
    """Every pixel holds the same statistics, whose means, per-sample variance and count are powers of two: every
    bw * value is an exact scaling, each sum is value * sw exactly whatever the weights round to, and the quotients
    return the values themselves."""
    f = _plane()
    hist = _constant((8.0, 1.0, 16.0), 4.0, 0.5, 6.0)       # m = (2, 0.25, 4), sv = 6 / 3 = 2
    out, info = ref.reproject(hist, f, f, W, H, DEFAULT, DEFAULT, details=True)
    assert out.dtype == ref.STATS and out.shape == (H, W) and info["carried"].all()
    assert (info["counted"][2:-2, 3:-3] == 4).all() and info["rejected"]["outside"] > 0
    _expect(out, info["carried"], (8.0, 1.0, 16.0), 4.0, 0.5, 6.0)
    assert not out["reserved"].any()
    # the cap below the history's n: n' is the cap and m2_y is rescaled to n' - 1
    out = ref.reproject(hist, f, f, W, H, DEFAULT, DEFAULT, max_history=2.0)
    _expect(out, np.ones((H, W), bool), (4.0, 0.5, 8.0), 2.0, 0.5, 2.0)
    out = ref.reproject(hist, f, f, W, H, DEFAULT, DEFAULT, max_history=1.0)
    _expect(out, np.ones((H, W), bool), (2.0, 0.25, 4.0), 1.0, 0.5, 0.0)


def test_single_samples_keep_their_mean_and_no_deviation():
    f = _plane()
    hist = _constant((2.0, 0.25, 4.0), 1.0, 0.5, 123.0)     # (m2_y of a single sample is not read)
    out = ref.reproject(hist, f, f, W, H, DEFAULT, DEFAULT)
    _expect(out, np.ones((H, W), bool), (2.0, 0.25, 4.0), 1.0, 0.5, 0.0)


def test_camera_facing_away_and_uncovered_pixels_carry_nothing():
    f = _plane()
    hist = _constant((8.0, 1.0, 16.0), 4.0, 0.5, 6.0)
    out, info = ref.reproject(hist, f, f, W, H, DEFAULT, AWAY, details=True)
    assert not info["carried"].any() and info["counted"].sum() == 0 and out.tobytes() == bytes(32 * W * H)
    cov = np.ones((H, W), np.float32)
    cov[4, 6], cov[0, 0], cov[8, 12] = 0.0, -1.0, np.nan
    out, info = ref.reproject(hist, f, _plane(coverage=cov), W, H, DEFAULT, DEFAULT, details=True)
    assert info["carried"].sum() == W * H - 3
    for y, x in ((4, 6), (0, 0), (8, 12)):
        assert out[y, x].tobytes() == bytes(32)


def test_tap_without_samples_is_left_out_and_the_others_renormalised():
    """The current camera half a pixel to the side, so that all four taps carry weight: a history pixel with n = 0
    (and values that would show) is left out of the pixels that tap it, which still return the constant."""
    f = _plane()
    asp = 13.0 / 9.0
    dx = 0.5 * (2.0 * float(temporal_ref.A) * asp * 45.0 / W)
    cur = ((dx, -25.0, 8.5), DEFAULT[1], DEFAULT[2])
    hist = _constant((8.0, 1.0, 16.0), 4.0, 0.5, 6.0)
    _, info0 = ref.reproject(hist, f, f, W, H, cur, DEFAULT, details=True)
    hist[4, 6] = ((1000.0, 1000.0, 1000.0), 0.0, 1000.0, 1000.0, (0, 0))
    out, info = ref.reproject(hist, f, f, W, H, cur, DEFAULT, details=True)
    assert info["rejected"]["count"] >= 2 and info0["rejected"]["count"] == 0
    three = (info0["counted"] == 4) & (info["counted"] == 3)
    assert three.any() and info["carried"][three].all()
    _expect(out, three, (8.0, 1.0, 16.0), 4.0, 0.5, 6.0)
    _expect(out, info["carried"], (8.0, 1.0, 16.0), 4.0, 0.5, 6.0)
    # uncovered and NaN-byte history records are selected away too, never multiplied by a zero weight
    hf = _plane()
    hf["coverage"][2, 3] = 0.0
    hist.view(np.uint8).reshape(H, W, 32)[2, 3] = 0xFF
    out, info = ref.reproject(hist, hf, f, W, H, cur, DEFAULT, details=True)
    assert info["rejected"]["coverage"] >= 1
    _expect(out, info["carried"], (8.0, 1.0, 16.0), 4.0, 0.5, 6.0)


def test_argument_checks_of_the_restatement():
    ok = dict(cur_view=DEFAULT, prev_view=DEFAULT, max_history=16.0, depth_tolerance=0.05, normal_threshold=0.9)
    assert ref.params_ok(**ok) and ref.params_ok(**{**ok, "max_history": 1.0}) and ref.params_ok(**{**ok, "max_history": 2.0 ** 20})
    for key, bad in (("max_history", 0.0), ("max_history", 0.5), ("max_history", 3.5), ("max_history", float("nan")),
                     ("max_history", float("inf")), ("max_history", 2.0 ** 20 + 1), ("depth_tolerance", -0.1),
                     ("depth_tolerance", 1.5), ("normal_threshold", -1.5), ("normal_threshold", float("nan")),
                     ("cur_view", ((0.0, float("nan"), 0.0), (0, 1, 0), (0, 0, 1))),
                     ("prev_view", ((0.0, 0.0, 0.0), (0, float("inf"), 0), (0, 0, 1)))):
        assert not ref.params_ok(**{**ok, key: bad}), (key, bad)
    with pytest.raises(ValueError):
        ref.reproject(_constant(0, 0, 0, 0), _plane(), _plane(), W, H, DEFAULT, DEFAULT, max_history=2.5)


# ---- the Python surface ---------------------------------------------------------------------------
def test_native_declares_the_entry_point():
    import clrt
    from clrt import _native as N
    assert "rtEnqueueReprojectSamples" in N.HIP_EXPORTS
    assert ctypes.sizeof(N.REPROJECT_PARAMS) == 84
    assert [f[0] for f in N.REPROJECT_PARAMS._fields_] == ["cur", "prev", "max_history", "depth_tolerance",
                                                            "normal_threshold"]
    assert N.PIXEL_STATS_DTYPE == ref.STATS
    lib = clrt.hip_lib()  # (loading the library does not touch the GPU)
    assert len(lib.rtEnqueueReprojectSamples.argtypes) == 9
    assert lib.rtEnqueueReprojectSamples.argtypes[7] == ctypes.POINTER(N.REPROJECT_PARAMS)


def test_reproject_samples_marshals_its_arguments():
    """CLContext.ReprojectSamples on a context whose library is a recorder: the handles in the C order, the sizes,
    and the parameter block field by field."""
    import clrt
    from clrt import _native as N
    calls = []

    class Lib:
        @staticmethod
        def rtEnqueueReprojectSamples(*args):
            p = ctypes.cast(args[7], ctypes.POINTER(N.REPROJECT_PARAMS)).contents
            calls.append((args[:7], args[8], [list(p.cur.pos), list(p.cur.front), list(p.cur.up)],
                          [list(p.prev.pos), list(p.prev.front), list(p.prev.up)],
                          (p.max_history, p.depth_tolerance, p.normal_threshold)))
            return Lib.rc

    class Handle:
        def __init__(self, handle):
            self.handle = handle

    ctx = clrt.CLContext.__new__(clrt.CLContext)
    ctx._lib, ctx.handle = Lib, 11
    cur = ((1.0, 2.0, 3.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0))
    prev = ((4.0, 5.0, 6.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0))
    Lib.rc = 0
    ctx.ReprojectSamples(Handle(22), Handle(33), Handle(44), Handle(55), 131, 77, Handle(66), cur, prev, 8, 0.25, -0.5)
    assert calls == [((11, 22, 33, 44, 55, 131, 77), 66, [list(v) for v in cur], [list(v) for v in prev],
                      (8.0, 0.25, -0.5))]
    ctx.ReprojectSamples(Handle(22), Handle(33), Handle(44), Handle(55), 5, 3, Handle(66), cur, prev)
    assert calls[1][4] == (16.0, F(0.05), F(0.9))
    Lib.rc = -30
    with pytest.raises(clrt.RTError) as e:
        ctx.ReprojectSamples(Handle(22), Handle(33), Handle(44), Handle(55), 5, 3, Handle(66), cur, prev)
    assert e.value.code == -30


def test_raytracer_declares_reproject_samples():
    import clrt
    sig = inspect.signature(clrt.Raytracer.reproject_samples)
    assert list(sig.parameters) == ["self", "prev", "n_frames", "max_history", "depth_tolerance", "normal_threshold"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [4, 16.0, 0.05, 0.9]
    assert sig.parameters["prev"].default is inspect.Parameter.empty
    for method in (clrt.Raytracer.reproject_samples, clrt.Raytracer.reset_samples):
        assert "move_vertices()" in method.__doc__ and "camera's motion only" in method.__doc__
    assert list(inspect.signature(clrt.Raytracer.reset_samples).parameters) == ["self"]


def test_header_and_sources_share_the_definition():
    with open(os.path.join(REPO, "include", "rt_hip.h")) as f:
        h = f.read()
    for needle in ("typedef struct rt_reproject_params {", "int rtEnqueueReprojectSamples(",
                   "sv = s.n >= 2.0f ? s.m2_y / (s.n - 1.0f) : s.mean_y * s.mean_y",
                   "n'         = fminf(floorf(sn / sw), max_history)"):
        assert needle in h, needle
    m = re.search(r"int rtEnqueueReprojectSamples\(([^;]*)\);", h)
    assert len(m.group(1).split(",")) == 9
    # the kernel and the CPU program compile the same projection, tap indices and merge
    with open(os.path.join(CSRC, "rt_reproject.hip")) as f:
        k = f.read()
    with open(SOURCES[0]) as f:
        prog = f.read()
    for text in (k, prog):
        for call in ("rtt::reproject(", "rtt::tap_index(", "rtt::tap_weight(", "tap_on_surface(", "add_tap(", "merge("):
            assert call in text, call
    with open(os.path.join(CSRC, "rt_reproject_math.hpp")) as f:
        m = f.read()
    assert '#include "rt_temporal_math.hpp"' in m and "floorf(" in m and "[q" not in m
    assert not re.search(r"\((u?int(\d+_t)?|size_t|unsigned|long)\)", m)    # no float becomes an integer there

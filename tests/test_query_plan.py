"""CPU: the ray-query plan (csrc/rt_query_plan.cpp) -- the range checks, the scene path and how the
rays are handed out in 64-ray units -- as a pure function, driven through the stand-alone
tests/native/query_plan_main.cpp built with plain g++; and the Python surface of the two entry
points (no GPU is touched).
"""
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "mini-opencl-raytracer_amd", "csrc")
SOURCES = [os.path.join(REPO, "tests", "native", "query_plan_main.cpp"), os.path.join(CSRC, "rt_query_plan.cpp")]


def _build(out, *flags):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-o", out, *SOURCES],
                   check=True, timeout=300)
    return out


@pytest.fixture(scope="module")
def plan_main(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("qplan") / "query_plan_main"))


def test_units_cover_every_ray_over_a_sweep(plan_main):
    p = subprocess.run([plan_main, "sweep"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and " 0 failures" in p.stdout, p.stdout[-3000:]
    m = re.search(r"(\d+) accepted \((\d+) LDS, (\d+) HBM/L2\)", p.stdout)
    assert m and int(m.group(2)) > 0 and int(m.group(3)) > 0, p.stdout


def test_error_rows_return_their_codes(plan_main):
    p = subprocess.run([plan_main, "errors"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "FAILED" not in p.stdout, p.stdout
    for row in ("n_rays_zero", "mode_2", "rays_buffer_short", "hits_buffer_short", "past_2_31", "sum_wraps",
                "same_buffer", "leaf_too_large"):
        assert f"ok     {row}:" in p.stdout, (row, p.stdout)


def test_plan_runs_clean_under_sanitizers(tmp_path):
    """The same stand-alone program with -fsanitize=address,undefined (host code, no preload)."""
    exe = _build(str(tmp_path / "query_plan_san"), "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    for arg in ("sweep", "errors"):
        p = subprocess.run([exe, arg], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (arg, p.stdout[-2000:], p.stderr[-3000:])
        assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]


def test_plan_unit_is_free_of_hip():
    for name in ("rt_query_plan.cpp", "rt_query_plan.hpp"):
        with open(os.path.join(CSRC, name)) as f:
            assert "#include <hip" not in f.read(), name


def test_native_declares_the_entry_points():
    import clrt
    from clrt import _native as N
    assert N.RAY_DTYPE.itemsize == 32 and N.RAY_HIT_DTYPE.itemsize == 16
    assert N.RAY_DTYPE.fields["tmin"][1] == 12 and N.RAY_DTYPE.fields["dir"][1] == 16 and N.RAY_DTYPE.fields["tmax"][1] == 28
    assert [N.RAY_HIT_DTYPE.fields[f][1] for f in ("prim", "t", "u", "v")] == [0, 4, 8, 12]
    assert (N.QUERY_CLOSEST, N.QUERY_ANY) == (0, 1)
    assert {"rtEnqueueIntersectRays", "rtEnqueueCameraRays"} <= set(N.HIP_EXPORTS)
    lib = clrt.hip_lib()  # (loading the library does not touch the GPU)
    assert len(lib.rtEnqueueIntersectRays.argtypes) == 7 and len(lib.rtEnqueueCameraRays.argtypes) == 4
    assert N.TUNING["query_refill_min"] == 26
    assert callable(clrt.CLContext.IntersectRays) and callable(clrt.CLContext.CameraRays)
    assert callable(clrt.Raytracer.cast)
    r = np.zeros(2, N.RAY_DTYPE)
    assert r["origin"].shape == (2, 3) and r["dir"].shape == (2, 3)


def test_header_declares_the_query_abi():
    with open(os.path.join(REPO, "include", "rt_hip.h")) as f:
        h = f.read()
    for needle in ("typedef struct rt_ray {", "typedef struct rt_ray_hit {", "#define RT_QUERY_CLOSEST 0",
                   "#define RT_QUERY_ANY 1", "int rtEnqueueIntersectRays(", "int rtEnqueueCameraRays(",
                   "RT_TUNE_QUERY_REFILL_MIN = 26"):
        assert needle in h, needle
    # earlier enumerators keep their numbers
    assert "RT_TUNE_STEP_WEIGHT_LEAF_GLOBAL = 25" in h and "RT_TUNE_PERFRAME_BATCH = 23" in h

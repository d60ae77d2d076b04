"""CPU: rtEnqueueSamplePixels' host side -- sample_check's error rows in their documented order and sample_plan's
units and grid (csrc/rt_adaptive_plan.{hpp,cpp} over csrc/rt_trace_plan.cpp), driven through the stand-alone
tests/native/sample_plan_main.cpp built with plain g++ and once more with sanitizers, as test_adaptive_plan.py
builds its program; and the Python and header surface of the entry point.  No GPU is touched.
"""
import inspect
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "mini-opencl-raytracer_amd", "csrc")
SOURCES = [os.path.join(REPO, "tests", "native", "sample_plan_main.cpp"), os.path.join(CSRC, "rt_adaptive_plan.cpp"),
           os.path.join(CSRC, "rt_trace_plan.cpp")]

# the error list of rt_hip.h, in its order
ROWS = ("range_past_2_31", "n_pixels_zero", "n_pixels_past_2_31", "ids_not_of_context", "stats_not_of_context",
        "count_not_of_context", "aliased", "ids_short", "count_short", "stats_short", "camera_slot_unset", "width_zero",
        "height_zero", "scene_unbound", "lights_unset", "leaf_too_large")
EXTRA = ("valid", "valid_without_count", "range_exactly_2_31", "range_wraps", "n_pixels_exactly_2_31", "n_zero",
         "n_zero_at_the_end_of_ids")


def _build(out, *flags):
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wextra", "-Werror", *flags, "-o", out,
                    *SOURCES], check=True, timeout=300)
    return out


@pytest.fixture(scope="module")
def plan_main(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("splan") / "sample_plan_main"))


def _rows_ok(stdout):
    assert "FAILED" not in stdout, stdout
    names = list(EXTRA) + list(ROWS) + [f"{r}_before_n_zero" for r in ROWS]
    names += [f"{a}_before_{b}" for i, a in enumerate(ROWS) for b in ROWS[i + 1:]]     # each pair, the earlier one wins
    for name in names:
        assert re.search(rf"ok     {name}:", stdout), (name, stdout)
    assert len(names) == 7 + 16 + 16 + 120


def test_error_rows_return_their_codes_and_the_earlier_row_wins(plan_main):
    p = subprocess.run([plan_main, "errors"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout
    _rows_ok(p.stdout)


def _sweep_ok(stdout):
    m = re.search(r"sweep: (\d+) plans, (\d+) launched \((\d+) LDS, (\d+) HBM/L2\), (\d+) device counts, 0 failures", stdout)
    assert m, stdout[-3000:]
    plans, launched, lds, glob, counts = map(int, m.groups())
    # four offsets x six counts (n = 0 launches nothing) x four scenes x forced or not x eight occupancies
    assert plans == 4 * 6 * 4 * 2 * 8 and launched == plans * 5 // 6 and lds > 0 and glob > 0
    assert counts == launched * 2 * 13


def test_units_and_grid_hold_for_every_count(plan_main):
    p = subprocess.run([plan_main, "sweep"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-3000:]
    _sweep_ok(p.stdout)


def test_the_plan_runs_clean_under_sanitizers(tmp_path):
    """The same stand-alone program with address, undefined-behaviour and float-cast-overflow checks (host code, no
    preload)."""
    exe = _build(str(tmp_path / "sample_plan_san"), "-g", "-fsanitize=address,undefined,float-cast-overflow",
                 "-fno-sanitize-recover=all")
    for arg in ("sweep", "errors"):
        p = subprocess.run([exe, arg], capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (arg, p.stdout[-2000:], p.stderr[-3000:])
        assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
        (_sweep_ok if arg == "sweep" else _rows_ok)(p.stdout)


# ---- the surface -----------------------------------------------------------------------------------

def test_native_declares_the_entry_point():
    import clrt
    from clrt import _native as N
    assert "rtEnqueueSamplePixels" in N.HIP_EXPORTS
    assert len(clrt.hip_lib().rtEnqueueSamplePixels.argtypes) == 8   # (loading the library does not touch the GPU)
    sig = inspect.signature(clrt.CLContext.SamplePixels)
    assert list(sig.parameters) == ["self", "kernel", "ids", "n", "n_pixels", "stats", "count", "first"]
    assert sig.parameters["count"].default is None and sig.parameters["first"].default == 0
    sig = inspect.signature(clrt.Raytracer.render_adaptive)
    assert sig.parameters["fused"].default is False and sig.parameters["sync_every"].default == 1


def test_header_wrapper_and_kernel_text():
    with open(os.path.join(REPO, "include", "rt_hip.h")) as f:
        h = f.read()
    assert "int rtEnqueueSamplePixels(rt_context ctx, rt_kernel k, rt_mem ids, rt_mem count /* may be NULL */" in h
    with open(os.path.join(REPO, "include", "rt_cl_compat.hpp")) as f:
        assert "CLContext::SamplePixels(" in f.read()
    # the kernel compiles the per-pixel text of the accumulate, tests a gid before it indexes anything, and takes
    # its division from outside the translation unit's flags
    with open(os.path.join(CSRC, "rt_sample.hpp")) as f:
        k = f.read()
    for needle in ('#include "rt_adaptive_math.hpp"', "#pragma clang fp contract(off)", "rta::pixel_in_range(",
                   "rta::finite_sample(", "rta::luminance(", "rta::sample_update(", "IeeeDiv{}", "trace_loop<"):
        assert needle in k, needle
    assert k.index("rta::pixel_in_range(") < k.index("q.stats + 2 *")
    assert " / " not in re.sub(r"//.*", "", k.split("struct SampleEnds")[1].split("void update")[1])   # no plain division

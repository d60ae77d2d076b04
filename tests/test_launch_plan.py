"""CPU: the launch plan (csrc/rt_launch_plan.cpp) -- how a launch's work is handed out -- as a pure
function, driven through the stand-alone tests/native/plan_main.cpp built with plain g++.

* tests/golden/launch_plans.json holds what the library planned on an MI355X *before* the plan was
  split out of rt_capi.cpp's enqueue (one row per launch: every input, the occupancies the runtime
  gave, every planned value; error and nothing-to-do rows included).  The plan must reproduce every
  row exactly.  After a deliberate rule change, `plan_main plan` fed the rows' inputs regenerates it.
* The hand-out invariants (plan_main.cpp, broken()) hold on every golden row -- so the recorded rule
  satisfies them -- and over a sweep of sizes, frame counts, bands, scene paths and occupancies.
* The A/B switches (-DRT_COUNTER_PARTS=..., as scripts/build_variant.sh passes them) reach the unit.
"""
import json
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "mini-opencl-raytracer_amd", "csrc")
GOLDEN = os.path.join(REPO, "tests", "golden", "launch_plans.json")


def _build(out, *defines):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *defines, "-o", out,
                    os.path.join(REPO, "tests", "native", "plan_main.cpp"), os.path.join(CSRC, "rt_launch_plan.cpp")],
                   check=True, timeout=300)
    return out


def _plan(exe, rows):
    text = "".join(" ".join(f"{k}={int(v)}" for k, v in {**r["in"], "occ": r.get("occ", 0),
                                                        "occ_s": r.get("occ_s", 0)}.items()) + "\n" for r in rows)
    p = subprocess.run([exe, "plan"], input=text, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    got = [json.loads(line) for line in p.stdout.splitlines()]
    assert len(got) == len(rows)
    return got


@pytest.fixture(scope="module")
def plan_main(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("plan") / "plan_main"))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def planned(plan_main, golden):
    return _plan(plan_main, golden)


def test_plans_equal_the_recorded_ones(golden, planned):
    bad = []
    for want, got in zip(golden, planned):
        if got["rc"] != want["rc"] or got["nothing"] != want["nothing"]:
            bad.append((want["case"], "rc/nothing", (want["rc"], want["nothing"]), (got["rc"], got["nothing"])))
            continue
        if "out" not in want:
            assert "out" not in got
            continue
        assert set(got["out"]) == set(want["out"]), want["case"]
        bad += [(want["case"], k, v, got["out"][k]) for k, v in want["out"].items() if got["out"][k] != v]
    assert not bad, f"{len(bad)} planned values differ from the recorded ones (case, field, want, got): {bad[:10]}"


def test_recorded_plans_satisfy_the_invariants(golden, planned):
    # (the plans equal the recorded ones, above: this is the recorded rule against the invariants)
    broken = [(w["case"], g["inv"]) for w, g in zip(golden, planned) if "out" in g and g["inv"]]
    assert not broken, broken[:10]


def test_recorded_plans_reach_every_branch(golden):
    outs = [r["out"] for r in golden if "out" in r]
    assert {r["rc"] for r in golden} >= {0, -63, -59}  # INVALID_GLOBAL_WORK_SIZE, INVALID_OPERATION
    assert any(r["nothing"] for r in golden)
    assert {o["si"] for o in outs} == {0, 2, 4}
    assert any(o["lds"] for o in outs) and any(o["goct"] and o["regrouped"] for o in outs)
    assert any(not o["lds"] and not o["goct"] and o["nTop"] > 0 for o in outs)
    assert {o["tileMajor"] for o in outs} == {0, 1, 2} and {o["flagTiles"] for o in outs} == {0, 1, 2}
    assert {o["nParts"] for o in outs} == {0, 8} and {o["tailChunk"] for o in outs} >= {64, 128, 256}
    assert any(o["chunkSplit"] > 0 for o in outs) and any(o["staticFirst"] and not o["nParts"] for o in outs)
    assert any(o["bandPeriod"] > 1 for o in outs) and any(o["gidBegin"] > 0 for o in outs)
    assert any(o["wf"] and o["G"] < o["nBlocks"] for o in outs) and any(o["own_stream"] for o in outs)


def test_handout_invariants_over_a_sweep(plan_main):
    p = subprocess.run([plan_main, "sweep"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and " 0 failures" in p.stdout, p.stdout[-3000:]


def test_ab_switches_reach_the_plan(tmp_path, golden, planned):
    """-DRT_COUNTER_PARTS=1 -DRT_TAIL_SHARE_WAVES=1: no partitions, and the tail chunk sized per wave."""
    exe = _build(str(tmp_path / "plan_variant"), "-DRT_COUNTER_PARTS=1", "-DRT_TAIL_SHARE_WAVES=1")
    assert subprocess.run([exe, "parts"], capture_output=True, text=True).stdout.strip() == "1"
    rows = [r for r, g in zip(golden, planned) if "out" in g and g["out"]["nParts"] == 8]
    base = [g for g in planned if "out" in g and g["out"]["nParts"] == 8]
    assert rows
    got = _plan(exe, rows)
    assert all(g["out"]["nParts"] == 0 and g["out"]["partLen"] == 0 and not g["inv"] for g in got)
    # without partitions the share rule was per workgroup (x4); per wave it picks a smaller chunk somewhere
    fused = [r for r in golden if "out" in r and r["in"]["fused"]]
    assert any(a["out"]["tailChunk"] < b["out"]["tailChunk"] for a, b in zip(_plan(exe, fused), fused))
    assert all(a["out"]["tailChunk"] <= b["out"]["tailChunk"] for a, b in zip(got, base))


def test_units_are_free_of_hip():
    for name in ("rt_launch_plan.cpp", "rt_launch_plan.hpp", "rt_scene_pack.cpp", "rt_scene_pack.hpp", "rt_layout.hpp"):
        with open(os.path.join(CSRC, name)) as f:
            assert "#include <hip" not in f.read(), name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                    os.path.join(CSRC, "rt_scene_pack.cpp")], check=True, timeout=300)

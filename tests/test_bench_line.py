"""GPU: the default bench line (what the driver records each round) carries the headline plus the
other BASELINE configs -- config 5 (bunny-class proxy), config 2 (1080p, 2 bounces) and config 3 in
the CPU-parity math -- each with its own timing and roofline, and the headline's roofline prices
the overlapped accumulation beside the render (bench.py, EXTRA_CONFIGS)."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_default_bench_line_carries_every_config():
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "2", "--warmup", "1",
                        "--full", "--no-cpu-baseline", "--no-drop-in"], capture_output=True, text=True, timeout=240, cwd=REPO)
    assert p.returncode == 0, p.stderr[-2000:]
    line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 1 and line["value"] > 0
    assert set(line["roofline"]) >= {"accum_valu_insts_per_launch", "frac_with_accum", "lane_util"}
    cfg = line["configs"]
    assert set(cfg) == {"cfg5_bunny", "cfg2_1080p", "cfg3_pinned"}
    for name, c in cfg.items():
        assert c["ms_per_frame"] > 0 and c["value"] > 0 and c["rays_per_step"] > 0, name
        assert c["roofline"]["bound"] == "valu" and c["roofline"]["launch_ms"] > 0, name
    assert cfg["cfg5_bunny"]["workload"].startswith("bunny 3840x2160 8spp 9-bounce")
    assert cfg["cfg2_1080p"]["workload"] == "cornell 1920x1080 1spp 2-bounce path trace"
    assert cfg["cfg3_pinned"]["math"] == "pinned"
    # pinned and shipped render the same paths: Intersect() counts differ only where the maths
    # flip a hit (SURVEY.md 7 hard part 1), by far less than a percent
    rel = abs(cfg["cfg3_pinned"]["rays_per_step"] - line["config"]["rays_per_step"]) / line["config"]["rays_per_step"]
    assert rel < 1e-3


SMALL = ["--width", "640", "--height", "360"]


def _bench(*extra):
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        *extra], capture_output=True, text=True, timeout=120, cwd=REPO)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_what_the_timed_path_computed(tmp_path, cornell):
    """A plain run carries the headline and its roofline only (what takes runs of its own waits for
    --full); --dump-outputs writes the image the last timed step left, the same bits in every run
    and the same bits a caller of that path reads back."""
    import numpy as np

    import bench
    line = _bench(*SMALL, "--dump-outputs", str(tmp_path / "a"))
    assert not {"drop_in", "configs", "cpu_baseline"} & set(line)
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["value"] > 0 and line["unit"] == "Mrays/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["metric"].startswith("Mrays/s (640x360 Cornell box")
    assert line["ms_per_step"] > 0 and line["roofline"]["launch_ms"] > 0
    # value = rays per step / time per step; ms_per_step is printed to 1e-4 ms and a step here takes > 0.02 ms
    assert line["value"] == pytest.approx(line["config"]["rays_per_step"] / line["ms_per_step"] / 1e3, rel=5e-3)
    _bench(*SMALL, "--dump-outputs", str(tmp_path / "b"))
    assert os.listdir(tmp_path / "a") == ["radiance.npy"]
    a = np.load(tmp_path / "a" / "radiance.npy")
    b = np.load(tmp_path / "b" / "radiance.npy")
    assert a.dtype == np.float32 and a.shape == (640 * 360, 3)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    args = bench.parse(SMALL)
    r = bench.Rank(cornell, args, 0)
    r.render()
    want = np.empty((640 * 360, 4), np.float32)
    r.ctx.ReadBuffer(r.out, want, blocking=True)
    r.release()
    assert np.isfinite(want).all() and (want[:, :3] > 0).any()
    assert np.array_equal(a.view(np.uint32), np.ascontiguousarray(want[:, :3]).view(np.uint32))


def test_dump_outputs_samples_a_large_image(tmp_path, monkeypatch):
    """CPU: an image over the dump's size limit is written as a fixed, seeded choice of its pixels
    in ascending order -- the same pixels every time."""
    import numpy as np

    import bench
    n = 5000
    img = np.arange(n * 4, dtype=np.float32).reshape(n, 4)

    class Ctx:
        def ReadBuffer(self, buf, host, blocking=True):
            host[:] = buf

    monkeypatch.setattr(bench, "DUMP_MAX_PIXELS", 1000)
    bench.dump_outputs(Ctx(), img, n, str(tmp_path / "a"))
    bench.dump_outputs(Ctx(), img, n, str(tmp_path / "b"))
    a = np.load(tmp_path / "a" / "radiance.npy")
    assert a.dtype == np.float32 and a.shape == (1000, 3)
    assert np.array_equal(a, np.load(tmp_path / "b" / "radiance.npy"))
    px = (a[:, 0] / 4).astype(np.int64)
    assert np.all(np.diff(px) > 0) and np.array_equal(a, img[px, :3])
    monkeypatch.setattr(bench, "DUMP_MAX_PIXELS", n)
    bench.dump_outputs(Ctx(), img, n, str(tmp_path / "c"))
    assert np.array_equal(np.load(tmp_path / "c" / "radiance.npy"), img[:, :3])


def test_every_bench_config_has_a_pmc_record():
    """CPU: the headline and every extra config of the default bench line are priced by a
    profiles/pmc.json record (scripts/profile.sh); `stale` in the line says whether the record was
    measured on the current kernel sources."""
    import bench
    db = json.load(open(os.path.join(REPO, "profiles", "pmc.json")))
    base = bench.parse([])
    keys = [bench.workload_key(base, 1, base.frames)]
    for _, over, _, _ in bench.EXTRA_CONFIGS:
        a = bench.parse([])
        a.__dict__.update(over)
        keys.append(bench.workload_key(a, 1, a.frames if a.frames > 1 else 1))
    missing = [k for k in keys if k not in db]
    assert not missing, f"no PMC record for {missing} (run scripts/profile.sh)"
    assert len(set(keys)) == len(keys)

"""CPU: the stress fixtures (stress_scenes.py) are legal inputs, the oracle is a sound checker on
them, and they reach what they are meant to reach.

For every fixture test_stress_gpu.py renders:
  * the reference kernel built for x86-64 (oracle/_ref/libref_cpu.so) equals the C oracle bit
    for bit, so the oracle speaks for the reference in these regimes too;
  * rtp::check_nodes (rtValidateBVH) accepts every hand-built tree, garbage tail included;
  * coverage conditions on the oracle's own output keep the GPU comparisons from being vacuous:
    they are conditions on the inputs (seeds are chosen so that they hold), not tolerances.
"""
import numpy as np
import pytest

import refcpu
import stress_scenes as SS
from clrt import _native as N

needs_refcpu = pytest.mark.skipif(not refcpu.available(),
                                  reason="needs oracle/_ref/libref_cpu.so or /root/reference")


def _bits(a):
    return np.ascontiguousarray(a[:, :3]).view(np.uint32)


@pytest.fixture(scope="module")
def sweeps(cornell):
    return SS.material_sweeps(cornell)


def _ref_equals_oracle(oracle, scene, W, H, camera, light_type, bounces, frames, key):
    want = SS.oracle_run(oracle, key, scene, W, H, camera, light_type, bounces, frames)[0]
    a = np.zeros((W * H, 4), np.float32)
    for f in frames:
        refcpu.render(scene, W, H, frame_count=f, light_bounces=bounces, light_type=light_type, camera=camera,
                      result=a, threads=16)
    nd = (_bits(a) != _bits(want)).any(axis=1).sum()
    assert nd == 0, f"{key}: {nd} pixels differ between the x86-64 reference and the oracle"


# ---- static conditions ----------------------------------------------------------------------
def test_sweep_contains_every_alpha_regime():
    seen = {SS.alpha_regime(v) for v in SS.SWEEP_VALUES}
    assert seen == set(SS.REGIMES), seen
    # alpha == -1 exactly (1/(alpha + 1) = inf) is out of fp32's reach: no fp32 r has r * r == 2
    # (the squares of sqrt(2)'s neighbours step over it) and 2 / x == 1 needs x == 2.  The sweep
    # holds the two values next to the pole instead: 1/(alpha + 1) = +2^23 and -2^23.
    r = SS.SQRT2
    for k in range(-8, 9):
        x = r
        for _ in range(abs(k)):
            x = np.nextafter(x, np.float32(2 if k > 0 else 1))
        assert np.float32(x * x) != np.float32(2.0) and SS.alpha32(x) != np.float32(-1.0)
    up = np.nextafter(r, np.float32(2))
    assert np.float32(1) / (SS.alpha32(r) + np.float32(1)) == np.float32(2.0 ** 23)
    assert np.float32(1) / (SS.alpha32(up) + np.float32(1)) == np.float32(-(2.0 ** 23))
    assert float(r) in SS.SWEEP_VALUES and float(up) in SS.SWEEP_VALUES
    # the exponent of pow(r, 1/(alpha+1)) lies strictly inside (0, 1) for some value
    with np.errstate(all="ignore"):
        e = [np.float32(1.0) / (SS.alpha32(v) + np.float32(1.0)) for v in SS.SWEEP_VALUES]
    assert any(0.0 < x < 1.0 for x in e)
    assert {SS.alpha_regime(v) for v in SS.MIXED_ROUGHNESS} >= {"+inf", "finite>0", "(-1,0)"}


def test_sweep_materials(cornell, sweeps):
    assert len(sweeps) == len(SS.SWEEP_VALUES) + 1
    assert {SS.sweep_light_type(i) for i in range(len(sweeps))} == {0, 1, 2}
    for name, sc in sweeps.items():
        assert sc.triangles is cornell.triangles and sc.nodes is cornell.nodes
        if name != "mixed":
            assert (sc.materials["specular"][:, :3] == 0.5).all()
            assert len({x.tobytes() for x in sc.materials["roughness"]}) == 1
    m = sweeps["mixed"].materials
    assert (m["specular"][:, :3] > 0.5).any() and (m["specular"][:, :3] != m["specular"][:, :1]).any()
    assert (m["emission"][:, :3] > 0).any(axis=1).sum() >= 2
    assert (cornell.materials["emission"][:, :3] > 0).any(axis=1).sum() + 1 == (m["emission"][:, :3] > 0).any(axis=1).sum()


def test_negative_zeros_survive_set_float3():
    """The cameras' -0.0 components reach rtSetKernelArg with their sign bit (and +0 stays +0)."""
    assert len(SS.CAMERAS) >= 9
    for name, cam in SS.CAMERAS.items():
        got = SS.packed_camera_bits(cam)
        want = [np.float32(list(v) + [0.0]).view(np.uint32) for v in cam]
        for g, w in zip(got, want):
            assert np.array_equal(g, w), name
    front = SS.packed_camera_bits(SS.CAMERAS["up0_negzero"])[1]
    assert front[0] == 0x80000000 and front[2] == 0x80000000
    front = SS.packed_camera_bits(SS.CAMERAS["axis_negz"])[1]
    assert front[0] == 0x80000000 and front[1] == 0x80000000
    assert (SS.packed_camera_bits(SS.CAMERAS["up0"])[1][[0, 2]] == 0).all()


def test_soup_defects():
    for seed in SS.SOUP_SEEDS:
        t, m = SS.soup(seed)
        p = [t[v]["position"][:, :3] for v in ("v1", "v2", "v3")]
        assert (p[1] == p[2]).all(axis=1).sum() >= 8                     # zero area
        raw = t.view(np.uint8).reshape(t.shape[0], -1)
        assert t.shape[0] - len({r.tobytes() for r in raw}) >= 8         # exact duplicates
        nn = np.linalg.norm(t["v1"]["normal"][:, :3].astype(np.float64), axis=1)
        assert (nn == 0).any() and (nn > 20).any() and ((nn > 0) & (nn < 1e-2)).any() and ((nn > 0.2) & (nn < 5)).any()
        assert m.shape[0] == 12 and (m["specular"][:, :3] > 1.0).any()
        assert (m["emission"][::4, :3] > 0).all() and (m["emission"][1::4, :3] == 0).all()
        assert {SS.alpha_regime(v) for v in m["roughness"]} == set(SS.REGIMES) - {"nan"}
        assert len(np.unique(t["mtlIndex"])) == 12
        assert np.isfinite(np.stack(p)).all()
        t2, _ = SS.soup(seed, nonfinite=True)
        q = np.stack([t2[v]["position"][:, :3] for v in ("v1", "v2", "v3")])
        assert np.isnan(q).sum() == 1 and np.isposinf(q).sum() == 1 and (np.abs(q[np.isfinite(q)]) > 1e29).sum() >= 3


# ---- the trees ---------------------------------------------------------------------------------
def _hand_built():
    return [(c, SS.soup_scene(*c)) for c in SS.soup_cases() if SS.SOUP_TREES[c[1]][0] != "sah"]


def test_check_nodes_accepts_hand_built_trees():
    for case, sc in _hand_built() + [(("nf", "rt7"), SS.soup_scene(SS.SOUP_SEEDS[0], "rt7", nonfinite=True))]:
        depth, end = SS.tree_depth(sc.nodes)
        assert end == sc.nodes.shape[0] - 5, case                        # the garbage tail
        assert (sc.nodes["offset"][end:] == 0xDEADBEEF).all()
        assert N.validate_bvh(sc.nodes, sc.n_triangles) == depth, case
        assert depth <= 60, case                                         # the reference's stack holds 64


def test_hand_built_tree_coverage():
    trees = _hand_built()
    leaf_max = max(int(sc.nodes["nPrimitives"][:SS.tree_depth(sc.nodes)[1]].max()) for c, sc in trees if c[1] == "rt127")
    assert 64 <= leaf_max <= 127, leaf_max
    assert max(SS.tree_depth(sc.nodes)[0] for c, sc in trees if c[1] == "chain") >= 55
    for c, sc in trees:
        n = SS.tree_depth(sc.nodes)[1]
        inner = sc.nodes[:n][sc.nodes["nPrimitives"][:n] == 0]
        if c[1] != "rt127":  # (a tree of large leaves may have only a few interior nodes)
            assert set(np.unique(inner["axis"])) == {0, 1, 2}, c
        if c[1] == "big":
            assert sc.nodes["nPrimitives"][:n].max() > 127
        if c[1] in ("rt1", "chain"):
            assert sc.nodes["nPrimitives"][:n].max() == 1
    sizes = set()
    for c, sc in trees:
        if c[1] in ("rt7", "rt127"):
            sizes |= set(sc.nodes["nPrimitives"][:SS.tree_depth(sc.nodes)[1]].tolist())
    assert len(sizes - {0}) >= 10, sizes                                 # leaves of mixed sizes


# ---- reference == oracle, and what the renders reach ------------------------------------------
@needs_refcpu
def test_sweeps_reference_cpu_equals_oracle(oracle_mod, sweeps):
    R = SS.SWEEP_RUN
    for i, (name, sc) in enumerate(sweeps.items()):
        _ref_equals_oracle(oracle_mod, sc, R["W"], R["H"], SS.DEFAULT, SS.sweep_light_type(i), R["bounces"],
                           R["frames"], ("sweep", name))


def test_sweeps_coverage(oracle_mod, sweeps):
    R = SS.SWEEP_RUN
    n = R["W"] * R["H"]
    for i, (name, sc) in enumerate(sweeps.items()):
        res, ids, t, c = SS.oracle_run(oracle_mod, ("sweep", name), sc, R["W"], R["H"], SS.DEFAULT,
                                       SS.sweep_light_type(i), R["bounces"], R["frames"])
        assert np.isfinite(res).all(), name
        black = (res[:, :3] == 0).all(axis=1).mean()
        rays = c["rays"] / (n * len(R["frames"]))
        print(f"{name}: black {black:.3f}, rays/pixel {rays:.2f}")
        assert black <= 0.25, (name, black)
        assert rays >= 1.4, (name, rays)


@needs_refcpu
def test_cameras_reference_cpu_equals_oracle(oracle_mod, sweeps):
    R = SS.SWEEP_RUN
    for name, cam in SS.CAMERAS.items():
        _ref_equals_oracle(oracle_mod, sweeps["mixed"], R["W"], R["H"], cam, 0, R["bounces"], R["frames"],
                           ("camera", name))


def test_cameras_coverage(oracle_mod, sweeps):
    """The degenerate bases give every pixel one ray; the axis-aligned ones hit the scene."""
    R = SS.SWEEP_RUN
    for name, cam in SS.CAMERAS.items():
        res, ids, t, _ = SS.oracle_run(oracle_mod, ("camera", name), sweeps["mixed"], R["W"], R["H"], cam, 0,
                                       R["bounces"], R["frames"])
        assert np.isfinite(res).all(), name
        if name in ("up0", "up0_negzero", "axis_x", "axis_negz"):
            assert len(np.unique(ids)) == 1 and ids[0] >= 0, name
            assert len(np.unique(t.view(np.uint32))) == 1, name
    inside = SS.oracle_run(oracle_mod, ("camera", "inside"), sweeps["mixed"], R["W"], R["H"], SS.CAMERAS["inside"],
                           0, R["bounces"], R["frames"])
    assert (inside[1] >= 0).mean() > 0.9


def _soup_run(oracle, case, cam_name, nonfinite=False):
    R = SS.SOUP_RUN
    sc = SS.soup_scene(*case, nonfinite=nonfinite)
    return sc, SS.oracle_run(oracle, ("soup", case, cam_name, nonfinite), sc, R["W"], R["H"],
                             SS.SOUP_CAMERAS[cam_name], 0, R["bounces"], R["frames"])


@needs_refcpu
@pytest.mark.parametrize("cam", list(SS.SOUP_CAMERAS))
def test_soups_reference_cpu_equals_oracle(oracle_mod, cam):
    R = SS.SOUP_RUN
    for case in SS.soup_cases():
        sc = SS.soup_scene(*case)
        _ref_equals_oracle(oracle_mod, sc, R["W"], R["H"], SS.SOUP_CAMERAS[cam], 0, R["bounces"], R["frames"],
                           ("soup", case, cam, False))


@needs_refcpu
def test_path_soups_reference_cpu_equals_oracle(oracle_mod):
    R = SS.SOUP_RUN
    for case in SS.PATH_SOUPS.values():
        _ref_equals_oracle(oracle_mod, SS.soup_scene(*case), R["W"], R["H"], SS.SOUP_CAMERAS["inside"], 0,
                           R["bounces"], SS.PATH_FRAMES, ("soup", case, "inside", "f012"))


@needs_refcpu
def test_nonfinite_soup_reference_cpu_equals_oracle(oracle_mod):
    R = SS.SOUP_RUN
    for tree in ("sah4", "rt7"):
        for cam in SS.SOUP_CAMERAS:
            case = (SS.SOUP_SEEDS[0], tree)
            sc = SS.soup_scene(*case, nonfinite=True)
            _ref_equals_oracle(oracle_mod, sc, R["W"], R["H"], SS.SOUP_CAMERAS[cam], 0, R["bounces"], R["frames"],
                               ("soup", case, cam, True))
            assert np.isfinite(SS._oracle_cache[("soup", case, cam, True)][0]).all()


def test_soups_coverage_inside(oracle_mod):
    behind = []
    for case in SS.soup_cases():
        _, (res, ids, t, _) = _soup_run(oracle_mod, case, "inside")
        assert np.isfinite(res).all(), case
        share = (ids >= 0).mean()
        neg = (t[ids >= 0] < 0).mean()
        print(f"{SS.case_id(case)}: primary-hit share {share:.2f}, t < 0 on {neg:.2f} of them")
        assert share >= 0.5, (case, share)
        behind.append(neg >= 0.5)
    assert np.mean(behind) >= 1 / 3, behind


def test_soups_coverage_default_camera(oracle_mod):
    for case in SS.soup_cases():
        _, (res, ids, t, _) = _soup_run(oracle_mod, case, "default")
        assert np.isfinite(res).all(), case
        share = (ids >= 0).mean()
        distinct = len(np.unique(ids[ids >= 0]))
        print(f"{SS.case_id(case)}: primary-hit share {share:.2f}, {distinct} distinct primary triangles")
        assert share >= 0.10, (case, share)
        if case[1] != "chain":
            assert distinct >= 30, (case, distinct)


def test_soups_hit_the_defects(oracle_mod):
    """The smooth normals matter (some hit triangle has differing vertex normals) and the
    zero-length ones are reached."""
    reached_zero = reached_smooth = False
    for case in SS.soup_cases():
        sc, (_, ids, _, _) = _soup_run(oracle_mod, case, "inside")
        tri = sc.triangles[np.unique(ids[ids >= 0])]
        n1, n2 = tri["v1"]["normal"][:, :3], tri["v2"]["normal"][:, :3]
        reached_zero |= bool((np.abs(n1).sum(axis=1) == 0).any())
        reached_smooth |= bool((n1 != n2).any())
    assert reached_zero and reached_smooth

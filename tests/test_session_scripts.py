"""CPU: the session scripts themselves (session_script.py) -- both generators are deterministic, the
text form round-trips, the cover set holds every ordered pair of kinds under the
observed-before-overwritten rule, every session is valid, and the inputs are not trivial: the CPU
model of the image (oracle.render on the model scene) changes when a step is taken out."""
import pytest

import session_script as SC
import tuning_table


@pytest.fixture(scope="module")
def cover():
    return SC.cover_sessions()


@pytest.fixture(scope="module")
def randoms():
    return SC.random_sessions()


def test_vocabulary():
    assert len(SC.KINDS) == 21 and len(set(SC.KINDS)) == 21
    assert SC.INADMISSIBLE == frozenset()           # every kind may follow every kind
    assert len(SC.all_pairs()) == 21 * 21
    assert set(SC.RESULT_NEUTRAL) <= set(SC.KINDS)
    assert (SC.W, SC.H, SC.BOUNCES, SC.N_RAYS) == (100, 37, 3, 64)
    assert SC.W % 16 and SC.H % 16 and SC.NPIX % 64
    for first, last in SC.RANGES[1:]:               # a set range starts and ends inside a tile
        assert (first % SC.W) % 16 and (last % SC.W) % 16 and (first // SC.W) % 16 and (last // SC.W) % 16
        assert 0 < first < last < SC.NPIX
    for w, h in SC.DENOISE_VIEWS:
        assert w * h <= SC.NPIX


def test_tune_values_are_legal_values_of_every_knob():
    knobs = {k[0]: k for k in tuning_table.KNOBS}
    assert set(SC.TUNE_VALUES) == set(knobs)
    for name, values in SC.TUNE_VALUES.items():
        _, _, lo, hi, mult = knobs[name]
        assert len(values) >= 2
        for v in values:
            assert lo <= v <= hi and v % mult == 0, (name, v)


def test_scene_sizes(cornell):
    import stress_scenes as SS
    assert SC.SCENES == {"cornell": len(cornell.triangles), "big": len(SS.soup_scene(12, "big").triangles)}


def test_generators_are_deterministic_and_text_round_trips(cover, randoms):
    assert SC.cover_sessions() == cover and SC.random_sessions() == randoms
    assert SC.cover_sessions(seed=2) != cover
    assert len(randoms) == 8 and all(len(s) == SC.SESSION_STEPS for s in randoms)
    assert len({SC.text(s) for s in randoms}) == 8
    for s in cover + randoms:
        assert SC.parse(SC.text(s)) == s
        assert len(s) <= SC.SESSION_STEPS


def test_cover_set_covers_every_ordered_pair(cover):
    got = set()
    for s in cover:
        got |= SC.covered_pairs(s)
    want = SC.all_pairs()
    steps = sum(len(s) for s in cover)
    print(f"cover set: {len(SC.KINDS)} kinds, {len(want)} pairs, {len(cover)} sessions, {steps} steps; "
          f"{len(got & want)} pairs covered")
    assert got >= want, sorted(want - got)
    # every counted pair ran both calls: the cover set scripts no refused call at all, the random
    # sessions bring refused ones on top
    assert not any(SC.refused_pairs(s) for s in cover)
    extra = set()
    for s in SC.random_sessions():
        extra |= SC.refused_pairs(s)
    print(f"pairs the random sessions also run with a refused member: {len(extra)}")
    assert extra
    # no session is idle: each adds pairs the ones before it did not hold, and 59 adjacent pairs per
    # session bound the count from below
    seen = set()
    for s in cover:
        new = SC.covered_pairs(s) - seen
        assert new
        seen |= new
    assert len(cover) >= -(-len(want) // (SC.SESSION_STEPS - 1))
    assert len(cover) <= 2 * -(-len(want) // (SC.SESSION_STEPS - 1))


def test_the_rule_drops_a_pair_whose_result_is_overwritten_unobserved():
    s = list(SC.PROLOGUE) + [SC.step("denoise", iterations=1, view=0), SC.step("denoise", iterations=2, view=0)]
    got = SC.covered_pairs(s)
    assert ("denoise", "denoise") in got and ("features", "denoise") not in got
    s.insert(4, SC.step("read"))
    assert ("features", "denoise") in SC.covered_pairs(s)
    s = list(SC.PROLOGUE) + [SC.step("frame"), SC.step("restart", cam=1, fc=1)]
    assert ("features", "frame") not in SC.covered_pairs(s)


def test_every_session_is_valid(cover, randoms):
    for s in cover + randoms:
        assert SC.problems(s) == []
        assert s[-1].kind == "read"
    # the check itself notices each rule
    t = SC.Track()
    assert t.query is None and t.feat is None
    bad = [SC.step("surfaces")]
    assert any("prologue" in p for p in SC.problems(bad)) and any("surfaces" in p for p in SC.problems(bad))
    assert any("features" in p for p in SC.problems([SC.step("temporal")]))
    pro = list(SC.PROLOGUE)
    assert SC.problems(pro + [SC.step("move", first=60, n=13, normals=0, seed=1)])
    assert not SC.problems(pro + [SC.step("rebind"), SC.step("move", first=60, n=13, normals=0, seed=1)])
    assert SC.problems(pro + [SC.step("read_nb")]) and not SC.problems(pro + [SC.step("read_nb"), SC.step("finish")])
    assert SC.problems(pro + [SC.step("interleave", period=3, phase=0), SC.step("sched", to="tiles")])


def test_temporal_views_are_the_cameras_of_its_features(cover, randoms):
    n = 0
    for s in cover + randoms:
        for step, t in zip(s, SC.tracks(s)):
            if step.kind in ("denoise", "temporal"):
                assert t.feat is not None and t.feat_cam[t.feat] is not None
                n += 1
            if step.kind == "temporal" and t.hist is not None:
                assert t.hist[2] is not None and t.temporal_target() != t.hist[0]
                assert t.feature_target() != t.hist[1]   # the next feature pass spares the history's
    assert n > 50


def test_a_pair_with_a_refused_member_does_not_count():
    pro = list(SC.PROLOGUE)
    s = pro + [SC.step("rebind"), SC.step("features", n=1), SC.step("denoise", iterations=1, view=0),
               SC.step("query", first=0, mode=1), SC.step("surfaces")]
    got = SC.covered_pairs(s)
    assert ("features", "rebind") in got
    for pair in (("rebind", "features"), ("features", "denoise"), ("denoise", "query"), ("query", "surfaces")):
        assert pair not in got and pair in SC.refused_pairs(s)
    # the same calls on Cornell count; a refused step is never the dropped-step check's choice
    s2 = pro + s[4:]
    assert {("features", "denoise"), ("denoise", "query"), ("query", "surfaces")} <= SC.covered_pairs(s2)
    assert SC.droppable(s, "features") is None and SC.droppable(s, "query") is None
    assert SC.droppable(s2 + [SC.step("read")], "query") == 5


def _sym(lines, only=("image",)):
    return SC.symbolic_observations(list(SC.PROLOGUE) + SC.parse(lines), only)


def test_symbolic_replay_known_answers():
    """symbolic_observations on cases whose answer is plain: what a later step overwrites wholesale
    before any read is not seen, everything else is."""
    # a frame the host overwrites at once / before a read in between
    assert _sym("frame\nwrite_out blocking=1 seed=1\nread") == _sym("write_out blocking=1 seed=1\nread")
    assert _sym("frame\nread\nwrite_out blocking=1 seed=1\nread") != _sym("read\nwrite_out blocking=1 seed=1\nread")
    # an accumulating frame is seen, and so is its frameCount in every later frame
    assert _sym("frame\nframe\nread") != _sym("frame\nread")
    assert _sym("frames n=2\nframe\nread") != _sym("frames n=3\nframe\nread")
    # a restart over the whole frame forgets the image, whether from frameCount 0 or 1
    for fc in (0, 1):
        assert _sym(f"frames n=8\nrestart cam=1 fc={fc}\nread") == _sym(f"restart cam=1 fc={fc}\nread")
    # over a work range it forgets that range only: the frame before it still shows outside,
    # a frame inside the same range does not, one inside another range does
    rng, other = "range first=523 last=3057", "range first=1703 last=2199"
    assert _sym(f"frame\n{rng}\nrestart cam=1 fc=0\nread") != _sym(f"{rng}\nrestart cam=1 fc=0\nread")
    assert _sym(f"{rng}\nframe\nrestart cam=1 fc=0\nread") == _sym(f"{rng}\nrestart cam=1 fc=0\nread")
    assert (_sym(f"{other}\nframe\n{rng}\nrestart cam=1 fc=0\nread") !=
            _sym(f"{other}\n{rng}\nrestart cam=1 fc=0\nread"))
    # the scene shows in the image only through a launch
    assert _sym("write_mat blocking=1 seed=1\nread") == _sym("read")
    assert _sym("write_mat blocking=1 seed=1\nframe\nread") != _sym("frame\nread")
    assert _sym("write_mat blocking=1 seed=1\nwrite_mat blocking=1 seed=2\nframe\nread") == \
        _sym("write_mat blocking=1 seed=2\nframe\nread")
    assert _sym("move first=0 n=9 normals=0 seed=1\nrebind\nframe\nread") == _sym("rebind\nframe\nread")
    assert _sym("move first=0 n=9 normals=0 seed=1\nframe\nread") != _sym("frame\nread")
    # with every buffer looked at, a move or a material write shows without a launch; result-neutral steps never
    assert _sym("move first=0 n=9 normals=0 seed=1\nread", None) != _sym("read", None)
    assert _sym("tune knob=shade_min value=1\nsched to=tiles\nfinish\nframe\nread", None) == _sym("frame\nread", None)
    # a non-blocking read sees the image at its place in the queue
    assert _sym("read_nb\nframe\nread") != _sym("frame\nread_nb\nread")


IMAGE_KINDS = ("frame", "frames", "restart", "write_out", "write_mat", "move", "rebind")


def test_cpu_image_model_notices_a_deleted_step(cover, oracle_mod):
    """The two shortest cover sessions, every frame / frames / restart / write_out / write_mat / move /
    rebind step taken out in turn: the CPU model's image at the reads changes.  A cover set must also
    hold pairs such as (frame, write_out) and (write_mat, write_mat), whose first step no image can
    show; those steps are told apart by the symbolic replay (the image's provenance at every read is
    the same without them) and must then leave the image as it was.  A cut that leaves a `move` outside
    the bound scene (a `rebind` gone) is no session and is skipped; a kind left without a usable step
    takes its first usable one from the other sessions."""
    import session_exec as X
    sessions = sorted(cover, key=len)[:2]
    visible = dict.fromkeys(IMAGE_KINDS, 0)
    hidden = 0
    for s in sessions:
        base = X.cpu_image_observations(s)
        assert len(set(base)) > 1
        sym = SC.symbolic_observations(s, only=("image",))
        for i in range(len(SC.PROLOGUE), len(s)):
            if s[i].kind not in IMAGE_KINDS:
                continue
            cut = s[:i] + s[i + 1:]
            if SC.problems(cut):
                continue
            changed = X.cpu_image_observations(cut) != base
            if SC.symbolic_observations(cut, only=("image",)) != sym:
                assert changed, f"step {i} ({SC.text([s[i]])}) leaves the image as it was"
                visible[s[i].kind] += 1
            else:
                assert not changed, f"step {i} ({SC.text([s[i]])})"
                hidden += 1
    # a kind the two shortest sessions hold no usable step of: its first usable step elsewhere
    for kind in [k for k, n in visible.items() if not n]:
        for s in sorted(cover, key=len)[2:]:
            i = SC.droppable(s, kind, only=("image",))
            if i is not None:
                assert X.cpu_image_observations(s[:i] + s[i + 1:]) != X.cpu_image_observations(s), (kind, i)
                visible[kind] += 1
                break
    print(f"deleted steps the image shows: {visible}; overwritten before any read: {hidden}")
    assert all(visible.values()), visible
    assert sum(visible.values()) > hidden       # most steps show

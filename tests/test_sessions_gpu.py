"""GPU: every ordered pair of queue operations against a plain replay.

A session (session_script.py) runs twice.  The live run keeps one context and one kernel for the whole
script, under a profile that forces one of the library's queueing paths (coalescing, automatic or
forced deferral, an exposed device pointer, the global scene records).  The plain replay
(session_exec.run_plain) gives every step a fresh context, kernel and buffers and carries nothing but
host arrays from step to step.  Whatever the host can read -- the image, primary hits, query hits,
camera rays, surfaces, features, the denoised and both temporal images, both scenes' triangle, node and
material buffers, every status, and the four counters while stats are on -- must be the same bytes at
every `read`, every non-blocking read and the session's end.  A profile holds its own knobs for the
whole session: the live run leaves out a `tune` step on one of them (session_exec.PROFILE_KNOBS).
In pinned math the plain replay's steps are also checked against the CPU references
(session_exec.check_plain_against_cpu).

The cover set holds every ordered pair of the 21 kinds adjacent at least once (test_session_scripts.py);
8 random sessions add longer interactions.  100 x 37 pixels, 3 bounces, 64 query rays.

To replay one session by hand:
    import session_script as SC, session_exec as X
    from clrt import _native as N
    s = SC.cover_sessions()[3]              # or SC.random_sessions()[i], or SC.parse(text)
    print(X.compare(X.run_live(s, "queued", N.MATH_SHIPPED), X.run_plain(s, N.MATH_SHIPPED), s, "c3", "queued"))
"""
import functools

import numpy as np
import pytest

import session_exec as X
import session_script as SC
from clrt import _native as N

pytestmark = pytest.mark.gpu

COVER = SC.cover_sessions()
RANDOM = SC.random_sessions()
# sessions that neither rebind nor rewrite the materials: the scene is prepared in full exactly once
STEADY_KINDS = tuple(k for k in SC.KINDS if k not in ("rebind", "write_mat"))


def _steady(count=2, seed=200):
    """The first `count` seeds from `seed` up whose session moves geometry, denoises at two or more view
    sizes and takes features twice or more."""
    out = []
    while len(out) < count:
        s = SC.random_sessions(count=1, seed=seed, kinds=STEADY_KINDS)[0]
        kinds = [x.kind for x in s]
        views = {SC.arg(x, "view") for x in s if x.kind == "denoise"}
        if kinds.count("move") >= 1 and len(views) >= 2 and kinds.count("features") >= 2:
            out.append((seed, s))
        seed += 1
    return out


STEADY = _steady()
# hand-written: the orders the suite never had -- two of the newer calls side by side, a newer call in
# front of frames, a refit between held-back frames, a smaller denoise after a larger one
HAND = {"newer_calls_side_by_side": SC.parse("""
    frame
    query first=0 mode=0
    features n=1
    move first=3 n=40 normals=1 seed=901
    features n=4
    temporal
    read
    denoise iterations=5 view=0
    denoise iterations=2 view=1
    features n=1
    frame
    frame
    frame
    move first=0 n=72 normals=0 seed=902
    frame
    frame
    surfaces
    camera_rays
    frames n=8
    temporal
    frames n=3
    read_nb
    restart cam=2 fc=1
    features n=1
    temporal
    denoise iterations=3 view=2
    read
""")}
SESSIONS = dict([(f"c{i}", s) for i, s in enumerate(COVER)] + [(f"r{i}", s) for i, s in enumerate(RANDOM)] +
                [(f"s{i}", s) for i, (_, s) in enumerate(STEADY)] + list(HAND.items()))
# how to make each session again: the mismatch message names the generator and its seed
ORIGIN = dict([(f"c{i}", f"c{i} = cover_sessions(seed=1)[{i}]") for i in range(len(COVER))] +
              [(f"r{i}", f"r{i} = random_sessions(seed=100)[{i}]") for i in range(len(RANDOM))] +
              [(f"s{i}", f"s{i} = random_sessions(1, seed={seed}, kinds=STEADY_KINDS)[0]")
               for i, (seed, _) in enumerate(STEADY)] + [(h, f"HAND[{h!r}]") for h in HAND])
# the kinds the dropped-step check takes out, one step each; the rest change no result by contract
OMITTED_KINDS = ("tune", "finish", "sched", "stats")
DROPPED_KINDS = tuple(k for k in SC.KINDS if k not in OMITTED_KINDS)
assert set(OMITTED_KINDS) == set(SC.RESULT_NEUTRAL)

_plain, _live = {}, {}


def plain(label, math, path="auto"):
    """The plain replay of a session: once per (session, math mode, scene path), shared, read-only."""
    key = (label, math, path)
    if key not in _plain:
        pinned = math == N.MATH_PINNED
        _plain[key] = X.run_plain(SESSIONS[label], math, path, tie_features=pinned, keep_steps=pinned)
    return _plain[key]


def live(label, profile, math, hits=True):
    key = (label, profile, math, hits)
    if key not in _live:
        _live[key] = X.run_live(SESSIONS[label], profile, math, hits=hits)
    return _live[key]


def check(label, profile, math, hits=True):
    path = "global" if profile == "global" else "auto"
    run = live(label, profile, math, hits)
    bad = X.compare(run, plain(label, math, path), SESSIONS[label], ORIGIN[label], profile,
                    skip=() if hits else ("hit_ids", "hit_t"))
    assert bad is None, str(bad)
    check_prepares(label, run)


def check_prepares(label, run):
    """rtDiagScenePrepares at the session's end: without `rebind` / `write_mat` the live kernel prepared
    its scene in full exactly once, and refitted once per `move`."""
    kinds = [s.kind for s in SESSIONS[label]]
    full, refits = run.prepares
    assert refits <= kinds.count("move") and full >= 1
    if "rebind" not in kinds and "write_mat" not in kinds:
        assert (full, refits) == (1, kinds.count("move")), (label, full, refits)


COVER_IDS = [f"c{i}" for i in range(len(COVER))]


@pytest.mark.parametrize("profile", X.PROFILES)
@pytest.mark.parametrize("label", COVER_IDS)
def test_live_equals_plain_shipped(label, profile):
    check(label, profile, N.MATH_SHIPPED)


@pytest.mark.parametrize("profile", ["defaults", "queued"])
@pytest.mark.parametrize("label", COVER_IDS)
def test_live_equals_plain_without_hit_buffers(label, profile):
    """With primary-hit buffers bound every fused render stays on the main stream (each writes them).
    The same sessions with none bound: fused renders rotate through the render streams and radiance
    sets beside the accumulation; everything else the host reads is the plain replay's."""
    check(label, profile, N.MATH_SHIPPED, hits=False)


@pytest.mark.parametrize("profile", ["defaults", "queued"])
@pytest.mark.parametrize("label", COVER_IDS)
def test_live_equals_plain_pinned(label, profile):
    check(label, profile, N.MATH_PINNED)


@pytest.mark.parametrize("hits", [True, False], ids=["hit_buffers", "no_hit_buffers"])
@pytest.mark.parametrize("profile", X.PROFILES)
@pytest.mark.parametrize("label", list(HAND))
def test_hand_written_sessions(label, profile, hits):
    assert SC.problems(SESSIONS[label]) == []
    check(label, profile, N.MATH_SHIPPED, hits=hits)
    assert live(label, profile, N.MATH_SHIPPED, hits).prepares == (1, 2)    # one preparation, two refits


@pytest.mark.parametrize("label", [f"r{i}" for i in range(len(RANDOM))])
def test_random_sessions_live_equals_plain(label):
    check(label, "queued", N.MATH_SHIPPED)


@pytest.mark.parametrize("profile", ["defaults", "queued", "global"])
@pytest.mark.parametrize("label", [f"s{i}" for i in range(len(STEADY))])
def test_one_preparation_and_one_refit_per_move(label, profile):
    """Sessions without `rebind` / `write_mat`: denoise views that grow and shrink, feature passes and
    queries reuse the kernel's scratch blocks, and the packed scene is prepared once."""
    kinds = [s.kind for s in SESSIONS[label]]
    assert kinds.count("move") >= 1 and kinds.count("denoise") >= 2 and kinds.count("features") >= 2
    assert "rebind" not in kinds and "write_mat" not in kinds
    check(label, profile, N.MATH_SHIPPED)
    assert live(label, profile, N.MATH_SHIPPED).prepares == (1, kinds.count("move"))


@pytest.mark.parametrize("label", COVER_IDS)
def test_plain_equals_cpu_model(label, oracle_mod):
    X.check_plain_against_cpu(SESSIONS[label], plain(label, N.MATH_PINNED), label)


@functools.lru_cache(maxsize=None)
def _droppable(label, kind):
    return SC.droppable(SESSIONS[label], kind)


def _drop_case(kind):
    """(label, index): the first cover session holding a `kind` step whose loss the host can observe
    (session_script.droppable), preferring the session that serves the most kinds."""
    for label in sorted(COVER_IDS, key=lambda c: -sum(_droppable(c, k) is not None for k in DROPPED_KINDS)):
        i = _droppable(label, kind)
        if i is not None:
            return label, i
    raise AssertionError(f"no cover session holds a droppable {kind} step")


@pytest.mark.parametrize("kind", DROPPED_KINDS)
def test_harness_notices_a_dropped_step(kind):
    """One step of `kind` taken out of the replay only: the comparison reports a mismatch at or after
    that step.  OMITTED_KINDS are result-neutral by contract and are left out."""
    label, i = _drop_case(kind)
    s = SESSIONS[label]
    assert s[i].kind == kind
    cut = s[:i] + s[i + 1:]
    bad = X.compare(live(label, "defaults", N.MATH_SHIPPED), X.run_plain(cut, N.MATH_SHIPPED), s, ORIGIN[label],
                    "defaults")
    assert bad is not None, f"{label}: step {i} ({SC.text([s[i]])}) can be dropped unnoticed"
    assert bad.index >= i, str(bad)
    assert f"session {label}" in str(bad) and "profile defaults" in str(bad) and "buffer" in str(bad) or \
        "no such observation" in str(bad)


def test_results_are_not_trivial():
    """The observed buffers hold results: most pixels rendered, hits and misses among the query's rays,
    covered and uncovered feature pixels, a denoised and a temporal image that differ from the image."""
    o = plain("c0", N.MATH_SHIPPED).obs[-1][2]
    assert (X.rgb(o["image"]) != 0).any(axis=1).mean() > 0.5
    prologue = X.run_plain(list(SC.PROLOGUE), N.MATH_SHIPPED).obs[-1][2]
    prim = prologue["qhits"]["prim"]
    assert (prim >= 0).sum() >= 8 and (prim < 0).sum() >= 1
    cov = prologue["feat0"]["coverage"]
    assert (cov > 0).sum() > 500 and (cov == 0).sum() > 50
    for name in ("denoise", "temp0"):
        ends = [plain(c, N.MATH_SHIPPED).obs[-1][2] for c in COVER_IDS]
        assert any(e[name].any() and e[name].tobytes() != e["image"].tobytes() for e in ends), name
    assert any("counters" in ob and ob["counters"].all() for c in COVER_IDS
               for _, _, ob in plain(c, N.MATH_SHIPPED).obs)
    # the random sessions hold refused calls (the cover set scripts none): the refusal is compared too
    assert any((np.asarray(ob.get("status", 0)) == X.INVALID_OPERATION).any() for c in [f"r{i}" for i in range(8)]
               for _, _, ob in plain(c, N.MATH_SHIPPED).obs)

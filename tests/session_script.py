"""Queue-API sessions as data: the vocabulary, the bookkeeping both executors share, and two seeded
generators.  Pure Python: no GPU, no library, no numpy.

A session is a list of Step(kind, args).  Its text form is one step per line, `kind key=value ...`,
and round-trips through parse().  Every session starts with PROLOGUE (Cornell bound by the executor;
one frame, one query, one feature pass), after which every kind is admissible at every position:
INADMISSIBLE, the table of ordered pairs that may not be adjacent, is empty and stays empty.

Track is the host's own bookkeeping while a session runs -- which scene is bound, what the kernel's
FRAME_COUNT and camera slots hold, which feature and temporal buffer is written next.  The generators
use it to pick legal parameters, the validity check replays it, and the executors (session_exec.py)
read every call's arguments from it, so the live run and the plain replay cannot disagree about what a
step means.

Two calls are refused by contract rather than run (nothing is launched, the status is the result):
`query` and `features` while the soup with a 140-triangle leaf is bound (RT_INVALID_OPERATION: no octant
records).  `surfaces` intersects nothing and runs on that scene too, over whatever the hit buffer holds.
The refusal is part of what both executors record and compare, but a pair with a refused member does
not count as covered: the cover walk never scripts one, the random sessions do.  A launch error, which
a coalesced launch would report late, is never scripted: the generators keep the tile schedule and a
band interleave apart.

`denoise` and `temporal` take the features as they are, with the camera they were taken at: a pair such
as (restart, denoise) has to be adjacent, so the features cannot always be of the camera that moved one
step earlier.  What the validity check holds is that features exist and that every view handed to
`temporal` is the camera its feature buffer was taken at.
"""
import random
from collections import namedtuple

KINDS = ("frame", "frames", "restart", "read", "finish", "read_nb", "write_out", "write_mat", "move",
         "rebind", "query", "camera_rays", "surfaces", "features", "denoise", "temporal", "sched", "range",
         "interleave", "tune", "stats")
# ordered pairs (a, b) that may not be adjacent: none
INADMISSIBLE = frozenset()
# kinds that change no result by contract (the dropped-step check leaves them out)
RESULT_NEUTRAL = ("tune", "finish", "sched", "stats")

W, H = 100, 37            # no multiple of the 16 x 16 tile or of 64 lanes
NPIX = W * H
BOUNCES = 3
N_RAYS = 64
SCENES = {"cornell": 72, "big": 200}                   # bound scene -> triangles (checked by the CPU tests)
N_CAMERAS = 4                                          # session_exec.CAMERAS
FRAMES_N = (2, 3, 8, 9)
FEATURES_N = (1, 4)
SCHEDS = ("tiles", "step", "wavefront")
RANGES = ((0, 0), (5 * W + 23, 30 * W + 57), (17 * W + 3, 21 * W + 99))   # start and end inside a tile
DENOISE_VIEWS = ((W, H), (37, 21), (64, 29))           # the image, or its first w x h slots
QUERY_FIRSTS = (0, 16)
SESSION_STEPS = 60
# rtKernelSetTuning knobs and a few legal values each (tuning_table.KNOBS; checked by the CPU tests)
TUNE_VALUES = {
    "refill_min": (1, 6, 64), "shade_min": (1, 40, 64), "refill_min_global": (0, 8, 64),
    "shade_min_global": (0, 16, 64), "step_weight_node": (1, 35, 1000), "step_weight_leaf": (1, 55, 1000),
    "step_weight_node_global": (0, 65, 1000), "step_weight_leaf_global": (0, 55, 1000),
    "chunk_pixels": (0, 64, 4096), "tail_chunk": (64, 128, 4096), "bulk_percent": (0, 50, 100),
    "tile_major": (-1, 0, 1, 2), "max_blocks": (0, 1, 64), "perframe_sky": (0, 1, 2),
    "wf_refill_min": (1, 32, 64), "wf_streams_per_cu": (0, 1, 64), "wf_top_nodes": (0, 7, 1024),
    "global_oct": (0, 1), "perframe_defer": (0, 1, 2), "perframe_defer_min": (0, 1024, 4194304),
    "perframe_batch": (1, 2, 3, 8), "query_refill_min": (1, 32, 64),
}

Step = namedtuple("Step", "kind args")          # args: a sorted tuple of (key, value) pairs


def step(kind, **args):
    assert kind in KINDS, kind
    return Step(kind, tuple(sorted(args.items())))


def arg(s, key, default=None):
    return dict(s.args).get(key, default)


def text(session):
    return "\n".join(" ".join([s.kind] + [f"{k}={v}" for k, v in s.args]) for s in session)


def parse(txt):
    out = []
    for line in txt.splitlines():
        parts = line.split()
        if not parts:
            continue
        args = {}
        for p in parts[1:]:
            k, v = p.split("=", 1)
            try:
                args[k] = int(v)
            except ValueError:
                args[k] = v
        out.append(step(parts[0], **args))
    return out


PROLOGUE = (step("frame"), step("query", first=0, mode=0), step("features", n=1))


class Track:
    """The host's bookkeeping, before and after each step."""

    def __init__(self):
        self.scene = "cornell"
        self.cam = 0               # the host's camera (the next frame's)
        self.next_fc = 1           # the next frame's frameCount
        self.slot_fc = 1           # what the kernel's FRAME_COUNT and camera slots hold
        self.slot_cam = 0
        self.sched = "step"
        self.range = (0, 0)
        self.interleave = (1, 0)
        self.stats = False
        self.query = None          # (first, mode) of the last answered query
        self.feat = None           # index of the feature buffer written last
        self.feat_cam = [None, None]   # camera each feature buffer was taken at
        self.hist = None           # (temporal buffer, feature buffer, camera) of the last temporal

    def refused(self, s):
        """True where the call is refused by contract (RT_INVALID_OPERATION) and nothing runs."""
        return self.scene == "big" and s.kind in ("query", "features")

    def feature_target(self):
        """The feature buffer a `features` step writes: never the one the last temporal call took as
        its current features, which the next one hands in as the history's."""
        return 0 if self.hist is None else 1 - self.hist[1]

    def temporal_target(self):
        return 0 if self.hist is None else 1 - self.hist[0]

    def apply(self, s):
        k = s.kind
        if k in ("frame", "frames"):
            n = arg(s, "n", 1)
            self.slot_fc, self.slot_cam = self.next_fc, self.cam
            self.next_fc += n
        elif k == "restart":
            self.cam = arg(s, "cam")
            self.slot_fc, self.slot_cam = arg(s, "fc"), self.cam
            self.next_fc = arg(s, "fc") + 1
        elif k == "rebind":
            self.scene = "big" if self.scene == "cornell" else "cornell"
        elif k == "query":
            if not self.refused(s):
                self.query = (arg(s, "first"), arg(s, "mode"))
        elif k == "features":
            if not self.refused(s):
                self.feat = self.feature_target()
                self.feat_cam[self.feat] = self.slot_cam
        elif k == "temporal":
            if self.feat is not None:   # (problems() reports a temporal without features)
                self.hist = (self.temporal_target(), self.feat, self.feat_cam[self.feat])
        elif k == "sched":
            self.sched = arg(s, "to")
        elif k == "range":
            self.range = (arg(s, "first"), arg(s, "last"))
        elif k == "interleave":
            self.interleave = (arg(s, "period"), arg(s, "phase"))
        elif k == "stats":
            self.stats = not self.stats

    # ---- what a step writes, for the observed-before-overwritten rule ---------------------------
    def writes(self, s):
        """(buffers the step writes, buffers it overwrites wholesale).  The image is a frame's result;
        the primary-hit buffers every frame rewrites are its by-product and are not counted."""
        k = s.kind
        if self.refused(s):
            return (), ()
        if k in ("frame", "frames"):
            return ("image",), ()
        if k in ("restart", "write_out"):
            return ("image",), ("image",)
        if k == "write_mat":
            return ("mats",), ("mats",)
        if k == "move":
            return ("tris", "nodes"), ()
        if k == "query":
            return ("qhits",), ("qhits",)
        if k == "camera_rays":
            return ("camrays",), ("camrays",)
        if k == "surfaces":
            return ("surfaces",), ("surfaces",)
        if k == "features":
            b = f"feat{self.feature_target()}"
            return (b,), (b,)
        if k == "denoise":
            return ("denoise",), ("denoise",)
        if k == "temporal":
            b = f"temp{self.temporal_target()}"
            return (b,), (b,)
        return (), ()


def tracks(session):
    """The Track before each step, and the one after the last."""
    import copy
    t, out = Track(), []
    for s in session:
        out.append(copy.deepcopy(t))
        t.apply(s)
    out.append(t)
    return out


def covered_pairs(session):
    """The ordered pairs (a, b) of adjacent kinds in `session` that count: both calls ran (neither was
    refused), and everything b wrote was observed (a `read`, or the session's end) before a later step
    overwrote it wholesale."""
    covered, waiting = set(), []      # waiting: [pair, buffers still unobserved]
    ts = tracks(session)
    for i, s in enumerate(session):
        written, clobbered = ts[i].writes(s)
        waiting = [w for w in waiting if not (set(w[1]) & set(clobbered))]
        if s.kind == "read":
            covered.update(w[0] for w in waiting)
            waiting = []
        if i and not ts[i].refused(s) and not ts[i - 1].refused(session[i - 1]):
            pair = (session[i - 1].kind, s.kind)
            if written:
                waiting.append((pair, written))
            else:
                covered.add(pair)
    covered.update(w[0] for w in waiting)     # the session's end observes everything
    return covered


def refused_pairs(session):
    """The adjacent pairs of `session` with a refused member: they run too (the refusal is compared),
    on top of the pairs that count."""
    ts = tracks(session)
    return {(session[i - 1].kind, session[i].kind) for i in range(1, len(session))
            if ts[i].refused(session[i]) or ts[i - 1].refused(session[i - 1])}


def all_pairs():
    return {(a, b) for a in KINDS for b in KINDS} - INADMISSIBLE


def problems(session):
    """Why `session` is not valid: a list of strings, empty for a valid one."""
    out = []
    if tuple(session[:len(PROLOGUE)]) != PROLOGUE:
        out.append("does not start with the prologue")
    t = Track()
    unwaited = 0        # non-blocking reads not yet followed by a host wait
    for i, s in enumerate(session):
        k = s.kind
        if k in ("read", "finish") or (k in ("write_out", "write_mat") and arg(s, "blocking")):
            unwaited = 0
        elif k == "read_nb":
            unwaited += 1
        if i and (session[i - 1].kind, k) in INADMISSIBLE:
            out.append(f"{i}: inadmissible pair")
        if k == "surfaces" and t.query is None:
            out.append(f"{i}: surfaces without a query on the same rays")
        if k in ("denoise", "temporal") and (t.feat is None or t.feat_cam[t.feat] is None):
            out.append(f"{i}: {k} without features")
        if k == "move" and not (0 <= arg(s, "first") and arg(s, "n") >= 1 and
                                arg(s, "first") + arg(s, "n") <= SCENES[t.scene]):
            out.append(f"{i}: move outside the bound scene's triangles")
        if k == "frames" and arg(s, "n") not in FRAMES_N:
            out.append(f"{i}: frames n")
        if k == "features" and arg(s, "n") not in FEATURES_N:
            out.append(f"{i}: features n")
        if k == "sched" and arg(s, "to") == "tiles" and t.interleave[0] > 1:
            out.append(f"{i}: tile schedule under a band interleave")
        if k == "interleave" and arg(s, "period") > 1 and t.sched == "tiles":
            out.append(f"{i}: band interleave under the tile schedule")
        if k == "tune" and arg(s, "value") not in TUNE_VALUES.get(arg(s, "knob"), ()):
            out.append(f"{i}: tune")
        t.apply(s)
    if unwaited:
        out.append("a read_nb is not followed by a host wait")
    return out


# ---- parameters --------------------------------------------------------------------------------
def make_step(kind, t, rng, serial):
    """A `kind` step with legal parameters for the bookkeeping `t`; `serial` makes seeds distinct."""
    if kind == "frames":
        return step(kind, n=rng.choice(FRAMES_N))
    if kind == "restart":
        return step(kind, cam=rng.choice([c for c in range(N_CAMERAS) if c != t.cam]), fc=rng.choice((0, 1)))
    if kind == "write_out":
        return step(kind, seed=serial, blocking=rng.choice((0, 1)))
    if kind == "write_mat":
        return step(kind, seed=serial, blocking=rng.choice((0, 1)))
    if kind == "move":
        n_tris = SCENES[t.scene]
        first = rng.randrange(0, n_tris - 1)
        return step(kind, seed=serial, first=first, n=rng.randrange(1, n_tris - first + 1),
                    normals=rng.choice((0, 1)))
    if kind == "query":
        prev = t.query or (0, 0)
        return step(kind, first=QUERY_FIRSTS[(QUERY_FIRSTS.index(prev[0]) + rng.choice((0, 1))) % 2],
                    mode=1 - prev[1])
    if kind == "features":
        return step(kind, n=rng.choice(FEATURES_N))
    if kind == "denoise":
        return step(kind, iterations=rng.randrange(1, 6), view=rng.randrange(len(DENOISE_VIEWS)))
    if kind == "sched":
        legal = [x for x in SCHEDS if x != t.sched and not (x == "tiles" and t.interleave[0] > 1)]
        return step(kind, to=rng.choice(legal))
    if kind == "range":
        first, last = rng.choice([r for r in RANGES if r != t.range])
        return step(kind, first=first, last=last)
    if kind == "interleave":
        if t.interleave[0] > 1 or t.sched == "tiles":
            return step(kind, period=1, phase=0)
        return step(kind, period=3, phase=rng.randrange(3))
    if kind == "tune":
        knob = rng.choice(sorted(TUNE_VALUES))
        return step(kind, knob=knob, value=rng.choice(TUNE_VALUES[knob]))
    return step(kind)


class _Builder:
    def __init__(self, rng):
        self.rng = rng
        self.steps = []
        self.t = Track()
        self.waiting = []   # [pair, buffers]: written, not yet observed
        self.done = set()   # pairs that count so far
        self.last_refused = False
        for s in PROLOGUE:
            self.push(s)

    def push(self, s):
        written, clobbered = self.t.writes(s)
        self.waiting = [w for w in self.waiting if not (set(w[1]) & set(clobbered))]
        if s.kind == "read":
            self.done.update(w[0] for w in self.waiting)
            self.waiting = []
        refused = self.t.refused(s)
        if self.steps and not refused and not self.last_refused:
            pair = (self.steps[-1].kind, s.kind)
            if written:
                self.waiting.append((pair, written))
            else:
                self.done.add(pair)
        self.last_refused = refused
        self.steps.append(s)
        self.t.apply(s)

    def add(self, kind):
        self.push(make_step(kind, self.t, self.rng, len(self.steps)))

    def would_refuse(self, kind):
        return self.t.refused(step(kind))

    def would_lose(self, kind, wanted):
        """The wanted pairs whose result a `kind` step would overwrite unobserved."""
        s = make_step(kind, self.t, random.Random(0), 0)
        clobbered = set(self.t.writes(s)[1])
        return {w[0] for w in self.waiting if w[0] in wanted and set(w[1]) & clobbered}

    def finish(self):
        if self.steps[-1].kind != "read":
            self.add("read")
        self.done.update(w[0] for w in self.waiting)
        assert self.done == covered_pairs(self.steps)
        return self.steps


def cover_sessions(seed=1):
    """Sessions of at most about SESSION_STEPS steps in which every ordered pair of kinds is adjacent
    at least once and counts by covered_pairs(): a greedy walk over the pair graph that prefers an
    uncovered pair out of the current kind, then the kind with the most uncovered pairs left, and
    puts a `read` in front of a step that would overwrite an unobserved result it still needs.  A pair
    with a refused member does not count, so while the soup is bound the walk covers what it can
    without `query` and `features` and rebinds when only their pairs are left."""
    rng = random.Random(seed)
    todo = all_pairs()
    sessions = []
    while todo:
        b = _Builder(rng)
        before = len(todo)
        while todo and len(b.steps) < SESSION_STEPS - 1:
            last = b.steps[-1].kind
            # pairs whose result is written and waiting for a read: still wanted until observed
            wanted = {w[0] for w in b.waiting} & todo
            left = todo - wanted
            out_of = {a: sum((a, c) in left for c in KINDS) for a in KINDS}
            best, best_key = None, None
            for kind in KINDS:
                refuse = b.would_refuse(kind)
                gain = (last, kind) in left and (last, kind) not in INADMISSIBLE and not refuse and not b.last_refused
                lose = len(b.would_lose(kind, wanted))
                key = (gain and not lose, -lose, -1 if refuse else out_of[kind], rng.random())
                if best_key is None or key > best_key:
                    best, best_key = kind, key
            if best_key[1] < 0 or (not best_key[0] and wanted):
                best = "read"           # observe what is waiting before anything overwrites it
            elif not best_key[0] and b.t.scene == "big" and any(k in p for p in left for k in ("query", "features")):
                best = "rebind"         # the pairs left need calls the soup refuses
            b.add(best)
            todo -= b.done
        steps = b.finish()
        todo -= covered_pairs(steps)
        sessions.append(steps)
        if len(todo) == before and len(sessions) > 200:
            raise RuntimeError(f"the cover walk does not converge: {sorted(todo)[:5]}")
    return sessions


def random_sessions(count=8, steps=SESSION_STEPS, seed=100, kinds=KINDS):
    """`count` seeded sessions of `steps` steps, kinds drawn uniformly from `kinds`."""
    out = []
    for i in range(count):
        rng = random.Random(seed + i)
        b = _Builder(rng)
        while len(b.steps) < steps - 1:
            b.add(rng.choice(kinds))
        out.append(b.finish())
    return out


# ---- a symbolic replay: which steps can be told apart by what the host observes -----------------
def symbolic_observations(session, only=None):
    """What the host could tell apart, as nested tuples: per observation (each `read`, each read_nb,
    the session's end) the provenance of every observed buffer -- which steps with which parameters and
    inputs produced it.  Two sessions with equal symbolic observations cannot be told apart; the
    dropped-step check uses it to pick a step whose loss is visible.  `only`: the buffers looked at
    (default: all of them, and the statuses)."""
    t = Track()
    v = {b: ("zero", ()) for b in ("image", "hits", "qhits", "camrays", "surfaces", "feat0", "feat1", "denoise",
                                "temp0", "temp1", "counters")}
    for sc in SCENES:
        for b in ("tris", "nodes", "mats"):
            v[f"{b}:{sc}"] = ("init", sc)
    obs, status = [], []

    def scene_state():
        return (t.scene, v[f"tris:{t.scene}"], v[f"nodes:{t.scene}"])

    def observe(tag):
        seen = sorted((k, hash(x)) for k, x in v.items()
                      if (k != "counters" or t.stats) and (only is None or k in only))
        obs.append((tag, tuple(seen), tuple(status) if only is None else ()))

    for i, s in enumerate(session):
        k, a = s.kind, s.args
        launched = None
        if t.refused(s):
            status.append((k, "refused"))
        elif k in ("frame", "frames", "restart"):
            cam = arg(s, "cam", t.cam)
            fc = arg(s, "fc", t.next_fc)
            launched = (k, a, fc, cam, scene_state(), v[f"mats:{t.scene}"], t.range, t.interleave)
            v["image"] = _launch_into(v["image"], launched, fc, (t.range, t.interleave))
            v["hits"] = (v["hits"], launched)
        elif k == "read":
            observe("read")
        elif k == "read_nb":
            obs.append(("read_nb", hash(v["image"])))
        elif k == "write_out":
            v["image"] = ((k, a), ())
        elif k == "write_mat":
            v[f"mats:{t.scene}"] = (k, a, t.scene)
        elif k == "move":
            v[f"tris:{t.scene}"] = (v[f"tris:{t.scene}"], k, a)
            v[f"nodes:{t.scene}"] = (v[f"nodes:{t.scene}"], v[f"tris:{t.scene}"])
        elif k == "query":
            launched = (k, a, scene_state())
            v["qhits"] = (v["qhits"], launched)
        elif k == "camera_rays":
            v["camrays"] = (k, t.slot_fc, t.slot_cam)
        elif k == "surfaces":
            launched = (k, t.query, v["qhits"], scene_state())
            v["surfaces"] = (v["surfaces"], launched)
        elif k == "features":
            launched = (k, a, t.slot_fc, t.slot_cam, scene_state(), v[f"mats:{t.scene}"])
            v[f"feat{t.feature_target()}"] = launched
        elif k == "denoise":
            v["denoise"] = (v["denoise"], k, a, v["image"], v[f"feat{t.feat}"])
        elif k == "temporal":
            h = t.hist
            v[f"temp{t.temporal_target()}"] = (k, v["image"], v[f"feat{t.feat}"], t.feat_cam[t.feat],
                                               None if h is None else (v[f"temp{h[0]}"], v[f"feat{h[1]}"], h[2]))
        if launched is not None and t.stats:
            v["counters"] = (v["counters"], launched)
        t.apply(s)
    observe("end")
    return obs


def _launch_into(image, launched, fc, mask):
    """The image's provenance after a launch: (what the whole image holds, ((mask, what was rendered over
    it), ...)).  frameCount 0 or 1 keeps nothing of the pixels it renders: over the whole frame it
    forgets everything, over a work range or band set everything rendered over that same set."""
    base, over = image if len(image) == 2 and isinstance(image[1], tuple) else (image, ())
    whole = mask == ((0, 0), (1, 0))
    if whole:
        return ((launched,), ()) if fc <= 1 else (((base, over), launched), ())
    if fc <= 1:
        return (base, tuple(o for o in over if o[0] != mask) + ((mask, launched),))
    if over and over[-1][0] == mask:
        return (base, over[:-1] + ((mask, (over[-1][1], launched)),))
    return (base, over + ((mask, ("onto", launched)),))


def droppable(session, kind, only=None):
    """Index of the first `kind` step (after the prologue) whose deletion changes what the host
    observes by the symbolic replay and leaves a valid session, or None."""
    base = symbolic_observations(session, only)
    ts = tracks(session)
    for i in range(len(PROLOGUE), len(session)):
        if session[i].kind != kind or ts[i].refused(session[i]):
            continue                    # (a refused call has no result to lose)
        cut = session[:i] + session[i + 1:]
        if not problems(cut) and symbolic_observations(cut, only) != base:
            return i
    return None

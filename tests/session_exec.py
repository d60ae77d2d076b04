"""The executors of the session tests (session_script.py holds the vocabulary).

run_live    one context and one kernel for the whole session, under a profile; exactly the script's
            calls, but for a `tune` of a knob the profile itself holds (PROFILE_KNOBS); the host waits
            only at `read`, `finish` and blocking writes.
run_plain   the plain replay: a fresh context, kernel and set of buffers for EVERY step, contents
            carried through host arrays, rtFinish and a full read-back after each step, per-frame
            launches one by one (perframe_batch 1, perframe_defer 0, perframe_sky 0, no accumulation
            overlap).  No packed scene, scratch block, counter slot, sky key or pending launch
            survives a step.  It does not depend on the profile.
CpuModel    the CPU references (oracle.render, ray_query_ref, surface_ref, denoise_ref, temporal_ref,
            refit_ref) applied to the plain replay's recorded steps, pinned math only.

Every comparison is of bytes.  compare() names the first observation and buffer that differ.
"""
import functools
import types

import numpy as np

import denoise_ref
import refit_ref as R
import session_script as SC
import stress_scenes as SS
import surface_ref
import temporal_ref
from hip_helpers import reference_camera, rgb
from session_script import BOUNCES, H, N_RAYS, NPIX, W, arg

CAMERAS = (reference_camera(), reference_camera(moves=("up", "right")), reference_camera(1.5, 1.65),
           reference_camera(1.62, 1.5, ("down", "left")))
assert len(CAMERAS) == SC.N_CAMERAS
INVALID_OPERATION = -59
PROFILES = ("defaults", "queued", "deferred", "exposed", "global")
# the knobs a profile sets and holds: the live run leaves a `tune` step on one of them out, so that the
# whole session runs under its profile (under `defaults` every knob is tuned)
PROFILE_KNOBS = {"defaults": (), "queued": ("perframe_defer_min", "perframe_sky", "tail_chunk", "perframe_defer"),
                 "deferred": ("perframe_defer", "perframe_batch"), "exposed": (), "global": ("global_oct",)}
COUNTERS = ("rays", "node_visits", "tri_tests", "hits")
FRAME_SEED = 12345


def _N():
    from clrt import _native as N
    return N


@functools.lru_cache(maxsize=None)
def scenes():
    """The two bound scenes; shared, never modified."""
    import clrt
    return {"cornell": clrt.scene.cornell(), "big": SS.soup_scene(12, "big")}


# ---- the data a step carries (a function of the script alone) ------------------------------------
def query_rays():
    N = _N()
    rng = np.random.default_rng(64)
    p = R.positions(scenes()["cornell"].triangles).reshape(-1, 3)
    rays = np.zeros(N_RAYS, N.RAY_DTYPE)
    rays["origin"] = rng.uniform(p.min(axis=0), p.max(axis=0), (N_RAYS, 3)).astype(np.float32)
    rays["dir"] = rng.standard_normal((N_RAYS, 3)).astype(np.float32)
    rays["tmin"], rays["tmax"] = -np.inf, 100000.0
    return rays


def image_data(seed):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (NPIX, 4)).astype(np.float32)


def material_data(scene_name, seed):
    m = scenes()[scene_name].materials.copy()
    rng = np.random.default_rng(seed)
    m["diffuse"][:, :3] = rng.uniform(0.1, 0.9, (len(m), 3)).astype(np.float32)
    m["specular"][:, :3] = rng.uniform(0.0, 1.0, (len(m), 3)).astype(np.float32)
    return m


def move_data(scene_name, s):
    """(position records, normal records or None) of a `move` step: the scene's original triangles of
    the range displaced by refit_ref.displaced, so the data does not depend on earlier moves."""
    first, n = arg(s, "first"), arg(s, "n")
    base = scenes()[scene_name].triangles[first:first + n]
    pos = R.tri_points(R.positions(R.displaced(base, arg(s, "seed"), sigma=0.3)))
    nrm = None
    if arg(s, "normals"):
        rng = np.random.default_rng(arg(s, "seed") + 7)
        nn = np.stack([base[v]["normal"][:, :3] for v in R.VERTS], axis=1).astype(np.float32)
        nrm = R.tri_points(nn + rng.normal(0.0, 0.3, nn.shape).astype(np.float32))
    return pos, nrm


def apply_move(tris, s, pos, nrm):
    first, n = arg(s, "first"), arg(s, "n")
    for v, p in zip(R.VERTS, ("p1", "p2", "p3")):
        tris[v]["position"][first:first + n, :3] = pos[p][:, :3]
        if nrm is not None:
            tris[v]["normal"][first:first + n, :3] = nrm[p][:, :3]


def initial_host():
    N = _N()
    host = {"image": np.zeros((NPIX, 4), np.float32), "hit_ids": np.zeros(NPIX, np.int32),
            "hit_t": np.zeros(NPIX, np.float32), "rays": query_rays(), "qhits": np.zeros(N_RAYS, N.RAY_HIT_DTYPE),
            "camrays": np.zeros(NPIX, N.RAY_DTYPE), "surfaces": np.zeros(N_RAYS, N.SURFACE_DTYPE),
            "feat0": np.zeros(NPIX, N.PIXEL_FEATURES_DTYPE), "feat1": np.zeros(NPIX, N.PIXEL_FEATURES_DTYPE),
            "denoise": np.zeros((NPIX, 4), np.float32), "temp0": np.zeros((NPIX, 4), np.float32),
            "temp1": np.zeros((NPIX, 4), np.float32)}
    for name, sc in scenes().items():
        host[f"tris:{name}"] = sc.triangles.copy()
        host[f"nodes:{name}"] = sc.nodes.copy()
        host[f"mats:{name}"] = sc.materials.copy()
    return host


OBSERVED = ("image", "hit_ids", "hit_t", "qhits", "camrays", "surfaces", "feat0", "feat1", "denoise", "temp0",
            "temp1", "tris:cornell", "nodes:cornell", "mats:cornell", "tris:big", "nodes:big", "mats:big")


# ---- one context, one kernel, every buffer -------------------------------------------------------
class Rig:
    def __init__(self, host, track, math, path, hits=True):
        import clrt
        N = self.N = _N()
        self.ctx = clrt.CLContext(0)
        self.k = clrt.CLKernel(self.ctx, "KernelEntry")
        rw = N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR
        self.host0 = host
        self.buf = {name: self.ctx.create_buffer(rw, a.nbytes, a) for name, a in host.items()}
        self.extra, self.keep = [], []
        k = self.k
        k.set_buffer(N.BUFFER_OUT, self.buf["image"])
        self.bind(track.scene)
        k.set_int(N.WIDTH, W)
        k.set_int(N.HEIGHT, H)
        k.set_math_mode(math)
        if hits:    # (with hit buffers bound, fused renders stay in order on the main stream)
            k.set_hit_buffers(self.buf["hit_ids"], self.buf["hit_t"])
        k.set_schedule(self.sched_id(track.sched))
        if path == "global":
            k.force_global_scene(True)
            k.set_tuning("global_oct", 0)
        if track.stats:
            k.set_stats(True)
        if track.range != (0, 0):
            k.set_work_range(*track.range)
        if track.interleave != (1, 0):
            k.set_row_interleave(*track.interleave)
        self.set_frame(track.slot_fc, track.slot_cam)

    def sched_id(self, name):
        N = self.N
        return {"tiles": N.SCHED_TILES, "step": N.SCHED_STEP, "wavefront": N.SCHED_WAVEFRONT}[name]

    def plain_settings(self):
        self.k.set_tuning("perframe_batch", 1)
        self.k.set_tuning("perframe_defer", 0)
        self.k.set_tuning("perframe_sky", 0)
        self.ctx.set_accum_overlap(False)

    def profile(self, name):
        k = self.k
        if name == "queued":
            k.set_tuning("perframe_defer_min", 0)
            k.set_tuning("perframe_sky", 2)
            k.set_tuning("tail_chunk", 64)
        elif name == "deferred":
            k.set_tuning("perframe_defer", 1)
            k.set_tuning("perframe_batch", 1)
        elif name == "exposed":
            self.buf["image"].device_pointer()
            # (only rect copies read this flag and no step makes one: set because a host that takes
            # pointers sets it, inert for this vocabulary)
            self.ctx.set_readback_on_accum_stream(True)
        elif name == "global":
            k.force_global_scene(True)
            k.set_tuning("global_oct", 0)
            k.set_tuning("top_nodes", 5)
        else:
            assert name == "defaults", name

    def bind(self, scene):
        N = self.N
        for slot, b in ((N.BUFFER_SCENE, "tris"), (N.BUFFER_NODE, "nodes"), (N.BUFFER_MATERIAL, "mats")):
            self.k.set_buffer(slot, self.buf[f"{b}:{scene}"])

    def set_frame(self, fc, cam):
        N, k = self.N, self.k
        pos, front, up = CAMERAS[cam]
        k.set_uint(N.FRAME_COUNT, fc)
        k.set_uint(N.FRAME_SEED, FRAME_SEED)
        k.set_int(N.LIGHT_BOUNCES, BOUNCES)
        k.set_int(N.LIGHT_TYPE, 0)
        k.set_float(N.SKYBOX_INTENSITY, 1.0)
        k.set_float3(N.CAMERA_POS, pos)
        k.set_float3(N.CAMERA_FRONT, front)
        k.set_float3(N.CAMERA_UP, up)

    def upload(self, a):
        N = self.N
        b = self.ctx.create_buffer(N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR, a.nbytes, a)
        self.extra.append(b)
        return b

    def do(self, s, t, tune=True):
        """Issue step `s` with the bookkeeping `t` as it stands before the step; returns the status
        (0, or the code of the first call that was refused).  `read`, `finish` and `read_nb` are the
        executors' own."""
        N = self.N
        try:
            self._do(s, t, tune)
        except N.RTError as e:
            return e.code
        return 0

    def _do(self, s, t, tune):
        N, ctx, k, buf, kind = self.N, self.ctx, self.k, self.buf, s.kind
        if kind == "frame":
            self.set_frame(t.next_fc, t.cam)
            ctx.ExecuteKernel(k, NPIX)
        elif kind == "frames":
            self.set_frame(t.next_fc, t.cam)
            ctx.ExecuteKernelFrames(k, NPIX, arg(s, "n"))
        elif kind == "restart":
            self.set_frame(arg(s, "fc"), arg(s, "cam"))
            ctx.ExecuteKernel(k, NPIX)
        elif kind == "write_out":
            data = image_data(arg(s, "seed"))
            self.keep.append(data)
            ctx.WriteBuffer(buf["image"], data, blocking=bool(arg(s, "blocking")))
        elif kind == "write_mat":
            data = np.ascontiguousarray(material_data(t.scene, arg(s, "seed")))
            self.keep.append(data)
            ctx.WriteBuffer(buf[f"mats:{t.scene}"], data, blocking=bool(arg(s, "blocking")))
        elif kind == "move":
            pos, nrm = move_data(t.scene, s)
            pb = self.upload(pos)
            nb = self.upload(nrm) if nrm is not None else None
            ctx.UpdateVertices(buf[f"tris:{t.scene}"], arg(s, "first"), arg(s, "n"), pb, nb)
            ctx.RefitBVH(k)
        elif kind == "rebind":
            self.bind("big" if t.scene == "cornell" else "cornell")
        elif kind == "query":
            first = arg(s, "first")
            ctx.IntersectRays(k, buf["rays"], buf["qhits"], N_RAYS - first,
                              N.QUERY_ANY if arg(s, "mode") else N.QUERY_CLOSEST, first)
        elif kind == "camera_rays":
            ctx.CameraRays(k, NPIX, buf["camrays"])
        elif kind == "surfaces":
            first = t.query[0]
            ctx.HitSurfaces(k, buf["rays"], buf["qhits"], buf["surfaces"], N_RAYS - first, first)
        elif kind == "features":
            ctx.FrameFeatures(k, NPIX, arg(s, "n"), buf[f"feat{t.feature_target()}"])
        elif kind == "denoise":
            w, h = SC.DENOISE_VIEWS[arg(s, "view")]
            ctx.Denoise(k, buf["image"], buf[f"feat{t.feat}"], w, h, buf["denoise"], iterations=arg(s, "iterations"))
        elif kind == "temporal":
            cur_view = CAMERAS[t.feat_cam[t.feat]]
            if t.hist is None:
                hist = hist_feat = None
                prev_view = cur_view
            else:
                hist, hist_feat, prev_view = buf[f"temp{t.hist[0]}"], buf[f"feat{t.hist[1]}"], CAMERAS[t.hist[2]]
            ctx.TemporalAccumulate(k, buf["image"], buf[f"feat{t.feat}"], hist, hist_feat, W, H,
                                   buf[f"temp{t.temporal_target()}"], cur_view, prev_view)
        elif kind == "sched":
            k.set_schedule(self.sched_id(arg(s, "to")))
        elif kind == "range":
            k.set_work_range(arg(s, "first"), arg(s, "last"))
        elif kind == "interleave":
            k.set_row_interleave(arg(s, "period"), arg(s, "phase"))
        elif kind == "tune":
            if tune:
                k.set_tuning(arg(s, "knob"), arg(s, "value"))
        elif kind == "stats":
            k.set_stats(not t.stats)
        else:
            raise AssertionError(kind)

    def read(self, name):
        out = np.empty_like(self.host0[name])
        self.ctx.ReadBuffer(self.buf[name], out, blocking=True)
        return out

    def snapshot(self):
        return {name: self.read(name) for name in OBSERVED}

    def counters(self):
        st = self.k.stats()
        return np.array([st[c] for c in COUNTERS], np.uint64)

    def per_frame(self, fc, cam, n_frames, scene, math):
        """The public per-frame calls behind a feature pass, on a kernel of their own: per frame the
        camera rays, their closest hits and the hits' surfaces."""
        import clrt
        N = self.N
        k = clrt.CLKernel(self.ctx, "KernelEntry")
        out = []
        try:
            for slot, b in ((N.BUFFER_SCENE, "tris"), (N.BUFFER_NODE, "nodes"), (N.BUFFER_MATERIAL, "mats")):
                k.set_buffer(slot, self.buf[f"{b}:{scene}"])
            k.set_int(N.WIDTH, W)
            k.set_int(N.HEIGHT, H)
            k.set_math_mode(math)
            pos, front, up = CAMERAS[cam]
            k.set_float3(N.CAMERA_POS, pos)
            k.set_float3(N.CAMERA_FRONT, front)
            k.set_float3(N.CAMERA_UP, up)
            rb = self.upload(np.zeros(NPIX, N.RAY_DTYPE))
            hb = self.upload(np.zeros(NPIX, N.RAY_HIT_DTYPE))
            sb = self.upload(np.zeros(NPIX, N.SURFACE_DTYPE))
            for j in range(n_frames):
                k.set_uint(N.FRAME_COUNT, fc + j)
                self.ctx.CameraRays(k, NPIX, rb)
                self.ctx.IntersectRays(k, rb, hb, NPIX)
                self.ctx.HitSurfaces(k, rb, hb, sb, NPIX)
                got = []
                for b, dt in ((rb, N.RAY_DTYPE), (hb, N.RAY_HIT_DTYPE), (sb, N.SURFACE_DTYPE)):
                    a = np.empty(NPIX, dt)
                    self.ctx.ReadBuffer(b, a, blocking=True)
                    got.append(a)
                out.append(tuple(got))
        finally:
            k.release()
        return out

    def close(self):
        self.ctx.Finish()
        for b in self.extra + list(self.buf.values()):
            b.release()
        self.k.release()
        self.ctx.release()


class Run:
    """What an executor saw: `obs`, a list of (type, step index, {buffer: array}) in script order --
    type "read" (a `read` step), "read_nb", "end"; the plain replay also keeps `steps`, every buffer
    after every step."""

    def __init__(self):
        self.obs, self.steps, self.prepares, self.extra = [], [], None, {}


def run_live(session, profile, math, hits=True):
    """`hits` False: no primary-hit buffers are bound (fused renders then rotate through the context's
    render streams) and the two buffers are left out of the observations."""
    t = SC.Track()
    rig = Rig(initial_host(), t, math, "auto", hits=hits)
    run = Run()
    try:
        rig.profile(profile)
        status, pending = [], []

        def waited():
            for i, dest in pending:
                run.obs.append(("read_nb", i, {"image": dest}))
            pending.clear()

        def observe(kind, i):
            snap = rig.snapshot()          # the first blocking read is the host's wait
            waited()
            snap["status"] = np.array(status, np.int64)
            if not hits:
                del snap["hit_ids"], snap["hit_t"]
            if t.stats:
                snap["counters"] = rig.counters()
            run.obs.append((kind, i, snap))

        for i, s in enumerate(session):
            if s.kind == "read":
                observe("read", i)
            elif s.kind == "finish":
                rig.ctx.Finish()
                waited()
            elif s.kind == "read_nb":
                dest = np.zeros((NPIX, 4), np.float32)
                rig.ctx.ReadBuffer(rig.buf["image"], dest, blocking=False)
                pending.append((i, dest))
            else:
                held = s.kind == "tune" and arg(s, "knob") in PROFILE_KNOBS[profile]
                status.append(rig.do(s, t, tune=not held))
                if s.kind in ("write_out", "write_mat") and arg(s, "blocking"):
                    waited()
            t.apply(s)
        observe("end", len(session))
        run.obs.sort(key=lambda o: o[1])
        run.prepares = rig.k.scene_prepares()
    finally:
        rig.close()
    return run


def run_plain(session, math, path="auto", tie_features=False, keep_steps=False):
    t = SC.Track()
    host = initial_host()
    run = Run()
    status = []
    counters = np.zeros(4, np.uint64)
    for i, s in enumerate(session):
        if s.kind in ("read", "finish", "read_nb"):
            snap = dict(host)
        else:
            rig = Rig(host, t, math, path)
            try:
                rig.plain_settings()
                status.append(rig.do(s, t, tune=False))
                rig.ctx.Finish()
                snap = rig.snapshot()
                if t.stats:
                    counters = counters + rig.counters()
                if tie_features and s.kind == "features" and not t.refused(s):
                    run.extra[i] = rig.per_frame(t.slot_fc, t.slot_cam, arg(s, "n"), t.scene, math)
            finally:
                rig.close()
            for name in OBSERVED:      # unchanged buffers share one array
                if snap[name].tobytes() == host[name].tobytes():
                    snap[name] = host[name]
            snap["rays"] = host["rays"]
        host = snap
        rec = dict(snap)
        rec["status"] = np.array(status, np.int64)
        if keep_steps:
            run.steps.append(rec)
        t.apply(s)
        if s.kind == "read_nb":
            run.obs.append(("read_nb", i, {"image": host["image"]}))
        if s.kind == "read":
            run.obs.append(("read", i, _observation(rec, t, counters)))
    run.obs.append(("end", len(session), _observation(rec, t, counters)))
    return run


def _observation(rec, t, counters):
    o = {name: rec[name] for name in OBSERVED + ("status",)}
    if t.stats:
        o["counters"] = counters.copy()
    return o


# ---- live against plain ---------------------------------------------------------------------------
class Mismatch:
    def __init__(self, index, message):
        self.index, self.message = index, message

    def __str__(self):
        return self.message


def _words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(-1) if a.nbytes % 4 else a.view(np.uint32).reshape(-1)


def compare(live, plain, session, label, profile, skip=()):
    """None when every observation of the live run equals the plain replay's, else a Mismatch: the
    first observation that differs, its first differing buffer, the count of differing elements and
    the script since the last matching observation.  Observations pair up by type and ordinal, so a
    replay of a shortened script is compared as far as it goes.  `skip`: buffers the live run did not
    observe."""
    by_ordinal, seen = {}, {}
    for kind, i, o in plain.obs:
        n = seen[kind] = seen.get(kind, 0) + 1
        by_ordinal[(kind, n)] = o
    seen, last_ok = {}, 0
    for kind, i, o in live.obs:
        n = seen[kind] = seen.get(kind, 0) + 1
        want = by_ordinal.get((kind, n))
        what = None
        if want is None:
            what = "the replay has no such observation"
        else:
            for name in sorted((set(o) | set(want)) - set(skip)):
                if name not in o or name not in want:
                    what = f"buffer {name}: observed by one run only"
                    break
                a, b = _words(o[name]), _words(want[name])
                if a.shape != b.shape:
                    what = f"buffer {name}: {a.size} against {b.size} words"
                    break
                if not np.array_equal(a, b):
                    bad = np.flatnonzero(a != b)
                    what = f"buffer {name}: {bad.size} of {a.size} words differ, first at {int(bad[0])}"
                    break
        if what is not None:
            since = SC.text(session[last_ok:min(i + 1, len(session))])
            return Mismatch(i, f"session {label}, profile {profile}: observation '{kind}' at step {i} differs from "
                               f"the plain replay -- {what}\nsteps since the last matching observation "
                               f"(from {last_ok}):\n{since}")
        if kind != "read_nb":
            last_ok = i
    return None


# ---- the CPU references against the plain replay ---------------------------------------------------
def rendered_mask(rng, interleave):
    """The work-items a launch renders: [first, last) of the work range, and with a band interleave
    the 8-row bands b of the range's rows (counted from its first row) with b % period == phase."""
    g0, g1 = min(rng[0], NPIX), (min(rng[1], NPIX) if rng[1] else NPIX)
    m = np.zeros(NPIX, bool)
    if g1 <= g0:
        return m, g0, g1
    m[g0:g1] = True
    period, phase = interleave
    if period > 1:
        row = np.arange(NPIX) // W
        m &= ((row - g0 // W) // 8) % period == phase
    return m, g0, g1


class CpuModel:
    """The session on the CPU: the scenes as numpy arrays (updated by move / write_mat / rebind) and
    the image through oracle.render.  step() advances it by one step and returns what the oracle says
    about a frame step's primary hits (else None)."""

    def __init__(self):
        import oracle
        oracle.build()
        self.oracle = oracle
        sc = scenes()
        self.scene = {n: types.SimpleNamespace(triangles=s.triangles.copy(), nodes=s.nodes.copy(),
                                               materials=s.materials.copy()) for n, s in sc.items()}
        self.image = np.zeros((NPIX, 4), np.float32)

    def render(self, scene, fcs, cam, rng, interleave, bounces=BOUNCES):
        """Frames `fcs` accumulated into self.image over the launch's work-items; -> (mask, ids, t) of
        the last frame."""
        mask, g0, g1 = rendered_mask(rng, interleave)
        ids = t = None
        if not mask.any():
            return mask, ids, t
        for fc in fcs:
            work = self.image.copy()
            work, ids, t, _ = self.oracle.render(self.scene[scene], W, H, frame_count=fc, light_bounces=bounces,
                                                 camera=CAMERAS[cam], result=work, first=g0, last=g1, want_hits=True,
                                                 threads=8)
            self.image[mask] = work[mask]
        return mask, ids, t

    def step(self, s, t):
        k = s.kind
        if k in ("frame", "frames"):
            fcs = [t.next_fc + j for j in range(arg(s, "n", 1))]
            return self.render(t.scene, fcs, t.cam, t.range, t.interleave)
        if k == "restart":
            return self.render(t.scene, [arg(s, "fc")], arg(s, "cam"), t.range, t.interleave)
        if k == "write_out":
            self.image = image_data(arg(s, "seed"))
        elif k == "write_mat":
            self.scene[t.scene].materials = material_data(t.scene, arg(s, "seed"))
        elif k == "move":
            sc = self.scene[t.scene]
            apply_move(sc.triangles, s, *move_data(t.scene, s))
            lo, hi = R.fold_bounds(sc.triangles, sc.nodes)
            sc.nodes["bmin"][:len(lo), :3] = lo
            sc.nodes["bmax"][:len(hi), :3] = hi
        return None


def cpu_image_observations(session):
    """The CPU model of the image alone: its bytes at every `read` and at the session's end."""
    m, t, out = CpuModel(), SC.Track(), []
    for s in session:
        m.step(s, t)
        if s.kind == "read":
            out.append(rgb(m.image).tobytes())
        t.apply(s)
    out.append(rgb(m.image).tobytes())
    return out


def _same(got, want, what):
    a, b = _words(got), _words(want)
    assert a.shape == b.shape and np.array_equal(a, b), \
        f"{what}: {int((a != b).sum()) if a.shape == b.shape else 'all'} of {a.size} words differ"


def check_plain_against_cpu(session, plain, label):
    """The plain replay's recorded steps (pinned math, tie_features=True) against the CPU references,
    step by step: each step's result from the inputs recorded before it."""
    from ray_query_ref import SceneWalker
    N = _N()
    m, t = CpuModel(), SC.Track()
    prev = initial_host()
    n_status = 0
    for i, s in enumerate(session):
        rec, k = plain.steps[i], s.kind
        where = f"session {label}, step {i} ({SC.text([s])})"
        sc = m.scene[t.scene]
        if k not in ("read", "finish", "read_nb"):
            st = int(rec["status"][n_status])
            n_status += 1
            assert st == (INVALID_OPERATION if t.refused(s) else 0), f"{where}: status {st}"
        m.image = prev["image"].copy()      # the same result buffer the device accumulated into
        hits = m.step(s, t)
        changed = set()
        if k in ("frame", "frames", "restart"):
            mask, ids, tt = hits
            _same(rgb(rec["image"]), rgb(m.image), f"{where}: image against oracle.render")
            _same(rec["image"][~mask], prev["image"][~mask], f"{where}: pixels outside the launch")
            if not mask.any():              # a band phase the work range's rows do not reach: no launch
                ids, tt = prev["hit_ids"], prev["hit_t"]
            _same(rec["hit_ids"][mask], ids[mask], f"{where}: primary hit ids")
            _same(rec["hit_t"][mask][ids[mask] >= 0], tt[mask][ids[mask] >= 0], f"{where}: primary hit t")
            _same(rec["hit_ids"][~mask], prev["hit_ids"][~mask], f"{where}: hit ids outside the launch")
            changed = {"image", "hit_ids", "hit_t"}
        elif k == "write_out":
            _same(rec["image"], m.image, f"{where}: image")
            changed = {"image"}
        elif k == "write_mat":
            _same(rec[f"mats:{t.scene}"], sc.materials, f"{where}: materials")
            changed = {f"mats:{t.scene}"}
        elif k == "move":
            nodes, before = rec[f"nodes:{t.scene}"], prev[f"nodes:{t.scene}"]
            _same(rec[f"tris:{t.scene}"], sc.triangles, f"{where}: triangles")
            lo, hi = R.fold_bounds(sc.triangles, before)
            assert (np.array_equal(nodes["bmin"][:len(lo), :3], lo) and
                    np.array_equal(nodes["bmax"][:len(hi), :3], hi)), \
                f"{where}: node bounds against fold_bounds"
            R.assert_only_bounds_changed(before, nodes)
            sc.nodes = nodes.copy()         # (the sign of a zero bound is the device's to choose)
            changed = {f"tris:{t.scene}", f"nodes:{t.scene}"}
        elif k == "query" and not t.refused(s):
            first = arg(s, "first")
            prim, tq, _, _ = SceneWalker(sc).walk_rays(prev["rays"][first:], any_hit=bool(arg(s, "mode")))
            _same(rec["qhits"]["prim"][first:], prim, f"{where}: prim against SceneWalker")
            _same(rec["qhits"]["t"][first:], tq, f"{where}: t against SceneWalker")
            _same(rec["qhits"][:first], prev["qhits"][:first], f"{where}: slots before `first`")
            changed = {"qhits"}
        elif k == "surfaces" and not t.refused(s):
            first = t.query[0]
            want = surface_ref.surfaces(sc.triangles, prev["rays"], prev["qhits"])
            _same(rec["surfaces"][first:], want[first:], f"{where}: against surface_ref.surfaces")
            _same(rec["surfaces"][:first], prev["surfaces"][:first], f"{where}: slots before `first`")
            changed = {"surfaces"}
        elif k == "features" and not t.refused(s):
            frames = []
            for j, (rays, fh, surf) in enumerate(plain.extra[i]):
                m.image = np.zeros((NPIX, 4), np.float32)
                _, ids, tt = m.render(t.scene, [(t.slot_fc + j) & 0xFFFFFFFF], t.slot_cam, (0, 0), (1, 0), bounces=1)
                _same(fh["prim"], ids, f"{where}: frame {j}: camera-ray hits against the oracle's primary hits")
                _same(fh["t"][ids >= 0], tt[ids >= 0], f"{where}: frame {j}: hit t")
                _same(surf, surface_ref.surfaces(sc.triangles, rays, fh), f"{where}: frame {j}: surfaces")
                frames.append((fh, surf))
            name = f"feat{t.feature_target()}"
            _same(rec[name], surface_ref.fold_features(frames, sc.materials, arg(s, "n")), f"{where}: fold_features")
            changed = {name}
        elif k == "camera_rays":
            # the record's fixed fields in full; the directions through every 7th ray (7 and the width
            # share no factor: every column), walked on the CPU against the oracle's primary hits
            cr = rec["camrays"]
            _same(cr["origin"], np.tile(np.float32(CAMERAS[t.slot_cam][0]), (NPIX, 1)), f"{where}: origins")
            _same(cr["tmin"], np.full(NPIX, -np.inf, np.float32), f"{where}: tmin")
            _same(cr["tmax"], np.full(NPIX, 100000.0, np.float32), f"{where}: tmax")
            m.image = np.zeros((NPIX, 4), np.float32)
            _, ids, tt = m.render(t.scene, [t.slot_fc], t.slot_cam, (0, 0), (1, 0), bounces=1)
            prim, tq, _, _ = SceneWalker(sc).walk_rays(cr[::7])
            _same(prim, ids[::7], f"{where}: camera rays' hits against the oracle's primary hits")
            _same(tq[prim >= 0], tt[::7][prim >= 0], f"{where}: camera rays' hit t")
            changed = {"camrays"}
        elif k == "denoise":
            w, h = SC.DENOISE_VIEWS[arg(s, "view")]
            want = denoise_ref.denoise(prev["image"][:w * h], prev[f"feat{t.feat}"][:w * h], w, h,
                                       iterations=arg(s, "iterations"))
            _same(rec["denoise"][:w * h], want.reshape(-1, 4), f"{where}: against denoise_ref.denoise")
            _same(rec["denoise"][w * h:], prev["denoise"][w * h:], f"{where}: slots past the view")
            changed = {"denoise"}
        elif k == "temporal":
            cur_view = CAMERAS[t.feat_cam[t.feat]]
            hist = hist_feat = None
            prev_view = cur_view
            if t.hist is not None:
                hist, hist_feat, prev_view = prev[f"temp{t.hist[0]}"], prev[f"feat{t.hist[1]}"], CAMERAS[t.hist[2]]
            want = temporal_ref.temporal(prev["image"], prev[f"feat{t.feat}"], hist, hist_feat, W, H, cur_view,
                                         prev_view)
            name = f"temp{t.temporal_target()}"
            _same(rec[name], want.reshape(-1, 4), f"{where}: against temporal_ref.temporal")
            changed = {name}
        for name in OBSERVED:               # a step writes nothing but its own results
            if name not in changed:
                _same(rec[name], prev[name], f"{where}: {name} must not change")
        prev = rec
        t.apply(s)

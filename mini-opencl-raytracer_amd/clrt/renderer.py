"""CLRaytracer without the GL/ImGui half (/root/reference/CLRaytracer.h:14-40).

Init -> SetupBuffers -> (scene upload = CLBVHScene::SetupBuffers) -> RenderFrame, with
the reference's defaults: m_FrameCount starts at 1, lightBounces 9, lightType 0,
skyboxIntensity 1.0 (CLRaytracer.h:30-34) and the CLCamera defaults
(CLcamera.h:8-10).  RenderFrame sets the per-frame uniforms (CLRaytracer.cpp:35-47),
executes W*H work-items, reads the output back and finishes (:51-56), then increments
the frame counter (:101).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from . import _native as N
from .device import Buffer, CLContext, CLKernel
from .scene import Scene


@dataclass
class Camera:
    """CLCamera defaults (CLcamera.h:8-10)."""
    position: tuple = (0.0, -25.0, 8.5)
    front: tuple = (0.0, 1.0, 0.0)
    up: tuple = (0.0, 0.0, 1.0)


@dataclass
class Raytracer:
    width: int
    height: int
    device: int = 0
    frame_count: int = 1          # m_FrameCount
    light_type: int = 0           # lightType
    light_bounces: int = 9        # lightBounces
    skybox_intensity: float = 1.0  # skyboxIntensity
    frame_seed: int = 0           # rand() in the reference; unused by the kernel
    camera: Camera = field(default_factory=Camera)
    read_back: bool = True        # RenderFrame reads the image back every frame

    def __post_init__(self):
        self.ctx: CLContext | None = None
        self.kernel: CLKernel | None = None
        self.output: Buffer | None = None
        self.pixels = np.zeros((self.height * self.width, 4), np.float32)
        self._shadow_rays = False             # shadow_rays before Init()
        self._scene_bufs: list = []
        self._cast_bufs: tuple | None = None  # (capacity in rays, ray buffer, hit buffer) of cast()
        self._surf_buf: tuple | None = None   # (capacity in records, surface buffer) of surfaces()
        self._trace_bufs: tuple | None = None  # (capacity in records, ray, seed and result buffers) of trace()
        self._adaptive: dict | None = None    # render_adaptive(): statistics, selected list, result, image
        self._sample_frame = 1                # render_adaptive(): FRAME_COUNT of the next sample
        self._feat_buf: Buffer | None = None  # features(): width * height records
        self._denoise_buf: Buffer | None = None  # denoise(): the filtered image, width * height slots
        self._sample_denoise: dict | None = None  # denoise_adaptive(): the filtered image and its variance plane
        self._reproject_feat: list = [None, None]  # reproject_samples(): the previous and the current view's features
        self._temporal_feat: list = [None, None]  # temporal(): this call's and the previous call's features
        self._temporal_img: list = [None, None]   # ... and outputs; index _temporal_at is the history
        self._temporal_at = 0
        self._temporal_view: tuple | None = None  # the camera of the last temporal() (None: no history)
        self._move_bufs: tuple | None = None  # (capacity in triangles, positions, normals) of move_vertices()
        self._move_keep: list = []            # host arrays of uploads still in the queue
        # move_vertices(keep_previous=True): the vertices before the move ("pos", "nrm"; "live" while they are
        # the scene's previous state), who has used them ("used"), whether the sample statistics' features
        # were taken with them ("feat": their n_frames, or None), and FrameMotion's records ("records")
        self._motion: dict | None = None

    # CLRaytracer::Init (CLRaytracer.cpp:104-120)
    def Init(self) -> None:
        self.ctx = CLContext(self.device)
        self.kernel = CLKernel(self.ctx, "KernelEntry")
        self.kernel.set_shadow_rays(self._shadow_rays)
        self.SetupBuffers()

    @property
    def shadow_rays(self) -> bool:
        """Shadow rays for the analytic light (rtKernelSetShadowRays): trace(), render_adaptive() and whatever
        else goes through TracePaths or SamplePixels follow it; RenderFrame and the other KernelEntry renders
        stay the reference's.  Default False."""
        return self.kernel.get_shadow_rays() if self.kernel is not None else self._shadow_rays

    @shadow_rays.setter
    def shadow_rays(self, enable: bool) -> None:
        self._shadow_rays = bool(enable)
        if self.kernel is not None:
            self.kernel.set_shadow_rays(self._shadow_rays)

    # CLRaytracer::SetupBuffers (CLRaytracer.cpp:122-137)
    def SetupBuffers(self) -> None:
        k = self.kernel
        k.set_int(N.WIDTH, self.width)
        k.set_int(N.HEIGHT, self.height)
        self.output = self.ctx.create_buffer(N.MEM_WRITE_ONLY, self.width * self.height * 16)
        k.set_buffer(N.BUFFER_OUT, self.output)

    # CLBVHScene::SetupBuffers (CLBVHnode.cpp:209-236)
    def upload_scene(self, scene: Scene) -> None:
        flags = N.MEM_READ_ONLY | N.MEM_COPY_HOST_PTR
        # (triangles and nodes read-write: move_vertices updates and refits them on the device)
        rw = N.MEM_READ_WRITE | N.MEM_COPY_HOST_PTR
        tb = self.ctx.create_buffer(rw, scene.triangles.nbytes, scene.triangles)
        nb = self.ctx.create_buffer(rw, scene.nodes.nbytes, scene.nodes)
        mb = self.ctx.create_buffer(flags, scene.materials.nbytes, scene.materials)
        for old in self._scene_bufs:
            old.release()
        self._scene_bufs = [tb, nb, mb]
        self._drop_motion()   # (a snapshot of another scene's vertices)
        self.kernel.set_buffer(N.BUFFER_SCENE, tb)
        self.kernel.set_buffer(N.BUFFER_NODE, nb)
        self.kernel.set_buffer(N.BUFFER_MATERIAL, mb)

    def set_uniforms(self) -> None:
        """CLRaytracer::RenderFrame uniform block (CLRaytracer.cpp:35-47)."""
        k = self.kernel
        k.set_uint(N.FRAME_COUNT, self.frame_count)
        k.set_uint(N.FRAME_SEED, self.frame_seed)
        k.set_int(N.LIGHT_BOUNCES, self.light_bounces)
        k.set_int(N.LIGHT_TYPE, self.light_type)
        k.set_float(N.SKYBOX_INTENSITY, self.skybox_intensity)
        k.set_float3(N.CAMERA_POS, self.camera.position)
        k.set_float3(N.CAMERA_FRONT, self.camera.front)
        k.set_float3(N.CAMERA_UP, self.camera.up)

    # CLRaytracer::RenderFrame (CLRaytracer.cpp:12-102), display half removed
    def RenderFrame(self) -> None:
        self.set_uniforms()
        work = self.width * self.height
        self.ctx.ExecuteKernel(self.kernel, work)
        if self.read_back:
            self.ctx.ReadBuffer(self.output, self.pixels, 16 * work)
        self.ctx.Finish()
        self._move_keep.clear()
        self.frame_count += 1

    def cast(self, origins, dirs, tmin=-np.inf, tmax=100000.0, any_hit: bool = False) -> np.ndarray:
        """Intersect caller rays with the uploaded scene (rtEnqueueIntersectRays): `origins` and `dirs`
        are (n, 3) arrays (directions need not be unit length), `tmin` / `tmax` scalars or (n,) arrays.
        Returns n N.RAY_HIT_DTYPE records {prim, t, u, v}; a miss is {-1, tmax, 0, 0}.  `any_hit` stops
        each walk at its first accepted triangle.  The device buffers are kept and reused."""
        n, rb, hb = self._enqueue_cast(origins, dirs, tmin, tmax, any_hit)
        hits = np.empty(n, N.RAY_HIT_DTYPE)
        if n == 0:
            return hits
        self.ctx.ReadBuffer(hb, hits, blocking=True)
        return hits

    def _enqueue_cast(self, origins, dirs, tmin, tmax, any_hit):
        """The rays uploaded into the kept buffers and their query enqueued: (n, ray buffer, hit buffer)."""
        origins = np.asarray(origins, np.float32).reshape(-1, 3)
        dirs = np.asarray(dirs, np.float32).reshape(-1, 3)
        n = len(origins)
        if len(dirs) != n:
            raise ValueError("origins and dirs differ in length")
        if n == 0:
            return 0, None, None
        rays = np.empty(n, N.RAY_DTYPE)
        rays["origin"], rays["dir"] = origins, dirs
        rays["tmin"], rays["tmax"] = tmin, tmax
        if self._cast_bufs is None or self._cast_bufs[0] < n:
            if self._cast_bufs:
                self._cast_bufs[1].release()
                self._cast_bufs[2].release()
            self._cast_bufs = (n, self.ctx.create_buffer(N.MEM_READ_WRITE, n * N.RAY_DTYPE.itemsize),
                               self.ctx.create_buffer(N.MEM_READ_WRITE, n * N.RAY_HIT_DTYPE.itemsize))
        _, rb, hb = self._cast_bufs
        self.ctx.WriteBuffer(rb, rays)
        self.ctx.IntersectRays(self.kernel, rb, hb, n, N.QUERY_ANY if any_hit else N.QUERY_CLOSEST)
        return n, rb, hb

    def surfaces(self, origins, dirs, tmin=-np.inf, tmax=100000.0) -> tuple:
        """cast()'s closest hits and the surface at each (rtEnqueueHitSurfaces): returns (hits, surfaces),
        n N.RAY_HIT_DTYPE and n N.SURFACE_DTYPE records -- position, the shading normal the render uses in
        the kernel's math mode, geometric normal, material index and texture coordinate; a miss has prim
        -1 and material 0xFFFFFFFF.  The hits never leave the device in between; cast()'s buffers are
        reused."""
        n, rb, hb = self._enqueue_cast(origins, dirs, tmin, tmax, False)
        hits = np.empty(n, N.RAY_HIT_DTYPE)
        surf = np.empty(n, N.SURFACE_DTYPE)
        if n == 0:
            return hits, surf
        if self._surf_buf is None or self._surf_buf[0] < n:
            if self._surf_buf:
                self._surf_buf[1].release()
            self._surf_buf = (n, self.ctx.create_buffer(N.MEM_READ_WRITE, n * N.SURFACE_DTYPE.itemsize))
        sb = self._surf_buf[1]
        self.ctx.HitSurfaces(self.kernel, rb, hb, sb, n)
        self.ctx.ReadBuffer(hb, hits)
        self.ctx.ReadBuffer(sb, surf, blocking=True)
        return hits, surf

    def _trace_buffers(self, n: int) -> tuple:
        """The kept (ray, seed, result) buffers of trace() and camera_paths(), at least n records each."""
        if self._trace_bufs is None or self._trace_bufs[0] < n:
            if self._trace_bufs:
                for b in self._trace_bufs[1:]:
                    b.release()
            self._trace_bufs = (n, self.ctx.create_buffer(N.MEM_READ_WRITE, n * N.RAY_DTYPE.itemsize),
                                self.ctx.create_buffer(N.MEM_READ_WRITE, n * 4),
                                self.ctx.create_buffer(N.MEM_READ_WRITE, n * N.PATH_RESULT_DTYPE.itemsize))
        return self._trace_bufs[1:]

    def trace(self, origins, dirs, seeds=None, seed_base: int = 0, tmin=-np.inf, tmax=100000.0,
              encoding: str = "linear") -> tuple:
        """Path-trace caller rays with the renderer's own path tracer (rtEnqueueTracePaths): `origins` and
        `dirs` are (n, 3) arrays (directions need not be unit length), `tmin` / `tmax` scalars or (n,)
        arrays bounding the first segment only.  Ray i starts the reference's Render with the RNG state
        seeds[i] (uint32), or seed_base + i without `seeds`, under the current light_bounces, light_type
        and skybox_intensity.  Returns (radiance float32[n, 3], prim int32[n]): with encoding "linear"
        max(radiance, 0) -- sum these to average samples -- and with "frame0" the value a frame-0 render
        stores; prim is the first segment's hit primitive, -1 on a miss."""
        if encoding not in ("linear", "frame0"):
            raise ValueError("encoding is 'linear' or 'frame0'")
        origins = np.asarray(origins, np.float32).reshape(-1, 3)
        dirs = np.asarray(dirs, np.float32).reshape(-1, 3)
        n = len(origins)
        if len(dirs) != n:
            raise ValueError("origins and dirs differ in length")
        if seeds is not None:
            seeds = np.ascontiguousarray(seeds, np.uint32).reshape(-1)
            if len(seeds) != n:
                raise ValueError("origins and seeds differ in length")
        res = np.empty(n, N.PATH_RESULT_DTYPE)
        if n == 0:
            return res["radiance"].copy(), res["prim"].copy()
        rays = np.empty(n, N.RAY_DTYPE)
        rays["origin"], rays["dir"] = origins, dirs
        rays["tmin"], rays["tmax"] = tmin, tmax
        self.set_uniforms()
        rb, sb, ob = self._trace_buffers(n)
        self.ctx.WriteBuffer(rb, rays)
        if seeds is not None:
            self.ctx.WriteBuffer(sb, seeds)
        self.ctx.TracePaths(self.kernel, rb, ob, n, seeds=sb if seeds is not None else None, seed_base=seed_base,
                            encoding=N.TRACE_FRAME0 if encoding == "frame0" else N.TRACE_LINEAR)
        self.ctx.ReadBuffer(ob, res, blocking=True)
        return res["radiance"].copy(), res["prim"].copy()

    def camera_paths(self) -> tuple:
        """The camera's primary rays of frame frame_count with their RNG states (rtEnqueueCameraPaths):
        (rays, seeds), width * height N.RAY_DTYPE records and uint32 seeds.  trace(rays["origin"],
        rays["dir"], seeds) continues exactly the paths RenderFrame traces for that frame."""
        self.set_uniforms()
        work = self.width * self.height
        rb, sb, _ = self._trace_buffers(work)
        self.ctx.CameraPaths(self.kernel, work, rb, sb)
        rays = np.empty(work, N.RAY_DTYPE)
        seeds = np.empty(work, np.uint32)
        self.ctx.ReadBuffer(rb, rays)
        self.ctx.ReadBuffer(sb, seeds, blocking=True)
        return rays, seeds

    def _adaptive_buffers(self) -> dict:
        """The kept buffers of render_adaptive(): statistics (zeroed when created), the selected list, the
        select's result and the resolved image."""
        if self._adaptive is None:
            work = self.width * self.height
            mk = self.ctx.create_buffer
            self._adaptive = {"stats": mk(N.MEM_READ_WRITE, work * N.PIXEL_STATS_DTYPE.itemsize),
                              "ids": mk(N.MEM_READ_WRITE, work * 4),
                              "result": mk(N.MEM_READ_WRITE, N.SELECT_RESULT_DTYPE.itemsize),
                              "image": mk(N.MEM_READ_WRITE, work * 16)}
            self.ctx.WriteBuffer(self._adaptive["stats"], np.zeros(work, N.PIXEL_STATS_DTYPE))
        return self._adaptive

    def render_adaptive(self, rounds: int, samples_per_round: int = 1, threshold: float = 0.05, floor_y: float = 0.01,
                        min_samples: int = 4, max_samples: int = 64, radius: int = 1, on_sample=None,
                        fused: bool = False, sync_every: int = 1) -> tuple:
        """Progressive rendering that puts its paths where the noise is.  Per round the device selects the
        pixels that still need samples (rtEnqueueSelectPixels: fewer than min_samples, or within `radius`
        of a pixel whose mean luminance has a relative standard error above `threshold`, and fewer than
        max_samples), the host reads the 16-B result and stops when nothing is selected; then
        samples_per_round times the selected pixels get one more path each: FRAME_COUNT is set to a kept
        sample-frame counter (1, 2, ...), and rtEnqueueCameraPathsFor, rtEnqueueTracePaths (linear) and
        rtEnqueueAccumulateSamples run over the list.  At the end the statistics are resolved
        (rtEnqueueResolveSamples) into a kept buffer.  Returns the (H, W, 4) image, whose w slot is the
        pixel's sample count, and a dict: rounds run, paths traced, and the last select's selected / hot.
        The statistics persist across calls: reproject_samples() or reset_samples() after a camera move;
        after move_vertices(keep_previous=True) reproject_samples_motion(), else reset_samples().
        frame_count and BUFFER_OUT are left as they are.  `on_sample(round, sample_frame, n, buffers)` is
        called after each sample's calls are enqueued (buffers: ids, results, stats; for tools and tests).

        fused=True runs each sample as one rtEnqueueSamplePixels launch that takes its record count from the
        select's result on the device: a round is the select, a non-blocking read of the result into that
        round's row of a host array, and the samples; the host waits only after every sync_every-th round and
        at the end, and then stops at the first round it finds with nothing selected.  Rounds enqueued past
        such a round change nothing (every later select finds nothing either), so the statistics, the image
        and the dict are those of fused=False for any sync_every.  on_sample then gets results=None."""
        b = self._adaptive_buffers()
        work = self.width * self.height
        if fused:
            info = self._adaptive_rounds_fused(b, int(rounds), int(samples_per_round), max(1, int(sync_every)), on_sample,
                                               (threshold, floor_y, min_samples, max_samples, radius))
            return self._resolve_adaptive(b), info
        rb, sb, ob = self._trace_buffers(work)
        res = np.zeros(1, N.SELECT_RESULT_DTYPE)
        info = {"rounds": 0, "paths": 0, "selected": 0, "hot": 0}
        at = self.frame_count
        try:
            for rnd in range(int(rounds)):
                self.ctx.SelectPixels(self.kernel, b["stats"], self.width, self.height, b["ids"], b["result"], threshold,
                                      floor_y, min_samples, max_samples, radius)
                self.ctx.ReadBuffer(b["result"], res, blocking=True)
                n = int(res["selected"][0])
                info["selected"], info["hot"] = n, int(res["hot"][0])
                if n == 0:
                    break
                info["rounds"] += 1
                for _ in range(int(samples_per_round)):
                    self.frame_count = self._sample_frame
                    self.set_uniforms()
                    self.ctx.CameraPathsFor(self.kernel, b["ids"], n, rb, sb)
                    self.ctx.TracePaths(self.kernel, rb, ob, n, seeds=sb, encoding=N.TRACE_LINEAR)
                    self.ctx.AccumulateSamples(self.kernel, b["ids"], ob, n, work, b["stats"])
                    if on_sample is not None:
                        on_sample(rnd, self._sample_frame, n, {"ids": b["ids"], "results": ob, "stats": b["stats"]})
                    self._sample_frame += 1
                    info["paths"] += n
        finally:
            self.frame_count = at
            self.kernel.set_uint(N.FRAME_COUNT, at)
        return self._resolve_adaptive(b), info

    def _resolve_adaptive(self, b: dict) -> np.ndarray:
        self.ctx.ResolveSamples(self.kernel, b["stats"], self.width, self.height, b["image"])
        out = np.empty((self.height, self.width, 4), np.float32)
        self.ctx.ReadBuffer(b["image"], out, blocking=True)
        return out

    def _adaptive_rounds_fused(self, b: dict, rounds: int, per_round: int, sync_every: int, on_sample, params) -> dict:
        """render_adaptive(fused=True)'s rounds: queued, with a wait after every sync_every-th one."""
        work = self.width * self.height
        rows = np.zeros(max(rounds, 1), N.SELECT_RESULT_DTYPE)   # row r: round r's select result, once waited for
        info = {"rounds": 0, "paths": 0, "selected": 0, "hot": 0}
        at, frame0 = self.frame_count, self._sample_frame
        seen, done = 0, False
        try:
            for rnd in range(rounds):
                self.ctx.SelectPixels(self.kernel, b["stats"], self.width, self.height, b["ids"], b["result"], *params)
                self.ctx.ReadBuffer(b["result"], rows[rnd:rnd + 1], blocking=False)
                for s in range(per_round):
                    # (the frames of the rounds so far, all of which selected something if this one does)
                    self.frame_count = frame0 + rnd * per_round + s
                    self.set_uniforms()
                    self.ctx.SamplePixels(self.kernel, b["ids"], work, work, b["stats"], count=b["result"])
                    if on_sample is not None:
                        on_sample(rnd, self.frame_count, None, {"ids": b["ids"], "results": None, "stats": b["stats"]})
                if (rnd + 1) % sync_every == 0 or rnd + 1 == rounds:
                    self.ctx.Finish()
                    while seen <= rnd and not done:
                        n = int(rows["selected"][seen])
                        info["selected"], info["hot"] = n, int(rows["hot"][seen])
                        done = n == 0
                        if not done:
                            info["rounds"] += 1
                            info["paths"] += n * per_round
                        seen += 1
                    if done:
                        break
        finally:
            self.ctx.Finish()   # (no read may land in `rows` after this returns)
            self._sample_frame = frame0 + info["rounds"] * per_round
            self.frame_count = at
            self.kernel.set_uint(N.FRAME_COUNT, at)
        return info

    def sample_stats(self) -> np.ndarray:
        """render_adaptive()'s per-pixel statistics as an (H, W) array of N.PIXEL_STATS_DTYPE."""
        out = np.empty((self.height, self.width), N.PIXEL_STATS_DTYPE)
        self.ctx.ReadBuffer(self._adaptive_buffers()["stats"], out, blocking=True)
        return out

    def reset_samples(self) -> None:
        """Zero render_adaptive()'s statistics and restart its sample frames at 1: after a camera move or
        move_vertices() the samples taken so far are of another image.  reproject_samples() carries them
        over instead after a camera move, reproject_samples_motion() after move_vertices(keep_previous=True).
        After a plain move_vertices() this stays the tool, since a reprojection without motion records knows
        the camera's motion only."""
        work = self.width * self.height
        self.ctx.WriteBuffer(self._adaptive_buffers()["stats"], np.zeros(work, N.PIXEL_STATS_DTYPE))
        self._sample_frame = 1

    def reproject_samples(self, prev: Camera, n_frames: int = 4, max_history: float = 16.0,
                          depth_tolerance: float = 0.05, normal_threshold: float = 0.9) -> None:
        """Carry render_adaptive()'s statistics across a camera move (rtEnqueueReprojectSamples), instead
        of reset_samples().  Call it after `camera` was changed, with `prev` the camera the statistics were
        gathered at.  Every pixel of the new view takes the mean, the per-sample variance and the sample
        count (an integer, at most max_history) of the history pixels that show the same surface --
        relative depth within depth_tolerance, normals' dot product at least normal_threshold -- and a
        pixel that finds none (a disocclusion, the image's new margin) is left without samples.  The next
        render_adaptive() round then selects those pixels and the ones that are still noisy, not the
        whole frame; a lower max_history trusts the old samples less.  The guides are the features of
        frames 1 .. n_frames at `prev` and at the current camera.  The result goes into a second kept
        buffer, which becomes render_adaptive()'s statistics buffer (the two swap at every call); the
        sample frames go on counting, so the samples that follow draw fresh seeds.  Nothing is read back;
        the camera, frame_count and BUFFER_OUT are left as they are.
        Moving geometry: this call knows the camera's motion only, so after move_vertices() the choice is
        reset_samples() or, when the move was made with keep_previous=True, reproject_samples_motion()."""
        self._reproject_samples(prev, n_frames, max_history, depth_tolerance, normal_threshold, False)

    def reproject_samples_motion(self, prev: Camera, n_frames: int = 4, max_history: float = 16.0,
                                 depth_tolerance: float = 0.05, normal_threshold: float = 0.9) -> None:
        """reproject_samples() across moved geometry (rtEnqueueReprojectSamplesMotion): the call after
        move_vertices(keep_previous=True), with or without a camera move (`prev` may be the current camera).
        Every pixel's previous point and normal come from rtEnqueueFrameMotion's records over the kept
        vertices, so the statistics follow the surfaces that moved, and the history features are the ones
        move_vertices() took before the move, not recomputed from the moved scene.  The kept vertices then
        count as used by this call; without any (no such move since the last call) the records say where
        the surfaces are now, and the history features are taken at `prev` as reproject_samples() does.
        The arguments and everything else are reproject_samples()'."""
        self._reproject_samples(prev, n_frames, max_history, depth_tolerance, normal_threshold, True)

    def _reproject_samples(self, prev, n_frames, max_history, depth_tolerance, normal_threshold, motion) -> None:
        b = self._adaptive_buffers()
        work = self.width * self.height
        if "spare" not in b:
            b["spare"] = self.ctx.create_buffer(N.MEM_READ_WRITE, work * N.PIXEL_STATS_DTYPE.itemsize)
        for i in range(2):
            if self._reproject_feat[i] is None:
                self._reproject_feat[i] = self.ctx.create_buffer(N.MEM_READ_WRITE,
                                                                 work * N.PIXEL_FEATURES_DTYPE.itemsize)
        hist_feat, cur_feat = self._reproject_feat
        at, cam = self.frame_count, self.camera
        kept = motion and self._motion is not None and self._motion["live"] and self._motion["feat"] is not None \
            and "samples" not in self._motion["used"]
        self.frame_count = 1
        try:
            if not kept:
                self.camera = prev
                try:
                    self._enqueue_features(n_frames, hist_feat)
                finally:
                    self.camera = cam
            self._enqueue_features(n_frames, cur_feat)
        finally:
            self.frame_count = at
            self.set_uniforms()   # (the kernel's camera slots and FRAME_COUNT, whatever was enqueued)
        view = (tuple(cam.position), tuple(cam.front), tuple(cam.up))
        prev_view = (tuple(prev.position), tuple(prev.front), tuple(prev.up))
        mb = self._enqueue_motion("samples") if motion else None
        self.ctx.ReprojectSamples(self.kernel, b["stats"], hist_feat, cur_feat, self.width, self.height, b["spare"],
                                  view, prev_view, max_history, depth_tolerance, normal_threshold, motion=mb)
        b["stats"], b["spare"] = b["spare"], b["stats"]

    def features(self, n_frames: int = 1) -> np.ndarray:
        """First-hit feature buffers for a denoiser (rtEnqueueFrameFeatures): an (H, W) array of
        N.PIXEL_FEATURES_DTYPE -- albedo, depth, normal and coverage averaged over the jittered camera
        rays of frames frame_count .. frame_count + n_frames - 1 at the current camera, the rays
        RenderFrame traces for those frames.  frame_count is left as it is."""
        self._enqueue_features(n_frames)
        out = np.empty((self.height, self.width), N.PIXEL_FEATURES_DTYPE)
        self.ctx.ReadBuffer(self._feat_buf, out, blocking=True)
        return out

    def _enqueue_features(self, n_frames: int, into: Buffer | None = None) -> Buffer:
        """The features of frames frame_count .. frame_count + n_frames - 1 enqueued into the kept buffer
        (or `into`)."""
        self.set_uniforms()
        work = self.width * self.height
        if into is None:
            if self._feat_buf is None:
                self._feat_buf = self.ctx.create_buffer(N.MEM_READ_WRITE, work * N.PIXEL_FEATURES_DTYPE.itemsize)
            into = self._feat_buf
        self.ctx.FrameFeatures(self.kernel, work, n_frames, into)
        return into

    def denoise(self, n_frames: int | None = None, iterations: int = 3, sigma_color: float = 4.0,
                sigma_normal: float = 0.5, sigma_depth: float = 0.1, sigma_albedo: float = 0.25) -> np.ndarray:
        """The accumulated image filtered on the device (rtEnqueueDenoise: an edge-avoiding a-trous wavelet
        filter guided by first-hit albedo, depth, normal and coverage), as an (H, W, 4) float32 array.
        The guides are features() over frames 1 .. n_frames; with n_frames None, over the frames rendered
        so far (frame_count - 1 of them, the first 4096 at the most), whose jittered camera rays are the
        ones the image was averaged over.  The accumulation buffer is only read -- the result goes into
        a kept buffer of its own -- and frame_count stays, so the progressive render goes on.  A sigma
        of 0 turns its edge-stopping term off.  The defaults suit a few frames per pixel; for a single
        frame the colour term mostly sees noise, and sigma_color=0 filtered a 1-frame Cornell box
        better in a host prototype (error 0.47 of the unfiltered image's against 0.78)."""
        if n_frames is None:
            n_frames = min(max(self.frame_count - 1, 1), 4096)
        at = self.frame_count
        self.frame_count = 1
        try:
            fb = self._enqueue_features(n_frames)
        finally:
            self.frame_count = at
            self.kernel.set_uint(N.FRAME_COUNT, at)
        work = self.width * self.height
        if self._denoise_buf is None:
            self._denoise_buf = self.ctx.create_buffer(N.MEM_READ_WRITE, work * 16)
        self.ctx.Denoise(self.kernel, self.output, fb, self.width, self.height, self._denoise_buf, iterations,
                         sigma_color, sigma_normal, sigma_depth, sigma_albedo)
        out = np.empty((self.height, self.width, 4), np.float32)
        self.ctx.ReadBuffer(self._denoise_buf, out, blocking=True)
        return out

    def denoise_adaptive(self, n_frames: int | None = None, iterations: int = 3, sigma_luminance: float = 8.0,
                         sigma_normal: float = 0.5, sigma_depth: float = 0.1, sigma_albedo: float = 0.25,
                         epsilon: float = 1e-4, encoding: str = "gamma", variance: bool = False):
        """render_adaptive()'s statistics filtered on the device (rtEnqueueDenoiseSamples: the a-trous
        filter of denoise() on linear radiance, with a luminance tolerance of `sigma_luminance` standard
        deviations of each pixel's own mean, so that a pixel of few samples is smoothed hard and a
        converged one barely), as an (H, W, 4) float32 array {r, g, b, sample count}, gamma-encoded like
        render_adaptive()'s image or, with encoding "linear", as filtered.  With `variance` the filtered
        variance of the mean luminance comes along as an (H, W) array: (image, variance).  The guides are
        features() over frames 1 .. n_frames at the current camera; with n_frames None, over the sample
        frames taken so far (the first 4096 at the most), whose jittered camera rays are the ones the
        samples were traced along.  The statistics are only read -- the results go into kept buffers of
        their own -- and frame_count stays.  A sigma of 0 turns its edge-stopping term off."""
        if encoding not in ("gamma", "linear"):
            raise ValueError("encoding is 'gamma' or 'linear'")
        if n_frames is None:
            n_frames = min(max(self._sample_frame - 1, 1), 4096)
        b = self._adaptive_buffers()
        at = self.frame_count
        self.frame_count = 1
        try:
            fb = self._enqueue_features(n_frames)
        finally:
            self.frame_count = at
            self.kernel.set_uint(N.FRAME_COUNT, at)
        work = self.width * self.height
        if self._sample_denoise is None:
            self._sample_denoise = {"image": self.ctx.create_buffer(N.MEM_READ_WRITE, work * 16),
                                    "variance": self.ctx.create_buffer(N.MEM_READ_WRITE, work * 4)}
        d = self._sample_denoise
        self.ctx.DenoiseSamples(self.kernel, b["stats"], fb, self.width, self.height, d["image"],
                                d["variance"] if variance else None, iterations, sigma_luminance, sigma_normal,
                                sigma_depth, sigma_albedo, epsilon,
                                N.DENOISE_GAMMA if encoding == "gamma" else N.DENOISE_LINEAR)
        out = np.empty((self.height, self.width, 4), np.float32)
        self.ctx.ReadBuffer(d["image"], out, blocking=True)
        if not variance:
            return out
        var = np.empty((self.height, self.width), np.float32)
        self.ctx.ReadBuffer(d["variance"], var, blocking=True)
        return out, var

    def temporal(self, n_frames: int | None = None, max_history: float = 32.0, depth_tolerance: float = 0.05,
                 normal_threshold: float = 0.9, motion: bool = False) -> np.ndarray:
        """The accumulated image joined with the result of the previous temporal() call, which is
        reprojected into the current camera on the device (rtEnqueueTemporalAccumulate), as an (H, W, 4)
        float32 array whose w slot is the pixel's sample count (at most max_history, which is raised to
        n_frames where it is below).  A history tap
        counts only where it lies on the same surface: relative depth within depth_tolerance, normals'
        dot product at least normal_threshold.  The guides are the features of frames 1 .. n_frames at
        the current camera, as in denoise(); with n_frames None, of the frames rendered so far.  So after
        a camera move (frame_count = 1 and a few new frames) the converged image is carried over instead
        of thrown away.  The first call, and the first after reset_history(), has no history and returns
        the image with w = n_frames.  The accumulation buffer is only read and frame_count stays, so the
        progressive render goes on.
        Moving geometry: without `motion` the reprojection knows the camera's motion only, so after
        move_vertices() the choice is reset_history() or, when the move was made with keep_previous=True,
        motion=True.  With `motion` every pixel's previous point and normal come from
        rtEnqueueFrameMotion's records over the kept vertices (rtEnqueueTemporalAccumulateMotion), so the
        history follows the moved surfaces; the kept vertices then count as used by this call, and without
        any (no such move since the last call) the records say where the surfaces are now."""
        if n_frames is None:
            n_frames = min(max(self.frame_count - 1, 1), 4096)
        work = self.width * self.height
        for bufs, size in ((self._temporal_feat, N.PIXEL_FEATURES_DTYPE.itemsize), (self._temporal_img, 16)):
            for i in range(2):
                if bufs[i] is None:
                    bufs[i] = self.ctx.create_buffer(N.MEM_READ_WRITE, work * size)
        prev, now = self._temporal_at, 1 - self._temporal_at
        at = self.frame_count
        self.frame_count = 1
        try:
            fb = self._enqueue_features(n_frames, self._temporal_feat[now])
        finally:
            self.frame_count = at
            self.kernel.set_uint(N.FRAME_COUNT, at)
        view = (tuple(self.camera.position), tuple(self.camera.front), tuple(self.camera.up))
        has = self._temporal_view is not None
        mb = self._enqueue_motion("temporal") if motion else None
        self.ctx.TemporalAccumulate(self.kernel, self.output, fb, self._temporal_img[prev] if has else None,
                                    self._temporal_feat[prev] if has else None, self.width, self.height,
                                    self._temporal_img[now], view, self._temporal_view if has else view,
                                    float(n_frames), 0.0, max(float(max_history), float(n_frames)), depth_tolerance,
                                    normal_threshold, motion=mb)
        out = np.empty((self.height, self.width, 4), np.float32)
        self.ctx.ReadBuffer(self._temporal_img[now], out, blocking=True)
        self._temporal_at, self._temporal_view = now, view
        return out

    def reset_history(self) -> None:
        """Drop temporal()'s history: the next call starts from the current image alone."""
        self._temporal_view = None

    def motion(self) -> np.ndarray:
        """The motion records of the current camera's centre rays (rtEnqueueFrameMotion) as an (H, W) array
        of N.PIXEL_MOTION_DTYPE: per pixel the first hit's triangle (-1: none), and where that surface
        point and its normal were before the last move_vertices(keep_previous=True) -- for triangles that
        did not move, and when no vertices are kept, where they are now.  The kept vertices stay unused."""
        mb = self._enqueue_motion(None)
        out = np.empty((self.height, self.width), N.PIXEL_MOTION_DTYPE)
        self.ctx.ReadBuffer(mb, out, blocking=True)
        return out

    def _enqueue_motion(self, user: str | None) -> Buffer:
        """FrameMotion at the current camera into the kept record buffer: over the kept vertices while they
        are live and `user` has not used them yet (they then count as used by it), else with nothing moved."""
        m = self._motion_state()
        if m["records"] is None:
            m["records"] = self.ctx.create_buffer(N.MEM_READ_WRITE,
                                                  self.width * self.height * N.PIXEL_MOTION_DTYPE.itemsize)
        use = m["live"] and user not in m["used"]
        self.set_uniforms()
        self.ctx.FrameMotion(self.kernel, self.width * self.height, m["records"], m["pos"] if use else None,
                             m["nrm"] if use else None, 0, m["n"] if use else 0)
        if use and user is not None:
            m["used"].add(user)
        return m["records"]

    def _motion_state(self) -> dict:
        if self._motion is None:
            self._motion = {"n": 0, "pos": None, "nrm": None, "records": None, "live": False, "used": set(),
                            "feat": None}
        return self._motion

    def _drop_motion(self) -> None:
        if self._motion:
            for key in ("pos", "nrm", "records"):
                if self._motion[key]:
                    self._motion[key].release()
        self._motion = None

    def _keep_previous(self, n_frames: int) -> None:
        """Before a move: the whole triangle array's vertices into the kept buffers (ExtractVertices), unless
        kept vertices that nobody has used yet are still live -- they are then the older "before".  With
        sample statistics, the features at the current camera go into reproject_samples()' history-feature
        buffer, since they must predate the move."""
        m = self._motion_state()
        if m["live"] and not m["used"]:
            return
        n = self._scene_bufs[0].size // N.TRIANGLE_DTYPE.itemsize
        if m["pos"] is None or m["n"] != n:
            for key in ("pos", "nrm"):
                if m[key]:
                    m[key].release()
                m[key] = self.ctx.create_buffer(N.MEM_READ_WRITE, n * N.TRI_POINTS_DTYPE.itemsize)
            m["n"] = n
        self.ctx.ExtractVertices(self._scene_bufs[0], 0, n, m["pos"], m["nrm"])
        m["live"], m["used"], m["feat"] = True, set(), None
        if self._adaptive is not None:
            if self._reproject_feat[0] is None:
                self._reproject_feat[0] = self.ctx.create_buffer(
                    N.MEM_READ_WRITE, self.width * self.height * N.PIXEL_FEATURES_DTYPE.itemsize)
            at = self.frame_count
            self.frame_count = 1
            try:
                self._enqueue_features(n_frames, self._reproject_feat[0])
            finally:
                self.frame_count = at
                self.kernel.set_uint(N.FRAME_COUNT, at)
            m["feat"] = n_frames

    def move_vertices(self, positions, normals=None, first: int = 0, keep_previous: bool = False,
                      feature_frames: int = 4) -> None:
        """Move triangles [first, first + n) of the uploaded scene and refit its BVH on the device
        (rtEnqueueUpdateVertices + rtRefitBVH; nothing waits on the host).  `positions` -- and `normals`
        when given -- are (n, 3, 3) arrays (triangle, vertex, xyz) or n N.TRI_POINTS_DTYPE records, in
        the uploaded triangle order (BVH leaf order).  The tree's topology stays: a caller whose tree has
        degraded after large deformations builds a new one.  The output buffer still holds the frames
        accumulated from the old geometry: the caller restarts the progressive accumulation (frame_count
        = 1), as the reference does on a camera move.  The device buffers are kept and reused.
        What was converged before the move -- temporal()'s history, render_adaptive()'s statistics -- is
        the caller's choice: drop it (reset_history(), reset_samples()), or move with keep_previous=True
        and carry it across with temporal(motion=True) / reproject_samples_motion().  keep_previous
        copies the whole triangle array's vertices aside on the device just ahead of the update
        (rtEnqueueExtractVertices), at the first such move since one of those calls used the copy, so
        several moves between two of them add up to one motion; when sample statistics exist it also takes
        the features of frames 1 .. feature_frames at the current camera, the history features
        reproject_samples_motion() needs from before the move."""
        recs = [self._tri_points(positions)]
        if normals is not None:
            recs.append(self._tri_points(normals))
            if len(recs[1]) != len(recs[0]):
                raise ValueError("positions and normals differ in length")
        n = len(recs[0])
        if n == 0:
            return
        if keep_previous:
            self._keep_previous(feature_frames)
        if self._move_bufs is None or self._move_bufs[0] < n:
            if self._move_bufs:
                self._move_bufs[1].release()
                self._move_bufs[2].release()
            size = n * N.TRI_POINTS_DTYPE.itemsize
            self._move_bufs = (n, self.ctx.create_buffer(N.MEM_READ_WRITE, size),
                               self.ctx.create_buffer(N.MEM_READ_WRITE, size))
        _, pb, nb = self._move_bufs
        self.ctx.WriteBuffer(pb, recs[0], blocking=False)
        if normals is not None:
            self.ctx.WriteBuffer(nb, recs[1], blocking=False)
        self.ctx.UpdateVertices(self._scene_bufs[0], first, n, pb, nb if normals is not None else None)
        self.ctx.RefitBVH(self.kernel)
        # the staging arrays must outlive the asynchronous uploads: kept until the queue is next
        # known to be drained (RenderFrame's Finish; after a few moves without one, a Finish here)
        self._move_keep.extend(recs)
        if len(self._move_keep) > 8:
            self.ctx.Finish()
            self._move_keep.clear()

    @staticmethod
    def _tri_points(a) -> np.ndarray:
        a = np.asarray(a)
        if a.dtype == N.TRI_POINTS_DTYPE:
            return np.ascontiguousarray(a)
        a = np.asarray(a, np.float32).reshape(-1, 3, 3)
        out = np.zeros(len(a), N.TRI_POINTS_DTYPE)
        for i, f in enumerate(("p1", "p2", "p3")):
            out[f][:, :3] = a[:, i]
        return out

    def image(self) -> np.ndarray:
        """Last read-back frame as (H, W, 3); row 0 is the bottom row (GL order)."""
        return self.pixels.reshape(self.height, self.width, 4)[:, :, :3]

    def save(self, path: str) -> None:
        """Write the last read-back frame (.png, else binary .ppm) -- the display step the
        reference does with glTexSubImage2D (CLRaytracer.cpp:64-67)."""
        from . import image
        w = image.write_png if path.lower().endswith(".png") else image.write_ppm
        w(path, self.pixels, self.width, self.height)

    def checkpoint(self, path: str) -> None:
        """Save the render state -- the accumulation buffer and m_FrameCount (include/rt_image.h
        rtiSaveAccum) -- so a progressive render can resume later from the same bits."""
        from . import image
        px = np.empty((self.height * self.width, 4), np.float32)
        self.ctx.ReadBuffer(self.output, px, blocking=True)
        image.save_accum(path, px, self.width, self.height, self.frame_count)

    def resume(self, path: str) -> None:
        """Restore a checkpoint into this (initialised) raytracer: the next RenderFrame continues
        the accumulation exactly where the saved run stopped."""
        from . import image
        px, nf = image.load_accum(path)
        if px.shape[0] != self.width * self.height:
            raise ValueError("checkpoint size differs from this raytracer's")
        self.ctx.WriteBuffer(self.output, px)
        self.pixels[:] = px
        self.frame_count = nf

    def release(self) -> None:
        for b in self._scene_bufs:
            b.release()
        self._scene_bufs = []
        if self._cast_bufs:
            self._cast_bufs[1].release()
            self._cast_bufs[2].release()
            self._cast_bufs = None
        if self._surf_buf:
            self._surf_buf[1].release()
            self._surf_buf = None
        if self._trace_bufs:
            for b in self._trace_bufs[1:]:
                b.release()
            self._trace_bufs = None
        if self._adaptive:
            for b in self._adaptive.values():
                b.release()
            self._adaptive = None
        if self._feat_buf:
            self._feat_buf.release()
            self._feat_buf = None
        if self._denoise_buf:
            self._denoise_buf.release()
            self._denoise_buf = None
        if self._sample_denoise:
            for b in self._sample_denoise.values():
                b.release()
            self._sample_denoise = None
        for bufs in (self._temporal_feat, self._temporal_img, self._reproject_feat):
            for i in range(2):
                if bufs[i]:
                    bufs[i].release()
                    bufs[i] = None
        self._temporal_view = None
        if self._move_bufs:
            self._move_bufs[1].release()
            self._move_bufs[2].release()
            self._move_bufs = None
        self._move_keep = []
        self._drop_motion()
        if self.output:
            self.output.release()
        if self.kernel:
            self.kernel.release()
        if self.ctx:
            self.ctx.release()

"""Python mirror of the reference's device wrapper over librt_hip.so.

``CLContext`` / ``CLKernel`` / ``Buffer`` keep the method names and argument meaning of
/root/reference/CLutils.h:116-145 (ReadBuffer, ExecuteKernel, Finish, SetArgument) and
raise ``RTError`` (the reference's CLException) on any non-zero status.
"""
from __future__ import annotations

import ctypes
import struct

import numpy as np

from . import _native as N
from ._native import RTError, check, hip_lib


def _tuning_id(name: str) -> int:
    for table in (N.TUNING, N.TRACE_TUNING):
        if name in table:
            return table[name]
    return N.PATH_KILL_TUNING[name]


class CLContext:
    """CLContext(platform) (CLutils.cpp:9-35): GPU `device` + one in-order HIP stream."""

    def __init__(self, device: int = 0):
        self._lib = hip_lib()
        h = ctypes.c_void_p()
        check(self._lib.rtCreateContext(int(device), ctypes.byref(h)), "Failed to create context")
        self.handle = h
        self.device = int(device)

    def create_buffer(self, flags: int, size: int, host: np.ndarray | None = None) -> "Buffer":
        return Buffer(self, flags, size, host)

    def ReadBuffer(self, buffer: "Buffer", out: np.ndarray, size: int | None = None,
                   blocking: bool = False) -> None:
        """enqueueReadBuffer(buffer, blocking=false, 0, size, ptr) (CLutils.cpp:37-42)."""
        size = out.nbytes if size is None else int(size)
        if not out.flags["C_CONTIGUOUS"] or size > out.nbytes:
            raise RTError("Failed to read buffer", -30)
        check(self._lib.rtEnqueueReadBuffer(self.handle, buffer.handle, int(blocking), 0, size,
                                            out.ctypes.data), "Failed to read buffer")

    def WriteBuffer(self, buffer: "Buffer", data: np.ndarray, blocking: bool = True) -> None:
        data = np.ascontiguousarray(data)
        check(self._lib.rtEnqueueWriteBuffer(self.handle, buffer.handle, int(blocking), 0, data.nbytes,
                                             data.ctypes.data), "Failed to write buffer")

    def BuildBVH(self, tris: "Buffer", n_tris: int, max_prims_in_node: int, nodes: "Buffer",
                 method: int = N.BVH_PLOC) -> int:
        """rtBuildBVHEx: device-side BVH (PLOC, or the linear BVH) over `tris` (permuted in place);
        returns the node count written to `nodes`."""
        n = ctypes.c_size_t()
        check(self._lib.rtBuildBVHEx(self.handle, tris.handle, int(n_tris), int(max_prims_in_node), int(method),
                                     nodes.handle, ctypes.byref(n)), "Failed to build BVH")
        return int(n.value)

    def CopyToDevicePointer(self, buffer: "Buffer", offset: int, size: int, dst: int) -> None:
        """Device-to-device copy into foreign device memory (e.g. a torch tensor)."""
        check(self._lib.rtEnqueueCopyBufferToPointer(self.handle, buffer.handle, int(offset), int(size),
                                                     ctypes.c_void_p(int(dst))), "Failed to copy buffer")

    def CopyRectToDevicePointer(self, buffer: "Buffer", src_offset: int, src_pitch: int, width: int,
                                rows: int, dst: int, dst_pitch: int) -> None:
        check(self._lib.rtEnqueueCopyBufferRectToPointer(self.handle, buffer.handle, int(src_offset), int(src_pitch),
                                                         int(width), int(rows), ctypes.c_void_p(int(dst)),
                                                         int(dst_pitch)), "Failed to copy rect")

    def CopyRectFromDevicePointer(self, src: int, src_pitch: int, buffer: "Buffer", dst_offset: int,
                                  dst_pitch: int, width: int, rows: int) -> None:
        check(self._lib.rtEnqueueCopyPointerRectToBuffer(self.handle, ctypes.c_void_p(int(src)), int(src_pitch),
                                                         buffer.handle, int(dst_offset), int(dst_pitch), int(width),
                                                         int(rows)), "Failed to copy rect")

    def ExecuteKernel(self, kernel: "CLKernel", work_size: int) -> None:
        """enqueueNDRangeKernel(kernel, NullRange, NDRange(workSize)) (CLutils.cpp:44-50)."""
        check(self._lib.rtEnqueueKernel(self.handle, kernel.handle, int(work_size)),
              "Failed to enqueue kernel")

    def ExecuteKernelFrames(self, kernel: "CLKernel", work_size: int, n_frames: int) -> None:
        """Extension: frames FRAME_COUNT .. FRAME_COUNT + n_frames - 1 (rtEnqueueKernelFrames),
        bit-identical to n_frames ExecuteKernel calls with those frame counts."""
        check(self._lib.rtEnqueueKernelFrames(self.handle, kernel.handle, int(work_size), int(n_frames)),
              "Failed to enqueue kernel frames")

    def IntersectRays(self, kernel: "CLKernel", rays: "Buffer", hits: "Buffer", n_rays: int,
                      mode: int = N.QUERY_CLOSEST, first: int = 0) -> None:
        """rtEnqueueIntersectRays: rays [first, first + n_rays) of `rays` (N.RAY_DTYPE records) against the
        scene bound to `kernel`, answered into the same slots of `hits` (N.RAY_HIT_DTYPE)."""
        check(self._lib.rtEnqueueIntersectRays(self.handle, kernel.handle, rays.handle, int(first), int(n_rays),
                                               int(mode), hits.handle), "Failed to enqueue ray query")

    def CameraRays(self, kernel: "CLKernel", work_size: int, rays: "Buffer") -> None:
        """rtEnqueueCameraRays: the primary ray KernelEntry would trace for each work-item, as N.RAY_DTYPE
        records (work range and row interleave ignored)."""
        check(self._lib.rtEnqueueCameraRays(self.handle, kernel.handle, int(work_size), rays.handle),
              "Failed to enqueue camera rays")

    def TracePaths(self, kernel: "CLKernel", rays: "Buffer", out: "Buffer", n: int, seeds: "Buffer | None" = None,
                   seed_base: int = 0, encoding: int = N.TRACE_LINEAR, first: int = 0) -> None:
        """rtEnqueueTracePaths: the reference's Render for records [first, first + n) of `rays` (N.RAY_DTYPE)
        against the scene, materials and light slots bound to `kernel`, into the same slots of `out`
        (N.PATH_RESULT_DTYPE).  Record i starts with seeds[i], or seed_base + i without `seeds`."""
        params = N.TRACE_PARAMS(int(seed_base) & 0xffffffff, int(encoding))
        check(self._lib.rtEnqueueTracePaths(self.handle, kernel.handle, rays.handle, seeds.handle if seeds else None,
                                            int(first), int(n), ctypes.byref(params), out.handle),
              "Failed to enqueue path trace")

    def CameraPaths(self, kernel: "CLKernel", work_size: int, rays: "Buffer", seeds: "Buffer") -> None:
        """rtEnqueueCameraPaths: CameraRays' records plus, per work-item, the RNG state after CreateRay's
        two draws (uint32), so that TracePaths over both continues KernelEntry's path."""
        check(self._lib.rtEnqueueCameraPaths(self.handle, kernel.handle, int(work_size), rays.handle, seeds.handle),
              "Failed to enqueue camera paths")

    def AccumulateSamples(self, kernel: "CLKernel", ids: "Buffer | None", results: "Buffer", n: int, n_pixels: int,
                          stats: "Buffer", first: int = 0) -> None:
        """rtEnqueueAccumulateSamples: the linear radiances of records [first, first + n) of `results`
        (N.PATH_RESULT_DTYPE) added to the statistics (N.PIXEL_STATS_DTYPE) of pixels ids[i] (uint32; without
        `ids`, of pixel i); out-of-range ids and non-finite samples are skipped."""
        check(self._lib.rtEnqueueAccumulateSamples(self.handle, kernel.handle, ids.handle if ids is not None else None,
                                                   results.handle, int(first), int(n), int(n_pixels), stats.handle),
              "Failed to enqueue sample accumulation")

    def SelectPixels(self, kernel: "CLKernel", stats: "Buffer", width: int, height: int, ids: "Buffer",
                     result: "Buffer", threshold: float = 0.05, floor_y: float = 0.01, min_samples: int = 4,
                     max_samples: int = 64, radius: int = 1) -> None:
        """rtEnqueueSelectPixels: the pixels of the width x height statistics that still need samples, as
        ascending uint32 indices at the head of `ids`; `result` (N.SELECT_RESULT_DTYPE) receives their
        number and the number of hot pixels."""
        params = N.ADAPTIVE_PARAMS(float(threshold), float(floor_y), int(min_samples), int(max_samples), int(radius))
        check(self._lib.rtEnqueueSelectPixels(self.handle, kernel.handle, stats.handle, int(width), int(height),
                                              ctypes.byref(params), ids.handle, result.handle),
              "Failed to enqueue pixel selection")

    def CameraPathsFor(self, kernel: "CLKernel", ids: "Buffer", n: int, rays: "Buffer", seeds: "Buffer",
                       first: int = 0) -> None:
        """rtEnqueueCameraPathsFor: CameraPaths' ray and seed of work-item ids[i] into records i of
        [first, first + n)."""
        check(self._lib.rtEnqueueCameraPathsFor(self.handle, kernel.handle, ids.handle, int(first), int(n), rays.handle,
                                                seeds.handle), "Failed to enqueue camera paths")

    def ResolveSamples(self, kernel: "CLKernel", stats: "Buffer", width: int, height: int, out: "Buffer") -> None:
        """rtEnqueueResolveSamples: the statistics as a gamma-encoded {r, g, b, sample count} image, the
        layout rtEnqueueDenoise and rtEnqueueTemporalAccumulate take."""
        check(self._lib.rtEnqueueResolveSamples(self.handle, kernel.handle, stats.handle, int(width), int(height),
                                                out.handle), "Failed to enqueue sample resolve")

    def SamplePixels(self, kernel: "CLKernel", ids: "Buffer", n: int, n_pixels: int, stats: "Buffer",
                     count: "Buffer | None" = None, first: int = 0) -> None:
        """rtEnqueueSamplePixels: one sample for the pixels ids[first, first + m) in one launch -- the camera
        path, its trace and the statistics update -- with m = n, or min(n, the first uint32 of `count`) read on
        the device when the launch runs (a SelectPixels result, no host read in between)."""
        check(self._lib.rtEnqueueSamplePixels(self.handle, kernel.handle, ids.handle,
                                              count.handle if count is not None else None, int(first), int(n),
                                              int(n_pixels), stats.handle), "Failed to enqueue pixel samples")

    def HitSurfaces(self, kernel: "CLKernel", rays: "Buffer", hits: "Buffer", surfaces: "Buffer", n: int,
                    first: int = 0) -> None:
        """rtEnqueueHitSurfaces: the surface (N.SURFACE_DTYPE: position, shading and geometric normal,
        material, texture coordinate) at hits [first, first + n) of `hits` along the same slots of `rays`,
        into the same slots of `surfaces`; nothing is intersected again."""
        check(self._lib.rtEnqueueHitSurfaces(self.handle, kernel.handle, rays.handle, hits.handle, int(first), int(n),
                                             surfaces.handle), "Failed to enqueue hit surfaces")

    def FrameFeatures(self, kernel: "CLKernel", work_size: int, n_frames: int, features: "Buffer") -> None:
        """rtEnqueueFrameFeatures: first-hit albedo, depth, normal and coverage per work-item
        (N.PIXEL_FEATURES_DTYPE), averaged over frames FRAME_COUNT .. FRAME_COUNT + n_frames - 1."""
        check(self._lib.rtEnqueueFrameFeatures(self.handle, kernel.handle, int(work_size), int(n_frames),
                                               features.handle), "Failed to enqueue frame features")

    def Denoise(self, kernel: "CLKernel", image: "Buffer", features: "Buffer", width: int, height: int,
                out: "Buffer", iterations: int = 3, sigma_color: float = 4.0, sigma_normal: float = 0.5,
                sigma_depth: float = 0.1, sigma_albedo: float = 0.25) -> None:
        """rtEnqueueDenoise: `iterations` passes of the edge-avoiding a-trous filter over the width x height
        image of 16-B {r, g, b, w} slots in `image`, guided by the N.PIXEL_FEATURES_DTYPE records of
        `features`, into `out`; a sigma of 0 turns its term off.  Asynchronous; neither input is written."""
        params = N.DENOISE_PARAMS(int(iterations), float(sigma_color), float(sigma_normal), float(sigma_depth),
                                  float(sigma_albedo))
        check(self._lib.rtEnqueueDenoise(self.handle, kernel.handle, image.handle, features.handle, int(width),
                                         int(height), ctypes.byref(params), out.handle), "Failed to enqueue denoise")

    def DenoiseSamples(self, kernel: "CLKernel", stats: "Buffer", features: "Buffer", width: int, height: int,
                       out: "Buffer", variance: "Buffer | None" = None, iterations: int = 3,
                       sigma_luminance: float = 8.0, sigma_normal: float = 0.5, sigma_depth: float = 0.1,
                       sigma_albedo: float = 0.25, epsilon: float = 1e-4, encoding: int = N.DENOISE_GAMMA) -> None:
        """rtEnqueueDenoiseSamples: `iterations` passes of the a-trous filter over the linear means of the
        width x height statistics (N.PIXEL_STATS_DTYPE), the luminance tolerance of each pixel
        `sigma_luminance` standard deviations of its mean, guided by the N.PIXEL_FEATURES_DTYPE records of
        `features`, into `out` ({r, g, b, sample count}, gamma-encoded or linear) and, when given, the
        filtered variance of the mean luminance into `variance` (4 B per pixel).  A sigma of 0 turns its
        term off.  Asynchronous; neither input is written."""
        params = N.DENOISE_SAMPLES_PARAMS(int(iterations), float(sigma_luminance), float(sigma_normal),
                                          float(sigma_depth), float(sigma_albedo), float(epsilon), int(encoding))
        check(self._lib.rtEnqueueDenoiseSamples(self.handle, kernel.handle, stats.handle, features.handle, int(width),
                                                int(height), ctypes.byref(params), out.handle,
                                                variance.handle if variance is not None else None),
              "Failed to enqueue sample denoise")

    def TemporalAccumulate(self, kernel: "CLKernel", cur: "Buffer", cur_features: "Buffer", hist: "Buffer | None",
                           hist_features: "Buffer | None", width: int, height: int, out: "Buffer", cur_view,
                           prev_view, cur_frames: float = 1.0, history_frames: float = 0.0,
                           max_history: float = 32.0, depth_tolerance: float = 0.05,
                           normal_threshold: float = 0.9, motion: "Buffer | None" = None) -> None:
        """rtEnqueueTemporalAccumulate: the previous image `hist` (with its features, both None when
        there is no history yet) reprojected from `prev_view` into `cur_view` and blended with `cur` by
        per-pixel sample count into `out`; images are width x height 16-B {r, g, b, w} slots, `out`'s w
        the new sample count.  A view is (position, front, up), three xyz triples.  Asynchronous; no
        input is written.  With `motion` (width x height N.PIXEL_MOTION_DTYPE records of the current
        view, FrameMotion's) it is rtEnqueueTemporalAccumulateMotion: each pixel's previous point and
        normal come from its record, so the history follows geometry that moved."""
        def view(v):
            pos, front, up = v
            return N.VIEW((ctypes.c_float * 3)(*map(float, pos)), (ctypes.c_float * 3)(*map(float, front)),
                          (ctypes.c_float * 3)(*map(float, up)))
        params = N.TEMPORAL_PARAMS(view(cur_view), view(prev_view), float(cur_frames), float(history_frames),
                                   float(max_history), float(depth_tolerance), float(normal_threshold))
        hist_h = hist.handle if hist is not None else None
        hist_features_h = hist_features.handle if hist_features is not None else None
        if motion is not None:
            check(self._lib.rtEnqueueTemporalAccumulateMotion(self.handle, kernel.handle, cur.handle, cur_features.handle,
                                                              hist_h, hist_features_h, motion.handle, int(width),
                                                              int(height), ctypes.byref(params), out.handle),
                  "Failed to enqueue temporal accumulate with motion")
            return
        check(self._lib.rtEnqueueTemporalAccumulate(self.handle, kernel.handle, cur.handle, cur_features.handle,
                                                    hist_h, hist_features_h,
                                                    int(width), int(height), ctypes.byref(params), out.handle),
              "Failed to enqueue temporal accumulate")

    def ReprojectSamples(self, kernel: "CLKernel", hist_stats: "Buffer", hist_features: "Buffer",
                         cur_features: "Buffer", width: int, height: int, out_stats: "Buffer", cur_view, prev_view,
                         max_history: float = 16.0, depth_tolerance: float = 0.05,
                         normal_threshold: float = 0.9, motion: "Buffer | None" = None) -> None:
        """rtEnqueueReprojectSamples (with `motion`, the current view's N.PIXEL_MOTION_DTYPE records:
        rtEnqueueReprojectSamplesMotion, whose previous points and normals come from the records): the width x height sample statistics `hist_stats`
        (N.PIXEL_STATS_DTYPE, with the features of their view) reprojected from `prev_view` into `cur_view`
        and recombined into `out_stats`: per pixel a mean, a per-sample variance and an integer sample
        count of at most `max_history` from the history taps on the same surface, or 32 zero bytes (no
        samples) where there is none.  A view is (position, front, up), three xyz triples.  Asynchronous;
        no input is written, and `out_stats` is none of them."""
        def view(v):
            pos, front, up = v
            return N.VIEW((ctypes.c_float * 3)(*map(float, pos)), (ctypes.c_float * 3)(*map(float, front)),
                          (ctypes.c_float * 3)(*map(float, up)))
        params = N.REPROJECT_PARAMS(view(cur_view), view(prev_view), float(max_history), float(depth_tolerance),
                                    float(normal_threshold))
        if motion is not None:
            check(self._lib.rtEnqueueReprojectSamplesMotion(self.handle, kernel.handle, hist_stats.handle,
                                                            hist_features.handle, cur_features.handle, motion.handle,
                                                            int(width), int(height), ctypes.byref(params),
                                                            out_stats.handle),
                  "Failed to enqueue sample reprojection with motion")
            return
        check(self._lib.rtEnqueueReprojectSamples(self.handle, kernel.handle, hist_stats.handle, hist_features.handle,
                                                  cur_features.handle, int(width), int(height), ctypes.byref(params),
                                                  out_stats.handle), "Failed to enqueue sample reprojection")

    def UpdateVertices(self, tris: "Buffer", first: int, n: int, positions: "Buffer",
                       normals: "Buffer | None" = None) -> None:
        """rtEnqueueUpdateVertices: the position (and normal) xyz of triangles [first, first + n) of `tris`
        from records [0, n) of `positions` / `normals` (N.TRI_POINTS_DTYPE); asynchronous."""
        check(self._lib.rtEnqueueUpdateVertices(self.handle, tris.handle, int(first), int(n), positions.handle,
                                                normals.handle if normals is not None else None),
              "Failed to update vertices")

    def ExtractVertices(self, tris: "Buffer", first: int, n: int, positions: "Buffer",
                        normals: "Buffer | None" = None) -> None:
        """rtEnqueueExtractVertices, UpdateVertices' inverse: records [0, n) of `positions` / `normals`
        (N.TRI_POINTS_DTYPE, w slots 0) from the position (and normal) xyz of triangles [first, first + n)
        of `tris`; asynchronous.  The "before" snapshot of a move, taken on the device."""
        check(self._lib.rtEnqueueExtractVertices(self.handle, tris.handle, int(first), int(n), positions.handle,
                                                 normals.handle if normals is not None else None),
              "Failed to extract vertices")

    def HitMotion(self, kernel: "CLKernel", hits: "Buffer", first: int, n: int, motion: "Buffer",
                  prev_positions: "Buffer | None" = None, prev_normals: "Buffer | None" = None, first_tri: int = 0,
                  n_tris: int = 0) -> None:
        """rtEnqueueHitMotion: for hits [first, first + n) of `hits` (N.RAY_HIT_DTYPE) the surface point and
        normal at the previous time into the same slots of `motion` (N.PIXEL_MOTION_DTYPE): triangles
        [first_tri, first_tri + n_tris) take their vertices from `prev_positions` / `prev_normals`
        (N.TRI_POINTS_DTYPE, ExtractVertices' records), the others from the scene bound to `kernel`."""
        check(self._lib.rtEnqueueHitMotion(self.handle, kernel.handle, hits.handle, int(first), int(n),
                                           prev_positions.handle if prev_positions is not None else None,
                                           prev_normals.handle if prev_normals is not None else None, int(first_tri),
                                           int(n_tris), motion.handle), "Failed to enqueue hit motion")

    def FrameMotion(self, kernel: "CLKernel", work_size: int, motion: "Buffer",
                    prev_positions: "Buffer | None" = None, prev_normals: "Buffer | None" = None, first_tri: int = 0,
                    n_tris: int = 0) -> None:
        """rtEnqueueFrameMotion: per work-item the closest hit of the pixel's centre ray and HitMotion's
        record of it (N.PIXEL_MOTION_DTYPE), one fused launch."""
        check(self._lib.rtEnqueueFrameMotion(self.handle, kernel.handle, int(work_size),
                                             prev_positions.handle if prev_positions is not None else None,
                                             prev_normals.handle if prev_normals is not None else None, int(first_tri),
                                             int(n_tris), motion.handle), "Failed to enqueue frame motion")

    def RefitBVH(self, kernel: "CLKernel") -> None:
        """rtRefitBVH: the bounds of the tree bound to `kernel` from its triangles, on the device, into the
        node buffer and every record the kernel packed; asynchronous.  Topology stays."""
        check(self._lib.rtRefitBVH(self.handle, kernel.handle), "Failed to refit BVH")

    def Finish(self) -> None:
        check(self._lib.rtFinish(self.handle), "Failed to finish queue")

    def stream(self) -> int:
        s = ctypes.c_void_p()
        check(self._lib.rtContextGetStream(self.handle, ctypes.byref(s)), "stream")
        return int(s.value or 0)

    def accum_stream(self) -> int:
        """The fused-frame accumulation stream (rtContextGetAccumStream)."""
        s = ctypes.c_void_p()
        check(self._lib.rtContextGetAccumStream(self.handle, ctypes.byref(s)), "accumulation stream")
        return int(s.value or 0)

    def set_accum_overlap(self, enable: bool) -> None:
        """rtContextSetAccumOverlap: fused frames' accumulation beside the next render (default)."""
        check(self._lib.rtContextSetAccumOverlap(self.handle, int(bool(enable))), "accumulation overlap")

    def set_readback_on_accum_stream(self, enable: bool) -> None:
        check(self._lib.rtContextSetReadbackOnAccumStream(self.handle, int(bool(enable))), "readback stream")

    def release(self) -> None:
        if self.handle:
            self._lib.rtReleaseContext(self.handle)
            self.handle = None


class Buffer:
    """cl::Buffer(context, flags, size, host_ptr) (CLBVHnode.cpp:215-236)."""

    def __init__(self, ctx: CLContext, flags: int, size: int, host: np.ndarray | None = None):
        self._lib = ctx._lib
        self.ctx = ctx
        h = ctypes.c_void_p()
        ptr = None
        if host is not None:
            host = np.ascontiguousarray(host)
            if host.nbytes < size:
                raise RTError("Failed to create buffer", -37)
            ptr = host.ctypes.data
        check(self._lib.rtCreateBuffer(ctx.handle, int(flags), int(size), ptr, ctypes.byref(h)),
              "Failed to create buffer")
        self.handle = h
        self.size = int(size)

    def device_pointer(self) -> int:
        p = ctypes.c_void_p()
        check(self._lib.rtBufferGetDevicePointer(self.handle, ctypes.byref(p)), "device pointer")
        return int(p.value)

    def release(self) -> None:
        if self.handle:
            self._lib.rtReleaseBuffer(self.handle)
            self.handle = None


class CLKernel:
    """CLKernel(file, devices) (CLutils.cpp:52-66).  The kernel is precompiled; only the
    name "KernelEntry" exists."""

    def __init__(self, ctx: CLContext, name: str = "KernelEntry"):
        self._lib = ctx._lib
        self.ctx = ctx
        h = ctypes.c_void_p()
        check(self._lib.rtCreateKernel(ctx.handle, name.encode(), ctypes.byref(h)),
              "Failed to create kernel")
        self.handle = h
        self._keep = {}

    def SetArgument(self, index: int, data: bytes) -> bool:
        """SetArgument(argIndex, data, size) (CLutils.cpp:68-77): raw bytes of the value."""
        buf = ctypes.create_string_buffer(bytes(data), len(data))
        check(self._lib.rtSetKernelArg(self.handle, int(index), len(data), buf),
              "Failed to set kernel argument")
        return True

    # typed helpers = CLRaytracer::SetUniform<T> instantiations (CLRaytracer.cpp:139-148)
    def set_buffer(self, index: int, buf: Buffer) -> bool:
        self._keep[index] = buf
        return self.SetArgument(index, struct.pack("P", buf.handle.value))

    def set_uint(self, index: int, v: int) -> bool:
        return self.SetArgument(index, struct.pack("<I", int(v) & 0xFFFFFFFF))

    def set_int(self, index: int, v: int) -> bool:
        return self.SetArgument(index, struct.pack("<i", int(v)))

    def set_float(self, index: int, v: float) -> bool:
        return self.SetArgument(index, struct.pack("<f", float(v)))

    def set_float3(self, index: int, v) -> bool:
        x, y, z = (float(c) for c in v)
        return self.SetArgument(index, struct.pack("<4f", x, y, z, 0.0))

    # extensions
    def set_math_mode(self, mode: int) -> None:
        check(self._lib.rtKernelSetMathMode(self.handle, int(mode)), "math mode")

    def set_shadow_rays(self, enable: bool) -> None:
        """rtKernelSetShadowRays: TracePaths and SamplePixels test the analytic light's term against the scene."""
        check(self._lib.rtKernelSetShadowRays(self.handle, int(bool(enable))), "shadow rays")

    def get_shadow_rays(self) -> bool:
        v = ctypes.c_int()
        check(self._lib.rtKernelGetShadowRays(self.handle, ctypes.byref(v)), "shadow rays")
        return bool(v.value)

    def set_schedule(self, sched: int) -> None:
        check(self._lib.rtKernelSetSchedule(self.handle, int(sched)), "schedule")

    def set_tuning(self, name: str, value: int) -> None:
        """rtKernelSetTuning: a scheduling parameter by name (N.TUNING, N.TRACE_TUNING); results are
        unchanged."""
        check(self._lib.rtKernelSetTuning(self.handle, _tuning_id(name), int(value)), f"tuning {name}")

    def get_tuning(self, name: str) -> int:
        v = ctypes.c_int()
        check(self._lib.rtKernelGetTuning(self.handle, _tuning_id(name), ctypes.byref(v)), f"tuning {name}")
        return int(v.value)

    def set_row_interleave(self, period: int, phase: int) -> None:
        check(self._lib.rtKernelSetRowInterleave(self.handle, int(period), int(phase)), "row interleave")

    def set_work_range(self, first: int, last: int) -> None:
        check(self._lib.rtKernelSetWorkRange(self.handle, int(first), int(last)), "work range")

    def set_hit_buffers(self, ids: Buffer | None, t: Buffer | None) -> None:
        check(self._lib.rtKernelSetHitBuffers(self.handle, ids.handle if ids else None,
                                              t.handle if t else None), "hit buffers")
        self._keep["hits"] = (ids, t)

    def set_stats(self, enable: bool) -> None:
        check(self._lib.rtKernelSetStats(self.handle, int(bool(enable))), "stats")

    def set_timing(self, enable: bool) -> None:
        check(self._lib.rtKernelSetTiming(self.handle, int(bool(enable))), "timing")

    def force_global_scene(self, force: bool) -> None:
        check(self._lib.rtKernelForceGlobalScene(self.handle, int(bool(force))), "force global")

    def scene_in_lds(self) -> bool:
        v = ctypes.c_int()
        check(self._lib.rtKernelGetSceneInLDS(self.handle, ctypes.byref(v)), "scene in lds")
        return bool(v.value)

    def stats(self) -> dict:
        s = N.Stats()
        check(self._lib.rtKernelGetStats(self.handle, ctypes.byref(s)), "stats")
        sched = dict(zip(("node_steps", "node_lanes", "tri_steps", "tri_lanes", "shade_rounds",
                          "shade_lanes", "refill_rounds", "refill_lanes", "other_lanes",
                          "shade_wait", "free_wait", "reserved"), list(s.sched)))
        # the last word by what it holds in the default stats build: the refill's pop iterations (the
        # diagnostic RT_TIMELINE / RT_LDS_CONFLICTS builds keep other things in these words: "reserved")
        sched["refill_pops"] = sched["reserved"]
        return {"rays": s.rays, "node_visits": s.node_visits, "tri_tests": s.tri_tests,
                "hits": s.hits, "launches": s.launches, "kernel_ms": s.kernel_ms, "accum_ms": s.accum_ms,
                "render_period_ms": s.render_period_ms,
                "cycles": {"refill": s.cycles_refill, "traverse": s.cycles_traverse,
                           "shade": s.cycles_shade, "total": s.cycles_total},
                "sched": sched}

    def path_kill(self) -> dict:
        """rtKernelGetPathKill: the segments the stats launches shaded with zero throughput (hits, misses),
        whether the scene passes the path-kill certificate, and whether the last render launch carried
        the kill."""
        s = N.PathKillInfo()
        check(self._lib.rtKernelGetPathKill(self.handle, ctypes.byref(s)), "path kill")
        return {"zero_hits": int(s.zero_hits), "zero_misses": int(s.zero_misses),
                "scene_certified": bool(s.scene_certified), "launch_certified": bool(s.launch_certified)}

    def node_collapse(self) -> dict:
        """rtKernelGetNodeCollapse: the link words the scene's collapsed record set changes, whether the
        set may be walked (not after a device refit), and whether the last launch walked it."""
        s = N.NodeCollapseInfo()
        check(self._lib.rtKernelGetNodeCollapse(self.handle, ctypes.byref(s)), "node collapse")
        return {"collapsed_links": int(s.collapsed_links), "scene_collapsible": bool(s.scene_collapsible),
                "launch_collapsed": bool(s.launch_collapsed)}

    def gate_skip(self) -> dict:
        """rtKernelGetGateSkip: the link words the scene's gate-skipped record set changes against the plain
        one (0: the tree's boxes do not nest), whether the scene has the set and it may be walked (not after
        a device refit), and whether the last launch walked it."""
        s = N.GateSkipInfo()
        check(self._lib.rtKernelGetGateSkip(self.handle, ctypes.byref(s)), "gate skip")
        return {"gate_links": int(s.gate_links), "scene_nested": bool(s.scene_nested),
                "launch_gate_skipped": bool(s.launch_gate_skipped)}

    def octant_cull(self) -> dict:
        """rtKernelGetOctantCull: the link words the scene's pruned record set changes (culled subtrees;
        contracted single-child nodes, always 0), whether the set may be walked (not after a device
        refit), and whether the last launch walked it."""
        s = N.OctantCullInfo()
        check(self._lib.rtKernelGetOctantCull(self.handle, ctypes.byref(s)), "octant cull")
        return {"pruned_links": int(s.pruned_links), "contracted_links": int(s.contracted_links),
                "scene_certified": bool(s.scene_certified), "launch_pruned": bool(s.launch_pruned)}

    def scene_prepares(self) -> tuple:
        """rtDiagScenePrepares: (full host-side scene preparations, device refits) since creation."""
        full, refits = ctypes.c_uint64(), ctypes.c_uint64()
        check(self._lib.rtDiagScenePrepares(self.handle, ctypes.byref(full), ctypes.byref(refits)),
              "scene prepares")
        return int(full.value), int(refits.value)

    def reset_stats(self) -> None:
        check(self._lib.rtKernelResetStats(self.handle), "reset stats")

    def release(self) -> None:
        if self.handle:
            self._lib.rtReleaseKernel(self.handle)
            self.handle = None

// rt_cl_compat.hpp -- header-only C++ face of librt_hip.so with the reference's shapes.
//
// A host written against the reference's device wrapper (CLutils.h:11-145) keeps its
// calls: CLContext::{ReadBuffer, ExecuteKernel, Finish, GetContext},
// CLKernel::SetArgument, RenderKernelArgument_t, CLException("msg (CL_NAME)").
// cl::Buffer becomes rtcl::Buffer (RAII over rt_mem); cl::Platform disappears (the
// context takes a GPU index).  Nothing here allocates device memory on its own.
#pragma once

#include <cstddef>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>

#include "rt_hip.h"
#include "rt_status.h"

namespace rtcl {

// CLutils.h:11-27
enum class RenderKernelArgument_t : unsigned int {
    BUFFER_OUT,
    BUFFER_SCENE,
    BUFFER_NODE,
    BUFFER_MATERIAL,
    WIDTH,
    HEIGHT,
    FRAME_COUNT,
    FRAME_SEED,
    LIGHT_BOUNCES,
    LIGHT_TYPE,
    SKYBOX_INTENSITY,
    CAMERA_POS,
    CAMERA_FRONT,
    CAMERA_UP
};

// CLutils.h:107-114
class CLException : public std::runtime_error {
public:
    CLException(const std::string& message, int errorCode)
        : std::runtime_error(message + " (" + rtGetErrorString(errorCode) + ")"), code(errorCode) {}
    int code;
};

inline void check(int rc, const char* what) {
    if (rc != RT_SUCCESS) throw CLException(what, rc);
}

class Buffer {
public:
    Buffer() = default;
    Buffer(rt_context ctx, uint64_t flags, size_t size, const void* host = nullptr) {
        check(rtCreateBuffer(ctx, flags, size, host, &mem_), "Failed to create buffer");
    }
    ~Buffer() { reset(); }
    Buffer(const Buffer&) = delete;
    Buffer& operator=(const Buffer&) = delete;
    Buffer(Buffer&& o) noexcept : mem_(o.mem_) { o.mem_ = nullptr; }
    Buffer& operator=(Buffer&& o) noexcept {
        if (this != &o) {
            reset();
            mem_ = o.mem_;
            o.mem_ = nullptr;
        }
        return *this;
    }
    rt_mem get() const { return mem_; }
    void reset() {
        if (mem_) rtReleaseBuffer(mem_);
        mem_ = nullptr;
    }

private:
    rt_mem mem_ = nullptr;
};

class CLKernel;

// CLutils.h:116-133
class CLContext {
public:
    explicit CLContext(int device = 0) { check(rtCreateContext(device, &ctx_), "Failed to create context"); }
    ~CLContext() {
        if (ctx_) rtReleaseContext(ctx_);
    }
    CLContext(const CLContext&) = delete;
    CLContext& operator=(const CLContext&) = delete;

    void ReadBuffer(const Buffer& buffer, void* ptr, size_t size) const {
        check(rtEnqueueReadBuffer(ctx_, buffer.get(), 0, 0, size, ptr), "Failed to read buffer");
    }
    inline void ExecuteKernel(std::shared_ptr<CLKernel> kernel, size_t workSize) const;
    // extensions: batched ray queries over caller rays (rtEnqueueIntersectRays, rtEnqueueCameraRays)
    inline void IntersectRays(std::shared_ptr<CLKernel> kernel, const Buffer& rays, const Buffer& hits, size_t nRays,
                              int mode = RT_QUERY_CLOSEST, size_t firstRay = 0) const;
    inline void CameraRays(std::shared_ptr<CLKernel> kernel, size_t workSize, const Buffer& rays) const;
    // extensions: the surface at each hit, and first-hit feature buffers (rtEnqueueHitSurfaces,
    // rtEnqueueFrameFeatures)
    inline void HitSurfaces(std::shared_ptr<CLKernel> kernel, const Buffer& rays, const Buffer& hits,
                            const Buffer& surfaces, size_t n, size_t first = 0) const;
    inline void FrameFeatures(std::shared_ptr<CLKernel> kernel, size_t workSize, unsigned nFrames,
                              const Buffer& features) const;
    // extension: the feature-guided a-trous denoiser over an image of 16-B slots (rtEnqueueDenoise)
    inline void Denoise(std::shared_ptr<CLKernel> kernel, const Buffer& image, const Buffer& features, unsigned width,
                        unsigned height, const rt_denoise_params& params, const Buffer& out) const;
    // extension: the variance-guided a-trous denoiser over the adaptive sample statistics
    // (rtEnqueueDenoiseSamples); variance may be null
    inline void DenoiseSamples(std::shared_ptr<CLKernel> kernel, const Buffer& stats, const Buffer& features,
                               unsigned width, unsigned height, const rt_denoise_samples_params& params, const Buffer& out,
                               const Buffer* variance = nullptr) const;
    // extension: temporal reprojection of the previous image into the current view (rtEnqueueTemporalAccumulate);
    // hist and histFeatures are both null when there is no history yet
    inline void TemporalAccumulate(std::shared_ptr<CLKernel> kernel, const Buffer& cur, const Buffer& curFeatures,
                                   const Buffer* hist, const Buffer* histFeatures, unsigned width, unsigned height,
                                   const rt_temporal_params& params, const Buffer& out) const;
    // extension: the adaptive sample statistics reprojected into the current view (rtEnqueueReprojectSamples)
    inline void ReprojectSamples(std::shared_ptr<CLKernel> kernel, const Buffer& histStats, const Buffer& histFeatures,
                                 const Buffer& curFeatures, unsigned width, unsigned height,
                                 const rt_reproject_params& params, const Buffer& outStats) const;
    // extensions: adaptive sampling (rt_hip.h): per-pixel sample statistics from linear path results (ids null:
    // record i is pixel i), the ordered list of pixels that still need samples, camera paths for such a list,
    // and the statistics resolved into an {r, g, b, sample count} image
    inline void AccumulateSamples(std::shared_ptr<CLKernel> kernel, const Buffer* ids, const Buffer& results, size_t first,
                                  size_t n, size_t nPixels, const Buffer& stats) const;
    inline void SelectPixels(std::shared_ptr<CLKernel> kernel, const Buffer& stats, unsigned width, unsigned height,
                             const rt_adaptive_params& params, const Buffer& ids, const Buffer& result) const;
    inline void CameraPathsFor(std::shared_ptr<CLKernel> kernel, const Buffer& ids, size_t first, size_t n,
                               const Buffer& rays, const Buffer& seeds) const;
    inline void ResolveSamples(std::shared_ptr<CLKernel> kernel, const Buffer& stats, unsigned width, unsigned height,
                               const Buffer& out) const;
    // one sample for ids[first, first + min(n, count's first word)) in one launch; count may be null (then n)
    inline void SamplePixels(std::shared_ptr<CLKernel> kernel, const Buffer& ids, const Buffer* count, size_t first,
                             size_t n, size_t nPixels, const Buffer& stats) const;
    // extensions: moving geometry (rtEnqueueUpdateVertices, rtRefitBVH); normals may be null
    void UpdateVertices(const Buffer& tris, size_t firstTri, size_t nTris, const Buffer& positions,
                        const Buffer* normals = nullptr) const {
        check(rtEnqueueUpdateVertices(ctx_, tris.get(), firstTri, nTris, positions.get(),
                                      normals ? normals->get() : nullptr),
              "Failed to update vertices");
    }
    inline void RefitBVH(std::shared_ptr<CLKernel> kernel) const;
    // extensions: motion records (rt_hip.h).  ExtractVertices is UpdateVertices' inverse, the "before" snapshot
    // of a move; HitMotion and FrameMotion give per hit / per pixel the surface point at the previous time
    // (prevPositions null: nothing moved; prevNormals null: the current normals); the two Motion calls are
    // TemporalAccumulate and ReprojectSamples whose previous points come from such records (motion null: the
    // plain calls)
    void ExtractVertices(const Buffer& tris, size_t firstTri, size_t nTris, const Buffer& positions,
                         const Buffer* normals = nullptr) const {
        check(rtEnqueueExtractVertices(ctx_, tris.get(), firstTri, nTris, positions.get(),
                                       normals ? normals->get() : nullptr),
              "Failed to extract vertices");
    }
    inline void HitMotion(std::shared_ptr<CLKernel> kernel, const Buffer& hits, size_t first, size_t n,
                          const Buffer* prevPositions, const Buffer* prevNormals, size_t firstTri, size_t nTris,
                          const Buffer& motion) const;
    inline void FrameMotion(std::shared_ptr<CLKernel> kernel, size_t globalWorkSize, const Buffer* prevPositions,
                            const Buffer* prevNormals, size_t firstTri, size_t nTris, const Buffer& motion) const;
    inline void TemporalAccumulateMotion(std::shared_ptr<CLKernel> kernel, const Buffer& cur, const Buffer& curFeatures,
                                         const Buffer* hist, const Buffer* histFeatures, const Buffer* motion,
                                         unsigned width, unsigned height, const rt_temporal_params& params,
                                         const Buffer& out) const;
    inline void ReprojectSamplesMotion(std::shared_ptr<CLKernel> kernel, const Buffer& histStats,
                                       const Buffer& histFeatures, const Buffer& curFeatures, const Buffer* motion,
                                       unsigned width, unsigned height, const rt_reproject_params& params,
                                       const Buffer& outStats) const;
    void Finish() const { check(rtFinish(ctx_), "Failed to finish queue"); }
    rt_context GetContext() const { return ctx_; }

private:
    rt_context ctx_ = nullptr;
};

// CLutils.h:135-145
class CLKernel {
public:
    CLKernel(const CLContext& ctx, const char* name = "KernelEntry") {
        check(rtCreateKernel(ctx.GetContext(), name, &k_), "Failed to create kernel");
    }
    ~CLKernel() {
        if (k_) rtReleaseKernel(k_);
    }
    CLKernel(const CLKernel&) = delete;
    CLKernel& operator=(const CLKernel&) = delete;

    // Same contract as the reference: throws on failure, returns true otherwise.
    bool SetArgument(RenderKernelArgument_t argIndex, const void* data, size_t size) {
        check(rtSetKernelArg(k_, static_cast<unsigned>(argIndex), size, data),
              "Failed to set kernel argument");
        return true;
    }
    bool SetBuffer(RenderKernelArgument_t argIndex, const Buffer& b) {
        rt_mem m = b.get();
        return SetArgument(argIndex, &m, sizeof(m));
    }
    rt_kernel GetKernel() const { return k_; }

private:
    rt_kernel k_ = nullptr;
};

inline void CLContext::ExecuteKernel(std::shared_ptr<CLKernel> kernel, size_t workSize) const {
    check(rtEnqueueKernel(ctx_, kernel->GetKernel(), workSize), "Failed to enqueue kernel");
}
inline void CLContext::IntersectRays(std::shared_ptr<CLKernel> kernel, const Buffer& rays, const Buffer& hits,
                                     size_t nRays, int mode, size_t firstRay) const {
    check(rtEnqueueIntersectRays(ctx_, kernel->GetKernel(), rays.get(), firstRay, nRays, mode, hits.get()),
          "Failed to enqueue ray query");
}
inline void CLContext::CameraRays(std::shared_ptr<CLKernel> kernel, size_t workSize, const Buffer& rays) const {
    check(rtEnqueueCameraRays(ctx_, kernel->GetKernel(), workSize, rays.get()), "Failed to enqueue camera rays");
}
inline void CLContext::HitSurfaces(std::shared_ptr<CLKernel> kernel, const Buffer& rays, const Buffer& hits,
                                   const Buffer& surfaces, size_t n, size_t first) const {
    check(rtEnqueueHitSurfaces(ctx_, kernel->GetKernel(), rays.get(), hits.get(), first, n, surfaces.get()),
          "Failed to enqueue hit surfaces");
}
inline void CLContext::FrameFeatures(std::shared_ptr<CLKernel> kernel, size_t workSize, unsigned nFrames,
                                     const Buffer& features) const {
    check(rtEnqueueFrameFeatures(ctx_, kernel->GetKernel(), workSize, nFrames, features.get()),
          "Failed to enqueue frame features");
}
inline void CLContext::Denoise(std::shared_ptr<CLKernel> kernel, const Buffer& image, const Buffer& features,
                               unsigned width, unsigned height, const rt_denoise_params& params,
                               const Buffer& out) const {
    check(rtEnqueueDenoise(ctx_, kernel->GetKernel(), image.get(), features.get(), width, height, &params, out.get()),
          "Failed to enqueue denoise");
}
inline void CLContext::DenoiseSamples(std::shared_ptr<CLKernel> kernel, const Buffer& stats, const Buffer& features,
                                      unsigned width, unsigned height, const rt_denoise_samples_params& params,
                                      const Buffer& out, const Buffer* variance) const {
    check(rtEnqueueDenoiseSamples(ctx_, kernel->GetKernel(), stats.get(), features.get(), width, height, &params, out.get(),
                                  variance ? variance->get() : nullptr),
          "Failed to enqueue sample denoise");
}
inline void CLContext::TemporalAccumulate(std::shared_ptr<CLKernel> kernel, const Buffer& cur, const Buffer& curFeatures,
                                          const Buffer* hist, const Buffer* histFeatures, unsigned width,
                                          unsigned height, const rt_temporal_params& params, const Buffer& out) const {
    check(rtEnqueueTemporalAccumulate(ctx_, kernel->GetKernel(), cur.get(), curFeatures.get(),
                                      hist ? hist->get() : nullptr, histFeatures ? histFeatures->get() : nullptr, width,
                                      height, &params, out.get()),
          "Failed to enqueue temporal accumulate");
}
inline void CLContext::ReprojectSamples(std::shared_ptr<CLKernel> kernel, const Buffer& histStats,
                                        const Buffer& histFeatures, const Buffer& curFeatures, unsigned width,
                                        unsigned height, const rt_reproject_params& params, const Buffer& outStats) const {
    check(rtEnqueueReprojectSamples(ctx_, kernel->GetKernel(), histStats.get(), histFeatures.get(), curFeatures.get(), width,
                                    height, &params, outStats.get()),
          "Failed to enqueue sample reprojection");
}
inline void CLContext::AccumulateSamples(std::shared_ptr<CLKernel> kernel, const Buffer* ids, const Buffer& results,
                                         size_t first, size_t n, size_t nPixels, const Buffer& stats) const {
    check(rtEnqueueAccumulateSamples(ctx_, kernel->GetKernel(), ids ? ids->get() : nullptr, results.get(), first, n,
                                     nPixels, stats.get()),
          "Failed to enqueue sample accumulation");
}
inline void CLContext::SelectPixels(std::shared_ptr<CLKernel> kernel, const Buffer& stats, unsigned width, unsigned height,
                                    const rt_adaptive_params& params, const Buffer& ids, const Buffer& result) const {
    check(rtEnqueueSelectPixels(ctx_, kernel->GetKernel(), stats.get(), width, height, &params, ids.get(), result.get()),
          "Failed to enqueue pixel selection");
}
inline void CLContext::CameraPathsFor(std::shared_ptr<CLKernel> kernel, const Buffer& ids, size_t first, size_t n,
                                      const Buffer& rays, const Buffer& seeds) const {
    check(rtEnqueueCameraPathsFor(ctx_, kernel->GetKernel(), ids.get(), first, n, rays.get(), seeds.get()),
          "Failed to enqueue camera paths");
}
inline void CLContext::ResolveSamples(std::shared_ptr<CLKernel> kernel, const Buffer& stats, unsigned width,
                                      unsigned height, const Buffer& out) const {
    check(rtEnqueueResolveSamples(ctx_, kernel->GetKernel(), stats.get(), width, height, out.get()),
          "Failed to enqueue sample resolve");
}
inline void CLContext::SamplePixels(std::shared_ptr<CLKernel> kernel, const Buffer& ids, const Buffer* count, size_t first,
                                    size_t n, size_t nPixels, const Buffer& stats) const {
    check(rtEnqueueSamplePixels(ctx_, kernel->GetKernel(), ids.get(), count ? count->get() : nullptr, first, n, nPixels,
                                stats.get()),
          "Failed to enqueue pixel samples");
}
inline void CLContext::RefitBVH(std::shared_ptr<CLKernel> kernel) const {
    check(rtRefitBVH(ctx_, kernel->GetKernel()), "Failed to refit BVH");
}
inline void CLContext::HitMotion(std::shared_ptr<CLKernel> kernel, const Buffer& hits, size_t first, size_t n,
                                 const Buffer* prevPositions, const Buffer* prevNormals, size_t firstTri, size_t nTris,
                                 const Buffer& motion) const {
    check(rtEnqueueHitMotion(ctx_, kernel->GetKernel(), hits.get(), first, n,
                             prevPositions ? prevPositions->get() : nullptr, prevNormals ? prevNormals->get() : nullptr,
                             firstTri, nTris, motion.get()),
          "Failed to enqueue hit motion");
}
inline void CLContext::FrameMotion(std::shared_ptr<CLKernel> kernel, size_t globalWorkSize, const Buffer* prevPositions,
                                   const Buffer* prevNormals, size_t firstTri, size_t nTris, const Buffer& motion) const {
    check(rtEnqueueFrameMotion(ctx_, kernel->GetKernel(), globalWorkSize, prevPositions ? prevPositions->get() : nullptr,
                               prevNormals ? prevNormals->get() : nullptr, firstTri, nTris, motion.get()),
          "Failed to enqueue frame motion");
}
inline void CLContext::TemporalAccumulateMotion(std::shared_ptr<CLKernel> kernel, const Buffer& cur,
                                                const Buffer& curFeatures, const Buffer* hist, const Buffer* histFeatures,
                                                const Buffer* motion, unsigned width, unsigned height,
                                                const rt_temporal_params& params, const Buffer& out) const {
    check(rtEnqueueTemporalAccumulateMotion(ctx_, kernel->GetKernel(), cur.get(), curFeatures.get(),
                                            hist ? hist->get() : nullptr, histFeatures ? histFeatures->get() : nullptr,
                                            motion ? motion->get() : nullptr, width, height, &params, out.get()),
          "Failed to enqueue temporal accumulate with motion");
}
inline void CLContext::ReprojectSamplesMotion(std::shared_ptr<CLKernel> kernel, const Buffer& histStats,
                                              const Buffer& histFeatures, const Buffer& curFeatures, const Buffer* motion,
                                              unsigned width, unsigned height, const rt_reproject_params& params,
                                              const Buffer& outStats) const {
    check(rtEnqueueReprojectSamplesMotion(ctx_, kernel->GetKernel(), histStats.get(), histFeatures.get(),
                                          curFeatures.get(), motion ? motion->get() : nullptr, width, height, &params,
                                          outStats.get()),
          "Failed to enqueue sample reprojection with motion");
}

}  // namespace rtcl

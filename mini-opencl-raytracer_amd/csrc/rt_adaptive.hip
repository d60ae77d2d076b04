// rt_adaptive.hip -- the kernels of adaptive sampling: rtEnqueueAccumulateSamples, rtEnqueueSelectPixels
// and rtEnqueueResolveSamples.  The operations are defined step by step in include/rt_hip.h and restated
// in numpy by tests/adaptive_ref.py: every fp32 operation here is one correctly rounded IEEE operation in
// the order written there (no contraction, denormals kept, IEEE division -- which is why this is a
// translation unit of its own, built with the standard flags and not with the shipped kernels' relaxed
// division).  The per-pixel arithmetic and every range test are rt_adaptive_math.hpp, the text a CPU
// program sweeps under sanitizers.
//
// Records move as 16-B vectors: a statistics record is two float4 {sum.rgb, n}, {mean_y, m2_y,
// reserved[2]}, a sample and a resolved pixel one.
//
// The select is four launches over rtp::SelectPlan's blocks (rt_adaptive_plan.hpp: kSelectBlockPixels
// consecutive pixels per workgroup, a wave's lanes on 64 consecutive pixels in every round):
//   select_flags    per pixel the hot test and the count's rule into a byte plane; hot pixels per block
//   select_count    per pixel the rule over its window of flag bytes -- re-read through L1/L2: a block is
//                   a run of consecutive pixels, not a tile, and a flag is one byte -- into a second byte
//                   plane; selected pixels per block
//   select_scan     ONE workgroup: the exclusive scan of the blocks' selected counts (kScanThreads per
//                   pass, a carry between passes), the totals into `result`
//   select_scatter  per block: ballot / lane-prefix ranks inside a wave, the waves' and rounds' counts
//                   through LDS, pixel indices stored in ascending order from the block's offset
// No atomic anywhere: the list's order and every count are functions of the inputs alone.
#include "rt_adaptive.hpp"

#include "../../include/rt_pinned_math.h"

#pragma clang fp contract(off)

namespace rta {

namespace {

constexpr uint32_t kThreads = rtp::kAdaptiveThreads;
constexpr uint32_t kSelThreads = rtp::kSelectThreads, kSelRounds = rtp::kSelectPixelsPerThread;
constexpr uint32_t kSelBlock = rtp::kSelectBlockPixels, kSelWaves = kSelThreads / 64u;
constexpr uint32_t kScanThreads = rtp::kScanThreads, kScanWaves = kScanThreads / 64u;

__device__ __forceinline__ uint32_t lane_id() { return threadIdx.x & 63u; }
__device__ __forceinline__ uint32_t popc64(unsigned long long m) { return (uint32_t)__popcll(m); }
// set bits of m below this lane
__device__ __forceinline__ uint32_t rank_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__global__ __launch_bounds__(kThreads) void accumulate_samples(AccumArgs a) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= a.count) return;
    const uint32_t r = a.first + i;  // first + count <= 2^31
    const uint32_t p = a.ids ? a.ids[r] : r;
    if (!pixel_in_range(p, a.n_pixels)) return;
    const float4 s = a.results[r];
    if (!finite_sample(s.x, s.y, s.z)) return;
    float4* rec = a.stats + 2 * (size_t)p;
    const float4 lo = rec[0], hi = rec[1];
    const Moments m = sample_update(Moments{lo.w, hi.x, hi.y}, luminance(s.x, s.y, s.z));
    rec[0] = make_float4(lo.x + s.x, lo.y + s.y, lo.z + s.z, m.n);
    rec[1] = make_float4(m.mean_y, m.m2_y, hi.z, hi.w);  // reserved: kept as found
}

struct SelectConsts {
    uint32_t width, height, pixels, radius, blocks;
    float threshold, floor_y, min_samples, max_samples;
};

// the block's sum of a wave-uniform per-wave count, stored by thread 0
__device__ __forceinline__ void store_block_count(uint32_t wave_count, uint32_t* slot) {
    __shared__ uint32_t ws[kSelWaves];
    if (lane_id() == 0u) ws[threadIdx.x >> 6] = wave_count;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < kSelWaves; ++w) t += ws[w];
        *slot = t;
    }
}

__global__ __launch_bounds__(kSelThreads) void select_flags(const float4* stats, uint8_t* flags, uint32_t* hot_counts,
                                                            SelectConsts c) {
    const uint32_t base = blockIdx.x * kSelBlock;  // blocks * kSelBlock < 2^31 + kSelBlock
    uint32_t nhot = 0;
#pragma unroll
    for (uint32_t i = 0; i < kSelRounds; ++i) {
        const uint32_t p = base + i * kSelThreads + threadIdx.x;
        bool hot = false;
        if (p < c.pixels) {
            const float4 lo = stats[2 * (size_t)p], hi = stats[2 * (size_t)p + 1];
            hot = is_hot(Moments{lo.w, hi.x, hi.y}, c.threshold, c.floor_y);
            flags[p] = flag_byte(hot, count_rule(lo.w, c.min_samples, c.max_samples));
        }
        nhot += popc64(__ballot(hot));
    }
    store_block_count(nhot, hot_counts + blockIdx.x);
}

__global__ __launch_bounds__(kSelThreads) void select_count(const uint8_t* flags, uint8_t* sel, uint32_t* sel_counts,
                                                            SelectConsts c) {
    const uint32_t base = blockIdx.x * kSelBlock;
    uint32_t nsel = 0;
#pragma unroll
    for (uint32_t i = 0; i < kSelRounds; ++i) {
        const uint32_t p = base + i * kSelThreads + threadIdx.x;
        bool s = false;
        if (p < c.pixels) {
            const uint32_t rule = flag_rule(flags[p]);
            const bool any = rule == kByWindow && window_any_hot(flags, p, c.width, c.height, c.radius);
            s = selected(rule, any);
            sel[p] = s ? 1 : 0;
        }
        nsel += popc64(__ballot(s));
    }
    store_block_count(nsel, sel_counts + blockIdx.x);
}

__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t v) {
    const uint32_t lane = lane_id();
#pragma unroll
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        const uint32_t t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

__global__ __launch_bounds__(kScanThreads) void select_scan(const uint32_t* sel_counts, const uint32_t* hot_counts,
                                                            uint32_t* offsets, uint32_t blocks, uint4* result) {
    __shared__ uint32_t ws[kScanWaves], hs[kScanWaves];
    const uint32_t tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    uint32_t carry = 0, hot = 0;
    for (uint32_t base = 0; base < blocks; base += kScanThreads) {  // blocks <= 2^21
        const uint32_t b = base + tid;
        const uint32_t v = b < blocks ? sel_counts[b] : 0u;
        hot += b < blocks ? hot_counts[b] : 0u;
        const uint32_t incl = wave_inclusive_scan(v);
        if (lane == 63u) ws[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
#pragma unroll
        for (uint32_t w = 0; w < kScanWaves; ++w) {
            before += w < wave ? ws[w] : 0u;
            total += ws[w];
        }
        if (b < blocks) offsets[b] = carry + before + (incl - v);
        carry += total;
        __syncthreads();  // ws is written again in the next pass
    }
    const uint32_t wave_hot = wave_inclusive_scan(hot);
    if (lane == 63u) hs[wave] = wave_hot;
    __syncthreads();
    if (tid == 0u) {
        uint32_t t = 0;
        for (uint32_t w = 0; w < kScanWaves; ++w) t += hs[w];
        *result = make_uint4(carry, t, 0u, 0u);
    }
}

__global__ __launch_bounds__(kSelThreads) void select_scatter(const uint8_t* sel, const uint32_t* offsets, uint32_t* ids,
                                                              uint32_t pixels) {
    __shared__ uint32_t seg[kSelRounds * kSelWaves];  // selected pixels per (round, wave), in pixel order
    const uint32_t base = blockIdx.x * kSelBlock, wave = threadIdx.x >> 6;
    bool s[kSelRounds];
    unsigned long long m[kSelRounds];
#pragma unroll
    for (uint32_t i = 0; i < kSelRounds; ++i) {
        const uint32_t p = base + i * kSelThreads + threadIdx.x;
        s[i] = p < pixels && sel[p] != 0;
        m[i] = __ballot(s[i]);
        if (lane_id() == 0u) seg[i * kSelWaves + wave] = popc64(m[i]);
    }
    __syncthreads();
    const uint32_t off = offsets[blockIdx.x];
    uint32_t before = 0, at = 0;  // selected pixels of the block before this wave's round i
#pragma unroll
    for (uint32_t i = 0; i < kSelRounds; ++i) {
        for (; at < i * kSelWaves + wave; ++at) before += seg[at];
        // off + before + rank < the total of selected pixels <= pixels: inside `ids`
        if (s[i]) ids[(size_t)off + before + rank_below(m[i])] = base + i * kSelThreads + threadIdx.x;
    }
}

__global__ __launch_bounds__(kThreads) void resolve_samples(ResolveArgs a, uint32_t pixels) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;  // grid * kThreads < 2^31 + kThreads
    if (p >= pixels) return;
    const float4 lo = a.stats[2 * (size_t)p];
    float4 o = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (!(lo.w == 0.0f)) {
        const float g = 0.45454545f;
        o = make_float4(pm_pow(lo.x / lo.w, g), pm_pow(lo.y / lo.w, g), pm_pow(lo.z / lo.w, g), lo.w);
    }
    a.out[p] = o;
}

}  // namespace

hipError_t launch_accumulate(const AccumArgs& a, const rtp::AccumPlan& p, hipStream_t st) {
    if (p.nothing || p.grid == 0 || a.first != p.first || a.count != p.count || a.n_pixels != p.n_pixels ||
        (uint64_t)p.grid * kThreads < p.count || !a.results || !a.stats)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(accumulate_samples, dim3(p.grid), dim3(kThreads), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_select(const SelectArgs& a, const rtp::SelectPlan& p, hipStream_t st) {
    if (p.blocks == 0 || (uint64_t)p.blocks * kSelBlock < p.pixels || (uint64_t)p.width * p.height != p.pixels ||
        !a.stats || !a.ids || !a.result || !a.scratch)
        return hipErrorInvalidValue;
    uint8_t* flags = a.scratch + p.flags_offset;
    uint8_t* sel = a.scratch + p.sel_offset;
    uint32_t* sel_counts = reinterpret_cast<uint32_t*>(a.scratch + p.counts_offset);
    uint32_t* hot_counts = sel_counts + p.blocks;
    uint32_t* offsets = hot_counts + p.blocks;
    const SelectConsts c{p.width, p.height, p.pixels, p.radius, p.blocks, p.threshold, p.floor_y, p.min_samples, p.max_samples};
    hipLaunchKernelGGL(select_flags, dim3(p.blocks), dim3(kSelThreads), 0, st, a.stats, flags, hot_counts, c);
    hipLaunchKernelGGL(select_count, dim3(p.blocks), dim3(kSelThreads), 0, st, flags, sel, sel_counts, c);
    hipLaunchKernelGGL(select_scan, dim3(1), dim3(kScanThreads), 0, st, sel_counts, hot_counts, offsets, p.blocks, a.result);
    hipLaunchKernelGGL(select_scatter, dim3(p.blocks), dim3(kSelThreads), 0, st, sel, offsets, a.ids, p.pixels);
    return hipGetLastError();
}

hipError_t launch_resolve(const ResolveArgs& a, const rtp::ResolvePlan& p, hipStream_t st) {
    if (p.grid == 0 || (uint64_t)p.grid * kThreads < p.pixels || !a.stats || !a.out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(resolve_samples, dim3(p.grid), dim3(kThreads), 0, st, a, p.pixels);
    return hipGetLastError();
}

}  // namespace rta

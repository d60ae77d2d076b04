// rt_kernel_state.hpp -- the device resources a kernel object owns besides its packed scene
// (rt_device_scene.hpp), one type per group, each with the invariant its members keep:
//   LaunchTimer      the event brackets of rtKernelSetTiming and what has been read from them;
//   RadianceSets     the fused frames' radiance and frame-flag buffers and the events ordering them;
//   WavefrontQueues  the wavefront schedule's ray queues, hit records and stream counts;
//   WorkCounters     the chunk counters, sky keys and statistics words, and their layout.
// rt_capi.cpp composes them in rt_kernel_s; a released part holds nothing, so release() may follow a
// creation that failed half way.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>
#include <vector>

#include "rt_internal.hpp"
#include "rt_layout.hpp"

namespace rti {

// Launch timing (rt_stats.kernel_ms, accum_ms, render_period_ms).  Every event the timer has created
// is in exactly one place: a pending pair, first_end_, or the pool -- so release() destroys each once.
class LaunchTimer {
public:
    enum List { kRender, kAccum };  // KernelEntry and the other timed launches; fused frames' accumulation

    // The timing bracket of one launch on `st`: an event before the launch and one after, kept in
    // the list until drain() reads them.  Does nothing when timing is off.
    class Bracket {
    public:
        bool begin();  // false: no events to be had
        void end();

    private:
        friend class LaunchTimer;
        Bracket(LaunchTimer* t, hipStream_t st, List list) : t_(t), st_(st), list_(list) {}
        LaunchTimer* t_;  // null: timing is off
        hipStream_t st_;
        List list_;
        hipEvent_t ev0_ = nullptr, ev1_ = nullptr;
    };
    Bracket bracket(bool timing, hipStream_t st, List list) { return Bracket(timing ? this : nullptr, st, list); }

    // waits for every pending bracket and adds it to the totals
    int drain();
    // after a launch: the brackets nobody has read yet stay bounded
    int drain_if_many() { return pending_[kRender].size() + pending_[kAccum].size() <= 4096 ? RT_SUCCESS : drain(); }
    // the totals and the render period start again (the caller has drained)
    void reset();
    void release();

    double kernel_ms() const { return total_ms_[kRender]; }
    double accum_ms() const { return total_ms_[kAccum]; }
    double render_period_ms() const { return period_intervals_ ? period_span_ms_ / (double)period_intervals_ : 0.0; }

private:
    using EventList = std::vector<std::pair<hipEvent_t, hipEvent_t>>;
    hipEvent_t take_event();
    int drain_list(List which);

    EventList pending_[2];
    std::vector<hipEvent_t> pool_;
    double total_ms_[2] = {};
    // render period: end of the first timed render to end of the latest one
    hipEvent_t first_end_ = nullptr;
    double period_span_ms_ = 0.0;
    uint64_t period_intervals_ = 0;
};

// Fused frames: radiance and primary-miss flag per (frame slot, work-item), RT_RAD_SETS sets used in
// rotation so a render can run while the previous launch's accumulation reads another set.  A set is
// written only after the accumulation that last read it (wait_free), and its buffers are replaced
// only after the accumulation stream has drained (ensure).
class RadianceSets {
public:
    // the set the next fused launch uses (one set without the overlap)
    int current(bool overlap) const { return overlap ? set_ : 0; }
    // set `rs` holds `need` radiance slots and `fneed` frame-flag bytes, and the events that order
    // its renders and accumulations exist
    int ensure(rt_context ctx, int rs, size_t need, size_t fneed);
    // a render on `rstr` writes set `rs`: after the accumulation that last read it
    hipError_t wait_free(int rs, hipStream_t rstr);
    // `as` waits for the render just enqueued on `rstr`
    hipError_t after_render(hipStream_t rstr, hipStream_t as);
    // an accumulation reading the current set was enqueued on `as`: the set is busy until then, `tail`
    // is the stream's new tail, and the next launch takes the next set
    hipError_t accumulated(hipStream_t as, hipEvent_t tail);
    void release();

    float4* radiance(int rs) const { return rad_[rs]; }
    uint8_t* flags(int rs) const { return flags_[rs]; }

private:
    float4* rad_[RT_RAD_SETS] = {};
    uint8_t* flags_[RT_RAD_SETS] = {};
    size_t rad_cap_[RT_RAD_SETS] = {};    // float4 slots
    size_t flags_cap_[RT_RAD_SETS] = {};  // frame-flag bytes
    hipEvent_t free_[RT_RAD_SETS] = {};   // recorded on the accumulation stream after the accumulation reading the set
    bool busy_[RT_RAD_SETS] = {};
    int set_ = 0;
    hipEvent_t render_done_ = nullptr;  // recorded on the render's stream after a fused render
};

// The wavefront schedule's ray queues (two sets of 4 float4 planes), hit records and stream counts
// (2 x (G + 1) words).  They only grow, and only after the stream whose renders read them has drained.
class WavefrontQueues {
public:
    // the queues hold `cap` entries per plane, the counts G streams
    int ensure(size_t cap, uint32_t G, hipStream_t rstr);
    void release();

    float4* queue(int i) const { return q_[i]; }
    float2* hits() const { return hits_; }
    uint32_t* counts(int i, uint32_t G) const { return cnt_ + (size_t)i * (G + 1); }

private:
    float4* q_[2] = {};
    float2* hits_ = nullptr;
    size_t cap_ = 0;  // entries per plane
    uint32_t* cnt_ = nullptr;
    size_t cnt_cap_ = 0;  // words
};

// The persistent schedules' chunk counters, the sky-shortcut keys and the rt_stats words, zeroed once
// at creation.  Counter block: 4 words per radiance set (renders of different sets may run together),
// then two per-frame slots of kMaxParts partitions kPartStride words apart, taken in turn: a launch
// counts in one and zeroes the other.  Keys: [0..3] fused frames, [4..5] per-frame, read and written
// in turn.
class WorkCounters {
public:
    // rt_stats counters kept on the device, then rt_path_kill_info's two (step_body: segments shaded
    // with zero throughput, hits and misses)
    static constexpr int kStatWords = 22;
    static constexpr int kZeroBetaWord = 20;

    // allocated and zeroed through `st`, which is synchronised
    hipError_t create(hipStream_t st);
    void release();

    uint32_t* fused(int rs) const { return counters_ + 4 * rs; }
    uint32_t* per_frame() const { return per_frame_slot(0); }
    uint32_t* per_frame_in_use() const { return per_frame_slot(slot_); }
    uint32_t* per_frame_to_clear() const { return per_frame_slot(slot_ ^ 1); }
    void flip_per_frame_slot() { slot_ ^= 1; }
    uint32_t* fused_keys() const { return keys_; }
    uint32_t* key_in() const { return keys_ + 4 + parity_; }
    uint32_t* key_out() const { return keys_ + 4 + (parity_ ^ 1); }
    void flip_key() { parity_ ^= 1; }
    unsigned long long* stats() const { return stats_; }
    hipError_t zero_stats(hipStream_t st) { return hipMemsetAsync(stats_, 0, kStatBytes, st); }

private:
    static constexpr size_t kSlotWords = (size_t)rtk::kMaxParts * rtk::kPartStride;
    static constexpr size_t kCounterBytes = sizeof(uint32_t) * (4 * RT_RAD_SETS + 2 * kSlotWords);
    static constexpr size_t kKeyBytes = 32;
    static constexpr size_t kStatBytes = kStatWords * sizeof(unsigned long long);
    uint32_t* per_frame_slot(int s) const { return counters_ + 4 * RT_RAD_SETS + s * kSlotWords; }

    uint32_t* counters_ = nullptr;
    uint32_t* keys_ = nullptr;
    unsigned long long* stats_ = nullptr;
    int slot_ = 0;    // per-frame counter slot of the next launch (RT_PF_COUNTER_SLOTS)
    int parity_ = 0;  // per-frame key read by the next launch
};

}  // namespace rti

// rt_kernel_state.cpp -- see rt_kernel_state.hpp.
#include "rt_kernel_state.hpp"

namespace rti {

// ---- LaunchTimer ----------------------------------------------------------------------------------

hipEvent_t LaunchTimer::take_event() {
    if (!pool_.empty()) {
        hipEvent_t e = pool_.back();
        pool_.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

bool LaunchTimer::Bracket::begin() {
    if (!t_) return true;
    ev0_ = t_->take_event();
    ev1_ = t_->take_event();
    if (!ev0_ || !ev1_) return false;
    (void)hipEventRecord(ev0_, st_);
    return true;
}

void LaunchTimer::Bracket::end() {
    if (!t_) return;
    (void)hipEventRecord(ev1_, st_);
    t_->pending_[list_].emplace_back(ev0_, ev1_);
}

int LaunchTimer::drain_list(List which) {
    EventList& list = pending_[which];
    for (auto& pr : list) {
        float ms = 0.0f;
        hipError_t e = hipEventSynchronize(pr.second);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, pr.first, pr.second);
        if (e != hipSuccess) return map_hip(e);
        total_ms_[which] += ms;
        if (which == kRender) {
            // render period: end of the first timed render to end of the latest one
            if (!first_end_) {
                first_end_ = pr.second;
            } else {
                float span = 0.0f;
                e = hipEventElapsedTime(&span, first_end_, pr.second);
                if (e != hipSuccess) return map_hip(e);
                period_span_ms_ = span;
                ++period_intervals_;
                pool_.push_back(pr.second);
            }
            pool_.push_back(pr.first);
            continue;
        }
        pool_.push_back(pr.first);
        pool_.push_back(pr.second);
    }
    list.clear();
    return RT_SUCCESS;
}

int LaunchTimer::drain() {
    const int rc = drain_list(kRender);
    return rc ? rc : drain_list(kAccum);
}

void LaunchTimer::reset() {
    total_ms_[kRender] = total_ms_[kAccum] = 0.0;
    if (first_end_) pool_.push_back(first_end_);
    first_end_ = nullptr;
    period_span_ms_ = 0.0;
    period_intervals_ = 0;
}

void LaunchTimer::release() {
    for (EventList& list : pending_) {
        for (auto& pr : list) {
            (void)hipEventDestroy(pr.first);
            (void)hipEventDestroy(pr.second);
        }
        list.clear();
    }
    if (first_end_) (void)hipEventDestroy(first_end_);
    first_end_ = nullptr;
    for (hipEvent_t e : pool_) (void)hipEventDestroy(e);
    pool_.clear();
}

// ---- RadianceSets ---------------------------------------------------------------------------------

int RadianceSets::ensure(rt_context ctx, int rs, size_t need, size_t fneed) {
    if (rad_cap_[rs] >= need && flags_cap_[rs] >= fneed) return RT_SUCCESS;
    // the set may still be read by an accumulation in flight
    hipError_t me = hipStreamSynchronize(ctx->astream);
    if (me != hipSuccess) return map_hip(me);
    if (rad_[rs]) (void)hipFree(rad_[rs]);
    if (flags_[rs]) (void)hipFree(flags_[rs]);
    rad_[rs] = nullptr;
    flags_[rs] = nullptr;
    rad_cap_[rs] = 0;
    flags_cap_[rs] = 0;
    me = hipMalloc(&rad_[rs], need * sizeof(float4));
    if (me == hipSuccess) me = hipMalloc(&flags_[rs], fneed);
    if (me == hipSuccess && !free_[rs]) me = hipEventCreateWithFlags(&free_[rs], hipEventDisableTiming);
    if (me == hipSuccess && !render_done_) me = hipEventCreateWithFlags(&render_done_, hipEventDisableTiming);
    if (me != hipSuccess) return map_hip(me);
    rad_cap_[rs] = need;
    flags_cap_[rs] = fneed;
    return RT_SUCCESS;
}

hipError_t RadianceSets::wait_free(int rs, hipStream_t rstr) {
    if (!busy_[rs]) return hipSuccess;
    const hipError_t e = hipStreamWaitEvent(rstr, free_[rs], 0);
    if (e == hipSuccess) busy_[rs] = false;
    return e;
}

hipError_t RadianceSets::after_render(hipStream_t rstr, hipStream_t as) {
    const hipError_t e = hipEventRecord(render_done_, rstr);
    return e == hipSuccess ? hipStreamWaitEvent(as, render_done_, 0) : e;
}

hipError_t RadianceSets::accumulated(hipStream_t as, hipEvent_t tail) {
    hipError_t e = hipEventRecord(free_[set_], as);
    if (e == hipSuccess) e = hipEventRecord(tail, as);
    if (e != hipSuccess) return e;
    busy_[set_] = true;
    set_ = (set_ + 1) % RT_RAD_SETS;
    return hipSuccess;
}

void RadianceSets::release() {
    for (int i = 0; i < RT_RAD_SETS; ++i) {
        if (rad_[i]) (void)hipFree(rad_[i]);
        if (flags_[i]) (void)hipFree(flags_[i]);
        if (free_[i]) (void)hipEventDestroy(free_[i]);
        rad_[i] = nullptr;
        flags_[i] = nullptr;
        free_[i] = nullptr;
        rad_cap_[i] = flags_cap_[i] = 0;
        busy_[i] = false;
    }
    if (render_done_) (void)hipEventDestroy(render_done_);
    render_done_ = nullptr;
}

// ---- WavefrontQueues ------------------------------------------------------------------------------

int WavefrontQueues::ensure(size_t cap, uint32_t G, hipStream_t rstr) {
    if (cap_ < cap) {
        // earlier renders on this stream may still read them
        hipError_t me = hipStreamSynchronize(rstr);
        for (float4*& q : q_) {
            if (q) (void)hipFree(q);
            q = nullptr;
        }
        if (hits_) (void)hipFree(hits_);
        hits_ = nullptr;
        cap_ = 0;
        for (float4*& q : q_)
            if (me == hipSuccess) me = hipMalloc(&q, cap * 4 * sizeof(float4));
        if (me == hipSuccess) me = hipMalloc(&hits_, cap * sizeof(float2));
        if (me != hipSuccess) return map_hip(me);
        cap_ = cap;
    }
    const size_t words = 2 * ((size_t)G + 1);
    if (cnt_cap_ < words) {
        hipError_t me = hipStreamSynchronize(rstr);
        if (cnt_) (void)hipFree(cnt_);
        cnt_ = nullptr;
        cnt_cap_ = 0;
        if (me == hipSuccess) me = hipMalloc(&cnt_, words * sizeof(uint32_t));
        if (me != hipSuccess) return map_hip(me);
        cnt_cap_ = words;
    }
    return RT_SUCCESS;
}

void WavefrontQueues::release() {
    for (float4*& q : q_) {
        if (q) (void)hipFree(q);
        q = nullptr;
    }
    if (hits_) (void)hipFree(hits_);
    if (cnt_) (void)hipFree(cnt_);
    hits_ = nullptr;
    cnt_ = nullptr;
    cap_ = cnt_cap_ = 0;
}

// ---- WorkCounters ---------------------------------------------------------------------------------

hipError_t WorkCounters::create(hipStream_t st) {
    hipError_t e = hipMalloc(&stats_, kStatBytes);
    if (e == hipSuccess) e = hipMalloc(&counters_, kCounterBytes);
    if (e == hipSuccess) e = hipMemsetAsync(counters_, 0, kCounterBytes, st);
    if (e == hipSuccess) e = hipMalloc(&keys_, kKeyBytes);
    if (e == hipSuccess) e = hipMemsetAsync(keys_, 0, kKeyBytes, st);
    if (e == hipSuccess) e = zero_stats(st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e;
}

void WorkCounters::release() {
    if (stats_) (void)hipFree(stats_);
    if (counters_) (void)hipFree(counters_);
    if (keys_) (void)hipFree(keys_);
    stats_ = nullptr;
    counters_ = nullptr;
    keys_ = nullptr;
}

}  // namespace rti

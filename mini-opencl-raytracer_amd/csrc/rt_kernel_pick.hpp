// rt_kernel_pick.hpp -- Variant -> KernelEntry entry point, written once for every math policy.
// Host code; rt_kernels.hip and rt_kernels_shipped.hip include it after the device code and list
// their policies' kernels in a rtk::Policy (with wf_pick, rt_wavefront.hpp, and query_pick,
// rt_query.hpp).
#pragma once

#include "rt_kernels_body.hpp"

namespace rtk {

// The step schedule's entry points of policy M.  Their names and register budgets differ per
// policy, so the TU that instantiates M specialises this with
//   template <bool kStats, int kMode> static KernelFn get(Walk w);
template <class M>
struct StepEntry;

template <class M, bool S>
KernelFn pick_entry_s(const Variant& v) {
    if (v.sched != kSchedStep) return v.lds() ? kernel_entry<M, true, S> : kernel_entry<M, false, S>;
    if constexpr (S || !RT_SPECIALIZE_FUSED)
        return StepEntry<M>::template get<S, 0>(v.walk);
    else
        return v.fused ? StepEntry<M>::template get<S, 1>(v.walk) : StepEntry<M>::template get<S, 2>(v.walk);
}
template <class M>
KernelFn pick_entry(const Variant& v) {
    return v.stats ? pick_entry_s<M, true>(v) : pick_entry_s<M, false>(v);
}

}  // namespace rtk

// rt_comm_state.hpp -- what a communicator (rt_comm_s, rtComm*) holds, as parts that each own their
// resources: the world it belongs to, its streams and events, its staging slots, and its copy-engine
// links; beside them the plan (plain values) and the options.  Every owning part has one per-plan
// reset() and one release(); rt_comm.cpp composes them (free_plan, release) and enqueues the gathers.
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <memory>
#include <vector>

#include "rt_comm_files.hpp"
#include "rt_comm_plan.hpp"
#include "rt_internal.hpp"

#ifndef RT_COMM_XFER_STREAMS
#define RT_COMM_XFER_STREAMS 2  // 1: the copies on the communicator stream itself
#endif
static_assert(RT_COMM_XFER_STREAMS >= 1 && RT_COMM_XFER_STREAMS <= 8, "copy streams");

namespace rti {

constexpr size_t kProbeBytes = 4096;  // per rank, the trial round's copy
// flag values 0 .. kFlagValues - 1 (512 KB per rank): the world re-plans, collectively, every
// kFlagValues - 2 gathers (ensure_plan), a few milliseconds once per 65k steps
constexpr uint64_t kFlagValues = 1ull << 16;

int map_nccl(ncclResult_t r);

// The world: its kind names which of the members below are in use.
struct CommWorld {
    rtp::World kind = rtp::World::RcclRank;
    int rank = 0, nranks = 1;
    ncclComm_t nc = nullptr;  // RCCL worlds: also the setup exchanges, reductions and barriers
    // loopback worlds: no RCCL; `group` identifies the world (shared by its members), whose gathers
    // always run on the copy engines with the members linked by address
    const void* group = nullptr;
    // shared worlds: no RCCL; setup exchanges, reductions and barriers go through files, the gathers
    // over the copy engines
    rtp::FileWorld files;
    // one-process worlds (loopback, RcclAll): the members still alive -- a member released before
    // its root joined takes its events out of the root's join (it has drained)
    std::shared_ptr<std::vector<rt_comm>> members;
    double* scratch = nullptr;  // RCCL reductions

    bool loopback() const { return kind == rtp::World::Loopback; }
    bool shared() const { return kind == rtp::World::Shared; }
    bool has_rccl() const { return rtp::has_collectives(kind); }

    int create();  // (on the current device)
    // every rank's `n` bytes in rank order / the world's maximum of v: files in a shared world, else
    // RCCL on stream `s`, which the call drains
    int allgather(const void* mine, size_t n, void* all, hipStream_t s);
    int max(int v, int* out, hipStream_t s);
    void release();
};

// The communicator's streams (transfer, root, and the extra transfer streams) run at the device's
// greatest stream priority.  Read off a kernel trace of the world-1 flow
// (profiles/r04/dist_flow_ab.txt): HIP maps streams onto a few hardware queues (GPU_MAX_HW_QUEUES
// 4); at normal priority the communicator's streams shared the main stream's and a render stream's
// queue, so the next fused render sat behind the previous step's gather.  High-priority streams
// get queues of their own.  (Reserving CUs per XCD for RCCL's transfer kernel let it run at once
// but cost the renders more than it saved -- 0.85 vs 0.82 ms/frame in the same flow; removed in
// round 5.)
struct CommStreams {
    hipStream_t cstream = nullptr;  // transfers (copy engines or RCCL), RCCL setup and reductions
    hipStream_t ustream = nullptr;  // root: releases (copy engines), unpack (RCCL)
    // the copies split over streams of their own, which the runtime spreads over several SDMA
    // engines (one engine: 61 GB/s; 2 streams 120, 8 streams 154 GB/s on MI355X,
    // scripts/probes/gather_engines_probe.hip split, profiles/r04/gather_engines_probe.txt).
    // Every stream shares the 4 hardware queues, though: in the world-1 flow 2 streams beat 1
    // (0.790 vs 0.798 ms/frame) and 8 stalled the renders (1.17; profiles/r04/dist_flow_ab.txt)
    hipStream_t xstream[8] = {};
    hipEvent_t xgo = nullptr, xdone[8] = {};
    hipEvent_t ready = nullptr;     // the root's bands of `out` are final (accumulation stream)
    hipEvent_t dsent = nullptr;     // the root's own copies (gathering into another buffer) are done
    hipEvent_t released = nullptr;  // root: the previous image is released (unpack stream)
    hipEvent_t xt0 = nullptr, xt1 = nullptr;  // timing: the last gather's transfer on cstream
    bool xt_valid = false;

    int create();       // (on the current device)
    void sync() const;  // every stream idle
    void reset() { xt_valid = false; }
    void release();
};

// Staging: ranks sending to another rank's root (copy engines); every rank (RCCL).  Two slots
// alternate, so step k's transfer runs under step k+1's render.
struct CommStaging {
    size_t bytes = 0;     // per rank: the largest rank's share (rtBandPackPlan)
    void* stage[2] = {};  // this rank's packed bands
    void* parts[2] = {};  // RCCL root: nranks x bytes received bands
    hipEvent_t packed[2] = {}, sent[2] = {}, unpacked[2] = {};
    bool sent_valid[2] = {}, unpacked_valid[2] = {};
    int slot = 0;

    int create();  // the events
    // the slots this plan still lacks; receive_ranks > 0 (an RCCL root): its receive slots too
    int ensure(int receive_ranks);
    void reset();
    void release();
};

// The copy-engine links of a plan: the root's destination as every rank addresses it, and the flags.
struct CommLinks {
    bool ce = false;          // this plan moves bytes on the copy engines
    bool ipc_linked = false;  // ... with its links exchanged as IPC handles (link_ipc)
    // root: other devices' copy engines write its destination, so its first read of a gathered
    // image runs a system-scope acquire on every XCD first (join_gather; RT_COMM_OPT_SYSTEM_ACQUIRE
    // forces it on one device)
    bool remote_writers = false;
    rt_mem target = nullptr;         // root: the plan's destination (pinned)
    uint8_t* peer_target = nullptr;  // the root's destination as this rank addresses it
    uint64_t* sflags = nullptr;      // [1] (fine-grained, this rank's memory): image released by the root, seq
    uint64_t* rflags = nullptr;      // root, [nranks] (fine-grained): rank q's bands of image seq in place
    uint8_t* probe = nullptr;        // root, [nranks][kProbeBytes] (fine-grained): the trial round's copies
    uint8_t* peer_probe = nullptr;
    uint64_t* peer_rflags = nullptr;     // the root's arrival flags, as this rank addresses them
    std::vector<uint64_t*> peer_sflags;  // root: every rank's release flag
    std::vector<void*> ipc_opened;       // IPC mappings to close with the plan
    uint64_t* vals = nullptr;        // device: vals[i] = i, the sources of the flag copies (kFlagValues)
    uint64_t join_seq = 0;           // root, IPC links: the gather whose arrivals the next read joins
    std::vector<hipEvent_t> join_events;  // root, one process: the ranks' `sent` events of that gather

    // the root's destination, pinned until the plan lets go of it
    void aim(rt_mem dst);
    void unpin();
    // The release and arrival flags and the probe are fine-grained memory (written by other
    // devices' engines, read coherently by the waits and the host), each its own allocation (an IPC
    // handle maps a whole allocation); zeroed, and the device drained.
    int alloc_flags(bool is_root, int nranks);
    int flag_values();  // the flag values' source array, once per communicator
    // a flag word (another device's, or this one's) := v, on the copy engine of stream s
    hipError_t flag_copy(uint64_t* dst, uint64_t v, hipStream_t s) const {
        return hipMemcpyAsync(dst, vals + v, sizeof(uint64_t), hipMemcpyDeviceToDeviceNoCU, s);
    }
    void unmap();  // the IPC mappings closed, the peers' addresses forgotten
    void reset();
    void release();
};

// The plan: one (width, height, root, destination); rebuilt when any changes.
struct CommPlan {
    rtp::PlanId id;
    std::vector<std::vector<rt_rect>> rects;  // per rank: its bands as 2-D rects (rtBandPackPlan)
    std::vector<rtp::Run> runs;               // this rank's band runs
    bool sends = false;  // this rank copies its bands (all but a root gathering into its out)
    uint64_t seq = 0;    // gathers enqueued with this plan (1, 2, ...)
    int fallback_reason = RT_COMM_FALLBACK_NONE;  // the plan wanted the copy engines and runs RCCL
    // being built by the gather in progress and not linked yet: a call that fails before the commit
    // frees it, so a comm never keeps a half-built plan
    bool building = false;

    bool planned() const { return id.W != 0; }
    void reset();
};

struct CommOptions {
    int transport = RT_COMM_TRANSPORT_COPY_ENGINES;  // requested (rtCommSetTransport)
    bool fail_links = false;                    // test hook (RT_COMM_OPT_FAIL_LINKS)
    uint64_t replan_after = kFlagValues - 2;    // gathers per plan (RT_COMM_OPT_REPLAN_PERIOD)
    bool force_acquire = false;                 // RT_COMM_OPT_SYSTEM_ACQUIRE
};

}  // namespace rti

struct rt_comm_s {
    rt_context ctx = nullptr;
    rti::CommWorld world;
    rti::CommOptions opt;
    rti::CommPlan plan;
    rti::CommStreams st;
    rti::CommStaging stage;
    rti::CommLinks links;
};

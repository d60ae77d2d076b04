// rt_comm.cpp -- multi-GPU band sharding + gather, behind include/rt_hip.h.
//
// The reference is single-device (CLRaytracer.cpp:104-120, one in-order queue CLutils.cpp:29).
// A frame shards with no exchange until the image is needed, because every pixel's seed is
// gid + HashUInt32(frameCount) over the GLOBAL work-item id (kernel_bvh.cl:445) and the gamma
// accumulation is per pixel (:449-455).  Rank r renders the interleaved 8-row bands
// b % nranks == r into its full-size output buffer (rtKernelSetRowInterleave), at the rows they
// occupy in the image; the gather moves them to the root.
//
// Copy-engine transport (default): nothing in a gather's steady state needs a compute unit.  A
// persistent render holds every CU slot until it drains, and anything that needs one -- RCCL's
// transfer kernel, the runtime's 2-D blit copies, and ROCclr's hipStreamWriteValue64 /
// hipStreamWaitValue64, which run as kernels (__amd_rocclr_streamOps*) -- waits behind it and then
// crawls beside it (profiles/r04/dist_flow_ab.txt, profiles/r05/flag_probe.txt).  So the bytes AND
// the flags move on the copy engines (SDMA, hipMemcpyDeviceToDeviceNoCU; over xGMI between GPUs):
//
//   rank q accumulation stream : [accumulate k] [pack k -> stage[s] (SDMA, per band)] [accumulate k+1]
//   rank q comm stream         :     (packed k)(release k-1) [bands -> root image (SDMA)] [arrive k (SDMA)]
//   root unpack stream         : (root's queue so far) [release k-1 -> every rank (SDMA)]
//   root, first read of image k: (wait arrive k from every rank)
//
// * The pack copies the rank's bands densely into one of two staging slots right after the
//   accumulation, on the accumulation stream: the next accumulation never waits for anything
//   across GPUs.  The transfer writes every band from the slot into the rows it occupies in the
//   root's destination -- mapped into the rank by IPC handle (one ncclAllGather per plan), or by
//   address for ranks driven by one process: no receive slot, no unpack.
// * `release k-1` (a flag in each rank's memory, written by the root's copy engine once everything
//   its context queued before gather k -- reads of image k-1 -- has run): a rank's copies never
//   change the root's image under a read.  The rank's wait for it is the one waiting kernel of a
//   gather, and it gates only the transfer.
// * `arrive k` (a flag per rank in the root's memory, written by the rank's copy engine after its
//   bands): the root joins the arrivals only when it next reads (rti::join_gather, from qs): no
//   kernel spins on the root while nobody looks at the image.
// * The root gathering into another buffer copies its own bands straight from its output (local
//   copies, ordered by events); gathering into its output, they are in place.
// * Flag values are copied from a device array holding 0, 1, 2, ... (vals); a plan is rebuilt
//   before the gather count reaches its end (every rank at the same gather).
//
// RCCL transport (RT_COMM_TRANSPORT_RCCL, and the fallback of a world whose copy-engine links do
// not hold): each rank packs its bands densely into a staging slot on its accumulation stream,
// grouped ncclSend/ncclRecv move the slots to the root, the root unpacks them; two slots alternate
// so step k's transfer runs under step k+1's render.  RCCL also carries the setup exchanges,
// reductions and barriers.
//
// Where the rules live: what can be said over plain values -- the band plan, the deal of the runs
// over the transfer streams, when a plan is current, how a fresh one is linked, who must be in a
// call, the status counts, the reductions' fold -- is rt_comm_plan.cpp; a shared world's file
// exchange is rt_comm_files.cpp; what a communicator owns is rt_comm_state.{hpp,cpp}.  This file
// plans, links and enqueues.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <thread>
#include <new>
#include <utility>
#include <vector>

#include "../../include/rt_hip.h"
#include "rt_comm_state.hpp"

using rti::kProbeBytes;
using rti::map_hip;
using rti::map_nccl;
using rti::qs;

namespace {

// A system-scope acquire on the CU each workgroup runs on: its L1 and its XCD's L2 drop what they
// cached of memory that another device may have written (buffer_inv sc0 sc1 on gfx950).  One
// workgroup per CU: the dispatcher deals workgroups round-robin over the 8 XCDs, so every XCD's L2
// sees at least one (the kernel itself reads and writes nothing).
__global__ void system_acquire_kernel() {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the invalidate has completed when the wave ends
}

// the root's acquire on `s`, where other devices write its image (or the test hook asks for it)
hipError_t system_acquire(rt_comm c, hipStream_t s) {
    if (!c->links.remote_writers && !c->opt.force_acquire) return hipSuccess;
    hipLaunchKernelGGL(system_acquire_kernel, dim3(c->ctx->num_cus > 0 ? c->ctx->num_cus : 256), dim3(64), 0, s);
    return hipGetLastError();
}

// No plan: every part back to where a new communicator has it (the streams idle: quiesce).
void free_plan(rt_comm c) {
    c->links.reset();
    c->stage.reset();
    c->plan.reset();
    c->st.reset();
    if (c->ctx->oread_ev == c->st.dsent) c->ctx->oread = false;
    if (c->ctx->gjoin == c) c->ctx->gjoin = nullptr;
}

void release(rt_comm c) {
    (void)hipSetDevice(c->ctx->device);
    c->st.sync();
    if (c->world.members) {  // (its transfers have drained: nobody needs to wait for its events)
        auto& m = *c->world.members;
        m.erase(std::remove(m.begin(), m.end(), c), m.end());
        for (rt_comm o : m) {
            auto& j = o->links.join_events;
            j.erase(std::remove_if(j.begin(), j.end(),
                                   [&](hipEvent_t ev) { return ev == c->stage.sent[0] || ev == c->stage.sent[1]; }),
                    j.end());
        }
    }
    free_plan(c);
    if (c->ctx->oread_ev == c->st.dsent) c->ctx->oread_ev = nullptr;
    c->stage.release();
    c->links.release();
    c->world.release();  // (the RCCL communicator before its stream)
    c->st.release();
    delete c;
}

// Every stream of the communicator (and the context's accumulation stream, whose accumulations
// a gather may follow) idle: a plan can be torn down.
void quiesce(rt_comm c) {
    c->st.sync();
    (void)hipStreamSynchronize(c->ctx->astream);
}

// staging for the RCCL transport: every rank's slots and the root's receive slots
int rccl_staging(rt_comm c) { return c->stage.ensure(c->world.rank == c->plan.id.root ? c->world.nranks : 0); }

// The plan of a W x H gather into `dst` (the root's destination; ranks other than the root pass
// nullptr) from `out` -- all earlier gathers of this comm have completed when it is rebuilt.  A
// copy-engine plan writes into the destination it was linked to, so a new one rebuilds it (the
// RCCL transport unpacks into whatever the call names); so does a gather count about to run past
// the flag values (every rank of the world at the same gather).  A plan that is rebuilt is
// `building` from here until the gather has linked it (commit, in rtCommEnqueueGatherBands).
int ensure_plan(rt_comm c, unsigned W, unsigned H, int root, rt_mem dst, rt_mem out) {
    const rti::CommWorld& w = c->world;
    const bool is_root = w.rank == root;
    if (rtp::plan_current(c->plan.id, W, H, root, is_root, c->links.ce, dst == c->links.target, c->plan.seq,
                          c->opt.replan_after))
        return RT_SUCCESS;
    quiesce(c);
    free_plan(c);
    c->plan.building = true;
    c->plan.rects.assign(w.nranks, {});
    size_t sb = 0;
    for (int q = 0; q < w.nranks; ++q) {
        rt_rect r[2];
        int n = 0;
        int rc = rtp::band_plan(W, H, (unsigned)w.nranks, (unsigned)q, r, 2, &n, &sb);
        if (rc) return rc;
        c->plan.rects[q].assign(r, r + n);
    }
    c->stage.bytes = sb;
    c->plan.id = rtp::PlanId{W, H, root};
    if (is_root) c->links.aim(dst);
    // the root gathering into its own output has its bands in place already
    c->plan.sends = !is_root || dst != out;
    if (c->opt.transport == RT_COMM_TRANSPORT_RCCL) return rccl_staging(c);
    c->plan.runs = rtp::band_runs(c->plan.rects[w.rank]);
    if (!is_root) {
        const int rc = c->stage.ensure(0);
        if (rc) return rc;
    }
    return c->links.alloc_flags(is_root, w.nranks);
}

// Copy-engine links of a plan whose members are all in this call (loopback worlds, and RCCL
// worlds driven by one process): the root's destination by address, the steps ordered by events.
// Between devices the copy engines reach peer memory once peer access is on.
int link_direct(const rt_comm* comms, int n_local, int root) {
    rt_comm R = nullptr;
    for (int i = 0; i < n_local; ++i)
        if (comms[i]->world.rank == root) R = comms[i];
    if (!R) return RT_INVALID_VALUE;
    for (int i = 0; i < n_local; ++i) {
        rt_comm c = comms[i];
        if (c->ctx->device != R->ctx->device) {
            int can = 0;
            hipError_t e = hipDeviceCanAccessPeer(&can, c->ctx->device, R->ctx->device);
            if (e != hipSuccess || !can) return RT_INVALID_OPERATION;
            for (auto [a, b] : {std::pair<int, int>{c->ctx->device, R->ctx->device}, {R->ctx->device, c->ctx->device}}) {
                (void)hipSetDevice(a);
                e = hipDeviceEnablePeerAccess(b, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return map_hip(e);
                (void)hipGetLastError();
            }
        }
    }
    for (int i = 0; i < n_local; ++i) {
        comms[i]->links.peer_target = static_cast<uint8_t*>(R->links.target->dptr);
        comms[i]->links.ce = true;
        if (comms[i]->ctx->device != R->ctx->device) R->links.remote_writers = true;
    }
    return RT_SUCCESS;
}

struct IpcBlob {
    hipIpcMemHandle_t target, rflags, probe, sflags;
};

// the host waits for `s` until `deadline` (no hang: a stream stuck on a flag is reported)
bool wait_until(hipStream_t s, std::chrono::steady_clock::time_point deadline) {
    for (;;) {
        const hipError_t q = hipStreamQuery(s);
        if (q == hipSuccess) return true;
        if (q != hipErrorNotReady || std::chrono::steady_clock::now() > deadline) return false;
        std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
}

// reads `n` u64 words of device memory until every word equals `v` or the deadline passes
bool poll_words(const uint64_t* dev, size_t n, uint64_t v, std::chrono::steady_clock::time_point deadline) {
    std::vector<uint64_t> h(n);
    for (;;) {
        if (hipMemcpy(h.data(), dev, h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) return false;
        bool all = true;
        for (size_t i = 0; i < n; ++i) all &= h[i] == v;
        if (all) return true;
        if (std::chrono::steady_clock::now() > deadline) return false;
        std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
}

// One trial round over fresh IPC links, with the production signalling: every rank copies a 4-KB
// pattern into its part of the root's probe and its arrival flag := 1 (copy engines); the root
// waits for every flag (from the host, then -- once they are in memory -- with the stream waits a
// read of the image uses), checks every pattern, copies release := 1 into every rank's flag; each
// rank waits for its own the same two ways; all flags go back to 0.  Returns 1 when anything
// failed or timed out.
int ipc_handshake(rt_comm c) {
    const rti::CommWorld& w = c->world;
    rti::CommLinks& l = c->links;
    const hipStream_t cstream = c->st.cstream, ustream = c->st.ustream;
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(20);
    uint8_t* src = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&src), kProbeBytes);
    if (e == hipSuccess) e = hipMemsetAsync(src, (w.rank + 1) & 0xff, kProbeBytes, cstream);
    if (e == hipSuccess)
        e = hipMemcpyAsync(l.peer_probe + (size_t)w.rank * kProbeBytes, src, kProbeBytes, hipMemcpyDeviceToDeviceNoCU,
                           cstream);
    if (e == hipSuccess) e = l.flag_copy(l.peer_rflags + w.rank, 1, cstream);
    const bool sent_ok = e == hipSuccess && wait_until(cstream, deadline);
    if (src) (void)hipFree(src);
    if (!sent_ok) return 1;
    if (w.rank == c->plan.id.root) {
        if (!poll_words(l.rflags, (size_t)w.nranks, 1, deadline)) return 1;
        for (int q = 0; q < w.nranks && e == hipSuccess; ++q)
            e = hipStreamWaitValue64(ustream, l.rflags + q, 1, hipStreamWaitValueGte, ~0ull);
        if (e != hipSuccess || !wait_until(ustream, deadline)) return 1;
        std::vector<uint8_t> got(kProbeBytes);
        for (int q = 0; q < w.nranks; ++q) {
            if (hipMemcpy(got.data(), l.probe + (size_t)q * kProbeBytes, kProbeBytes, hipMemcpyDeviceToHost) != hipSuccess)
                return 1;
            for (uint8_t b : got)
                if (b != (uint8_t)((q + 1) & 0xff)) return 1;
        }
        for (int q = 0; q < w.nranks && e == hipSuccess; ++q) e = l.flag_copy(l.peer_sflags[q], 1, ustream);
        if (e == hipSuccess) e = hipMemsetAsync(l.rflags, 0, sizeof(uint64_t) * w.nranks, ustream);
        if (e != hipSuccess || !wait_until(ustream, deadline)) return 1;
    }
    if (!poll_words(l.sflags, 1, 1, deadline)) return 1;
    e = hipStreamWaitValue64(cstream, l.sflags, 1, hipStreamWaitValueGte, ~0ull);
    if (e != hipSuccess || !wait_until(cstream, deadline)) return 1;
    e = hipMemset(l.sflags, 0, sizeof(uint64_t));
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return e == hipSuccess ? 0 : 1;
}

// The same links across processes: every rank publishes IPC handles of its allocations (the
// root: destination, arrival flags and probe; everyone: release flag) with one all-gather through
// the world (ncclAllGather, or a shared world's files), maps the ones it needs, and the world agrees
// (its maximum) whether every rank could -- if one could not, the whole world keeps the RCCL
// transport for this plan.
int link_ipc(rt_comm c) {
    rti::CommWorld& w = c->world;
    rti::CommLinks& l = c->links;
    const bool is_root = w.rank == c->plan.id.root;
    hipError_t e = hipSetDevice(c->ctx->device);
    IpcBlob mine{};
    // 0: links hold; RT_COMM_FALLBACK_IPC_MAP / _HANDSHAKE: why not (the world agrees on the max)
    int bad = c->opt.fail_links ? RT_COMM_FALLBACK_HANDSHAKE : 0;
    if (e == hipSuccess && l.flag_values() != RT_SUCCESS) bad = RT_COMM_FALLBACK_HANDSHAKE;
    if (e == hipSuccess) e = hipIpcGetMemHandle(&mine.sflags, l.sflags);
    if (e == hipSuccess && is_root) {
        e = hipIpcGetMemHandle(&mine.target, l.target->dptr);
        if (e == hipSuccess) e = hipIpcGetMemHandle(&mine.rflags, l.rflags);
        if (e == hipSuccess) e = hipIpcGetMemHandle(&mine.probe, l.probe);
    }
    if (e != hipSuccess) bad = std::max(bad, (int)RT_COMM_FALLBACK_IPC_MAP);
    std::vector<IpcBlob> all(w.nranks);
    auto open = [&](const hipIpcMemHandle_t& h) -> void* {
        void* p = nullptr;
        if (bad) return nullptr;
        if (hipIpcOpenMemHandle(&p, h, hipIpcMemLazyEnablePeerAccess) != hipSuccess) {
            bad = RT_COMM_FALLBACK_IPC_MAP;
            return nullptr;
        }
        l.ipc_opened.push_back(p);
        return p;
    };
    int rc = w.allgather(&mine, sizeof(mine), all.data(), c->st.cstream);
    if (!rc) {
        if (is_root) {
            l.peer_target = static_cast<uint8_t*>(l.target->dptr);
            l.peer_rflags = l.rflags;
            l.peer_probe = l.probe;
            l.peer_sflags.assign(w.nranks, nullptr);
            for (int q = 0; q < w.nranks; ++q)
                l.peer_sflags[q] = q == w.rank ? l.sflags : static_cast<uint64_t*>(open(all[q].sflags));
        } else {
            const IpcBlob& r = all[c->plan.id.root];
            l.peer_target = static_cast<uint8_t*>(open(r.target));
            l.peer_rflags = static_cast<uint64_t*>(open(r.rflags));
            l.peer_probe = static_cast<uint8_t*>(open(r.probe));
        }
        // does every rank hold its links?
        rc = w.max(bad, &bad, c->st.cstream);
    }
    // the links hold: one small transfer and both flags across the world, polled from the host
    // with a deadline, before any gather relies on them (a world whose first real gather waited on
    // a flag that never arrives would hang instead of falling back)
    if (!rc && !bad) {
        bad = ipc_handshake(c) ? RT_COMM_FALLBACK_HANDSHAKE : 0;
        rc = w.max(bad, &bad, c->st.cstream);
    }
    if (rc) return rc;
    if (bad && !w.has_rccl()) return RT_INVALID_OPERATION;  // a shared world has no RCCL to fall back to
    if (bad) {  // the world falls back to RCCL transfers for this plan
        l.unmap();
        l.ce = false;
        c->plan.fallback_reason = bad;
        return rccl_staging(c);
    }
    l.ce = l.ipc_linked = true;
    // one process per GPU (an RCCL world): the other ranks' copy engines write the root's image
    // from other devices (a shared world's ranks all run on one)
    l.remote_writers = is_root && w.nranks > 1 && !w.shared();
    return RT_SUCCESS;
}

// The links of the fresh plans of a call (every rank of the world builds its plan at the same
// gather).  The root's destination is part of a copy-engine plan: linked by address (every rank in
// this call) a new one rebuilds it; linked by IPC handles the root cannot tell the other processes,
// so it refuses a new destination until a collective re-plan (rtCommEnqueueGatherBands).
int link_plans(const rt_comm* comms, int n_local, int root) {
    const rt_comm c0 = comms[0];
    switch (rtp::link_choice(c0->opt.transport, c0->world.kind, n_local, c0->world.nranks)) {
        case rtp::Link::Refuse: return RT_INVALID_OPERATION;
        case rtp::Link::None: return RT_SUCCESS;
        case rtp::Link::Ipc: return link_ipc(c0);
        case rtp::Link::Direct: break;
    }
    int rc = link_direct(comms, n_local, root);  // every member is in this call
    if (rc && !c0->world.loopback()) {           // (RCCL world: keep RCCL's transfers)
        rc = RT_SUCCESS;
        for (int i = 0; i < n_local && !rc; ++i) {
            comms[i]->links.ce = false;
            comms[i]->plan.fallback_reason = RT_COMM_FALLBACK_NO_PEER_ACCESS;
            rc = rccl_staging(comms[i]);
        }
    }
    return rc;
}

// The plans of a gather, current or rebuilt and linked: everything that can fail before the first
// stream operation.  The caller frees the plans still `building` when this fails.
int plan_gather(const rt_comm* comms, const rt_mem* outs, int n_local, unsigned W, unsigned H, int root,
                rt_mem root_dst, bool* on_copy_engines) {
    bool fresh = false;
    for (int i = 0; i < n_local; ++i) {
        rt_comm c = comms[i];
        hipError_t e = hipSetDevice(c->ctx->device);
        if (e != hipSuccess) return map_hip(e);
        const bool is_root = c->world.rank == root;
        rt_mem dst = is_root ? (root_dst ? root_dst : outs[i]) : nullptr;
        if (c->links.ipc_linked && is_root && c->plan.id.W == W && c->plan.id.H == H && c->plan.id.root == root &&
            c->links.target != dst)
            return RT_INVALID_OPERATION;
        int rc = ensure_plan(c, W, H, root, dst, outs[i]);
        if (rc) return rc;
        fresh |= c->plan.building;
    }
    if (fresh)
        if (int rc = link_plans(comms, n_local, root)) return rc;
    // only a copy-engine plan writes into the destination it was built with: an RCCL plan (asked
    // for, or a fallback) unpacks into whatever each call names, so it keeps no pin on the first one
    bool ce = true;
    for (int i = 0; i < n_local; ++i) {
        if (fresh && !comms[i]->links.ce) comms[i]->links.unpin();
        ce &= comms[i]->links.ce;
    }
    // loopback and shared worlds move bytes on the copy engines only
    if (!comms[0]->world.has_rccl() && !ce) return RT_INVALID_OPERATION;
    for (int i = 0; i < n_local; ++i) comms[i]->plan.building = false;  // commit
    *on_copy_engines = ce;
    return RT_SUCCESS;
}

// pack / unpack copies of the RCCL transport (the runtime runs 2-D device copies as blit kernels)
hipError_t copy_rects(const std::vector<rt_rect>& plan, uint8_t* img, uint8_t* stage, bool to_stage, hipStream_t s) {
    for (const rt_rect& r : plan) {
        hipError_t e = to_stage
            ? hipMemcpy2DAsync(stage + r.stage_offset, r.width, img + r.img_offset, r.img_pitch, r.width, r.rows,
                               hipMemcpyDeviceToDevice, s)
            : hipMemcpy2DAsync(img + r.img_offset, r.img_pitch, stage + r.stage_offset, r.width, r.width, r.rows,
                               hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// Copies of this rank's band runs on the copy engines: run i (image offset o_i, n_i bytes, dense
// offset d_i -- its place in the staging slot) from src + (src_dense ? d_i : o_i) to
// dst + (dst_dense ? d_i : o_i).  On stream `s` alone, or (split) dealt out over the transfer
// streams in image order in pieces of at least 1 MiB (rtp::deal_runs), after and before everything
// on `s`.
hipError_t copy_runs(rt_comm c, hipStream_t s, bool split, uint8_t* dst, bool dst_dense, const uint8_t* src,
                     bool src_dense) {
    const std::vector<rtp::Run>& runs = c->plan.runs;
    const std::vector<rtp::Piece> pieces = rtp::deal_runs(runs, RT_COMM_XFER_STREAMS, split);
    const bool own = pieces.empty() || pieces.back().stream == 0;  // one stream: `s` itself
    const rti::CommStreams& st = c->st;
    hipError_t e = own ? hipSuccess : hipEventRecord(st.xgo, s);
    for (size_t i = 0; i < pieces.size() && e == hipSuccess; ++i) {
        const rtp::Piece& p = pieces[i];
        const hipStream_t on = own ? s : st.xstream[p.stream];
        if (!own && (i == 0 || pieces[i - 1].stream != p.stream)) e = hipStreamWaitEvent(on, st.xgo, 0);
        const uint64_t o = runs[p.run].first + p.at;
        if (e == hipSuccess)
            e = hipMemcpyAsync(dst + (dst_dense ? p.dense : o), src + (src_dense ? p.dense : o), p.bytes,
                               hipMemcpyDeviceToDeviceNoCU, on);
        if (!own && (i + 1 == pieces.size() || pieces[i + 1].stream != p.stream)) {
            if (e == hipSuccess) e = hipEventRecord(st.xdone[p.stream], on);
            if (e == hipSuccess) e = hipStreamWaitEvent(s, st.xdone[p.stream], 0);
        }
    }
    return e;
}

// Copy-engine gather (see the top of the file).  Flags carry the gather's sequence number seq
// (1, 2, ... within a plan): rflags[q] = seq when rank q's bands of image seq are in the root's
// destination, sflags = seq when the root has released image seq (everything its context queued
// before gather seq + 1 has run) -- a rank's transfer of image seq + 1 waits for it.  Ranks driven
// by this process (loopback worlds, rtCommInitAll) order the same steps with events instead (the
// root's `released`, the ranks' `sent`), joined by the root at once (events wait without a
// kernel).
int ce_gather(const rt_comm* comms, int n_local, int root, const rt_mem* outs) {
    rt_comm R = nullptr;  // the root, when it is driven by this call
    rt_mem Rout = nullptr;
    for (int i = 0; i < n_local; ++i)
        if (comms[i]->world.rank == root) {
            R = comms[i];
            Rout = outs[i];
        }
    // 1. the root releases the previous image once everything its context queued so far has run
    if (R) {
        rti::CommStreams& st = R->st;
        hipError_t e = hipSetDevice(R->ctx->device);
        const uint64_t prev = R->plan.seq;
        if (e == hipSuccess) e = rti::main_tail_wait(R->ctx, st.ustream);
        // (reads on the accumulation stream: rtContextSetReadbackOnAccumStream)
        if (e == hipSuccess && R->ctx->readback_on_astream) e = hipStreamWaitEvent(st.ustream, R->ctx->atail, 0);
        for (int q = 0; R->links.ipc_linked && prev > 0 && q < R->world.nranks && e == hipSuccess; ++q)
            if (q != root) e = R->links.flag_copy(R->links.peer_sflags[q], prev, st.ustream);
        if (e == hipSuccess) e = hipEventRecord(st.released, st.ustream);
        // 1b. gathering into another buffer, the root copies its own bands there straight from its
        // output: after the accumulations and per-frame launches that wrote them, after the reads
        // of the previous image; the next accumulation waits for the copies (out_read_wait)
        if (e == hipSuccess && R->plan.sends) {
            rt_context ctx = R->ctx;
            ++R->plan.seq;
            e = rti::main_tail_wait(ctx, ctx->astream);
            if (e == hipSuccess) e = hipEventRecord(st.ready, ctx->astream);
            if (e == hipSuccess) e = hipStreamWaitEvent(st.cstream, st.ready, 0);
            if (e == hipSuccess) e = hipStreamWaitEvent(st.cstream, st.released, 0);
            if (e == hipSuccess) e = hipEventRecord(st.xt0, st.cstream);
            if (e == hipSuccess)
                e = copy_runs(R, st.cstream, true, static_cast<uint8_t*>(R->links.target->dptr), false,
                              static_cast<const uint8_t*>(Rout->dptr), false);
            if (e == hipSuccess) e = hipEventRecord(st.xt1, st.cstream);
            if (e == hipSuccess) e = hipEventRecord(st.dsent, st.cstream);
            if (e == hipSuccess) {
                st.xt_valid = true;
                ctx->oread_ev = st.dsent;
                ctx->oread = true;
            }
        } else if (e == hipSuccess) {
            ++R->plan.seq;
        }
        if (e != hipSuccess) return map_hip(e);
    }
    // 2. every other rank: pack its bands into a staging slot right after the accumulation
    // (accumulation stream: the next accumulation never waits across GPUs), then -- once the root
    // has released the previous image -- transfer them into the root's destination and raise its
    // arrival flag, all on the copy engines
    for (int i = 0; i < n_local; ++i) {
        rt_comm c = comms[i];
        if (c == R) continue;
        rt_context ctx = c->ctx;
        rti::CommStreams& st = c->st;
        rti::CommStaging& sg = c->stage;
        const rti::CommLinks& l = c->links;
        const uint64_t seq = ++c->plan.seq;
        const int s = sg.slot;
        hipError_t e = hipSetDevice(ctx->device);
        if (e == hipSuccess) e = rti::main_tail_wait(ctx, ctx->astream);
        if (e == hipSuccess && sg.sent_valid[s]) e = hipStreamWaitEvent(ctx->astream, sg.sent[s], 0);  // slot free
        if (e == hipSuccess)
            e = copy_runs(c, ctx->astream, false, static_cast<uint8_t*>(sg.stage[s]), true,
                          static_cast<const uint8_t*>(outs[i]->dptr), false);
        if (e == hipSuccess) e = hipEventRecord(sg.packed[s], ctx->astream);
        if (e == hipSuccess) e = hipEventRecord(ctx->atail, ctx->astream);
        if (e == hipSuccess) ctx->apending = true;
        if (e == hipSuccess) e = hipStreamWaitEvent(st.cstream, sg.packed[s], 0);
        if (e == hipSuccess && seq > 1) {  // the root is done with the previous image
            e = l.ipc_linked ? hipStreamWaitValue64(st.cstream, l.sflags, seq - 1, hipStreamWaitValueGte, ~0ull)
                             : hipStreamWaitEvent(st.cstream, R->st.released, 0);
        }
        if (e == hipSuccess) e = hipEventRecord(st.xt0, st.cstream);
        if (e == hipSuccess)
            e = copy_runs(c, st.cstream, !(!l.ipc_linked && c->world.nranks > 1), l.peer_target, false,
                          static_cast<const uint8_t*>(sg.stage[s]), true);
        if (e == hipSuccess) e = hipEventRecord(st.xt1, st.cstream);
        if (e == hipSuccess && l.ipc_linked) e = l.flag_copy(l.peer_rflags + c->world.rank, seq, st.cstream);
        if (e == hipSuccess) e = hipEventRecord(sg.sent[s], st.cstream);
        // reads on this rank's context wait for its transfer (qs)
        if (e == hipSuccess) e = hipEventRecord(ctx->gtail, st.cstream);
        if (e != hipSuccess) return map_hip(e);
        sg.sent_valid[s] = true;
        st.xt_valid = true;
        ctx->gpending = true;
        sg.slot ^= 1;
    }
    // 3. the root's context joins the arrivals when the image is next read (join_gather): flag
    // waits between processes, the ranks' events within one.  Nothing waits at gather time: even
    // an event wait on the root's stream cost the world-1 flow 2 % (0.804 vs 0.788 ms/frame,
    // profiles/r05/gather_world1_ab.txt)
    if (R) {
        rti::CommLinks& l = R->links;
        auto sent = [](rt_comm c) { return c->stage.sent[c->stage.slot ^ 1]; };  // of the gather just enqueued
        l.join_seq = R->plan.seq;
        l.join_events.clear();
        if (!l.ipc_linked && !R->world.members && n_local > 1) {  // (no member list: join now, on the root's stream)
            const hipStream_t us = R->st.ustream;
            hipError_t e = hipSetDevice(R->ctx->device);
            for (int j = 0; j < n_local && e == hipSuccess; ++j)
                if (comms[j] != R) e = hipStreamWaitEvent(us, sent(comms[j]), 0);
            if (e == hipSuccess && R->plan.sends) e = hipStreamWaitEvent(us, R->st.dsent, 0);
            if (e == hipSuccess) e = system_acquire(R, us);  // (see join_gather)
            if (e == hipSuccess) e = hipEventRecord(R->ctx->gtail, us);
            if (e != hipSuccess) return map_hip(e);
            R->ctx->gpending = true;
            return RT_SUCCESS;
        }
        for (int j = 0; !l.ipc_linked && j < n_local; ++j)
            if (comms[j] != R) l.join_events.push_back(sent(comms[j]));
        R->ctx->gjoin = R;
        R->ctx->gpending = false;
    }
    return RT_SUCCESS;
}

// RCCL transport.  Phase 1: every rank (the root too) packs its bands on its context's accumulation
// stream
int rccl_pack(const rt_comm* comms, int n_local, int root, const rt_mem* outs) {
    for (int i = 0; i < n_local; ++i) {
        rt_comm c = comms[i];
        rt_context ctx = c->ctx;
        rti::CommStaging& sg = c->stage;
        const hipStream_t cstream = c->st.cstream;
        hipError_t e = hipSetDevice(ctx->device);
        if (e != hipSuccess) return map_hip(e);
        if (int rc = rccl_staging(c)) return rc;
        const int s = sg.slot;
        ++c->plan.seq;
        uint8_t* out = static_cast<uint8_t*>(outs[i]->dptr);
        // the bands are final after every accumulation enqueued so far (astream, in order) and
        // after whatever the main stream has queued (per-frame launches write `out` there)
        e = rti::main_tail_wait(ctx, ctx->astream);
        if (e == hipSuccess && sg.sent_valid[s]) e = hipStreamWaitEvent(ctx->astream, sg.sent[s], 0);  // slot free
        if (e == hipSuccess)
            e = copy_rects(c->plan.rects[c->world.rank], out, static_cast<uint8_t*>(sg.stage[s]), true, ctx->astream);
        if (e == hipSuccess) e = hipEventRecord(sg.packed[s], ctx->astream);
        if (e == hipSuccess) e = hipStreamWaitEvent(cstream, sg.packed[s], 0);
        if (e == hipSuccess && c->world.rank == root && sg.unpacked_valid[s])
            e = hipStreamWaitEvent(cstream, sg.unpacked[s], 0);  // receive slot's last unpack done
        if (e == hipSuccess) e = hipEventRecord(ctx->atail, ctx->astream);
        if (e == hipSuccess) e = hipEventRecord(c->st.xt0, cstream);
        if (e != hipSuccess) return map_hip(e);
        ctx->apending = true;
    }
    return RT_SUCCESS;
}

// phase 2: the transfers, one group over every local rank (required when one thread drives
// several GPUs).  The root posts one receive per rank, so all its links carry data at once;
// its own bands take the same path (a send to itself, a device-local copy) -- one uniform
// unpack, and a world of one still runs the whole RCCL flow.
int rccl_transfer(const rt_comm* comms, int n_local, int root) {
    int rc = map_nccl(ncclGroupStart());
    if (rc) return rc;
    for (int i = 0; i < n_local && rc == RT_SUCCESS; ++i) {
        rt_comm c = comms[i];
        const rti::CommStaging& sg = c->stage;
        const int s = sg.slot;
        rc = map_nccl(ncclSend(sg.stage[s], sg.bytes, ncclInt8, root, c->world.nc, c->st.cstream));
        if (c->world.rank == root)
            for (int q = 0; q < c->world.nranks && rc == RT_SUCCESS; ++q)
                rc = map_nccl(ncclRecv(static_cast<uint8_t*>(sg.parts[s]) + (size_t)q * sg.bytes, sg.bytes, ncclInt8, q,
                                       c->world.nc, c->st.cstream));
    }
    const int rc_end = map_nccl(ncclGroupEnd());
    if (rc) return rc;
    return rc_end;
}

// phase 3: the root unpacks every rank's bands into the destination
int rccl_unpack(const rt_comm* comms, int n_local, int root, rt_mem root_dst, const rt_mem* outs) {
    for (int i = 0; i < n_local; ++i) {
        rt_comm c = comms[i];
        rt_context ctx = c->ctx;
        rti::CommStaging& sg = c->stage;
        const hipStream_t cstream = c->st.cstream, ustream = c->st.ustream;
        const bool is_root = c->world.rank == root;
        const int s = sg.slot;
        hipError_t e = hipSetDevice(ctx->device);
        if (e == hipSuccess) e = hipEventRecord(c->st.xt1, cstream);
        if (e == hipSuccess) e = hipEventRecord(sg.sent[s], cstream);
        if (e != hipSuccess) return map_hip(e);
        c->st.xt_valid = true;
        sg.sent_valid[s] = true;
        if (is_root) {
            // Gathering into the root's own output: its own bands are in place already and are
            // not unpacked, so the unpack writes only other ranks' rows, which no later render,
            // accumulation or pack of this context touches -- nothing on the context waits for
            // it.  (An unpack that the next accumulation had to wait for chained that
            // accumulation, and the render after it, to the transfer: RCCL's kernel gets CUs only
            // as a persistent render drains, so every second render started a step late --
            // world-1 0.90 vs 0.77 ms/frame, profiles/r04/dist_flow_ab.txt.)  Reads of the
            // image wait for it through the context's queue (gtail, qs()); the unpack waits for
            // the reads queued before this gather.
            const bool into_out = !root_dst || root_dst == outs[i];
            uint8_t* dst = static_cast<uint8_t*>((root_dst ? root_dst : outs[i])->dptr);
            e = rti::main_tail_wait(ctx, ustream);
            if (e == hipSuccess) e = hipStreamWaitEvent(ustream, sg.sent[s], 0);
            for (int q = 0; q < c->world.nranks && e == hipSuccess; ++q)
                if (!(into_out && q == c->world.rank))
                    e = copy_rects(c->plan.rects[q], dst, static_cast<uint8_t*>(sg.parts[s]) + (size_t)q * sg.bytes, false,
                                   ustream);
            if (e == hipSuccess) e = hipEventRecord(sg.unpacked[s], ustream);
            if (e != hipSuccess) return map_hip(e);
            sg.unpacked_valid[s] = true;
        }
        e = hipEventRecord(ctx->gtail, is_root ? ustream : cstream);
        if (e != hipSuccess) return map_hip(e);
        ctx->gpending = true;
        sg.slot ^= 1;
    }
    return RT_SUCCESS;
}

// One communicator on `ctx`, its parts created on the context's device; it owns `nc` from here on.
// On failure everything made so far is released.
int make_comm(rt_context ctx, rtp::World kind, int rank, int nranks, ncclComm_t nc, const void* group, rt_comm* out) {
    *out = nullptr;
    rt_comm c = new (std::nothrow) rt_comm_s();
    if (!c) {
        if (nc) (void)ncclCommDestroy(nc);
        return RT_OUT_OF_HOST_MEMORY;
    }
    c->ctx = ctx;
    c->world.kind = kind;
    c->world.rank = rank;
    c->world.nranks = nranks;
    c->world.nc = nc;
    c->world.group = group;
    int rc = map_hip(hipSetDevice(ctx->device));
    if (!rc) rc = c->st.create();
    if (!rc) rc = c->stage.create();
    if (!rc) rc = c->world.create();
    if (rc) {
        release(c);
        return rc;
    }
    *out = c;
    return RT_SUCCESS;
}

// A world of n communicators in this process (ncs: their RCCL communicators, or null), who know
// each other (CommWorld::members).  On failure none is left.
int make_world(const rt_context* ctxs, int n, rtp::World kind, ncclComm_t* ncs, const void* group, rt_comm* comms) {
    for (int i = 0; i < n; ++i) {
        const int rc = make_comm(ctxs[i], kind, i, n, ncs ? ncs[i] : nullptr, group, &comms[i]);
        if (!rc) continue;
        for (int j = 0; j < i; ++j) {
            release(comms[j]);
            comms[j] = nullptr;
        }
        for (int j = i + 1; ncs && j < n; ++j) (void)ncclCommDestroy(ncs[j]);
        return rc;
    }
    try {
        auto m = std::make_shared<std::vector<rt_comm>>(comms, comms + n);
        for (int i = 0; i < n; ++i) comms[i]->world.members = m;
    } catch (const std::bad_alloc&) {  // (no exception crosses the C ABI; a join then waits at once)
        for (int i = 0; i < n; ++i) comms[i]->world.members.reset();
    }
    return RT_SUCCESS;
}

// a loopback world's calls must name all its members, each once
int check_loopback(const rt_comm* comms, int n_local) {
    return rtp::check_members(n_local, [&](int i) {
        const rti::CommWorld& w = comms[i]->world;
        return rtp::Member{w.group, w.rank, w.nranks};
    });
}

}  // namespace

// The root's first read of a gathered image: `s` waits for every rank's arrival (flags between
// processes, events within one; and the root's own copies), and the context's gather tail
// becomes that point of `s`.  Where other devices' copy engines wrote the image (remote_writers),
// the root's caches may still hold lines of the previous image that the root read before (its
// blits, kernels): a system-scope acquire on every XCD follows the waits, before any read.
// (Multi-GPU byte parity of the direct-write gather has not been verified on hardware: every run
// so far wrote from one device; RT_COMM_OPT_SYSTEM_ACQUIRE runs the acquire there, tests/test_comm.py.)
hipError_t rti::join_gather(rt_comm c, hipStream_t s) {
    const rti::CommLinks& l = c->links;
    hipError_t e = hipSetDevice(c->ctx->device);
    for (int q = 0; l.ipc_linked && q < c->world.nranks && e == hipSuccess; ++q)
        if (q != c->plan.id.root) e = hipStreamWaitValue64(s, l.rflags + q, l.join_seq, hipStreamWaitValueGte, ~0ull);
    for (size_t j = 0; j < l.join_events.size() && e == hipSuccess; ++j) e = hipStreamWaitEvent(s, l.join_events[j], 0);
    if (e == hipSuccess && c->plan.sends) e = hipStreamWaitEvent(s, c->st.dsent, 0);
    if (e == hipSuccess) e = system_acquire(c, s);
    if (e == hipSuccess) e = hipEventRecord(c->ctx->gtail, s);
    return e;
}

extern "C" {

int rtCommGetUniqueId(void* id) {
    if (!id) return RT_INVALID_VALUE;
    static_assert(sizeof(ncclUniqueId) == RT_COMM_ID_BYTES, "unique id size");
    ncclUniqueId u;
    int rc = map_nccl(ncclGetUniqueId(&u));
    if (rc) return rc;
    std::memcpy(id, &u, sizeof(u));
    return RT_SUCCESS;
}

int rtCommInitRank(rt_context ctx, int nranks, const void* id, int rank, rt_comm* out) {
    if (!out) return RT_INVALID_VALUE;
    *out = nullptr;
    if (!ctx) return RT_INVALID_CONTEXT;
    if (!id || nranks < 1 || rank < 0 || rank >= nranks) return RT_INVALID_VALUE;
    hipError_t he = hipSetDevice(ctx->device);
    if (he != hipSuccess) return map_hip(he);
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof(u));
    ncclComm_t nc = nullptr;
    int rc = map_nccl(ncclCommInitRank(&nc, nranks, u, rank));
    if (rc) return rc;
    return make_comm(ctx, rtp::World::RcclRank, rank, nranks, nc, nullptr, out);
}

int rtCommInitAll(const rt_context* ctxs, int n, rt_comm* comms_out) {
    if (!ctxs || !comms_out || n < 1) return RT_INVALID_VALUE;
    std::vector<int> devs(n);
    for (int i = 0; i < n; ++i) {
        comms_out[i] = nullptr;
        if (!ctxs[i]) return RT_INVALID_CONTEXT;
        devs[i] = ctxs[i]->device;
    }
    std::vector<ncclComm_t> nc(n, nullptr);
    int rc = map_nccl(ncclCommInitAll(nc.data(), n, devs.data()));
    if (rc) return rc;
    return make_world(ctxs, n, rtp::World::RcclAll, nc.data(), nullptr, comms_out);
}

int rtCommInitLoopback(const rt_context* ctxs, int n, rt_comm* comms_out) {
    // (rtp::check_members tracks the members of a call in a 64-bit mask)
    if (!ctxs || !comms_out || n < 1 || n > 64) return RT_INVALID_VALUE;
    for (int i = 0; i < n; ++i) {
        comms_out[i] = nullptr;
        if (!ctxs[i]) return RT_INVALID_CONTEXT;
    }
    static std::atomic<uintptr_t> next_group{1};
    const void* group = reinterpret_cast<const void*>(next_group.fetch_add(1));
    return make_world(ctxs, n, rtp::World::Loopback, nullptr, group, comms_out);
}

int rtCommInitShared(rt_context ctx, int nranks, int rank, const char* dir, rt_comm* out) {
    if (!out) return RT_INVALID_VALUE;
    *out = nullptr;
    if (!ctx) return RT_INVALID_CONTEXT;
    if (!dir || !*dir || nranks < 1 || rank < 0 || rank >= nranks) return RT_INVALID_VALUE;
    hipError_t he = hipSetDevice(ctx->device);
    if (he != hipSuccess) return map_hip(he);
    rtp::FileWorld files;
    int rc = files.join(dir, rank, nranks);
    if (rc) return rc;
    // (a world that has joined and exchanged nothing has no file of its own to remove)
    rc = make_comm(ctx, rtp::World::Shared, rank, nranks, nullptr, nullptr, out);
    if (!rc) (*out)->world.files = std::move(files);
    return rc;
}

int rtCommDestroy(rt_comm c) {
    if (!c) return RT_INVALID_VALUE;
    (void)hipSetDevice(c->ctx->device);
    (void)hipStreamSynchronize(qs(c->ctx));
    release(c);
    return RT_SUCCESS;
}

int rtCommGetRank(rt_comm c, int* rank, int* nranks) {
    if (!c) return RT_INVALID_VALUE;
    if (rank) *rank = c->world.rank;
    if (nranks) *nranks = c->world.nranks;
    return RT_SUCCESS;
}

int rtCommSetTransport(rt_comm c, int transport) {
    if (!c) return RT_INVALID_VALUE;
    if (transport != RT_COMM_TRANSPORT_COPY_ENGINES && transport != RT_COMM_TRANSPORT_RCCL &&
        transport != RT_COMM_TRANSPORT_COPY_ENGINES_IPC)
        return RT_INVALID_VALUE;
    if (c->world.loopback() && transport != RT_COMM_TRANSPORT_COPY_ENGINES) return RT_INVALID_OPERATION;
    if (!c->world.has_rccl() && transport == RT_COMM_TRANSPORT_RCCL) return RT_INVALID_OPERATION;  // shared worlds
    (void)hipSetDevice(c->ctx->device);
    quiesce(c);
    c->opt.transport = transport;
    free_plan(c);  // the next gather builds the plan for it (also: a new destination)
    return RT_SUCCESS;
}

int rtCommGetTransport(rt_comm c, int* transport, int* active) {
    if (!c) return RT_INVALID_VALUE;
    if (transport) *transport = c->opt.transport;
    if (active) *active = rtp::active_transport(c->plan.planned(), c->links.ce, c->links.ipc_linked);
    return RT_SUCCESS;
}

int rtCommGetStatus(rt_comm c, rt_comm_status* out) {
    if (!c || !out) return RT_INVALID_VALUE;
    std::memset(out, 0, sizeof(*out));
    out->rank = c->world.rank;
    out->nranks = c->world.nranks;
    (void)rtCommGetTransport(c, &out->transport, &out->active);
    out->fallback = c->plan.fallback_reason != RT_COMM_FALLBACK_NONE;
    out->fallback_reason = c->plan.fallback_reason;
    out->gathers = c->plan.seq;
    const rtp::GatherCounts g =
        rtp::gather_counts(c->plan.planned(), c->links.ce, c->plan.sends, c->world.rank == c->plan.id.root,
                           c->links.ipc_linked, c->plan.runs, c->stage.bytes);
    out->bytes_per_gather = g.bytes;
    out->copies_per_gather = g.copies;
    out->last_xfer_ms = -1.0;
    float ms = 0.0f;
    if (c->st.xt_valid && hipEventQuery(c->st.xt1) == hipSuccess &&
        hipEventElapsedTime(&ms, c->st.xt0, c->st.xt1) == hipSuccess)
        out->last_xfer_ms = ms;
    return RT_SUCCESS;
}

int rtCommSetOption(rt_comm c, int option, int value) {
    if (!c) return RT_INVALID_VALUE;
    if (option == RT_COMM_OPT_FAIL_LINKS) {
        c->opt.fail_links = value != 0;
        return RT_SUCCESS;
    }
    if (option == RT_COMM_OPT_REPLAN_PERIOD) {
        if (value < 1 || (uint64_t)value > rti::kFlagValues - 2) return RT_INVALID_VALUE;
        c->opt.replan_after = (uint64_t)value;
        return RT_SUCCESS;
    }
    if (option == RT_COMM_OPT_SYSTEM_ACQUIRE) {
        c->opt.force_acquire = value != 0;
        return RT_SUCCESS;
    }
    return RT_INVALID_VALUE;
}

int rtCommShardKernel(rt_comm c, rt_kernel k) {
    if (!c) return RT_INVALID_VALUE;
    return rti::shard_kernel(k, (unsigned)c->world.nranks, (unsigned)c->world.rank);
}

int rtCommEnqueueGatherBands(const rt_comm* comms, const rt_mem* outs, int n_local, unsigned W, unsigned H,
                             int root, rt_mem root_dst) {
    if (!comms || !outs || n_local < 1 || W == 0 || H == 0) return RT_INVALID_VALUE;
    const uint64_t img_bytes = (uint64_t)W * H * rtp::kPixelBytes;
    for (int i = 0; i < n_local; ++i) {
        rt_comm c = comms[i];
        if (!c || !outs[i] || outs[i]->released) return RT_INVALID_VALUE;
        if (root < 0 || root >= c->world.nranks) return RT_INVALID_VALUE;
        if (outs[i]->ctx != c->ctx || outs[i]->size < img_bytes) return RT_INVALID_MEM_OBJECT;
        if (c->world.rank == root && root_dst &&
            (root_dst->released || root_dst->ctx != c->ctx || root_dst->size < img_bytes))
            return RT_INVALID_MEM_OBJECT;
    }
    if (int rc = check_loopback(comms, n_local)) return rc;
    for (int i = 0; i < n_local; ++i)  // coalesced per-frame launches first: the gather reads their output
        (void)rti::flush_frames(comms[i]->ctx);
    // the plans (rebuilt, by every rank alike, when the size, the root or the transport changes).
    // A plan is committed only built and linked: a call that fails on the way leaves no plan, and
    // the next gather plans and links afresh
    bool ce = false;
    if (int rc = plan_gather(comms, outs, n_local, W, H, root, root_dst, &ce)) {
        for (int i = 0; i < n_local; ++i)
            if (comms[i]->plan.building) {
                (void)hipSetDevice(comms[i]->ctx->device);
                free_plan(comms[i]);
            }
        return rc;
    }
    if (ce) return ce_gather(comms, n_local, root, outs);
    int rc = rccl_pack(comms, n_local, root, outs);
    if (!rc) rc = rccl_transfer(comms, n_local, root);
    if (!rc) rc = rccl_unpack(comms, n_local, root, root_dst, outs);
    return rc;
}

int rtCommAllReduceF64(const rt_comm* comms, int n_local, double* values, int count, int op) {
    if (!comms || n_local < 1 || !values || count < 1 || count > 64) return RT_INVALID_VALUE;
    if (op != RT_COMM_SUM && op != RT_COMM_MAX) return RT_INVALID_VALUE;
    for (int i = 0; i < n_local; ++i)
        if (!comms[i]) return RT_INVALID_VALUE;
    if (int rc = check_loopback(comms, n_local)) return rc;
    if (comms[0]->world.shared()) {
        // shared world: one rank per call, the reduction through the exchange files, after this
        // rank's earlier gathers have drained (as RCCL's stream order would have it)
        if (n_local != 1) return RT_INVALID_VALUE;
        rt_comm c = comms[0];
        hipError_t e = hipSetDevice(c->ctx->device);
        if (e == hipSuccess) e = hipStreamSynchronize(c->st.cstream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->st.ustream);
        if (e != hipSuccess) return map_hip(e);
        std::vector<double> all((size_t)c->world.nranks * count);
        int rc = c->world.files.allgather(values, sizeof(double) * count, all.data());
        if (rc) return rc;
        rtp::fold_rows(all.data(), c->world.nranks, count, op, values);
        return RT_SUCCESS;
    }
    if (comms[0]->world.loopback()) {
        // loopback world: every member is here, so the reduction is over these rows, after the
        // members' communicator streams (earlier gathers) have drained, as RCCL's would
        for (int i = 0; i < n_local; ++i) {
            hipError_t e = hipSetDevice(comms[i]->ctx->device);
            if (e == hipSuccess) e = hipStreamSynchronize(comms[i]->st.cstream);
            if (e != hipSuccess) return map_hip(e);
        }
        rtp::fold_rows(values, n_local, count, op, values);
        for (int i = 1; i < n_local; ++i) std::memcpy(values + (size_t)i * count, values, count * sizeof(double));
        return RT_SUCCESS;
    }
    for (int i = 0; i < n_local; ++i) {
        hipError_t e = hipSetDevice(comms[i]->ctx->device);
        if (e == hipSuccess)
            e = hipMemcpyAsync(comms[i]->world.scratch, values + (size_t)i * count, count * sizeof(double),
                               hipMemcpyHostToDevice, comms[i]->st.cstream);
        if (e != hipSuccess) return map_hip(e);
    }
    int rc = map_nccl(ncclGroupStart());
    if (rc) return rc;
    for (int i = 0; i < n_local && rc == RT_SUCCESS; ++i)
        rc = map_nccl(ncclAllReduce(comms[i]->world.scratch, comms[i]->world.scratch, count, ncclFloat64,
                                    op == RT_COMM_SUM ? ncclSum : ncclMax, comms[i]->world.nc, comms[i]->st.cstream));
    const int rc_end = map_nccl(ncclGroupEnd());
    if (rc) return rc;
    if (rc_end) return rc_end;
    for (int i = 0; i < n_local; ++i) {
        hipError_t e = hipSetDevice(comms[i]->ctx->device);
        if (e == hipSuccess)
            e = hipMemcpyAsync(values + (size_t)i * count, comms[i]->world.scratch, count * sizeof(double),
                               hipMemcpyDeviceToHost, comms[i]->st.cstream);
        if (e == hipSuccess) e = hipStreamSynchronize(comms[i]->st.cstream);
        if (e != hipSuccess) return map_hip(e);
    }
    return RT_SUCCESS;
}

int rtCommBarrier(const rt_comm* comms, int n_local) {
    if (!comms || n_local < 1) return RT_INVALID_VALUE;
    std::vector<double> v((size_t)n_local, 0.0);
    return rtCommAllReduceF64(comms, n_local, v.data(), 1, RT_COMM_SUM);
}

int rtBandPackPlan(unsigned width, unsigned height, unsigned period, unsigned phase, rt_rect* rects,
                   int capacity, int* n_rects, size_t* staging_bytes) {
    return rtp::band_plan(width, height, period, phase, rects, capacity, n_rects, staging_bytes);
}

}  // extern "C"

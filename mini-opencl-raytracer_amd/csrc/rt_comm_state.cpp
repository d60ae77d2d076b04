// rt_comm_state.cpp -- the parts of a communicator (rt_comm_state.hpp): how each creates, resets and
// releases what it owns.
#include "rt_comm_state.hpp"

#include <algorithm>
#include <new>

namespace rti {

int map_nccl(ncclResult_t r) {
    switch (r) {
        case ncclSuccess: return RT_SUCCESS;
        case ncclInvalidArgument:
        case ncclInvalidUsage: return RT_INVALID_VALUE;
        case ncclSystemError: return RT_OUT_OF_RESOURCES;
        default: return RT_INVALID_OPERATION;
    }
}

// ---- the world ----

int CommWorld::create() { return map_hip(hipMalloc(reinterpret_cast<void**>(&scratch), 64 * sizeof(double))); }

// RCCL: [mine | everyone's] in one device block, gathered on `s`
int CommWorld::allgather(const void* mine, size_t n, void* all, hipStream_t s) {
    if (shared()) return files.allgather(mine, n, all);
    void* dev = nullptr;
    hipError_t e = hipMalloc(&dev, n * (nranks + 1));
    if (e != hipSuccess) return map_hip(e);
    uint8_t* d = static_cast<uint8_t*>(dev);
    int rc = map_hip(hipMemcpy(d, mine, n, hipMemcpyHostToDevice));
    if (!rc) rc = map_nccl(ncclAllGather(d, d + n, n, ncclUint8, nc, s));
    if (!rc) rc = map_hip(hipStreamSynchronize(s));
    if (!rc) rc = map_hip(hipMemcpy(all, d + n, n * nranks, hipMemcpyDeviceToHost));
    (void)hipFree(dev);
    return rc;
}

int CommWorld::max(int v, int* out, hipStream_t s) {
    if (shared()) return files.max(v, out);
    int* d = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&d), 2 * sizeof(int));
    if (e != hipSuccess) return map_hip(e);
    int rc = map_hip(hipMemcpy(d, &v, sizeof(int), hipMemcpyHostToDevice));
    if (!rc) rc = map_nccl(ncclAllReduce(d, d + 1, 1, ncclInt32, ncclMax, nc, s));
    if (!rc) rc = map_hip(hipStreamSynchronize(s));
    if (!rc) rc = map_hip(hipMemcpy(out, d + 1, sizeof(int), hipMemcpyDeviceToHost));
    (void)hipFree(d);
    return rc;
}

void CommWorld::release() {
    if (scratch) (void)hipFree(scratch);
    if (nc) (void)ncclCommDestroy(nc);
    scratch = nullptr;
    nc = nullptr;
    if (shared()) files.remove_own();
}

// ---- streams and events ----

int CommStreams::create() {
    int least = 0, greatest = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&cstream, hipStreamNonBlocking, greatest);
    if (e == hipSuccess) e = hipStreamCreateWithPriority(&ustream, hipStreamNonBlocking, greatest);
    for (int i = 0; RT_COMM_XFER_STREAMS > 1 && i < RT_COMM_XFER_STREAMS && e == hipSuccess; ++i) {
        e = hipStreamCreateWithPriority(&xstream[i], hipStreamNonBlocking, greatest);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&xdone[i], hipEventDisableTiming);
    }
    for (hipEvent_t* ev : {&xgo, &ready, &dsent, &released})
        if (e == hipSuccess) e = hipEventCreateWithFlags(ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreate(&xt0);
    if (e == hipSuccess) e = hipEventCreate(&xt1);
    return map_hip(e);
}

void CommStreams::sync() const {
    for (hipStream_t s : {cstream, ustream})
        if (s) (void)hipStreamSynchronize(s);
    for (hipStream_t s : xstream)
        if (s) (void)hipStreamSynchronize(s);
}

void CommStreams::release() {
    for (hipEvent_t ev : {ready, dsent, released, xt0, xt1, xgo})
        if (ev) (void)hipEventDestroy(ev);
    for (int i = 0; i < 8; ++i) {
        if (xstream[i]) (void)hipStreamDestroy(xstream[i]);
        if (xdone[i]) (void)hipEventDestroy(xdone[i]);
    }
    if (cstream) (void)hipStreamDestroy(cstream);
    if (ustream) (void)hipStreamDestroy(ustream);
    *this = CommStreams{};
}

// ---- staging ----

int CommStaging::create() {
    hipError_t e = hipSuccess;
    for (int s = 0; s < 2 && e == hipSuccess; ++s) {
        e = hipEventCreateWithFlags(&packed[s], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&sent[s], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&unpacked[s], hipEventDisableTiming);
    }
    return map_hip(e);
}

int CommStaging::ensure(int receive_ranks) {
    hipError_t e = hipSuccess;
    for (int s = 0; s < 2 && e == hipSuccess; ++s) {
        if (!stage[s]) e = hipMalloc(&stage[s], std::max<size_t>(bytes, 16));
        if (e == hipSuccess && receive_ranks > 0 && !parts[s])
            e = hipMalloc(&parts[s], std::max<size_t>(bytes * receive_ranks, 16));
    }
    return map_hip(e);
}

void CommStaging::reset() {
    for (int s = 0; s < 2; ++s) {
        if (stage[s]) (void)hipFree(stage[s]);
        if (parts[s]) (void)hipFree(parts[s]);
        stage[s] = parts[s] = nullptr;
        sent_valid[s] = unpacked_valid[s] = false;
    }
    slot = 0;
}

void CommStaging::release() {
    reset();
    for (int s = 0; s < 2; ++s)
        for (hipEvent_t* ev : {&packed[s], &sent[s], &unpacked[s]}) {
            if (*ev) (void)hipEventDestroy(*ev);
            *ev = nullptr;
        }
}

// ---- copy-engine links ----

void CommLinks::aim(rt_mem dst) {
    target = dst;
    pin(dst);
}

void CommLinks::unpin() {
    if (target) rti::unpin(target);
    target = nullptr;
}

int CommLinks::alloc_flags(bool is_root, int nranks) {
    hipError_t e = hipExtMallocWithFlags(reinterpret_cast<void**>(&sflags), sizeof(uint64_t), hipDeviceMallocFinegrained);
    if (e == hipSuccess && is_root)
        e = hipExtMallocWithFlags(reinterpret_cast<void**>(&rflags), sizeof(uint64_t) * nranks, hipDeviceMallocFinegrained);
    if (e == hipSuccess && is_root)
        e = hipExtMallocWithFlags(reinterpret_cast<void**>(&probe), kProbeBytes * nranks, hipDeviceMallocFinegrained);
    if (e == hipSuccess) e = hipMemset(sflags, 0, sizeof(uint64_t));
    if (e == hipSuccess && rflags) e = hipMemset(rflags, 0, sizeof(uint64_t) * nranks);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return map_hip(e);
}

int CommLinks::flag_values() {
    if (vals) return RT_SUCCESS;
    std::vector<uint64_t> v;
    try {
        v.resize(kFlagValues);
    } catch (const std::bad_alloc&) {
        return RT_OUT_OF_HOST_MEMORY;
    }
    for (uint64_t i = 0; i < kFlagValues; ++i) v[i] = i;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&vals), kFlagValues * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMemcpy(vals, v.data(), kFlagValues * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e != hipSuccess && vals) {
        (void)hipFree(vals);
        vals = nullptr;
    }
    return map_hip(e);
}

void CommLinks::unmap() {
    for (void* p : ipc_opened) (void)hipIpcCloseMemHandle(p);
    ipc_opened.clear();
    peer_target = peer_probe = nullptr;
    peer_rflags = nullptr;
    peer_sflags.clear();
}

void CommLinks::reset() {
    unmap();
    for (uint64_t** f : {&sflags, &rflags})
        if (*f) (void)hipFree(*f);
    if (probe) (void)hipFree(probe);
    sflags = rflags = nullptr;
    probe = nullptr;
    unpin();
    ce = ipc_linked = remote_writers = false;
    join_seq = 0;
    join_events.clear();
}

void CommLinks::release() {
    reset();
    if (vals) (void)hipFree(vals);
    vals = nullptr;
}

// ---- the plan ----

void CommPlan::reset() {
    runs.clear();
    sends = false;
    fallback_reason = RT_COMM_FALLBACK_NONE;
    seq = 0;
    id = rtp::PlanId{};
    building = false;
}

}  // namespace rti

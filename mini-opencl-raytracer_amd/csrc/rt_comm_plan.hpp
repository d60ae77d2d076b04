// rt_comm_plan.hpp -- the rules of the multi-GPU gather (rtComm*, rt_comm.cpp) as functions of plain
// values: the band plan and its runs, how the runs are dealt over the transfer streams, the kinds of
// world, when a plan is still current, how a fresh plan is linked, who must be in a loopback call,
// what rtCommGetStatus counts, and the row fold of the host reductions.  Pure host code: no HIP or
// collective-library header, no allocation but the returned vectors (tests/test_comm_plan.py builds
// it with g++).
#pragma once

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "../../include/rt_hip.h"

namespace rtp {

constexpr unsigned kBandRows = 8;   // = the 8x8 tile height of the persistent schedules
constexpr size_t kPixelBytes = 16;  // one float3 slot of the output buffer

// mirror of clrt/multigpu.py pack_plan (tests compare the two); rtBandPackPlan
int band_plan(unsigned W, unsigned H, unsigned period, unsigned phase, rt_rect* rects, int cap, int* n,
              size_t* staging);

// a byte run of the image: (image byte offset, bytes)
using Run = std::pair<uint64_t, uint64_t>;

// The byte runs of the image one rank's bands occupy (adjacent bands merged: one run for a world of
// one), in image order.
std::vector<Run> band_runs(const std::vector<rt_rect>& plan);

// One copy of a gather: `bytes` of runs[run] from `at` bytes into it, on transfer stream `stream`;
// `dense` is the piece's offset in the rank's staging slot (the runs packed back to back).
struct Piece {
    unsigned stream;
    size_t run;
    uint64_t at, bytes, dense;
};

// The streams a copy of `total` bytes is dealt over: one per MiB up to `streams`; 1 = the caller's
// own stream (split off, or less than 2 MiB).
unsigned deal_streams(uint64_t total, unsigned streams, bool split);

// The runs dealt over deal_streams() streams in image order: every stream takes an equal share
// (rounded up to 256 B) of the bytes, a run is cut where a share ends.  One stream: one piece per run.
std::vector<Piece> deal_runs(const std::vector<Run>& runs, unsigned streams, bool split);

// The kind of world a communicator belongs to, set once by its init call.
enum class World {
    RcclRank,  // rtCommInitRank: one process per GPU
    RcclAll,   // rtCommInitAll: one process driving every GPU
    Loopback,  // rtCommInitLoopback: n contexts of one process, no collective library
    Shared,    // rtCommInitShared: one process per rank, setup through files
};
constexpr bool has_collectives(World w) { return w == World::RcclRank || w == World::RcclAll; }

// What a plan is compared by.
struct PlanId {
    unsigned W = 0, H = 0;  // W == 0: no plan
    int root = -1;
};

// The plan still serves a W x H gather to `root`: same size and root, gathers left before the flag
// values run out (seq < replan_after), and -- a copy-engine plan writes into the destination it was
// linked to -- on the root of a copy-engine plan the same destination.
bool plan_current(const PlanId& plan, unsigned W, unsigned H, int root, bool is_root, bool ce, bool same_dst,
                  uint64_t seq, uint64_t replan_after);

// How a fresh plan gets its copy-engine links.
enum class Link {
    Direct,  // every member is in the call: by address
    Ipc,     // one rank per call: IPC handles exchanged through the world
    None,    // RCCL transfers: asked for, or several local ranks of a larger RCCL world
    Refuse,  // RT_INVALID_OPERATION: the IPC transport with several local ranks, or in a loopback world
};
Link link_choice(int transport, World kind, int n_local, int nranks);

// One communicator of a call, as the membership check sees it (group: the loopback world's id, null
// for every other kind).
struct Member {
    const void* group;
    int rank, nranks;
};

// A loopback world's calls must name all its members, each once (ranks < 64: the call's members are
// tracked in a 64-bit mask); no other call may name a loopback member.  `member(i)` is the i-th Member.
template <class Get>
int check_members(int n_local, Get member) {
    const Member first = member(0);
    if (!first.group) {
        for (int i = 1; i < n_local; ++i)
            if (member(i).group) return RT_INVALID_VALUE;
        return RT_SUCCESS;
    }
    if (n_local != first.nranks) return RT_INVALID_VALUE;
    uint64_t seen = 0;
    for (int i = 0; i < n_local; ++i) {
        const Member m = member(i);
        if (m.group != first.group || m.rank >= 64) return RT_INVALID_VALUE;
        const uint64_t bit = 1ull << m.rank;
        if (seen & bit) return RT_INVALID_VALUE;
        seen |= bit;
    }
    return RT_SUCCESS;
}

// rtCommGetTransport's `active`: the transport the current plan uses (-1: no plan)
int active_transport(bool planned, bool ce, bool ipc_linked);

// rtCommGetStatus: the bytes this rank moves and the copy commands it issues per gather.  Copy engines,
// the root: its own bands straight into the destination (none when they are in place); the others:
// pack + transfer per run, + the arrival flag between processes.  RCCL: the staging slot, one transfer.
struct GatherCounts {
    uint64_t bytes = 0;
    unsigned copies = 0;
};
GatherCounts gather_counts(bool planned, bool ce, bool sends, bool is_root, bool ipc_linked,
                           const std::vector<Run>& runs, size_t stage_bytes);

// out[j] = rows[0][j] (+ or max) rows[1][j] (+ or max) ... in that order (op: RT_COMM_SUM / RT_COMM_MAX);
// `out` may be a row of `rows`.
void fold_rows(const double* rows, int n_rows, int count, int op, double* out);

}  // namespace rtp

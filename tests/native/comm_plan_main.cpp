// comm_plan_main.cpp -- stand-alone driver of the gather's rules over plain values
// (csrc/rt_comm_plan.{hpp,cpp}), CPU only; built by tests/test_comm_plan.py with plain g++ and once more
// with -fsanitize=address,undefined.  Prints one line per case; the expected answers are in the test,
// not here.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../mini-opencl-raytracer_amd/csrc/rt_comm_plan.hpp"

namespace {

void print_deal(const std::vector<rtp::Run>& runs, unsigned streams, bool split) {
    std::printf(" runs");
    for (const rtp::Run& r : runs) std::printf(" %llu:%llu", (unsigned long long)r.first, (unsigned long long)r.second);
    std::printf(" pieces");
    for (const rtp::Piece& p : rtp::deal_runs(runs, streams, split))
        std::printf(" %u:%zu:%llu:%llu:%llu", p.stream, p.run, (unsigned long long)p.at, (unsigned long long)p.bytes,
                    (unsigned long long)p.dense);
    std::printf("\n");
}

// the runs of rank `rank` of `n` over a W x H image, through band_plan and band_runs
std::vector<rtp::Run> runs_of(unsigned W, unsigned H, unsigned n, unsigned rank) {
    rt_rect r[2];
    int k = 0;
    size_t sb = 0;
    if (rtp::band_plan(W, H, n, rank, r, 2, &k, &sb) != RT_SUCCESS) std::abort();
    return rtp::band_runs(std::vector<rt_rect>(r, r + k));
}

const int kTransports[3] = {RT_COMM_TRANSPORT_COPY_ENGINES, RT_COMM_TRANSPORT_RCCL, RT_COMM_TRANSPORT_COPY_ENGINES_IPC};
const rtp::World kKinds[4] = {rtp::World::RcclRank, rtp::World::RcclAll, rtp::World::Loopback, rtp::World::Shared};

int members(const char* name, const std::vector<rtp::Member>& m) {
    const int rc = rtp::check_members((int)m.size(), [&](int i) { return m[i]; });
    std::printf("members %s %d\n", name, rc);
    return rc;
}

void counts(const char* name, bool planned, bool ce, bool sends, bool is_root, bool ipc) {
    const std::vector<rtp::Run> runs = {{0, 100}, {4096, 50}};
    const rtp::GatherCounts g = rtp::gather_counts(planned, ce, sends, is_root, ipc, runs, 4096);
    std::printf("status %s %d %llu %u\n", name, rtp::active_transport(planned, ce, ipc), (unsigned long long)g.bytes, g.copies);
}

}  // namespace

int main() {
    // deal_runs over image sizes, world sizes, every rank, 1..8 streams, split on and off
    const unsigned sizes[][3] = {{3840, 2160, 1}, {3840, 2160, 2}, {3840, 2160, 8}, {1277, 731, 3}, {640, 37, 8}, {5, 7, 4}};
    for (const auto& z : sizes)
        for (unsigned rank = 0; rank < z[2]; ++rank)
            for (unsigned streams = 1; streams <= 8; ++streams)
                for (int split = 0; split < 2; ++split) {
                    std::printf("deal %u %u %u %u %u %d", z[0], z[1], z[2], rank, streams, split);
                    print_deal(runs_of(z[0], z[1], z[2], rank), streams, split != 0);
                }
    // hand-made runs: 1 MiB, 2 MiB, 1 MiB over 2 streams -- the split falls inside the middle run
    std::printf("hand three_runs");
    print_deal({{0, 1u << 20}, {4u << 20, 2u << 20}, {16u << 20, 1u << 20}}, 2, true);

    // plan_current: plan (64, 40, root 1); argument order W H root is_root ce same_dst seq replan_after
    const rtp::PlanId id{64, 40, 1};
    auto cur = [&](const char* name, unsigned W, unsigned H, int root, bool is_root, bool ce, bool same, uint64_t seq) {
        std::printf("current %s %d\n", name, rtp::plan_current(id, W, H, root, is_root, ce, same, seq, 10) ? 1 : 0);
    };
    cur("same", 64, 40, 1, true, true, true, 5);
    cur("width", 65, 40, 1, true, true, true, 5);
    cur("height", 64, 41, 1, true, true, true, 5);
    cur("root", 64, 40, 0, true, true, true, 5);
    cur("not_root", 64, 40, 1, false, true, true, 5);
    cur("not_ce", 64, 40, 1, true, false, true, 5);
    cur("other_dst", 64, 40, 1, true, true, false, 5);
    cur("other_dst_not_root", 64, 40, 1, false, true, false, 5);
    cur("other_dst_not_ce", 64, 40, 1, true, false, false, 5);
    cur("seq_before_end", 64, 40, 1, true, true, true, 9);
    cur("seq_at_end", 64, 40, 1, true, true, true, 10);
    std::printf("current no_plan %d\n", rtp::plan_current(rtp::PlanId{}, 64, 40, 1, true, false, true, 0, 10) ? 1 : 0);

    // link_choice: transport x kind x n_local in {1, nranks, neither} at nranks 4, and a world of one
    for (int t = 0; t < 3; ++t)
        for (int k = 0; k < 4; ++k) {
            std::printf("link %d %d", kTransports[t], k);
            for (int n_local : {1, 4, 2}) std::printf(" %d", (int)rtp::link_choice(kTransports[t], kKinds[k], n_local, 4));
            std::printf(" %d\n", (int)rtp::link_choice(kTransports[t], kKinds[k], 1, 1));
        }

    // check_members
    char groups[2];
    const void *g = &groups[0], *other = &groups[1];
    members("all", {{g, 2, 3}, {g, 0, 3}, {g, 1, 3}});
    members("one_missing", {{g, 0, 3}, {g, 1, 3}});
    members("one_repeated", {{g, 0, 3}, {g, 1, 3}, {g, 1, 3}});
    members("foreign_group", {{g, 0, 3}, {other, 1, 3}, {g, 2, 3}});
    members("mixed_plain_first", {{nullptr, 0, 2}, {g, 1, 2}});
    members("mixed_loopback_first", {{g, 0, 2}, {nullptr, 1, 2}});
    members("no_loopback", {{nullptr, 0, 4}, {nullptr, 1, 4}});
    std::vector<rtp::Member> big;
    for (int r = 63; r >= 0; --r) big.push_back({g, r, 64});
    members("world_of_64", big);
    big.clear();
    for (int r = 0; r < 65; ++r) big.push_back({g, r, 65});
    members("rank_64", big);

    // rtCommGetStatus: runs of 100 and 50 bytes, a 4096-byte staging slot
    counts("root_in_place", true, true, false, true, false);
    counts("root_elsewhere", true, true, true, true, false);
    counts("sender_direct", true, true, true, false, false);
    counts("sender_ipc", true, true, true, false, true);
    counts("root_ipc_in_place", true, true, false, true, true);
    counts("rccl", true, false, true, false, false);
    counts("no_plan", false, false, false, false, false);

    // fold_rows: 3 rows x 2 values; the sums differ in the last bit by association order
    const double tiny = 1.0 / 9007199254740992.0;  // 2^-53
    double sum[6] = {1.0, tiny, tiny, tiny, tiny, 1.0}, out[2];
    rtp::fold_rows(sum, 3, 2, RT_COMM_SUM, out);
    std::printf("fold sum %a %a\n", out[0], out[1]);
    double mx[6] = {1.0, -1.0, 3.0, -5.0, 2.0, -0.5};
    rtp::fold_rows(mx, 3, 2, RT_COMM_MAX, out);
    std::printf("fold max %a %a\n", out[0], out[1]);
    rtp::fold_rows(sum, 3, 2, RT_COMM_SUM, sum);  // in place, into row 0
    std::printf("fold in_place %a %a %a\n", sum[0], sum[1], sum[2]);
    return 0;
}

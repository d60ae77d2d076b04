// rt_comm_plan.cpp -- the gather's rules over plain values (rt_comm_plan.hpp).  A band copied twice or
// never, a piece past its run, a plan taken for current with another destination or a world linked
// the wrong way starts here, so it is kept where a CPU test can sweep it
// (tests/native/comm_plan_main.cpp).
#include "rt_comm_plan.hpp"

#include <algorithm>

namespace rtp {

int band_plan(unsigned W, unsigned H, unsigned period, unsigned phase, rt_rect* rects, int cap, int* n,
              size_t* staging) {
    if (W == 0 || H == 0 || period == 0 || phase >= period) return RT_INVALID_VALUE;
    const uint64_t nb = (H + kBandRows - 1) / kBandRows;
    const uint64_t band_bytes = (uint64_t)kBandRows * W * kPixelBytes;
    const uint64_t per_rank = (nb + period - 1) / period;
    if (staging) *staging = (size_t)(per_rank * band_bytes);
    // bands phase, phase + period, ... < nb; only band nb - 1 can be short
    uint64_t count = phase < nb ? (nb - 1 - phase) / period + 1 : 0;
    const uint64_t last = count ? phase + (count - 1) * period : 0;
    const bool short_last = count && (last + 1) * kBandRows > H;
    const uint64_t full = short_last ? count - 1 : count;
    int k = 0;
    rt_rect tmp[2];
    if (full) tmp[k++] = rt_rect{phase * band_bytes, period * band_bytes, band_bytes, full, 0};
    if (short_last) {
        const uint64_t rows = H - last * kBandRows;
        tmp[k++] = rt_rect{last * band_bytes, band_bytes, rows * W * kPixelBytes, 1, full * band_bytes};
    }
    if (n) *n = k;
    if (rects) {
        if (cap < k) return RT_INVALID_VALUE;
        for (int i = 0; i < k; ++i) rects[i] = tmp[i];
    }
    return RT_SUCCESS;
}

std::vector<Run> band_runs(const std::vector<rt_rect>& plan) {
    std::vector<Run> runs;
    for (const rt_rect& r : plan)
        for (uint64_t i = 0; i < r.rows; ++i) {
            const uint64_t off = r.img_offset + i * r.img_pitch;
            if (!runs.empty() && runs.back().first + runs.back().second == off)
                runs.back().second += r.width;
            else
                runs.emplace_back(off, r.width);
        }
    return runs;
}

unsigned deal_streams(uint64_t total, unsigned streams, bool split) {
    return split ? (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(streams, total >> 20)) : 1u;
}

std::vector<Piece> deal_runs(const std::vector<Run>& runs, unsigned streams, bool split) {
    uint64_t total = 0;
    for (const Run& r : runs) total += r.second;
    const uint64_t k = deal_streams(total, streams, split);
    std::vector<Piece> pieces;
    if (k == 1) {
        uint64_t dense = 0;
        for (size_t i = 0; i < runs.size(); ++i) {
            pieces.push_back(Piece{0, i, 0, runs[i].second, dense});
            dense += runs[i].second;
        }
        return pieces;
    }
    const uint64_t share = ((total + k - 1) / k + 255) & ~(uint64_t)255;
    size_t run = 0;
    uint64_t run_done = 0, dense = 0;  // bytes of runs[run] already dealt out; its dense offset
    for (unsigned i = 0; i < k && run < runs.size(); ++i) {
        uint64_t left = share;
        while (left > 0 && run < runs.size()) {
            const uint64_t n = std::min(left, runs[run].second - run_done);
            pieces.push_back(Piece{i, run, run_done, n, dense + run_done});
            left -= n;
            run_done += n;
            if (run_done == runs[run].second) {
                dense += run_done;
                ++run;
                run_done = 0;
            }
        }
    }
    return pieces;
}

bool plan_current(const PlanId& plan, unsigned W, unsigned H, int root, bool is_root, bool ce, bool same_dst,
                  uint64_t seq, uint64_t replan_after) {
    return plan.W == W && plan.H == H && plan.root == root && (!is_root || !ce || same_dst) && seq < replan_after;
}

Link link_choice(int transport, World kind, int n_local, int nranks) {
    if (transport == RT_COMM_TRANSPORT_RCCL) return Link::None;
    const bool exchanges = kind != World::Loopback;  // a world that can pass IPC handles around
    if (transport == RT_COMM_TRANSPORT_COPY_ENGINES_IPC) return n_local == 1 && exchanges ? Link::Ipc : Link::Refuse;
    if (n_local == nranks) return Link::Direct;
    return n_local == 1 && exchanges ? Link::Ipc : Link::None;
}

int active_transport(bool planned, bool ce, bool ipc_linked) {
    return !planned ? -1 : !ce ? RT_COMM_TRANSPORT_RCCL : ipc_linked ? RT_COMM_TRANSPORT_COPY_ENGINES_IPC
                                                                    : RT_COMM_TRANSPORT_COPY_ENGINES;
}

GatherCounts gather_counts(bool planned, bool ce, bool sends, bool is_root, bool ipc_linked,
                           const std::vector<Run>& runs, size_t stage_bytes) {
    GatherCounts g;
    if (planned && ce) {
        if (sends)
            for (const Run& r : runs) g.bytes += r.second;
        const unsigned n = (unsigned)runs.size();
        g.copies = !sends ? 0u : is_root ? n : 2u * n + (ipc_linked ? 1u : 0u);
    } else if (planned) {
        g.bytes = stage_bytes;
        g.copies = 1;
    }
    return g;
}

void fold_rows(const double* rows, int n_rows, int count, int op, double* out) {
    for (int j = 0; j < count; ++j) {
        double acc = rows[j];
        for (int q = 1; q < n_rows; ++q) {
            const double v = rows[(size_t)q * count + j];
            acc = op == RT_COMM_SUM ? acc + v : std::max(acc, v);
        }
        out[j] = acc;
    }
}

}  // namespace rtp

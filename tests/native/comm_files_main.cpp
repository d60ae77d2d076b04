// comm_files_main.cpp -- stand-alone driver of a shared world's file exchange
// (csrc/rt_comm_files.{hpp,cpp}), CPU only: the ranks run as threads of this program and share nothing
// but the directory.  Built by tests/test_comm_files.py with plain g++ and once more with
// -fsanitize=address,undefined.  Prints what every rank saw; the expected answers are in the test.
// usage: comm_files_main world N DIR | second DIR | absent DIR | truncated DIR
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../mini-opencl-raytracer_amd/csrc/rt_comm_files.hpp"

namespace {

std::mutex g_print;

// byte i of rank q's payload in exchange e (1, 2, 3)
uint8_t pattern(int q, int e, size_t i) { return (uint8_t)(q * 31 + e * 7 + (int)i); }

// one rank of `world`: joins, three all-gathers of 4, 64 and 4096 bytes, a maximum, the cleanup
void rank_main(const char* dir, int rank, int n) {
    rtp::FileWorld w;
    const int joined = w.join(dir, rank, n);
    std::string out = "join " + std::to_string(rank) + " " + std::to_string(joined) + "\n";
    const size_t sizes[3] = {4, 64, 4096};
    for (int e = 1; e <= 3 && joined == 0; ++e) {
        const size_t bytes = sizes[e - 1];
        std::vector<uint8_t> mine(bytes), all(bytes * n);
        for (size_t i = 0; i < bytes; ++i) mine[i] = pattern(rank, e, i);
        const int rc = w.allgather(mine.data(), bytes, all.data());
        // per source rank: first byte, last byte, sum of the bytes
        out += "gather " + std::to_string(rank) + " " + std::to_string(e) + " " + std::to_string(rc);
        for (int q = 0; q < n; ++q) {
            unsigned long sum = 0;
            for (size_t i = 0; i < bytes; ++i) sum += all[q * bytes + i];
            out += " " + std::to_string(all[q * bytes]) + ":" + std::to_string(all[q * bytes + bytes - 1]) + ":" +
                   std::to_string(sum);
        }
        out += "\n";
    }
    if (joined == 0) {
        int mx = 0;
        const int rc = w.max((rank * 37) % 11 - 3, &mx);
        char id[17];
        std::snprintf(id, sizeof(id), "%016llx", (unsigned long long)w.id());
        out += "max " + std::to_string(rank) + " " + std::to_string(rc) + " " + std::to_string(mx) + "\n";
        out += "id " + std::to_string(rank) + " " + id + "\n";
        w.remove_own();
    }
    std::lock_guard<std::mutex> lock(g_print);
    std::fputs(out.c_str(), stdout);
}

long ms_since(std::chrono::steady_clock::time_point t0) {
    return (long)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0).count();
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string what = argv[1];
    if (what == "world" && argc == 4) {
        const int n = std::atoi(argv[2]);
        std::vector<std::thread> ranks;
        for (int r = 0; r < n; ++r) ranks.emplace_back(rank_main, argv[3], r, n);
        for (std::thread& t : ranks) t.join();
        return 0;
    }
    const char* dir = argv[2];
    if (what == "second") {  // a directory that holds a world's id takes no second world
        rtp::FileWorld a, b;
        std::printf("first %d\n", a.join(dir, 0, 1));
        std::printf("second %d\n", b.join(dir, 0, 1));
        return 0;
    }
    if (what == "absent") {  // rank 1 of 2 never arrives; and a rank 1 whose rank 0 never does
        rtp::FileWorld w;
        w.deadline = std::chrono::milliseconds(50);
        std::printf("join %d\n", w.join(dir, 0, 2));
        int mine = 7, all[2] = {};
        auto t0 = std::chrono::steady_clock::now();
        std::printf("gather %d\n", w.allgather(&mine, sizeof(mine), all));
        std::printf("gather_ms %ld\n", ms_since(t0));
        rtp::FileWorld late;
        late.deadline = std::chrono::milliseconds(50);
        const std::string empty = std::string(dir) + "/empty";
        t0 = std::chrono::steady_clock::now();
        std::printf("late_join %d\n", late.join(empty.c_str(), 1, 2));
        std::printf("late_join_ms %ld\n", ms_since(t0));
        return 0;
    }
    if (what == "truncated") {  // rank 1's file of exchange 1 holds 2 of the 4 bytes
        rtp::FileWorld w;
        std::printf("join %d\n", w.join(dir, 0, 2));
        char name[64];
        std::snprintf(name, sizeof(name), "/x%016llx_1_r1", (unsigned long long)w.id());
        std::FILE* f = std::fopen((std::string(dir) + name).c_str(), "wb");
        if (!f || std::fwrite("ab", 1, 2, f) != 2 || std::fclose(f) != 0) return 3;
        int mine = 7, all[2] = {};
        std::printf("gather %d\n", w.allgather(&mine, sizeof(mine), all));
        return 0;
    }
    return 2;
}

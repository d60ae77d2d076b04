// rt_comm_files.cpp -- a shared world's exchange through files (rt_comm_files.hpp).
#include "rt_comm_files.hpp"

#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdio>
#include <new>
#include <thread>
#include <vector>

#include "../../include/rt_status.h"

namespace rtp {

using Clock = std::chrono::steady_clock;

std::string FileWorld::name(uint64_t seq, int q) const {
    char w[17];
    std::snprintf(w, sizeof(w), "%016llx", (unsigned long long)id_);
    return dir_ + "/x" + w + "_" + std::to_string(seq) + "_r" + std::to_string(q);
}

int FileWorld::join(const char* dir, int rank, int nranks) {
    try {
        dir_ = dir;
    } catch (const std::bad_alloc&) {
        return RT_OUT_OF_HOST_MEMORY;
    }
    rank_ = rank;
    nranks_ = nranks;
    const std::string path = dir_ + "/world";
    if (rank == 0) {
        uint64_t id = (uint64_t)Clock::now().time_since_epoch().count() * 0x9e3779b97f4a7c15ull ^ (uint64_t)getpid() << 32;
        if (id == 0) id = 1;
        const std::string tmp = path + ".tmp" + std::to_string(getpid());
        std::FILE* f = std::fopen(tmp.c_str(), "wb");
        if (!f) return RT_FILE_NOT_FOUND;
        const bool ok = std::fwrite(&id, sizeof(id), 1, f) == 1;
        if (std::fclose(f) != 0 || !ok) {
            (void)std::remove(tmp.c_str());
            return RT_OUT_OF_RESOURCES;
        }
        const int linked = link(tmp.c_str(), path.c_str());
        const int why = errno;
        (void)std::remove(tmp.c_str());
        if (linked != 0) return why == EEXIST ? RT_INVALID_VALUE : RT_OUT_OF_RESOURCES;
        id_ = id;
        return RT_SUCCESS;
    }
    const auto until = Clock::now() + deadline;
    for (;;) {
        if (std::FILE* f = std::fopen(path.c_str(), "rb")) {
            uint64_t id = 0;
            const bool ok = std::fread(&id, sizeof(id), 1, f) == 1;
            std::fclose(f);
            if (ok && id != 0) {
                id_ = id;
                return RT_SUCCESS;
            }
        }
        if (Clock::now() > until) return RT_OUT_OF_RESOURCES;
        std::this_thread::sleep_for(std::chrono::milliseconds(1));
    }
}

int FileWorld::allgather(const void* mine, size_t n, void* all) {
    const uint64_t seq = ++seq_;
    {
        const std::string own = name(seq, rank_), tmp = own + ".tmp";
        std::FILE* f = std::fopen(tmp.c_str(), "wb");
        if (!f) return RT_FILE_NOT_FOUND;
        const bool ok = std::fwrite(mine, 1, n, f) == n;
        if (std::fclose(f) != 0 || !ok || std::rename(tmp.c_str(), own.c_str()) != 0) return RT_OUT_OF_RESOURCES;
    }
    const auto until = Clock::now() + deadline;
    for (int q = 0; q < nranks_; ++q) {
        const std::string theirs = name(seq, q);
        for (;;) {
            if (std::FILE* f = std::fopen(theirs.c_str(), "rb")) {
                const bool ok = std::fread(static_cast<uint8_t*>(all) + (size_t)q * n, 1, n, f) == n;
                std::fclose(f);
                if (!ok) return RT_PARSE_ERROR;
                break;
            }
            if (Clock::now() > until) return RT_OUT_OF_RESOURCES;
            std::this_thread::sleep_for(std::chrono::milliseconds(1));
        }
    }
    return RT_SUCCESS;
}

int FileWorld::max(int v, int* out) {
    std::vector<int> all((size_t)nranks_);
    const int rc = allgather(&v, sizeof(v), all.data());
    if (rc) return rc;
    *out = *std::max_element(all.begin(), all.end());
    return RT_SUCCESS;
}

void FileWorld::remove_own() {
    for (uint64_t q = 1; q < seq_; ++q) (void)std::remove(name(q, rank_).c_str());
}

}  // namespace rtp

// rt_comm_files.hpp -- a shared world's exchange (rtCommInitShared): the ranks are separate processes
// that meet through files in one directory.  Rank 0 publishes the world's id in DIR/world; every
// exchange is an all-gather through the files DIR/x<world id>_<exchange>_r<rank>, so files an earlier
// world left are never read.  Pure POSIX host code: no HIP (tests/test_comm_files.py runs the ranks as
// threads of a stand-alone program).  Returns rt_status.h codes.
#pragma once

#include <chrono>
#include <cstddef>
#include <cstdint>
#include <string>

namespace rtp {

class FileWorld {
public:
    // how long join() waits for rank 0's id, and allgather() for the slowest rank
    std::chrono::milliseconds deadline{60000};

    // Rank 0 writes the id aside and links it into place: a directory that already holds one -- an
    // earlier world's -- is refused (RT_INVALID_VALUE).  The other ranks wait for it
    // (RT_OUT_OF_RESOURCES at the deadline).
    int join(const char* dir, int rank, int nranks);
    // `all` := every rank's `n` bytes, in rank order.  Each rank writes its file under a temporary
    // name and renames it, so a reader never sees half of one; a file shorter than n: RT_PARSE_ERROR.
    int allgather(const void* mine, size_t n, void* all);
    // the world's maximum of v
    int max(int v, int* out);
    // Removes this rank's own exchange files but the last: every rank wrote its file of exchange k
    // only after reading all files of exchange k - 1, so those have all been read; the last one may
    // still be awaited by a slower rank (the caller removes the directory).
    void remove_own();

    uint64_t id() const { return id_; }

private:
    std::string name(uint64_t seq, int q) const;

    std::string dir_;
    int rank_ = 0, nranks_ = 1;
    uint64_t id_ = 0;   // rank 0's, from DIR/world: part of every exchange file name
    uint64_t seq_ = 0;  // exchanges so far
};

}  // namespace rtp

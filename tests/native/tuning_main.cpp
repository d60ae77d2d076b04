// tuning_main.cpp -- stand-alone driver of the tuning table (csrc/rt_tuning.cpp), CPU only; built
// with -fsanitize=address,undefined by tests/test_tuning.py.  Reads one command per line from stdin,
// all on one rtp::Tuning, and prints one line per command:
//   fresh            start again from a default-constructed Tuning   -> "ok"
//   set ID VALUE     tuning_set                                      -> "RC"
//   get ID           tuning_get                                      -> "RC VALUE" (VALUE 0 when refused)
//   flag             refill_min_set                                  -> "0" or "1"
#include <cstdio>
#include <cstring>

#include "../../mini-opencl-raytracer_amd/csrc/rt_tuning.hpp"

int main() {
    rtp::Tuning t;
    char line[256], cmd[16];
    while (std::fgets(line, sizeof(line), stdin)) {
        int id = 0, value = 0;
        const int n = std::sscanf(line, "%15s %d %d", cmd, &id, &value);
        if (n == 1 && std::strcmp(cmd, "fresh") == 0) {
            t = rtp::Tuning{};
            std::printf("ok\n");
        } else if (n == 3 && std::strcmp(cmd, "set") == 0) {
            std::printf("%d\n", rtp::tuning_set(t, id, value));
        } else if (n == 2 && std::strcmp(cmd, "get") == 0) {
            int out = 0;
            const int rc = rtp::tuning_get(t, id, &out);
            std::printf("%d %d\n", rc, out);
        } else if (n == 1 && std::strcmp(cmd, "flag") == 0) {
            std::printf("%d\n", (int)t.refill_min_set);
        } else if (n >= 1) {
            std::fprintf(stderr, "tuning_main: bad command: %s", line);
            return 2;
        }
    }
    return 0;
}

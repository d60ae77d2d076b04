// refit_sanitize_main.cpp -- stand-alone driver of rtsRefitBounds (host/scene.cpp) for
// tests/test_refit_host.py, which builds it with -fsanitize=address,undefined.
//
//   refit_sanitize_main <triangles.bin> <nodes.bin> <nodes_out.bin>
//
// reads the raw CLTriangle / CLLinearBVHNode arrays, refits the nodes in exactly-sized heap blocks
// (so that a read or write past either array is a sanitizer report), prints the status code and
// writes the nodes as they are afterwards.  Exit status 0 whatever the status code; 2 on a usage or
// file error.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/rt_scene.h"

static bool read_file(const char* path, std::vector<unsigned char>& out) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    out.resize(n > 0 ? (size_t)n : 0);
    const bool ok = out.empty() || std::fread(out.data(), 1, out.size(), f) == out.size();
    std::fclose(f);
    return ok;
}

int main(int argc, char** argv) {
    if (argc != 4) {
        std::fprintf(stderr, "usage: %s triangles.bin nodes.bin nodes_out.bin\n", argv[0]);
        return 2;
    }
    std::vector<unsigned char> tb, nb;
    if (!read_file(argv[1], tb) || !read_file(argv[2], nb)) return 2;
    if (tb.size() % sizeof(rt_cl_triangle) || nb.size() % sizeof(rt_cl_bvh_node)) return 2;
    const size_t nt = tb.size() / sizeof(rt_cl_triangle), nn = nb.size() / sizeof(rt_cl_bvh_node);
    // exactly-sized blocks of the right type and alignment
    rt_cl_triangle* tris = nt ? static_cast<rt_cl_triangle*>(std::malloc(tb.size())) : nullptr;
    rt_cl_bvh_node* nodes = nn ? static_cast<rt_cl_bvh_node*>(std::malloc(nb.size())) : nullptr;
    if ((nt && !tris) || (nn && !nodes)) return 2;
    if (nt) std::memcpy(tris, tb.data(), tb.size());
    if (nn) std::memcpy(nodes, nb.data(), nb.size());
    const int rc = rtsRefitBounds(tris, nt, nodes, nn);
    std::printf("%d\n", rc);
    FILE* f = std::fopen(argv[3], "wb");
    if (!f) return 2;
    const bool ok = nn == 0 || std::fwrite(nodes, sizeof(rt_cl_bvh_node), nn, f) == nn;
    std::fclose(f);
    std::free(tris);
    std::free(nodes);
    return ok ? 0 : 2;
}

// node_collapse_main.cpp -- stand-alone driver of the octant records' collapsed link set
// (csrc/rt_scene_pack.cpp: collapse_oct_links through pack_scene_host), CPU only; built with
// -fsanitize=address,undefined by tests/test_node_collapse.py.
//   node_collapse_main pack NODES TRIS PREFIX
//       packs the scene of the two raw files (rt_cl_bvh_node / rt_cl_triangle arrays) and writes the
//       four record sets as raw words to PREFIX.oct, .octc (collapsed), .goct, .goctc (an empty file:
//       the set does not exist); prints "n N oct_ok K links C goct_b B group G".
//   node_collapse_main walk NODES TRIS RAYS
//       replays every ray of RAYS (raw float32 x 6: origin, direction) over the plain and over the
//       collapsed records with the kernels' node step (oct_step, rt_kernels_body.hpp) and a plain
//       Moeller-Trumbore triangle step, compares the two walks event for event, and counts during the
//       plain walk the visits the rule implies: an interior node reached from its parent's hit_next
//       whose six bound words (from the node buffer, not the records) are the parent's, or the
//       implied parent's.  Prints "rays R visits_plain A visits_collapsed B implied I implied_failed F
//       mismatches M leaves L tests T hits H".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../mini-opencl-raytracer_amd/csrc/rt_scene_pack.hpp"

namespace {

bool read_file(const char* path, std::vector<uint8_t>& out) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    out.resize(n > 0 ? (size_t)n : 0);
    const size_t got = out.empty() ? 0 : std::fread(out.data(), 1, out.size(), f);
    std::fclose(f);
    return got == out.size();
}

bool write_words(const std::string& path, const std::vector<uint32_t>& w) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const size_t put = w.empty() ? 0 : std::fwrite(w.data(), 4, w.size(), f);
    std::fclose(f);
    return put == w.size();
}

float as_float(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

struct Event {  // one leaf entry or one triangle test
    uint32_t kind, a, b;
    bool operator==(const Event& o) const { return kind == o.kind && a == o.a && b == o.b; }
};

struct Walk {
    std::vector<Event> events;
    uint64_t visits = 0, implied = 0, implied_failed = 0, leaves = 0, tests = 0;
    float t = 0.0f;
    int32_t prim = -1;
};

struct Scene {
    std::vector<uint8_t> nodes, tris;
    rtp::HostPack pack;
    const rt_cl_bvh_node* nd() const { return reinterpret_cast<const rt_cl_bvh_node*>(nodes.data()); }
    const rt_cl_triangle* tr() const { return reinterpret_cast<const rt_cl_triangle*>(tris.data()); }
};

bool same_bounds(const rt_cl_bvh_node& a, const rt_cl_bvh_node& b) {
    return std::memcmp(&a.bounds.pmin, &b.bounds.pmin, 12) == 0 && std::memcmp(&a.bounds.pmax, &b.bounds.pmax, 12) == 0;
}

// One ray over one record set.  count_implied: the plain walk's bookkeeping of implied visits.
void walk(const Scene& sc, const std::vector<uint32_t>& oct, const float* ray, bool count_implied, Walk* out) {
    const uint32_t n = sc.pack.n_nodes, stride = rtp::oct_stride(n), bofs = rtp::oct_b(n);
    const float o[3] = {ray[0], ray[1], ray[2]}, d[3] = {ray[3], ray[4], ray[5]};
    const float inv[3] = {1.0f / d[0], 1.0f / d[1], 1.0f / d[2]};
    const uint32_t sgn = (inv[0] < 0.0f ? 1u : 0u) | (inv[1] < 0.0f ? 2u : 0u) | (inv[2] < 0.0f ? 4u : 0u);
    Walk& w = *out;
    w.t = 100000.0f;
    uint32_t cur = 0;
    int64_t via_hit_from = -1;  // the node whose hit_next led here, when it (or its chain) has cur's box
    while (cur < n) {
        const uint32_t* A = &oct[((size_t)sgn * stride + cur) * 4];
        const uint32_t* B = &oct[((size_t)bofs + (size_t)sgn * stride + cur) * 4];
        float t0 = fmaxf(0.0f, (as_float(A[0]) - o[0]) * inv[0]);
        float t1 = fminf(w.t, (as_float(A[3]) - o[0]) * inv[0]);
        t0 = fmaxf(t0, (as_float(A[1]) - o[1]) * inv[1]);
        t1 = fminf(t1, (as_float(B[0]) - o[1]) * inv[1]);
        t0 = fmaxf(t0, (as_float(A[2]) - o[2]) * inv[2]);
        t1 = fminf(t1, (as_float(B[1]) - o[2]) * inv[2]);
        const bool hit = t1 >= t0;
        ++w.visits;
        const bool interior = sc.nd()[cur].nPrimitives == 0;
        const bool implied = count_implied && via_hit_from >= 0 && interior && same_bounds(sc.nd()[via_hit_from], sc.nd()[cur]);
        if (implied) {
            ++w.implied;
            if (!hit) ++w.implied_failed;
        }
        const uint32_t hn = B[2], mn = B[3];
        if (!hit) {
            cur = mn;
            via_hit_from = -1;
            continue;
        }
        if (hn < rtp::kLeafMin) {
            via_hit_from = cur;
            cur = hn;
            continue;
        }
        const uint32_t first = hn & 0x00ffffffu, count = hn >> 24;
        w.events.push_back(Event{0u, first, count});
        ++w.leaves;
        for (uint32_t k = first; k < first + count; ++k) {
            w.events.push_back(Event{1u, k, 0u});
            ++w.tests;
            const rt_cl_triangle& T = sc.tr()[k];
            const float p[3] = {T.v1.position.x, T.v1.position.y, T.v1.position.z};
            const float e1[3] = {T.v2.position.x - p[0], T.v2.position.y - p[1], T.v2.position.z - p[2]};
            const float e2[3] = {T.v3.position.x - p[0], T.v3.position.y - p[1], T.v3.position.z - p[2]};
            const float pv[3] = {d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]};
            const float det = e1[0] * pv[0] + e1[1] * pv[1] + e1[2] * pv[2];
            if (!(std::fabs(det) > 1e-12f)) continue;
            const float id = 1.0f / det;
            const float tv[3] = {o[0] - p[0], o[1] - p[1], o[2] - p[2]};
            const float u = (tv[0] * pv[0] + tv[1] * pv[1] + tv[2] * pv[2]) * id;
            const float qv[3] = {tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0]};
            const float v = (d[0] * qv[0] + d[1] * qv[1] + d[2] * qv[2]) * id;
            const float t = (e2[0] * qv[0] + e2[1] * qv[1] + e2[2] * qv[2]) * id;
            if (u >= 0.0f && v >= 0.0f && u + v <= 1.0f && t > 0.0f && t < w.t) {
                w.t = t;
                w.prim = (int32_t)k;
            }
        }
        cur = mn;  // the visited record's continuation
        via_hit_from = -1;
    }
}

bool load(const char* nodes, const char* tris, Scene* sc) {
    if (!read_file(nodes, sc->nodes) || !read_file(tris, sc->tris)) return false;
    rtp::SceneBytes in;
    in.nodes = sc->nodes.data(), in.nodes_size = sc->nodes.size();
    in.tris = sc->tris.data(), in.tris_size = sc->tris.size();
    return rtp::pack_scene_host(in, 384, &sc->pack) == 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 5 && std::strcmp(argv[1], "pack") == 0) {
        Scene sc;
        if (!load(argv[2], argv[3], &sc)) return 2;
        const rtp::HostPack& p = sc.pack;
        const std::string pre = argv[4];
        if (!write_words(pre + ".oct", p.oct_nodes) || !write_words(pre + ".octc", p.oct_nodes_collapsed) ||
            !write_words(pre + ".goct", p.goct_nodes) || !write_words(pre + ".goctc", p.goct_nodes_collapsed))
            return 3;
        std::printf("n %u oct_ok %d links %u goct_b %u group %d\n", p.n_nodes, (int)p.oct_ok, p.collapsed_links, p.goct_b,
                    (int)RT_GOCT_GROUP);
        return 0;
    }
    if (argc == 5 && std::strcmp(argv[1], "walk") == 0) {
        Scene sc;
        std::vector<uint8_t> rays;
        if (!load(argv[2], argv[3], &sc) || !sc.pack.oct_ok || !read_file(argv[4], rays)) return 2;
        const std::vector<uint32_t>& plain = sc.pack.oct_nodes;
        const std::vector<uint32_t>& coll = sc.pack.collapsed_links ? sc.pack.oct_nodes_collapsed : plain;
        const size_t n_rays = rays.size() / 24;
        uint64_t vp = 0, vc = 0, implied = 0, failed = 0, mism = 0, leaves = 0, tests = 0, hits = 0;
        for (size_t r = 0; r < n_rays; ++r) {
            float ray[6];
            std::memcpy(ray, rays.data() + r * 24, 24);
            Walk a, b;
            walk(sc, plain, ray, true, &a);
            walk(sc, coll, ray, false, &b);
            uint32_t ta, tb;
            std::memcpy(&ta, &a.t, 4);
            std::memcpy(&tb, &b.t, 4);
            if (!(a.events == b.events) || ta != tb || a.prim != b.prim) ++mism;
            vp += a.visits, vc += b.visits, implied += a.implied, failed += a.implied_failed;
            leaves += a.leaves, tests += a.tests, hits += a.prim >= 0;
        }
        std::printf("rays %zu visits_plain %llu visits_collapsed %llu implied %llu implied_failed %llu mismatches %llu "
                    "leaves %llu tests %llu hits %llu\n",
                    n_rays, (unsigned long long)vp, (unsigned long long)vc, (unsigned long long)implied,
                    (unsigned long long)failed, (unsigned long long)mism, (unsigned long long)leaves,
                    (unsigned long long)tests, (unsigned long long)hits);
        return 0;
    }
    std::fprintf(stderr, "usage: node_collapse_main pack NODES TRIS PREFIX | walk NODES TRIS RAYS\n");
    return 2;
}

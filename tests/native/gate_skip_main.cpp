// gate_skip_main.cpp -- stand-alone driver of the octant records' gate-skipped link set
// (csrc/rt_scene_pack.cpp: boxes_nest, select_gate_skips, gate_skip_oct_links through pack_scene_host and
// pack_pruned_links), CPU only; built with -fsanitize=address,undefined by tests/test_gate_skip.py.
//   gate_skip_main pack NODES TRIS PREFIX
//       packs the scene of the two raw files (rt_cl_bvh_node / rt_cl_triangle arrays) and writes the record
//       sets as raw words to PREFIX.oct, .octc (collapsed), .octg (gate-skipped), .octp (pruned over the
//       collapsed set), .octgp (pruned over the gate-skipped set), .goct, .goctg, .goctgp, and the removed
//       set, one byte per node, to PREFIX.removed (an empty file: the set does not exist); prints
//       "n N oct_ok K nested X links C gate G gated E pruned P gated_pruned Q goct_b B group R".
//   gate_skip_main walk NODES TRIS RAYS
//       replays every ray of RAYS (raw float32 x 7: origin, direction, tmax) over the plain, the collapsed and
//       the gate-skipped records, and over the two pruned sets, with the kernels' node step written out for
//       three reciprocals of the direction (the IEEE quotient of the pinned and device-library policies; the
//       frexp / ldexp form; a reciprocal one ulp off, as the shipped policy's hardware rcp may be), as a
//       closest-hit walk and as an any-hit walk that ends at the first accepted test.  The gate-skipped walk's
//       leaf entries and triangle tests must be the plain walk's, in its order, and {t, prim} its bits; the
//       two pruned walks must agree likewise.  A scene that has no gate-skipped set walks its collapsed
//       records in its place.  Prints "rays R walks W visits_plain A visits_collapsed B visits_gated C
//       visits_pruned D visits_gated_pruned E tests T mismatches M hits H misses Z".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../mini-opencl-raytracer_amd/csrc/rt_octant_cull.hpp"
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

template <class T>
bool write_vec(const std::string& path, const std::vector<T>& w) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f) return false;
    const size_t put = w.empty() ? 0 : std::fwrite(w.data(), sizeof(T), w.size(), f);
    std::fclose(f);
    return put == w.size();
}

float as_float(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}
uint32_t as_bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

// the three reciprocals a node step may see
float rcp_of(float d, int policy) {
    if (policy == 0) return 1.0f / d;
    if (policy == 1) {
        int e = 0;
        const float m = std::frexp(d, &e);  // (0, inf and NaN come back as they are, e = 0)
        return std::ldexp(1.0f / m, -e);
    }
    const float r = 1.0f / d;
    if (!std::isfinite(r) || r == 0.0f) return r;
    return std::nextafterf(r, r < 0.0f ? -INFINITY : INFINITY);
}

struct Event {  // one leaf entry (kind 0: first, count) or one triangle test (kind 1: triangle)
    uint32_t kind, a, b;
    bool operator==(const Event& o) const { return kind == o.kind && a == o.a && b == o.b; }
};

struct Walk {
    std::vector<Event> events;
    uint64_t visits = 0, tests = 0;
    float t = 0.0f;
    int32_t prim = -1;
};

struct Scene {
    std::vector<uint8_t> nodes, tris, mask;
    rtp::HostPack pack;
    const rt_cl_triangle* tr() const { return reinterpret_cast<const rt_cl_triangle*>(tris.data()); }
};

// the kernels' node step (oct_step, oct_step_w, oct_step_g of rt_kernels_body.hpp: one arithmetic) and the
// reference's triangle test
void walk(const Scene& sc, const std::vector<uint32_t>& oct, const float* ray, int policy, bool any_hit, Walk* out) {
    const uint32_t n = sc.pack.n_nodes, stride = rtp::oct_stride(n), bofs = rtp::oct_b(n);
    const float o[3] = {ray[0], ray[1], ray[2]}, d[3] = {ray[3], ray[4], ray[5]};
    const float inv[3] = {rcp_of(d[0], policy), rcp_of(d[1], policy), rcp_of(d[2], policy)};
    const uint32_t sgn = (inv[0] < 0.0f ? 1u : 0u) | (inv[1] < 0.0f ? 2u : 0u) | (inv[2] < 0.0f ? 4u : 0u);
    Walk& w = *out;
    w.t = ray[6];
    uint32_t cur = 0;
    while (cur < n) {
        const uint32_t* A = &oct[((size_t)sgn * stride + cur) * 4];
        const uint32_t* B = &oct[((size_t)bofs + (size_t)sgn * stride + cur) * 4];
        float t0 = fmaxf(0.0f, (as_float(A[0]) - o[0]) * inv[0]);
        float t1 = fminf(w.t, (as_float(A[3]) - o[0]) * inv[0]);
        t0 = fmaxf(t0, (as_float(A[1]) - o[1]) * inv[1]);
        t1 = fminf(t1, (as_float(B[0]) - o[1]) * inv[1]);
        t0 = fmaxf(t0, (as_float(A[2]) - o[2]) * inv[2]);
        t1 = fminf(t1, (as_float(B[1]) - o[2]) * inv[2]);
        ++w.visits;
        const uint32_t hn = B[2], mn = B[3];
        if (!(t1 >= t0)) {
            cur = mn;
            continue;
        }
        if (hn < rtp::kLeafMin) {
            cur = hn;
            continue;
        }
        const uint32_t first = hn & 0x00ffffffu, count = hn >> 24;
        w.events.push_back(Event{0u, first, count});
        for (uint32_t k = first; k < first + count; ++k) {
            ++w.tests;
            w.events.push_back(Event{1u, k, 0u});
            const rt_cl_triangle& T = sc.tr()[k];
            const rtp::CullEdges e = rtp::octant_cull_edges(T);
            const float p[3] = {T.v1.position.x, T.v1.position.y, T.v1.position.z};
            const float pv[3] = {d[1] * e.e2[2] - d[2] * e.e2[1], d[2] * e.e2[0] - d[0] * e.e2[2],
                                 d[0] * e.e2[1] - d[1] * e.e2[0]};
            const float det = (e.e1[0] * pv[0] + e.e1[1] * pv[1]) + e.e1[2] * pv[2];
            if (det < 1e-8f) continue;
            const float id = 1.0f / det;
            const float tv[3] = {o[0] - p[0], o[1] - p[1], o[2] - p[2]};
            const float u = ((tv[0] * pv[0] + tv[1] * pv[1]) + tv[2] * pv[2]) * id;
            if (u < 0.0f || u > 1.0f) continue;
            const float qv[3] = {tv[1] * e.e1[2] - tv[2] * e.e1[1], tv[2] * e.e1[0] - tv[0] * e.e1[2],
                                 tv[0] * e.e1[1] - tv[1] * e.e1[0]};
            const float v = ((d[0] * qv[0] + d[1] * qv[1]) + d[2] * qv[2]) * id;
            if (v < 0.0f || u + v > 1.0f) continue;
            const float t = ((e.e2[0] * qv[0] + e.e2[1] * qv[1]) + e.e2[2] * qv[2]) * id;
            if (t < w.t) {
                w.t = t;
                w.prim = (int32_t)k;
                if (any_hit) return;
            }
        }
        cur = mn;  // the visited record's continuation
    }
}

bool load(const char* nodes, const char* tris, Scene* sc) {
    if (!read_file(nodes, sc->nodes) || !read_file(tris, sc->tris)) return false;
    rtp::SceneBytes in;
    in.nodes = sc->nodes.data(), in.nodes_size = sc->nodes.size();
    in.tris = sc->tris.data(), in.tris_size = sc->tris.size();
    if (rtp::pack_scene_host(in, 384, &sc->pack) != 0) return false;
    sc->mask.resize(sc->pack.n_tris);
    rtp::octant_cull_masks(sc->tr(), sc->pack.n_tris, sc->mask.data());
    rtp::pack_pruned_links(sc->mask.data(), &sc->pack);
    return true;
}

bool same(const Walk& a, const Walk& b) {
    return a.events == b.events && as_bits(a.t) == as_bits(b.t) && a.prim == b.prim;
}
bool same_result(const Walk& a, const Walk& b) { return as_bits(a.t) == as_bits(b.t) && a.prim == b.prim; }

}  // namespace

int main(int argc, char** argv) {
    if (argc == 5 && std::strcmp(argv[1], "pack") == 0) {
        Scene sc;
        if (!load(argv[2], argv[3], &sc)) return 2;
        const rtp::HostPack& p = sc.pack;
        const std::string pre = argv[4];
        if (!write_vec(pre + ".oct", p.oct_nodes) || !write_vec(pre + ".octc", p.oct_nodes_collapsed) ||
            !write_vec(pre + ".octg", p.oct_nodes_gated) || !write_vec(pre + ".octp", p.oct_nodes_pruned) ||
            !write_vec(pre + ".octgp", p.oct_nodes_gated_pruned) || !write_vec(pre + ".goct", p.goct_nodes) ||
            !write_vec(pre + ".goctg", p.goct_nodes_gated) || !write_vec(pre + ".goctgp", p.goct_nodes_gated_pruned) ||
            !write_vec(pre + ".removed", p.gate_removed))
            return 3;
        std::printf("n %u oct_ok %d nested %d links %u gate %u gated %d pruned %u gated_pruned %u goct_b %u group %d\n",
                    p.n_nodes, (int)p.oct_ok, (int)p.nested, p.collapsed_links, p.gate_links,
                    (int)!p.oct_nodes_gated.empty(), p.pruned_links, p.gated_pruned_links, p.goct_b, (int)RT_GOCT_GROUP);
        return 0;
    }
    if (argc == 5 && std::strcmp(argv[1], "walk") == 0) {
        Scene sc;
        std::vector<uint8_t> rays;
        if (!load(argv[2], argv[3], &sc) || !sc.pack.oct_ok || !read_file(argv[4], rays)) return 2;
        const rtp::HostPack& p = sc.pack;
        const std::vector<uint32_t>& plain = p.oct_nodes;
        const std::vector<uint32_t>& coll = p.collapsed_links ? p.oct_nodes_collapsed : plain;
        const std::vector<uint32_t>& gate = p.oct_nodes_gated.empty() ? coll : p.oct_nodes_gated;
        const std::vector<uint32_t>& prun = p.pruned_links ? p.oct_nodes_pruned : coll;
        const std::vector<uint32_t>& gprun = p.oct_nodes_gated.empty() ? prun
                                             : p.gated_pruned_links   ? p.oct_nodes_gated_pruned
                                                                      : gate;
        const size_t n_rays = rays.size() / 28;
        uint64_t walks = 0, vp = 0, vc = 0, vg = 0, vq = 0, vgq = 0, tests = 0, mism = 0, hits = 0, misses = 0;
        for (size_t r = 0; r < n_rays; ++r) {
            float ray[7];
            std::memcpy(ray, rays.data() + r * 28, 28);
            for (int policy = 0; policy < 3; ++policy)
                for (int any = 0; any < 2; ++any) {
                    Walk a, b, c, q, gq;
                    walk(sc, plain, ray, policy, any != 0, &a);
                    walk(sc, coll, ray, policy, any != 0, &b);
                    walk(sc, gate, ray, policy, any != 0, &c);
                    walk(sc, prun, ray, policy, any != 0, &q);
                    walk(sc, gprun, ray, policy, any != 0, &gq);
                    // a pruned walk leaves certified tests out: its events are the other pruned walk's, its
                    // result the plain walk's (an any-hit walk accepts the same first test: none is removed)
                    if (!same(a, b) || !same(a, c) || !same(q, gq) || !same_result(a, gq)) ++mism;
                    ++walks;
                    vp += a.visits, vc += b.visits, vg += c.visits, vq += q.visits, vgq += gq.visits, tests += a.tests;
                    if (policy == 0 && any == 0) (a.prim >= 0 ? hits : misses) += 1;
                }
        }
        std::printf("rays %zu walks %llu visits_plain %llu visits_collapsed %llu visits_gated %llu visits_pruned %llu "
                    "visits_gated_pruned %llu tests %llu mismatches %llu hits %llu misses %llu\n",
                    n_rays, (unsigned long long)walks, (unsigned long long)vp, (unsigned long long)vc,
                    (unsigned long long)vg, (unsigned long long)vq, (unsigned long long)vgq, (unsigned long long)tests,
                    (unsigned long long)mism, (unsigned long long)hits, (unsigned long long)misses);
        return 0;
    }
    std::fprintf(stderr, "usage: gate_skip_main pack NODES TRIS PREFIX | walk NODES TRIS RAYS\n");
    return 2;
}

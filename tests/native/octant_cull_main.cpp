// octant_cull_main.cpp -- stand-alone driver of the octant-cull certificate (csrc/rt_octant_cull.cpp) and
// of the pruned link set it allows (csrc/rt_scene_pack.cpp: prune_oct_links through pack_pruned_links), CPU
// only; built with -fsanitize=address,undefined by tests/test_octant_cull.py.
//   octant_cull_main cert TRIS MASKS
//       evaluates the certificate on every triangle of the raw rt_cl_triangle file, writes one mask byte per
//       triangle to MASKS, and checks every certified (triangle, octant) pair by brute force: det in fp32 over
//       the octant's directions (a lattice of magnitudes from 0 and the smallest denormal to 1, which holds
//       the +-0 components, the single-axis directions and components of 1e-30; unit vectors on an angular
//       grid; seeded random unit vectors), each in four evaluations -- without and with fma contraction, in
//       both association orders of the dot product.  Prints "tris N pairs P dirs D evals E violations V
//       max_det_e12 M" (violations: evaluations that are neither < 1e-8 nor NaN; M = the largest det seen, in
//       units of 1e-12, clamped to +-10^9).
//   octant_cull_main pack NODES TRIS PREFIX
//       packs the scene and writes the record sets as raw words to PREFIX.oct, .octc (collapsed), .octp
//       (pruned), .goct, .goctp and the masks to PREFIX.mask (an empty file: the set does not exist); prints
//       "n N oct_ok K links C pruned P pairs Q goct_b B group G".
//   octant_cull_main walk NODES TRIS RAYS
//       replays every ray of RAYS (raw float32 x 6: origin, direction) over the plain, the collapsed and the
//       pruned records with the kernels' node step and the reference's triangle test (det < 1e-8, u, v, then
//       t < best), and compares: the pruned walk's events must be the plain walk's without the entries and
//       tests of leaves that are wholly certified for the ray's octant, and the final {t, prim, u, v} of the
//       three walks must be the same bits.  Prints "rays R visits_plain A visits_collapsed B visits_pruned C
//       tests_plain T tests_pruned U removed_tests X removed_accepts Y certified_left Z mismatches M hits H
//       octants O" (removed_accepts: removed tests that the plain walk accepted; certified_left: tests of the
//       pruned walk whose pair is certified -- both must be 0 for "exactly the certified tests"; O: a bit per
//       octant that occurred).  An octant for which every triangle of the scene is certified keeps its links:
//       there the pruned walk must be the plain one.
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

// ---- det, four ways (this file is compiled with -ffp-contract=off: a plain expression rounds every
// operation, std::fmaf is the only fusion) ---------------------------------------------------------------
// kind 0: the pinned policy; 1: the device-library and shipped policy (rt_math.hpp); 2, 3: the same two
// with the dot product associated from the right and the other product of each cross component fused
float det_eval(const float d[3], const float e1[3], const float e2[3], int kind) {
    float pv[3];
    for (int i = 0; i < 3; ++i) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;  // pv.i = d.j e2.k - d.k e2.j
        if (kind == 0 || kind == 2)
            pv[i] = d[j] * e2[k] - d[k] * e2[j];
        else if (kind == 1)
            pv[i] = std::fmaf(d[j], e2[k], e2[j] * -d[k]);
        else
            pv[i] = std::fmaf(-d[k], e2[j], d[j] * e2[k]);
    }
    switch (kind) {
        case 0: return (e1[0] * pv[0] + e1[1] * pv[1]) + e1[2] * pv[2];
        case 1: return std::fmaf(e1[2], pv[2], std::fmaf(e1[1], pv[1], e1[0] * pv[0]));
        case 2: return e1[0] * pv[0] + (e1[1] * pv[1] + e1[2] * pv[2]);
        default: return std::fmaf(e1[0], pv[0], std::fmaf(e1[1], pv[1], e1[2] * pv[2]));
    }
}

struct Dir {
    float d[3];
};

// the directions of octant o: every component carries the octant's sign, zeros included
std::vector<Dir> octant_dirs(uint32_t o) {
    std::vector<Dir> out;
    const float sg[3] = {(o & 1u) ? -1.0f : 1.0f, (o & 2u) ? -1.0f : 1.0f, (o & 4u) ? -1.0f : 1.0f};
    const float mags[] = {0.0f, 1.4e-45f, 1e-40f, 1e-30f, 1e-10f, 1e-3f, 0.1f, 0.3f, 0.5f, 0.7f, 0.9f, 1.0f};
    for (float x : mags)
        for (float y : mags)
            for (float z : mags) out.push_back(Dir{{sg[0] * x, sg[1] * y, sg[2] * z}});
    // unit vectors on an angular grid of the octant, its edges included
    const int G = 32;
    for (int a = 0; a <= G; ++a)
        for (int b = 0; b <= G; ++b) {
            const double th = 1.5707963267948966 * a / G, ph = 1.5707963267948966 * b / G;
            out.push_back(Dir{{sg[0] * (float)(std::sin(th) * std::cos(ph)), sg[1] * (float)(std::sin(th) * std::sin(ph)),
                               sg[2] * (float)std::cos(th)}});
        }
    // seeded random unit vectors
    uint64_t s = 0x9e3779b97f4a7c15ull + o;
    auto rnd = [&]() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (double)(s >> 11) * (1.0 / 9007199254740992.0);
    };
    for (int i = 0; i < 2000; ++i) {
        const double x = rnd(), y = rnd(), z = rnd(), l = std::sqrt(x * x + y * y + z * z);
        if (l < 1e-3) continue;
        out.push_back(Dir{{sg[0] * (float)(x / l), sg[1] * (float)(y / l), sg[2] * (float)(z / l)}});
    }
    return out;
}

// ---- the replay walker -----------------------------------------------------------------------------------
struct Event {  // one leaf entry (kind 0: first, count) or one triangle test (kind 1: triangle)
    uint32_t kind, a, b;
    bool operator==(const Event& o) const { return kind == o.kind && a == o.a && b == o.b; }
};

struct Walk {
    std::vector<Event> events;
    std::vector<uint8_t> accepted;  // per event: the test was accepted
    uint64_t visits = 0, tests = 0;
    float t = 0.0f, u = 0.0f, v = 0.0f;
    int32_t prim = -1;
};

struct Scene {
    std::vector<uint8_t> nodes, tris, mask;
    rtp::HostPack pack;
    const rt_cl_triangle* tr() const { return reinterpret_cast<const rt_cl_triangle*>(tris.data()); }
};

void walk(const Scene& sc, const std::vector<uint32_t>& oct, const float* ray, Walk* out) {
    const uint32_t n = sc.pack.n_nodes, stride = rtp::oct_stride(n), bofs = rtp::oct_b(n);
    const float o[3] = {ray[0], ray[1], ray[2]}, d[3] = {ray[3], ray[4], ray[5]};
    const float inv[3] = {1.0f / d[0], 1.0f / d[1], 1.0f / d[2]};
    const uint32_t sgn = (inv[0] < 0.0f ? 1u : 0u) | (inv[1] < 0.0f ? 2u : 0u) | (inv[2] < 0.0f ? 4u : 0u);
    Walk& w = *out;
    w.t = 100000.0f;
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
        w.accepted.push_back(0);
        for (uint32_t k = first; k < first + count; ++k) {
            ++w.tests;
            w.events.push_back(Event{1u, k, 0u});
            w.accepted.push_back(0);
            // kernel_bvh.cl:98-153 with the edges as the device packs them
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
                w.t = t, w.u = u, w.v = v;
                w.prim = (int32_t)k;
                w.accepted.back() = 1;
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

bool same_result(const Walk& a, const Walk& b) {
    return as_bits(a.t) == as_bits(b.t) && a.prim == b.prim && as_bits(a.u) == as_bits(b.u) && as_bits(a.v) == as_bits(b.v);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc == 4 && std::strcmp(argv[1], "cert") == 0) {
        std::vector<uint8_t> bytes;
        if (!read_file(argv[2], bytes)) return 2;
        const rt_cl_triangle* tr = reinterpret_cast<const rt_cl_triangle*>(bytes.data());
        const uint32_t n = (uint32_t)(bytes.size() / sizeof(rt_cl_triangle));
        std::vector<uint8_t> mask(n);
        const uint32_t pairs = rtp::octant_cull_masks(tr, n, mask.data());
        if (!write_vec(argv[3], mask)) return 3;
        uint64_t evals = 0, violations = 0, dirs = 0;
        float max_det = -INFINITY;
        for (uint32_t o = 0; o < 8; ++o) {
            const std::vector<Dir> ds = octant_dirs(o);
            dirs += ds.size();
            for (uint32_t i = 0; i < n; ++i) {
                if (!((mask[i] >> o) & 1u)) continue;
                if (mask[i] != rtp::octant_cull_mask(tr[i])) return 4;
                const rtp::CullEdges e = rtp::octant_cull_edges(tr[i]);
                for (const Dir& d : ds)
                    for (int kind = 0; kind < 4; ++kind) {
                        const float det = det_eval(d.d, e.e1, e.e2, kind);
                        ++evals;
                        if (std::isnan(det)) continue;
                        if (!(det < 1e-8f)) ++violations;
                        if (det > max_det) max_det = det;
                    }
            }
        }
        const double m = std::fmin(1e9, std::fmax(-1e9, (double)max_det * 1e12));
        std::printf("tris %u pairs %u dirs %llu evals %llu violations %llu max_det_e12 %lld\n", n, pairs,
                    (unsigned long long)dirs, (unsigned long long)evals, (unsigned long long)violations,
                    evals ? (long long)m : 0ll);
        return 0;
    }
    if (argc == 5 && std::strcmp(argv[1], "pack") == 0) {
        Scene sc;
        if (!load(argv[2], argv[3], &sc)) return 2;
        const rtp::HostPack& p = sc.pack;
        const std::string pre = argv[4];
        if (!write_vec(pre + ".oct", p.oct_nodes) || !write_vec(pre + ".octc", p.oct_nodes_collapsed) ||
            !write_vec(pre + ".octp", p.oct_nodes_pruned) || !write_vec(pre + ".goct", p.goct_nodes) ||
            !write_vec(pre + ".goctp", p.goct_nodes_pruned) || !write_vec(pre + ".mask", sc.mask))
            return 3;
        uint32_t pairs = 0;
        for (uint8_t m : sc.mask) pairs += (uint32_t)__builtin_popcount(m);
        std::printf("n %u oct_ok %d links %u pruned %u pairs %u goct_b %u group %d\n", p.n_nodes, (int)p.oct_ok,
                    p.collapsed_links, p.pruned_links, pairs, p.goct_b, (int)RT_GOCT_GROUP);
        return 0;
    }
    if (argc == 5 && std::strcmp(argv[1], "walk") == 0) {
        Scene sc;
        std::vector<uint8_t> rays;
        if (!load(argv[2], argv[3], &sc) || !sc.pack.oct_ok || !read_file(argv[4], rays)) return 2;
        const std::vector<uint32_t>& plain = sc.pack.oct_nodes;
        const std::vector<uint32_t>& coll = sc.pack.collapsed_links ? sc.pack.oct_nodes_collapsed : plain;
        const std::vector<uint32_t>& prun = sc.pack.pruned_links ? sc.pack.oct_nodes_pruned : coll;
        const size_t n_rays = rays.size() / 24;
        uint64_t vp = 0, vc = 0, vq = 0, tp = 0, tq = 0, removed = 0, removed_acc = 0, left = 0, mism = 0, hits = 0;
        uint32_t octants = 0;
        // octants whose every triangle is certified: the root is culled there, and the links stay as they are
        uint8_t everything = 0xff;
        for (uint8_t m : sc.mask) everything &= m;
        for (size_t r = 0; r < n_rays; ++r) {
            float ray[6];
            std::memcpy(ray, rays.data() + r * 24, 24);
            Walk a, b, c;
            walk(sc, plain, ray, &a);
            walk(sc, coll, ray, &b);
            walk(sc, prun, ray, &c);
            const uint32_t sgn = (1.0f / ray[3] < 0.0f ? 1u : 0u) | (1.0f / ray[4] < 0.0f ? 2u : 0u) |
                                 (1.0f / ray[5] < 0.0f ? 4u : 0u);
            octants |= 1u << sgn;
            // the plain walk without the leaves wholly certified for this octant
            std::vector<Event> want;
            bool drop = false;
            const bool untouched = !RT_OCTANT_CULL || ((everything >> sgn) & 1u);
            for (size_t i = 0; i < a.events.size(); ++i) {
                const Event& e = a.events[i];
                if (e.kind == 0u) {
                    drop = true;
                    for (uint32_t k = e.a; k < e.a + e.b; ++k) drop = drop && !untouched && ((sc.mask[k] >> sgn) & 1u);
                }
                if (!drop) {
                    want.push_back(e);
                } else if (e.kind == 1u) {
                    ++removed;
                    removed_acc += a.accepted[i];
                }
            }
            for (const Event& e : c.events) left += !untouched && e.kind == 1u && ((sc.mask[e.a] >> sgn) & 1u);
            if (!(want == c.events) || !(a.events == b.events) || !same_result(a, b) || !same_result(a, c)) ++mism;
            vp += a.visits, vc += b.visits, vq += c.visits, tp += a.tests, tq += c.tests, hits += a.prim >= 0;
        }
        std::printf("rays %zu visits_plain %llu visits_collapsed %llu visits_pruned %llu tests_plain %llu tests_pruned %llu "
                    "removed_tests %llu removed_accepts %llu certified_left %llu mismatches %llu hits %llu octants %u\n",
                    n_rays, (unsigned long long)vp, (unsigned long long)vc, (unsigned long long)vq, (unsigned long long)tp,
                    (unsigned long long)tq, (unsigned long long)removed, (unsigned long long)removed_acc,
                    (unsigned long long)left, (unsigned long long)mism, (unsigned long long)hits, octants);
        return 0;
    }
    std::fprintf(stderr, "usage: octant_cull_main cert TRIS MASKS | pack NODES TRIS PREFIX | walk NODES TRIS RAYS\n");
    return 2;
}

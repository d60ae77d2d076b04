// rt_device_scene.cpp -- rti::DeviceScene: the device half of a scene preparation (allocation, the
// uploads, the pack and refit launches) around the pure host half, rtp::pack_scene_host.
#include "rt_device_scene.hpp"

#include <cstring>
#include <vector>

#include "rt_kernels.hpp"
#include "rt_octant_cull.hpp"
#include "rt_path_kill.hpp"
#include "rt_refit.hpp"
#include "rt_scene_pack.hpp"

namespace rti {

namespace {

// Host view of a buffer's bytes (shadow, or a device read-back).
int host_bytes(rt_mem m, std::vector<uint8_t>& tmp, const uint8_t** out) {
    if (m->shadow_valid) {
        *out = m->shadow.data();
        return RT_SUCCESS;
    }
    tmp.resize(m->size);
    hipError_t e = hipMemcpyAsync(tmp.data(), m->dptr, m->size, hipMemcpyDeviceToHost, qs(m->ctx));
    if (e == hipSuccess) e = hipStreamSynchronize(qs(m->ctx));
    if (e != hipSuccess) return map_hip(e);
    *out = tmp.data();
    return RT_SUCCESS;
}

template <class T>
int ensure_dev(T*& p, size_t& cap, size_t count) {
    if (cap >= count) return RT_SUCCESS;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    hipError_t e = hipMalloc(&p, count * sizeof(T));
    if (e != hipSuccess) return map_hip(e);
    cap = count;
    return RT_SUCCESS;
}

// every host-to-device copy of a preparation: `src` must outlive a synchronisation of `st`
hipError_t upload(void* dst, const std::vector<uint32_t>& src, hipStream_t st) {
    return hipMemcpyAsync(dst, src.data(), src.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st);
}

}  // namespace

int DeviceScene::allocate(uint32_t nn, uint32_t nt, uint32_t nmat, size_t goct_words, bool collapsed,
                          bool pruned) {
    int rc = ensure_dev(g_nodes_, g_nodes_cap_, (size_t)nn * 4);
    if (!rc) rc = ensure_dev(refit_links_, refit_links_cap_, (size_t)nn * 2);
    if (!rc) rc = ensure_dev(refit_arrivals_, refit_arrivals_cap_, (size_t)nn);
    if (!rc) rc = ensure_dev(oct_nodes_, oct_nodes_cap_, (size_t)rtp::oct_records(nn));
    if (!rc) rc = ensure_dev(goct_nodes_, goct_nodes_cap_, goct_words / 4);
    if (!rc && collapsed) rc = ensure_dev(oct_collapsed_, oct_collapsed_cap_, (size_t)rtp::oct_records(nn));
    if (!rc && collapsed) rc = ensure_dev(goct_collapsed_, goct_collapsed_cap_, goct_words / 4);
    if (!rc && pruned) rc = ensure_dev(oct_pruned_, oct_pruned_cap_, (size_t)rtp::oct_records(nn));
    if (!rc && pruned) rc = ensure_dev(goct_pruned_, goct_pruned_cap_, goct_words / 4);
    if (!rc) rc = ensure_dev(packed_tris_, packed_tris_cap_, (size_t)nt * 3);
    if (!rc) rc = ensure_dev(shade_tris_, shade_tris_cap_, (size_t)nt * 3);
    // two material tables: IEEE divisions (pinned, devicelib), then the shipped policy's
    if (!rc) rc = ensure_dev(shade_mats_, shade_mats_cap_, (size_t)nmat * 8);
    return rc;
}

int DeviceScene::prepare(rt_context ctx, rt_mem tm, rt_mem nm, rt_mem mm) {
    if (!stale(tm, nm, mm)) return RT_SUCCESS;
    // the host half: nothing on the device changes unless the scene is sound
    std::vector<uint8_t> tmp_t, tmp_n;
    rtp::SceneBytes in;
    in.tris_size = tm->size, in.nodes_size = nm->size;
    int rc = host_bytes(tm, tmp_t, &in.tris);
    if (!rc) rc = host_bytes(nm, tmp_n, &in.nodes);
    if (rc) return rc;
    if (mm) {  // (the host reads no material byte: the bound buffer's address stands for them)
        in.mats = static_cast<const uint8_t*>(mm->dptr);
        in.mats_size = mm->size;
    }
    rtp::HostPack p;
    rc = rtp::pack_scene_host(in, top_limit, &p);
    if (rc) return rc;
    // the octant-cull certificate per triangle, on the vertices the device packs its edges from, and the
    // pruned link set it allows
    if (RT_OCTANT_CULL && p.oct_ok) {
        std::vector<uint8_t> tri_octants(p.n_tris);
        rtp::octant_cull_masks(reinterpret_cast<const rt_cl_triangle*>(in.tris), p.n_tris, tri_octants.data());
        rtp::pack_pruned_links(tri_octants.data(), &p);
    }
    // the device half: from here on the records are no longer those of the scene remembered
    invalidate();
    // the second and third record sets a launch walks: the gate-skipped set and its pruned form where the
    // scene has one, else the collapsed set and the pruned set over it
    const bool gated = !p.oct_nodes_gated.empty();
    const std::vector<uint32_t>& oct2 = gated ? p.oct_nodes_gated : p.oct_nodes_collapsed;
    const std::vector<uint32_t>& goct2 = gated ? p.goct_nodes_gated : p.goct_nodes_collapsed;
    const std::vector<uint32_t>& oct3 = gated ? p.oct_nodes_gated_pruned : p.oct_nodes_pruned;
    const std::vector<uint32_t>& goct3 = gated ? p.goct_nodes_gated_pruned : p.goct_nodes_pruned;
    rc = allocate(p.n_nodes, p.n_tris, p.n_mats, p.goct_nodes.size(), !oct2.empty(), !oct3.empty());
    if (rc) return rc;
    hipStream_t st = qs(ctx);
    hipError_t e = upload(g_nodes_, p.global_nodes, st);
    if (e == hipSuccess) e = upload(refit_links_, p.refit_links, st);
    if (e == hipSuccess) e = upload(oct_nodes_, p.oct_nodes, st);
    if (e == hipSuccess && !p.goct_nodes.empty()) e = upload(goct_nodes_, p.goct_nodes, st);
    if (e == hipSuccess && !oct2.empty()) e = upload(oct_collapsed_, oct2, st);
    if (e == hipSuccess && !goct2.empty()) e = upload(goct_collapsed_, goct2, st);
    if (e == hipSuccess && !oct3.empty()) e = upload(oct_pruned_, oct3, st);
    if (e == hipSuccess && !goct3.empty()) e = upload(goct_pruned_, goct3, st);
    if (e == hipSuccess)
        e = rtk::launch_pack(static_cast<const rt_cl_triangle*>(tm->dptr), p.n_tris, packed_tris_, shade_tris_,
                             mm ? static_cast<const rt_cl_material*>(mm->dptr) : nullptr, p.n_mats, shade_mats_, st);
    // `p` is the source of the copies enqueued above: it outlives this wait whatever `e` says
    const hipError_t waited = hipStreamSynchronize(st);
    if (e == hipSuccess) e = waited;
    if (e != hipSuccess) return map_hip(e);
    n_nodes_ = p.n_nodes, n_tris_ = p.n_tris, n_mats_ = p.n_mats, n_top_ = p.n_top;
    oct_ok_ = p.oct_ok, goct_b_ = p.goct_b;
    collapsed_links_ = p.collapsed_links, collapse_known_ = RT_NODE_COLLAPSE != 0;
    pruned_links_ = p.pruned_links, cull_known_ = RT_OCTANT_CULL != 0 && p.oct_ok;
    gate_links_ = p.gate_links, gate_skipped_ = gated;
    has_collapsed_ = !oct2.empty(), has_pruned_ = !oct3.empty();
    root_known_ = p.n_nodes > 0 && in.nodes_size >= sizeof(rt_cl_bvh_node);
    if (root_known_) {
        rt_cl_bvh_node root;
        std::memcpy(&root, in.nodes, sizeof(root));
        const float b[6] = {root.bounds.pmin.x, root.bounds.pmin.y, root.bounds.pmin.z,
                            root.bounds.pmax.x, root.bounds.pmax.y, root.bounds.pmax.z};
        std::memcpy(root_bounds_, b, sizeof(b));
    }
    // the path-kill certificate, on the material records as the device just formed them (both tables)
    kill_known_ = false;
    if (mm && p.n_mats > 0) {
        std::vector<float> recs((size_t)p.n_mats * 32);
        e = hipMemcpyAsync(recs.data(), shade_mats_, recs.size() * sizeof(float), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return map_hip(e);
        const rt_cl_triangle* ht = reinterpret_cast<const rt_cl_triangle*>(in.tris);
        for (int t = 0; t < 2; ++t)
            kill_ok_[t] = rtp::path_kill_scene_ok(recs.data() + (size_t)t * 16 * p.n_mats, p.n_mats, ht, p.n_tris,
                                                  root_bounds());
        kill_known_ = true;
    }
    for_tris_ = tm, tris_gen_ = tm->generation, tris_struct_ = tm->structural;
    for_nodes_ = nm, nodes_gen_ = nm->generation, nodes_struct_ = nm->structural;
    for_mats_ = mm, mats_gen_ = mm ? mm->generation : 0;
    ++full_prepares_;
    return RT_SUCCESS;
}

int DeviceScene::refit(rt_context ctx, rt_mem tm, rt_mem nm, rt_mem mm) {
    if (!structurally_current(tm, nm)) {
        // the full preparation of a launch, which validates as a launch would (the generations may
        // match all the same: after a refit they are the buffers' current ones)
        invalidate();
        const int rc = prepare(ctx, tm, nm, mm);
        if (rc) return rc;
    }
    rtr::RefitArgs a{};
    a.tris = static_cast<const rt_cl_triangle*>(tm->dptr);
    a.n_tris = n_tris_;
    a.nodes = static_cast<rt_cl_bvh_node*>(nm->dptr);
    a.n_nodes = n_nodes_;
    a.parent = refit_links_;
    a.slot = refit_links_ + n_nodes_;
    a.arrivals = refit_arrivals_;
    a.oct = oct_nodes_;
    a.oct_stride = rtp::oct_stride(n_nodes_), a.oct_b = rtp::oct_b(n_nodes_);
    a.goct = goct_b_ ? goct_nodes_ : nullptr;
    a.goct_b = goct_b_, a.goct_group = RT_GOCT_GROUP ? RT_GOCT_GROUP : 1;
    a.g_nodes = g_nodes_;
    root_known_ = false;  // the refit moves the root's bounds on the device
    collapse_known_ = false;  // ... and every box, in the plain records only: equal boxes may now differ
    cull_known_ = false;  // ... and the triangles the octant-cull certificate was evaluated on
    kill_known_ = false;  // ... and reads vertices and normals the host has not seen
    hipStream_t st = qs(ctx);
    hipError_t e = rtr::launch_refit(a, st);
    // the triangle and shading records from the moved vertices; materials stay as packed
    if (e == hipSuccess) e = rtk::launch_pack(a.tris, n_tris_, packed_tris_, shade_tris_, nullptr, 0, shade_mats_, st);
    mark_device_write(nm, false);  // bounds only
    if (e != hipSuccess) {
        invalidate();  // whatever was enqueued, the next launch prepares in full
        return map_hip(e);
    }
    tris_gen_ = tm->generation;
    nodes_gen_ = nm->generation;
    ++refits_;
    return RT_SUCCESS;
}

void DeviceScene::release() {
    for (void* p : {(void*)packed_tris_, (void*)shade_tris_, (void*)shade_mats_, (void*)oct_nodes_, (void*)goct_nodes_,
                    (void*)oct_collapsed_, (void*)goct_collapsed_, (void*)oct_pruned_, (void*)goct_pruned_,
                    (void*)g_nodes_, (void*)refit_links_,
                    (void*)refit_arrivals_})
        if (p) (void)hipFree(p);
    *this = DeviceScene();
}

}  // namespace rti

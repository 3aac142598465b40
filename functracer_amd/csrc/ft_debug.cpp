// ft_debug.cpp — ft_debug_*: explicit ray queries through the device paths and views of the committed scene, for the tests.
#include "ft_context.h"
#include "ft_ls_topology.h"
using namespace ftc;

extern "C" {

// ------------------------------------------------------------------------------------------ debug / tests
// The start of a ray query (ft_debug_closest / ft_debug_blocked): the checks, the device, the rays into d_dbg_in (origins, directions and,
// when `max_dist` is given, the lengths), room for `out_bytes` per ray in d_dbg_out, and the overflow count cleared (in slot 0's counters).
static int32_t debug_rays_in(ft_context* c, const double* origins, const double* dirs, const double* max_dist, int64_t n, size_t out_bytes) {
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    if (!c->committed) { c->err = "scene not committed"; return FT_ERR_STATE; }
    if (n == 0) return FT_OK;
    FT_HIP(c, hipSetDevice(c->device));
    int32_t rc;
    const size_t N = (size_t)n;
    if ((rc = ensure(c, c->d_dbg_in, N * (max_dist ? 56 : 48))) != FT_OK) return rc;
    if ((rc = ensure(c, c->d_dbg_out, N * out_bytes)) != FT_OK) return rc;
    double* din = c->d_dbg_in.as<double>();
    FT_HIP(c, hipMemcpyAsync(din, origins, N * 24, hipMemcpyHostToDevice, c->stream));
    FT_HIP(c, hipMemcpyAsync(din + 3 * N, dirs, N * 24, hipMemcpyHostToDevice, c->stream));
    if (max_dist) FT_HIP(c, hipMemcpyAsync(din + 6 * N, max_dist, N * 8, hipMemcpyHostToDevice, c->stream));
    c->slots[0].fc_clean = false;
    FT_HIP(c, hipMemsetAsync(c->slots[0].d_fc.p, 0, sizeof(unsigned long long), c->stream));   // the overflow count of this query
    return FT_OK;
}
// ... and its end, behind the copies of the results: the overflow count read back, the stream synchronised.
static int32_t debug_rays_done(ft_context* c) {
    unsigned long long n_overflow = 0;
    FT_HIP(c, hipMemcpyAsync(&n_overflow, c->slots[0].d_fc.p, sizeof n_overflow, hipMemcpyDeviceToHost, c->stream));
    FT_HIP(c, hipStreamSynchronize(c->stream));
    if (n_overflow) { c->err = "CSG hit list overflow"; return FT_ERR_OVERFLOW; }
    return FT_OK;
}

static int32_t debug_closest(ft_context* c, const double* origins, const double* dirs, int64_t n, int32_t* hit, double* t, double* p, double* nrm, double* colour) {
    if (!c || !origins || !dirs || n < 0 || !hit || !t || !p || !nrm || !colour) return FT_ERR_INVALID;
    int32_t rc = debug_rays_in(c, origins, dirs, nullptr, n, 4 + 8 + 72);
    if (rc != FT_OK || n == 0) return rc;
    const size_t N = (size_t)n;
    double* din = c->d_dbg_in.as<double>();
    double* dt = c->d_dbg_out.as<double>();
    double* dp = dt + N; double* dn = dp + 3 * N; double* dc = dn + 3 * N;
    int32_t* dh = reinterpret_cast<int32_t*>(dc + 3 * N);
    ftk::Launch L{c->stream, c->n_cu * 4, lds_bytes_for(c->flat), 0};
    ftk::launch_debug_closest(L, c->dev_scene, din, din + 3 * N, (uint32_t)n, dh, dt, dp, dn, dc, c->slots[0].d_fc.as<unsigned long long>());
    FT_HIP(c, hipGetLastError());
    FT_HIP(c, hipMemcpyAsync(t, dt, N * 8, hipMemcpyDeviceToHost, c->stream));
    FT_HIP(c, hipMemcpyAsync(p, dp, N * 24, hipMemcpyDeviceToHost, c->stream));
    FT_HIP(c, hipMemcpyAsync(nrm, dn, N * 24, hipMemcpyDeviceToHost, c->stream));
    FT_HIP(c, hipMemcpyAsync(colour, dc, N * 24, hipMemcpyDeviceToHost, c->stream));
    FT_HIP(c, hipMemcpyAsync(hit, dh, N * 4, hipMemcpyDeviceToHost, c->stream));
    return debug_rays_done(c);
}
int32_t ft_debug_closest(ft_context* c, const double* origins, const double* dirs, int64_t n, int32_t* hit, double* t, double* p, double* nrm, double* colour) {
    if (!c) return FT_ERR_INVALID;
    return with_growing_hit_lists(c, [&] { return debug_closest(c, origins, dirs, n, hit, t, p, nrm, colour); });
}

static int32_t debug_blocked(ft_context* c, const double* origins, const double* dirs, const double* max_dist, int64_t n, int32_t* blocked) {
    if (!c || !origins || !dirs || !max_dist || n < 0 || !blocked) return FT_ERR_INVALID;
    int32_t rc = debug_rays_in(c, origins, dirs, max_dist, n, 4);
    if (rc != FT_OK || n == 0) return rc;
    const size_t N = (size_t)n;
    double* din = c->d_dbg_in.as<double>();
    ftk::Launch L{c->stream, c->n_cu * 4, lds_bytes_for(c->flat), 0};
    ftk::launch_debug_blocked(L, c->dev_scene, din, din + 3 * N, din + 6 * N, (uint32_t)n, c->d_dbg_out.as<int32_t>(), c->slots[0].d_fc.as<unsigned long long>());
    FT_HIP(c, hipGetLastError());
    FT_HIP(c, hipMemcpyAsync(blocked, c->d_dbg_out.p, N * 4, hipMemcpyDeviceToHost, c->stream));
    return debug_rays_done(c);
}
int32_t ft_debug_blocked(ft_context* c, const double* origins, const double* dirs, const double* max_dist, int64_t n, int32_t* blocked) {
    if (!c) return FT_ERR_INVALID;
    return with_growing_hit_lists(c, [&] { return debug_blocked(c, origins, dirs, max_dist, n, blocked); });
}

// getColourForRay (Shading.fs:131-139) for explicit rays through the device path: the rays enter k_bounce as level 0 with weight 1
// and are followed to their end, so closest hit, shadow queries, shaders and up to max_depth reflection bounces run exactly as they
// do for a frame's samples.  Streams of soft lights are keyed with seed 0 and sample = ray index.
static int32_t debug_colour(ft_context* c, const double* origins, const double* dirs, int64_t n, int32_t max_depth, double* rgb) {
    if (!c || !origins || !dirs || n < 0 || !rgb || max_depth < 0) return FT_ERR_INVALID;
    if (max_depth > ftk::kMaxBounce) { c->err = "max_depth above 16"; return FT_ERR_UNSUPPORTED; }
    if (n >= (1ll << 30)) return FT_ERR_INVALID;
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    if (!c->committed) { c->err = "scene not committed"; return FT_ERR_STATE; }
    if (n == 0) return FT_OK;
    FT_HIP(c, hipSetDevice(c->device));
    int32_t rc;
    if ((rc = ensure_frame_buffers(c, n, true)) != FT_OK) return rc;
    const size_t N = (size_t)n, cap = (size_t)c->ray_capacity;
    std::vector<double> soa(7 * N);
    std::vector<uint32_t> slot(N);
    for (size_t i = 0; i < N; ++i) {
        for (int k = 0; k < 3; ++k) { soa[(size_t)k * N + i] = origins[3 * i + k]; soa[(size_t)(3 + k) * N + i] = dirs[3 * i + k]; }
        soa[6 * N + i] = 1.0; slot[i] = (uint32_t)i;
    }
    auto* fc = c->slots[0].d_fc.as<ftk::FrameCounters>();
    c->slots[0].fc_clean = false;
    FT_HIP(c, hipMemsetAsync(fc, 0, sizeof(ftk::FrameCounters), c->stream));
    const ftk::RayBuf rb0 = ray_view(c->d_rays[0], c->ray_capacity), rb1 = ray_view(c->d_rays[1], c->ray_capacity);
    for (int k = 0; k < 7; ++k) FT_HIP(c, hipMemcpyAsync(c->d_rays[0].as<double>() + (size_t)k * cap, soa.data() + (size_t)k * N, N * 8, hipMemcpyHostToDevice, c->stream));
    FT_HIP(c, hipMemcpyAsync(rb0.slot, slot.data(), N * 4, hipMemcpyHostToDevice, c->stream));
    const uint32_t n_rays = (uint32_t)n;
    FT_HIP(c, hipMemcpyAsync(&fc->cc.n_rays[0], &n_rays, 4, hipMemcpyHostToDevice, c->stream));
    FT_HIP(c, hipMemsetAsync(c->d_acc[0].p, 0, 3 * N * 8, c->stream));
    const size_t lds = lds_bytes_for(c->flat);
    ftk::Launch Lt{c->stream, c->n_cu * c->blocks_bounce, lds, c->variant};
    ftk::Primary gen{};
    gen.pixel_ids = nullptr; gen.pix_base = 0; gen.n_pix = n_rays; gen.spp = 1; gen.inv_n_pix = 1.0 / (double)n_rays; gen.seed = 0ull; gen.counts = nullptr; gen.block_map = nullptr;
    ftk::launch_bounce(Lt, c->dev_scene, gen, rb0, rb1, c->d_acc[0].as<double>(), n_rays, 0, max_depth, true, fc);   // level 0, followed to the end
    FT_HIP(c, hipGetLastError());
    std::vector<double> planes(3 * N);
    FT_HIP(c, hipMemcpyAsync(planes.data(), c->d_acc[0].p, 3 * N * 8, hipMemcpyDeviceToHost, c->stream));
    struct { ftk::RenderCounters stats[ftk::kStatStripes]; } tail;
    FT_HIP(c, hipMemcpyAsync(&tail, &fc->stats[0], sizeof tail, hipMemcpyDeviceToHost, c->stream));
    FT_HIP(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < N; ++i) { rgb[3 * i] = planes[i]; rgb[3 * i + 1] = planes[N + i]; rgb[3 * i + 2] = planes[2 * N + i]; }
    unsigned long long ovf = 0;
    for (int k = 0; k < ftk::kStatStripes; ++k) ovf += tail.stats[k].csg_overflow;
    if (ovf) { c->err = "CSG hit list overflow"; return FT_ERR_OVERFLOW; }
    return FT_OK;
}
int32_t ft_debug_colour(ft_context* c, const double* origins, const double* dirs, int64_t n, int32_t max_depth, double* rgb) {
    if (!c) return FT_ERR_INVALID;
    return with_growing_hit_lists(c, [&] { return debug_colour(c, origins, dirs, n, max_depth, rgb); });
}

/* Diagnostic builds (-DFT_STAMPS): the s_memrealtime stamps k_classify's workgroups left behind (8 per workgroup). */
int32_t ft_debug_classify_stamps(ft_context* c, unsigned long long* out, int32_t n_groups) {
    if (!c || !out || n_groups < 1 || n_groups > 2048 || !c->d_wave_counts.p) return FT_ERR_INVALID;
    if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return FT_ERR_HIP;
    return hipMemcpy(out, c->d_wave_counts.as<uint32_t>() + 4096, (size_t)n_groups * 64, hipMemcpyDeviceToHost) == hipSuccess ? FT_OK : FT_ERR_HIP;
}

int32_t ft_debug_scene_info(ft_context* c, int64_t out[12]) {
    if (!c || !out) return FT_ERR_INVALID;
    if (!c->committed) { c->err = "scene not committed"; return FT_ERR_STATE; }
    const fth::FlatScene& f = c->flat;
    out[0] = (int64_t)f.leaves.size(); out[1] = (int64_t)f.program.size(); out[2] = (int64_t)f.meshes.size(); out[3] = (int64_t)f.nodes.size() - f.bvh_nodes;
    out[4] = (int64_t)f.bsp_leaves.size() - f.bvh_leaves; out[5] = (int64_t)(f.tris.size() / 9) - f.bvh_tris; out[6] = f.csg_capacity; out[7] = f.bsp_stack_capacity;   // BSP-only: excludes the device-side BVH
    int64_t bounded = 0; for (size_t k = 0; k + 1 < f.item_pc.size(); ++k) if (f.cull_items[8 * k + 3] < 1e30f) ++bounded;
    out[8] = (int64_t)f.item_pc.size() - 1; out[9] = bounded; out[10] = f.unbounded ? 1 : 0; out[11] = f.cull_bundle ? (int64_t)(f.cull_rows.size() / 3) : -1;
    return FT_OK;
}

// The per-leaf matrices of the scene the context holds (the last successful commit's, also while the graph is being edited): 12
// doubles each, rows of the 3x4 model->world and world->model matrices.
int32_t ft_debug_leaf_matrices(ft_context* c, int64_t* n_leaves, double* m2w, double* w2m) {
    if (!c || !n_leaves) return FT_ERR_INVALID;
    if (!c->holds_commit) { c->err = "scene not committed"; return FT_ERR_STATE; }
    const fth::FlatScene& f = c->flat;
    *n_leaves = (int64_t)f.leaves.size();
    if (m2w) std::memcpy(m2w, f.m2w.data(), f.leaves.size() * 12 * sizeof(double));
    if (w2m) for (size_t k = 0; k < f.leaves.size(); ++k) std::memcpy(w2m + 12 * k, f.leaves[k].w2m, sizeof f.leaves[k].w2m);
    return FT_OK;
}

int32_t ft_debug_light_space(ft_context* c, int64_t sizes[4], double* pairs, uint32_t* nodes, double* tris, uint32_t* leaf_pairs) {
    if (!c || !sizes) return FT_ERR_INVALID;
    if (!c->committed) { c->err = "scene not committed"; return FT_ERR_STATE; }
    const fth::FlatScene& f = c->flat;
    sizes[0] = (int64_t)(f.ls_pairs.size() / ftd::kLsPairDoubles); sizes[1] = (int64_t)(f.ls_nodes.size() / ftd::kLsNodeWords);
    sizes[2] = (int64_t)(f.ls_tris.size() / 9); sizes[3] = (int64_t)f.leaves.size();
    if (!c->host_only && c->lightspace.rewritten) {
        // an ft_scene_commit_lights has rewritten trees and grids in HBM since the full commit: the arrays as they lie there, at the
        // sizes they have there (as ft_debug_mesh_trees)
        const ft_context::LightSpace& L = c->lightspace;
        sizes[1] = (int64_t)(L.node_words / ftd::kLsNodeWords); sizes[2] = (int64_t)(L.tri_doubles / 9);
        FT_HIP(c, hipSetDevice(c->device));
        const int32_t rc = drain_frame_streams(c);
        if (rc != FT_OK) return rc;
        const DeviceBuf* B = c->d_scene;
        if (B[kLsPairs].bytes < f.ls_pairs.size() * 8 || B[kLsNodes].bytes < L.node_words * 4 || B[kLsTris].bytes < L.tri_doubles * 8) {
            c->err = "ft_debug_light_space: a light-space array in device memory is smaller than recorded"; return FT_ERR_STATE;
        }
        if (pairs) FT_HIP(c, hipMemcpy(pairs, B[kLsPairs].p, f.ls_pairs.size() * sizeof(double), hipMemcpyDeviceToHost));
        if (nodes) FT_HIP(c, hipMemcpy(nodes, B[kLsNodes].p, L.node_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (tris) FT_HIP(c, hipMemcpy(tris, B[kLsTris].p, L.tri_doubles * sizeof(double), hipMemcpyDeviceToHost));
    } else {
        if (pairs) std::memcpy(pairs, f.ls_pairs.data(), f.ls_pairs.size() * sizeof(double));
        if (nodes) std::memcpy(nodes, f.ls_nodes.data(), f.ls_nodes.size() * sizeof(uint32_t));
        if (tris) std::memcpy(tris, f.ls_tris.data(), f.ls_tris.size() * sizeof(double));
    }
    if (leaf_pairs) for (size_t k = 0; k < f.leaves.size(); ++k) leaf_pairs[k] = f.leaves[k].ls_pairs;
    return FT_OK;
}

// "light_space_retree": the pairs' table as the last ft_scene_commit_lights / ft_scene_commit_deformed left it.
int32_t ft_debug_ls_retree(ft_context* c, int64_t* n_pairs, int64_t* rows, double* R) {
    if (!c || !n_pairs) return FT_ERR_INVALID;
    if (c->host_only) return FT_ERR_NO_DEVICE;
    const ft_context::LightSpace& T = c->lightspace;
    *n_pairs = T.ready ? (int64_t)T.pairs.size() : 0;
    for (int64_t k = 0; k < *n_pairs; ++k) {
        const ft_context::LightSpace::Pair& P = T.pairs[(size_t)k];
        if (rows) {
            int64_t* r = rows + 8 * k;
            r[0] = P.rec; r[1] = P.leaf; r[2] = P.light; r[3] = P.n_tris; r[4] = P.ls_first == ~0u ? -1 : (int64_t)P.ls_first;
            r[5] = P.retreed ? 1 : 0; r[6] = P.block == ~0u ? -1 : (int64_t)P.block; r[7] = P.block_nodes;
        }
        if (R) R[k] = P.R;
    }
    return FT_OK;
}

// The host half of "light_space_retree" (ft_ls_topology.h), context-free.
int32_t ft_debug_ls_topology(int64_t n, int64_t ls_first, int64_t first_node, int64_t sizes[2], uint32_t* child, uint32_t* order, uint32_t* levels) {
    if (!sizes || n < 0 || ls_first < 0 || first_node < 0 || n > 0xFFFFFFFFll || ls_first > 0xFFFFFFFFll || first_node > 0xFFFFFFFFll) return FT_ERR_INVALID;
    fth::LsTopology topo;
    if (!fth::ls_retree_topology((uint32_t)n, (uint32_t)ls_first, (uint32_t)first_node, topo)) return FT_ERR_INVALID;
    const size_t N = topo.nodes.size() / fth::kLsTopoNodeWords;
    sizes[0] = (int64_t)N; sizes[1] = (int64_t)topo.levels.size();
    if (child) for (size_t k = 0; k < N; ++k) std::memcpy(child + 4 * k, &topo.nodes[k * fth::kLsTopoNodeWords + 20], 16);
    if (order) std::memcpy(order, topo.order.data(), N * 4);
    if (levels) for (size_t k = 0; k < topo.levels.size(); ++k) { levels[2 * k] = topo.levels[k].first; levels[2 * k + 1] = topo.levels[k].second; }
    return FT_OK;
}

// The mesh trees as they lie in HBM after the last commit (device contexts: copied back from device memory, so what ft_bvh.hip built
// into the ranges the flattener reserved is seen; host-only contexts: the flattened arrays), and the host-side tables needed to walk them.
int32_t ft_debug_mesh_trees(ft_context* c, int64_t sizes[12], void* nodes, uint32_t* bsp_leaves, double* tris, uint32_t* tri_orig, uint32_t* tri_src, double* wide,
                            float* coarse_boxes, int32_t* meshes, uint32_t* jobs) {
    if (!c || !sizes) return FT_ERR_INVALID;
    if (!c->committed) { c->err = "scene not committed"; return FT_ERR_STATE; }
    const fth::FlatScene& f = c->flat;
    sizes[0] = (int64_t)f.nodes.size(); sizes[1] = (int64_t)f.bsp_leaves.size(); sizes[2] = (int64_t)(f.tris.size() / 9); sizes[3] = (int64_t)f.tri_orig.size();
    sizes[4] = (int64_t)f.tri_src.size(); sizes[5] = (int64_t)(f.wide.size() / ftd::kWideNodeDoubles); sizes[6] = (int64_t)(f.coarse_boxes.size() / 6);
    sizes[7] = (int64_t)f.meshes.size(); sizes[8] = (int64_t)f.bvh_jobs.size(); sizes[9] = c->host_only ? f.stack_capacity : c->dev_scene.stack_cap;
    sizes[10] = c->host_only ? 0 : 1; sizes[11] = 0;
    if (!c->host_only) {
        FT_HIP(c, hipSetDevice(c->device));
        const int32_t rc = drain_frame_streams(c);
        if (rc != FT_OK) return rc;
    }
    auto get = [&](void* dst, SceneArray k, const void* host, size_t bytes) -> int32_t {
        if (!dst || bytes == 0) return FT_OK;
        if (c->host_only) { std::memcpy(dst, host, bytes); return FT_OK; }
        const DeviceBuf& b = geo_array(c, k);                       // (the live geometry set's where a refit rewrites the array)
        if (b.bytes < bytes) { c->err = "ft_debug_mesh_trees: a scene array in device memory is smaller than the flattened one"; return FT_ERR_STATE; }
        FT_HIP(c, hipMemcpy(dst, b.p, bytes, hipMemcpyDeviceToHost));
        return FT_OK;
    };
    int32_t rc;
    if ((rc = get(nodes, kNodes, f.nodes.data(), f.nodes.size() * sizeof(ftd::BspNode))) != FT_OK) return rc;
    if ((rc = get(bsp_leaves, kBspLeaves, f.bsp_leaves.data(), f.bsp_leaves.size() * sizeof(ftd::BspLeaf))) != FT_OK) return rc;
    if ((rc = get(tris, kTris, f.tris.data(), f.tris.size() * sizeof(double))) != FT_OK) return rc;
    if ((rc = get(tri_orig, kTriOrig, f.tri_orig.data(), f.tri_orig.size() * sizeof(uint32_t))) != FT_OK) return rc;
    if ((rc = get(tri_src, kTriSrc, f.tri_src.data(), f.tri_src.size() * sizeof(uint32_t))) != FT_OK) return rc;
    if ((rc = get(wide, kWide, f.wide.data(), f.wide.size() * sizeof(double))) != FT_OK) return rc;
    if ((rc = get(coarse_boxes, kCoarse, f.coarse_boxes.data(), f.coarse_boxes.size() * sizeof(float))) != FT_OK) return rc;
    if (meshes) for (size_t m = 0; m < f.meshes.size(); ++m) {
        int32_t* r = meshes + 6 * m;
        r[0] = f.meshes[m].root; r[1] = f.meshes[m].bvh_root; r[2] = (int32_t)f.meshes[m].n_source_tris; r[3] = f.mesh_wide[m];
        r[4] = (int32_t)f.mesh_coarse[2 * m]; r[5] = (int32_t)f.mesh_coarse[2 * m + 1];
    }
    static_assert(sizeof(fth::FlatScene::BvhJob) == 9 * sizeof(uint32_t), "a job goes out as nine words");
    if (jobs && !f.bvh_jobs.empty()) std::memcpy(jobs, f.bvh_jobs.data(), f.bvh_jobs.size() * sizeof(fth::FlatScene::BvhJob));
    return FT_OK;
}

// The candidate lists of the last frame queued if it was classified (none otherwise), as k_block_lists left them in its slot (the frame's counters are gone by
// then: the active block count comes from its report, the entries in use from the headers).
int32_t ft_debug_block_lists(ft_context* c, int64_t sizes[4], double plane[4], uint32_t* heads, uint32_t* pos_block, uint32_t* entries) {
    if (!c || !sizes) return FT_ERR_INVALID;
    if (c->host_only) return FT_ERR_NO_DEVICE;
    sizes[0] = sizes[1] = sizes[3] = 0; sizes[2] = -1;
    if (c->last_classified_slot < 0) return FT_OK;
    FT_HIP(c, hipSetDevice(c->device));
    int32_t rc = retire_queued(c);
    if (rc != FT_OK) return rc;
    if ((rc = drain_frame_streams(c)) != FT_OK) return rc;
    const ft_context::FrameSlot& F = c->slots[c->last_classified_slot];
    if (F.list_leaf < 0 || !F.h_report) return FT_OK;
    const size_t n_active = std::min<size_t>(F.h_report->n_pix_active / 64u, F.d_list_heads.bytes / 4);
    std::vector<uint32_t> h(n_active);
    if (n_active) FT_HIP(c, hipMemcpy(h.data(), F.d_list_heads.p, n_active * 4, hipMemcpyDeviceToHost));
    size_t used = 0;
    for (uint32_t v : h) if (v != ftk::kListNone) used = std::max<size_t>(used, (size_t)(v >> 7) + (v & 127u));
    const size_t cap = F.d_list_pool.bytes / (ftk::kListEntryWords * 4);
    if (used > cap) { c->err = "ft_debug_block_lists: a header points past the pool"; return FT_ERR_STATE; }
    sizes[0] = (int64_t)n_active; sizes[1] = (int64_t)used; sizes[2] = F.list_leaf; sizes[3] = (int64_t)cap;
    if (plane) { plane[0] = F.list_cam.tlx; plane[1] = F.list_cam.tly; plane[2] = F.list_cam.pw; plane[3] = F.list_cam.ph; }
    if (heads && n_active) std::memcpy(heads, h.data(), n_active * 4);
    if (pos_block && n_active) FT_HIP(c, hipMemcpy(pos_block, F.d_pos_block.p, n_active * 4, hipMemcpyDeviceToHost));
    if (entries && used) FT_HIP(c, hipMemcpy(entries, F.d_list_pool.p, used * ftk::kListEntryWords * 4, hipMemcpyDeviceToHost));
    return FT_OK;
}

// The edge records (ft_edges.h) beside the arrays ft_debug_light_space and ft_debug_block_lists hand out, under the same indices.
int32_t ft_debug_edge_records(ft_context* c, int64_t sizes[2], float* grid_edges, float* list_edges) {
    if (!c || !sizes) return FT_ERR_INVALID;
    if (c->host_only) return FT_ERR_NO_DEVICE;
    sizes[0] = sizes[1] = 0;
    FT_HIP(c, hipSetDevice(c->device));
    int32_t rc = retire_queued(c);
    if (rc != FT_OK) return rc;
    if ((rc = drain_frame_streams(c)) != FT_OK) return rc;
    const size_t rec_bytes = ftk::kEdgeFloats * sizeof(float);
    if (c->committed && c->lightspace.d_edges.p) {
        const size_t n_recs = (c->lightspace.rewritten ? c->lightspace.tri_doubles : c->flat.ls_tris.size()) / 9;
        if (c->lightspace.d_edges.bytes < n_recs * rec_bytes) { c->err = "ft_debug_edge_records: the edge array in device memory is smaller than recorded"; return FT_ERR_STATE; }
        sizes[0] = (int64_t)n_recs;
        if (grid_edges && n_recs) FT_HIP(c, hipMemcpy(grid_edges, c->lightspace.d_edges.p, n_recs * rec_bytes, hipMemcpyDeviceToHost));
    }
    if (c->last_classified_slot < 0) return FT_OK;
    const ft_context::FrameSlot& F = c->slots[c->last_classified_slot];
    if (F.list_leaf < 0 || !F.h_report) return FT_OK;
    const size_t n_active = std::min<size_t>(F.h_report->n_pix_active / 64u, F.d_list_heads.bytes / 4);
    std::vector<uint32_t> h(n_active);
    if (n_active) FT_HIP(c, hipMemcpy(h.data(), F.d_list_heads.p, n_active * 4, hipMemcpyDeviceToHost));
    size_t used = 0;
    for (uint32_t v : h) if (v != ftk::kListNone) used = std::max<size_t>(used, (size_t)(v >> 7) + (v & 127u));
    if (used * rec_bytes > F.d_list_edges.bytes) { c->err = "ft_debug_edge_records: a header points past the edge pool"; return FT_ERR_STATE; }
    sizes[1] = (int64_t)used;
    if (list_edges && used) FT_HIP(c, hipMemcpy(list_edges, F.d_list_edges.p, used * rec_bytes, hipMemcpyDeviceToHost));
    return FT_OK;
}

// What the frame driver did with the classifications and windows of the frames queued since ft_create, summed over the context's devices.
int32_t ft_debug_classify_reuse(ft_context* c, int64_t out[4]) {
    if (!c || !out) return FT_ERR_INVALID;
    if (c->host_only) return FT_ERR_NO_DEVICE;
    for (int k = 0; k < 4; ++k) out[k] = 0;
    for (const ft_context* d : devices(c)) for (int k = 0; k < 4; ++k) out[k] += d->reuse_counts[k];
    return FT_OK;
}

// What the queued pose and light commits did since ft_create (ft_context::PoseSets::counts), and the pose sets the first device holds.
int32_t ft_debug_pose_queue(ft_context* c, int64_t out[8]) {
    if (!c || !out) return FT_ERR_INVALID;
    for (int k = 0; k < 8; ++k) out[k] = c->pose.counts[k];
    out[6] = c->host_only ? 0 : std::max<int64_t>(1, (int64_t)c->pose.sets.size());
    return FT_OK;
}

// What the queued deform commits did since ft_create (ft_context::GeoSets::counts), and the geometry sets the first device holds.
int32_t ft_debug_deform_queue(ft_context* c, int64_t out[8]) {
    if (!c || !out) return FT_ERR_INVALID;
    for (int k = 0; k < 8; ++k) out[k] = c->geo.counts[k];
    out[3] = c->host_only ? 0 : std::max<int64_t>(1, (int64_t)c->geo.sets.size());
    out[7] = 0;
    return FT_OK;
}

// Which kernel the bounce-0 launches of the frames queued since ft_create went to: k_primary, k_primary_mesh.
int32_t ft_debug_primary_kernels(ft_context* c, int64_t out[2]) {
    if (!c || !out) return FT_ERR_INVALID;
    if (c->host_only) return FT_ERR_NO_DEVICE;
    out[0] = out[1] = 0;
    for (const ft_context* d : devices(c)) for (int k = 0; k < 2; ++k) out[k] += d->primary_launches[k];
    return FT_OK;
}

int32_t ft_debug_slice(const double p0[3], const double n[3], const double tri[9], double above[18], int32_t* n_above, double below[18], int32_t* n_below) {
    if (!p0 || !n || !tri || !above || !below || !n_above || !n_below) return FT_ERR_INVALID;
    std::vector<double> a, b; std::string err;
    int32_t rc = fth::slice_triangle(p0, n, tri, a, b, err);
    if (rc != FT_OK) return rc;
    *n_above = (int32_t)(a.size() / 9); *n_below = (int32_t)(b.size() / 9);
    if (!a.empty()) std::memcpy(above, a.data(), a.size() * 8);
    if (!b.empty()) std::memcpy(below, b.data(), b.size() * 8);
    return FT_OK;
}

int32_t ft_debug_devices(ft_context* c, int32_t* ordinals, int32_t capacity) {   // the device ordinals behind a context, in order; returns how many
    if (!c || capacity < 0 || (capacity > 0 && !ordinals)) return FT_ERR_INVALID;
    if (c->host_only) return 0;
    int32_t n = 0;
    if (n < capacity) ordinals[n] = c->device;
    ++n;
    for (ft_context* p : c->peers) { if (n < capacity) ordinals[n] = p->device; ++n; }
    return n;
}

} // extern "C"

// ft_capi.cpp — the C ABI of libfunctracer_hip.so (include/functracer_hip.h): context, scene
// builder, options, commit and HBM residency of the flattened scene, and the frame's way out of HBM.  The frame driver is ft_frame.cpp,
// the features over it ft_progressive.cpp and ft_passes.cpp, the test entry points ft_debug.cpp.
// Reference citations are relative to FuncTracer/ of the reference (antonburger/FuncTracer).
#include <map>

#include "ft_context.h"
#include "ft_ls_topology.h"
#include "ft_refit_cost.h"

namespace ftc {

bool need_device(ft_context* c) {
    if (!c) return false;
    if (c->host_only) { c->err = "host-only context: no HIP device bound (there is no CPU fallback for rendering)"; return false; }
    return true;
}

bool need_committed(ft_context* c) {
    if (!c->committed) c->err = "scene not committed (ft_scene_commit)";
    return c->committed;
}

static void norm3(double v[3]) {                                           // Vector.normalise (CommonTypes.fs:63-67)
    double l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (!(l < 0.0000001)) { double s = 1.0 / l; v[0] = s * v[0]; v[1] = s * v[1]; v[2] = s * v[2]; }
}
// ImagePlane.create (Image.fs:48-53, 67-81), evaluated once per frame on the host.
ftk::Camera make_camera(const ft_camera& cam, int res_h, int res_v) {
    ftk::Camera out{};
    double k[3] = {cam.look_at[0] - cam.o[0], cam.look_at[1] - cam.o[1], cam.look_at[2] - cam.o[2]};
    norm3(k);
    const double* u = cam.up;
    double i[3] = {u[1] * k[2] - u[2] * k[1], k[0] * u[2] - k[2] * u[0], u[0] * k[1] - u[1] * k[0]};     // up .** k
    norm3(i);
    double j[3] = {k[1] * i[2] - k[2] * i[1], i[0] * k[2] - i[2] * k[0], k[0] * i[1] - k[1] * i[0]};     // k .** i
    const double height = std::tan(cam.fov_y / 2.0) * 2.0;
    const double width = height * cam.aspect_ratio;
    const double pixel_height = height / (double)(res_h - 1);      // sic, Image.fs:71: resH
    const double pixel_width = width / (double)(res_v - 1);        // sic, Image.fs:72: resV
    for (int a = 0; a < 3; ++a) { out.o[a] = cam.o[a]; out.k[a] = k[a]; out.i[a] = i[a]; out.j[a] = j[a]; }
    out.pw = pixel_width; out.ph = pixel_height;
    out.tlx = -width / 2.0 + pixel_width / 2.0; out.tly = height / 2.0 - pixel_height / 2.0;
    out.res_h = res_h; out.res_v = res_v;
    out.has_focus = cam.has_focus ? 1 : 0; out.focal_length = cam.focal_length;
    out.tan_half_aperture = std::tan(cam.aperture_angular_size / 2.0);          // Jitter.fs:30
    return out;
}

// LDS per workgroup: the per-lane CSG hit lists (4 words per entry) and tree stacks.  When the lists alone would not fit, lanes are
// folded (ft_kernels.hip, HitList): fold live lanes share the columns of 64 lanes, so a column needs only ceil(capacity / fold) rows.
constexpr size_t kLdsPerWorkgroup = 160 * 1024;
static size_t lds_bytes_at(const fth::FlatScene& f, int fold) {
    const size_t rows = ((size_t)f.csg_capacity + (size_t)fold - 1) / (size_t)fold;
    return (4 * rows + (size_t)f.stack_capacity) * ftk::kBlock * 4;
}
static int lane_fold_for(const fth::FlatScene& f) {
    for (int fold = 1; fold <= 16; fold *= 2) if (lds_bytes_at(f, fold) <= kLdsPerWorkgroup) return fold;
    return 0;
}
// Materials only the FANCY kernel variants shade: Oren-Nayar, textures, and a specular exponent that is not a small whole number
// (ftd::small_whole_exponent: the lean variants do not carry Math.Pow).
static bool needs_fancy(const ftd::Material& m) {
    return m.roughness != 0.0 || m.texture >= 0 || (m.shineyness > 0.0 && !ftd::small_whole_exponent(m.shineyness)) || m.shineyness != m.shineyness;
}
// The context's devices: itself, then its peers.
std::vector<ft_context*> devices(ft_context* c) {
    std::vector<ft_context*> devs{c};
    devs.insert(devs.end(), c->peers.begin(), c->peers.end());
    return devs;
}
// Waits for everything that may still write the frame in HBM: frames queued with ft_render_enqueue may be running on any main stream
// (the streams are non-blocking), their k_resolve on its own stream.
int32_t drain_frame_streams(ft_context* c) {
    FT_HIP(c, hipStreamSynchronize(c->stream));
    for (hipStream_t m : c->more_mains) if (m) FT_HIP(c, hipStreamSynchronize(m));
    FT_HIP(c, hipStreamSynchronize(c->tail));
    if (c->geo.deform) FT_HIP(c, hipStreamSynchronize(c->geo.deform));   // a queued refit may still write the live geometry set
    return FT_OK;
}
size_t lds_bytes_for(const fth::FlatScene& f) { return lds_bytes_at(f, std::max(1, lane_fold_for(f))); }

} // namespace ftc
using namespace ftc;

extern "C" {

int32_t ft_abi_version(void) { return FT_ABI_VERSION; }

static int32_t create_single(int32_t device_id, int count, ft_context** out) {
    if (device_id < 0 || device_id >= count) return FT_ERR_INVALID;
    ft_context* c = new ft_context();
    c->device = device_id;
    hipDeviceProp_t prop;
    if (hipSetDevice(c->device) != hipSuccess || hipGetDeviceProperties(&prop, c->device) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return FT_ERR_HIP; }
    int pr_low = 0, pr_high = 0;                                   // the side stream's few workgroups go first whenever slots come free
    if (hipDeviceGetStreamPriorityRange(&pr_low, &pr_high) != hipSuccess) pr_high = 0;
    if (hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, pr_high) != hipSuccess || hipStreamCreateWithPriority(&c->tail, hipStreamNonBlocking, pr_high) != hipSuccess) {
        if (c->side) (void)hipStreamDestroy(c->side);
        (void)hipStreamDestroy(c->stream); delete c; return FT_ERR_HIP;
    }
    for (hipStream_t& m : c->more_mains) if (hipStreamCreateWithFlags(&m, hipStreamNonBlocking) != hipSuccess) { m = nullptr; c->opt.mains = 1; }   // (without them every frame takes the one main stream)
    c->n_cu = prop.multiProcessorCount;
    *out = c;
    return FT_OK;
}

int32_t ft_create(const int32_t* device_ids, int32_t n_devices, ft_context** out) {
    if (!out) return FT_ERR_INVALID;
    *out = nullptr;
    if (n_devices < 1 || !device_ids) return FT_ERR_NO_DEVICE;     // no CPU backend exists in this library
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return FT_ERR_NO_DEVICE;
    ft_context* c = nullptr;
    int32_t rc = create_single(device_ids[0], count, &c);
    if (rc != FT_OK) return rc;
    // More devices: the scene is replicated and every frame is split into 8-row bands dealt round-robin (no exchange
    // between devices; the bands meet in the caller's host buffer).  The same ordinal may be listed twice.
    for (int32_t k = 1; k < n_devices; ++k) {
        ft_context* p = nullptr;
        rc = create_single(device_ids[k], count, &p);
        if (rc != FT_OK) { ft_destroy(c); return rc; }
        c->peers.push_back(p);
        DeviceWorker* w = new DeviceWorker();
        w->start();
        c->workers.push_back(w);
    }
    *out = c;
    return FT_OK;
}

int32_t ft_create_host_only(ft_context** out) {
    if (!out) return FT_ERR_INVALID;
    ft_context* c = new ft_context();
    c->host_only = true;
    *out = c;
    return FT_OK;
}

void ft_destroy(ft_context* c) {
    if (!c) return;
    for (DeviceWorker* w : c->workers) { w->stop(); delete w; }
    c->workers.clear();
    for (ft_context* p : c->peers) ft_destroy(p);
    c->peers.clear();
    if (!c->host_only) {
        (void)hipSetDevice(c->device);
        (void)drain_frame_streams(c);
        if (c->side) (void)hipStreamSynchronize(c->side);
        if (c->pose.copies) (void)hipStreamSynchronize(c->pose.copies);
        c->pose.release();
        c->geo.release();
        for (DeviceBuf& b : c->d_scene) b.release();
        for (DeviceBuf& b : c->d_rays) b.release();
        for (DeviceBuf& b : c->d_acc) b.release();
        for (DeviceBuf* b : {&c->d_out, &c->d_out8, &c->d_out_index, &c->d_pixels, &c->d_jitter, &c->d_wave_counts, &c->d_dbg_in, &c->d_dbg_out}) b->release();
        for (auto& f : c->slots) f.release();
        c->prog.release(); c->aov.release(); c->denoise.release(); c->temporal.release(); c->refit.release(); c->morph.release(); c->skin.release(); c->lightspace.release();   // what the features own
        if (c->classified) (void)hipEventDestroy(c->classified);
        for (hipEvent_t& e : c->acc_free) if (e) { (void)hipEventDestroy(e); e = nullptr; }
        if (c->side) (void)hipStreamDestroy(c->side);
        if (c->tail) (void)hipStreamDestroy(c->tail);
        for (hipStream_t m : c->more_mains) if (m) (void)hipStreamDestroy(m);
        if (c->stream) (void)hipStreamDestroy(c->stream);
    }
    delete c;
}

const char* ft_last_error(const ft_context* c) { return c ? c->err.c_str() : "null context"; }

// The keys of ft_set_option.  A flag takes any value as 0 / 1; any other value must lie in [lo, hi] (and be 0 or a power of two where
// kPowerOfTwo says so).  It goes into an Options member of every device of the context, or into device 0's scene graph: the peers
// receive the scene flattened on device 0.  kCommit / kLevelHint / kZeroFill: a change invalidates the committed scene, the staged
// level hint, the zero-fill signatures.  kOrZero: 0 is valid beside [lo, hi].  kClassified: setting it drops what the frame slots keep of their last classification.
enum { kFlag = 1, kPowerOfTwo = 2, kCommit = 4, kLevelHint = 8, kZeroFill = 16, kOrZero = 32, kClassified = 64, kOneElseZero = 128 };   // kOneElseZero: 1 is 1, any other value 0
struct OptionSpec {
    const char* key;
    int64_t lo, hi;
    int64_t Options::* field;
    void (*to_graph)(fth::SceneGraph&, int64_t);
    int rules;
};
constexpr int64_t kNoLimit = std::numeric_limits<int64_t>::max();
const OptionSpec kOptions[] = {
    {"chunk_samples", 64, kNoLimit, &Options::chunk_samples, nullptr, 0},
    {"wave_samples", 0, 16, &Options::wave_samples, nullptr, kPowerOfTwo},   // 1 .. 16 samples per wavefront (k_resolve's LDS tile holds 16)
    {"coherent_waves", 0, 1, &Options::coherent_waves, nullptr, kFlag},
    {"timing", 0, 2, &Options::timing, nullptr, 0},
    {"classify_pixels", 0, 1, &Options::classify_pixels, nullptr, kFlag | kClassified},
    {"follow_below", -1, kNoLimit, &Options::follow_below, nullptr, kLevelHint},
    {"level_hint", 0, 1, &Options::level_hint, nullptr, kFlag},
    {"classify_ahead", 0, 1, &Options::classify_ahead, nullptr, kFlag},
    {"resolve_aside", 0, 1, &Options::resolve_aside, nullptr, kFlag},
    {"zero_fill_skip", 0, 1, &Options::zero_fill_skip, nullptr, kFlag | kZeroFill},
    {"classify_reuse", 0, 1, &Options::classify_reuse, nullptr, kFlag | kClassified},
    {"mains", 1, ft_context::kMains, &Options::mains, nullptr, 0},
    {"bvh_builder", 0, 3, &Options::bvh_builder, nullptr, kCommit},
    {"csg_auto_grow", 0, 1, &Options::csg_auto_grow, nullptr, kFlag},
    {"primary_block_lists", 0, 1, &Options::primary_block_lists, nullptr, kFlag | kClassified},
    {"uniform_surface", 0, 1, &Options::uniform_surface, nullptr, kFlag},
    {"edge_cull", 0, 1, &Options::edge_cull, nullptr, kFlag},       // (read per frame; the records are written whatever it says: nothing kept depends on it)
    {"primary_mesh_kernel", 0, 1, &Options::primary_mesh_kernel, nullptr, kFlag},   // (no classification depends on it: the slots keep theirs)
    // read by ft_scene_commit_deformed and ft_temporal_accumulate: no commit depends on it either
    {"temporal_follow_deformed", 0, 1, &Options::temporal_follow_deformed, nullptr, kFlag},
    // read by ft_scene_commit_deformed alone: no commit depends on it, so it leaves the committed scene as it is
    {"refit_rebuild_percent", 100, 1000000, &Options::refit_rebuild_percent, nullptr, kOrZero},
    // read by ft_scene_commit_deformed alone, as the one above (any value other than 0 means 1)
    {"deform_light_space", 0, 1, &Options::deform_light_space, nullptr, kFlag},
    // read by ft_scene_commit_lights and ft_scene_commit_deformed alone, as the ones above (any value other than 0 means 1)
    {"light_space_retree", 0, 1, &Options::light_space_retree, nullptr, kFlag},
    // read by ft_scene_commit_deformed alone, as the ones above (the default is 1, and any other value means 0)
    {"morph_on_device", 0, 1, &Options::morph_on_device, nullptr, kOneElseZero},
    {"skin_on_device", 0, 1, &Options::skin_on_device, nullptr, kOneElseZero},
    // read by ft_scene_commit_moved alone, as the ones above (any value other than 0 means 1)
    {"moved_in_place", 0, 1, &Options::moved_in_place, nullptr, kFlag},
    {"csg_mesh_capacity", 1, 255, nullptr, [](fth::SceneGraph& g, int64_t v) { g.csg_mesh_capacity = (int32_t)v; }, kCommit},
    // directional shadow rays of coherent waves: 0 the BVH; 1 light-space trees; 2 (default) light-space grids, the trees for wide waves.
    // It was a flag before the grids: it still takes any value, and any other than 0 / 1 means 2.
    {"light_space_shadows", std::numeric_limits<int64_t>::min(), kNoLimit, nullptr,
     [](fth::SceneGraph& g, int64_t v) { g.light_space_shadows = v == 0 || v == 1 ? (int32_t)v : 2; }, kCommit},
    {"mesh_unclipped_bvh", 0, 1, nullptr, [](fth::SceneGraph& g, int64_t v) { g.mesh_unclipped_bvh = v != 0; }, kFlag | kCommit},
};

int32_t ft_set_option(ft_context* c, const char* key, int64_t value) {
    if (!c || !key) return FT_ERR_INVALID;
    for (const OptionSpec& o : kOptions) {
        if (std::strcmp(key, o.key)) continue;
        if (o.rules & kFlag) value = value != 0;
        else if (o.rules & kOneElseZero) value = value == 1;
        else if (!((o.rules & kOrZero) && value == 0) && (value < o.lo || value > o.hi || ((o.rules & kPowerOfTwo) && (value & (value - 1))))) return FT_ERR_INVALID;
        if (o.to_graph) { o.to_graph(c->graph, value); c->committed = false; c->options_pending = true; return FT_OK; }
        for (ft_context* d : devices(c)) {
            d->opt.*o.field = value;
            for (hipStream_t m : d->more_mains) if (!m) d->opt.mains = 1;   // (without them every frame takes the one main stream)
            d->dev_scene.coherent_waves = d->opt.coherent_waves ? 1 : 0;
            d->dev_scene.uniform_surface = d->opt.uniform_surface ? 1 : 0;
            d->dev_scene.ls_edges = d->opt.edge_cull ? d->lightspace.d_edges.as<float>() : nullptr;
            if (!d->opt.temporal_follow_deformed) temporal_drop_snapshots(d);   // (nothing to do unless the option has just gone back to 0)
            if (o.rules & kCommit) { d->committed = false; c->options_pending = true; }
            if (o.rules & kLevelHint) d->staged_hint = -1;
            if (o.rules & kZeroFill) d->zero_signature[0] = d->zero_signature[1] = 0;
            if (o.rules & kClassified) for (auto& F : d->slots) { F.kept.valid = false; F.keeps = false; }   // (a frame still queued goes on reading its slot's buffers)
        }
        return FT_OK;
    }
    c->err = std::string("unknown option: ") + key;
    return FT_ERR_INVALID;
}

// ------------------------------------------------------------------------------------------ builder
static ft_node add_node(ft_context* c, fth::GraphNode&& n) { c->graph.nodes.push_back(std::move(n)); c->committed = false; c->restructured = true; return (ft_node)c->graph.nodes.size() - 1; }

ft_node ft_sg_primitive(ft_context* c, int32_t kind) {
    if (!c || kind < 0 || kind > FT_PRIM_CYLINDER) return FT_ERR_INVALID;
    fth::GraphNode n; n.kind = fth::GraphNode::Prim; n.prim = kind; return add_node(c, std::move(n));
}
ft_node ft_sg_triangle(ft_context* c, const double v[9]) {
    if (!c || !v) return FT_ERR_INVALID;
    fth::GraphNode n; n.kind = fth::GraphNode::TriangleP; std::memcpy(n.tri, v, sizeof n.tri); return add_node(c, std::move(n));
}
ft_node ft_sg_bsp_mesh(ft_context* c, int32_t depth, const double* tris, int64_t n_tris) {
    if (!c || n_tris < 0 || (n_tris > 0 && !tris) || depth < 0) return FT_ERR_INVALID;
    fth::GraphNode n; n.kind = fth::GraphNode::Mesh; n.depth = depth; n.tris.assign(tris, tris + 9 * n_tris); return add_node(c, std::move(n));
}
ft_node ft_sg_transform(ft_context* c, const ft_transform* ts, int32_t n_ts, ft_node child) {
    if (!c || !c->graph.valid(child) || !ts || n_ts < 1) return FT_ERR_INVALID;
    fth::GraphNode n; n.kind = fth::GraphNode::Transform;
    for (int i = 0; i < n_ts; ++i) { if (ts[i].kind < FT_TRANSLATE || ts[i].kind > FT_ROTATE) return FT_ERR_INVALID; n.xf.push_back(ts[i]); }
    n.children = {child};
    return add_node(c, std::move(n));
}
// The transform list of an existing Transform node replaced; the child stays.  Not a structural change: the graph flattens to the same
// leaves in the same order, which is what ft_scene_commit_moved needs.
int32_t ft_sg_set_transform(ft_context* c, ft_node node, const ft_transform* ts, int32_t n_ts) {
    if (!c) return FT_ERR_INVALID;
    if (!c->graph.valid(node) || c->graph.nodes[node].kind != fth::GraphNode::Transform) { c->err = "ft_sg_set_transform: not a transform node"; return FT_ERR_INVALID; }
    if (!ts || n_ts < 1) { c->err = "ft_sg_set_transform: no transforms"; return FT_ERR_INVALID; }
    for (int i = 0; i < n_ts; ++i) if (ts[i].kind < FT_TRANSLATE || ts[i].kind > FT_ROTATE) { c->err = "ft_sg_set_transform: bad transform kind"; return FT_ERR_INVALID; }
    c->graph.nodes[node].xf.assign(ts, ts + n_ts);
    c->committed = false; c->moved_pending = true;
    return FT_OK;
}
// The vertices of an existing mesh node replaced; the count stays.  Not a structural change either: the graph flattens to the same leaves
// over the same meshes, which is what ft_scene_commit_deformed needs.
int32_t ft_sg_set_mesh_triangles(ft_context* c, ft_node node, const double* tris, int64_t n_tris) {
    if (!c) return FT_ERR_INVALID;
    if (!c->graph.valid(node) || c->graph.nodes[node].kind != fth::GraphNode::Mesh) { c->err = "ft_sg_set_mesh_triangles: not a bspMesh node"; return FT_ERR_INVALID; }
    if (!tris) { c->err = "ft_sg_set_mesh_triangles: no triangles"; return FT_ERR_INVALID; }
    fth::GraphNode& n = c->graph.nodes[node];
    if (n_tris < 0 || (uint64_t)n_tris != n.tris.size() / 9) { c->err = "ft_sg_set_mesh_triangles: the triangle count differs from the node's"; return FT_ERR_INVALID; }
    n.tris.assign(tris, tris + 9 * n_tris);
    n.by_weights = false; n.tris_stale = false;                     // explicit vertices; base and deltas stay for a later ft_sg_set_mesh_weights
    n.shape_serial = ++c->skin.serials; n.posed_stale = true;       // (under a palette they are the shape U: the palette stays in force)
    n.deformed = true;
    c->committed = false;
    return FT_OK;
}
// Morph targets: the base is the node's vertices as they stand, the targets are kept as deltas from it.  Not a structural
// change and no edit: the vertices stay what they are.
static_assert(ftk::kMaxMorphTargets == FT_MAX_MORPH_TARGETS, "ftk::MorphBlend carries FT_MAX_MORPH_TARGETS weights");
static void drop_resident_targets(ft_context* c, ft_node node) {
    if (c->host_only) return;
    for (ft_context* d : devices(c)) {
        auto& held = d->morph.meshes;
        for (size_t k = 0; k < held.size(); ++k) {
            if (held[k].node != node) continue;
            (void)hipSetDevice(d->device);
            held[k].d.release();
            held.erase(held.begin() + (long)k);
            break;
        }
    }
    (void)hipSetDevice(c->device);
}
int32_t ft_sg_set_mesh_targets(ft_context* c, ft_node node, const double* targets, int32_t n_targets, int64_t n_tris) {
    if (!c) return FT_ERR_INVALID;
    if (!c->graph.valid(node) || c->graph.nodes[node].kind != fth::GraphNode::Mesh) { c->err = "ft_sg_set_mesh_targets: not a bspMesh node"; return FT_ERR_INVALID; }
    fth::GraphNode& n = c->graph.nodes[node];
    if (n_tris < 0 || (uint64_t)n_tris != n.tris.size() / 9) { c->err = "ft_sg_set_mesh_targets: the triangle count differs from the node's"; return FT_ERR_INVALID; }
    if (n_targets < 0 || n_targets > FT_MAX_MORPH_TARGETS) { c->err = "ft_sg_set_mesh_targets: the target count is outside 0 .. FT_MAX_MORPH_TARGETS"; return FT_ERR_INVALID; }
    if (n_targets > 0 && !targets) { c->err = "ft_sg_set_mesh_targets: no targets"; return FT_ERR_INVALID; }
    const std::vector<double>& B = n.shape();                       // (blended first where weights describe them: they are explicit from here on; under a palette the shape U, not the skinned V)
    if (n.by_weights) n.shape_serial = ++c->skin.serials;           // (what a device holds as the rest shape is not this)
    n.by_weights = false; n.tris_stale = false;
    n.weights.clear();
    n.n_targets = n_targets;
    n.targets_serial = ++c->morph.serials;
    if (n_targets == 0) {
        std::vector<double>().swap(n.base); std::vector<double>().swap(n.deltas);
        drop_resident_targets(c, node);
        return FT_OK;
    }
    const size_t count = B.size();
    n.base = B;
    n.deltas.resize((size_t)n_targets * count);
    for (int32_t k = 0; k < n_targets; ++k) for (size_t i = 0; i < count; ++i) n.deltas[(size_t)k * count + i] = targets[(size_t)k * count + i] - B[i];
    return FT_OK;
}
int32_t ft_sg_set_mesh_weights(ft_context* c, ft_node node, const double* weights, int32_t n_weights) {
    if (!c) return FT_ERR_INVALID;
    if (!c->graph.valid(node) || c->graph.nodes[node].kind != fth::GraphNode::Mesh) { c->err = "ft_sg_set_mesh_weights: not a bspMesh node"; return FT_ERR_INVALID; }
    fth::GraphNode& n = c->graph.nodes[node];
    if (n.n_targets == 0) { c->err = "ft_sg_set_mesh_weights: the node has no targets (ft_sg_set_mesh_targets)"; return FT_ERR_INVALID; }
    if (n_weights != n.n_targets) { c->err = "ft_sg_set_mesh_weights: the weight count differs from the node's target count"; return FT_ERR_INVALID; }
    if (!weights) { c->err = "ft_sg_set_mesh_weights: no weights"; return FT_ERR_INVALID; }
    for (int32_t k = 0; k < n_weights; ++k) if (!std::isfinite(weights[k])) { c->err = "ft_sg_set_mesh_weights: a weight is not finite"; return FT_ERR_INVALID; }
    n.weights.assign(weights, weights + n_weights);
    n.by_weights = true; n.tris_stale = true; n.posed_stale = true;
    n.deformed = true;
    c->committed = false;
    return FT_OK;
}
int32_t ft_debug_morph(ft_context* c, ft_node node, int64_t counts[4], double scan[8]) {
    if (!c || !counts || !scan) return FT_ERR_INVALID;
    if (!c->graph.valid(node) || c->graph.nodes[node].kind != fth::GraphNode::Mesh) { c->err = "ft_debug_morph: not a bspMesh node"; return FT_ERR_INVALID; }
    const ft_context::Morph& M = c->morph;
    for (int k = 0; k < 3; ++k) counts[k] = M.counts[k];
    counts[3] = 0;
    for (const ft_context::Morph::Resident& r : M.meshes) if (r.node == node) counts[3] = (int64_t)r.used;
    for (int k = 0; k < 8; ++k) scan[k] = 0.0;
    for (const ft_context::Morph::Used& u : M.last) if (u.node == node) for (int k = 0; k < 8; ++k) scan[k] = u.scan[k];
    return FT_OK;
}
// Skinning: a skin is indices and weights per corner, a palette the bone matrices of one pose; V = skin(U, palette).
static_assert(ftk::kMaxSkinBones == FT_MAX_SKIN_BONES && ftk::kMaxSkinInfluences == FT_MAX_SKIN_INFLUENCES, "k_skin reads a byte per index and a word per corner");
static void drop_resident_skin(ft_context* c, ft_node node) {
    if (c->host_only) return;
    for (ft_context* d : devices(c)) {
        auto& held = d->skin.meshes;
        for (size_t k = 0; k < held.size(); ++k) {
            if (held[k].node != node) continue;
            (void)hipSetDevice(d->device);
            ft_context::Skin::drop(held[k]);
            held.erase(held.begin() + (long)k);
            break;
        }
    }
    (void)hipSetDevice(c->device);
}
int32_t ft_sg_set_mesh_skin(ft_context* c, ft_node node, const int32_t* bone_index, const double* bone_weight, int32_t influences, int64_t n_tris) {
    if (!c) return FT_ERR_INVALID;
    if (!c->graph.valid(node) || c->graph.nodes[node].kind != fth::GraphNode::Mesh) { c->err = "ft_sg_set_mesh_skin: not a bspMesh node"; return FT_ERR_INVALID; }
    fth::GraphNode& n = c->graph.nodes[node];
    if (n_tris < 0 || (uint64_t)n_tris != n.tris.size() / 9) { c->err = "ft_sg_set_mesh_skin: the triangle count differs from the node's"; return FT_ERR_INVALID; }
    if (influences < 0 || influences > FT_MAX_SKIN_INFLUENCES) { c->err = "ft_sg_set_mesh_skin: influences outside 0 .. FT_MAX_SKIN_INFLUENCES"; return FT_ERR_INVALID; }
    if (influences > 0 && (!bone_index || !bone_weight)) { c->err = "ft_sg_set_mesh_skin: no indices or no weights"; return FT_ERR_INVALID; }
    const size_t corners = 3 * (size_t)n_tris, J = (size_t)influences;
    int32_t largest = 0;
    for (size_t k = 0; k < corners * J; ++k) {
        if (bone_index[k] < 0 || bone_index[k] >= FT_MAX_SKIN_BONES) { c->err = "ft_sg_set_mesh_skin: a bone index is outside 0 .. FT_MAX_SKIN_BONES - 1"; return FT_ERR_INVALID; }
        if (!std::isfinite(bone_weight[k])) { c->err = "ft_sg_set_mesh_skin: a weight is not finite"; return FT_ERR_INVALID; }
        largest = std::max(largest, bone_index[k]);
    }
    if (n.n_bones > 0) { n.deformed = true; c->committed = false; }  // a palette was in force: the vertices are the shape again
    n.n_bones = 0; n.palette_kind = fth::GraphNode::NoPalette;
    std::vector<double>().swap(n.palette); std::vector<double>().swap(n.posed);
    n.posed_stale = false;
    n.skin_influences = influences; n.skin_max_index = largest;
    n.skin_serial = ++c->skin.serials;
    if (influences == 0) {
        std::vector<uint32_t>().swap(n.skin_index); std::vector<double>().swap(n.skin_weight);
        drop_resident_skin(c, node);
        return FT_OK;
    }
    n.skin_index.assign(corners, 0u);
    for (size_t k = 0; k < corners; ++k) for (size_t j = 0; j < J; ++j) n.skin_index[k] |= (uint32_t)bone_index[k * J + j] << (8 * j);
    n.skin_weight.assign(bone_weight, bone_weight + corners * J);
    return FT_OK;
}
// One pose's palette of either kind (a node holds at most one): per_bone doubles per bone, `what` names the entries in the messages.
static int32_t set_palette(ft_context* c, ft_node node, const double* data, int32_t n_bones, int32_t kind, size_t per_bone, const char* call, const char* what, const char* entry) {
    if (!c) return FT_ERR_INVALID;
    const std::string name(call);
    if (!c->graph.valid(node) || c->graph.nodes[node].kind != fth::GraphNode::Mesh) { c->err = name + ": not a bspMesh node"; return FT_ERR_INVALID; }
    fth::GraphNode& n = c->graph.nodes[node];
    if (n.skin_influences == 0) { c->err = name + ": the node has no skin (ft_sg_set_mesh_skin)"; return FT_ERR_INVALID; }
    if (n_bones < 0 || n_bones > FT_MAX_SKIN_BONES) { c->err = name + ": the bone count is outside 0 .. FT_MAX_SKIN_BONES"; return FT_ERR_INVALID; }
    if (n_bones > 0 && n_bones <= n.skin_max_index) { c->err = name + ": the skin uses a bone index the palette does not have"; return FT_ERR_INVALID; }
    if (n_bones > 0 && !data) { c->err = name + ": no " + what; return FT_ERR_INVALID; }
    for (size_t k = 0; k < per_bone * (size_t)n_bones; ++k) if (!std::isfinite(data[k])) { c->err = name + ": " + entry + " is not finite"; return FT_ERR_INVALID; }
    n.n_bones = n_bones;
    n.palette_kind = n_bones > 0 ? kind : (int32_t)fth::GraphNode::NoPalette;
    if (n_bones > 0) n.palette.assign(data, data + per_bone * (size_t)n_bones);
    else { std::vector<double>().swap(n.palette); std::vector<double>().swap(n.posed); }
    n.posed_stale = n_bones > 0;
    n.deformed = true;
    c->committed = false;
    return FT_OK;
}
int32_t ft_sg_set_mesh_bones(ft_context* c, ft_node node, const double* matrices, int32_t n_bones) {
    return set_palette(c, node, matrices, n_bones, fth::GraphNode::Matrices, 12, "ft_sg_set_mesh_bones", "matrices", "a matrix entry");
}
// Dual-quaternion palettes: 8 doubles per bone, used as given - neither normalised nor checked for unit length.
int32_t ft_sg_set_mesh_bones_dq(ft_context* c, ft_node node, const double* dual_quaternions, int32_t n_bones) {
    return set_palette(c, node, dual_quaternions, n_bones, fth::GraphNode::DualQuaternions, 8, "ft_sg_set_mesh_bones_dq", "dual quaternions", "a dual-quaternion entry");
}
int32_t ft_debug_skin(ft_context* c, ft_node node, int64_t counts[4]) {
    if (!c || !counts) return FT_ERR_INVALID;
    if (!c->graph.valid(node) || c->graph.nodes[node].kind != fth::GraphNode::Mesh) { c->err = "ft_debug_skin: not a bspMesh node"; return FT_ERR_INVALID; }
    for (int k = 0; k < 3; ++k) counts[k] = c->skin.counts[k];
    counts[3] = 0;
    for (const ft_context::Skin::Resident& r : c->skin.meshes) if (r.node == node) counts[3] = (int64_t)(r.used_rest + r.used_skin + r.used_palette);
    return FT_OK;
}
int32_t ft_debug_skin_dq(ft_context* c, ft_node node, int64_t counts[4]) {
    if (!c || !counts) return FT_ERR_INVALID;
    if (!c->graph.valid(node) || c->graph.nodes[node].kind != fth::GraphNode::Mesh) { c->err = "ft_debug_skin_dq: not a bspMesh node"; return FT_ERR_INVALID; }
    for (int k = 0; k < 3; ++k) counts[k] = c->skin.counts_dq[k];
    counts[3] = c->graph.nodes[node].palette_kind;
    return FT_OK;
}
ft_node ft_sg_material(ft_context* c, const ft_material* m, ft_node child) {
    if (!c || !c->graph.valid(child) || !m) return FT_ERR_INVALID;
    fth::GraphNode n; n.kind = fth::GraphNode::MaterialF; n.mat = *m; n.children = {child}; return add_node(c, std::move(n));
}
ft_node ft_sg_hue_shift(ft_context* c, double, ft_node child) {
    if (!c || !c->graph.valid(child)) return FT_ERR_INVALID;
    fth::GraphNode n; n.kind = fth::GraphNode::HueShift; n.children = {child}; return add_node(c, std::move(n));
}
ft_node ft_sg_ignore_light(ft_context* c, ft_node child) {
    if (!c || !c->graph.valid(child)) return FT_ERR_INVALID;
    fth::GraphNode n; n.kind = fth::GraphNode::IgnoreLight; n.children = {child}; return add_node(c, std::move(n));
}
ft_node ft_sg_group(ft_context* c, const ft_node* children, int32_t n_children) {
    if (!c || n_children < 0 || (n_children > 0 && !children)) return FT_ERR_INVALID;
    fth::GraphNode n; n.kind = fth::GraphNode::Group;
    for (int i = 0; i < n_children; ++i) { if (!c->graph.valid(children[i])) return FT_ERR_INVALID; n.children.push_back(children[i]); }
    return add_node(c, std::move(n));
}
ft_node ft_sg_csg(ft_context* c, int32_t op, ft_node a, ft_node b) {
    if (!c || !c->graph.valid(a) || !c->graph.valid(b) || op < FT_CSG_UNION || op > FT_CSG_EXCLUDE) return FT_ERR_INVALID;
    fth::GraphNode n; n.kind = fth::GraphNode::Csg; n.op = op; n.children = {a, b}; return add_node(c, std::move(n));
}
ft_node ft_sg_texture_grid(ft_context* c, const double ca[3], const double cb[3], const double* uv_ops, int32_t n_uv_ops, ft_node child) {
    if (!c || !c->graph.valid(child) || !ca || !cb || n_uv_ops < 0 || (n_uv_ops > 0 && !uv_ops)) return FT_ERR_INVALID;
    fth::GraphNode n; n.kind = fth::GraphNode::Texture;
    std::memcpy(n.ca, ca, sizeof n.ca); std::memcpy(n.cb, cb, sizeof n.cb);
    n.uv_ops.assign(uv_ops, uv_ops + 3 * n_uv_ops); n.children = {child};
    return add_node(c, std::move(n));
}

ft_node ft_sg_texture_image(ft_context* c, const uint8_t* rgb24, int32_t width, int32_t height, const double* uv_ops, int32_t n_uv_ops, ft_node child) {
    if (!c || !c->graph.valid(child) || !rgb24 || width <= 0 || height <= 0 || (int64_t)width * height > (1ll << 28) || n_uv_ops < 0 || (n_uv_ops > 0 && !uv_ops)) return FT_ERR_INVALID;
    fth::GraphNode n; n.kind = fth::GraphNode::Texture;
    n.pixels.assign(rgb24, rgb24 + (size_t)width * height * 3); n.img_w = width; n.img_h = height;
    n.uv_ops.assign(uv_ops, uv_ops + 3 * n_uv_ops); n.children = {child};
    return add_node(c, std::move(n));
}

int32_t ft_scene_clear(ft_context* c) {
    if (!c) return FT_ERR_INVALID;
    progressive_close(c);
    temporal_close(c);
    c->graph.nodes.clear(); c->graph.lights.clear(); c->graph.root = -1; c->committed = false; c->restructured = true;
    if (!c->host_only) {                                            // the morph targets of nodes that are gone (no frame reads them)
        for (ft_context* d : devices(c)) {
            if (d->morph.meshes.empty()) continue;
            (void)hipSetDevice(d->device);
            for (ft_context::Morph::Resident& r : d->morph.meshes) r.d.release();
            d->morph.meshes.clear();
        }
        for (ft_context* d : devices(c)) {                          // and their skins
            if (d->skin.meshes.empty()) continue;
            (void)hipSetDevice(d->device);
            d->skin.release();
        }
        (void)hipSetDevice(c->device);
    }
    c->morph.last.clear();
    return FT_OK;
}
int32_t ft_scene_set_objects(ft_context* c, ft_node root) {
    if (!c || !c->graph.valid(root)) return FT_ERR_INVALID;
    c->graph.root = root; c->committed = false; c->restructured = true;
    return FT_OK;
}
int32_t ft_scene_add_directional(ft_context* c, const double dir[3], const double colour[3]) {      // Light.directional (Light.fs:19-20)
    if (!c || !dir || !colour) return FT_ERR_INVALID;
    ftd::Light l{}; l.kind = ftd::LT_DIRECTIONAL;
    std::memcpy(l.v, dir, sizeof l.v); norm3(l.v); std::memcpy(l.colour, colour, sizeof l.colour);
    c->graph.lights.push_back(l); c->committed = false; c->restructured = true;
    return FT_OK;
}
int32_t ft_scene_add_soft_directional(ft_context* c, const double dir[3], int32_t samples, double scatter_rad, const double colour[3]) {  // Light.fs:22-23
    if (!c || !dir || !colour || samples < 1) return FT_ERR_INVALID;
    ftd::Light l{}; l.kind = ftd::LT_SOFT; l.samples = samples; l.scatter = scatter_rad;
    std::memcpy(l.v, dir, sizeof l.v); norm3(l.v); std::memcpy(l.colour, colour, sizeof l.colour);
    c->graph.lights.push_back(l); c->committed = false; c->restructured = true;            // rejected at commit until the seeded stream lands
    return FT_OK;
}
int32_t ft_scene_add_positional(ft_context* c, const double pos[3], const double falloff[3], const double colour[3]) {  // Light.fs:25-26
    if (!c || !pos || !falloff || !colour) return FT_ERR_INVALID;
    ftd::Light l{}; l.kind = ftd::LT_POINT;
    std::memcpy(l.v, pos, sizeof l.v); std::memcpy(l.falloff, falloff, sizeof l.falloff); std::memcpy(l.colour, colour, sizeof l.colour);
    c->graph.lights.push_back(l); c->committed = false; c->restructured = true;
    return FT_OK;
}
// The values of an existing light replaced, with the arithmetic of the ft_scene_add_* of its kind; the kind and a soft light's sample count
// stay (they fix the kernel variant, shadow_rays_per_hit and the byte packing).  Not a structural change: what ft_scene_commit_lights needs.
static ftd::Light* light_to_set(ft_context* c, int32_t light, uint32_t kind, const char* who) {
    if (light < 0 || (size_t)light >= c->graph.lights.size()) { c->err = std::string(who) + ": no such light"; return nullptr; }
    if (c->graph.lights[(size_t)light].kind != kind) { c->err = std::string(who) + ": the light is of another kind (ft_scene_clear / ft_scene_add_* change kinds)"; return nullptr; }
    c->committed = false; c->lights_pending = true;
    return &c->graph.lights[(size_t)light];
}
int32_t ft_scene_set_directional(ft_context* c, int32_t light, const double dir[3], const double colour[3]) {
    if (!c || !dir || !colour) return FT_ERR_INVALID;
    ftd::Light* l = light_to_set(c, light, ftd::LT_DIRECTIONAL, "ft_scene_set_directional");
    if (!l) return FT_ERR_INVALID;
    std::memcpy(l->v, dir, sizeof l->v); norm3(l->v); std::memcpy(l->colour, colour, sizeof l->colour);
    return FT_OK;
}
int32_t ft_scene_set_soft_directional(ft_context* c, int32_t light, const double dir[3], double scatter_rad, const double colour[3]) {
    if (!c || !dir || !colour) return FT_ERR_INVALID;
    ftd::Light* l = light_to_set(c, light, ftd::LT_SOFT, "ft_scene_set_soft_directional");
    if (!l) return FT_ERR_INVALID;
    l->scatter = scatter_rad;
    std::memcpy(l->v, dir, sizeof l->v); norm3(l->v); std::memcpy(l->colour, colour, sizeof l->colour);
    return FT_OK;
}
int32_t ft_scene_set_positional(ft_context* c, int32_t light, const double pos[3], const double falloff[3], const double colour[3]) {
    if (!c || !pos || !falloff || !colour) return FT_ERR_INVALID;
    ftd::Light* l = light_to_set(c, light, ftd::LT_POINT, "ft_scene_set_positional");
    if (!l) return FT_ERR_INVALID;
    std::memcpy(l->v, pos, sizeof l->v); std::memcpy(l->falloff, falloff, sizeof l->falloff); std::memcpy(l->colour, colour, sizeof l->colour);
    return FT_OK;
}

} // extern "C"

namespace ftc {

static const char* const kLdsRefusal = "scene needs more than 160 KiB of LDS per workgroup for CSG lists / BSP stacks even with 4 live lanes per wave";
static int32_t lds_fits(ft_context* c) {
    if (lane_fold_for(c->flat) != 0) return FT_OK;
    c->err = kLdsRefusal;
    return FT_ERR_UNSUPPORTED;
}

// What d_scene[kCullItems] holds: the items' float records and, behind them, a float image of every parallel-sensitive direction (x, y, z,
// its length rounded up), which lane k of a coherent wave tests against the bundle's cone before any ray is tested against it exactly
// (rows_nearly_parallel, ft_kernels.hip).
static void cull_items_image(const fth::FlatScene& f, std::vector<float>& v) {
    v = f.cull_items;
    v.resize(8 * (f.item_pc.size() - 1), 0.0f);
    for (size_t k = 0; k + 2 < f.cull_rows.size(); k += 3) {
        const double len = std::sqrt(f.cull_rows[k] * f.cull_rows[k] + f.cull_rows[k + 1] * f.cull_rows[k + 1] + f.cull_rows[k + 2] * f.cull_rows[k + 2]);
        float lf = (float)len; while ((double)lf < len) lf = std::nextafter(lf, std::numeric_limits<float>::infinity());
        v.push_back((float)f.cull_rows[k]); v.push_back((float)f.cull_rows[k + 1]); v.push_back((float)f.cull_rows[k + 2]); v.push_back(lf);
    }
}

// The ranges of a device job in the context's scene arrays, as ft_bvh.hip takes them.
static ftk::LbvhTarget lbvh_target(ft_context* c, const fth::FlatScene::BvhJob& j) {
    const DeviceBuf* B = c->d_scene;
    return ftk::LbvhTarget{geo_array(c, kTris).as<double>(), j.first_global, j.n, geo_array(c, kNodes).as<ftd::BspNode>(), j.node_base, B[kBspLeaves].as<ftd::BspLeaf>(), j.leaf_base,
                           B[kTriOrig].as<uint32_t>(), j.tri_base, geo_array(c, kWide).as<double>(), j.wide_base, geo_array(c, kCoarse).as<float>() + 6 * (size_t)j.coarse_first, j.coarse_count,
                           B[kTriSrc].as<uint32_t>()};
}

// Room in the per-lane node stacks of the incoherent walk (LDS) for a device-built tree of `height` node levels.
static int32_t fit_stacks(ft_context* c, uint32_t height) {
    if ((int32_t)height + 1 > c->flat.stack_capacity) c->flat.stack_capacity = (int32_t)height + 1;
    return lds_fits(c);
}

// The scene k_primary_mesh is written for (ft_kernels.hip): one top-level item whose program is a single OP_LEAF_FOLD of leaf 0, a lit LK_MESH
// leaf with a BVH (`bspMesh 0`), under directional lights only; no material that needs a FANCY variant or reflects.  `variant`: the scene's.
static bool mesh_kernel_scene(const fth::FlatScene& f, int variant) {
    if (variant != 4 || f.item_pc.size() != 2 || f.leaves.size() != 1 || f.any_reflective) return false;
    size_t pc = f.item_pc[0] & 0x7FFFFFFFu;
    if (pc < f.program.size() && (f.program[pc] & 0xFFu) == ftd::OP_CULL) pc += 2;   // the item's own cull: it only ever skips a query that finds nothing
    if (pc + 1 >= f.program.size() || f.program[pc] != (uint32_t)ftd::OP_LEAF_FOLD || (f.program[pc + 1] & 0xFFu) != ftd::OP_END) return false;   // (leaf 0: arg = 0)
    const ftd::Leaf& L = f.leaves[0];
    if (L.kind != ftd::LK_MESH || !(L.flags & ftd::LF_LIT) || L.mesh >= f.meshes.size() || f.meshes[L.mesh].bvh_root < 0) return false;
    for (auto& l : f.lights) if (l.kind != ftd::LT_DIRECTIONAL) return false;
    for (auto& m : f.materials) if (m.reflectance > 0.0) return false;
    return true;
}

// What the launches read of the scene `flat` describes and the arrays in HBM hold: the device scene's counts and capacities, the kernel
// variants and the resident workgroups per CU.  At the end of every upload, and again when a rebuild in place made a taller tree.
static void derive_launch_shape(ft_context* c) {
    const fth::FlatScene& f = c->flat;
    ftk::DevScene& S = c->dev_scene;
    S.coherent_waves = c->opt.coherent_waves ? 1 : 0;
    S.uniform_surface = c->opt.uniform_surface ? 1 : 0;
    S.n_simd = c->n_cu * 4;
    S.n_items = (int32_t)f.item_pc.size() - 1; S.n_cull_rows = f.cull_bundle ? (int32_t)(f.cull_rows.size() / 3) : -1;
    S.n_leaves = (int32_t)f.leaves.size(); S.n_lights = (int32_t)f.lights.size();
    S.csg_cap = f.csg_capacity; S.stack_cap = f.stack_capacity;
    S.lane_fold = lane_fold_for(f); S.csg_rows = (f.csg_capacity + S.lane_fold - 1) / S.lane_fold;
    S.shadow_rays_per_hit = 0;
    for (auto& l : f.lights) S.shadow_rays_per_hit += (l.kind == ftd::LT_SOFT) ? l.samples : 1;   // Shading.fs:24-42
    c->variant = 0;
    for (auto& m : f.materials) if (needs_fancy(m)) c->variant |= 1;                               // FANCY
    for (auto& l : f.lights) if (l.kind == ftd::LT_SOFT) c->variant |= 2;                          // SOFT
    if (!f.meshes.empty()) c->variant |= 4;                                                        // MESH
    const size_t lds = lds_bytes_for(c->flat);
    c->variant_primary = c->variant;
    c->blocks_primary = ftk::occupancy_blocks_primary(lds, &c->variant_primary);
    c->blocks_bounce = ftk::occupancy_blocks_bounce(lds, c->variant);
    c->blocks_resolve = ftk::occupancy_blocks_resolve();
    c->blocks_aov = ftk::occupancy_blocks_aov(lds, c->variant);
    c->mesh_kernel_scene = mesh_kernel_scene(f, c->variant);
    c->blocks_primary_mesh = ftk::occupancy_blocks_primary_mesh();
}

// The edge records of every shadow grid of the scene as it lies in HBM (option "edge_cull"; ft_edges.h, k_ls_edges), after an upload or a
// rebuild of the light-space arrays: pairs = the pair records as just uploaded (their grid words name the cell tables), node_words and
// tri_doubles the sizes of ls_nodes and ls_tris there.  Zeros - the record that cuts nothing off - under every record no grid entry
// points at.  No grid, or more records than kLsEdgeMaxBytes holds: no array, and the shadow queries go by the rectangles alone.
static int32_t build_ls_edges(ft_context* c, const std::vector<double>& pairs, size_t node_words, size_t tri_doubles) {
    ft_context::LightSpace& L = c->lightspace;
    ftk::DevScene& S = c->dev_scene;
    S.ls_edges = nullptr;
    const size_t n_recs = tri_doubles / 9, bytes = n_recs * ftk::kEdgeFloats * sizeof(float);
    bool grids = false;
    for (size_t r = 0; r + 1 <= pairs.size() / ftd::kLsPairDoubles; ++r) {
        uint32_t w[2];
        std::memcpy(w, &pairs[ftd::kLsPairDoubles * r + 15], sizeof w);
        grids = grids || w[1] != 0u;
    }
    if (!grids || n_recs == 0 || bytes > ftd::kLsEdgeMaxBytes || node_words > 0xFFFFFFFFull || n_recs > 0xFFFFFFFFull) { L.d_edges.release(); return FT_OK; }
    int32_t rc;
    if ((rc = ensure(c, L.d_edges, bytes)) != FT_OK) return rc;
    FT_HIP(c, hipMemsetAsync(L.d_edges.p, 0, bytes, c->stream));
    const DeviceBuf* B = c->d_scene;
    for (size_t r = 0; r + 1 <= pairs.size() / ftd::kLsPairDoubles; ++r) {
        uint32_t w[2];
        std::memcpy(w, &pairs[ftd::kLsPairDoubles * r + 15], sizeof w);
        int32_t root;
        std::memcpy(&root, &pairs[ftd::kLsPairDoubles * r + 14], 4);
        if (w[1] == 0u || root == INT32_MIN) continue;
        ftk::ls_edge_records(c->stream, B[kLsPairs].as<double>() + ftd::kLsPairDoubles * r, B[kLsNodes].as<uint32_t>(), (uint32_t)node_words, B[kLsTris].as<double>(),
                             (uint32_t)n_recs, (w[1] & 0xFFFFu) * (w[1] >> 16), L.d_edges.as<float>());
    }
    FT_HIP(c, hipGetLastError());
    FT_HIP(c, hipStreamSynchronize(c->stream));
    S.ls_edges = c->opt.edge_cull ? L.d_edges.as<float>() : nullptr;
    return FT_OK;
}

static int32_t upload_scene(ft_context* c) {
    int32_t rc;
    FT_HIP(c, hipSetDevice(c->device));
    // frames still queued trace the scene these uploads replace, and not all of them on the stream the uploads travel on (FrameSlot::main_ix);
    // queued temporal calls read the frames, and their guide passes the scene
    if (any_queued(c)) { if ((rc = retire_queued(c)) != FT_OK) return rc; c->accum_open = false; }
    const fth::FlatScene& f = c->flat;
    if ((rc = lds_fits(c)) != FT_OK) return rc;
    // back to pose set 0, the arrays uploaded below; the other sets have the previous commit's sizes and go (nothing reads them: every
    // frame and temporal call has been retired, and an upload nobody has read yet ends here)
    if (c->pose.copies) FT_HIP(c, hipStreamSynchronize(c->pose.copies));
    c->pose.free_spares();
    // and to geometry set 0, the same way (a queued refit nobody has read yet ends here)
    if (c->geo.deform) FT_HIP(c, hipStreamSynchronize(c->geo.deform));
    c->geo.free_spares();
    c->refit.ready = false;                                         // the trees these uploads bring are not the ones its tables describe
    c->lightspace.reset();                                          // nor the light-space trees ft_scene_commit_lights' tables describe
    ftk::DevScene& S = c->dev_scene;
    rc = FT_OK;
    auto put = [&](SceneArray k, const auto& v, auto*& ptr) {   // array k into its buffer, and the device scene's pointer to it
        if (rc == FT_OK) rc = upload(c, c->d_scene[k], v);
        ptr = static_cast<std::remove_reference_t<decltype(ptr)>>(c->d_scene[k].p);
    };
    put(kLeaves, f.leaves, S.leaves); put(kM2w, f.m2w, S.m2w); put(kMaterials, f.materials, S.materials); put(kLights, f.lights, S.lights);
    put(kTextures, f.textures, S.textures); put(kTexPixels, f.tex_pixels, S.tex_pixels); put(kProgram, f.program, S.program);
    put(kMeshes, f.meshes, S.meshes); put(kNodes, f.nodes, S.nodes); put(kBspLeaves, f.bsp_leaves, S.bsp_leaves); put(kTris, f.tris, S.tris);
    put(kCulls, f.culls, S.culls);
    cull_items_image(f, c->cull_items_and_rows);
    put(kCullItems, c->cull_items_and_rows, S.cull_items);
    put(kCullRows, f.cull_rows, S.cull_rows); put(kItemPc, f.item_pc, S.item_pc); put(kWide, f.wide, S.wide); put(kMeshWide, f.mesh_wide, S.mesh_wide);
    put(kCoarse, f.coarse_boxes, S.coarse_boxes); put(kTriOrig, f.tri_orig, S.tri_orig);
    put(kLsPairs, f.ls_pairs, S.ls_pairs); put(kLsNodes, f.ls_nodes, S.ls_nodes); put(kLsTris, f.ls_tris, S.ls_tris);
    if (rc == FT_OK) rc = upload(c, c->d_scene[kTriSrc], f.tri_src);
    if (rc == FT_OK) rc = upload(c, c->d_scene[kRunNodes], f.run_nodes);
    if (rc != FT_OK) return rc;
    for (auto& F : c->slots) { if ((rc = ensure(c, F.d_fc, sizeof(ftk::SlotCounters))) != FT_OK) return rc; F.fc_clean = false; }
    c->zero_signature[0] = c->zero_signature[1] = 0;
    FT_HIP(c, hipStreamSynchronize(c->stream));
    {   // the BVHs the flattener left to the device (ft_bvh.hip), straight into the ranges reserved in the arrays just uploaded
        const auto t0 = std::chrono::steady_clock::now();
        uint32_t tallest = 0;
        for (const fth::FlatScene::BvhJob& j : f.bvh_jobs) {
            uint32_t height = 0;
            FT_HIP(c, ftk::build_lbvh(c->stream, lbvh_target(c, j), &height, c->opt.bvh_builder == 1 ? 0 : 1));
            // height 0: a non-finite coordinate; > 40: deeper than the packet walk's 64-entry stack allows (3 entries per 4-wide level)
            if (height == 0 || height > 40) { c->err = "device BVH build refused (non-finite vertex or a tree deeper than 40 levels): the host builder takes over"; return FT_ERR_BUILD; }
            tallest = std::max(tallest, height);
        }
        if (!f.bvh_jobs.empty()) {
            c->commit_ms[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            c->commit_ms[3] = tallest;
            if ((rc = fit_stacks(c, tallest)) != FT_OK) return rc;
        }
    }
    if ((rc = build_ls_edges(c, f.ls_pairs, f.ls_nodes.size(), f.ls_tris.size())) != FT_OK) return rc;
    derive_launch_shape(c);
    c->committed = true;
    ++c->commit_serial; c->staged_hint = -1;
    return FT_OK;
}

int32_t commit_scene(ft_context* c) {
    using clock = std::chrono::steady_clock;
    auto ms_since = [](clock::time_point t0) { return std::chrono::duration<double, std::milli>(clock::now() - t0).count(); };
    for (double& v : c->commit_ms) v = 0.0;
    const bool held = c->holds_commit;
    const auto done = [c](int32_t rc) {
        if (rc == FT_OK) { c->holds_commit = true; c->restructured = false; c->moved_pending = false; c->options_pending = false; c->lights_pending = false; for (fth::GraphNode& n : c->graph.nodes) n.deformed = false; }
        return rc;
    };
    // A device context builds the exact BVH of top-level-Leaf meshes on the device ("bvh_builder" = 1; 2, the default: from 4096 triangles on): the flattener
    // reserves the ranges, upload_scene fills them.  A build the device refuses (a tree too deep for the traversal stacks) falls
    // back to the host's builder, once, for the whole scene.
    for (int attempt = 0; attempt < 2; ++attempt) {
        c->graph.device_bvh = !c->host_only && c->opt.bvh_builder >= 1 && attempt == 0;
        c->graph.device_bvh_min_tris = c->opt.bvh_builder == 2 ? kDeviceBvhMinTris : 0;   // 1: the device's linear BVH, 3: its surface-area tree, whatever the size
        auto t0 = clock::now();
        fth::FlatScene fresh;
        int32_t rc = c->graph.flatten(fresh, c->err);
        if (rc == FT_OK && !c->host_only && lane_fold_for(fresh) == 0) { rc = FT_ERR_UNSUPPORTED; c->err = kLdsRefusal; }
        c->commit_ms[0] += ms_since(t0);
        if (rc != FT_OK) {
            // Refused by the flattener (a limit of the device path; a graph without objects) before anything was replaced:
            // `flat` and the arrays in HBM are still the previous commit's, whole, and stay renderable - as after a refused
            // ft_scene_commit_deformed.
            if (attempt == 0 && held) for (ft_context* d : devices(c)) d->committed = true;
            return rc;
        }
        c->holds_commit = false;                                    // `flat` is being replaced
        c->tree_quality.clear();                                    // and with it every tree the costs and rebuild counts were of
        c->flat = std::move(fresh);
        if (c->host_only) { c->committed = true; return done(FT_OK); }
        t0 = clock::now();
        rc = upload_scene(c);
        for (ft_context* p : c->peers) {                            // replicate the flattened scene on every other device
            if (rc != FT_OK) break;
            p->flat = c->flat;
            if ((rc = upload_scene(p)) != FT_OK) c->err = p->err;
            c->commit_ms[1] += p->commit_ms[1];
        }
        c->commit_ms[2] += ms_since(t0) - c->commit_ms[1];
        if (rc == FT_ERR_BUILD && c->graph.device_bvh) continue;    // refused by the device builder: the host builds it
        return done(rc);
    }
    return FT_ERR_BUILD;
}

// ------------------------------------------------------------------------------------------ refit (ft_scene_commit_deformed)
// One edited mesh of the held scene: its index, its builder node and what one pass over the new vertices gave.
// at: where its new vertices lie in ft_context::Refit::d_verts (doubles; even, so that every mesh starts on 16 bytes); on_device: weights
// describe them and k_morph_blend writes them there on every device - the host holds no copy of them.
// blended / skinned: which of k_morph_blend and k_skin make them (the blend writes the shape there, the skin poses it in
// place; without a blend the skin reads the rest shape resident beside its indices and weights).
struct DeformedMesh { uint32_t mesh; int32_t node; fth::MeshScan scan; size_t at = 0; bool on_device = false, blended = false, skinned = false; };
static size_t verts_doubles(const fth::SceneGraph& g, const std::vector<DeformedMesh>& edits) {
    size_t n = 0;
    for (const DeformedMesh& e : edits) n = std::max(n, e.at + g.nodes[(size_t)e.node].tris.size());
    return n;
}

using ftk::refit::refit_ranges;                                    // one mesh's ranges as the refit kernels take them (ft_refit_cost.h)

static bool refittable(const fth::FlatScene& f, uint32_t mesh) { return f.meshes[mesh].root < 0 && f.meshes[mesh].bvh_root != INT32_MIN; }
static const fth::FlatScene::BvhJob* job_of(const fth::FlatScene& f, uint32_t mesh) {
    for (const fth::FlatScene::BvhJob& j : f.bvh_jobs) if (j.mesh == mesh) return &j;
    return nullptr;
}
// The scene's arrays in HBM - of what a refit rewrites, the live geometry set's (geo_array) - and, once a refit has made them, the
// refit's own tables.
static ftk::RefitArrays refit_arrays(ft_context* c) {
    DeviceBuf* B = c->d_scene;
    ft_context::Refit& R = c->refit;
    return ftk::RefitArrays{geo_array(c, kTris).as<double>(), geo_array(c, kNodes).as<ftd::BspNode>(), B[kBspLeaves].as<ftd::BspLeaf>(), B[kTriOrig].as<uint32_t>(), geo_array(c, kWide).as<double>(),
                            geo_array(c, kCoarse).as<float>(), R.d_wide_node.as<int32_t>(), R.d_parent_node.as<int32_t>(), R.d_parent_leaf.as<int32_t>(), R.d_arrived.as<uint32_t>(),
                            R.d_leaf_boxes.as<double>()};
}

// The cost of mesh `mesh`'s tree as it lies in this device's HBM (ftk::refit_cost); blocks until it is there.  Nothing else may be
// writing the scene's arrays: the caller has retired the queued frames.
static int32_t measure_cost(ft_context* c, const fth::FlatScene& f, uint32_t mesh, double* cost) {
    const ftk::RefitMesh m = refit_ranges(f, mesh, 0.0);
    const uint32_t blocks = ftk::refit_cost_blocks(m);
    int32_t rc;
    if ((rc = ensure(c, c->refit.d_cost, ((size_t)blocks + 1) * 8)) != FT_OK) return rc;
    double* d = c->refit.d_cost.as<double>();
    ftk::refit_cost(c->stream, refit_arrays(c), m, d, d + blocks);
    FT_HIP(c, hipGetLastError());
    FT_HIP(c, hipMemcpyAsync(cost, d + blocks, 8, hipMemcpyDeviceToHost, c->stream));
    FT_HIP(c, hipStreamSynchronize(c->stream));
    return FT_OK;
}
// cost_built of every refittable mesh that has none yet (the context's first device; before a refit rewrites anything).
static int32_t record_built_costs(ft_context* c, const fth::FlatScene& f) {
    c->tree_quality.resize(f.meshes.size());
    for (uint32_t k = 0; k < (uint32_t)f.meshes.size(); ++k) {
        ft_context::TreeQuality& q = c->tree_quality[k];
        if (q.known || !refittable(f, k)) continue;
        const int32_t rc = measure_cost(c, f, k, &q.cost_built);
        if (rc != FT_OK) return rc;
        q.known = true;
    }
    return FT_OK;
}

// The tree of a device job built again in place from the list-order records the refit has just written.  The job's node,
// leaf and 4-wide ranges first go back to what the flattener reserved (build_bsp, all zero bytes): k_bvh_emit leaves the slots past the
// new node count alone and real_node() reads the leaf twin of every slot, so a twin the old tree left there would pass for a node of
// the new one.  Then the builder, as upload_scene runs it, and the refit's parent tables of the mesh's ranges.
static int32_t rebuild_in_place(ft_context* c, const fth::FlatScene& f, const fth::FlatScene::BvhJob& j, uint32_t* height) {
    DeviceBuf* B = c->d_scene;
    ft_context::Refit& R = c->refit;
    const fth::FlatScene::JobSpans sp = fth::FlatScene::reserved_spans(j);
    FT_HIP(c, hipMemsetAsync(geo_array(c, kNodes).as<ftd::BspNode>() + sp.node_first, 0, sp.node_count * sizeof(ftd::BspNode), c->stream));
    FT_HIP(c, hipMemsetAsync(B[kBspLeaves].as<ftd::BspLeaf>() + sp.leaf_first, 0, sp.leaf_count * sizeof(ftd::BspLeaf), c->stream));
    FT_HIP(c, hipMemsetAsync(geo_array(c, kWide).as<double>() + ftd::kWideNodeDoubles * sp.wide_first, 0, sp.wide_count * ftd::kWideNodeDoubles * 8, c->stream));
    FT_HIP(c, ftk::build_lbvh(c->stream, lbvh_target(c, j), height, c->opt.bvh_builder == 1 ? 0 : 1));
    if (*height == 0 || *height > 40) { c->err = "ft_scene_commit_deformed: the rebuild in place was refused (a tree deeper than 40 levels): ft_scene_commit"; return FT_ERR_BUILD; }
    FT_HIP(c, hipMemsetAsync(R.d_parent_node.as<int32_t>() + sp.node_first, 0xFF, sp.node_count * 4, c->stream));
    FT_HIP(c, hipMemsetAsync(R.d_parent_leaf.as<int32_t>() + sp.leaf_first, 0xFF, sp.leaf_count * 4, c->stream));
    ftk::refit_parents(c->stream, refit_arrays(c), refit_ranges(f, j.mesh, 0.0));
    FT_HIP(c, hipGetLastError());
    FT_HIP(c, hipStreamSynchronize(c->stream));
    return FT_OK;
}

// The list-order records of every mesh of `edits` that holds no snapshot yet, copied device to device behind what the accumulation
// already keeps (ft_context::Temporal::d_snap), on the context's stream: ahead of the refit kernels that overwrite them.
static int32_t snapshot_records(ft_context* c, const fth::FlatScene& f, const std::vector<DeformedMesh>& edits) {
    ft_context::Temporal& T = c->temporal;
    std::vector<ft_context::Temporal::Snapshot> fresh;
    size_t need = T.snap_used;
    for (const DeformedMesh& e : edits) {
        bool held = false;
        for (const ft_context::Temporal::Snapshot& s : T.snaps) held = held || s.mesh == e.mesh;
        const ftk::RefitMesh m = refit_ranges(f, e.mesh, 0.0);
        if (held || m.n == 0 || (size_t)m.first_global + m.n > f.tris.size() / 9) continue;
        fresh.push_back({e.mesh, (uint32_t)need, m.n});
        need += m.n;
    }
    if (fresh.empty()) return FT_OK;
    if (need > 0xFFFFFFFFull) { c->err = "ft_scene_commit_deformed: more than 2^32 triangles to snapshot"; return FT_ERR_INVALID; }
    int32_t rc;
    if (T.d_snap.bytes < need * 72) {                               // grows by a buffer of the new size that takes over what is kept
        DeviceBuf grown;
        if ((rc = ensure(c, grown, need * 72)) != FT_OK) return rc;
        if (T.snap_used) FT_HIP(c, hipMemcpyAsync(grown.p, T.d_snap.p, T.snap_used * 72, hipMemcpyDeviceToDevice, c->stream));
        FT_HIP(c, hipStreamSynchronize(c->stream));
        T.d_snap.release();
        T.d_snap = grown;
    }
    const double* tris = geo_array(c, kTris).as<double>();
    for (const ft_context::Temporal::Snapshot& s : fresh) {
        const ftk::RefitMesh m = refit_ranges(f, s.mesh, 0.0);
        FT_HIP(c, hipMemcpyAsync(T.d_snap.as<double>() + 9 * (size_t)s.first, tris + 9 * (size_t)m.first_global, (size_t)s.n * 72, hipMemcpyDeviceToDevice, c->stream));
        T.snaps.push_back(s);
    }
    T.snap_used = need;
    return FT_OK;
}

// The page-locked block of a queued call (ft_context::GeoSets::staging): what the call's asynchronous copies take from the host passes
// through it, one piece behind the other on 16 bytes.  The caller has sized it (stage_begin).
struct Stager {
    char* base = nullptr; size_t used = 0, cap = 0;
    const void* put(const void* src, size_t bytes) {
        if (bytes > cap - used) return src;                         // (never: stage_begin counted the same pieces)
        char* at = base + used;
        std::memcpy(at, src, bytes);
        used += (bytes + 15) / 16 * 16;
        return at;
    }
};
// Refit::d_verts of at least `bytes`.  queued: the last queued refit may still read it on `deform`, which is waited for before it grows.
static int32_t ensure_verts(ft_context* c, size_t bytes, bool queued) {
    if (queued && c->refit.d_verts.bytes < std::max<size_t>(bytes, 16) && c->geo.deform) FT_HIP(c, hipStreamSynchronize(c->geo.deform));
    return ensure(c, c->refit.d_verts, bytes);
}

// Morph targets and skinning on one device of the context: the vertices of every `on_device` edit made in d_verts at
// the edit's place - `blended`: k_morph_blend from base and deltas; `skinned`: k_skin behind it, in place, or from the rest shape resident
// beside the skin's index words and slot-major weights (uploaded when the device holds another ft_sg_set_mesh_skin call's / another
// shape's), with this pose's palette (ms[0] += those uploads).
// The blend: the vertices of every `blended` edit blended into d_verts at the edit's
// place, from base and deltas resident in this device's HBM - uploaded here when the device holds none of the node's current
// ft_sg_set_mesh_targets call (ms[0] += that upload).  Only d_verts is written, which no frame reads, so queued frames go on.  lead:
// the context's first device, which also scans every blended mesh, bit for bit fth::scan_mesh, into the edit (ms[1] += blend, scan
// and readback).  The others' blends are left queued on their streams: their refit_device follows on the same stream.
static int32_t morph_device(ft_context* c, const fth::SceneGraph& g, std::vector<DeformedMesh>& edits, double ms[2], bool lead, Stager* stage = nullptr) {
    using clock = std::chrono::steady_clock;
    auto since = [](clock::time_point t0) { return std::chrono::duration<double, std::milli>(clock::now() - t0).count(); };
    int32_t rc;
    FT_HIP(c, hipSetDevice(c->device));
    ft_context::Morph& M = c->morph;
    const auto t0 = clock::now();
    const hipStream_t on = stage ? c->geo.deform : c->stream;
    if ((rc = ensure_verts(c, verts_doubles(g, edits) * 8, stage != nullptr)) != FT_OK) return rc;
    bool uploaded = false;
    size_t blocks = 1, n_scans = 0;
    std::vector<std::vector<double>> staged;                        // slot-major weights, until the stream has taken them
    for (const DeformedMesh& e : edits) {
        if (!e.on_device) continue;
        const fth::GraphNode& n = g.nodes[(size_t)e.node];
        blocks = std::max(blocks, (size_t)ftk::morph_blocks((uint32_t)(n.tris.size() / 9)));
        ++n_scans;
        if (e.skinned) {                                            // indices and weights of the skin, the rest shape where no blend makes the shape, this pose's palette
            ft_context::Skin& S = c->skin;
            ft_context::Skin::Resident* s = nullptr;
            for (ft_context::Skin::Resident& h : S.meshes) if (h.node == e.node) s = &h;
            if (!s) { S.meshes.emplace_back(); s = &S.meshes.back(); s->node = e.node; s->skin_serial = s->rest_serial = ~0ull; s->wstride = 0; s->used_skin = s->used_rest = s->used_palette = 0; }
            const size_t corners = n.tris.size() / 3, J = (size_t)n.skin_influences;
            if (s->skin_serial != n.skin_serial) {
                if ((rc = ensure(c, s->d_index, corners * 4)) != FT_OK || (rc = ensure(c, s->d_weight, J * corners * 8)) != FT_OK) return rc;
                staged.emplace_back(J * corners);
                std::vector<double>& w = staged.back();
                for (size_t k = 0; k < corners; ++k) for (size_t j = 0; j < J; ++j) w[j * corners + k] = n.skin_weight[k * J + j];
                if (corners) {
                    FT_HIP(c, hipMemcpyAsync(s->d_index.p, n.skin_index.data(), corners * 4, hipMemcpyHostToDevice, on));
                    FT_HIP(c, hipMemcpyAsync(s->d_weight.p, w.data(), J * corners * 8, hipMemcpyHostToDevice, on));
                }
                s->skin_serial = n.skin_serial; s->wstride = corners; s->used_skin = corners * 4 + J * corners * 8;
                uploaded = true;
            }
            if (!e.blended && s->rest_serial != n.shape_serial) {
                if ((rc = ensure(c, s->d_rest, n.tris.size() * 8)) != FT_OK) return rc;
                if (!n.tris.empty()) FT_HIP(c, hipMemcpyAsync(s->d_rest.p, n.tris.data(), n.tris.size() * 8, hipMemcpyHostToDevice, on));
                s->rest_serial = n.shape_serial; s->used_rest = n.tris.size() * 8;
                uploaded = true;
            }
            if ((rc = ensure(c, s->d_palette, n.palette.size() * 8)) != FT_OK) return rc;
            FT_HIP(c, hipMemcpyAsync(s->d_palette.p, stage ? stage->put(n.palette.data(), n.palette.size() * 8) : n.palette.data(), n.palette.size() * 8, hipMemcpyHostToDevice, on));
            s->used_palette = n.palette.size() * 8;
            if (!stage) uploaded = true;                            // (a queued call's palette left page-locked memory: the stream orders it, nothing is waited for)
        }
        if (!e.blended) continue;
        ft_context::Morph::Resident* r = nullptr;
        for (ft_context::Morph::Resident& h : M.meshes) if (h.node == e.node) r = &h;
        if (!r) { M.meshes.push_back({e.node, 0, 0, 0, DeviceBuf{}}); r = &M.meshes.back(); }
        if (r->serial != n.targets_serial) {
            const size_t count = n.base.size(), stride = count + (count & 1);
            if ((rc = ensure(c, r->d, (size_t)(n.n_targets + 1) * stride * 8)) != FT_OK) return rc;
            if (count) {
                FT_HIP(c, hipMemcpyAsync(r->d.p, n.base.data(), count * 8, hipMemcpyHostToDevice, on));
                for (int32_t k = 0; k < n.n_targets; ++k)
                    FT_HIP(c, hipMemcpyAsync(r->d.as<double>() + (size_t)(k + 1) * stride, n.deltas.data() + (size_t)k * count, count * 8, hipMemcpyHostToDevice, on));
            }
            r->serial = n.targets_serial; r->stride = stride; r->used = (size_t)(n.n_targets + 1) * count * 8;
            uploaded = true;
        }
    }
    if (uploaded) FT_HIP(c, hipStreamSynchronize(on));
    ms[0] += since(t0);
    const auto t1 = clock::now();
    if (lead && ((rc = ensure(c, M.d_partials, blocks * sizeof(ftk::MorphPartial))) != FT_OK || (rc = ensure(c, M.d_out, n_scans * sizeof(ftk::MorphScanOut))) != FT_OK)) return rc;
    std::vector<ftk::MorphScanOut> out(n_scans);
    size_t k_scan = 0;
    for (const DeformedMesh& e : edits) {
        if (!e.on_device) continue;
        const fth::GraphNode& n = g.nodes[(size_t)e.node];
        double* out = c->refit.d_verts.as<double>() + e.at;
        if (e.blended) {
            const ft_context::Morph::Resident* r = nullptr;
            for (const ft_context::Morph::Resident& h : M.meshes) if (h.node == e.node) r = &h;
            ftk::MorphBlend a{};
            a.resident = r->d.as<double>(); a.out = out; a.count = n.tris.size(); a.stride = r->stride; a.n_targets = n.n_targets;
            for (int32_t k = 0; k < n.n_targets; ++k) a.w[k] = n.weights[(size_t)k];
            ftk::morph_blend(on, a);
        }
        if (e.skinned) {                                            // behind the blend on the stream, in place; else from the rest shape
            const ft_context::Skin::Resident* s = nullptr;
            for (const ft_context::Skin::Resident& h : c->skin.meshes) if (h.node == e.node) s = &h;
            ftk::SkinPose a{};
            a.src = e.blended ? out : s->d_rest.as<double>(); a.out = out; a.index = s->d_index.as<uint32_t>(); a.weight = s->d_weight.as<double>();
            a.palette = s->d_palette.as<double>(); a.corners = n.tris.size() / 3; a.wstride = s->wstride; a.influences = n.skin_influences; a.n_bones = n.n_bones;
            if (n.palette_kind == fth::GraphNode::DualQuaternions) ftk::skin_dq(on, a);   // (the palette holds 8 doubles per bone: DESIGN.md 16.6)
            else ftk::skin(on, a);
        }
        // (one scan after the other on the stream: they share the partials)
        if (lead) ftk::morph_scan(on, out, (uint32_t)(n.tris.size() / 9), M.d_partials.as<ftk::MorphPartial>(), M.d_out.as<ftk::MorphScanOut>() + k_scan++);
    }
    FT_HIP(c, hipGetLastError());
    if (lead && n_scans) {
        FT_HIP(c, hipMemcpyAsync(out.data(), M.d_out.p, n_scans * sizeof(ftk::MorphScanOut), hipMemcpyDeviceToHost, on));
        FT_HIP(c, hipStreamSynchronize(on));
        k_scan = 0;
        for (DeformedMesh& e : edits) {
            if (!e.on_device) continue;
            const ftk::MorphScanOut& o = out[k_scan++];
            for (int k = 0; k < 6; ++k) e.scan.bounds[k] = o.bounds[k];
            e.scan.extent = o.extent; e.scan.finite = o.finite != 0.0;
        }
        ms[1] += since(t1);
    }
    return FT_OK;
}
// fth::ls_pair_extent(vertices = true) of a blended mesh about `centre`, reduced on the context's first device from the vertices
// morph_device left in d_verts: a maximum of non-negative finite values, so the order cannot show.  ms[1] += kernels and readback.
static int32_t morph_pair_extent(ft_context* c, const fth::SceneGraph& g, const DeformedMesh& e, const double centre[3], double* R, double ms[2]) {
    const auto t0 = std::chrono::steady_clock::now();
    int32_t rc;
    FT_HIP(c, hipSetDevice(c->device));
    ft_context::Morph& M = c->morph;
    const uint32_t n = (uint32_t)(g.nodes[(size_t)e.node].tris.size() / 9);
    if ((rc = ensure(c, M.d_partials, (size_t)ftk::morph_blocks(n) * 8)) != FT_OK) return rc;   // (the scan's partials hold more: nothing is allocated here)
    double* partials = M.d_partials.as<double>();
    double* out = M.d_out.as<double>();
    ftk::morph_extent(c->stream, c->refit.d_verts.as<double>() + e.at, n, centre, partials, out);
    FT_HIP(c, hipGetLastError());
    FT_HIP(c, hipMemcpyAsync(R, out, 8, hipMemcpyDeviceToHost, c->stream));
    FT_HIP(c, hipStreamSynchronize(c->stream));
    ms[1] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return FT_OK;
}

// What the context's first device decides for the others ("refit_rebuild_percent"): per edit whether its tree is rebuilt in place, and the
// tallest tree the rebuilds made.
struct RebuildPlan { std::vector<uint8_t> rebuild; uint32_t tallest = 0; };

// The refit of `edits` on one device of the context: `f` is the held scene with the new cull records and leaves already in it, `g` the
// graph with the new vertices.  ms[0] += uploads and the rest, ms[1] += the kernels.  lead: the context's first device, which measures
// the costs and fills `plan`; the others carry the plan out.
static int32_t refit_device(ft_context* c, const fth::FlatScene& f, const fth::SceneGraph& g, const std::vector<DeformedMesh>& edits, double ms[2], bool lead, RebuildPlan& plan) {
    using clock = std::chrono::steady_clock;
    auto since = [](clock::time_point t0) { return std::chrono::duration<double, std::milli>(clock::now() - t0).count(); };
    int32_t rc;
    FT_HIP(c, hipSetDevice(c->device));
    const auto t0 = clock::now();
    // frames still queued trace the scene this refit rewrites (as upload_scene)
    if (any_queued(c)) { if ((rc = retire_queued(c)) != FT_OK) return rc; c->accum_open = false; }
    if ((rc = drain_frame_streams(c)) != FT_OK) return rc;
    if (c->side) FT_HIP(c, hipStreamSynchronize(c->side));
    ft_context::Refit& R = c->refit;
    const bool first = !R.ready;
    if (first) {
        if ((rc = ensure(c, R.d_parent_node, f.nodes.size() * 4)) != FT_OK || (rc = ensure(c, R.d_arrived, f.nodes.size() * 4)) != FT_OK ||
            (rc = ensure(c, R.d_parent_leaf, f.bsp_leaves.size() * 4)) != FT_OK || (rc = ensure(c, R.d_leaf_boxes, f.bsp_leaves.size() * 48)) != FT_OK ||
            (rc = upload(c, R.d_wide_node, f.wide_node)) != FT_OK) return rc;
        FT_HIP(c, hipMemsetAsync(R.d_parent_node.p, 0xFF, R.d_parent_node.bytes, c->stream));
        FT_HIP(c, hipMemsetAsync(R.d_parent_leaf.p, 0xFF, R.d_parent_leaf.bytes, c->stream));
    }
    const ftk::RefitArrays A = refit_arrays(c);
    if ((rc = ensure(c, R.d_verts, verts_doubles(g, edits) * 8)) != FT_OK) return rc;   // (no larger than what a blend has already written into)
    for (const DeformedMesh& e : edits) {
        if (e.on_device) continue;                                  // k_morph_blend has filled them
        const std::vector<double>& v = g.nodes[(size_t)e.node].vertices();
        if (!v.empty()) FT_HIP(c, hipMemcpyAsync(R.d_verts.as<double>() + e.at, v.data(), v.size() * 8, hipMemcpyHostToDevice, c->stream));
    }
    // "temporal_follow_deformed": what the open accumulation's history saw of each edited mesh, before the first refit since the last
    // accumulate overwrites it (later ones keep it, so several deformations between two accumulates compose)
    if (c->opt.temporal_follow_deformed && c->temporal.open && c->temporal.calls > 0 && (rc = snapshot_records(c, f, edits)) != FT_OK) return rc;
    // (into the live pose set, which dev_scene points into: d_scene's own arrays unless a queued commit has moved on)
    if ((rc = upload(c, pose_array(c, kLeaves), f.leaves)) != FT_OK || (rc = upload(c, pose_array(c, kCulls), f.culls)) != FT_OK) return rc;
    cull_items_image(f, c->cull_items_and_rows);
    if ((rc = upload(c, pose_array(c, kCullItems), c->cull_items_and_rows)) != FT_OK) return rc;
    FT_HIP(c, hipStreamSynchronize(c->stream));
    ms[0] += since(t0);
    const auto t1 = clock::now();
    if (lead && (rc = record_built_costs(c, f)) != FT_OK) return rc;   // of the trees as they were built: nothing has been rewritten yet
    if (first) {
        for (uint32_t k = 0; k < (uint32_t)f.meshes.size(); ++k) if (refittable(f, k)) ftk::refit_parents(c->stream, A, refit_ranges(f, k, 0.0));
        R.ready = true;
    }
    for (const DeformedMesh& e : edits) {
        const ftk::RefitMesh m = refit_ranges(f, e.mesh, 1e-7 * e.scan.extent + 1e-300);
        if (m.node_count) FT_HIP(c, hipMemsetAsync(R.d_arrived.as<uint32_t>() + m.node_first, 0, (size_t)m.node_count * 4, c->stream));
        ftk::refit_mesh(c->stream, A, m, R.d_verts.as<double>() + e.at);
        // (the live geometry set now holds this call's refit of the mesh: the other sets are behind it)
        if (!c->geo.sets.empty() && e.mesh < c->geo.sets[(size_t)c->geo.live].wrote.size()) c->geo.sets[(size_t)c->geo.live].wrote[e.mesh] = ++c->geo.serial;
    }
    FT_HIP(c, hipGetLastError());
    FT_HIP(c, hipStreamSynchronize(c->stream));
    // "refit_rebuild_percent": a device-built tree whose cost has grown past the host's threshold is built again in place
    const int64_t percent = c->opt.refit_rebuild_percent;
    if (lead) plan.rebuild.assign(edits.size(), 0);
    for (size_t k = 0; percent > 0 && k < edits.size(); ++k) {
        const uint32_t mesh = edits[k].mesh;
        const fth::FlatScene::BvhJob* j = job_of(f, mesh);
        if (!j || !refittable(f, mesh)) continue;                   // host-built trees are measured (ft_scene_tree_quality) and never rebuilt
        if (lead) {
            double now = 0.0;
            if ((rc = measure_cost(c, f, mesh, &now)) != FT_OK) return rc;
            plan.rebuild[k] = now * 100.0 > (double)percent * c->tree_quality[mesh].cost_built ? 1 : 0;
        }
        if (!plan.rebuild[k]) continue;
        uint32_t height = 0;
        if ((rc = rebuild_in_place(c, f, *j, &height)) != FT_OK) return rc;
        // (every other geometry set holds the old tree's child words: the next queued call that picks one carries the mesh over whole)
        for (size_t k2 = 0; k2 < c->geo.sets.size(); ++k2) if ((int)k2 != c->geo.live && mesh < c->geo.sets[k2].wrote.size()) c->geo.sets[k2].wrote[mesh] = ~0ull;
        plan.tallest = std::max(plan.tallest, height);
        if (lead) {
            ft_context::TreeQuality& q = c->tree_quality[mesh];
            if ((rc = measure_cost(c, f, mesh, &q.cost_built)) != FT_OK) return rc;
            ++q.rebuilds;
        }
    }
    ms[1] += since(t1);
    c->zero_signature[0] = c->zero_signature[1] = 0;                // the blocks k_classify finishes are another scene's
    c->committed = true;
    ++c->commit_serial; c->staged_hint = -1;
    return FT_OK;
}

// ------------------------------------------------------------------------------------------ moving lights (ft_scene_commit_lights)
// What the first ft_scene_commit_lights after a full commit reads off `f` as that commit left it (ft_context::LightSpace): the pairs that
// have a tree, what of their records does not depend on the direction, and each tree's 4-wide nodes by level, deepest first.
static void derive_light_space_tables(const fth::FlatScene& f, ft_context::LightSpace& T) {
    T.pairs.clear(); T.order.clear(); T.src.clear();
    T.base_node_words = f.ls_nodes.size(); T.base_tri_doubles = f.ls_tris.size();
    const size_t n_nodes = f.ls_nodes.size() / ftd::kLsNodeWords, n_recs = f.ls_pairs.size() / ftd::kLsPairDoubles;
    std::vector<uint8_t> seen(n_nodes, 0);
    for (uint32_t leaf = 0; leaf < (uint32_t)f.leaves.size(); ++leaf) {
        const ftd::Leaf& L = f.leaves[leaf];
        if (L.ls_pairs == ~0u || L.kind != ftd::LK_MESH || L.mesh >= f.meshes.size() || f.meshes[L.mesh].root >= 0) continue;
        const size_t bl = (size_t)~f.meshes[L.mesh].root;
        if (bl >= f.bsp_leaves.size()) continue;
        const ftd::BspLeaf src = f.bsp_leaves[bl];
        if ((size_t)src.first_tri + src.n_tris > f.tris.size() / 9) continue;
        const double* mb = &f.mesh_bounds[6 * (size_t)L.mesh];
        const double c[3] = {0.5 * (mb[0] + mb[3]), 0.5 * (mb[1] + mb[4]), 0.5 * (mb[2] + mb[5])};
        const double R = fth::ls_pair_extent(&f.tris[9 * (size_t)src.first_tri], src.n_tris, false, c);   // as build_light_space sums it: it does not depend on the frame
        for (uint32_t l = 0; l < (uint32_t)f.lights.size(); ++l) {
            const size_t rec = (size_t)L.ls_pairs + l;
            if (f.lights[l].kind != ftd::LT_DIRECTIONAL || rec >= n_recs) continue;
            int32_t root;
            std::memcpy(&root, &f.ls_pairs[ftd::kLsPairDoubles * rec + 14], 4);
            if (root < 0 || (size_t)root >= n_nodes || seen[(size_t)root]) continue;   // none at the commit: none until the next one
            ft_context::LightSpace::Pair P{};
            P.rec = (uint32_t)rec; P.leaf = leaf; P.light = l; P.root = root; P.R = R; P.first_tri = src.first_tri; P.n_tris = src.n_tris;
            P.mesh = L.mesh; P.ls_first = ~0u; P.src_at = (uint32_t)T.src.size(); P.deformed = false;
            for (int q = 0; q < 3; ++q) { P.c[q] = c[q]; P.v0[q] = f.lights[l].v[q]; }
            std::memcpy(P.w2m0, L.w2m, sizeof P.w2m0); P.flags0 = L.flags;
            std::memcpy(P.rec0, &f.ls_pairs[ftd::kLsPairDoubles * rec], sizeof P.rec0);
            // breadth first: `level` holds one level of the tree; the levels are then laid out deepest first
            std::vector<std::vector<uint32_t>> by_level;
            std::vector<uint32_t> level{(uint32_t)root};
            seen[(size_t)root] = 1;
            while (!level.empty()) {
                std::vector<uint32_t> next;
                for (uint32_t n : level) for (int k = 0; k < 4; ++k) {
                    const int32_t ch = (int32_t)f.ls_nodes[(size_t)ftd::kLsNodeWords * n + 20 + k];
                    if (ch < 0 && ch != INT32_MIN) P.ls_first = std::min(P.ls_first, (uint32_t)~ch >> 3);   // the builder appended the tree's leaves in one run
                    if (ch < 0 || (size_t)ch >= n_nodes || seen[(size_t)ch]) continue;   // a leaf, an empty slot (or no tree at all)
                    seen[(size_t)ch] = 1;
                    next.push_back((uint32_t)ch);
                }
                by_level.push_back(std::move(level));
                level = std::move(next);
            }
            for (size_t d = by_level.size(); d-- > 0;) {
                P.levels.push_back({(uint32_t)T.order.size(), (uint32_t)by_level[d].size()});
                T.order.insert(T.order.end(), by_level[d].begin(), by_level[d].end());
            }
            // the triangles the tree's leaf records copy; a run that does not lie in ls_src leaves the pair without them, and a deformed
            // commit then strips its leaf as it did before "deform_light_space"
            if ((size_t)P.ls_first + P.n_tris <= f.ls_src.size() && (size_t)P.ls_first + P.n_tris <= f.ls_tris.size() / 9)
                T.src.insert(T.src.end(), f.ls_src.begin() + P.ls_first, f.ls_src.begin() + P.ls_first + P.n_tris);
            else P.ls_first = ~0u;
            T.pairs.push_back(std::move(P));
        }
    }
    T.ready = true;
}

// Is the pair still the full commit's - may it have that commit's record (rec0) and, with it, the grid that lies where that commit put it?
// Only with the light at that commit's direction (`v`: the light's direction now) over the leaf in that commit's pose, its mesh not
// deformed and its tree not retreed since.  ft_scene_commit_lights, ft_scene_commit_deformed and ft_scene_commit_moved all ask here.
static bool full_commits_pair(const fth::FlatScene& f, const ft_context::LightSpace::Pair& P, const double v[3]) {
    const ftd::Leaf& L = f.leaves[P.leaf];
    return !P.deformed && !P.retreed && std::memcmp(v, P.v0, sizeof P.v0) == 0 && std::memcmp(L.w2m, P.w2m0, sizeof P.w2m0) == 0 && ((L.flags ^ P.flags0) & ftd::LF_XFORM) == 0u;
}

// One pair's share of an ft_scene_commit_lights: its frame; whether its tree is refit (its direction changed in this call); whether its
// grid is built again behind the arrays of the full commit (every pair whose direction is not that commit's, in every call that
// turns any light: the region is laid out anew each time, so it never grows), and what the context's first device decided for that grid.
// gather: its mesh was refit in this call (ft_scene_commit_deformed, "deform_light_space"), so the tree's leaf records are copied again
// from the mesh's list-order records before anything reads them - also where the record is unusable and nothing else is done, so that the
// tree is current whenever a later call refits its boxes.
// retree ("light_space_retree"): the tree that is refit is the one in the pair's block, over leaf records sorted again
// along the Morton curve of the current projection before they are copied.
struct LightJob {
    const ft_context::LightSpace::Pair* pair; ftk::LsFrame frame; bool refit, regrid;
    bool gather = false, retree = false;
    bool grid = false; float s = 0.0f; uint32_t nu = 0, nv = 0, entries = 0, at = 0, tri_at = 0;
    size_t slot = 0;                                                // of the device's per-pair scratch (ft_context::LightSpace::d_ebox, d_counts)
};

// The record of a pair that is not the full commit's any more - its light points elsewhere, or its mesh has been deformed - derived again
// from the pair's current centre and R as build_light_space derives it, and the pair's job: its tree refit (`refit`: the direction or the
// vertices changed in this call), its grid built again behind the full commit's arrays (`grids`: the scene has them).  No usable frame,
// or R from 2e29 on: root INT32_MIN and no grid - its rays walk the BVH, and the tree's nodes and records stay where they are.
// `retree`: the option is on - a pair that is refit here and has a block takes the block's tree from now on.
static void moved_pair_job(fth::FlatScene& f, ft_context::LightSpace::Pair& P, const ftd::Light& light, bool refit, bool gather, bool grids, bool retree, std::vector<LightJob>& jobs,
                           size_t& n_regrid) {
    double* rec = &f.ls_pairs[(size_t)ftd::kLsPairDoubles * P.rec];
    LightJob j{&P, {}, false, false};
    j.gather = gather;
    for (int k = 0; k < ftd::kLsPairDoubles; ++k) rec[k] = 0.0;
    fth::LsPairFrame fr;
    // (every projected coordinate is at most R in size: the builder's finiteness test, five of them below 1e30, holds with R < 2e29)
    const bool usable = fth::ls_pair_frame(f.leaves[P.leaf], light, fr) && P.R < 2e29;
    if (usable && refit && retree && P.block != ~0u && P.ls_first != ~0u) {
        j.retree = true;
        if (!P.retreed) { P.retreed = true; P.root = (int32_t)P.block; P.levels = P.block_levels; }
    }
    const int32_t root = usable ? P.root : INT32_MIN;               // none: the tree's nodes and records stay where they are for the direction's return
    std::memcpy(&rec[14], &root, 4);
    if (usable) {
        for (int q = 0; q < 3; ++q) { rec[q] = j.frame.U[q] = fr.U[q]; rec[3 + q] = j.frame.V[q] = fr.V[q]; rec[6 + q] = j.frame.D[q] = fr.D[q]; rec[9 + q] = j.frame.c[q] = P.c[q]; }
        rec[12] = fr.k_rel; rec[13] = (fr.k_rel + 1e-6) * P.R + 1e-20;
        j.frame.pad = 1e-7 * P.R + 1e-30;
        j.refit = refit; j.regrid = grids;
        if (j.regrid) j.slot = n_regrid++;
    }
    if (usable || gather) jobs.push_back(j);
}

// "light_space_retree", the first call under the option since the full commit: where every pair's block of nodes lies behind that commit's
// nodes (ft_ls_topology.h), the blocks' child words, and their levels behind the trees' in `order`.
static void lay_retree_blocks(ft_context::LightSpace& T) {
    std::vector<uint32_t> n(T.pairs.size(), 0u), block;
    for (size_t k = 0; k < T.pairs.size(); ++k) if (T.pairs[k].ls_first != ~0u && T.pairs[k].src_at + (size_t)T.pairs[k].n_tris <= T.src.size()) n[k] = T.pairs[k].n_tris;
    const uint64_t nodes = fth::ls_retree_layout(n, T.base_node_words / ftd::kLsNodeWords, (uint64_t)T.base_node_words * 4 + (uint64_t)T.base_tri_doubles * 8, ftd::kLsMaxBytes, block);
    T.block_init.assign((size_t)nodes * ftd::kLsNodeWords, fth::kLsTopoNaN);
    fth::LsTopology topo;
    for (size_t k = 0; k < T.pairs.size(); ++k) {
        ft_context::LightSpace::Pair& P = T.pairs[k];
        if (block[k] == ~0u || !fth::ls_retree_topology(P.n_tris, P.ls_first, block[k], topo)) continue;
        P.block = block[k]; P.block_nodes = (uint32_t)(topo.nodes.size() / ftd::kLsNodeWords);
        std::copy(topo.nodes.begin(), topo.nodes.end(), T.block_init.begin() + ((size_t)block[k] * ftd::kLsNodeWords - T.base_node_words));
        for (const auto& lv : topo.levels) P.block_levels.push_back({(uint32_t)T.order.size() + lv.first, lv.second});
        T.order.insert(T.order.end(), topo.order.begin(), topo.order.end());
    }
    T.block_words = T.block_init.size();
    T.blocks_laid = true;
}

// build_grid's decisions for one pair (ft_scene.cpp), its host loops run as passes on the device: readback 1 Ru and Rv, readback 2 the
// entries under each candidate of the attempt loop, readback 3 the fullest cell.  `bytes`: what the arrays hold so far, against the cap.
// The pair's entry boxes and cell counts stay in its scratch slot for the pass that writes the grid.
static int32_t plan_grid(ft_context* c, LightJob& j, uint64_t& bytes) {
    ft_context::LightSpace& L = c->lightspace;
    DeviceBuf& ebox = L.d_ebox[j.slot];
    DeviceBuf& counts = L.d_counts[j.slot];
    const uint32_t n = j.pair->n_tris;
    int32_t rc;
    if ((rc = ensure(c, ebox, (size_t)n * 20)) != FT_OK) return rc;
    const double* tris = geo_array(c, kTris).as<double>() + 9 * (size_t)j.pair->first_tri;
    uint32_t* small = L.d_small.as<uint32_t>();                     // [0] Ru, [1] Rv, [2] the fullest cell, [4 ..] eight 64-bit sums
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(small + 4);
    FT_HIP(c, hipMemsetAsync(small, 0, 128, c->stream));
    ftk::ls_grid_entries(c->stream, tris, n, j.frame, ebox.as<float>(), small);
    float ruv[2];
    FT_HIP(c, hipMemcpyAsync(ruv, small, 8, hipMemcpyDeviceToHost, c->stream));
    FT_HIP(c, hipStreamSynchronize(c->stream));
    // build_grid's own arithmetic from here on
    const double Ru = (double)ruv[0], Rv = (double)ruv[1];
    const double side = 2.0 * std::max(Ru, Rv);
    if (!(side > 0.0)) return FT_OK;
    const double h = std::max(std::sqrt(4.0 * Ru * Rv / (double)n), side / 1024.0);
    float s = (float)(1.0 / h);
    ftk::LsGridCandidates C{};
    for (int attempt = 0; attempt < 8 && s > 0.0f; ++attempt, s *= 0.75f) {
        C.s[C.n] = s;
        C.nu[C.n] = (uint32_t)std::min(1024.0, std::max(1.0, std::ceil(2.0 * Ru * (double)s)));
        C.nv[C.n] = (uint32_t)std::min(1024.0, std::max(1.0, std::ceil(2.0 * Rv * (double)s)));
        ++C.n;
    }
    if (C.n == 0) return FT_OK;
    ftk::ls_grid_count(c->stream, ebox.as<float>(), n, C, sums);
    unsigned long long got[8];
    FT_HIP(c, hipMemcpyAsync(got, sums, sizeof got, hipMemcpyDeviceToHost, c->stream));
    FT_HIP(c, hipStreamSynchronize(c->stream));
    int a = 0;
    while (a < C.n && !((uint64_t)C.nu[a] * C.nv[a] <= 2 * (uint64_t)n && got[a] <= (uint64_t)ftd::kLsGridEntriesPerTri * n)) ++a;
    if (a == C.n || (uint64_t)C.nu[a] * C.nv[a] < 2) return FT_OK;
    const uint32_t cells = C.nu[a] * C.nv[a];
    if ((rc = ensure(c, counts, (size_t)cells * 4)) != FT_OK) return rc;
    FT_HIP(c, hipMemsetAsync(counts.p, 0, (size_t)cells * 4, c->stream));
    ftk::ls_grid_cell_counts(c->stream, ebox.as<float>(), n, C.s[a], C.nu[a], C.nv[a], counts.as<uint32_t>(), small + 2);
    uint32_t fullest = 0;
    FT_HIP(c, hipMemcpyAsync(&fullest, small + 2, 4, hipMemcpyDeviceToHost, c->stream));
    FT_HIP(c, hipStreamSynchronize(c->stream));
    if (fullest > ftd::kLsGridMaxCell) return FT_OK;
    const uint64_t need = (uint64_t)cells * 16 + got[a] * (72 + 20) + ftd::kLsNodeWords * 4;
    if (bytes + need > ftd::kLsMaxBytes) return FT_OK;
    bytes += need;
    j.grid = true; j.s = C.s[a]; j.nu = C.nu[a]; j.nv = C.nv[a]; j.entries = (uint32_t)got[a];
    return FT_OK;
}

// The light-space structures of one device of the context brought up to the pair records in `f` (the grid words of the jobs' records
// excepted: the first device, `lead`, decides them here and writes them into f; the others carry them out), for ft_scene_commit_lights
// and ft_scene_commit_deformed alike (`who` names the caller in an error).  Nothing else may be reading or writing the scene's arrays:
// the caller has retired the queued frames and drained the streams.  On the stream, in order: the leaf records of the jobs that gather,
// the trees of the jobs that refit written again in their frames, the grids laid out anew behind the full commit's arrays
// (ft_lightspace.hip; `relay`: the scene has grids and what one of them must hold changed), the pair records, the edge records.
// ms[0] += uploads and the rest, ms[1] += the kernels and their readbacks.
static int32_t rebuild_light_space(ft_context* c, fth::FlatScene& f, const ft_context::LightSpace& T, std::vector<LightJob>& jobs, bool relay, bool lead, double ms[2], const char* who) {
    using clock = std::chrono::steady_clock;
    auto since = [](clock::time_point t0) { return std::chrono::duration<double, std::milli>(clock::now() - t0).count(); };
    int32_t rc;
    const auto t0 = clock::now();
    DeviceBuf* B = c->d_scene;
    ft_context::LightSpace& L = c->lightspace;
    if (L.node_words == 0) { L.node_words = T.base_node_words; L.tri_doubles = T.base_tri_doubles; }   // the first call since the upload
    if (!jobs.empty() && (!L.order_uploaded || L.order_words != T.order.size())) {   // (the blocks' levels were appended since: "light_space_retree")
        if ((rc = upload(c, L.d_order, T.order)) != FT_OK) return rc;
        L.order_uploaded = true; L.order_words = T.order.size();
    }
    bool gathers = false, retrees = false;
    for (const LightJob& j : jobs) { gathers = gathers || j.gather || j.retree; retrees = retrees || j.retree; }
    if (gathers && !L.src_uploaded) {
        if ((rc = upload(c, L.d_src, T.src)) != FT_OK) return rc;
        L.src_uploaded = true;
    }
    FT_HIP(c, hipStreamSynchronize(c->stream));
    ms[0] += since(t0);
    const auto t1 = clock::now();
    if (B[kLsNodes].bytes < L.node_words * 4 || B[kLsTris].bytes < L.tri_doubles * 8 || L.node_words < T.base_node_words + L.block_words_here || L.tri_doubles < T.base_tri_doubles ||
        geo_array(c, kTris).bytes < f.tris.size() * 8) { c->err = std::string(who) + ": a scene array in device memory is smaller than the flattened one"; return FT_ERR_STATE; }
    bool regrid = relay;                                            // a light turned: the region behind the full commit's arrays is laid out anew, be it to nothing
    if (retrees && L.block_words_here != T.block_words) {
        // "light_space_retree", this device's first retree since the full commit: the blocks take their place behind that commit's nodes.
        // What lay there - the grids of earlier calls - is laid out anew below, behind the blocks: every pair that has one there has a job.
        const size_t front = T.base_node_words + T.block_words;
        DeviceBuf nodes;
        if ((rc = ensure(c, nodes, front * 4)) != FT_OK) { nodes.release(); return rc; }
        if (hipMemcpyAsync(nodes.p, B[kLsNodes].p, T.base_node_words * 4, hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(nodes.as<uint32_t>() + T.base_node_words, T.block_init.data(), T.block_words * 4, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) { nodes.release(); c->err = std::string(who) + ": laying out the retree blocks failed"; return FT_ERR_HIP; }
        B[kLsNodes].release();
        B[kLsNodes] = nodes;
        c->dev_scene.ls_nodes = static_cast<std::remove_reference_t<decltype(c->dev_scene.ls_nodes)>>(nodes.p);
        L.node_words = front; L.block_words_here = T.block_words;
        L.rewritten = true; regrid = true;
    }
    const size_t front = T.base_node_words + L.block_words_here;    // the full commit's nodes and the blocks: what every call carries forward
    const uint32_t n_nodes = (uint32_t)(front / ftd::kLsNodeWords), n_tris = (uint32_t)(T.base_tri_doubles / 9);   // the trees lie in that part
    size_t slots = 0;
    for (const LightJob& j : jobs) {                                // (a pair's tree lies apart from every other's: one pass over the jobs keeps each tree's order)
        if (j.regrid) slots = std::max(slots, j.slot + 1);
        const bool sorts = j.retree && j.pair->src_at + (size_t)j.pair->n_tris <= T.src.size() && (size_t)j.pair->first_tri + j.pair->n_tris <= f.tris.size() / 9;
        if (sorts) {
            // the pair's part of d_src becomes its list-order triangles sorted by the Morton code of their centres in the job's frame
            // (stable: equal codes keep the list order); the gather below and every later one copy the records in that order
            const uint32_t n = j.pair->n_tris;
            size_t sort_bytes = 0;
            if (ftk::ls_sort_pairs(c->stream, nullptr, nullptr, nullptr, nullptr, n, nullptr, &sort_bytes) != hipSuccess) { c->err = std::string(who) + ": sizing the sort failed"; return FT_ERR_HIP; }
            if ((rc = ensure(c, L.d_keys, (size_t)n * 12)) != FT_OK || (rc = ensure(c, L.d_sort, sort_bytes)) != FT_OK) return rc;
            uint32_t* keys = L.d_keys.as<uint32_t>();               // n keys, n sorted keys, n values
            ftk::ls_morton_keys(c->stream, geo_array(c, kTris).as<double>(), (uint32_t)(f.tris.size() / 9), j.pair->first_tri, n, j.frame, j.pair->R, keys, keys + 2 * (size_t)n);
            if (ftk::ls_sort_pairs(c->stream, keys, keys + n, keys + 2 * (size_t)n, L.d_src.as<uint32_t>() + j.pair->src_at, n, L.d_sort.p, &sort_bytes) != hipSuccess) {
                c->err = std::string(who) + ": the sort failed"; return FT_ERR_HIP;
            }
        }
        if ((j.gather || sorts) && j.pair->src_at + (size_t)j.pair->n_tris <= T.src.size()) {
            ftk::ls_gather(c->stream, geo_array(c, kTris).as<double>(), (uint32_t)(f.tris.size() / 9), j.pair->first_tri, j.pair->n_tris, L.d_src.as<uint32_t>() + j.pair->src_at, j.pair->n_tris,
                           B[kLsTris].as<double>(), n_tris, j.pair->ls_first);
            L.rewritten = true;
        }
        if (!j.refit) continue;
        for (const auto& lv : j.pair->levels)                       // deepest level first: a node's children are done before it
            ftk::ls_refit_level(c->stream, B[kLsNodes].as<uint32_t>(), n_nodes, B[kLsTris].as<double>(), n_tris, L.d_order.as<uint32_t>() + lv.first, lv.second, j.frame);
        L.rewritten = true;
    }
    FT_HIP(c, hipGetLastError());
    size_t words = front, doubles = T.base_tri_doubles;             // the arrays' sizes: the full commit's part and the blocks, the grids behind them
    if (regrid) {
        if (L.d_ebox.size() < slots) { L.d_ebox.resize(slots); L.d_counts.resize(slots); }
        if ((rc = ensure(c, L.d_small, 128)) != FT_OK) return rc;
        if (lead) {                                                 // the decisions that need a readback, and with them the layout
            uint64_t bytes = (uint64_t)front * 4 + (uint64_t)T.base_tri_doubles * 8;
            size_t at = front, recs = T.base_tri_doubles / 9;
            for (LightJob& j : jobs) {
                if (!j.regrid) continue;
                if ((rc = plan_grid(c, j, bytes)) != FT_OK) return rc;
                if (!j.grid) continue;
                j.at = (uint32_t)at; j.tri_at = (uint32_t)recs;
                const size_t own = 4 * (size_t)j.nu * j.nv + 5 * (size_t)j.entries;
                at += (own + ftd::kLsNodeWords - 1) / ftd::kLsNodeWords * ftd::kLsNodeWords;   // padded to a whole node, as build_grid pads
                recs += j.entries;
                uint32_t w[3] = {j.at, 0u, j.nu | j.nv << 16};
                std::memcpy(&w[1], &j.s, 4);
                std::memcpy(reinterpret_cast<char*>(&f.ls_pairs[(size_t)ftd::kLsPairDoubles * j.pair->rec + 14]) + 4, w, sizeof w);
            }
        }
        for (const LightJob& j : jobs) {
            if (!j.grid) continue;
            const size_t own = 4 * (size_t)j.nu * j.nv + 5 * (size_t)j.entries;
            words = std::max(words, (size_t)j.at + (own + ftd::kLsNodeWords - 1) / ftd::kLsNodeWords * ftd::kLsNodeWords);
            doubles = std::max(doubles, 9 * ((size_t)j.tri_at + j.entries));
        }
        if (words == front && doubles == T.base_tri_doubles && words == L.node_words && doubles == L.tri_doubles) regrid = false;   // no grid before, none now
    }
    if (regrid) {
        // Fresh arrays of exactly that size: the full commit's part as it lies in HBM now (the refit trees in it), the grids behind it.
        DeviceBuf nodes, tris;
        if ((rc = ensure(c, nodes, words * 4)) != FT_OK || (rc = ensure(c, tris, doubles * 8)) != FT_OK) { nodes.release(); tris.release(); return rc; }
        const auto fail = [&](int32_t code) { nodes.release(); tris.release(); return code; };
        if (hipMemcpyAsync(nodes.p, B[kLsNodes].p, front * 4, hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(tris.p, B[kLsTris].p, T.base_tri_doubles * 8, hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
            (words > front && hipMemsetAsync(nodes.as<uint32_t>() + front, 0, (words - front) * 4, c->stream) != hipSuccess) ||
            (doubles > T.base_tri_doubles && hipMemsetAsync(tris.as<double>() + T.base_tri_doubles, 0, (doubles - T.base_tri_doubles) * 8, c->stream) != hipSuccess)) {
            c->err = std::string(who) + ": copying the light-space arrays failed"; return fail(FT_ERR_HIP);
        }
        for (const LightJob& j : jobs) {
            if (!j.grid) continue;
            const uint32_t n = j.pair->n_tris, cells = j.nu * j.nv;
            const double* mesh = geo_array(c, kTris).as<double>() + 9 * (size_t)j.pair->first_tri;
            size_t scan_bytes = 0;
            if (ftk::ls_grid_scan(c->stream, nullptr, nullptr, cells, nullptr, &scan_bytes) != hipSuccess) { c->err = std::string(who) + ": sizing the scan failed"; return fail(FT_ERR_HIP); }
            DeviceBuf& ebox = L.d_ebox[j.slot];
            DeviceBuf& counts = L.d_counts[j.slot];
            if ((rc = ensure(c, ebox, (size_t)n * 20)) != FT_OK || (rc = ensure(c, counts, (size_t)cells * 4)) != FT_OK || (rc = ensure(c, L.d_first, (size_t)cells * 4)) != FT_OK ||
                (rc = ensure(c, L.d_cursor, (size_t)cells * 4)) != FT_OK || (rc = ensure(c, L.d_idx, (size_t)j.entries * 4)) != FT_OK || (rc = ensure(c, L.d_scan, scan_bytes)) != FT_OK) return fail(rc);
            if (hipMemsetAsync(L.d_cursor.p, 0, (size_t)cells * 4, c->stream) != hipSuccess) { c->err = std::string(who) + ": hipMemsetAsync failed"; return fail(FT_ERR_HIP); }
            if (!lead) {                                            // (the first device's slot holds both since plan_grid)
                if (hipMemsetAsync(counts.p, 0, (size_t)cells * 4, c->stream) != hipSuccess) { c->err = std::string(who) + ": hipMemsetAsync failed"; return fail(FT_ERR_HIP); }
                ftk::ls_grid_entries(c->stream, mesh, n, j.frame, ebox.as<float>(), nullptr);
                ftk::ls_grid_cell_counts(c->stream, ebox.as<float>(), n, j.s, j.nu, j.nv, counts.as<uint32_t>(), nullptr);
            }
            if (ftk::ls_grid_scan(c->stream, counts.as<uint32_t>(), L.d_first.as<uint32_t>(), cells, L.d_scan.p, &scan_bytes) != hipSuccess) { c->err = std::string(who) + ": the scan failed"; return fail(FT_ERR_HIP); }
            ftk::ls_grid_emit(c->stream, ebox.as<float>(), mesh, n, j.s, j.nu, j.nv, counts.as<uint32_t>(), L.d_first.as<uint32_t>(), L.d_cursor.as<uint32_t>(), L.d_idx.as<uint32_t>(),
                              j.entries, nodes.as<uint32_t>(), j.at, tris.as<double>(), j.tri_at);
        }
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { c->err = std::string(who) + ": the grid kernels failed"; return fail(FT_ERR_HIP); }
        // nothing reads the old arrays any more: the streams were drained above
        B[kLsNodes].release(); B[kLsTris].release();
        B[kLsNodes] = nodes; B[kLsTris] = tris;
        ftk::DevScene& S = c->dev_scene;
        S.ls_nodes = static_cast<std::remove_reference_t<decltype(S.ls_nodes)>>(nodes.p);
        S.ls_tris = static_cast<std::remove_reference_t<decltype(S.ls_tris)>>(tris.p);
        L.node_words = words; L.tri_doubles = doubles;
        L.rewritten = true;
    }
    FT_HIP(c, hipStreamSynchronize(c->stream));
    ms[1] += since(t1);
    const auto t2 = clock::now();
    if ((rc = upload(c, B[kLsPairs], f.ls_pairs)) != FT_OK) return rc;
    FT_HIP(c, hipStreamSynchronize(c->stream));
    ms[0] += since(t2);
    // the edge records of the grids as they lie now: the rebuilt ones, and the full commit's under the frames the refit gave their pairs
    const auto t3 = clock::now();
    if (!jobs.empty() && (rc = build_ls_edges(c, f.ls_pairs, L.node_words, L.tri_doubles)) != FT_OK) return rc;   // (no job: no pair record and no array changed)
    ms[1] += since(t3);
    return FT_OK;
}

// The new lights on one device of the context: `f` is the held scene with the new lights and pair records already in it.  The lights are
// uploaded, then the light-space structures follow (rebuild_light_space; `relay`: some light turned and the scene has grids).
static int32_t relight_device(ft_context* c, fth::FlatScene& f, const ft_context::LightSpace& T, std::vector<LightJob>& jobs, bool relay, bool lead, double ms[2]) {
    using clock = std::chrono::steady_clock;
    int32_t rc;
    FT_HIP(c, hipSetDevice(c->device));
    const auto t0 = clock::now();
    // frames still queued trace the scene these uploads rewrite (as upload_scene): they show the old lights
    if (any_queued(c)) { if ((rc = retire_queued(c)) != FT_OK) return rc; c->accum_open = false; }
    if ((rc = drain_frame_streams(c)) != FT_OK) return rc;
    if (c->side) FT_HIP(c, hipStreamSynchronize(c->side));
    if ((rc = upload(c, pose_array(c, kLights), f.lights)) != FT_OK) return rc;   // (the live pose set's: what dev_scene points into)
    ms[0] += std::chrono::duration<double, std::milli>(clock::now() - t0).count();
    if ((rc = rebuild_light_space(c, f, T, jobs, relay, lead, ms, "ft_scene_commit_lights")) != FT_OK) return rc;
    c->zero_signature[0] = c->zero_signature[1] = 0;                // (as every commit)
    c->committed = true;
    ++c->commit_serial; c->staged_hint = -1;
    return FT_OK;
}

// Every array of a pose set as `f` and the device's cull image hold it now fits the one in HBM (all sets have set 0's sizes).
static int32_t pose_arrays_fit(ft_context* c, const fth::FlatScene& f, const char* who) {
    const DeviceBuf* B = c->d_scene;
    if (B[kLeaves].bytes < f.leaves.size() * sizeof(ftd::Leaf) || B[kM2w].bytes < f.m2w.size() * 8 || B[kCulls].bytes < f.culls.size() * sizeof(ftd::CullRecord) ||
        B[kCullItems].bytes < c->cull_items_and_rows.size() * 4 || B[kCullRows].bytes < f.cull_rows.size() * 8 || B[kLights].bytes < f.lights.size() * sizeof(ftd::Light)) {
        c->err = std::string(who) + ": a scene array in device memory is smaller than the flattened one"; return FT_ERR_STATE;
    }
    return FT_OK;
}

// The new poses on one device of the context ("moved_in_place"): `f` is the held scene with the new leaves, m2w, cull
// records and face directions already in it, every array as long as it was.  They are uploaded over the old ones, then the light-space
// structures follow where a pair's frame changed (rebuild_light_space; `turned`: some pair's did - otherwise no kernel is launched).
static int32_t move_device(ft_context* c, fth::FlatScene& f, const ft_context::LightSpace& T, std::vector<LightJob>& jobs, bool turned, bool relay, bool lead, double ms[2]) {
    using clock = std::chrono::steady_clock;
    int32_t rc;
    FT_HIP(c, hipSetDevice(c->device));
    const auto t0 = clock::now();
    // frames still queued trace the scene these uploads rewrite (as upload_scene): they show the old poses
    if (any_queued(c)) { if ((rc = retire_queued(c)) != FT_OK) return rc; c->accum_open = false; }
    if ((rc = drain_frame_streams(c)) != FT_OK) return rc;
    if (c->side) FT_HIP(c, hipStreamSynchronize(c->side));
    cull_items_image(f, c->cull_items_and_rows);
    if ((rc = pose_arrays_fit(c, f, "ft_scene_commit_moved")) != FT_OK) return rc;
    // into the live pose set, which dev_scene points into: d_scene's own arrays unless a queued commit has moved on
    if ((rc = upload(c, pose_array(c, kLeaves), f.leaves)) != FT_OK || (rc = upload(c, pose_array(c, kM2w), f.m2w)) != FT_OK || (rc = upload(c, pose_array(c, kCulls), f.culls)) != FT_OK ||
        (rc = upload(c, pose_array(c, kCullItems), c->cull_items_and_rows)) != FT_OK || (rc = upload(c, pose_array(c, kCullRows), f.cull_rows)) != FT_OK) return rc;
    FT_HIP(c, hipStreamSynchronize(c->stream));
    ms[0] += std::chrono::duration<double, std::milli>(clock::now() - t0).count();
    // (a pair that lost its usable frame has a new record and no job)
    if (turned && (rc = rebuild_light_space(c, f, T, jobs, relay, lead, ms, "ft_scene_commit_moved")) != FT_OK) return rc;
    c->zero_signature[0] = c->zero_signature[1] = 0;                // (as every commit)
    c->committed = true;
    ++c->commit_serial; c->staged_hint = -1;
    return FT_OK;
}

// Does a pending frame or a queued temporal call hold pose set k?  (From the host's view: what it has not retired yet.)
static bool pose_set_held(const ft_context* c, int k) {
    for (const ft_context::FrameSlot& F : c->slots) if (F.pending && F.pose_set == k) return true;
    const ft_context::Temporal& T = c->temporal;
    for (int q = 1; q <= T.q_pending; ++q) if (T.queue[(T.q_turn + ft_context::Temporal::kQueue - q) % ft_context::Temporal::kQueue].pose_set == k) return true;
    return false;
}

// A further pose set with set 0's sizes; the first call also makes the entry that stands for set 0 and the uploads' stream.
static int32_t add_pose_set(ft_context* c) {
    ft_context::PoseSets& P = c->pose;
    if (!P.copies) FT_HIP(c, hipStreamCreateWithFlags(&P.copies, hipStreamNonBlocking));
    const bool first = P.sets.empty();
    P.sets.emplace_back();
    ft_context::PoseSets::Set& S = P.sets.back();
    int32_t rc;
    size_t at = 0;
    for (int a = 0; a < ft_context::kPoseArrayCount; ++a) {
        const size_t bytes = c->d_scene[kPoseArrays[a]].bytes;
        S.at[a] = at;
        at += (bytes + 255) / 256 * 256;
        if (!first && (rc = ensure(c, S.buf[a], bytes)) != FT_OK) { S.release(); P.sets.pop_back(); return rc; }
    }
    S.at[ft_context::kPoseArrayCount] = at;
    if (hipHostMalloc(reinterpret_cast<void**>(&S.staging), at, hipHostMallocDefault) != hipSuccess || hipEventCreateWithFlags(&S.ready, hipEventDisableTiming) != hipSuccess) {
        S.release(); P.sets.pop_back();
        c->err = "a pose set's staging memory or event could not be made"; return FT_ERR_HIP;
    }
    return FT_OK;
}

// A queued pose or light commit on one device of the context (ft_scene_commit_moved_enqueue / ft_scene_commit_lights_enqueue, DESIGN.md
// 14.2): `f` is the held scene with the new poses or lights already in it, every array as long as it was.  Nothing is retired and no
// stream is drained: the arrays go into a pose set no pending frame or temporal call was given, on a stream of their own, dev_scene is
// pointed at that set, and every stream that launches scene-reading kernels waits for the upload before its next launch.  `moved`: the
// poses changed (the cull image is made again).  ms[0] += the host time to queue the uploads.
static int32_t pose_enqueue_device(ft_context* c, const fth::FlatScene& f, bool moved, double ms[2], const char* who) {
    using clock = std::chrono::steady_clock;
    int32_t rc;
    FT_HIP(c, hipSetDevice(c->device));
    const auto t0 = clock::now();
    ft_context::PoseSets& P = c->pose;
    if (moved) cull_items_image(f, c->cull_items_and_rows);
    if ((rc = pose_arrays_fit(c, f, who)) != FT_OK) return rc;
    if (P.sets.empty() && (rc = add_pose_set(c)) != FT_OK) return rc;   // set 0's entry: its staging memory and event
    // The set: the live one when nothing pending was given it (nothing on the device reads it any more: blocking calls end before they
    // return), else any other that is free, else a new one; with every set held and none left to make, the oldest pending frame or
    // temporal call is retired, as queuing a fifth frame retires the first.
    int pick = -1;
    for (;;) {
        if (!pose_set_held(c, P.live)) pick = P.live;
        for (int k = 0; pick < 0 && k < (int)P.sets.size(); ++k) if (!pose_set_held(c, k)) pick = k;
        if (pick >= 0) break;
        if ((int)P.sets.size() < P.max_sets) { if ((rc = add_pose_set(c)) != FT_OK) return rc; pick = (int)P.sets.size() - 1; break; }
        ++P.retired_for_set;
        if ((rc = any_pending(c) ? retire_oldest_frame(c) : retire_oldest_temporal(c)) != FT_OK) return rc;
    }
    ft_context::PoseSets::Set& S = P.sets[(size_t)pick];
    // The staging copy is the source of the set's previous upload, which waits for nothing on the device: it has ended, or ends now.
    // (The host's own vectors are pageable and rewritten by the next call: they are never the source of an asynchronous copy.)
    if (S.uploaded) FT_HIP(c, hipEventSynchronize(S.ready));
    const void* src[ft_context::kPoseArrayCount] = {f.leaves.data(), f.m2w.data(), f.culls.data(), c->cull_items_and_rows.data(), f.cull_rows.data(), f.lights.data()};
    const size_t bytes[ft_context::kPoseArrayCount] = {f.leaves.size() * sizeof(ftd::Leaf), f.m2w.size() * 8, f.culls.size() * sizeof(ftd::CullRecord),
                                                       c->cull_items_and_rows.size() * 4, f.cull_rows.size() * 8, f.lights.size() * sizeof(ftd::Light)};
    ftk::DevScene& D = c->dev_scene;
    for (int a = 0; a < ft_context::kPoseArrayCount; ++a) {
        void* dst = pick == 0 ? c->d_scene[kPoseArrays[a]].p : S.buf[a].p;
        if (bytes[a]) {
            std::memcpy(S.staging + S.at[a], src[a], bytes[a]);
            FT_HIP(c, hipMemcpyAsync(dst, S.staging + S.at[a], bytes[a], hipMemcpyHostToDevice, P.copies));
        }
    }
    FT_HIP(c, hipEventRecord(S.ready, P.copies));
    S.uploaded = true;
    const auto point = [&](auto*& ptr, int a) { ptr = static_cast<std::remove_reference_t<decltype(ptr)>>(pick == 0 ? c->d_scene[kPoseArrays[a]].p : S.buf[a].p); };
    point(D.leaves, 0); point(D.m2w, 1); point(D.culls, 2); point(D.cull_items, 3); point(D.cull_rows, 4); point(D.lights, 5);
    P.live = pick;
    // every stream that launches kernels that read the scene: the main streams and `side`, where k_classify runs ahead (`tail` runs
    // k_resolve, which reads no scene array)
    FT_HIP(c, hipStreamWaitEvent(c->stream, S.ready, 0));
    for (hipStream_t m : c->more_mains) if (m) FT_HIP(c, hipStreamWaitEvent(m, S.ready, 0));
    if (c->side) FT_HIP(c, hipStreamWaitEvent(c->side, S.ready, 0));
    ms[0] += std::chrono::duration<double, std::milli>(clock::now() - t0).count();
    c->zero_signature[0] = c->zero_signature[1] = 0;                // (as every commit)
    c->committed = true;
    ++c->commit_serial; c->staged_hint = -1;
    return FT_OK;
}

// What ft_debug_pose_queue reports of one _enqueue call (`lights`: of the lights call): why it took the blocking path, or 0, and what the
// host still had pending on the first device when it returned.
static void note_pose_call(ft_context* c, bool lights, int64_t why) {
    int64_t* n = c->pose.counts + (lights ? 3 : 0);
    ++n[why == 0 ? 0 : 1]; n[2] = why;
    int64_t pending = c->temporal.q_pending;
    for (const ft_context::FrameSlot& F : c->slots) pending += F.pending ? 1 : 0;
    c->pose.counts[7] = pending;
}

// ------------------------------------------------------------------------------------------ queued deforms (ft_scene_commit_deformed_enqueue)
// Does a pending frame or a queued temporal call hold geometry set k?  (From the host's view, as pose_set_held.)
static bool geo_set_held(const ft_context* c, int k) {
    for (const ft_context::FrameSlot& F : c->slots) if (F.pending && F.geo_set == k) return true;
    const ft_context::Temporal& T = c->temporal;
    for (int q = 1; q <= T.q_pending; ++q) if (T.queue[(T.q_turn + ft_context::Temporal::kQueue - q) % ft_context::Temporal::kQueue].geo_set == k) return true;
    return false;
}

// A further geometry set with set 0's sizes, filled on `deform` by one device-to-device copy of the live set: the topology, and every
// mesh as the live set holds it.  The first call makes the entry that stands for set 0 instead.
static int32_t add_geo_set(ft_context* c, size_t n_meshes) {
    ft_context::GeoSets& G = c->geo;
    const bool first = G.sets.empty();
    G.sets.emplace_back();
    ft_context::GeoSets::Set& S = G.sets.back();
    const auto fail = [&](int32_t rc) { S.release(); G.sets.pop_back(); return rc; };
    if (hipEventCreateWithFlags(&S.ready, hipEventDisableTiming) != hipSuccess) { c->err = "a geometry set's event could not be made"; return fail(FT_ERR_HIP); }
    if (first) { S.wrote.assign(n_meshes, 0); return FT_OK; }
    int32_t rc;
    for (int a = 0; a < ft_context::kGeoArrayCount; ++a) {
        const DeviceBuf& from = geo_array(c, kGeoArrays[a]);
        if ((rc = ensure(c, S.buf[a], c->d_scene[kGeoArrays[a]].bytes)) != FT_OK) return fail(rc);
        if (from.bytes != S.buf[a].bytes || hipMemcpyAsync(S.buf[a].p, from.p, from.bytes, hipMemcpyDeviceToDevice, G.deform) != hipSuccess) {
            c->err = "a geometry set could not be filled from the live one"; return fail(FT_ERR_HIP);
        }
    }
    S.wrote = G.sets[(size_t)G.live].wrote;
    return FT_OK;
}

// What a queued call needs before its first launch: the stream, the staging block's event, and the page-locked block itself with room
// for `bytes` - grown only once `deform` has been waited for, written again only behind the event of the copies that last read it.
static int32_t stage_begin(ft_context* c, size_t bytes, Stager& st) {
    ft_context::GeoSets& G = c->geo;
    FT_HIP(c, hipSetDevice(c->device));
    if (!G.deform) FT_HIP(c, hipStreamCreateWithFlags(&G.deform, hipStreamNonBlocking));
    if (!G.staged) FT_HIP(c, hipEventCreateWithFlags(&G.staged, hipEventDisableTiming));
    if (G.staging_bytes < bytes) {
        FT_HIP(c, hipStreamSynchronize(G.deform));
        if (G.staging) FT_HIP(c, hipHostFree(G.staging));
        G.staging = nullptr; G.staging_bytes = 0; G.staged_used = false;
        FT_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&G.staging), bytes, hipHostMallocDefault));
        G.staging_bytes = bytes;
    }
    if (G.staged_used) FT_HIP(c, hipEventSynchronize(G.staged));
    st.base = G.staging; st.used = 0; st.cap = G.staging_bytes;
    return FT_OK;
}
// The bytes a queued call passes through the staging block: the palettes of the meshes skinned on the device, the vertices the host made.
static size_t stage_bytes(const fth::SceneGraph& g, const std::vector<DeformedMesh>& edits) {
    size_t n = 0;
    for (const DeformedMesh& e : edits) {
        const fth::GraphNode& node = g.nodes[(size_t)e.node];
        if (e.skinned) n += (node.palette.size() * 8 + 15) / 16 * 16;
        if (!e.on_device) n += (node.tris.size() * 8 + 15) / 16 * 16;
    }
    return n;
}

// A queued deform on the context's one device: `f` is the held scene with the new cull records and leaves already in it, `g` the graph
// with the new vertices; morph_device has made those of the `on_device` edits in d_verts, on `deform`.  Nothing is retired and no stream
// a frame runs on is waited for.  The refit goes into a geometry set no pending frame or temporal call was given - the live one when
// nothing holds it, else a free one, else a new one - after the ranges of the meshes it does not edit, where that set is behind the live
// one, have been carried over (k_refit_carry); the new leaves and cull records go out as a queued pose commit's do; dev_scene is pointed at
// the set, and every stream that launches scene-reading kernels waits for the refit before its next launch.  ms[0] += the host time.
static int32_t deform_enqueue_device(ft_context* c, const fth::FlatScene& f, const fth::SceneGraph& g, const std::vector<DeformedMesh>& edits, Stager& st, double ms[2]) {
    using clock = std::chrono::steady_clock;
    int32_t rc;
    FT_HIP(c, hipSetDevice(c->device));
    const auto t0 = clock::now();
    ft_context::GeoSets& G = c->geo;
    ft_context::Refit& R = c->refit;
    const DeviceBuf* B = c->d_scene;
    static_assert(sizeof(ftd::BspNode) % 8 == 0 && (ftd::kWideNodeDoubles * 8) % 8 == 0, "k_refit_carry copies 8-byte elements at the least");
    if (B[kNodes].bytes < f.nodes.size() * sizeof(ftd::BspNode) || B[kTris].bytes < f.tris.size() * 8 || B[kWide].bytes < f.wide.size() * 8 ||
        B[kCoarse].bytes < f.coarse_boxes.size() * 4 || R.d_arrived.bytes < f.nodes.size() * 4) {
        c->err = "ft_scene_commit_deformed_enqueue: a scene array in device memory is smaller than the flattened one"; return FT_ERR_STATE;
    }
    if (G.sets.empty() && (rc = add_geo_set(c, f.meshes.size())) != FT_OK) return rc;   // set 0's entry
    for (ft_context::GeoSets::Set& S : G.sets) if (S.wrote.size() != f.meshes.size()) { c->err = "ft_scene_commit_deformed_enqueue: the geometry sets are another scene's"; return FT_ERR_STATE; }
    // 1. The set, by the rule of the pose sets (pose_enqueue_device).
    int pick = -1;
    for (;;) {
        if (!geo_set_held(c, G.live)) pick = G.live;
        for (int k = 0; pick < 0 && k < (int)G.sets.size(); ++k) if (!geo_set_held(c, k)) pick = k;
        if (pick >= 0) break;
        if ((int)G.sets.size() < G.max_sets) { if ((rc = add_geo_set(c, f.meshes.size())) != FT_OK) return rc; pick = (int)G.sets.size() - 1; break; }
        ++G.counts[5];
        if ((rc = any_pending(c) ? retire_oldest_frame(c) : retire_oldest_temporal(c)) != FT_OK) return rc;
    }
    ft_context::GeoSets::Set& S = G.sets[(size_t)pick];
    const ft_context::GeoSets::Set& L = G.sets[(size_t)G.live];
    const auto buf_of = [&](int set, int a) -> const DeviceBuf& { return set == 0 ? c->d_scene[kGeoArrays[a]] : G.sets[(size_t)set].buf[a]; };
    // 2. The stale meshes: live -> picked, every range a refit writes (a mesh this call edits has them all written below - unless the
    // live set's tree is another one, rebuilt in place since: then its topology comes over first).
    std::vector<uint8_t> edited(f.meshes.size(), 0);
    for (const DeformedMesh& e : edits) edited[e.mesh] = 1;
    ftk::CarryTable table{};
    const auto flush = [&] { if (table.n) ftk::refit_carry(G.deform, table); table.n = 0; };
    int64_t carried = 0;
    for (uint32_t m = 0; pick != G.live && m < (uint32_t)f.meshes.size(); ++m) {
        if (S.wrote[m] == L.wrote[m] || (edited[m] && S.wrote[m] != ~0ull) || f.meshes[m].root >= 0) continue;
        const ftk::RefitMesh r = refit_ranges(f, m, 0.0);
        // array of kGeoArrays, first byte, bytes: nodes, list-order records, sorted copies, 4-wide nodes, coarse boxes
        const uint64_t spans[5][3] = {{0, (uint64_t)r.node_first * sizeof(ftd::BspNode), (uint64_t)r.node_count * sizeof(ftd::BspNode)},
                                      {1, (uint64_t)r.first_global * 72, (uint64_t)r.n * 72}, {1, (uint64_t)r.tri_first * 72, (uint64_t)r.tri_count * 72},
                                      {2, (uint64_t)r.wide_first * ftd::kWideNodeDoubles * 8, (uint64_t)r.wide_count * ftd::kWideNodeDoubles * 8},
                                      {3, (uint64_t)r.coarse_first * 24, (uint64_t)r.coarse_count * 24}};
        if (table.n + 5 > (uint32_t)ftk::kCarryRanges) flush();
        for (const auto& sp : spans) {
            if (sp[2] == 0) continue;
            const DeviceBuf& from = buf_of(G.live, (int)sp[0]);
            const DeviceBuf& to = buf_of(pick, (int)sp[0]);
            if (sp[1] + sp[2] > from.bytes || sp[1] + sp[2] > to.bytes) { c->err = "ft_scene_commit_deformed_enqueue: a mesh's range lies outside its array"; return FT_ERR_STATE; }
            table.r[table.n++] = ftk::CarryRange{static_cast<const char*>(from.p) + sp[1], static_cast<char*>(to.p) + sp[1], sp[2]};
            ++carried;
        }
        S.wrote[m] = L.wrote[m];
    }
    flush();
    G.counts[6] = carried;
    // 3. The vertices the host made, through the staging block, beside the ones morph_device left in d_verts.
    if ((rc = ensure_verts(c, verts_doubles(g, edits) * 8, true)) != FT_OK) return rc;   // (no larger than what a blend has already written into)
    for (const DeformedMesh& e : edits) {
        if (e.on_device) continue;
        const std::vector<double>& v = g.nodes[(size_t)e.node].vertices();
        if (!v.empty()) FT_HIP(c, hipMemcpyAsync(R.d_verts.as<double>() + e.at, st.put(v.data(), v.size() * 8), v.size() * 8, hipMemcpyHostToDevice, G.deform));
    }
    if (st.used) { FT_HIP(c, hipEventRecord(G.staged, G.deform)); G.staged_used = true; }
    // 4. The new leaves, cull records and cull image: a queued pose commit's steps (the serial, the signatures and the level hint with them).
    double pose_ms[2] = {0.0, 0.0};                                 // (its host time is part of this call's, taken below)
    if ((rc = pose_enqueue_device(c, f, true, pose_ms, "ft_scene_commit_deformed_enqueue")) != FT_OK) return rc;
    // 5. The refit, with the four arrays it rewrites taken from the picked set; `arrived` and `leaf_boxes` are scratch the stream orders.
    ftk::RefitArrays A = refit_arrays(c);
    A.nodes = buf_of(pick, 0).as<ftd::BspNode>(); A.tris = buf_of(pick, 1).as<double>(); A.wide = buf_of(pick, 2).as<double>(); A.coarse = buf_of(pick, 3).as<float>();
    for (const DeformedMesh& e : edits) {
        const ftk::RefitMesh m = refit_ranges(f, e.mesh, 1e-7 * e.scan.extent + 1e-300);
        if (m.node_count) FT_HIP(c, hipMemsetAsync(R.d_arrived.as<uint32_t>() + m.node_first, 0, (size_t)m.node_count * 4, G.deform));
        ftk::refit_mesh(G.deform, A, m, R.d_verts.as<double>() + e.at);
        S.wrote[e.mesh] = ++G.serial;
    }
    FT_HIP(c, hipGetLastError());
    FT_HIP(c, hipEventRecord(S.ready, G.deform));
    // 6. Live: dev_scene's four pointers, and every stream that launches kernels that read the scene behind the refit (`tail` reads no scene array).
    ftk::DevScene& D = c->dev_scene;
    D.nodes = A.nodes; D.tris = A.tris; D.wide = A.wide; D.coarse_boxes = A.coarse;
    G.live = pick;
    FT_HIP(c, hipStreamWaitEvent(c->stream, S.ready, 0));
    for (hipStream_t m : c->more_mains) if (m) FT_HIP(c, hipStreamWaitEvent(m, S.ready, 0));
    if (c->side) FT_HIP(c, hipStreamWaitEvent(c->side, S.ready, 0));
    ms[0] += std::chrono::duration<double, std::milli>(clock::now() - t0).count();
    return FT_OK;
}

// What ft_debug_deform_queue reports of one call: why it took the blocking path, or 0, and what the host still had pending on the first
// device when it returned.
static void note_deform_call(ft_context* c, int64_t why) {
    int64_t* n = c->geo.counts;
    ++n[why == 0 ? 0 : 1]; n[2] = why;
    int64_t pending = c->temporal.q_pending;
    for (const ft_context::FrameSlot& F : c->slots) pending += F.pending ? 1 : 0;
    n[4] = pending;
}

// ft_scene_commit_moved under "moved_in_place".  FT_OK with *in_place false: the re-flatten differs in more than poses and nothing was
// changed - the caller takes the full commit.
// `queue` (ft_scene_commit_moved_enqueue): when no light-space pair's frame changed the poses are queued instead (pose_enqueue_device) and
// *queued says so; with a changed pair the call goes on as the blocking one.
static int32_t move_in_place(ft_context* c, bool* in_place, bool queue = false, bool* queued = nullptr) {
    using clock = std::chrono::steady_clock;
    const auto t0 = clock::now();
    *in_place = false;
    fth::FlatScene& f = c->flat;
    // the pairs' tables, off `f` as the full commit left it: the poses in it are still that commit's, or an earlier call here derived them
    ft_context::LightSpace& T = c->lightspace;
    const bool ls = c->graph.light_space_shadows != 0;
    if (ls && !T.ready) derive_light_space_tables(f, T);
    const bool retree = ls && c->opt.light_space_retree != 0;
    if (retree && !T.blocks_laid) lay_retree_blocks(T);
    std::string why;
    if (c->graph.reflatten_moved(f, why) != FT_OK) return FT_OK;
    *in_place = true;
    // A pair's frame follows from its leaf's w2m and its light's direction alone (fth::ls_pair_frame); c and R are model-space and stay.
    // A pair whose frame is what its record holds is not touched: a translation changes no frame.
    const bool grids = c->graph.light_space_shadows == 2;
    std::vector<uint8_t> changed(T.pairs.size(), 0);
    bool turned = false;
    for (size_t k = 0; ls && k < T.pairs.size(); ++k) {
        const ft_context::LightSpace::Pair& P = T.pairs[k];
        if (f.leaves[P.leaf].ls_pairs == ~0u) continue;            // (stripped by ft_scene_commit_deformed: stays stripped)
        const double* rec = &f.ls_pairs[(size_t)ftd::kLsPairDoubles * P.rec];
        int32_t root;
        std::memcpy(&root, &rec[14], 4);
        fth::LsPairFrame fr;
        const bool usable = fth::ls_pair_frame(f.leaves[P.leaf], f.lights[P.light], fr) && P.R < 2e29;
        const bool same = usable ? root != INT32_MIN && std::memcmp(&rec[0], fr.U, 24) == 0 && std::memcmp(&rec[3], fr.V, 24) == 0 && std::memcmp(&rec[6], fr.D, 24) == 0 &&
                                       std::memcmp(&rec[12], &fr.k_rel, 8) == 0
                                 : root == INT32_MIN;
        changed[k] = same ? 0 : 1;
        turned = turned || !same;
    }
    std::vector<LightJob> jobs;
    size_t n_regrid = 0;
    int64_t n_refit = 0;
    for (size_t k = 0; turned && k < T.pairs.size(); ++k) {
        ft_context::LightSpace::Pair& P = T.pairs[k];
        if (f.leaves[P.leaf].ls_pairs == ~0u) continue;
        const bool refit = changed[k] != 0;
        // as in ft_scene_commit_lights: every pair that is not the full commit's has a job, since the region behind that commit's arrays
        // is laid out anew; a pair back at that commit's pose under that commit's direction takes its record, and with it its grid
        if ((retree && refit && P.block != ~0u) || !full_commits_pair(f, P, f.lights[P.light].v)) {
            const size_t before = jobs.size();
            moved_pair_job(f, P, f.lights[P.light], refit, false, grids, retree, jobs, n_regrid);
            if (refit && jobs.size() > before) ++n_refit;
            continue;
        }
        double* rec = &f.ls_pairs[(size_t)ftd::kLsPairDoubles * P.rec];
        std::memcpy(rec, P.rec0, sizeof P.rec0);
        if (!refit) continue;
        LightJob j{&P, {}, refit, false};
        for (int q = 0; q < 3; ++q) { j.frame.U[q] = rec[q]; j.frame.V[q] = rec[3 + q]; j.frame.D[q] = rec[6 + q]; j.frame.c[q] = rec[9 + q]; }
        j.frame.pad = 1e-7 * P.R + 1e-30;
        jobs.push_back(j);
        ++n_refit;
    }
    progressive_close(c);
    const double tallest = c->commit_ms[3];
    for (double& v : c->commit_ms) v = 0.0;
    c->commit_ms[3] = tallest;
    c->commit_ms[0] = std::chrono::duration<double, std::milli>(clock::now() - t0).count();
    double ms[2] = {0.0, 0.0};
    int32_t rc = FT_OK;
    const bool queues = queue && !turned;                           // (a changed pair means refit and grid kernels that write what frames in flight read)
    if (queued) *queued = queues;
    for (ft_context* d : devices(c)) {                              // every device rewrites its own copy; the first decides the grids
        rc = queues ? pose_enqueue_device(d, f, true, ms, "ft_scene_commit_moved_enqueue") : move_device(d, f, T, jobs, turned, turned && grids, d == c, ms);
        if (rc != FT_OK) { if (d != c) c->err = d->err; break; }
    }
    for (ft_context* p : c->peers) {
        p->flat.leaves = f.leaves; p->flat.m2w = f.m2w; p->flat.culls = f.culls; p->flat.cull_items = f.cull_items; p->flat.cull_rows = f.cull_rows;
        if (turned) p->flat.ls_pairs = f.ls_pairs;
    }
    c->commit_ms[1] = ms[1]; c->commit_ms[2] = ms[0];
    if (rc != FT_OK) { for (ft_context* d : devices(c)) d->committed = false; c->holds_commit = false; return rc; }   // HBM holds neither scene whole: ft_scene_commit
    c->moved_pending = false;
    c->moved_counts[3] = n_refit;
    return FT_OK;
}

} // namespace ftc

extern "C" {

// A caller's commit ends the progressive and the temporal accumulation; the re-commit of with_growing_hit_lists (commit_scene) does not.
int32_t ft_scene_commit(ft_context* c) {
    if (!c) return FT_ERR_INVALID;
    progressive_close(c);
    temporal_close(c);
    return commit_scene(c);
}

// The commit of a graph whose transforms alone changed (ft_sg_set_transform): ft_scene_commit's, but the temporal accumulation stays
// open - the leaves are the same in the same order, and the next ft_temporal_accumulate takes each moved leaf's surfaces back to the
// pose its history was written in (ft_passes.cpp).  A progressive accumulation's sums belong to the old scene: it ends.
// `queue`: ft_scene_commit_moved_enqueue - the call as under "moved_in_place" = 1 whatever the option says, queued when it can be.
static int32_t commit_moved(ft_context* c, bool queue) {
    if (!c) return FT_ERR_INVALID;
    if (!c->holds_commit) { c->err = "ft_scene_commit_moved: no committed scene to move (ft_scene_commit)"; return FT_ERR_STATE; }
    if (c->restructured) { c->err = "ft_scene_commit_moved: the graph, the root or the lights changed since the commit (ft_scene_commit)"; return FT_ERR_STATE; }
    // Option "moved_in_place" (DESIGN.md 14.1): the new poses go over the old ones and the light-space pairs follow on the device.  What
    // a full commit has always absorbed - a pending light setter, new vertices, a commit-time option - is still the full commit's.
    int64_t why = 0;
    if (c->host_only || !(c->opt.moved_in_place || queue)) why = 1;
    else if (c->lights_pending || c->options_pending) why = 2;
    else for (const fth::GraphNode& n : c->graph.nodes) if (n.deformed) why = 2;
    if (why == 0) {
        bool in_place = false, queued = false;
        const int32_t rc = move_in_place(c, &in_place, queue, &queued);
        if (in_place) {
            if (rc == FT_OK) { ++c->pose_serial; ++c->moved_counts[0]; c->moved_counts[2] = 0; if (queue) note_pose_call(c, false, queued ? 0 : 4); }
            return rc;
        }
        if (rc != FT_OK) return rc;
        why = 3;
    }
    progressive_close(c);
    const int32_t rc = commit_scene(c);
    if (rc == FT_OK) { ++c->pose_serial; ++c->moved_counts[1]; c->moved_counts[2] = why; c->moved_counts[3] = 0; if (queue) note_pose_call(c, false, why); }
    return rc;
}
int32_t ft_scene_commit_moved(ft_context* c) { return commit_moved(c, false); }
int32_t ft_scene_commit_moved_enqueue(ft_context* c) { return commit_moved(c, true); }

int32_t ft_debug_moved_commits(ft_context* c, int64_t out[4]) {
    if (!c || !out) return FT_ERR_INVALID;
    for (int k = 0; k < 4; ++k) out[k] = c->moved_counts[k];
    return FT_OK;
}

// The commit of a graph whose mesh vertices alone changed (ft_sg_set_mesh_triangles): the trees keep their topology and are refit on the
// device (ft_refit.hip); the temporal accumulation stays open and the pose counter stays, a progressive accumulation ends.
// `queue`: ft_scene_commit_deformed_enqueue - the same call, rule for rule, but nothing is retired and no stream a frame
// runs on is waited for: the refit goes into a geometry set no frame in flight reads (deform_enqueue_device).  A call that cannot be
// queued goes on as the blocking one; ft_debug_deform_queue says why.
static int32_t commit_deformed(ft_context* c, bool queue) {
    if (!c) return FT_ERR_INVALID;
    if (!c->holds_commit) { c->err = "ft_scene_commit_deformed: no committed scene to deform (ft_scene_commit)"; return FT_ERR_STATE; }
    if (c->restructured) { c->err = "ft_scene_commit_deformed: the graph, the root or the lights changed since the commit (ft_scene_commit)"; return FT_ERR_STATE; }
    if (c->moved_pending) { c->err = "ft_scene_commit_deformed: an ft_sg_set_transform is pending (ft_scene_commit_moved first)"; return FT_ERR_STATE; }
    if (c->options_pending) { c->err = "ft_scene_commit_deformed: a commit-time option changed since the commit (ft_scene_commit)"; return FT_ERR_STATE; }
    if (c->lights_pending) { c->err = "ft_scene_commit_deformed: a light setter is pending (ft_scene_commit_lights first)"; return FT_ERR_STATE; }
    using clock = std::chrono::steady_clock;
    const auto t0 = clock::now();
    fth::FlatScene& f = c->flat;
    // Host: one pass over every edited mesh - bounds, extent, finiteness - before anything is changed or uploaded.
    std::vector<DeformedMesh> edits;
    size_t verts_at = 0, n_on_device = 0, n_blended = 0, n_skinned = 0, n_skinned_dq = 0;
    // ft_debug_morph counts[2]: the meshes this call - whichever way it ends - has the host blend (GraphNode::vertices)
    struct HostBlends {
        ft_context* c; uint64_t before;
        static uint64_t total(const ft_context* c) { uint64_t n = 0; for (const fth::GraphNode& g : c->graph.nodes) n += g.host_blends; return n; }
        explicit HostBlends(ft_context* ctx) : c(ctx), before(total(ctx)) {}
        ~HostBlends() { c->morph.counts[2] = (int64_t)(total(c) - before); }
    } host_blends(c);
    struct HostSkins {                                              // ft_debug_skin counts[2], the same way
        ft_context* c; uint64_t before;
        static uint64_t total(const ft_context* c) { uint64_t n = 0; for (const fth::GraphNode& g : c->graph.nodes) n += g.host_skins; return n; }
        explicit HostSkins(ft_context* ctx) : c(ctx), before(total(ctx)) {}
        ~HostSkins() { c->skin.counts[2] = (int64_t)(total(c) - before); }
    } host_skins(c);
    struct HostSkinsDq {                                            // ft_debug_skin_dq counts[2], the same way
        ft_context* c; uint64_t before;
        static uint64_t total(const ft_context* c) { uint64_t n = 0; for (const fth::GraphNode& g : c->graph.nodes) n += g.host_skins_dq; return n; }
        explicit HostSkinsDq(ft_context* ctx) : c(ctx), before(total(ctx)) {}
        ~HostSkinsDq() { c->skin.counts_dq[2] = (int64_t)(total(c) - before); }
    } host_skins_dq(c);
    auto refuse = [c](bool depth) {
        c->err = depth ? "ft_scene_commit_deformed: an edited mesh has depth above 0 - its clipped BSP depends on the positions (ft_scene_commit)"
                       : "ft_scene_commit_deformed: an edited mesh holds a non-finite coordinate (ft_scene_commit)";
        c->committed = true;                                         // the old commit stays in HBM and stays renderable
        return (int32_t)FT_ERR_UNSUPPORTED;
    };
    for (uint32_t m = 0; m < (uint32_t)f.meshes.size(); ++m) {
        const int32_t id = f.mesh_node[m];
        if (id < 0 || !c->graph.valid(id) || !c->graph.nodes[(size_t)id].deformed) continue;
        const fth::GraphNode& n = c->graph.nodes[(size_t)id];
        const bool refuse_depth = n.depth > 0 && !c->graph.mesh_unclipped_bvh;
        // "morph_on_device" (DESIGN.md 16.4): weights describe the vertices - the device blends and scans them, below, once every
        // refusal that needs no vertices has been looked at (the positions 3 x triangle + corner are 32 bits wide there)
        const bool fits = !c->host_only && n.tris.size() / 9 <= 0x55555555u;
        const bool morph_device_ok = n.by_weights && fits && c->opt.morph_on_device == 1;
        // "skin_on_device" (DESIGN.md 16.5): a palette poses the shape - k_skin does, where the shape is explicit or blended on the device in
        // this same call; in every other case the host makes V (GraphNode::vertices) and the mesh goes the ft_sg_set_mesh_triangles way
        const bool skinned = n.n_bones > 0 && fits && c->opt.skin_on_device == 1 && (!n.by_weights || morph_device_ok);
        const bool blended = morph_device_ok && (n.n_bones == 0 || skinned);
        const bool on_device = blended || skinned;
        const fth::MeshScan scan = refuse_depth || on_device ? fth::MeshScan{{0, 0, 0, 0, 0, 0}, 0.0, true} : fth::scan_mesh(n.vertices().data(), (int64_t)(n.tris.size() / 9));
        if (refuse_depth || !scan.finite || f.meshes[m].root >= 0) return refuse(refuse_depth || f.meshes[m].root >= 0);
        DeformedMesh e{m, id, scan};
        e.at = verts_at; e.on_device = on_device; e.blended = blended; e.skinned = skinned;
        verts_at += n.tris.size() + (n.tris.size() & 1);
        n_on_device += on_device ? 1 : 0; n_blended += blended ? 1 : 0;
        const bool dq = n.palette_kind == fth::GraphNode::DualQuaternions;   // (the same route, k_skin_dq, counters of its own)
        n_skinned += skinned && !dq ? 1 : 0; n_skinned_dq += skinned && dq ? 1 : 0;
        edits.push_back(e);
    }
    // Why a queued call takes the blocking path (include/functracer_hip.h): decided before anything is changed or launched.
    int64_t why = 0;
    if (queue) {
        const bool ls_kept = c->opt.deform_light_space != 0 && c->graph.light_space_shadows != 0;
        if (c->host_only) why = 1;
        else if (!c->peers.empty()) why = 2;
        else if (!c->refit.ready) why = 3;
        else if (c->opt.refit_rebuild_percent > 0) why = 4;
        else if (ls_kept) {                                         // an edited mesh with a pair that still has its tree gets a light-space job, below
            if (!c->lightspace.ready) derive_light_space_tables(f, c->lightspace);
            std::vector<uint8_t> is_edited(f.meshes.size(), 0);
            for (const DeformedMesh& e : edits) is_edited[e.mesh] = 1;
            std::vector<uint8_t> keeps(f.leaves.size(), 1);       // (a leaf with a pair that cannot be refit is stripped instead: no job)
            for (const ft_context::LightSpace::Pair& P : c->lightspace.pairs) if (P.ls_first == ~0u) keeps[P.leaf] = 0;
            for (const ft_context::LightSpace::Pair& P : c->lightspace.pairs)
                if (f.leaves[P.leaf].ls_pairs != ~0u && keeps[P.leaf] && P.mesh < is_edited.size() && is_edited[P.mesh]) why = 5;
        }
        if (why == 0 && c->opt.temporal_follow_deformed && c->temporal.open && c->temporal.calls > 0) why = 6;
    }
    const bool queues = queue && why == 0;
    Stager stager;
    if (queues) { const int32_t src = stage_begin(c, stage_bytes(c->graph, edits), stager); if (src != FT_OK) return src; }
    // (the blocking call's blend and refit share d_verts and the scan's scratch with the queued calls' stream)
    else if (!c->host_only && c->geo.deform) { FT_HIP(c, hipSetDevice(c->device)); FT_HIP(c, hipStreamSynchronize(c->geo.deform)); }
    c->geo.counts[6] = 0;
    double morph_ms[2] = {0.0, 0.0};                                // uploads, kernels with their readbacks
    ft_context::Morph& M = c->morph;
    M.counts[1] = (int64_t)n_blended;
    c->skin.counts[1] = (int64_t)n_skinned;
    c->skin.counts_dq[1] = (int64_t)n_skinned_dq;
    if (n_on_device) {
        if (n_blended) ++M.counts[0];
        if (n_skinned) ++c->skin.counts[0];
        if (n_skinned_dq) ++c->skin.counts_dq[0];
        for (ft_context* d : devices(c)) {
            const int32_t mrc = morph_device(d, c->graph, edits, morph_ms, d == c, queues ? &stager : nullptr);
            if (mrc != FT_OK) { if (d != c) c->err = d->err; return mrc; }   // (only d_verts has been written: the old commit stands)
        }
    }
    M.last.clear();
    for (const DeformedMesh& e : edits) {
        ft_context::Morph::Used u{e.node, {0, 0, 0, 0, 0, 0, e.scan.extent, e.on_device ? 1.0 : 0.0}};
        for (int k = 0; k < 6; ++k) u.scan[k] = e.scan.bounds[k];
        M.last.push_back(u);
    }
    for (const DeformedMesh& e : edits) if (e.on_device && !e.scan.finite) return refuse(false);
    if (c->host_only) {                                             // the same rules; the commit itself is the full one
        progressive_close(c);
        const int32_t hrc = commit_scene(c);
        if (hrc == FT_OK && queue) note_deform_call(c, why);
        return hrc;
    }
    // "deform_light_space": the pairs' tables, off `f` as the full commit left it - before anything in it changes
    const bool keep_ls = c->opt.deform_light_space != 0 && c->graph.light_space_shadows != 0;
    ft_context::LightSpace& T = c->lightspace;
    if (keep_ls && !T.ready) derive_light_space_tables(f, T);
    const bool retree = keep_ls && c->opt.light_space_retree != 0;
    if (retree && !T.blocks_laid) lay_retree_blocks(T);
    std::vector<double> bounds = f.mesh_bounds;
    for (const DeformedMesh& e : edits) for (int k = 0; k < 6; ++k) bounds[6 * (size_t)e.mesh + k] = e.scan.bounds[k];
    int32_t rc = c->graph.reflatten_deformed(f, bounds, c->err);   // the cull records, by the flattener's own walk
    if (rc != FT_OK) { if (rc == FT_ERR_UNSUPPORTED) c->committed = true; return rc; }
    // The light-space structures are built from the vertices.  By default they are not refit: the directional shadow rays of an edited
    // mesh walk its BVH (the same bits, include/functracer_hip.h "light_space_shadows") until the next full commit brings them back.
    // Under "deform_light_space" a leaf keeps its pairs where every one of them that had a tree can be refit.
    std::vector<const DeformedMesh*> edited(f.meshes.size(), nullptr);
    for (const DeformedMesh& e : edits) edited[e.mesh] = &e;
    std::vector<uint8_t> kept(f.leaves.size(), keep_ls ? 1 : 0);
    if (keep_ls) for (const ft_context::LightSpace::Pair& P : T.pairs) if (P.ls_first == ~0u) kept[P.leaf] = 0;
    for (size_t k = 0; k < f.leaves.size(); ++k) {
        ftd::Leaf& L = f.leaves[k];
        if (L.kind == ftd::LK_MESH && L.mesh < edited.size() && edited[L.mesh] && !kept[k]) L.ls_pairs = ~0u;
    }
    // Every pair of an edited mesh: the centre of the new bounds, R over the new records.  With it, as in ft_scene_commit_lights, every
    // pair that is not the full commit's any more: the region behind that commit's arrays is laid out anew and holds all their grids.
    std::vector<LightJob> jobs;
    size_t n_regrid = 0;
    bool touched = false;
    const bool grids = c->graph.light_space_shadows == 2;
    std::map<uint32_t, double> extent_of;
    if (keep_ls) {
        for (ft_context::LightSpace::Pair& P : T.pairs) {
            if (f.leaves[P.leaf].ls_pairs == ~0u || P.mesh >= edited.size() || !edited[P.mesh]) continue;   // (stripped before: stays stripped)
            const DeformedMesh& e = *edited[P.mesh];
            for (int q = 0; q < 3; ++q) P.c[q] = 0.5 * (e.scan.bounds[q] + e.scan.bounds[3 + q]);
            if (e.on_device) {                                      // the vertices are in HBM alone: reduced there (once per mesh - every pair of it has this centre)
                if (!(extent_of.count(e.mesh))) {
                    double R = 0.0;
                    if ((rc = morph_pair_extent(c, c->graph, e, P.c, &R, morph_ms)) != FT_OK) {   // (a HIP error; the held scene is half rewritten: ft_scene_commit)
                        for (ft_context* d : devices(c)) d->committed = false;
                        c->holds_commit = false;
                        return rc;
                    }
                    extent_of[e.mesh] = R;
                }
                P.R = extent_of[e.mesh];
            } else {
                const std::vector<double>& v = c->graph.nodes[(size_t)e.node].vertices();
                P.R = fth::ls_pair_extent(v.data(), v.size() / 9, true, P.c);
            }
            P.deformed = true;
            touched = true;
        }
        for (ft_context::LightSpace::Pair& P : T.pairs) {
            if (!touched || f.leaves[P.leaf].ls_pairs == ~0u) continue;
            const bool now = P.mesh < edited.size() && edited[P.mesh];
            if (now || !full_commits_pair(f, P, f.lights[P.light].v)) moved_pair_job(f, P, f.lights[P.light], now, now, grids, retree, jobs, n_regrid);
        }
    }
    progressive_close(c);
    const double tallest = c->commit_ms[3];
    for (double& v : c->commit_ms) v = 0.0;
    c->commit_ms[3] = tallest;
    c->commit_ms[0] = std::chrono::duration<double, std::milli>(clock::now() - t0).count() - morph_ms[0] - morph_ms[1];
    double ms[2] = {morph_ms[0], morph_ms[1]};
    RebuildPlan plan;
    if (queues) rc = deform_enqueue_device(c, f, c->graph, edits, stager, ms);   // (one device, no light-space job, no rebuild: the reasons above)
    else for (ft_context* d : devices(c)) {                         // every device refits its own copy
        if ((rc = refit_device(d, f, c->graph, edits, ms, d == c, plan)) != FT_OK) { if (d != c) c->err = d->err; break; }
        // behind the refit, which has written the list-order records the gather and the grid passes read
        if (!jobs.empty() && (rc = rebuild_light_space(d, f, T, jobs, grids, d == c, ms, "ft_scene_commit_deformed")) != FT_OK) { if (d != c) c->err = d->err; break; }
    }
    if (!jobs.empty()) for (ft_context* p : c->peers) p->flat.ls_pairs = f.ls_pairs;
    if (rc == FT_OK && plan.tallest > 0) {                          // rebuilt trees: the height figure, and room in the stacks for a taller one
        c->commit_ms[3] = std::max(c->commit_ms[3], (double)plan.tallest);
        for (ft_context* d : devices(c)) {
            if ((int32_t)plan.tallest + 1 <= d->flat.stack_capacity) continue;
            if ((rc = fit_stacks(d, plan.tallest)) != FT_OK) { if (d != c) c->err = d->err; break; }
            derive_launch_shape(d);
        }
    }
    c->commit_ms[1] = ms[1]; c->commit_ms[2] = ms[0];
    if (rc != FT_OK) { for (ft_context* d : devices(c)) d->committed = false; c->holds_commit = false; return rc; }   // HBM holds neither scene whole: ft_scene_commit
    for (fth::GraphNode& n : c->graph.nodes) n.deformed = false;
    if (queue) note_deform_call(c, why);
    return FT_OK;
}
int32_t ft_scene_commit_deformed(ft_context* c) { return commit_deformed(c, false); }
int32_t ft_scene_commit_deformed_enqueue(ft_context* c) { return commit_deformed(c, true); }

// The commit of a graph whose lights alone changed (ft_scene_set_directional / _soft_directional / _positional): no flatten and no BVH
// work.  The lights are uploaded again; every light-space pair whose direction changed gets its record derived again on the host, as
// build_light_space derives it, its tree refit and its grid built again on the device (ft_lightspace.hip).  The temporal accumulation
// stays open and the pose counter stays; a progressive accumulation ends.
// `queue`: ft_scene_commit_lights_enqueue - queued when no light that has a light-space pair turns.
static int32_t commit_lights(ft_context* c, bool queue) {
    if (!c) return FT_ERR_INVALID;
    if (!c->holds_commit) { c->err = "ft_scene_commit_lights: no committed scene to relight (ft_scene_commit)"; return FT_ERR_STATE; }
    if (c->restructured) { c->err = "ft_scene_commit_lights: the graph, the root or the number or kinds of the lights changed since the commit (ft_scene_commit)"; return FT_ERR_STATE; }
    if (c->moved_pending) { c->err = "ft_scene_commit_lights: an ft_sg_set_transform is pending (ft_scene_commit_moved first)"; return FT_ERR_STATE; }
    for (const fth::GraphNode& n : c->graph.nodes) if (n.deformed) { c->err = "ft_scene_commit_lights: an ft_sg_set_mesh_triangles is pending (ft_scene_commit_deformed first)"; return FT_ERR_STATE; }
    if (c->options_pending) { c->err = "ft_scene_commit_lights: a commit-time option changed since the commit (ft_scene_commit)"; return FT_ERR_STATE; }
    if (c->host_only) {                                             // the same rules; the commit itself is the full one
        progressive_close(c);
        const int32_t rc = commit_scene(c);
        if (rc == FT_OK && queue) note_pose_call(c, true, 1);
        return rc;
    }
    using clock = std::chrono::steady_clock;
    const auto t0 = clock::now();
    fth::FlatScene& f = c->flat;
    if (c->graph.lights.size() != f.lights.size()) { c->err = "ft_scene_commit_lights: the number of lights changed since the commit (ft_scene_commit)"; return FT_ERR_STATE; }
    ft_context::LightSpace& T = c->lightspace;
    if (!T.ready) derive_light_space_tables(f, T);                  // off the records as the full commit left them
    const bool retree = c->opt.light_space_retree != 0 && c->graph.light_space_shadows != 0;
    if (retree && !T.blocks_laid) lay_retree_blocks(T);
    std::vector<ftd::Light> lights = c->graph.lights;
    for (ftd::Light& l : lights) if (l.kind == ftd::LT_SOFT) l.tan_half_scatter = std::tan(l.scatter / 2.0);   // (as the flattener)
    const auto same_dir = [](const double a[3], const double b[3]) { return std::memcmp(a, b, 3 * sizeof(double)) == 0; };
    // Only a direction that changes touches a pair: colours and the other kinds of light are the upload alone.
    bool turned = false;
    for (const ft_context::LightSpace::Pair& P : T.pairs) turned = turned || (f.leaves[P.leaf].ls_pairs != ~0u && !same_dir(lights[P.light].v, f.lights[P.light].v));
    const bool grids = c->graph.light_space_shadows == 2;
    std::vector<LightJob> jobs;
    size_t n_regrid = 0;
    for (ft_context::LightSpace::Pair& P : T.pairs) {
        if (!turned || f.leaves[P.leaf].ls_pairs == ~0u) continue;  // (stripped by ft_scene_commit_deformed: stays stripped)
        const bool refit = !same_dir(lights[P.light].v, f.lights[P.light].v);
        if ((retree && refit && P.block != ~0u) || !full_commits_pair(f, P, lights[P.light].v)) { moved_pair_job(f, P, lights[P.light], refit, false, grids, retree, jobs, n_regrid); continue; }
        // the full commit's direction (again) over that commit's vertices in that commit's pose: its record, and with it its grid, which
        // still lies where that commit put it.  (Not for a deformed pair: rec0 and that grid describe vertices that are gone.  Not for a retreed one: that
        // commit's tree leads to leaf records that have been sorted anew since.)
        double* rec = &f.ls_pairs[(size_t)ftd::kLsPairDoubles * P.rec];
        std::memcpy(rec, P.rec0, sizeof P.rec0);
        if (!refit) continue;
        LightJob j{&P, {}, refit, false};
        for (int q = 0; q < 3; ++q) { j.frame.U[q] = rec[q]; j.frame.V[q] = rec[3 + q]; j.frame.D[q] = rec[6 + q]; j.frame.c[q] = rec[9 + q]; }
        j.frame.pad = 1e-7 * P.R + 1e-30;
        jobs.push_back(j);
    }
    f.lights = lights;
    progressive_close(c);
    const double tallest = c->commit_ms[3];
    for (double& v : c->commit_ms) v = 0.0;
    c->commit_ms[3] = tallest;
    c->commit_ms[0] = std::chrono::duration<double, std::milli>(clock::now() - t0).count();
    double ms[2] = {0.0, 0.0};
    int32_t rc = FT_OK;
    const bool queues = queue && !turned;                           // (a light with pairs that turns means refit and grid kernels that write what frames in flight read)
    for (ft_context* d : devices(c)) {                              // every device rewrites its own copy; the first decides the grids
        rc = queues ? pose_enqueue_device(d, f, false, ms, "ft_scene_commit_lights_enqueue") : relight_device(d, f, T, jobs, turned && grids, d == c, ms);
        if (rc != FT_OK) { if (d != c) c->err = d->err; break; }
    }
    for (ft_context* p : c->peers) { p->flat.lights = f.lights; p->flat.ls_pairs = f.ls_pairs; }
    c->commit_ms[1] = ms[1]; c->commit_ms[2] = ms[0];
    if (rc != FT_OK) { for (ft_context* d : devices(c)) d->committed = false; c->holds_commit = false; return rc; }   // HBM holds neither scene whole: ft_scene_commit
    c->lights_pending = false;
    if (queue) note_pose_call(c, true, queues ? 0 : 4);
    return FT_OK;
}
int32_t ft_scene_commit_lights(ft_context* c) { return commit_lights(c, false); }
int32_t ft_scene_commit_lights_enqueue(ft_context* c) { return commit_lights(c, true); }


// The measured quality of one mesh's tree: what a host sets "refit_rebuild_percent" by.
int32_t ft_scene_tree_quality(ft_context* c, ft_node mesh_node, double out[4]) {
    if (!c || !out) return FT_ERR_INVALID;
    if (!c->graph.valid(mesh_node) || c->graph.nodes[mesh_node].kind != fth::GraphNode::Mesh) { c->err = "ft_scene_tree_quality: not a bspMesh node"; return FT_ERR_INVALID; }
    if (!c->holds_commit) { c->err = "ft_scene_tree_quality: no committed scene (ft_scene_commit)"; return FT_ERR_STATE; }
    const fth::FlatScene& f = c->flat;
    uint32_t mesh = 0;
    while (mesh < (uint32_t)f.meshes.size() && f.mesh_node[mesh] != mesh_node) ++mesh;   // a node under several transforms is one mesh
    if (mesh == (uint32_t)f.meshes.size()) { c->err = "ft_scene_tree_quality: the node is not part of the committed scene (ft_scene_commit)"; return FT_ERR_STATE; }
    if ((c->graph.nodes[mesh_node].depth > 0 && !c->graph.mesh_unclipped_bvh) || !refittable(f, mesh)) {
        c->err = "ft_scene_tree_quality: the mesh has no BVH (depth above 0, or fewer than 8 triangles)"; return FT_ERR_UNSUPPORTED;
    }
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    int32_t rc;
    FT_HIP(c, hipSetDevice(c->device));
    if (any_queued(c)) { if ((rc = retire_queued(c)) != FT_OK) return rc; c->accum_open = false; }
    if ((rc = drain_frame_streams(c)) != FT_OK) return rc;
    if (c->side) FT_HIP(c, hipStreamSynchronize(c->side));
    c->tree_quality.resize(f.meshes.size());
    ft_context::TreeQuality& q = c->tree_quality[mesh];
    double now = 0.0;
    if ((rc = measure_cost(c, f, mesh, &now)) != FT_OK) return rc;
    if (!q.known) { q.cost_built = now; q.known = true; }           // no refit since the build, or it would have been recorded then
    out[0] = now; out[1] = q.cost_built; out[2] = job_of(f, mesh) ? 1.0 : 0.0; out[3] = (double)q.rebuilds;
    return FT_OK;
}

int32_t ft_get_commit_times(ft_context* c, double ms[4]) {
    if (!c || !ms) return FT_ERR_INVALID;
    for (int k = 0; k < 4; ++k) ms[k] = c->commit_ms[k];
    return FT_OK;
}

} // extern "C"

namespace ftc {

// ------------------------------------------------------------------------------------------ frames out of HBM
// The device keeps the last frame in FRAME layout (row 0 = top, Image.fs:39) whatever the tiles were: d_out as FP64 RGB or d_out8 as
// Image.write's RGBA8 bytes (Image.fs:36).  Fetching copies the rendered rects - whole rows as one copy, narrower rects as a 2D copy -
// straight into the caller's frame; nothing is gathered or scattered on the host.
// `rects` of a frame-layout buffer in HBM (px bytes per pixel, res_h pixels per row) into the caller's frame of the same layout.
int32_t copy_rects_out(ft_context* c, void* out, const void* frame, size_t px, int32_t res_h, const std::vector<ft_rect>& rects, hipStream_t async) {
    auto copy1 = [&](void* d, const void* s_, size_t n) { return async ? hipMemcpyAsync(d, s_, n, hipMemcpyDeviceToHost, async) : hipMemcpy(d, s_, n, hipMemcpyDeviceToHost); };
    auto copy2 = [&](void* d, size_t dp, const void* s_, size_t sp, size_t w, size_t h) { return async ? hipMemcpy2DAsync(d, dp, s_, sp, w, h, hipMemcpyDeviceToHost, async) : hipMemcpy2D(d, dp, s_, sp, w, h, hipMemcpyDeviceToHost); };
    const size_t pitch = (size_t)res_h * px;
    const char* src = static_cast<const char*>(frame);
    char* dst = static_cast<char*>(out);
    // A device of a multi-device context holds every N-th 8-row band of the frame: whole rows, equally high, equally spaced.  Those go
    // out as ONE two-dimensional copy whose "rows" are the bands (band = 8 x pitch contiguous bytes, 8 N x pitch apart on both sides) -
    // 34 blocking copies of 737 KB per device at 4K otherwise.  A shorter last band follows on its own.
    size_t k0 = 0;
    {
        const auto& R = rects;
        size_t run = 0;
        if (R.size() >= 3 && R[0].x0 == 0 && R[0].w == res_h) {
            const int step = R[1].y0 - R[0].y0;
            run = 1;
            while (run < R.size() && R[run].x0 == 0 && R[run].w == R[0].w && R[run].h == R[0].h && R[run].y0 == R[0].y0 + (int)run * step) ++run;
            if (step > R[0].h && run >= 3) {
                const size_t off = (size_t)R[0].y0 * pitch;
                FT_HIP(c, copy2(dst + off, (size_t)step * pitch, src + off, (size_t)step * pitch, (size_t)R[0].h * pitch, run));
                k0 = run;
            }
        }
    }
    for (size_t k = k0; k < rects.size();) {
        const ft_rect r = rects[k];
        if (r.x0 == 0 && r.w == res_h) {                    // whole rows; vertically adjacent rects go out as one copy
            int rows = r.h;
            size_t k2 = k + 1;
            while (k2 < rects.size() && rects[k2].x0 == 0 && rects[k2].w == r.w && rects[k2].y0 == r.y0 + rows) { rows += rects[k2].h; ++k2; }
            FT_HIP(c, copy1(dst + (size_t)r.y0 * pitch, src + (size_t)r.y0 * pitch, (size_t)rows * pitch));
            k = k2;
        } else {
            const size_t off = (size_t)r.y0 * pitch + (size_t)r.x0 * px;
            FT_HIP(c, copy2(dst + off, pitch, src + off, pitch, (size_t)r.w * px, (size_t)r.h));
            ++k;
        }
    }
    return FT_OK;
}

// The rects of the context's pixel list out of d_out / d_out8 into the caller's frame: blocking copies, or (async != null) queued on that
// stream behind the frame's k_resolve - the caller's memory should then be page-locked (ft_host_alloc), or the runtime stages the copy.
int32_t copy_frame_out(ft_context* c, void* out, int format, hipStream_t async) {
    return copy_rects_out(c, out, format == 1 ? c->d_out8.p : c->d_out.p, format == 1 ? 4 : 24, c->last_res_h, c->pixel_rects, async);
}
int32_t fetch_single(ft_context* c, void* out, int format) {
    if (c->last_n_pix <= 0) { c->err = "no frame rendered yet"; return FT_ERR_STATE; }
    if (format != c->last_format) { c->err = format == 1 ? "the last frame was rendered as FP64 RGB (ft_render): no RGBA8 frame to fetch" : "the last frame was rendered as RGBA8 (ft_render_rgba8): no FP64 frame to fetch"; return FT_ERR_STATE; }
    FT_HIP(c, hipSetDevice(c->device));
    const int32_t rc = drain_frame_streams(c);
    if (rc != FT_OK) return rc;
    return copy_frame_out(c, out, format, nullptr);
}

} // namespace ftc

extern "C" {

static int32_t fetch_all(ft_context* c, void* out, int format) {
    if (!c || !out) return FT_ERR_INVALID;
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    const std::vector<ft_context*> devs = devices(c);
    std::vector<ft_context*> with;
    for (ft_context* d : devs) if (d->last_n_pix > 0) with.push_back(d);
    if (with.empty()) { c->err = "no frame rendered yet"; return FT_ERR_STATE; }
    if (with.size() == 1) { const int32_t rc = fetch_single(with[0], out, format); if (rc != FT_OK && with[0] != c) c->err = with[0]->err; return rc; }
    return on_every_device(c, nullptr, {}, [&](size_t, ft_context* D, ft_stats*) {   // every device copies its own bands into the caller's frame, all at once
        return D->last_n_pix > 0 ? fetch_single(D, out, format) : (int32_t)FT_OK;
    });
}
int32_t ft_fetch_frame(ft_context* c, double* out_rgb) { return fetch_all(c, out_rgb, 0); }
int32_t ft_fetch_frame_rgba8(ft_context* c, uint8_t* out_rgba) { return fetch_all(c, out_rgba, 1); }

/* Page-locked host memory for frames (hipHostMalloc): a D2H copy into it is one DMA at link rate, without the runtime's staging. */
void* ft_host_alloc(size_t bytes) { void* p = nullptr; return (bytes && hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess) ? p : nullptr; }
void ft_host_free(void* p) { if (p) (void)hipHostFree(p); }

int32_t ft_quantise_rgba8(const double* rgb, int64_t n_pixels, uint8_t* out) {   // Image.fs:36, Math.fs:12-16
    if (!rgb || !out || n_pixels < 0) return FT_ERR_INVALID;
    for (int64_t i = 0; i < n_pixels; ++i) {
        for (int k = 0; k < 3; ++k) {
            double x = rgb[3 * i + k];
            if (x > 1.0) x = 1.0; else if (x < 0.0) x = 0.0;                     // NaN passes through the clamp unchanged
            x = x * 255.0;
            out[4 * i + k] = (x != x) ? 0 : (uint8_t)x;                          // truncation, not rounding
        }
        out[4 * i + 3] = 255;
    }
    return FT_OK;
}

} // extern "C"

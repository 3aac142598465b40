// refit_host_check.cpp — the host side of ft_scene_commit_deformed under AddressSanitizer + UBSan, as a stand-alone program (CPU only).
// It drives a host-only context through ft_sg_set_mesh_triangles / ft_scene_commit_deformed and every refusal, and then the flattener's
// part of a device refit directly (fth::scan_mesh, SceneGraph::reflatten_deformed), whose cull records must be the fresh flatten's.
// Build and run from the repository root (the device objects are linked as they are: make -C functracer_amd/csrc first):
//   C=functracer_amd/csrc; S="-fsanitize=address,undefined -fno-omit-frame-pointer -g -O1 -std=c++17 -ffp-contract=off"
//   g++ $S -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include tools/refit_host_check.cpp $C/ft_capi.cpp $C/ft_frame.cpp $C/ft_progressive.cpp \
//       $C/ft_passes.cpp $C/ft_debug.cpp $C/ft_scene.cpp $(for o in $(make -s -C $C print-DEVICE_OBJS); do echo $C/$o; done) \
//       -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib -o build/refit_host_check && build/refit_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../functracer_amd/csrc/ft_scene.h"

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); std::exit(1); } } while (0)

static std::vector<double> blob(int n, unsigned seed, double shift = 0.0, double scale = 1.0) {
    std::mt19937 rng(seed);
    std::normal_distribution<double> g;
    std::vector<double> t((size_t)9 * n);
    for (int i = 0; i < n; ++i) {
        const double c[3] = {0.8 * g(rng), 0.8 * g(rng), 0.8 * g(rng)};
        for (int k = 0; k < 9; ++k) t[(size_t)9 * i + k] = scale * (c[k % 3] + 0.08 * g(rng)) + shift;
    }
    return t;
}

int main() {
    // ---- the C ABI on a host-only context
    ft_context* c = nullptr;
    CHECK(ft_create_host_only(&c) == FT_OK);
    CHECK(ft_scene_commit_deformed(nullptr) == FT_ERR_INVALID && ft_scene_commit_deformed(c) == FT_ERR_STATE);
    const std::vector<double> a = blob(300, 1), b = blob(40, 2);
    const ft_node flat = ft_sg_bsp_mesh(c, 0, a.data(), 300), deep = ft_sg_bsp_mesh(c, 2, b.data(), 40);
    const ft_transform up{FT_TRANSLATE, 0, {0, 3, 0}, 0};
    const ft_node xf = ft_sg_transform(c, &up, 1, deep);
    const ft_node kids[2] = {flat, xf};
    CHECK(ft_scene_set_objects(c, ft_sg_group(c, kids, 2)) == FT_OK);
    const double dir[3] = {0, -1, 1}, white[3] = {1, 1, 1};
    CHECK(ft_scene_add_directional(c, dir, white) == FT_OK && ft_scene_commit(c) == FT_OK);
    CHECK(ft_sg_set_mesh_triangles(nullptr, flat, a.data(), 300) == FT_ERR_INVALID && ft_sg_set_mesh_triangles(c, -1, a.data(), 300) == FT_ERR_INVALID);
    CHECK(ft_sg_set_mesh_triangles(c, xf, a.data(), 300) == FT_ERR_INVALID && ft_sg_set_mesh_triangles(c, flat, nullptr, 300) == FT_ERR_INVALID);
    CHECK(ft_sg_set_mesh_triangles(c, flat, a.data(), 299) == FT_ERR_INVALID && ft_sg_set_mesh_triangles(c, flat, a.data(), 301) == FT_ERR_INVALID);
    const std::vector<double> a2 = blob(300, 1, 1e3);
    CHECK(ft_sg_set_mesh_triangles(c, flat, a2.data(), 300) == FT_OK && ft_scene_commit_deformed(c) == FT_OK);
    CHECK(ft_sg_set_transform(c, xf, &up, 1) == FT_OK && ft_scene_commit_deformed(c) == FT_ERR_STATE && ft_scene_commit_moved(c) == FT_OK);
    CHECK(ft_sg_set_mesh_triangles(c, deep, b.data(), 40) == FT_OK && ft_scene_commit_deformed(c) == FT_ERR_UNSUPPORTED && ft_scene_commit(c) == FT_OK);
    std::vector<double> bad = a;
    bad[77] = std::numeric_limits<double>::quiet_NaN();
    CHECK(ft_sg_set_mesh_triangles(c, flat, bad.data(), 300) == FT_OK && ft_scene_commit_deformed(c) == FT_ERR_UNSUPPORTED);
    int64_t n_leaves = 0;
    CHECK(ft_debug_leaf_matrices(c, &n_leaves, nullptr, nullptr) == FT_OK && n_leaves == 2);
    CHECK(ft_sg_set_mesh_triangles(c, flat, a.data(), 300) == FT_OK && ft_scene_commit_deformed(c) == FT_OK);
    CHECK(ft_sg_primitive(c, FT_PRIM_SPHERE) >= 0 && ft_scene_commit_deformed(c) == FT_ERR_STATE);
    ft_destroy(c);

    // ---- the flattener's part of a device refit: bounds pass + cull regeneration against a fresh flatten
    for (int pass = 0; pass < 3; ++pass) {
        fth::SceneGraph g;
        auto add = [&](fth::GraphNode n) { g.nodes.push_back(std::move(n)); return (int32_t)g.nodes.size() - 1; };
        fth::GraphNode m; m.kind = fth::GraphNode::Mesh; m.tris = blob(500, 3);
        const int32_t mesh = add(m);
        fth::GraphNode t1; t1.kind = fth::GraphNode::Transform; t1.xf = {ft_transform{FT_ROTATE, 0, {0, 1, 0}, 0.7}}; t1.children = {mesh};
        fth::GraphNode t2; t2.kind = fth::GraphNode::Transform; t2.xf = {ft_transform{FT_TRANSLATE, 0, {4, 0, 0}, 0}}; t2.children = {mesh};   // the same node twice
        fth::GraphNode s; s.kind = fth::GraphNode::Prim; s.prim = FT_PRIM_SPHERE;
        fth::GraphNode few; few.kind = fth::GraphNode::Mesh; few.tris = blob(5, 4);
        fth::GraphNode grp; grp.kind = fth::GraphNode::Group; grp.children = {add(t1), add(t2), add(s), add(few)};
        g.root = add(grp);
        fth::FlatScene held, fresh;
        std::string err;
        CHECK(g.flatten(held, err) == FT_OK);
        CHECK(held.mesh_node.size() == held.meshes.size() && held.mesh_ranges.size() == held.meshes.size() && held.wide_node.size() * ftd::kWideNodeDoubles == held.wide.size());
        g.nodes[(size_t)mesh].tris = pass == 0 ? blob(500, 5, 0.0, 3.0) : pass == 1 ? blob(500, 3, 1e3) : blob(500, 3, 0.0, 1.0 / 256.0);
        std::vector<double> bounds = held.mesh_bounds;
        for (size_t k = 0; k < held.meshes.size(); ++k) {
            if (held.mesh_node[k] != mesh) continue;
            const fth::MeshScan sc = fth::scan_mesh(g.nodes[(size_t)mesh].tris.data(), 500);
            CHECK(sc.finite && sc.extent > 0.0);
            std::memcpy(&bounds[6 * k], sc.bounds, sizeof sc.bounds);
        }
        CHECK(g.reflatten_deformed(held, bounds, err) == FT_OK);
        CHECK(g.flatten(fresh, err) == FT_OK);
        CHECK(held.culls.size() == fresh.culls.size() && std::memcmp(held.culls.data(), fresh.culls.data(), held.culls.size() * sizeof(ftd::CullRecord)) == 0);
        CHECK(held.cull_items.size() == fresh.cull_items.size());
        for (size_t k = 0; k < held.cull_items.size(); k += 8) {   // ([5], [6]: a bare mesh's coarse range, which belongs to the tree each scene holds)
            CHECK(std::memcmp(&held.cull_items[k], &fresh.cull_items[k], 5 * 4) == 0 && std::memcmp(&held.cull_items[k + 7], &fresh.cull_items[k + 7], 4) == 0);
        }
        CHECK(held.mesh_bounds.size() == fresh.mesh_bounds.size() && std::memcmp(held.mesh_bounds.data(), fresh.mesh_bounds.data(), held.mesh_bounds.size() * 8) == 0);
        // a deformation that pushes the item out of what has bounds is refused, with the held scene untouched
        std::vector<double> huge = bounds;
        huge[3] = 1e305;
        const std::vector<ftd::CullRecord> before = held.culls;
        CHECK(g.reflatten_deformed(held, huge, err) == FT_ERR_UNSUPPORTED);
        CHECK(std::memcmp(before.data(), held.culls.data(), before.size() * sizeof(ftd::CullRecord)) == 0);
    }
    std::printf("refit_host_check: ok\n");
    return 0;
}

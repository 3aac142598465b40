// moved_host_check.cpp — the host half of "moved_in_place" (fth::SceneGraph::reflatten_moved, ft_scene.cpp) under
// AddressSanitizer + UBSan, as a stand-alone program (CPU only, no device object).  It builds a hand scene (a ground plane, a sphere under
// a translate, a cube under rotate + non-uniform scale, a mesh as `bspMesh 0` under scale + rotate + translate, a CSG subtract whose
// second operand moves, two directional lights) and a union of three cubes each under its own transform, flattens them, and then walks
// pose sequences - translations, rotations by 1 .. 180 degrees, a non-uniform scale change, a list that becomes the identity and leaves it
// again, a singular scale and back, the original pose - calling reflatten_moved on the held scene at every pose.  Where the call reports
// "in place", every array it wrote (each leaf's w2m and flags, m2w, culls, cull_items, cull_rows) equals a fresh flatten of the same graph
// byte for byte, every field it must keep (Leaf::ls_pairs, the rest of each leaf, every mesh and ls_* array, the program, the flags and
// capacities) is what it was, and every field a fresh flatten would change is among those written; where it refuses, the held scene is
// untouched, field for field, and the fresh flatten does differ in more than poses.  Both outcomes must occur.
// Build and run from the repository root:
//   g++ -fsanitize=address,undefined -fno-omit-frame-pointer -g -O1 -std=c++17 -ffp-contract=off tools/moved_host_check.cpp \
//       functracer_amd/csrc/ft_scene.cpp -o build/moved_host_check && build/moved_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../functracer_amd/csrc/ft_scene.h"

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); std::exit(1); } } while (0)

using fth::FlatScene;
using fth::GraphNode;
using fth::SceneGraph;
using Ops = std::vector<ft_transform>;

static ft_transform translate(double x, double y, double z) { ft_transform t{}; t.kind = FT_TRANSLATE; t.v[0] = x; t.v[1] = y; t.v[2] = z; return t; }
static ft_transform scale(double x, double y, double z) { ft_transform t{}; t.kind = FT_SCALE; t.v[0] = x; t.v[1] = y; t.v[2] = z; return t; }
static ft_transform rotate(double x, double y, double z, double deg) { ft_transform t{}; t.kind = FT_ROTATE; t.v[0] = x; t.v[1] = y; t.v[2] = z; t.angle = deg * 3.14159265358979323846 / 180.0; return t; }

static int32_t add(SceneGraph& g, GraphNode n) { g.nodes.push_back(std::move(n)); return (int32_t)g.nodes.size() - 1; }
static int32_t prim(SceneGraph& g, int32_t kind) { GraphNode n; n.kind = GraphNode::Prim; n.prim = kind; return add(g, n); }
static int32_t xform(SceneGraph& g, const Ops& ops, int32_t child) { GraphNode n; n.kind = GraphNode::Transform; n.xf = ops; n.children = {child}; return add(g, n); }
static int32_t csg(SceneGraph& g, int32_t op, int32_t a, int32_t b) { GraphNode n; n.kind = GraphNode::Csg; n.op = op; n.children = {a, b}; return add(g, n); }
static int32_t group(SceneGraph& g, std::vector<int32_t> kids) { GraphNode n; n.kind = GraphNode::Group; n.children = std::move(kids); return add(g, n); }
static int32_t material(SceneGraph& g, double r, double gr, double b, bool lit, int32_t child) {
    GraphNode n; n.kind = GraphNode::MaterialF;
    n.mat = ft_material{};
    n.mat.colour[0] = r; n.mat.colour[1] = gr; n.mat.colour[2] = b; n.mat.apply_lighting = lit ? 1 : 0;
    n.children = {child};
    return add(g, n);
}
// A bumpy closed strip of 2 * 48 triangles around the y axis: enough for a light-space tree (8 triangles and up).
static int32_t mesh(SceneGraph& g) {
    GraphNode n; n.kind = GraphNode::Mesh; n.depth = 0;
    const int ring = 48;
    auto at = [&](int k, double y) { const double a = 6.283185307179586 * (k % ring) / ring, r = 1.0 + 0.2 * std::sin(5.0 * a + y); return std::vector<double>{r * std::cos(a), y, r * std::sin(a)}; };
    for (int k = 0; k < ring; ++k) {
        const std::vector<double> a = at(k, -0.5), b = at(k + 1, -0.5), c = at(k, 0.6), d = at(k + 1, 0.6);
        for (const auto* t : {&a, &b, &c}) n.tris.insert(n.tris.end(), t->begin(), t->end());
        for (const auto* t : {&b, &d, &c}) n.tris.insert(n.tris.end(), t->begin(), t->end());
    }
    return add(g, n);
}
static void directional(SceneGraph& g, double x, double y, double z) {
    ftd::Light l{}; l.kind = ftd::LT_DIRECTIONAL;
    const double len = std::sqrt(x * x + y * y + z * z);
    l.v[0] = x / len; l.v[1] = y / len; l.v[2] = z / len; l.colour[0] = l.colour[1] = l.colour[2] = 1.0;
    g.lights.push_back(l);
}

template <class T> static bool same_bytes(const std::vector<T>& a, const std::vector<T>& b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
// Everything of a flattened scene a moved commit in place must keep (`poses` false) or may write (`poses` true), compared byte for byte.
static bool same_part(const FlatScene& a, const FlatScene& b, bool poses) {
    if (a.leaves.size() != b.leaves.size()) return false;
    if (poses) {
        for (size_t k = 0; k < a.leaves.size(); ++k)
            if (std::memcmp(a.leaves[k].w2m, b.leaves[k].w2m, sizeof a.leaves[k].w2m) != 0 || a.leaves[k].flags != b.leaves[k].flags) return false;
        return same_bytes(a.m2w, b.m2w) && same_bytes(a.culls, b.culls) && same_bytes(a.cull_items, b.cull_items) && same_bytes(a.cull_rows, b.cull_rows);
    }
    for (size_t k = 0; k < a.leaves.size(); ++k) {
        ftd::Leaf x = a.leaves[k], y = b.leaves[k];
        std::memset(x.w2m, 0, sizeof x.w2m); std::memset(y.w2m, 0, sizeof y.w2m);
        x.flags = y.flags = 0u;
        if (std::memcmp(&x, &y, sizeof x) != 0) return false;      // kind, material, mesh, ls_pairs, the builder nodes
    }
    return same_bytes(a.materials, b.materials) && same_bytes(a.lights, b.lights) && same_bytes(a.textures, b.textures) && a.tex_pixels == b.tex_pixels &&
           a.program == b.program && same_bytes(a.meshes, b.meshes) && same_bytes(a.nodes, b.nodes) && same_bytes(a.bsp_leaves, b.bsp_leaves) && same_bytes(a.tris, b.tris) &&
           a.tri_orig == b.tri_orig && a.tri_src == b.tri_src && a.run_nodes == b.run_nodes && same_bytes(a.wide, b.wide) && a.mesh_wide == b.mesh_wide &&
           same_bytes(a.coarse_boxes, b.coarse_boxes) && a.mesh_coarse == b.mesh_coarse && a.item_pc == b.item_pc && a.unbounded == b.unbounded &&
           a.cull_bundle == b.cull_bundle && same_bytes(a.mesh_bounds, b.mesh_bounds) && a.csg_capacity == b.csg_capacity && a.stack_capacity == b.stack_capacity &&
           a.bsp_stack_capacity == b.bsp_stack_capacity && a.any_reflective == b.any_reflective && a.any_texture == b.any_texture && a.mesh_under_csg == b.mesh_under_csg &&
           same_bytes(a.ls_pairs, b.ls_pairs) && a.ls_nodes == b.ls_nodes && same_bytes(a.ls_tris, b.ls_tris) && a.ls_src == b.ls_src && a.mesh_node == b.mesh_node &&
           a.wide_node == b.wide_node;
}
// What a fresh flatten of a moved graph may differ in from the held scene and a call in place still be right: the poses, and the
// light-space structures, which the caller of reflatten_moved brings up to the poses on the device.
static bool differs_in_poses_only(const FlatScene& fresh, FlatScene held) {
    held.ls_pairs = fresh.ls_pairs; held.ls_nodes = fresh.ls_nodes; held.ls_tris = fresh.ls_tris; held.ls_src = fresh.ls_src;
    if (held.leaves.size() != fresh.leaves.size()) return false;
    for (size_t k = 0; k < held.leaves.size(); ++k) held.leaves[k].ls_pairs = fresh.leaves[k].ls_pairs;
    return same_part(fresh, held, false) && fresh.cull_rows.size() == held.cull_rows.size() && fresh.culls.size() == held.culls.size() && fresh.cull_items.size() == held.cull_items.size();
}

struct Pose { const char* what; std::vector<std::pair<int32_t, Ops>> lists; };

static void walk(SceneGraph& g, const std::vector<Pose>& poses, const char* scene, int counts[2]) {
    std::string err;
    FlatScene held;
    CHECK(g.flatten(held, err) == FT_OK);
    for (const Pose& p : poses) {
        for (const auto& l : p.lists) g.nodes[(size_t)l.first].xf = l.second;
        FlatScene fresh;
        CHECK(g.flatten(fresh, err) == FT_OK);
        const FlatScene before = held;
        const int32_t rc = g.reflatten_moved(held, err);
        CHECK(rc == FT_OK || rc == FT_ERR_UNSUPPORTED);
        if (rc == FT_OK) {
            ++counts[0];
            CHECK(same_part(held, fresh, true));                    // what it wrote is the fresh flatten's
            CHECK(same_part(held, before, false));                  // what it must keep is what it was
            CHECK(differs_in_poses_only(fresh, before));            // and nothing else would have had to change
        } else {
            ++counts[1];
            CHECK(same_part(held, before, true) && same_part(held, before, false));   // untouched
            CHECK(!differs_in_poses_only(fresh, before));           // refused for a reason
            std::printf("moved_host_check: %s, %s: refused (%s)\n", scene, p.what, err.c_str());
            CHECK(g.flatten(held, err) == FT_OK);                   // the full commit the caller then takes
        }
    }
}

int main() {
    int hand[2] = {0, 0}, cubes[2] = {0, 0};
    {
        SceneGraph g;
        g.light_space_shadows = 2;
        const int32_t ground = material(g, 0.6, 0.6, 0.55, true, prim(g, FT_PRIM_PLANE));
        const Ops sphere0{translate(-4.0, 1.0, -2.0)}, cube0{rotate(0, 1, 0, 20.0), scale(2.0, 0.8, 1.0), translate(12.2, 2.75, 1.5)};
        const Ops mesh0{scale(2.0, 2.0, 2.0), rotate(0, 1, 0, 180.0), translate(-4.9, 3.2, 0.5)}, operand0{scale(0.8, 0.8, 0.8), translate(1.9, 1.2, -0.5)};
        const int32_t sphere = xform(g, sphere0, prim(g, FT_PRIM_SPHERE)), cube = xform(g, cube0, prim(g, FT_PRIM_CUBE)), m = xform(g, mesh0, mesh(g));
        const int32_t operand = xform(g, operand0, prim(g, FT_PRIM_SPHERE));
        const int32_t block = xform(g, Ops{scale(1.4, 1.4, 1.4), translate(1.8, 0.7, 0.0)}, prim(g, FT_PRIM_CUBE));
        g.root = group(g, {ground, material(g, 0.9, 0.3, 0.2, false, sphere), material(g, 0.2, 0.5, 0.9, true, cube), material(g, 0.8, 0.8, 0.3, true, m),
                           material(g, 0.3, 0.8, 0.4, true, csg(g, FT_CSG_SUBTRACT, block, operand))});
        directional(g, 0.4, -1.0, 0.6);
        directional(g, -1.0, -2.0, 0.5);
        std::vector<Pose> poses{{"translate only", {{sphere, {translate(-3.0, 1.0, -2.0)}}, {m, {mesh0[0], mesh0[1], translate(-4.5, 3.0, 0.7)}}}}};
        for (double deg : {1.0, 30.0, 90.0, 180.0})
            poses.push_back({"rotated", {{m, {mesh0[0], rotate(1, 2, 0.5, deg), mesh0[1], mesh0[2]}}, {cube, {rotate(0, 1, 0, 20.0 + deg), cube0[1], cube0[2]}}}});
        poses.push_back({"non-uniform scale", {{m, {scale(2.0, 1.5, 2.5), mesh0[1], mesh0[2]}}, {cube, {cube0[0], scale(2.0, 1.0, 0.7), cube0[2]}}, {operand, {scale(0.8, 0.6, 0.8), operand0[1]}}}});
        poses.push_back({"the identity", {{m, {translate(0, 0, 0)}}, {sphere, {scale(1, 1, 1)}}}});
        poses.push_back({"off the identity", {{m, mesh0}, {sphere, sphere0}}});
        poses.push_back({"singular", {{m, {scale(1, 0, 1), mesh0[1], mesh0[2]}}}});
        poses.push_back({"regular again", {{m, {scale(1.0, 0.5, 1.0), mesh0[1], mesh0[2]}}}});
        poses.push_back({"original", {{sphere, sphere0}, {cube, cube0}, {m, mesh0}, {operand, operand0}}});
        walk(g, poses, "hand scene", hand);
    }
    {
        // Three cubes in one union.  A and C aligned with the axes, B turned about y: x, y, z, B's x and z - five face directions (B's y row
        // is A's where the rotation's arithmetic gives exactly (0, 1, 0)).  Turning C about x as well takes the item past six: its OP_CULL
        // pair leaves the program.
        SceneGraph g;
        const Ops a0{translate(-0.4, 0.0, 0.0)}, b0{rotate(0, 1, 0, 30.0), translate(0.4, 0.1, 0.0)}, c0{translate(0.0, 0.5, 0.3)};
        const int32_t a = xform(g, a0, prim(g, FT_PRIM_CUBE)), b = xform(g, b0, prim(g, FT_PRIM_CUBE)), c = xform(g, c0, prim(g, FT_PRIM_CUBE));
        const int32_t whole = xform(g, Ops{translate(0.0, 1.0, 0.0)}, csg(g, FT_CSG_UNION, csg(g, FT_CSG_UNION, a, b), c));
        g.root = group(g, {material(g, 0.5, 0.5, 0.5, true, whole), material(g, 0.6, 0.6, 0.6, true, xform(g, Ops{scale(8, 1, 8), translate(-4, 0, -4)}, prim(g, FT_PRIM_SQUARE)))});
        directional(g, 0.3, -1.0, 0.2);
        std::vector<Pose> poses{{"slid", {{whole, {translate(0.5, 1.0, 0.0)}}}},
                                {"B turned further", {{b, {rotate(0, 1, 0, 50.0), b0[1]}}}},
                                {"the union turned", {{whole, {rotate(0, 1, 0, 40.0), translate(0.5, 1.0, 0.0)}}}},
                                {"C turned: past six directions", {{c, {rotate(1, 0, 0, 20.0), c0[0]}}}},
                                {"C turned further", {{c, {rotate(1, 0, 0, 35.0), c0[0]}}}},
                                {"C back: six or fewer again", {{c, c0}}},
                                {"original", {{whole, {translate(0.0, 1.0, 0.0)}}, {b, b0}}}};
        walk(g, poses, "three-cube union", cubes);
    }
    CHECK(hand[0] > 0 && cubes[0] > 0 && cubes[1] > 0);
    std::printf("moved_host_check: ok (hand scene: %d in place, %d refused; three-cube union: %d in place, %d refused)\n", hand[0], hand[1], cubes[0], cubes[1]);
    return 0;
}

// deform_ls_host_check.cpp — the host side of "deform_light_space"  under AddressSanitizer + UBSan, as a stand-alone
// program (CPU only; the flattener alone, no device object).  It checks what ft_scene_commit_deformed relies on:
//   - after a fresh flatten every record of ls_tris is the bitwise copy of tris[ls_src[i]], trees and grids alike, with duplicate
//     triangles in the mesh (where matching records after the fact could not tell the copies apart);
//   - c, R, s_abs and pad derived from new vertices alone (fth::scan_mesh, fth::ls_pair_extent) are what a fresh flatten of those
//     vertices writes into the pair record, bit for bit.
// Build and run from the repository root:
//   g++ -fsanitize=address,undefined -fno-omit-frame-pointer -g -O1 -std=c++17 -ffp-contract=off tools/deform_ls_host_check.cpp \
//       functracer_amd/csrc/ft_scene.cpp -o build/deform_ls_host_check && build/deform_ls_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static fth::SceneGraph graph_of(const std::vector<double>& tris, int shadows) {
    fth::SceneGraph g;
    auto add = [&](fth::GraphNode n) { g.nodes.push_back(std::move(n)); return (int32_t)g.nodes.size() - 1; };
    fth::GraphNode m; m.kind = fth::GraphNode::Mesh; m.tris = tris;
    const int32_t mesh = add(m);
    fth::GraphNode t1; t1.kind = fth::GraphNode::Transform; t1.xf = {ft_transform{FT_ROTATE, 0, {0, 1, 0}, 0.7}}; t1.children = {mesh};
    fth::GraphNode s; s.kind = fth::GraphNode::Prim; s.prim = FT_PRIM_SPHERE;
    fth::GraphNode grp; grp.kind = fth::GraphNode::Group; grp.children = {add(t1), add(s)};
    g.root = add(grp);
    const double dirs[2][3] = {{0.0, -1.0, 0.0}, {0.4, -0.8, 0.2}};
    for (const double* v : {dirs[0], dirs[1]}) {
        ftd::Light l{};
        const double len = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        for (int q = 0; q < 3; ++q) { l.v[q] = v[q] / len; l.colour[q] = 1.0; }
        l.kind = ftd::LT_DIRECTIONAL;
        g.lights.push_back(l);
    }
    g.light_space_shadows = shadows;
    return g;
}

int main() {
    for (int shadows = 1; shadows <= 2; ++shadows) {
        std::vector<double> a = blob(400, 7);
        for (int k = 0; k < 40; ++k) std::memcpy(&a[(size_t)9 * (200 + k)], &a[(size_t)9 * k], 72);   // forty triangles twice
        fth::SceneGraph g = graph_of(a, shadows);
        fth::FlatScene held;
        std::string err;
        CHECK(g.flatten(held, err) == FT_OK);
        const size_t n_recs = held.ls_tris.size() / 9;
        CHECK(held.ls_src.size() == n_recs && n_recs >= 800);      // two trees at least (and under option 2 the grids' entries behind each)
        CHECK(shadows == 1 || n_recs > 800);
        for (size_t i = 0; i < n_recs; ++i) {
            CHECK((size_t)held.ls_src[i] < held.tris.size() / 9);
            CHECK(std::memcmp(&held.ls_tris[9 * i], &held.tris[9 * (size_t)held.ls_src[i]], 72) == 0);
        }
        // every list-order triangle is named by each tree exactly once: the first 400 records of each pair's run
        CHECK(held.leaves[0].ls_pairs != ~0u);
        const ftd::BspLeaf src = held.bsp_leaves[(size_t)~held.meshes[held.leaves[0].mesh].root];
        CHECK(src.n_tris == 400);
        {
            std::vector<int> named(400, 0);
            for (size_t i = 0; i < 400; ++i) { CHECK(held.ls_src[i] >= src.first_tri && held.ls_src[i] - src.first_tri < 400); ++named[held.ls_src[i] - src.first_tri]; }
            for (int k : named) CHECK(k == 1);
        }
        // the derivation from new vertices against a fresh flatten of them
        const std::vector<std::vector<double>> moved = {blob(400, 8, 0.0, 3.0), blob(400, 7, 1e3), blob(400, 7, 0.0, 1.0 / 256.0), std::vector<double>(a.size(), 0.25)};
        for (const std::vector<double>& v : moved) {
            const fth::MeshScan sc = fth::scan_mesh(v.data(), 400);
            CHECK(sc.finite);
            const double c[3] = {0.5 * (sc.bounds[0] + sc.bounds[3]), 0.5 * (sc.bounds[1] + sc.bounds[4]), 0.5 * (sc.bounds[2] + sc.bounds[5])};
            const double R = fth::ls_pair_extent(v.data(), 400, true, c);
            fth::SceneGraph g2 = graph_of(v, shadows);
            fth::FlatScene fresh;
            CHECK(g2.flatten(fresh, err) == FT_OK && fresh.leaves[0].ls_pairs != ~0u);
            const ftd::BspLeaf s2 = fresh.bsp_leaves[(size_t)~fresh.meshes[fresh.leaves[0].mesh].root];
            CHECK(R == fth::ls_pair_extent(&fresh.tris[9 * (size_t)s2.first_tri], s2.n_tris, false, c));   // records or vertices: one sum
            for (size_t l = 0; l < g2.lights.size(); ++l) {
                const double* rec = &fresh.ls_pairs[(size_t)ftd::kLsPairDoubles * (fresh.leaves[0].ls_pairs + l)];
                int32_t root;
                std::memcpy(&root, &rec[14], 4);
                CHECK(root >= 0);
                fth::LsPairFrame fr;
                CHECK(fth::ls_pair_frame(held.leaves[0], g2.lights[l], fr));   // the frame of the HELD leaf: it does not depend on the vertices
                const double want[14] = {fr.U[0], fr.U[1], fr.U[2], fr.V[0], fr.V[1], fr.V[2], fr.D[0], fr.D[1], fr.D[2], c[0], c[1], c[2], fr.k_rel, (fr.k_rel + 1e-6) * R + 1e-20};
                CHECK(std::memcmp(rec, want, sizeof want) == 0);
            }
        }
    }
    std::printf("deform_ls_host_check: ok\n");
    return 0;
}

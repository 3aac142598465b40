// morph_host_check.cpp — the host side of morph targets under AddressSanitizer + UBSan, as a stand-alone program (CPU only).
// It drives a host-only context through ft_sg_set_mesh_targets / ft_sg_set_mesh_weights and every refusal, through the commits that blend
// the vertices only when they are needed (ft_scene_commit, ft_scene_commit_moved, ft_scene_commit_deformed) and through fth::morph_blend
// and GraphNode::vertices directly, against the formula evaluated here.
// Build and run from the repository root (the device objects are linked as they are: make -C functracer_amd/csrc first):
//   C=functracer_amd/csrc; S="-fsanitize=address,undefined -fno-omit-frame-pointer -g -O1 -std=c++17 -ffp-contract=off"
//   g++ $S -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include tools/morph_host_check.cpp $C/ft_capi.cpp $C/ft_frame.cpp $C/ft_progressive.cpp \
//       $C/ft_passes.cpp $C/ft_debug.cpp $C/ft_scene.cpp $(for o in $(make -s -C $C print-DEVICE_OBJS); do echo $C/$o; done) \
//       -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib -o build/morph_host_check && build/morph_host_check
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
// The header's formula, spelled out: D_k = T_k - B, then product and sum rounded apart.
static std::vector<double> blend(const std::vector<double>& B, const std::vector<double>& T, const std::vector<double>& w) {
    std::vector<double> v(B.size());
    for (size_t i = 0; i < B.size(); ++i) {
        double acc = B[i];
        for (size_t k = 0; k < w.size(); ++k) { volatile double d = T[k * B.size() + i] - B[i]; volatile double p = w[k] * d; acc = acc + p; }
        v[i] = acc;
    }
    return v;
}
// The list-order records of the first mesh of the committed scene against vertices `v`.
static bool committed_is(ft_context* c, const std::vector<double>& v) {
    int64_t sizes[12] = {0};
    if (ft_debug_mesh_trees(c, sizes, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != FT_OK) return false;
    std::vector<double> tris((size_t)sizes[2] * 9);
    std::vector<char> nodes((size_t)sizes[0] * 256);
    std::vector<int32_t> meshes((size_t)sizes[7] * 6);
    std::vector<float> coarse((size_t)sizes[6] * 6);
    std::vector<uint32_t> leaves((size_t)sizes[1] * 2), orig((size_t)sizes[3]), src((size_t)sizes[4]), jobs((size_t)sizes[8] * 9);
    std::vector<double> wide((size_t)sizes[5] * 28);
    if (ft_debug_mesh_trees(c, sizes, nodes.data(), leaves.data(), tris.data(), orig.data(), src.data(), wide.data(), coarse.data(), meshes.data(), jobs.data()) != FT_OK) return false;
    if (tris.size() < v.size()) return false;
    for (size_t i = 0; i < v.size(); i += 9)
        for (int a = 0; a < 3; ++a) {
            const double rec[3] = {v[i + a], v[i + 3 + a] - v[i + a], v[i + 6 + a] - v[i + a]};
            const double got[3] = {tris[i + a], tris[i + 3 + a], tris[i + 6 + a]};
            if (std::memcmp(rec, got, sizeof rec) != 0) return false;
        }
    return true;
}

int main() {
    const int n = 300;
    const std::vector<double> B = blob(n, 1);
    std::vector<double> T = blob(n, 2, 0.5);
    { const std::vector<double> t1 = blob(n, 3, 0.0, 2.0), t2 = blob(n, 1, 1e3); T.insert(T.end(), t1.begin(), t1.end()); T.insert(T.end(), t2.begin(), t2.end()); }
    ft_context* c = nullptr;
    CHECK(ft_create_host_only(&c) == FT_OK);
    const ft_node mesh = ft_sg_bsp_mesh(c, 0, B.data(), n);
    const ft_transform up{FT_TRANSLATE, 0, {0, 3, 0}, 0};
    const ft_node xf = ft_sg_transform(c, &up, 1, mesh);
    CHECK(ft_scene_set_objects(c, ft_sg_group(c, &xf, 1)) == FT_OK);
    const double dir[3] = {0, -1, 1}, white[3] = {1, 1, 1};
    CHECK(ft_scene_add_directional(c, dir, white) == FT_OK && ft_scene_commit(c) == FT_OK && committed_is(c, B));
    CHECK(ft_set_option(c, "morph_on_device", 0) == FT_OK && ft_set_option(c, "morph_on_device", 1) == FT_OK);
    // ---- refusals: nothing changes
    std::vector<double> w = {0.25, -0.5, 0.001};
    CHECK(ft_sg_set_mesh_weights(c, mesh, w.data(), 3) == FT_ERR_INVALID);
    CHECK(ft_sg_set_mesh_targets(nullptr, mesh, T.data(), 3, n) == FT_ERR_INVALID && ft_sg_set_mesh_targets(c, -1, T.data(), 3, n) == FT_ERR_INVALID);
    CHECK(ft_sg_set_mesh_targets(c, xf, T.data(), 3, n) == FT_ERR_INVALID && ft_sg_set_mesh_targets(c, mesh, T.data(), 3, n - 1) == FT_ERR_INVALID);
    CHECK(ft_sg_set_mesh_targets(c, mesh, T.data(), 17, n) == FT_ERR_INVALID && ft_sg_set_mesh_targets(c, mesh, T.data(), -1, n) == FT_ERR_INVALID);
    CHECK(ft_sg_set_mesh_targets(c, mesh, nullptr, 3, n) == FT_ERR_INVALID);
    CHECK(ft_sg_set_mesh_targets(c, mesh, T.data(), 3, n) == FT_OK);
    CHECK(ft_sg_set_mesh_weights(c, mesh, w.data(), 2) == FT_ERR_INVALID && ft_sg_set_mesh_weights(c, mesh, nullptr, 3) == FT_ERR_INVALID);
    std::vector<double> bad = w;
    bad[1] = std::numeric_limits<double>::quiet_NaN();
    CHECK(ft_sg_set_mesh_weights(c, mesh, bad.data(), 3) == FT_ERR_INVALID);
    bad[1] = std::numeric_limits<double>::infinity();
    CHECK(ft_sg_set_mesh_weights(c, mesh, bad.data(), 3) == FT_ERR_INVALID);
    CHECK(ft_scene_commit_deformed(c) == FT_OK && committed_is(c, B));
    // ---- the three commits that need the vertices
    CHECK(ft_sg_set_mesh_weights(c, mesh, w.data(), 3) == FT_OK && ft_scene_commit_deformed(c) == FT_OK && committed_is(c, blend(B, T, w)));
    int64_t counts[4];
    double scan[8];
    CHECK(ft_debug_morph(c, mesh, counts, scan) == FT_OK && counts[0] == 0 && counts[1] == 0 && counts[2] == 1 && counts[3] == 0 && scan[7] == 0.0 && scan[6] > 0.0);
    CHECK(ft_debug_morph(c, xf, counts, scan) == FT_ERR_INVALID && ft_debug_morph(c, mesh, nullptr, scan) == FT_ERR_INVALID);
    w = {0.0, 1.0, 0.0};
    CHECK(ft_sg_set_mesh_weights(c, mesh, w.data(), 3) == FT_OK && ft_scene_commit(c) == FT_OK && committed_is(c, blend(B, T, w)));
    w = {1.0, 1.0, 0.5};
    CHECK(ft_sg_set_mesh_weights(c, mesh, w.data(), 3) == FT_OK && ft_sg_set_transform(c, xf, &up, 1) == FT_OK);
    CHECK(ft_scene_commit_deformed(c) == FT_ERR_STATE && ft_scene_commit_moved(c) == FT_OK && committed_is(c, blend(B, T, w)));
    // explicit vertices between two weight sets: base and deltas stay
    const std::vector<double> E = blob(n, 9);
    CHECK(ft_sg_set_mesh_weights(c, mesh, w.data(), 3) == FT_OK && ft_sg_set_mesh_triangles(c, mesh, E.data(), n) == FT_OK);
    CHECK(ft_scene_commit_deformed(c) == FT_OK && committed_is(c, E));
    CHECK(ft_sg_set_mesh_weights(c, mesh, w.data(), 3) == FT_OK && ft_scene_commit_deformed(c) == FT_OK && committed_is(c, blend(B, T, w)));
    // an overflow is refused and the next pose commits
    bad = {1e308, 0.0, 0.0};
    CHECK(ft_sg_set_mesh_weights(c, mesh, bad.data(), 3) == FT_OK && ft_scene_commit_deformed(c) == FT_ERR_UNSUPPORTED && committed_is(c, blend(B, T, w)));
    w = {0.5, 0.5, 0.0};
    CHECK(ft_sg_set_mesh_weights(c, mesh, w.data(), 3) == FT_OK && ft_scene_commit_deformed(c) == FT_OK && committed_is(c, blend(B, T, w)));
    // new targets over the blended vertices; then none
    const std::vector<double> B2 = blend(B, T, w);
    std::vector<double> one(T.begin(), T.begin() + (long)B.size()), w1 = {0.75};
    CHECK(ft_sg_set_mesh_targets(c, mesh, one.data(), 1, n) == FT_OK && ft_scene_commit_deformed(c) == FT_OK && committed_is(c, B2));
    CHECK(ft_sg_set_mesh_weights(c, mesh, w1.data(), 1) == FT_OK && ft_scene_commit_deformed(c) == FT_OK && committed_is(c, blend(B2, one, w1)));
    CHECK(ft_sg_set_mesh_targets(c, mesh, nullptr, 0, n) == FT_OK && ft_sg_set_mesh_weights(c, mesh, w1.data(), 1) == FT_ERR_INVALID);
    CHECK(ft_scene_commit(c) == FT_OK && committed_is(c, blend(B2, one, w1)));
    ft_destroy(c);

    // ---- fth::morph_blend and the accessor directly, sixteen targets, an odd count
    {
        const size_t count = 9 * 7;
        std::vector<double> base = blob(7, 4), deltas, ws;
        std::vector<double> targets;
        for (int k = 0; k < 16; ++k) { const std::vector<double> t = blob(7, 10 + (unsigned)k, 0.1 * k); targets.insert(targets.end(), t.begin(), t.end()); ws.push_back(0.1 * (k - 7)); }
        deltas.resize(targets.size());
        for (int k = 0; k < 16; ++k) for (size_t i = 0; i < count; ++i) deltas[(size_t)k * count + i] = targets[(size_t)k * count + i] - base[i];
        std::vector<double> out(count);
        fth::morph_blend(base.data(), deltas.data(), ws.data(), 16, count, out.data());
        const std::vector<double> want = blend(base, targets, ws);
        CHECK(std::memcmp(out.data(), want.data(), count * 8) == 0);
        fth::GraphNode m; m.kind = fth::GraphNode::Mesh; m.tris = base; m.base = base; m.deltas = deltas; m.weights = ws; m.n_targets = 16; m.by_weights = true; m.tris_stale = true;
        CHECK(std::memcmp(m.vertices().data(), want.data(), count * 8) == 0 && !m.tris_stale);
        const fth::MeshScan s = fth::scan_mesh(m.vertices().data(), 7);
        CHECK(s.finite && s.extent > 0.0);
    }
    std::printf("morph_host_check: ok\n");
    return 0;
}

// skin_host_check.cpp — the host side of skinning under AddressSanitizer + UBSan, as a stand-alone program (CPU only).
// It drives a host-only context through ft_sg_set_mesh_skin / ft_sg_set_mesh_bones and every refusal, through the commits that skin the
// vertices only when they are needed (ft_scene_commit, ft_scene_commit_moved, ft_scene_commit_deformed), morph targets under a skin,
// removal of palette and skin, a palette of 256 bones, and through fth::skin_blend and GraphNode::vertices directly, against the formula
// evaluated here.
// Build and run from the repository root (the device objects are linked as they are: make -C functracer_amd/csrc first):
//   C=functracer_amd/csrc; S="-fsanitize=address,undefined -fno-omit-frame-pointer -g -O1 -std=c++17 -ffp-contract=off"
//   g++ $S -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include tools/skin_host_check.cpp $C/ft_capi.cpp $C/ft_frame.cpp $C/ft_progressive.cpp \
//       $C/ft_passes.cpp $C/ft_debug.cpp $C/ft_scene.cpp $(for o in $(make -s -C $C print-DEVICE_OBJS); do echo $C/$o; done) \
//       -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,/opt/rocm/lib -o build/skin_host_check && build/skin_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../functracer_amd/csrc/ft_scene.h"

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); std::exit(1); } } while (0)

static std::vector<double> blob(int n, unsigned seed, double shift = 0.0) {
    std::mt19937 rng(seed);
    std::normal_distribution<double> g;
    std::vector<double> t((size_t)9 * n);
    for (int i = 0; i < n; ++i) {
        const double c[3] = {0.8 * g(rng), 0.8 * g(rng), 0.8 * g(rng)};
        for (int k = 0; k < 9; ++k) t[(size_t)9 * i + k] = c[k % 3] + 0.08 * g(rng) + shift;
    }
    return t;
}
// Bone matrices near the identity: a small shear and scale per bone, and a translation.
static std::vector<double> bones(int n, unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> u(-0.2, 0.2);
    std::vector<double> m((size_t)12 * n);
    for (int b = 0; b < n; ++b) for (int i = 0; i < 3; ++i) for (int k = 0; k < 4; ++k) m[(size_t)12 * b + 4 * i + k] = (i == k ? 1.0 : 0.0) + u(rng);
    return m;
}
struct Skin { std::vector<int32_t> index; std::vector<double> weight; int J; };
static Skin skin_of(int n_tris, int J, int n_bones, unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_int_distribution<int> pick(0, n_bones - 1);
    std::uniform_real_distribution<double> u(-0.5, 1.0);
    Skin s{std::vector<int32_t>((size_t)3 * n_tris * J), std::vector<double>((size_t)3 * n_tris * J), J};
    for (size_t k = 0; k < s.index.size(); ++k) { s.index[k] = pick(rng); s.weight[k] = u(rng); }
    s.index.back() = n_bones - 1;
    return s;
}
// The header's formula, spelled out: every product and sum rounded apart.
static std::vector<double> posed(const std::vector<double>& U, const Skin& s, const std::vector<double>& P) {
    std::vector<double> v(U.size());
    for (size_t c = 0; c < U.size() / 3; ++c) {
        const double x = U[3 * c], y = U[3 * c + 1], z = U[3 * c + 2];
        for (int i = 0; i < 3; ++i) {
            double acc = 0.0;
            for (int j = 0; j < s.J; ++j) {
                const double* M = &P[(size_t)12 * s.index[c * s.J + j] + 4 * i];
                volatile double px = M[0] * x, py = M[1] * y, pz = M[2] * z;
                volatile double t = px + py;
                t = t + pz;
                t = t + M[3];
                volatile double q = s.weight[c * s.J + j] * t;
                acc = j == 0 ? (double)q : acc + q;
            }
            v[3 * c + i] = acc;
        }
    }
    return v;
}
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
    const std::vector<double> U = blob(n, 1);
    const Skin s = skin_of(n, 3, 5, 7);
    const std::vector<double> P = bones(5, 11);
    ft_context* c = nullptr;
    CHECK(ft_create_host_only(&c) == FT_OK);
    const ft_node mesh = ft_sg_bsp_mesh(c, 0, U.data(), n);
    const ft_transform up{FT_TRANSLATE, 0, {0, 3, 0}, 0};
    const ft_node xf = ft_sg_transform(c, &up, 1, mesh);
    CHECK(ft_scene_set_objects(c, ft_sg_group(c, &xf, 1)) == FT_OK);
    const double dir[3] = {0, -1, 1}, white[3] = {1, 1, 1};
    CHECK(ft_scene_add_directional(c, dir, white) == FT_OK && ft_scene_commit(c) == FT_OK && committed_is(c, U));
    CHECK(ft_set_option(c, "skin_on_device", 0) == FT_OK && ft_set_option(c, "skin_on_device", 1) == FT_OK);
    // ---- refusals: nothing changes
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    CHECK(ft_sg_set_mesh_bones(c, mesh, P.data(), 5) == FT_ERR_INVALID);
    CHECK(ft_sg_set_mesh_skin(nullptr, mesh, s.index.data(), s.weight.data(), 3, n) == FT_ERR_INVALID && ft_sg_set_mesh_skin(c, -1, s.index.data(), s.weight.data(), 3, n) == FT_ERR_INVALID);
    CHECK(ft_sg_set_mesh_skin(c, xf, s.index.data(), s.weight.data(), 3, n) == FT_ERR_INVALID && ft_sg_set_mesh_skin(c, mesh, s.index.data(), s.weight.data(), 3, n - 1) == FT_ERR_INVALID);
    CHECK(ft_sg_set_mesh_skin(c, mesh, s.index.data(), s.weight.data(), 5, n) == FT_ERR_INVALID && ft_sg_set_mesh_skin(c, mesh, s.index.data(), s.weight.data(), -1, n) == FT_ERR_INVALID);
    CHECK(ft_sg_set_mesh_skin(c, mesh, nullptr, s.weight.data(), 3, n) == FT_ERR_INVALID && ft_sg_set_mesh_skin(c, mesh, s.index.data(), nullptr, 3, n) == FT_ERR_INVALID);
    {
        Skin bad = s;
        bad.index[100] = 256;
        CHECK(ft_sg_set_mesh_skin(c, mesh, bad.index.data(), bad.weight.data(), 3, n) == FT_ERR_INVALID);
        bad.index[100] = -1;
        CHECK(ft_sg_set_mesh_skin(c, mesh, bad.index.data(), bad.weight.data(), 3, n) == FT_ERR_INVALID);
        bad = s;
        bad.weight[2699] = nan;
        CHECK(ft_sg_set_mesh_skin(c, mesh, bad.index.data(), bad.weight.data(), 3, n) == FT_ERR_INVALID);
        bad.weight[2699] = -inf;
        CHECK(ft_sg_set_mesh_skin(c, mesh, bad.index.data(), bad.weight.data(), 3, n) == FT_ERR_INVALID);
    }
    CHECK(ft_sg_set_mesh_bones(c, mesh, P.data(), 5) == FT_ERR_INVALID);
    CHECK(ft_sg_set_mesh_skin(c, mesh, s.index.data(), s.weight.data(), 3, n) == FT_OK);
    CHECK(ft_sg_set_mesh_bones(nullptr, mesh, P.data(), 5) == FT_ERR_INVALID && ft_sg_set_mesh_bones(c, xf, P.data(), 5) == FT_ERR_INVALID);
    CHECK(ft_sg_set_mesh_bones(c, mesh, nullptr, 5) == FT_ERR_INVALID && ft_sg_set_mesh_bones(c, mesh, P.data(), 4) == FT_ERR_INVALID);
    CHECK(ft_sg_set_mesh_bones(c, mesh, P.data(), -1) == FT_ERR_INVALID && ft_sg_set_mesh_bones(c, mesh, P.data(), 257) == FT_ERR_INVALID);
    {
        std::vector<double> bad = P;
        bad[17] = nan;
        CHECK(ft_sg_set_mesh_bones(c, mesh, bad.data(), 5) == FT_ERR_INVALID);
        bad[17] = inf;
        CHECK(ft_sg_set_mesh_bones(c, mesh, bad.data(), 5) == FT_ERR_INVALID);
    }
    CHECK(ft_scene_commit_deformed(c) == FT_OK && committed_is(c, U));
    // ---- the three commits that need the vertices
    CHECK(ft_sg_set_mesh_bones(c, mesh, P.data(), 5) == FT_OK && ft_scene_commit_deformed(c) == FT_OK && committed_is(c, posed(U, s, P)));
    int64_t counts[4];
    CHECK(ft_debug_skin(c, mesh, counts) == FT_OK && counts[0] == 0 && counts[1] == 0 && counts[2] == 1 && counts[3] == 0);
    CHECK(ft_debug_skin(c, xf, counts) == FT_ERR_INVALID && ft_debug_skin(c, mesh, nullptr) == FT_ERR_INVALID);
    const std::vector<double> P2 = bones(5, 12), P3 = bones(6, 13);
    CHECK(ft_sg_set_mesh_bones(c, mesh, P2.data(), 5) == FT_OK && ft_scene_commit(c) == FT_OK && committed_is(c, posed(U, s, P2)));
    CHECK(ft_sg_set_mesh_bones(c, mesh, P3.data(), 6) == FT_OK && ft_sg_set_transform(c, xf, &up, 1) == FT_OK);
    CHECK(ft_scene_commit_deformed(c) == FT_ERR_STATE && ft_scene_commit_moved(c) == FT_OK && committed_is(c, posed(U, s, P3)));
    // a new shape under the palette in force
    const std::vector<double> E = blob(n, 9);
    CHECK(ft_sg_set_mesh_triangles(c, mesh, E.data(), n) == FT_OK && ft_scene_commit_deformed(c) == FT_OK && committed_is(c, posed(E, s, P3)));
    // morph under skin: the targets' base is the shape, the pose is skin(blend)
    std::vector<double> T = blob(n, 2, 0.5);
    { const std::vector<double> t1 = blob(n, 3, -0.25); T.insert(T.end(), t1.begin(), t1.end()); }
    const std::vector<double> w = {0.25, -0.5};
    CHECK(ft_sg_set_mesh_targets(c, mesh, T.data(), 2, n) == FT_OK && ft_scene_commit_deformed(c) == FT_OK && committed_is(c, posed(E, s, P3)));
    CHECK(ft_sg_set_mesh_weights(c, mesh, w.data(), 2) == FT_OK && ft_scene_commit_deformed(c) == FT_OK && committed_is(c, posed(blend(E, T, w), s, P3)));
    CHECK(ft_sg_set_mesh_bones(c, mesh, P.data(), 5) == FT_OK && ft_scene_commit(c) == FT_OK && committed_is(c, posed(blend(E, T, w), s, P)));
    // an overflow is refused and the next pose commits
    const std::vector<double> over((size_t)12 * 5, 1e300);
    CHECK(ft_sg_set_mesh_bones(c, mesh, over.data(), 5) == FT_OK && ft_scene_commit_deformed(c) == FT_ERR_UNSUPPORTED && committed_is(c, posed(blend(E, T, w), s, P)));
    CHECK(ft_sg_set_mesh_bones(c, mesh, P2.data(), 5) == FT_OK && ft_scene_commit_deformed(c) == FT_OK && committed_is(c, posed(blend(E, T, w), s, P2)));
    // removal: the palette, then the skin
    CHECK(ft_sg_set_mesh_bones(c, mesh, nullptr, 0) == FT_OK && ft_scene_commit_deformed(c) == FT_OK && committed_is(c, blend(E, T, w)));
    CHECK(ft_sg_set_mesh_bones(c, mesh, P.data(), 5) == FT_OK && ft_scene_commit_deformed(c) == FT_OK && committed_is(c, posed(blend(E, T, w), s, P)));
    CHECK(ft_sg_set_mesh_skin(c, mesh, nullptr, nullptr, 0, n) == FT_OK && ft_sg_set_mesh_bones(c, mesh, P.data(), 5) == FT_ERR_INVALID);
    CHECK(ft_scene_commit_deformed(c) == FT_OK && committed_is(c, blend(E, T, w)));
    // 256 bones, four influences
    const Skin s4 = skin_of(n, 4, 256, 21);
    const std::vector<double> P256 = bones(256, 22);
    CHECK(ft_sg_set_mesh_skin(c, mesh, s4.index.data(), s4.weight.data(), 4, n) == FT_OK && ft_sg_set_mesh_bones(c, mesh, P256.data(), 255) == FT_ERR_INVALID);
    CHECK(ft_sg_set_mesh_bones(c, mesh, P256.data(), 256) == FT_OK && ft_scene_commit_deformed(c) == FT_OK && committed_is(c, posed(blend(E, T, w), s4, P256)));
    CHECK(ft_scene_clear(c) == FT_OK);
    ft_destroy(c);

    // ---- fth::skin_blend and the accessors directly, an odd corner count
    {
        const std::vector<double> shape = blob(7, 4);
        const Skin k = skin_of(7, 4, 256, 5);
        std::vector<uint32_t> words(21, 0u);
        for (size_t q = 0; q < 21; ++q) for (int j = 0; j < 4; ++j) words[q] |= (uint32_t)k.index[q * 4 + j] << (8 * j);
        std::vector<double> out(shape.size());
        fth::skin_blend(shape.data(), words.data(), k.weight.data(), 4, P256.data(), 21, out.data());
        const std::vector<double> want = posed(shape, k, P256);
        CHECK(std::memcmp(out.data(), want.data(), out.size() * 8) == 0);
        fth::GraphNode m; m.kind = fth::GraphNode::Mesh; m.tris = shape; m.skin_index = words; m.skin_weight = k.weight; m.skin_influences = 4; m.skin_max_index = 255;
        CHECK(&m.vertices() == &m.shape());
        m.palette = P256; m.n_bones = 256; m.posed_stale = true;
        CHECK(std::memcmp(m.vertices().data(), want.data(), out.size() * 8) == 0 && !m.posed_stale && m.host_skins == 1);
        CHECK(std::memcmp(m.shape().data(), shape.data(), out.size() * 8) == 0 && m.vertices().size() == shape.size() && m.host_skins == 1);
    }
    std::printf("skin_host_check: ok\n");
    return 0;
}

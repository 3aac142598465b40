// skin_dq_host_check.cpp — the host side of dual-quaternion skinning under AddressSanitizer + UBSan, as a stand-alone
// program (CPU only).  It drives a host-only context through ft_sg_set_mesh_bones_dq and every refusal, the switches between the two
// palette kinds and their removal, the commits that skin the vertices only when they are needed (ft_scene_commit, ft_scene_commit_moved,
// ft_scene_commit_deformed), morph targets under the skin, a palette of 256 bones and the zero-blend refusal, and through
// fth::skin_blend_dq and GraphNode::vertices directly, against the formula evaluated here.
// Build and run from the repository root by the recipe at the top of tools/skin_host_check.cpp, with this file in place of that one
// and build/skin_dq_host_check as the output.
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
// Bone matrices near the identity (the other palette kind).
static std::vector<double> bones(int n, unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> u(-0.2, 0.2);
    std::vector<double> m((size_t)12 * n);
    for (int b = 0; b < n; ++b) for (int i = 0; i < 3; ++i) for (int k = 0; k < 4; ++k) m[(size_t)12 * b + 4 * i + k] = (i == k ? 1.0 : 0.0) + u(rng);
    return m;
}
// Unit dual quaternions of small rotations and translations; the odd bones negated (the same motions).
static std::vector<double> dual_quaternions(int n, unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> u(-1.0, 1.0);
    std::vector<double> d((size_t)8 * n);
    for (int b = 0; b < n; ++b) {
        double ax[3] = {u(rng), u(rng), u(rng) + 1.5};
        const double len = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]), ang = 0.6 * u(rng);
        const double r[4] = {std::cos(0.5 * ang), std::sin(0.5 * ang) * ax[0] / len, std::sin(0.5 * ang) * ax[1] / len, std::sin(0.5 * ang) * ax[2] / len};
        const double t[3] = {0.3 * u(rng), 0.3 * u(rng), 0.3 * u(rng)};
        double* D = &d[(size_t)8 * b];
        for (int k = 0; k < 4; ++k) D[k] = r[k];
        D[4] = -0.5 * (t[0] * r[1] + t[1] * r[2] + t[2] * r[3]);     // 0.5 * (0, t) (x) r
        D[5] = 0.5 * (r[0] * t[0] + (t[1] * r[3] - t[2] * r[2]));
        D[6] = 0.5 * (r[0] * t[1] + (t[2] * r[1] - t[0] * r[3]));
        D[7] = 0.5 * (r[0] * t[2] + (t[0] * r[2] - t[1] * r[1]));
        if (b & 1) for (int k = 0; k < 8; ++k) D[k] = -D[k];
    }
    return d;
}
struct Skin { std::vector<int32_t> index; std::vector<double> weight; int J; };
static Skin skin_of(int n_tris, int J, int n_bones, unsigned seed) {
    std::mt19937 rng(seed);
    std::uniform_int_distribution<int> pick(0, n_bones - 1);
    std::uniform_real_distribution<double> u(0.1, 1.0);
    Skin s{std::vector<int32_t>((size_t)3 * n_tris * J), std::vector<double>((size_t)3 * n_tris * J), J};
    for (size_t k = 0; k < s.index.size(); ++k) { s.index[k] = pick(rng); s.weight[k] = u(rng); }
    s.index.back() = n_bones - 1;
    return s;
}
// The header's formula, spelled out: every operation rounded apart (volatile keeps each result a double of its own).
static double crossi(const double a[3], const double b[3], int i) {
    volatile double l = a[(i + 1) % 3] * b[(i + 2) % 3];
    volatile double r = a[(i + 2) % 3] * b[(i + 1) % 3];
    volatile double d = l - r;
    return d;
}
static std::vector<double> posed(const std::vector<double>& U, const Skin& s, const std::vector<double>& P) {
    std::vector<double> out(U.size());
    for (size_t c = 0; c < U.size() / 3; ++c) {
        const double p[3] = {U[3 * c], U[3 * c + 1], U[3 * c + 2]};
        const double* R0 = &P[(size_t)8 * s.index[c * s.J]];
        double a[8];
        for (int j = 0; j < s.J; ++j) {
            const double* D = &P[(size_t)8 * s.index[c * s.J + j]];
            double ws = s.weight[c * s.J + j];
            if (j > 0) {
                volatile double g0 = D[0] * R0[0], g1 = D[1] * R0[1], g2 = D[2] * R0[2], g3 = D[3] * R0[3];
                volatile double g = g0 + g1;
                g = g + g2;
                g = g + g3;
                if (g < 0) ws = -ws;
            }
            for (int k = 0; k < 8; ++k) {
                volatile double q = ws * D[k];
                if (j == 0) a[k] = q;
                else { volatile double sum = a[k] + q; a[k] = sum; }
            }
        }
        volatile double s0 = a[0] * a[0], s1 = a[1] * a[1], s2 = a[2] * a[2], s3 = a[3] * a[3];
        volatile double n2 = s0 + s1;
        n2 = n2 + s2;
        n2 = n2 + s3;
        volatile double n = std::sqrt(n2);
        volatile double inv = 1.0 / n;
        double u[8];
        for (int k = 0; k < 8; ++k) { volatile double t = a[k] * inv; u[k] = t; }
        const double w = u[0], e = u[4];
        const double* v = u + 1;
        const double* f = u + 5;
        double cc[3], h[3];
        for (int i = 0; i < 3; ++i) { volatile double wp = w * p[i]; volatile double t = crossi(v, p, i) + wp; cc[i] = t; }
        for (int i = 0; i < 3; ++i) h[i] = crossi(v, cc, i);
        for (int i = 0; i < 3; ++i) {
            volatile double wf = w * f[i], ev = e * v[i];
            volatile double m = wf - ev;
            m = m + crossi(v, f, i);
            volatile double t = p[i] + 2.0 * h[i];
            t = t + 2.0 * m;
            out[3 * c + i] = t;
        }
    }
    return out;
}
// (the other kind: skin_host_check.cpp's formula)
static std::vector<double> posed_linear(const std::vector<double>& U, const Skin& s, const std::vector<double>& P) {
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
static int64_t kind_of(ft_context* c, ft_node mesh) {
    int64_t counts[4] = {-1, -1, -1, -1};
    CHECK(ft_debug_skin_dq(c, mesh, counts) == FT_OK);
    return counts[3];
}

int main() {
    const int n = 300;
    const std::vector<double> U = blob(n, 1);
    const Skin s = skin_of(n, 3, 5, 7);
    const std::vector<double> Q = dual_quaternions(5, 11), M = bones(5, 11);
    ft_context* c = nullptr;
    CHECK(ft_create_host_only(&c) == FT_OK);
    const ft_node mesh = ft_sg_bsp_mesh(c, 0, U.data(), n);
    const ft_transform up{FT_TRANSLATE, 0, {0, 3, 0}, 0};
    const ft_node xf = ft_sg_transform(c, &up, 1, mesh);
    CHECK(ft_scene_set_objects(c, ft_sg_group(c, &xf, 1)) == FT_OK);
    const double dir[3] = {0, -1, 1}, white[3] = {1, 1, 1};
    CHECK(ft_scene_add_directional(c, dir, white) == FT_OK && ft_scene_commit(c) == FT_OK && committed_is(c, U));
    // ---- refusals: nothing changes
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    int64_t counts[4];
    CHECK(ft_sg_set_mesh_bones_dq(c, mesh, Q.data(), 5) == FT_ERR_INVALID);                      // no skin
    CHECK(ft_sg_set_mesh_skin(c, mesh, s.index.data(), s.weight.data(), 3, n) == FT_OK);
    CHECK(ft_sg_set_mesh_bones_dq(nullptr, mesh, Q.data(), 5) == FT_ERR_INVALID && ft_sg_set_mesh_bones_dq(c, xf, Q.data(), 5) == FT_ERR_INVALID);
    CHECK(ft_sg_set_mesh_bones_dq(c, -1, Q.data(), 5) == FT_ERR_INVALID && ft_sg_set_mesh_bones_dq(c, 1 << 20, Q.data(), 5) == FT_ERR_INVALID);
    CHECK(ft_sg_set_mesh_bones_dq(c, mesh, nullptr, 5) == FT_ERR_INVALID && ft_sg_set_mesh_bones_dq(c, mesh, Q.data(), 4) == FT_ERR_INVALID);
    CHECK(ft_sg_set_mesh_bones_dq(c, mesh, Q.data(), -1) == FT_ERR_INVALID && ft_sg_set_mesh_bones_dq(c, mesh, Q.data(), 257) == FT_ERR_INVALID);
    for (size_t at : {(size_t)2, (size_t)17, (size_t)39}) {
        std::vector<double> bad = Q;
        for (double v : {nan, inf, -inf}) { bad[at] = v; CHECK(ft_sg_set_mesh_bones_dq(c, mesh, bad.data(), 5) == FT_ERR_INVALID); }
    }
    CHECK(ft_debug_skin_dq(c, xf, counts) == FT_ERR_INVALID && ft_debug_skin_dq(c, mesh, nullptr) == FT_ERR_INVALID && ft_debug_skin_dq(nullptr, mesh, counts) == FT_ERR_INVALID);
    CHECK(kind_of(c, mesh) == 0 && ft_scene_commit_deformed(c) == FT_OK && committed_is(c, U));
    // ---- the three commits that need the vertices
    CHECK(ft_sg_set_mesh_bones_dq(c, mesh, Q.data(), 5) == FT_OK && kind_of(c, mesh) == 2 && ft_scene_commit_deformed(c) == FT_OK && committed_is(c, posed(U, s, Q)));
    CHECK(ft_debug_skin_dq(c, mesh, counts) == FT_OK && counts[0] == 0 && counts[1] == 0 && counts[2] == 1 && counts[3] == 2);
    CHECK(ft_debug_skin(c, mesh, counts) == FT_OK && counts[0] == 0 && counts[1] == 0 && counts[2] == 0 && counts[3] == 0);
    const std::vector<double> Q2 = dual_quaternions(5, 12), Q3 = dual_quaternions(6, 13);
    CHECK(ft_sg_set_mesh_bones_dq(c, mesh, Q2.data(), 5) == FT_OK && ft_scene_commit(c) == FT_OK && committed_is(c, posed(U, s, Q2)));
    CHECK(ft_sg_set_mesh_bones_dq(c, mesh, Q3.data(), 6) == FT_OK && ft_sg_set_transform(c, xf, &up, 1) == FT_OK);
    CHECK(ft_scene_commit_deformed(c) == FT_ERR_STATE && ft_scene_commit_moved(c) == FT_OK && committed_is(c, posed(U, s, Q3)));
    // ---- the switches between the palette kinds; a refused call leaves the kind in force
    CHECK(ft_sg_set_mesh_bones(c, mesh, M.data(), 5) == FT_OK && kind_of(c, mesh) == 1 && ft_scene_commit_deformed(c) == FT_OK && committed_is(c, posed_linear(U, s, M)));
    CHECK(ft_debug_skin(c, mesh, counts) == FT_OK && counts[2] == 1 && ft_debug_skin_dq(c, mesh, counts) == FT_OK && counts[2] == 0);
    CHECK(ft_sg_set_mesh_bones_dq(c, mesh, Q.data(), 4) == FT_ERR_INVALID && kind_of(c, mesh) == 1);
    CHECK(ft_sg_set_mesh_bones_dq(c, mesh, Q.data(), 5) == FT_OK && kind_of(c, mesh) == 2 && ft_scene_commit_deformed(c) == FT_OK && committed_is(c, posed(U, s, Q)));
    CHECK(ft_sg_set_mesh_bones(c, mesh, M.data(), 4) == FT_ERR_INVALID && kind_of(c, mesh) == 2);
    CHECK(ft_sg_set_mesh_bones(c, mesh, nullptr, 0) == FT_OK && kind_of(c, mesh) == 0 && ft_scene_commit_deformed(c) == FT_OK && committed_is(c, U));
    CHECK(ft_sg_set_mesh_bones(c, mesh, M.data(), 5) == FT_OK && ft_sg_set_mesh_bones_dq(c, mesh, nullptr, 0) == FT_OK && kind_of(c, mesh) == 0);
    CHECK(ft_scene_commit(c) == FT_OK && committed_is(c, U));
    CHECK(ft_sg_set_mesh_bones_dq(c, mesh, Q3.data(), 6) == FT_OK && ft_scene_commit_deformed(c) == FT_OK && committed_is(c, posed(U, s, Q3)));
    // a new shape under the palette in force
    const std::vector<double> E = blob(n, 9);
    CHECK(ft_sg_set_mesh_triangles(c, mesh, E.data(), n) == FT_OK && ft_scene_commit_deformed(c) == FT_OK && committed_is(c, posed(E, s, Q3)));
    // morph under skin: the targets' base is the shape, the pose is skin(blend)
    std::vector<double> T = blob(n, 2, 0.5);
    { const std::vector<double> t1 = blob(n, 3, -0.25); T.insert(T.end(), t1.begin(), t1.end()); }
    const std::vector<double> w = {0.25, -0.5};
    CHECK(ft_sg_set_mesh_targets(c, mesh, T.data(), 2, n) == FT_OK && ft_scene_commit_deformed(c) == FT_OK && committed_is(c, posed(E, s, Q3)));
    CHECK(ft_sg_set_mesh_weights(c, mesh, w.data(), 2) == FT_OK && ft_scene_commit_deformed(c) == FT_OK && committed_is(c, posed(blend(E, T, w), s, Q3)));
    CHECK(ft_sg_set_mesh_bones_dq(c, mesh, Q.data(), 5) == FT_OK && ft_scene_commit(c) == FT_OK && committed_is(c, posed(blend(E, T, w), s, Q)));
    // ---- a blend whose real part is zero is refused (NaN vertices) and the next pose commits
    {
        Skin z{std::vector<int32_t>((size_t)3 * n * 2, 1), std::vector<double>((size_t)3 * n * 2), 2};
        for (size_t k = 0; k < z.weight.size(); ++k) z.weight[k] = k & 1 ? -0.5 : 0.5;
        CHECK(ft_sg_set_mesh_skin(c, mesh, z.index.data(), z.weight.data(), 2, n) == FT_OK && kind_of(c, mesh) == 0);
        CHECK(ft_sg_set_mesh_bones_dq(c, mesh, Q.data(), 5) == FT_OK && ft_scene_commit_deformed(c) == FT_ERR_UNSUPPORTED);
        CHECK(std::strstr(ft_last_error(c), "non-finite") != nullptr && committed_is(c, posed(blend(E, T, w), s, Q)));
        const std::vector<double> v = posed(U, z, Q);
        CHECK(std::isnan(v[0]) && std::isnan(v[v.size() - 1]));
        CHECK(ft_sg_set_mesh_skin(c, mesh, s.index.data(), s.weight.data(), 3, n) == FT_OK);
        CHECK(ft_sg_set_mesh_bones_dq(c, mesh, Q2.data(), 5) == FT_OK && ft_scene_commit_deformed(c) == FT_OK && committed_is(c, posed(blend(E, T, w), s, Q2)));
    }
    // removal: ft_sg_set_mesh_skin removes a dual-quaternion palette and the skin
    CHECK(ft_sg_set_mesh_skin(c, mesh, nullptr, nullptr, 0, n) == FT_OK && kind_of(c, mesh) == 0 && ft_sg_set_mesh_bones_dq(c, mesh, Q.data(), 5) == FT_ERR_INVALID);
    CHECK(ft_scene_commit_deformed(c) == FT_OK && committed_is(c, blend(E, T, w)));
    // 256 bones, four influences
    const Skin s4 = skin_of(n, 4, 256, 21);
    const std::vector<double> Q256 = dual_quaternions(256, 22);
    CHECK(ft_sg_set_mesh_skin(c, mesh, s4.index.data(), s4.weight.data(), 4, n) == FT_OK && ft_sg_set_mesh_bones_dq(c, mesh, Q256.data(), 255) == FT_ERR_INVALID);
    CHECK(ft_sg_set_mesh_bones_dq(c, mesh, Q256.data(), 256) == FT_OK && ft_scene_commit_deformed(c) == FT_OK && committed_is(c, posed(blend(E, T, w), s4, Q256)));
    CHECK(ft_scene_clear(c) == FT_OK);
    ft_destroy(c);

    // ---- fth::skin_blend_dq and the accessors directly, an odd corner count
    {
        const std::vector<double> shape = blob(7, 4);
        const Skin k = skin_of(7, 4, 256, 5);
        std::vector<uint32_t> words(21, 0u);
        for (size_t q = 0; q < 21; ++q) for (int j = 0; j < 4; ++j) words[q] |= (uint32_t)k.index[q * 4 + j] << (8 * j);
        std::vector<double> out(shape.size());
        fth::skin_blend_dq(shape.data(), words.data(), k.weight.data(), 4, Q256.data(), 21, out.data());
        const std::vector<double> want = posed(shape, k, Q256);
        CHECK(std::memcmp(out.data(), want.data(), out.size() * 8) == 0);
        for (int J = 1; J <= 3; ++J) {                               // fewer influences: the first J slots of each corner
            Skin kj{std::vector<int32_t>(21 * (size_t)J), std::vector<double>(21 * (size_t)J), J};
            for (size_t q = 0; q < 21; ++q) for (int j = 0; j < J; ++j) { kj.index[q * J + j] = k.index[q * 4 + j]; kj.weight[q * J + j] = k.weight[q * 4 + j]; }
            fth::skin_blend_dq(shape.data(), words.data(), kj.weight.data(), J, Q256.data(), 21, out.data());
            const std::vector<double> wj = posed(shape, kj, Q256);
            CHECK(std::memcmp(out.data(), wj.data(), out.size() * 8) == 0);
        }
        fth::GraphNode m; m.kind = fth::GraphNode::Mesh; m.tris = shape; m.skin_index = words; m.skin_weight = k.weight; m.skin_influences = 4; m.skin_max_index = 255;
        CHECK(&m.vertices() == &m.shape());
        m.palette = Q256; m.n_bones = 256; m.palette_kind = fth::GraphNode::DualQuaternions; m.posed_stale = true;
        CHECK(std::memcmp(m.vertices().data(), want.data(), out.size() * 8) == 0 && !m.posed_stale && m.host_skins_dq == 1 && m.host_skins == 0);
        CHECK(std::memcmp(m.shape().data(), shape.data(), out.size() * 8) == 0 && m.vertices().size() == shape.size() && m.host_skins_dq == 1);
    }
    std::printf("skin_dq_host_check: ok\n");
    return 0;
}

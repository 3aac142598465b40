// refit_cost_host_check.cpp — the host-checkable part of ft_scene_tree_quality and of the rebuild in place under
// AddressSanitizer + UBSan, as a stand-alone program (CPU only).  It compiles the arithmetic of k_refit_cost (ft_refit_cost.h: the
// per-slot term, real_node, the leaf bounds, the division by the root's area) as plain C++ and runs it over trees the host builder made,
// summed in the kernel's own shape - xor butterflies over 64 lanes, four waves per block, the partials in index order - against a direct
// walk of the tree; over a device job's reserved ranges, where no slot is a node yet; and it checks the ranges a rebuild puts back to
// zero bytes (FlatScene::reserved_spans) against a fresh flatten.
// Build and run from the repository root:
//   g++ -fsanitize=address,undefined -fno-omit-frame-pointer -g -O1 -std=c++17 -ffp-contract=off -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       tools/refit_cost_host_check.cpp functracer_amd/csrc/ft_scene.cpp -o build/refit_cost_host_check && build/refit_cost_host_check
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../functracer_amd/csrc/ft_refit_cost.h"

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); std::exit(1); } } while (0)

static std::vector<double> blob(int n, unsigned seed, double spread = 0.8) {
    std::mt19937 rng(seed);
    std::normal_distribution<double> g;
    std::vector<double> t((size_t)9 * n);
    for (int i = 0; i < n; ++i) {
        const double c[3] = {spread * g(rng), spread * g(rng), spread * g(rng)};
        for (int k = 0; k < 9; ++k) t[(size_t)9 * i + k] = c[k % 3] + 0.08 * g(rng);
    }
    return t;
}

static ftk::RefitArrays arrays_of(fth::FlatScene& f) {
    return ftk::RefitArrays{f.tris.data(), f.nodes.data(), f.bsp_leaves.data(), f.tri_orig.data(), f.wide.data(), f.coarse_boxes.data(), nullptr, nullptr, nullptr, nullptr, nullptr};
}

// k_refit_cost + k_refit_cost_sum, lane by lane.
static double cost_in_kernel_shape(const ftk::RefitArrays& A, const ftk::RefitMesh& m) {
    const uint32_t blocks = ftk::refit_cost_blocks(m);
    double sum = 0.0;
    for (uint32_t b = 0; b < blocks; ++b) {
        double wave[4];
        for (uint32_t w = 0; w < 4; ++w) {
            double lane[64], next[64];
            for (uint32_t l = 0; l < 64; ++l) lane[l] = ftk::refit::cost_term(A, m, b * 256u + w * 64u + l);
            for (int off = 32; off > 0; off >>= 1) { for (int l = 0; l < 64; ++l) next[l] = lane[l] + lane[l ^ off]; std::memcpy(lane, next, sizeof lane); }
            wave[w] = lane[0];
        }
        sum += ((wave[0] + wave[1]) + wave[2]) + wave[3];
    }
    return ftk::refit::cost_of_sum(A, m, sum);
}

// The definition, by a walk from the root: every inner node's stored box, every leaf's triangles.
static void walk(const fth::FlatScene& f, int32_t ref, double& sum, size_t& leaves, size_t& tris) {
    if (ref >= 0) {
        const ftd::BspNode& nd = f.nodes[(size_t)ref];
        sum += ftk::refit::half_area(nd.bmin, nd.bmax);
        walk(f, nd.left, sum, leaves, tris); walk(f, nd.right, sum, leaves, tris);
        return;
    }
    const ftd::BspLeaf& L = f.bsp_leaves[(size_t)~ref];
    double lo[3] = {1e308, 1e308, 1e308}, hi[3] = {-1e308, -1e308, -1e308};
    for (uint32_t k = 0; k < L.n_tris; ++k) {
        const double* T = &f.tris[9 * (size_t)(L.first_tri + k)];
        for (int v = 0; v < 3; ++v) for (int a = 0; a < 3; ++a) { const double q = T[a] + (v == 1 ? T[3 + a] : v == 2 ? T[6 + a] : 0.0); lo[a] = std::fmin(lo[a], q); hi[a] = std::fmax(hi[a], q); }
    }
    sum += (double)L.n_tris * ftk::refit::half_area(lo, hi);
    ++leaves; tris += L.n_tris;
}

static fth::SceneGraph graph_of(const std::vector<std::vector<double>>& meshes) {
    fth::SceneGraph g;
    fth::GraphNode grp; grp.kind = fth::GraphNode::Group;
    for (const auto& t : meshes) { fth::GraphNode m; m.kind = fth::GraphNode::Mesh; m.tris = t; g.nodes.push_back(m); grp.children.push_back((int32_t)g.nodes.size() - 1); }
    g.nodes.push_back(grp);
    g.root = (int32_t)g.nodes.size() - 1;
    return g;
}

int main() {
    std::vector<double> same_tri = blob(300, 9);
    for (size_t k = 9; k < same_tri.size(); ++k) same_tri[k] = same_tri[k % 9];                 // 300 copies of one triangle
    std::vector<double> flat = blob(500, 10);
    for (size_t k = 2; k < flat.size(); k += 3) flat[k] = 0.37;                                 // every vertex in the plane z = 0.37
    const std::vector<std::vector<double>> meshes = {blob(8, 1), blob(9, 2), blob(257, 3), blob(1025, 4), same_tri, flat, blob(7, 5), blob(5000, 6, 3.0)};

    // ---- the cost over host-built trees: the kernel's shape against the walk
    {
        fth::SceneGraph g = graph_of(meshes);
        fth::FlatScene f;
        std::string err;
        CHECK(g.flatten(f, err) == FT_OK && f.bvh_jobs.empty() && f.mesh_ranges.size() == f.meshes.size());
        const ftk::RefitArrays A = arrays_of(f);
        size_t measured = 0;
        for (uint32_t k = 0; k < (uint32_t)f.meshes.size(); ++k) {
            if (f.meshes[k].root >= 0 || f.meshes[k].bvh_root == INT32_MIN) { CHECK(meshes[k].size() / 9 < 8); continue; }
            const ftk::RefitMesh m = ftk::refit::refit_ranges(f, k, 0.0);
            CHECK(!m.device_built && m.n == meshes[k].size() / 9 && ftk::refit::node_in(m, m.bvh_root));
            double sum = 0.0; size_t leaves = 0, tris = 0;
            walk(f, m.bvh_root, sum, leaves, tris);
            CHECK(tris == m.n && leaves <= m.leaf_count);
            const double want = ftk::refit::cost_of_sum(A, m, sum), got = cost_in_kernel_shape(A, m);
            CHECK(std::isfinite(got) && got >= 1.0);                                            // the root's own box alone gives 1
            CHECK(std::fabs(got - want) <= 1e-12 * want);
            // a slot past the range adds nothing, and a leaf reference outside the mesh's ranges is not followed
            CHECK(ftk::refit::cost_term(A, m, m.node_count) == 0.0 && ftk::refit::cost_term(A, m, 0xFFFFFFFFu) == 0.0);
            CHECK(!ftk::refit::leaf_in(m, INT32_MIN) && !ftk::refit::leaf_in(m, ~(int32_t)(m.leaf_first + m.leaf_count)) && !ftk::refit::node_in(m, (int32_t)(m.node_first + m.node_count)));
            ++measured;
        }
        CHECK(measured == 7);
        // a root box without area, or not finite, gives 0
        const ftk::RefitMesh m = ftk::refit::refit_ranges(f, 2, 0.0);
        ftd::BspNode& root = f.nodes[(size_t)m.bvh_root];
        const ftd::BspNode keep = root;
        for (int a = 0; a < 3; ++a) root.bmax[a] = root.bmin[a];
        CHECK(cost_in_kernel_shape(A, m) == 0.0);
        root = keep; root.bmax[0] = INFINITY;
        CHECK(cost_in_kernel_shape(A, m) == 0.0);
        root = keep; root.bmax[1] = NAN;
        CHECK(cost_in_kernel_shape(A, m) == 0.0);
        root = keep;
        CHECK(cost_in_kernel_shape(A, m) >= 1.0);
    }

    // ---- a device job's ranges as the flattener reserves them: no slot is a node, the cost is 0; and the reset of a rebuild in place
    {
        fth::SceneGraph g = graph_of(meshes);
        g.device_bvh = true; g.device_bvh_min_tris = 0;
        fth::FlatScene fresh;
        std::string err;
        CHECK(g.flatten(fresh, err) == FT_OK && fresh.bvh_jobs.size() == 7);
        fth::FlatScene work = fresh;
        const ftk::RefitArrays A = arrays_of(work);
        for (const fth::FlatScene::BvhJob& j : fresh.bvh_jobs) {
            const ftk::RefitMesh m = ftk::refit::refit_ranges(work, j.mesh, 0.0);
            const fth::FlatScene::JobSpans sp = fth::FlatScene::reserved_spans(j);
            CHECK(m.device_built && m.bvh_root == (int32_t)j.node_base);
            CHECK(sp.node_first == m.node_first && sp.node_count == m.node_count && sp.leaf_first == m.leaf_first && sp.leaf_count == m.leaf_count);
            CHECK(sp.wide_first == m.wide_first && sp.wide_count == m.wide_count && j.tri_base == m.tri_first && j.n == m.tri_count);
            CHECK(sp.leaf_first == (size_t)~work.meshes[j.mesh].root + 1);                      // the list-order leaf lies in front of the range and stays
            CHECK(cost_in_kernel_shape(A, m) == 0.0);
            // what an old tree may have left anywhere in the ranges ...
            std::memset(work.nodes.data() + sp.node_first, 0xAB, sp.node_count * sizeof(ftd::BspNode));
            std::memset(work.bsp_leaves.data() + sp.leaf_first, 0xAB, sp.leaf_count * sizeof(ftd::BspLeaf));
            std::memset(work.wide.data() + ftd::kWideNodeDoubles * sp.wide_first, 0xAB, sp.wide_count * ftd::kWideNodeDoubles * 8);
            CHECK(std::memcmp(work.nodes.data(), fresh.nodes.data(), fresh.nodes.size() * sizeof(ftd::BspNode)) != 0);
            // ... is gone after the reset: zero bytes over the spans give the fresh flatten back, everywhere
            std::memset(work.nodes.data() + sp.node_first, 0, sp.node_count * sizeof(ftd::BspNode));
            std::memset(work.bsp_leaves.data() + sp.leaf_first, 0, sp.leaf_count * sizeof(ftd::BspLeaf));
            std::memset(work.wide.data() + ftd::kWideNodeDoubles * sp.wide_first, 0, sp.wide_count * ftd::kWideNodeDoubles * 8);
            CHECK(work.nodes.size() == fresh.nodes.size() && std::memcmp(work.nodes.data(), fresh.nodes.data(), fresh.nodes.size() * sizeof(ftd::BspNode)) == 0);
            CHECK(work.bsp_leaves.size() == fresh.bsp_leaves.size() && std::memcmp(work.bsp_leaves.data(), fresh.bsp_leaves.data(), fresh.bsp_leaves.size() * sizeof(ftd::BspLeaf)) == 0);
            CHECK(work.wide.size() == fresh.wide.size() && std::memcmp(work.wide.data(), fresh.wide.data(), fresh.wide.size() * 8) == 0);
        }
    }
    std::printf("refit_cost_host_check: ok\n");
    return 0;
}

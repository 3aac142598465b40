// ft_refit_cost.h — what the refit kernels (ft_refit.hip) know about one mesh's tree in the scene's arrays, and the arithmetic of
// k_refit_cost over it, written so that it also compiles as plain C++: tools/refit_cost_host_check.cpp runs it over a host-built tree
// under AddressSanitizer and UBSan.  No HIP device code beyond the function qualifiers.
#ifndef FT_REFIT_COST_H
#define FT_REFIT_COST_H
#include <math.h>
#include <stdint.h>

#include "ft_device.h"
#include "ft_scene.h"

#if defined(__HIPCC__)
#define FT_REFIT_FN __host__ __device__ __forceinline__
#else
#define FT_REFIT_FN inline
#endif

namespace ftk {
namespace refit {

constexpr uint32_t kLeafTris = 4;                                   // as the builders

// One mesh's ranges in the flattened scene, as the refit kernels take them; pad: the builders' inflation for the mesh's vertices.
inline RefitMesh refit_ranges(const fth::FlatScene& f, uint32_t mesh, double pad) {
    const ftd::Mesh& M = f.meshes[mesh];
    const fth::FlatScene::MeshRange& r = f.mesh_ranges[mesh];
    RefitMesh m{};
    m.first_global = f.bsp_leaves[(size_t)~M.root].first_tri; m.n = f.bsp_leaves[(size_t)~M.root].n_tris;
    m.node_first = r.node_first; m.node_count = r.node_count; m.leaf_first = r.leaf_first; m.leaf_count = r.leaf_count;
    m.tri_first = r.tri_first; m.tri_count = r.tri_count; m.wide_first = r.wide_first; m.wide_count = r.wide_count;
    m.bvh_root = M.bvh_root;
    for (const fth::FlatScene::BvhJob& j : f.bvh_jobs) if (j.mesh == mesh) m.device_built = 1u;
    m.coarse_first = f.mesh_coarse[2 * mesh]; m.coarse_count = f.mesh_coarse[2 * mesh + 1];
    m.pad = pad;
    return m;
}

FT_REFIT_FN bool node_in(const RefitMesh& m, int32_t r) { return r >= 0 && (uint32_t)r >= m.node_first && (uint32_t)r - m.node_first < m.node_count; }
FT_REFIT_FN bool leaf_in(const RefitMesh& m, int32_t r) { return r < 0 && r != INT32_MIN && (uint32_t)~r >= m.leaf_first && (uint32_t)~r - m.leaf_first < m.leaf_count; }
// Node r of the mesh's range is a node of its tree.  A device job wrote a record for every node of its build, and lets those of at most
// four triangles stand as leaves (ft_bvh.hip, scene_ref): build node i is also BspLeaf leaf_first + i, which holds its triangle count
// (0 where the surface-area builder made fewer nodes than the range has room for).
FT_REFIT_FN bool real_node(const RefitArrays& A, const RefitMesh& m, uint32_t r) {
    return !m.device_built || A.leaves[m.leaf_first + (r - m.node_first)].n_tris > kLeafTris;
}

// The exact bound of the vertices of leaf `l` (an index into the scene's BspLeaf array) as the hit test sees them, or false when it is no
// leaf of the tree's size.
FT_REFIT_FN bool leaf_bound(const RefitArrays& A, const RefitMesh& m, uint32_t l, double box[6], uint32_t* n_tris = nullptr) {
    const ftd::BspLeaf L = A.leaves[l];
    if (L.n_tris == 0u || L.n_tris > kLeafTris || L.first_tri < m.tri_first || L.first_tri - m.tri_first + L.n_tris > m.tri_count) return false;
    for (int a = 0; a < 3; ++a) { box[a] = __builtin_inf(); box[3 + a] = -__builtin_inf(); }
    for (uint32_t k = 0; k < L.n_tris; ++k) {
        const double* T = A.tris + 9ull * (L.first_tri + k);
        for (int a = 0; a < 3; ++a) {
            const double v0 = T[a], v1 = T[a] + T[3 + a], v2 = T[a] + T[6 + a];
            box[a] = fmin(box[a], fmin(v0, fmin(v1, v2))); box[3 + a] = fmax(box[3 + a], fmax(v0, fmax(v1, v2)));
        }
    }
    if (n_tris) *n_tris = L.n_tris;
    return true;
}

FT_REFIT_FN double half_area(const double* lo, const double* hi) { const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2]; return dx * dy + dy * dz + dz * dx; }

// What node slot i of the mesh's range adds to the cost: nothing unless it is a real node; then the area of its stored
// box and, for each child that is a leaf, that leaf's triangle count times the area of the exact bound of its sorted records.  Every
// leaf has one parent, so every leaf is counted once.
FT_REFIT_FN double cost_term(const RefitArrays& A, const RefitMesh& m, uint32_t i) {
    if (i >= m.node_count || !real_node(A, m, m.node_first + i)) return 0.0;
    const ftd::BspNode* nd = A.nodes + (m.node_first + i);
    double term = half_area(nd->bmin, nd->bmax);
    const int32_t ch[2] = {nd->left, nd->right};
    for (int c = 0; c < 2; ++c) {
        double box[6]; uint32_t n_tris = 0;
        if (leaf_in(m, ch[c]) && leaf_bound(A, m, (uint32_t)~ch[c], box, &n_tris)) term += (double)n_tris * half_area(box, box + 3);
    }
    return term;
}
// The sum of the terms over the area of the root's stored box; 0 when that area is 0 or not finite (such a tree never asks for a rebuild).
FT_REFIT_FN double cost_of_sum(const RefitArrays& A, const RefitMesh& m, double sum) {
    double root = 0.0;
    if (node_in(m, m.bvh_root)) root = half_area(A.nodes[m.bvh_root].bmin, A.nodes[m.bvh_root].bmax);
    return root > 0.0 && root < __builtin_inf() ? sum / root : 0.0;
}

} // namespace refit
} // namespace ftk
#endif

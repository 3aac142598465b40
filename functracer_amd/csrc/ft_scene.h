// ft_scene.h — host-side scene graph arena (mirror of Scene.fs:8-53, 107-110) and its
// compilation to the flat HBM layout of ft_flat.h.  Pure C++; no HIP here.
#ifndef FT_SCENE_H
#define FT_SCENE_H
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/functracer_hip.h"
#include "ft_flat.h"

namespace fth {

struct GraphNode {
    enum Kind { Prim, TriangleP, Mesh, Transform, MaterialF, HueShift, IgnoreLight, Texture, Group, Csg } kind = Prim;
    int32_t prim = 0;                 // ft_primitive_kind
    double tri[9] = {0};              // TriangleP
    int32_t depth = 0;                // Mesh: BspMesh.bspMesh depth
    // Mesh: n x 9 (a,b,c).  Stale (the right size, old contents) while `tris_stale`: every reader of a mesh's vertices asks vertices().
    mutable std::vector<double> tris;
    bool deformed = false;            // Mesh: the vertices were replaced (ft_sg_set_mesh_triangles / ft_sg_set_mesh_weights) since the last successful commit
    // Mesh: morph targets (ft_sg_set_mesh_targets).  base: B, n x 9; deltas: K x n x 9, D_k = T_k - B; weights: K once
    // ft_sg_set_mesh_weights was called; targets_serial: another value after every ft_sg_set_mesh_targets (what a device holds of base
    // and deltas is that call's).  by_weights: the vertices are blend(B, D, w) and not what ft_sg_set_mesh_triangles gave.
    std::vector<double> base, deltas, weights;
    int32_t n_targets = 0;
    uint64_t targets_serial = 0;
    bool by_weights = false;
    mutable bool tris_stale = false;  // by_weights and `tris` has not been blended from the weights as they stand
    mutable uint64_t host_blends = 0; // times vertices() has blended them on the host (ft_debug_morph counts[2])
    // Mesh: skinning (ft_sg_set_mesh_skin / ft_sg_set_mesh_bones).  skin_index: per corner (3 x triangle + corner) one word
    // of four bone indices, slot j in byte j, unused slots 0 - as the device reads them; skin_weight: per corner J weights, corner-major as
    // given; palette: n_bones x 12, the rows of a 3x4 matrix per bone (n_bones 0: no palette in force).  skin_serial: another value after
    // every ft_sg_set_mesh_skin, shape_serial: after every call that makes the shape explicit vertices of other contents
    // (ft_sg_set_mesh_triangles, ft_sg_set_mesh_targets) - what a device holds of indices and weights / of the rest shape is that call's.
    std::vector<uint32_t> skin_index;
    std::vector<double> skin_weight, palette;
    int32_t skin_influences = 0, skin_max_index = 0, n_bones = 0;
    // palette_kind: what `palette` holds while n_bones > 0 - Matrices as above, or DualQuaternions (ft_sg_set_mesh_bones_dq):
    // n_bones x 8, real part (w, x, y, z) then dual part per bone.  A node holds at most one palette.
    enum PaletteKind : int32_t { NoPalette = 0, Matrices = 1, DualQuaternions = 2 };
    int32_t palette_kind = NoPalette;
    uint64_t skin_serial = 0, shape_serial = 0;
    mutable std::vector<double> posed;   // skin(shape(), palette) while a palette is in force and not `posed_stale`
    mutable bool posed_stale = false;
    mutable uint64_t host_skins = 0;  // times vertices() has skinned them on the host (ft_debug_skin counts[2])
    mutable uint64_t host_skins_dq = 0;   // the same for a dual-quaternion palette (ft_debug_skin_dq counts[2])
    // The shape U as it stands: `tris`, blended first where the weights describe them (morph_blend's arithmetic).
    const std::vector<double>& shape() const;
    // The vertices V as they stand: the shape, skinned first where a palette is in force (skin_blend's / skin_blend_dq's arithmetic).
    const std::vector<double>& vertices() const;
    std::vector<ft_transform> xf;     // Transform: one basic transform or a Composed list
    ft_material mat{};                // MaterialF
    int32_t op = 0;                   // Csg
    std::vector<int32_t> children;
    double ca[3] = {0}, cb[3] = {0};  // Texture grid colours
    std::vector<double> uv_ops;
    std::vector<uint8_t> pixels;      // Texture image: Rgb24 rows (empty = grid)
    int32_t img_w = 0, img_h = 0;
};

struct FlatScene {
    std::vector<ftd::Leaf> leaves;
    std::vector<double> m2w;          // 12 per leaf
    std::vector<ftd::Material> materials;
    std::vector<ftd::Light> lights;
    std::vector<ftd::Texture> textures;
    std::vector<uint8_t> tex_pixels;  // Rgb24 rows of all image textures, back to back
    std::vector<uint32_t> program;
    std::vector<ftd::Mesh> meshes;
    std::vector<ftd::BspNode> nodes;
    std::vector<ftd::BspLeaf> bsp_leaves;
    std::vector<double> tris;         // 9 per triangle: v0, e1, e2
    std::vector<uint32_t> tri_orig;   // 1 per triangle (see ft_flat.h)
    std::vector<uint32_t> tri_src;    // 1 per triangle: the index of its face in the list the mesh was built from (ft_flat.h)
    std::vector<int32_t> run_nodes;   // the builder nodes of runs of bare triangles, one per triangle (Leaf::pad[1], ft_flat.h)
    std::vector<double> wide;         // 28 doubles per 4-wide BVH node (ft_flat.h), walked by coherent wavefronts
    std::vector<int32_t> mesh_wide;   // per mesh: root of its 4-wide BVH, or INT32_MIN
    std::vector<float> coarse_boxes;  // 6 floats per box (lo, hi; model space, rounded outward): <= 64 boxes per mesh that cover all its triangles
    std::vector<uint32_t> mesh_coarse;// per mesh: first box, box count (0 = none) - k_classify tests pixel blocks against them
    std::vector<ftd::CullRecord> culls;
    std::vector<uint32_t> item_pc;    // program counter of every top-level item, in order, + one sentinel (the OP_END word)
    std::vector<float> cull_items;    // 8 floats per top-level item: centre, radius (rounded up; +inf = unbounded), row mask (bits), pad - the wave-level pre-test
    std::vector<double> cull_rows;    // 3 per distinct parallel-sensitive direction of the whole scene (<= 32, else the pre-test is off)
    bool unbounded = false;           // some top-level item has no bounds (a plane): every pixel block can see something, k_classify has nothing to do
    bool cull_bundle = true;          // false: more than 32 distinct directions
    std::vector<double> mesh_bounds;  // 6 per mesh: model-space AABB of the source triangles (lo > hi when empty)
    int32_t csg_capacity = 0;         // per-lane hit-list entries needed (0 = scene has no CSG)
    int32_t stack_capacity = 0;       // per-lane BSP / BVH stack entries needed (0 = no trees)
    int32_t bsp_stack_capacity = 0;   // the part of it the reference-shaped BSP trees need
    int64_t bvh_nodes = 0, bvh_leaves = 0, bvh_tris = 0;   // device-side BVH additions (not part of BspMesh.compile)
    bool any_reflective = false;
    bool any_texture = false;
    bool mesh_under_csg = false;
    // Light-space shadow trees (ft_flat.h, kLsPairDoubles): pair records, nodes and the triangle records they point at.
    std::vector<double> ls_pairs;
    std::vector<uint32_t> ls_nodes;
    std::vector<double> ls_tris;
    // Per record the builders appended to ls_tris, the record of `tris` it is a bitwise copy of.  Host only: no commit uploads it; the first
    // ft_scene_commit_deformed under "deform_light_space" uploads the trees' part (ft_lightspace.hip, k_ls_gather).
    std::vector<uint32_t> ls_src;
    // Meshes whose exact BVH is built on the device after the upload (ft_bvh.hip): the flattener only reserves their ranges.
    struct BvhJob { uint32_t mesh, first_global, n, node_base, leaf_base, tri_base, wide_base, coarse_first, coarse_count; };
    std::vector<BvhJob> bvh_jobs;
    // What build_bsp reserved for a job as zero bytes and the device builder may leave partly untouched: [first, first + count) records of
    // nodes, bsp_leaves and 4-wide nodes.  A rebuild in place (ft_scene_commit_deformed) puts them back to zero bytes first.
    struct JobSpans { size_t node_first, node_count, leaf_first, leaf_count, wide_first, wide_count; };
    static JobSpans reserved_spans(const BvhJob& j) { return JobSpans{j.node_base, (size_t)j.n - 1, j.leaf_base, 2 * (size_t)j.n - 1, j.wide_base, (size_t)j.n - 1}; }
    // What a refit (ft_scene_commit_deformed, ft_refit.hip) needs to find a mesh again: per mesh the builder node it was made from (-1: a
    // bare triangle or a run of them) and the ranges its BVH occupies in nodes / bsp_leaves / tris (the sorted copies) / wide - all counts
    // 0 for a mesh without one; per 4-wide node the binary node it is two levels of (device-built ranges: node_base + its offset).
    struct MeshRange { uint32_t node_first, node_count, leaf_first, leaf_count, tri_first, tri_count, wide_first, wide_count; };
    std::vector<int32_t> mesh_node;
    std::vector<MeshRange> mesh_ranges;
    std::vector<int32_t> wide_node;
};

// One pass over the vertices of a mesh (n x 9 doubles): the bounds as the flattener keeps them (mesh_bounds), the largest |coordinate| of
// the vertices as the hit test sees them (v0, v0 + e1, v0 + e2: what the BVH builders inflate their boxes by) and whether every
// coordinate passes the builders' own test, |v| < 1e300.
struct MeshScan { double bounds[6]; double extent; bool finite; };
MeshScan scan_mesh(const double* tris_abc, int64_t n_tris);
// Morph targets: out[i] = blend(base, deltas, w)[i], i < count - acc = base[i]; for k = 0 .. K-1 in order: p = w[k] * deltas[k * count + i],
// acc = acc + p; every term evaluated, product and sum each rounded once (this unit is built with -ffp-contract=off).
void morph_blend(const double* base, const double* deltas, const double* w, int32_t n_targets, size_t count, double* out);
// Skinning: out = skin(shape, palette) over `corners` corners of three doubles.  Per corner (x, y, z), for j = 0 .. J-1 in order with
// b = byte j of index[corner], M = palette + 12 * b, wj = weight[corner * J + j]: t_i = ((M[4i] * x + M[4i+1] * y) + M[4i+2] * z) + M[4i+3],
// q_i = wj * t_i, acc_i = j == 0 ? q_i : acc_i + q_i; every influence evaluated, every product and sum rounded once (-ffp-contract=off).
// out may not alias shape.
void skin_blend(const double* shape, const uint32_t* index, const double* weight, int32_t influences, const double* palette, size_t corners, double* out);
// Dual-quaternion skinning: the same arguments, palette = n_bones x 8 (real part w, x, y, z, then the dual part).  Per corner p, with R0 the
// real part of slot 0's bone: for j in order D = palette + 8 * b, g = ((D0*R0_0 + D1*R0_1) + D2*R0_2) + D3*R0_3 (j > 0), ws = g < 0 ? -wj : wj
// (slot 0: wj), a_k = j == 0 ? ws * D_k : a_k + ws * D_k; n = sqrt(((a0*a0 + a1*a1) + a2*a2) + a3*a3), s = 1 / n, u = a * s; with w = u0,
// v = u1..3, e = u4, f = u5..7: c = cross(v, p) + w*p, h = cross(v, c), m = (w*f - e*v) + cross(v, f), V = (p + 2h) + 2m - the header's
// formula ("dual-quaternion skinning"), every product, sum, difference, square root and division rounded once (-ffp-contract=off).
void skin_blend_dq(const double* shape, const uint32_t* index, const double* weight, int32_t influences, const double* palette, size_t corners, double* out);

struct SceneGraph {
    std::vector<GraphNode> nodes;
    int32_t root = -1;
    std::vector<ftd::Light> lights;
    int32_t csg_mesh_capacity = 32;
    // Non-default fast mode: ignore the `depth` of bspMesh and trace every mesh through the device-side BVH over
    // its ORIGINAL triangles.  The reference clips triangles at BSP planes; unclipped triangles give the same surface but the
    // hit arithmetic differs in the last bits, so pixels may differ at the 1e-12 level (and on silhouette ties).
    bool mesh_unclipped_bvh = false;
    // Who builds the exact BVH of top-level-Leaf meshes: true = the device (linear BVH, ft_bvh.hip; device contexts' default),
    // false = the host's recursive surface-area sweep (host-only contexts, and the fallback when a device build is refused).
    bool device_bvh = false;
    int64_t device_bvh_min_tris = 0;   // with device_bvh: meshes with fewer triangles than this get the host's SAH tree (better tree, slower build)
    // Directional shadow rays of coherent waves: 2 = a grid in the light's frame, with the tree below as the fallback of wide waves; 1 = a
    // tree built in the light's frame (ft_flat.h, kLsPairDoubles); 0 = the BVH of every ray.
    int32_t light_space_shadows = 2;

    bool valid(int32_t id) const { return id >= 0 && id < (int32_t)nodes.size(); }
    // Returns FT_OK or a negative ft_status with err set.
    int32_t flatten(FlatScene& out, std::string& err) const;
    // The cull records of a graph that differs from the one `held` was flattened from in mesh vertices only (ft_scene_commit_deformed):
    // the flattener's walk again, with held's meshes taken as they are and `bounds` (6 per mesh of held) as their bounds.  On FT_OK
    // held.mesh_bounds, culls and cull_items are the fresh flatten's; FT_ERR_UNSUPPORTED, with held untouched, when the new bounds change
    // anything else (an item that gains or loses its bounds).
    int32_t reflatten_deformed(FlatScene& held, const std::vector<double>& bounds, std::string& err) const;
    // The poses of a graph that differs from the one `held` was flattened from in transform lists only (ft_scene_commit_moved under
    // "moved_in_place"): the flattener's walk again, with held's meshes and bounds taken as they are.  On FT_OK every leaf's w2m and flags,
    // m2w, culls, cull_items and cull_rows of held are the fresh flatten's; Leaf::ls_pairs, every mesh array and every ls_* array stay -
    // the caller brings the pair records up to the new poses.  FT_ERR_UNSUPPORTED, with held untouched, when anything else differs: an
    // item that crosses six face directions (its OP_CULL pair appears in or leaves the program), an item that gains or loses its bounds,
    // a face-direction table of another length.
    int32_t reflatten_moved(FlatScene& held, std::string& err) const;
};

// BspMesh.compile (BspMesh.fs:51-65) on the host: appends nodes / leaves / clipped triangles to
// the flat arrays and returns the root reference (>= 0 branch node, < 0 ~leaf) via mesh.
int32_t build_bsp(const double* tris_abc, int64_t n_tris, int32_t depth, FlatScene& out, ftd::Mesh& mesh, std::string& err, bool device_bvh = false);

// The light-space shadow trees of every (top-level-Leaf mesh leaf with a BVH, directional light) pair of a flattened scene (ft_flat.h),
// and with `grids` each pair's grid as well.
void build_light_space(FlatScene& out, bool grids);
// What build_light_space derives from a leaf's w2m and a light's direction alone, for ft_scene_commit_lights to derive again.
struct LsPairFrame { double U[3], V[3], D[3], k_rel; };
bool ls_pair_frame(const ftd::Leaf& L, const ftd::Light& light, LsPairFrame& out);
// R of a pair as build_light_space sums it - the largest L1 distance of a vertex from c, (T[q] - c[q]) + e - over n triangles given as
// records (v0, e1, e2) or, `vertices`, as corners (a, b, c), of which the records are formed as the flattener forms them.
double ls_pair_extent(const double* tris, size_t n, bool vertices, const double c[3]);

// Triangle.slice (Triangle.fs:24-41) exposed for the known-answer tests of the product's own builder.
int32_t slice_triangle(const double p0[3], const double n[3], const double tri[9],
                       std::vector<double>& above, std::vector<double>& below, std::string& err);

} // namespace fth
#endif

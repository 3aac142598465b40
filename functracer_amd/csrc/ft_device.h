// ft_device.h — device-side buffer descriptors and the host-callable launch interface of
// ft_kernels.hip.  Included by the C-ABI layer (ft_context.h); contains no HIP device code.
#ifndef FT_DEVICE_H
#define FT_DEVICE_H
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "ft_flat.h"

namespace ftk {

constexpr int kBlock = 256;        // 4 wavefronts of 64; waves never synchronise with each other
constexpr int kMaxBounce = 16;     // recursion limits above this are rejected by ft_render
constexpr int kWorkGroups = 64;    // independent work cursors per launch

struct DevScene {
    const double* leaves;          // n_leaves x 16 doubles (ftd::Leaf)
    const double* m2w;             // n_leaves x 12
    const ftd::Material* materials;
    const ftd::Light* lights;
    const ftd::Texture* textures;
    const uint32_t* program;
    const ftd::Mesh* meshes;
    const ftd::BspNode* nodes;
    const ftd::BspLeaf* bsp_leaves;
    const double* tris;            // 9 per triangle: v0, e1, e2
    const double* culls;           // 24 doubles per ftd::CullRecord
    const uint32_t* tri_orig;      // 1 per triangle
    const double* wide;            // 28 doubles per 4-wide BVH node (ft_flat.h)
    const int32_t* mesh_wide;      // per mesh: root of its 4-wide BVH or INT32_MIN
    const double* ls_pairs;        // light-space shadow trees (ft_flat.h, kLsPairDoubles): pair records,
    const uint32_t* ls_nodes;      //   their nodes
    const double* ls_tris;         //   and the triangle records their leaves point at
    const uint8_t* tex_pixels;     // Rgb24 rows of the image textures (ftd::Texture::pixel_base indexes into it)
    const float* cull_items;       // 8 floats per top-level item (centre, radius, row mask; bare meshes: + first coarse box, count, leaf)
    const float* coarse_boxes;     // 6 floats per box: model-space boxes that cover a mesh (k_classify)
    const uint32_t* item_pc;       // n_items + 1 program counters: where each top-level item starts (last: the OP_END word)
    const double* cull_rows;       // 3 per distinct parallel-sensitive direction
    const float* ls_edges;         // option "edge_cull": kEdgeFloats floats per record of ls_tris, the edge records of the shadow grids' entries (ft_edges.h,
                                   // k_ls_edges; zeros for every other record), or null: the option is 0, or the scene has no grid
    int32_t n_leaves, n_lights, csg_cap, stack_cap;
    int32_t shadow_rays_per_hit;   // sum over lights of the shadow rays the reference casts per hit
    int32_t n_items, n_cull_rows;  // n_cull_rows < 0: pre-test disabled
    int32_t csg_rows, lane_fold;   // LDS rows per hit-list column and lanes folded together (see HitList): csg_cap <= csg_rows * lane_fold
    int32_t n_simd;                // SIMDs of the device (CUs x 4): how far few rays are spread (batch_lanes_for)
    int32_t coherent_waves;        // 1 (default): bounce-0 wavefronts use the bundle paths (cone cull, packet traversal); 0: every wave is treated as incoherent (diagnostic)   // sum over lights of the shadow rays the reference casts per hit
    int32_t uniform_surface;       // 1 (default): a k_primary batch whose hit lanes share one leaf reads that leaf and its material through scalar loads, the shaders
                                   // skip what no lane of the wave can use, a batch with an empty candidate list stores Colour.Zero unseen; 0: per lane, everything (A/B)
};

// Ray wavefront buffer, struct-of-arrays so a wave's 64 records are 512 contiguous bytes per field: 7 doubles + the sample slot =
// 60 bytes per reflection ray (roofline).  Hits never become records: a level's closest hits are shaded in the same kernel.
struct RayBuf { double *ox, *oy, *oz, *dx, *dy, *dz, *w; uint32_t* slot; };
constexpr uint64_t kRayRecBytes = 60;
// Bytes a launch has to move per unit, by construction of the pipeline (roofline): a primary ray costs a 4-byte pixel id
// read and its sample's 24-byte colour stored (it is generated, never stored); a reflection ray a 60-byte record written once and read
// once; a hit of a later bounce a 48-byte read-modify-write of its sample's colour; a pixel 24 B (4 B as RGBA8) out.
constexpr uint64_t kPixelIdBytes = 4, kAccBytes = 24;

// Length of the frame's active pixel list (k_classify), in device memory: the later stages size themselves from it.
struct PixCount { uint32_t n_pix, pad[3]; };
// Per-chunk device counters (zeroed before every chunk).
struct ChunkCounters {
    uint32_t n_rays[kMaxBounce + 2];   // rays queued for bounce k
    uint32_t pad[14];
    // Work cursors: kWorkGroups independent counters per bounce, one 64-byte line each (see ft_kernels.hip).
    uint32_t work_trace[kMaxBounce + 2][kWorkGroups * 16];
};
// Per-render device statistics.  Every wave adds what it counted to one of kStatStripes copies (its wave index mod 64), one
// no-return atomic per non-zero counter at the end of a launch; the host sums the stripes when it retires the frame.
struct RenderCounters {
    unsigned long long rays_shadow, rays_reflect, hits_primary, csg_overflow;
    double ref_equiv;
    unsigned long long hits_total;      // hits shaded over all bounces
    unsigned long long unused[3];
    unsigned long long pixels_culled;                   // k_classify: pixels whose every primary ray provably misses everything
    unsigned long long rays_shadow_primary, rays_reflect_primary;   // the k_primary share of rays_shadow / rays_reflect
    unsigned long long pad[4];                          // 128 bytes: one stripe per pair of cache lines
};
constexpr int kStatStripes = 64;
// Everything a frame's kernels count in, in one allocation so that ONE fill clears it: the chunk counters (cleared again before
// every further chunk), the statistic stripes and k_classify's ticket / error words.
struct FrameCounters {
    ChunkCounters cc;
    RenderCounters stats[kStatStripes];
    uint32_t classify_ticket;      // k_classify: waves take their 64-block segment in ticket order, so a wave's predecessors are always running
    uint32_t classify_error;       // set when a bounded wait ran out (never observed; the host then fails the frame instead of hanging)
    uint32_t report_ticket;        // k_resolve / k_report: ticket stripes that are complete (the workgroup that completes the last one writes the frame's report)
    uint32_t list_cursor;          // k_block_lists: entries of the slot's list pool handed out so far
    uint32_t report_stripe[64];    // workgroups of stripe blockIdx % 64 that have finished (8000 tickets on one word took 80 us)
};
// A frame slot's counters as they lie in HBM.  `kept`, the length of the active pixel list in the slot's classification buffers, is
// outside what the hand-over and the host's fills clear: only k_classify writes it, so that a later frame of the same view can read the
// buffers and their length as they are ("classify_reuse").
struct SlotCounters { FrameCounters fc; PixCount kept; };
// What the host reads of a frame's counters, in pinned host memory.  The last workgroup of the frame's last k_resolve writes it and
// then clears the FrameCounters for the next frame: a steady stream of frames needs no fill and no device-to-host copy in between
// (three dispatches less per frame, ~20 us of a 0.4 ms frame with the gaps around them).
struct FrameReport {               // 256 bytes: one wavefront writes it with one store instruction (word by word over PCIe a report of
    RenderCounters total;          // all 64 stripes took 200 us); the stripes summed in stripe order
    uint32_t n_rays[kMaxBounce + 2];   // the last chunk's rays per bounce
    uint32_t n_pix_active;         // the length of the frame's active list (SlotCounters::kept); 0 for a frame that was not classified
    uint32_t classify_error;
    uint32_t pad[12];
};
static_assert(sizeof(FrameReport) == 256, "FrameReport is written as 64 words");

struct Camera {                    // ImagePlane (Image.fs:55-63), computed on the host
    double o[3], k[3], i[3], j[3];
    double pw, ph, tlx, tly;
    double focal_length, tan_half_aperture;   // Image.Focus (Image.fs:9), tan (apetureAngularSize / 2) from the host
    int32_t res_h, res_v;
    int32_t has_focus, pad;
};

struct Launch {
    hipStream_t stream;
    int grid;                      // persistent grid size (workgroups)
    size_t lds_bytes;
    int variant;                   // kernel variant: bit 0 = Oren-Nayar / textures, bit 1 = soft lights, bit 2 = meshes compiled in
};

// Everything bounce 0 needs to regenerate a primary ray from its sample index i = s*n_pix + pixel.
struct Primary {
    Camera cam;
    const uint32_t* pixel_ids;     // pixel id (y*res_h + x) of list entry pix_base + pixel
    const double* jitter;          // spp x 2, the ONE pattern shared by every pixel (Image.fs:105)
    uint32_t pix_base, n_pix;
    int32_t spp;
    uint32_t stride;               // ids are y*stride + x: res_h for pixels, res_h + 1 for the corner grid of `samples corner`
    unsigned long long seed;       // keys the counter-based streams of soft shadows / depth of field
    double inv_n_pix, inv_stride;  // 1.0 / n_pix, 1.0 / stride (division-free index arithmetic, see div_by)
    const PixCount* counts;        // non-null: the chunk's list is the FRAME's active pixel list (k_classify), counts->n_pix its length, and this
                                   // chunk works on the window [pix_base, pix_base + n_pix) of it
    const uint32_t* block_map;     // with counts: block b of the active list is block block_map[b] of pixel_ids; null: pixel_ids is the list itself
    int32_t group_log2;            // samples are numbered in groups of 2^this per 64-pixel block (slot_at, ft_kernels.hip); 0: sample plane by sample plane
    // The frame's per-block triangle candidate lists (k_block_lists), or null: one header per block of the ACTIVE list and the pool
    // their entries lie in; list_leaf is the bare mesh leaf they are for.
    const uint32_t* list_heads; const uint32_t* list_pool; int32_t list_leaf;
    const float* list_edges;       // option "edge_cull": kEdgeFloats floats per entry of list_pool (BlockLists::edges), or null
};
// Bounce 0 fused (k_primary): generate the primary rays of the chunk, closest hit, shadow queries, shaders, reflection spawn, and
// one colour per sample stored into acc (Colour.Zero for a miss).
void launch_primary(const Launch& L, const DevScene& S, const Primary& gen, RayBuf next, double* acc, uint32_t acc_stride, int max_depth, FrameCounters* fc);
int occupancy_blocks_primary(size_t lds_bytes, int* variant);   // may add bit 3 to *variant: the lean kernel built for five workgroups per CU
// Launch::variant bit 4, for launch_primary alone: k_primary_mesh, the kernel of a scene that is one bare mesh under directional lights
// (ft_kernels.hip; the caller has checked scene and frame, sets lds_bytes = 0 and sizes the grid by occupancy_blocks_primary_mesh).
constexpr int kVariantMeshKernel = 16;
int occupancy_blocks_primary_mesh();
// One level of the reflection tree (bounce k >= 1) fused (k_bounce): closest hit, shadow queries, shaders and accumulation for every
// ray of rays (n = fc->cc.n_rays[bounce]); the level's reflection rays are compacted into `next`, or, with `follow`, followed to their
// end inside the launch (the last level the host launches).  A launch that finds no rays returns at once.
void launch_bounce(const Launch& L, const DevScene& S, const Primary& gen, RayBuf rays, RayBuf next, double* acc, uint32_t acc_stride, int bounce, int max_depth, bool follow, FrameCounters* fc);
int occupancy_blocks_bounce(size_t lds_bytes, int variant);
// Pixel-block classification + compaction in one kernel.  One LANE per 64-pixel block (an 8x8 tile of the pixel list): the block's
// ray bundle - all samples of its pixels - is bounded by a cone through its outermost jittered corners and tested against every
// top-level item (bare meshes also against their coarse boxes).  Blocks nothing can be hit from get block_pos = -1 (k_resolve writes
// their pixels as Colour.Zero; none of their rays is ever generated); the others are appended, in block order, to the frame's active
// pixel list (pos_block: the block of the pixel list behind each block of the active list), whose length lands in out.kept.  `epoch` tags this frame's entries of wave_counts.
// Progressive passes (ft_progressive_pass) also hand over their blocks' words (ProgressiveArgs::blk_in): a retired block is neither listed nor
// finished but gets block_pos = kBlockRetired; with `mask_only` the cone and box tests are skipped and every block that has not retired is listed.
struct ClassifyOut { int32_t* block_pos; uint32_t* pos_block; uint32_t* wave_counts; PixCount* kept; };
constexpr int32_t kBlockRetired = -2;
void launch_classify(const Launch& L, const DevScene& S, const Primary& gen_list, const ClassifyOut& out, double jitter_extent, uint32_t epoch, FrameCounters* fc,
                     const uint32_t* retired = nullptr, bool mask_only = false);
// Per-block triangle candidate lists for the primaries of a classified frame (k_block_lists, queued behind its k_classify): one wave
// per active block walks the 4-wide tree of the bare mesh leaf `leaf` with the block's pyramid and keeps the triangles whose rectangle on
// the image plane overlaps the block's.  heads[b], for block b of the active list: kListNone (more than kListCap triangles, the pool
// is full, or the pyramid is degenerate: the block's rays walk the tree) or first entry << 7 | count.  An entry is kListEntryWords
// words: the triangle's record in DevScene::tris, its list index (tri_orig), and the rectangle x0, x1, y0, y1 as floats, rounded outward,
// in the (jx, jy) coordinates of the primary rays.  fc->list_cursor hands out the pool; `counts`: the length of the active list (ClassifyOut::kept).
// edges: a second pool under the same entry index, kEdgeFloats floats per entry, the entry's edge record (ft_edges.h), or null.
constexpr uint32_t kListNone = 0xFFFFFFFFu, kListCap = 64, kListEntryWords = 6, kEdgeFloats = 9;
struct BlockLists { uint32_t* heads; uint32_t* pool; uint32_t pool_entries; int32_t leaf; float* edges; };
void launch_block_lists(const Launch& L, const DevScene& S, const Primary& gen_list, const uint32_t* pos_block, const BlockLists& out, double jitter_extent, FrameCounters* fc, const PixCount* counts);
// The frame's pixels: mean over the spp samples of each pixel of the chunk's window, in sample order (Image.fs:112-116), written as
// FP64 RGB (out_rgb) and / or as Image.write's RGBA8 bytes (out_rgba, Image.fs:36); with `zero_culled` also Colour.Zero for every
// pixel of the blocks k_classify finished.  Pixel p of the list goes to out index pixel_ids[p] (whole frame) or p (tiles, packed).
struct ResolveArgs {
    const double* acc; uint32_t acc_stride; const PixCount* counts; uint32_t first, n_pix_host; int32_t spp;
    const uint32_t* pos_block;     // classified frames: block of the ORIGINAL pixel list behind block b of the active list; else null (identity)
    const int32_t* block_pos;      // non-null: this launch also clears the culled blocks (block_pos[b] < 0) of the n_blocks_total blocks
    uint32_t n_blocks_total;
    const uint32_t* pixel_ids;     // the original pixel list (whole frame: out index = pixel id); null: out index = list position
    double* out_rgb; uint8_t* out_rgba;
    uint32_t group_log2;           // the chunk's slot numbering (Primary::group_log2)
    FrameCounters* fc; FrameReport* report;   // report non-null: the frame's last launch (see FrameReport; fc is cleared behind it)
};
void launch_resolve(const Launch& L, const ResolveArgs& a);   // L.grid: at most this many workgroups (occupancy_blocks_resolve() per CU: one resident round)
int occupancy_blocks_resolve();
// The running state of a progressive accumulation, by POSITION in the frame's pixel list (fixed for the accumulation): per pixel the sums of
// its samples so far (3 planes of n_list doubles) and, adaptive only, of their squares; per 64-entry block of the list one word: samples so
// far (bits 0-30) and kRetired.  A pass reads the `in` side and writes every entry of the `out` side (the host swaps them after a pass
// that did not overflow).
struct ProgressiveArgs {
    const double* sum_in; double* sum_out;
    const double* sq_in; double* sq_out;       // null: plain accumulation, nothing retires
    const uint32_t* blk_in; uint32_t* blk_out;
    uint32_t n_list, min_samples;
    double tolerance;                          // a block retires when its largest standard error of the mean is <= this
};
constexpr uint32_t kRetired = 0x80000000u;
// k_resolve of a progressive pass: each pixel's sum goes on from its running sum (same additions in the same order as one k_resolve
// over the concatenated pattern), mean = S / n out, S / Q / n back, retirement per block; finished blocks add spp zero samples.
void launch_resolve_progressive(const Launch& L, const ResolveArgs& a, const ProgressiveArgs& pa);
void launch_report(const Launch& L, FrameCounters* fc, FrameReport* report);   // the same hand-over as a launch of its own (frames that end in another kernel: none of them is classified)
// CornerSampling.blendPixels (Image.fs:134-144) for a w x h rect whose (w+1) x (h+1) corner colours are in acc (one sample each).
void launch_resolve_corner(const Launch& L, const double* acc, uint32_t acc_stride, uint32_t w, uint32_t h, const uint32_t* out_index, double* out_rgb, uint8_t* out_rgba);
// Device-side BVH build (ft_bvh.hip): a linear BVH over triangles [first_global, first_global + n) of `tris`, written into the ranges
// the flattener reserved for the mesh: n - 1 BspNodes at node_base, (n - 1) + n BspLeafs at leaf_base, n sorted triangle records and
// list indices at tri_base, n - 1 4-wide nodes at wide_base, coarse_count (<= 64) float boxes at coarse.  *height = height of the
// binary tree in nodes, 0 when the mesh holds a non-finite coordinate (nothing usable was written).
struct LbvhTarget {
    double* tris; uint32_t first_global, n;
    ftd::BspNode* nodes; uint32_t node_base;
    ftd::BspLeaf* leaves; uint32_t leaf_base;
    uint32_t* tri_orig; uint32_t tri_base;
    double* wide; uint32_t wide_base;
    float* coarse; uint32_t coarse_count;
    uint32_t* tri_src;                 // per triangle record: its input face (ft_flat.h); the sorted copies take their leaf record's
};
hipError_t build_lbvh(hipStream_t stream, const LbvhTarget& t, uint32_t* height, int kind = 1);   // kind 0: linear BVH, 1: binned surface-area tree over the Morton order

// Refit of a mesh whose vertices changed (ft_refit.hip, ft_scene_commit_deformed): the topology every builder left in the scene's arrays
// stays, the triangle records and every box over them are written again.  RefitArrays: the scene's arrays in HBM and the refit's own
// tables, all indexed as the scene's - parent_node / arrived per BspNode, parent_leaf / leaf_boxes (6 doubles) per BspLeaf, wide_node per
// 4-wide node (the binary node it is two levels of).  RefitMesh: one mesh's ranges (fth::FlatScene::MeshRange); device_built: the ranges
// are a device job's, where binary node i also exists as BspLeaf leaf_first + i and only those of more than four triangles are nodes of
// the tree; pad: the builders' inflation for the new vertices, 1e-7 * extent + 1e-300.
struct RefitArrays {
    double* tris; ftd::BspNode* nodes; const ftd::BspLeaf* leaves; const uint32_t* tri_orig; double* wide; float* coarse;
    const int32_t* wide_node; int32_t* parent_node; int32_t* parent_leaf; uint32_t* arrived; double* leaf_boxes;
};
struct RefitMesh {
    uint32_t first_global, n;
    uint32_t node_first, node_count, leaf_first, leaf_count, tri_first, tri_count, wide_first, wide_count;
    int32_t bvh_root;                  // INT32_MIN: the mesh has no BVH - its records alone are written
    uint32_t device_built;
    uint32_t coarse_first, coarse_count;
    double pad;
};
// The parent of every node and leaf of the mesh's tree, once per full commit (the tables must hold -1 in the mesh's ranges before).
void refit_parents(hipStream_t stream, const RefitArrays& A, const RefitMesh& m);
// verts: the mesh's new vertices in HBM, n x 9 doubles (a, b, c).  Records and sorted copies, boxes leaves to root, 4-wide slots, coarse boxes.
void refit_mesh(hipStream_t stream, const RefitArrays& A, const RefitMesh& m, const double* verts);
// Ranges of bytes copied from one geometry set to another (k_refit_carry, ft_scene_commit_deformed_enqueue): the ranges
// of the meshes a queued refit does not edit, where the set it writes is behind the live one.  One launch copies every range of the
// table, in 16-byte lanes with an 8-byte element at an unaligned end; src, dst and bytes are multiples of 8, src and dst congruent
// modulo 16 (the same offset into two hipMalloc'ed arrays), and no two ranges of a table overlap.
constexpr int kCarryRanges = 60;                                   // per launch: twelve meshes' five ranges
struct CarryRange { const char* src; char* dst; uint64_t bytes; };
struct CarryTable { uint32_t n, pad; CarryRange r[kCarryRanges]; };
void refit_carry(hipStream_t stream, const CarryTable& t);
// The surface-area cost of the mesh's binary tree as it lies in HBM (k_refit_cost), with A(box) = dx dy + dy dz + dz dx:
//   ( sum over the real inner nodes of A(stored box) + sum over the leaves of n_tris x A(exact bound of the leaf's sorted records) ) / A(root's stored box),
// 0 when the root's area is 0 or not finite.  Reads A.tris, A.nodes and A.leaves only (the refit's own tables may be null).  partials:
// refit_cost_blocks(m) doubles of scratch in HBM; *cost (in HBM) receives the result.  The sum has a fixed shape - lane shuffles, the four
// waves of a block through LDS, the blocks' partials in index order - so that one tree gives the same bits on every device and run.
inline uint32_t refit_cost_blocks(const RefitMesh& m) { return (m.node_count + 255u) / 256u; }
void refit_cost(hipStream_t stream, const RefitArrays& A, const RefitMesh& m, double* partials, double* cost);

// Morph targets (ft_morph.hip, ft_sg_set_mesh_weights + ft_scene_commit_deformed).  MorphBlend: resident = the mesh's
// base, then its n_targets deltas, `stride` doubles apart (count = 9 x triangles of them used; stride even and resident and out 16-byte
// aligned); out[i] = blend(base, deltas, w)[i] in fth::morph_blend's arithmetic - what refit_mesh then reads as `verts`.
constexpr int kMaxMorphTargets = 16;                               // FT_MAX_MORPH_TARGETS (ft_capi.cpp asserts it)
struct MorphBlend { const double* resident; double* out; uint64_t count, stride; int32_t n_targets; double w[kMaxMorphTargets]; };
void morph_blend(hipStream_t stream, const MorphBlend& a);
// fth::scan_mesh over n triangles in HBM, bit for bit (a zero bound has the sign of the first zero in list order): out->bounds, extent,
// finite (1.0 / 0.0).  partials: morph_blocks(n) records of scratch, one per block of 256 triangles in a fixed slot, folded by a second launch.
struct MorphPartial { double b[6]; double extent; uint32_t at[6]; uint32_t finite, pad; };
struct MorphScanOut { double bounds[6]; double extent; double finite; };
struct MorphCentre { double c[3]; };
inline uint32_t morph_blocks(uint32_t n) { return n / 256u + (n % 256u ? 1u : 0u); }
void morph_scan(hipStream_t stream, const double* verts, uint32_t n, MorphPartial* partials, MorphScanOut* out);
// fth::ls_pair_extent(verts, n, true, c) over vertices in HBM: *out (in HBM) = the largest L1 distance of a vertex from c, in that
// function's arithmetic; partials: morph_blocks(n) doubles of scratch.
void morph_extent(hipStream_t stream, const double* verts, uint32_t n, const double c[3], double* partials, double* out);

// Skinning (ft_skin.hip, ft_sg_set_mesh_bones + ft_scene_commit_deformed).  SkinPose: out[3c .. 3c+2] = the corner
// src[3c .. 3c+2] posed by fth::skin_blend's arithmetic, c < corners.  index: one word per corner, bone j in byte j (every byte below
// n_bones); weight: slot-major, weight[j * wstride + c]; palette: n_bones x 12 doubles, 16-byte aligned.  src == out is allowed (a lane
// reads its own corner before it writes it); corners <= 0xFFFFFFFF.
constexpr int kMaxSkinBones = 256, kMaxSkinInfluences = 4;        // FT_MAX_SKIN_BONES, FT_MAX_SKIN_INFLUENCES (ft_capi.cpp asserts them)
struct SkinPose { const double* src; double* out; const uint32_t* index; const double* weight; const double* palette; uint64_t corners, wstride; int32_t influences, n_bones; };
void skin(hipStream_t stream, const SkinPose& a);
// Dual-quaternion skinning (k_skin_dq, ft_sg_set_mesh_bones_dq): the same arguments, posed by fth::skin_blend_dq's
// arithmetic; palette: n_bones x 8 doubles (real part, then dual part), 16-byte aligned.
void skin_dq(hipStream_t stream, const SkinPose& a);

// Refit of a light-space shadow tree whose light turned (ft_lightspace.hip, ft_scene_commit_lights).  LsFrame: the pair's new frame and
// centre as its record holds them (ft_flat.h, kLsPairDoubles) and the builder's inflation, 1e-7 * R + 1e-30.  One call per level of the
// tree, deepest first: order[0 .. count) are that level's 4-wide nodes (indices into ls_nodes), whose child boxes are written again -
// leaf children from their records in ls_tris, node children from the boxes the call before wrote.
struct LsFrame { double U[3], V[3], D[3], c[3], pad; };
void ls_refit_level(hipStream_t stream, uint32_t* ls_nodes, uint32_t n_nodes, const double* ls_tris, uint32_t n_tris, const uint32_t* order, uint32_t count, const LsFrame& F);
// The leaf records of a tree whose mesh was refit (k_ls_gather): ls_tris[ls_first + i] = tris[src[i]] bitwise, i < count, for every src[i]
// inside the mesh's list-order records [mesh_first, mesh_first + mesh_n); n_tris, n_ls: the sizes of tris and ls_tris in records.
void ls_gather(hipStream_t stream, const double* tris, uint32_t n_tris, uint32_t mesh_first, uint32_t mesh_n, const uint32_t* src, uint32_t count, double* ls_tris, uint32_t n_ls,
               uint32_t ls_first);
// The order of a pair's leaf records under "light_space_retree" (DESIGN.md 17.1).  ls_morton_keys (k_ls_keys): for the pair's n list-order
// triangles, records first_tri .. first_tri + n of tris (n_tris records in all), keys[k] = the 32-bit Morton code of the centre of
// triangle k's (u, v) rectangle in frame F - 16 bits per axis over [-R, R], u in the even bits - and vals[k] = first_tri + k.
// ls_sort_pairs: rocprim's stable radix sort of (keys, vals) ascending by key (tmp = null: *tmp_bytes receives the scratch size needed).
void ls_morton_keys(hipStream_t stream, const double* tris, uint32_t n_tris, uint32_t first_tri, uint32_t n, const LsFrame& F, double R, uint32_t* keys, uint32_t* vals);
hipError_t ls_sort_pairs(hipStream_t stream, const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out, uint32_t n, void* tmp, size_t* tmp_bytes);
// The grid of such a pair built again (ft_scene.cpp, build_grid, its host loops as passes; tris: the mesh's n list-order records in HBM):
//   ls_grid_entries     ebox[5 k ..] = triangle k's entry box; ruv (zeroed by the caller, or null): the bits of Ru and Rv
//   ls_grid_count       sums[a] (zeroed by the caller) += the cells every entry covers under candidate a of build_grid's attempt loop
//   ls_grid_cell_counts counts[cell] (zeroed) = entries of the cell under the chosen candidate; *max_count (zeroed, or null) = the fullest cell's
//   ls_grid_scan        first = exclusive scan of counts (tmp = null: *tmp_bytes receives the scratch size needed)
//   ls_grid_emit        the grid itself: cell words at ls_nodes[at ..], entry boxes behind them, the entries' records at ls_tris[9 tri_at ..];
//                       cursor: n_u x n_v zeroed words, idx: n_entries words of scratch.  Entries of a cell sorted by (w_max descending, list
//                       index ascending), so two builds of the same input are byte-identical whatever order the atomics arrive in.
struct LsGridCandidates { int n; float s[8]; uint32_t nu[8], nv[8]; };
void ls_grid_entries(hipStream_t stream, const double* tris, uint32_t n, const LsFrame& F, float* ebox, uint32_t* ruv);
void ls_grid_count(hipStream_t stream, const float* ebox, uint32_t n, const LsGridCandidates& C, unsigned long long* sums);
void ls_grid_cell_counts(hipStream_t stream, const float* ebox, uint32_t n, float s, uint32_t nu, uint32_t nv, uint32_t* counts, uint32_t* max_count);
hipError_t ls_grid_scan(hipStream_t stream, const uint32_t* counts, uint32_t* first, uint32_t n_cells, void* tmp, size_t* tmp_bytes);
void ls_grid_emit(hipStream_t stream, const float* ebox, const double* tris, uint32_t n, float s, uint32_t nu, uint32_t nv, const uint32_t* counts, const uint32_t* first,
                  uint32_t* cursor, uint32_t* idx, uint32_t n_entries, uint32_t* ls_nodes, uint32_t at, double* ls_tris, uint32_t tri_at);
// The edge records of one pair's grid (k_ls_edges; option "edge_cull"): `pair`, the pair's record in HBM, names the frame and the cell
// table; one wave per cell, one lane per entry, edges[kEdgeFloats * r ..] for the entry's record r of ls_tris.  node_words, n_recs: the
// sizes of ls_nodes and of ls_tris (and so of edges): nothing beyond them is read or written.  No host twin: it runs after every upload
// or rebuild of the arrays, on every device.
void ls_edge_records(hipStream_t stream, const double* pair, const uint32_t* ls_nodes, uint32_t node_words, const double* ls_tris, uint32_t n_recs, uint32_t n_cells, float* edges);

// Per-pixel surface buffers (ft_render_aov): for every entry of the chunk's pixel list (gen: pix_base, n_pix; one sample plane) the
// closest hit of the geometry ray of sample `sample` - primary_ray_from exactly as k_primary calls it, then slightOffset - and what
// the shaders would see there.  Planes are struct-of-arrays by list position: out.<x>[i] for entry pix_base + i, the 3-vectors as
// three planes of `stride` entries (x, y, z).  A null plane is not written.  counters[0] += hits, counters[1] += rays whose hit
// list overflowed.
struct AovOut {
    double *t, *p, *n, *colour, *material;
    int32_t *leaf, *node, *triangle;
    uint32_t stride;
};
struct AovSource { const uint32_t* tri_src; const int32_t* run_nodes; };   // the tables only k_aov reads (ft_flat.h)
void launch_aov(const Launch& L, const DevScene& S, const Primary& gen, uint32_t sample, const AovSource& src, const AovOut& out, unsigned long long* counters);
int occupancy_blocks_aov(size_t lds_bytes, int variant);

// A window of k_aov's planes by position, as the passes below read it: entry i of the window is the pixel pixel_ids[first + i]
// (y * res_h + x), 0 <= i < n; p, n and colour are three planes of `stride` entries each (x, y, z), leaf and triangle one.  A pass fills
// in the planes it asked k_aov for; the others stay null.  (triangle comes first: behind stride it shifts the kernel arguments of the
// kernels that do not read it, and k_temporal<false> and k_temporal<true> then schedule to 4 more bytes of code - DESIGN.md 16.2.)
struct GuideWindow { const int32_t* triangle; const uint32_t* pixel_ids; uint32_t first, n; const double *p_plane, *n_plane, *colour; const int32_t* leaf; uint32_t stride; };

// ft_denoise (ft_denoise.hip; the filter is defined in functracer_hip.h and DESIGN.md 11).  The guide record of a pixel, in FRAME
// layout (index y * res_h + x), one plane per component: what a tap reads of its neighbour (n, p, class: 49 bytes) and what only the
// pixel itself needs (the demodulation divisor d, the variance factor V: 32 bytes).
enum : uint8_t { kDenoiseMiss = 0, kDenoiseHit = 1, kDenoiseOutside = 2 };   // outside the request's tiles: no tap matches it
struct DenoiseGuides { double* n[3]; double* p[3]; double* d[3]; double* v; uint8_t* cls; };
constexpr size_t kDenoiseGuideBytes = 10 * 8 + 1;
// k_denoise_scatter: a window of k_aov's planes (n, p, colour, leaf) into the guide records of its pixels, and u0 = frame / d.
// sum != null: V from the running sums of an adaptive progressive accumulation over the same list (ProgressiveArgs' layout, n_list
// entries); else V = 1.
struct DenoiseScatterArgs {
    GuideWindow win;
    const double* frame; double* u0;
    DenoiseGuides g;
    int32_t demodulate; double albedo_floor;
    const double *sum, *sq; const uint32_t* blk; uint32_t n_list; double variance_floor;
};
void launch_denoise_scatter(hipStream_t stream, const DenoiseScatterArgs& a);
// k_denoise: one a-trous iteration with taps `step` pixels apart over the whole frame, u_in -> u_out (res_v x res_h x 3 doubles each).
// inv_s*2 = 1 / sigma^2 (the colour one already scaled by 4^i), 0: that term is off.  `last`: the result is multiplied by d and goes
// to out8 as RGBA8 bytes when that is non-null, else to u_out.
struct DenoiseArgs {
    const double* u_in; double* u_out; uint8_t* out8;
    DenoiseGuides g;
    int32_t res_h, res_v, step;
    double inv_sn2, inv_sp2, inv_sc2;
};
void launch_denoise(hipStream_t stream, const DenoiseArgs& a, bool last);
void launch_denoise_quantise(hipStream_t stream, const double* rgb, uint8_t* out8, uint32_t n_px);   // ft_quantise_rgba8 on the device

// ft_temporal_* (ft_temporal.hip; the accumulation is defined in functracer_hip.h and DESIGN.md 12).  A history set in FRAME layout
// (index y * res_h + x), one plane per component as DenoiseGuides: what decides whether a tap takes part first (leaf, N: 12 bytes,
// then n, p: 48), then what it contributes (M, Q: 48).
struct TemporalSet { double* m[3]; double* q[3]; double* len; double* p[3]; double* n[3]; int32_t* leaf; };
constexpr size_t kTemporalSetBytes = 13 * 8 + 4;
constexpr double kTemporalMinWeight = 1.0 / 16.0;   // FT_TEMPORAL_MIN_WEIGHT (functracer_hip.h; ft_context.h asserts that they agree)
// k_temporal: one lane per entry of a window of the pixel list.  k_aov's planes of the window (p, n, leaf) and the frame's colour
// at the pixel are blended with what `prev` holds where the pixel's point projects to through the previous call's image plane (o, i,
// j, k, tlx, tly, pw, ph); the pixel's record goes into `cur`, its mean into out_rgb (frame layout, 3 doubles per pixel) and out8
// (RGBA8) where those are non-null.  has_prev == 0: the first call after begin.
// tol_scale = position_tolerance_px * max(pw, ph).  counters[0] += pixels with valid history, counters[1] += pixels at max_history
// (three words: [2] is the clamp's, below).
// motion: null (the scene has the pose the history was written in), or one record of kTemporalMotionDoubles per leaf of the scene
// (n_leaves of them) that takes a hit pixel's point and normal back to that pose before they are projected and compared:
//   [0..11] D, rows of the 3x4 map from a current world point of the leaf to where that point was; [12..20] A, rows of the 3x3
//   inverse of D's linear part (a normal goes back through its transpose); [21] 1.0 if the leaf moved, 0.0: p and n are used as they
//   are; [22], [23] unused.
constexpr int kTemporalMotionDoubles = 24;
// deform: null, or one record per leaf of the scene for k_temporal<MOVING, true> ("temporal_follow_deformed"): a hit pixel
// on a leaf whose mesh was snapshotted before a refit (n > 0) and whose triangle (the window's triangle plane) changed goes back to
// where its material point was - its barycentric coordinates in the live record tris[first_live + triangle], the same coordinates in
// snap[snap_first + triangle] (9 doubles each: v0, e1, e2), then H.  W: the live w2m of the leaf; H, Wh: its m2w and the linear part of
// its w2m in the pose the history was written in (rows).  Such a pixel does not take the motion record's way: this one ends in that pose.
struct TemporalDeformLeaf { double W[12], H[12], Wh[9]; uint32_t first_live, snap_first, n, pad; };
// The colour boxes of the neighbourhood clamp (clause 3a of ft_temporal_accumulate): per channel the planes lo and hi in FRAME layout,
// written by k_temporal_box from the frame and read by k_temporal by pixel id.  counters[2] += pixels the clamp moved.
struct TemporalBox { double* lo[3]; double* hi[3]; };
constexpr size_t kTemporalBoxBytes = 6 * 8;
constexpr int kTemporalClampMaxRadius = 3;
struct TemporalArgs {
    GuideWindow win;
    const double* frame;
    TemporalSet prev, cur;
    double o[3], i[3], j[3], k[3], tlx, tly, pw, ph;
    int32_t res_h, res_v, has_prev;
    double max_history, min_normal_dot, tol_scale;
    double* out_rgb; uint8_t* out8;
    unsigned long long* counters;
    const double* motion; uint32_t n_leaves;
    const TemporalDeformLeaf* deform; const double *tris, *snap;
    // the neighbourhood clamp (ft_temporal_set_clamp), read by k_temporal<.., .., true> alone: box.lo[0] null = off and
    // k_temporal<.., .., false> runs.  Behind everything else, so the arguments the unclamped kernels read lie where they lay.
    TemporalBox box; double clamped_history;
};
void launch_temporal(hipStream_t stream, const TemporalArgs& a);
// k_temporal_box: one lane per pixel of the rect (x0, y0, w, h), clipped to the frame; a workgroup stages its 64 x 4 pixels and a halo
// of `radius` (1 .. 3) of the frame's colours in the LDS and writes box.lo and box.hi of clause 3a.  mask: one byte per frame pixel,
// non-zero for the pixels in T.
struct TemporalBoxArgs {
    const double* frame; const uint8_t* mask; TemporalBox box;
    int32_t res_h, res_v, x0, y0, w, h, radius;
    double gamma, floor;
};
void launch_temporal_box(hipStream_t stream, const TemporalBoxArgs& a);
// k_temporal_report: the hand-over at the end of a queued temporal call (ft_temporal_enqueue), the frame driver's launch_report for the
// temporal counts.  One wavefront, the call's last kernel on its stream: it copies k_temporal's three counts and the guide pass's two
// (hits, rays whose hit list overflowed) into `report` - the device-side address of a pinned record the host reads once the call's last
// event has passed - and clears both sets of counters for the next call.
struct TemporalReport { unsigned long long with_history, at_max, clamped, hits, overflow, pad[3]; };   // 64 bytes
static_assert(sizeof(TemporalReport) == 64, "k_temporal_report writes the record as eight 8-byte cells");
void launch_temporal_report(hipStream_t stream, unsigned long long* temporal_counters, unsigned long long* guide_counters, TemporalReport* report);

// ft_temporal_filter (ft_temporal_filter.hip; the filter is defined in functracer_hip.h and DESIGN.md 13): a variance-guided a-trous
// filter that reads a history set in place.  Its own planes, in FRAME layout: the demodulation divisor d (one plane per channel; null
// without `demodulate`: d = 1), the class (DenoiseGuides' values), and two colour buffers (3 doubles per pixel) and two variance planes
// the iterations alternate between.  Before k_tfilter_prepare the class plane holds kDenoiseOutside outside the tiles and anything
// else inside; prepare makes that hit or miss.
struct TFilterPlanes { const double* d[3]; uint8_t* cls; };
// The demodulate scatter: a window of k_aov's planes (colour, leaf) into d of its pixels: max(colour, albedo_floor) where the set's
// leaf is a hit and the guide's leaf is the same one, else 1.
struct TFilterScatterArgs {
    GuideWindow win;
    const int32_t* set_leaf; double* d[3]; double albedo_floor;
};
void launch_tfilter_scatter(hipStream_t stream, const TFilterScatterArgs& a);
// k_tfilter_prepare: one lane per pixel of the rect (x0, y0, w, h), clipped to the frame.  Writes the class, u0 = M / d (M itself with
// `raw`: the call has no iterations and returns M bit for bit; then also out8 where non-null) and v0, the temporal variance or, where
// N < min_history, the larger of it and the 7x7 spatial estimate.  inv_s*2 = 1 / sigma^2, 0: that term is off.
struct TFilterPrepareArgs {
    TemporalSet set; TFilterPlanes g;
    double* u0; double* v0; uint8_t* out8;
    int32_t res_h, res_v, x0, y0, w, h, raw;
    double min_history, inv_sn2, inv_sp2;
};
void launch_tfilter_prepare(hipStream_t stream, const TFilterPrepareArgs& a);
// k_tfilter: one a-trous iteration with taps `step` pixels apart over the whole frame, the 3x3 prefilter of the variance fused in:
// (u_in, v_in) -> (u_out, v_out).  n, p are read from the set's planes.  `last`: the colour is multiplied by d and goes to u_out
// and, as RGBA8 bytes, to out8, each where non-null.  At steps 1 and 2 tile and halo are staged in the LDS.
struct TFilterArgs {
    const double* u_in; const double* v_in; double* u_out; double* v_out; uint8_t* out8;
    TemporalSet set; TFilterPlanes g;
    int32_t res_h, res_v, step;
    double inv_sn2, inv_sp2, inv_sc2, variance_floor;
};
void launch_tfilter(hipStream_t stream, const TFilterArgs& a, bool last);

// Debug: closest hit / blocked for arbitrary rays (no slightOffset).
void launch_debug_closest(const Launch& L, const DevScene& S, const double* o, const double* d, uint32_t n,
                          int32_t* hit, double* t, double* p, double* nrm, double* colour, unsigned long long* overflow);
void launch_debug_blocked(const Launch& L, const DevScene& S, const double* o, const double* d, const double* max_dist,
                          uint32_t n, int32_t* blocked, unsigned long long* overflow);

} // namespace ftk
#endif

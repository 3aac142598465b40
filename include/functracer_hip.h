/*
 * functracer_hip.h — C ABI of libfunctracer_hip.so, the MI355X (gfx950) replacement for
 * FuncTracer's per-pixel render loop.
 *
 * The reference (antonburger/FuncTracer, F#) has no FFI seam of its own.  The seam this
 * library fills is the module surface of Scene.fs + Image.fs as consumed by SceneParser.fs
 * and Program.fs:
 *
 *   - the ft_sg_* / ft_scene_* builder mirrors the constructors of Scene.Primitive
 *     (Scene.fs:8-18), Scene.SceneGraph / SceneFunction (Scene.fs:33-46), Transform
 *     (Transform.fs:25-38), Ray.Material (Ray.fs:4-10), Light (Light.fs:19-26) and
 *     Scene.Scene (Scene.fs:107-110);
 *   - ft_render replaces, in one call, what Program.fs:54-64 does on the CPU:
 *     ImagePlane.create (Image.fs:67-81), JitteredSampling.generateRays (Image.fs:100-110),
 *     Shading.shade (Shading.fs:141-147) and JitteredSampling.blendPixels (Image.fs:112-116);
 *   - ft_quantise_rgba8 is Image.write's toByte (Image.fs:36).
 *
 * Conventions: plain C, no exceptions cross the boundary.  Functions returning int32_t return
 * FT_OK (0) or a negative ft_status; functions returning ft_node return a non-negative handle
 * or a negative ft_status.  ft_last_error(ctx) gives a UTF-8 message owned by the context.
 * All arrays are caller-owned and only read for the duration of the call.  A context is not
 * re-entrant (one call at a time); different contexts may be used from different threads.
 * All floating point is IEEE double, as in the reference (F# float).
 *
 * There is NO CPU fallback: ft_create fails with FT_ERR_NO_DEVICE when no HIP device is
 * usable.  The CPU restatement under oracle/ is test infrastructure and is never linked here.
 */
#ifndef FUNCTRACER_HIP_H
#define FUNCTRACER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FT_ABI_VERSION 2

typedef struct ft_context ft_context;
typedef int32_t ft_node;

typedef enum ft_status {
    FT_OK = 0,
    FT_ERR_INVALID = -1,      /* bad argument / bad handle                                   */
    FT_ERR_NO_DEVICE = -2,    /* no usable HIP device (there is no CPU fallback)            */
    FT_ERR_HIP = -3,          /* a HIP runtime call failed; see ft_last_error               */
    FT_ERR_UNSUPPORTED = -4,  /* part of the Scene.fs surface not on the device path yet     */
    FT_ERR_STATE = -5,        /* call order violated (e.g. render before commit)            */
    FT_ERR_OVERFLOW = -6,     /* a per-ray CSG hit list exceeded its capacity (never silent) */
    FT_ERR_BUILD = -7         /* BSP build failed (degenerate edge, see Triangle.fs:8-10)    */
} ft_status;

/* Scene.Primitive without payload, in the order of Scene.fs:10-17. */
typedef enum ft_primitive_kind {
    FT_PRIM_CIRCLE = 0,         /* Cylinder.circle        Cylinder.fs:22    */
    FT_PRIM_SQUARE = 1,         /* Cube.square            Cube.fs:9-15      */
    FT_PRIM_CUBE = 2,           /* Cube.cube              Cube.fs:17-25     */
    FT_PRIM_SPHERE = 3,         /* Sphere.sphere          Sphere.fs:11-21   */
    FT_PRIM_PLANE = 4,          /* Plane.plane            Plane.fs:28-33    */
    FT_PRIM_CONE = 5,           /* Cone.cone              Cone.fs:7-27      */
    FT_PRIM_SOLID_CYLINDER = 6, /* Cylinder.solidCylinder Cylinder.fs:25-29 */
    FT_PRIM_CYLINDER = 7        /* Cylinder.cylinder      Cylinder.fs:8-20  */
} ft_primitive_kind;

/* Csg.union / intersect / subtract / exclude, Csg.fs:96-99, Scene.fs:36-39. */
typedef enum ft_csg_op { FT_CSG_UNION = 0, FT_CSG_INTERSECT = 1, FT_CSG_SUBTRACT = 2, FT_CSG_EXCLUDE = 3 } ft_csg_op;

/* One basic Transform.Transform (Transform.fs:25-29).  A list of them is a Composed
 * (Transform.fs:30, 41-45): first listed is applied first (Transform.fs:70-71). */
typedef enum ft_transform_kind { FT_TRANSLATE = 0, FT_SCALE = 1, FT_ROTATE = 2 } ft_transform_kind;
typedef struct ft_transform {
    int32_t kind;     /* ft_transform_kind                                                   */
    int32_t _pad;
    double v[3];      /* translation vector | scale factors | rotation axis (normalised by the
                         library exactly as Transform.rotate does, Transform.fs:37-38)       */
    double angle;     /* radians, FT_ROTATE only                                             */
} ft_transform;

/* Ray.Material (Ray.fs:4-10). */
typedef struct ft_material {
    double colour[3];
    double roughness;
    double reflectance;
    double shineyness;
    int32_t apply_lighting; /* bool */
    int32_t _pad;
} ft_material;

/* Image.Camera (Image.fs:10-17).  focus = depth of field (Image.fs:91-94); the reference draws its
 * direction jitter from an unseeded System.Random, here it comes from the seeded stream keyed by
 * ft_render's `seed`. */
typedef struct ft_camera {
    double o[3];
    double look_at[3];
    double up[3];
    double fov_y;        /* radians */
    double aspect_ratio;
    int32_t has_focus;
    int32_t _pad;
    double focal_length;
    double aperture_angular_size; /* radians */
} ft_camera;

typedef struct ft_rect { int32_t x0, y0, w, h; } ft_rect;

/* Counters and timings of one ft_render call. */
typedef struct ft_stats {
    uint64_t rays_primary;   /* W*H*spp over the rendered tiles                                */
    uint64_t rays_shadow;    /* shadow rays actually traced                                    */
    uint64_t rays_reflect;   /* reflection rays actually traced                                */
    uint64_t rays_traced;    /* rays the device traced: rays_primary - rays_primary_culled + rays_shadow + rays_reflect */
    double   rays_reference_equivalent; /* what the F# recursion would trace (Shading.fs:109-139):
                                L shadow rays per hit and L reflection rays per reflective hit  */
    uint64_t hits_primary;   /* primary rays that hit something                                */
    uint64_t csg_overflow;   /* rays whose CSG hit list overflowed (render then fails)         */
    double   kernel_ms;      /* HIP-event time over all kernels of the call, on the library's stream */
    double   wall_ms;        /* host wall time of the call incl. copies                        */
    double   trace_kernel_ms;/* HIP-event time of the closest-hit + shade/shadow kernels only  */
    uint64_t algorithmic_bytes; /* bytes the pipeline has to move for this frame by construction (roofline) */
    int32_t  n_launches;     /* kernels of the call as it is planned from the request: k_classify (one, also when "classify_reuse" finds it done), then per
                              * window k_primary, the k_bounce levels the level hint asks for and k_resolve - also for windows "classify_reuse" does not launch.
                              * k_block_lists, which rides behind k_classify, is not counted.  ft_debug_classify_reuse tells what really ran */
    int32_t  n_chunks;       /* windows of the pixel list the call is cut into, planned the same way (launched or not) */
    uint64_t hits_total;     /* hits shaded over all bounces                                   */
    uint64_t algorithmic_bytes_closest; /* unused since ABI 2 (always 0)                       */
    uint64_t algorithmic_bytes_shade;   /* the k_bounce share (bounces >= 1)                   */
    uint64_t rays_tail;      /* unused since ABI 2 (always 0): kept so the layout of ABI 1 callers' struct prefix stays */
    uint64_t rays_primary_culled; /* primary rays (part of rays_primary) resolved as misses per 64-pixel block: the block's ray
                                   * bundle cannot reach any object, so they were never generated one by one          */
    uint64_t algorithmic_bytes_primary; /* the k_primary (fused bounce 0) share of algorithmic_bytes                          */
    uint64_t rays_shadow_primary;  /* the part of rays_shadow cast by hits of primary rays (traced inside k_primary)          */
    uint64_t rays_reflect_primary; /* the part of rays_reflect spawned by hits of primary rays                                */
} ft_stats;

/* ---- context ---------------------------------------------------------------------------- */
int32_t ft_abi_version(void);
/* device_ids: HIP device ordinals; n_devices must be >= 1 (0 ⇒ FT_ERR_NO_DEVICE: no CPU path).  With several
 * ordinals the scene is replicated on each device and every ft_render splits its region into 8-row bands dealt
 * round-robin over them, one host thread per device, no exchange between devices: every device copies its bands (whole rows of
 * the frame) straight into the caller's buffer. */
int32_t ft_create(const int32_t* device_ids, int32_t n_devices, ft_context** out);
void    ft_destroy(ft_context* ctx);
const char* ft_last_error(const ft_context* ctx);
/* Tunables: "chunk_samples" (samples in flight per launch; default 16 Mi, frames whose pixel blocks are classified use twice that), "csg_mesh_capacity" (hit-list entries a mesh may add under
 * CSG; default 32), "csg_auto_grow" (default 1: a blocking ft_render (and the ft_debug_* ray queries) whose hit lists overflow doubles that capacity, re-commits and renders the
 * frame again instead of returning FT_ERR_OVERFLOW; the error remains for lists that stop fitting in the LDS and for ft_render_enqueue), "timing" (HIP events recorded inside ft_render: 0 around the frame only, 1 = default: also around
 * k_primary and the k_bounce levels, 2 around every stage; each bracketed boundary costs about 6 us of stream time), "classify_pixels" (default 1: 64-pixel blocks whose ray bundle
 * cannot reach any object are finished before any ray is generated; the bundle is bounded from the jitter pattern handed to ft_render, whatever its range), "level_hint" (default 1: a frame launches as many levels of the reflection tree as the
 * previous frame of the same scene, size and samples had rays in, plus one, whose rays are followed to the end inside the launch; 0: always max_depth levels), "follow_below" (levels in which that
 * previous frame had no more rays than this are not worth a launch and are followed as well; -1 = default: two rays per SIMD of the device; 0: every level that had a ray), "mesh_unclipped_bvh" (non-default fast mode: ignore bspMesh depth, BVH over the original triangles; pixels may
 * differ from the reference-shaped clipped BSP in the last bits), "bvh_builder" (who builds the exact BVH of top-level-Leaf meshes at commit - 0: the host, a swept
 * surface-area split (the best tree, a slow build: 160 ms for 70 K triangles); 1: the device, a linear BVH (1 ms, traces ~9 % slower); 3: the device, a binned surface-area tree
 * over the Morton order (5.5 ms, traces like the host's or better); 2 = default: the host below 4096 triangles, the device's surface-area tree from there on),
 * "light_space_shadows" (2 = default: the shadow rays of a directional light in a coherent wave look up a uniform grid built at commit in the light's frame
 * for each top-level `bspMesh 0` leaf, and walk the tree of option 1 where a wave spans more than a few cells; 1: they walk a tree built in the light's
 * frame; 0: they walk the mesh's BVH like every other ray.  Same triangle records, same results bit for bit; a value other than 0 / 1 means 2; a change
 * re-commits),
 * "primary_block_lists" (1 = default: in a classified frame over a scene with exactly one top-level `bspMesh 0` leaf, one wave per active 8x8 block walks the
 * mesh's tree once with the block's pyramid and keeps the triangles whose rectangle on the image plane overlaps the block's; the block's primary rays then test
 * that short list instead of walking the tree, each from the root.  Blocks with more than 64 candidates, progressive passes and scenes with several such leaves
 * keep the walk; 0: the walk everywhere.  Same triangle records, the closest hit does not depend on the order they are offered in: same frames bit for bit),
 * "uniform_surface" (1 = default: a bounce-0 wavefront whose hit lanes all lie on one leaf reads that leaf's record, matrices and material once, through scalar
 * loads, instead of once per lane (scenes with meshes and without textures, rough materials or soft lights: the kernel the headline runs); the shaders leave out what no lane of the wavefront reads (the specular term's three normalisations, the regenerated view ray);
 * and, with "primary_block_lists", a wavefront whose block has an empty candidate list stores Colour.Zero without generating its rays when the mesh is the scene's
 * only item and the camera has no focus.  0: everything per lane, nothing left out.  Same expressions either way: same frames and counters bit for bit),
 * "primary_mesh_kernel" (1 = default: bounce 0 of a scene that is one lit top-level `bspMesh 0` leaf and nothing else, under directional lights only, with no
 * rough, textured or reflective material and no specular exponent that needs Math.Pow, runs k_primary_mesh - the same steps and expressions as k_primary's for such
 * a scene, without the code such a scene never reaches, in fewer registers and with more waves in flight - when the camera has no focus and the frame is a plain
 * (not progressive, not corner-sampled) one in grouped numbering with "coherent_waves" and "uniform_surface" on; 0: k_primary everywhere.  Same frames and
 * ft_stats (times aside) bit for bit; no re-commit, and what the frame slots keep of their classifications stays),
 * "edge_cull" (1 = default: beside its rectangle every entry of a block's candidate list and of a directional light's shadow grid carries the three edges of its
 * projected triangle, and a wavefront whose own rectangle lies wholly outside one of them skips the triangle without fetching it; slivers, triangles that reach the
 * camera plane and scenes past the record cap carry none.  Only triangles no ray of the wavefront can hit are skipped: same frames and ft_stats (times aside) bit
 * for bit.  0: the rectangles alone.  Read per frame; no re-commit, and what the frame slots keep of their classifications stays),
 * "classify_reuse" (1 = default: a classified frame whose scene commit, frame size, tiles, camera, jitter extent (not the offsets) and candidate-list leaf equal, field
 * for field, those of the frame that last classified into the same one of the four frame slots launches neither k_classify nor k_block_lists: it reads that frame's
 * block maps, lists and active count as they are, and launches only the windows of its pixel list that hold active pixels - a held view, whatever its pattern, seed, samples
 * or max_depth, from the fifth frame on.  Every commit, a frame of another key, a progressive pass, a corner-sampled or unclassified frame in the slot, an error, and setting
 * this option, "classify_pixels" or "primary_block_lists" drop what a slot keeps.  0: every frame classifies.  Same frames and ft_stats (times aside) bit for bit),
 * "classify_ahead" / "resolve_aside" / "zero_fill_skip" (1 = default: what a stream of queued frames does that a single frame cannot - the next frame's k_classify on a second
 * stream, k_resolve on a third with the sample colours double-buffered, Colour.Zero not written again into blocks the last frame of the same signature left zero; 0 switches each off; k_resolve goes aside only in frames of one chunk), "mains" (2 = default, 1 .. 3: queued frames of one chunk take turns on that many main streams, so a frame's kernels are dispatched while its predecessor's drain
 * and two frames' reflection levels fill each other's idle stretches), "wave_samples" (0 = default, 16: a bounce-0 wavefront takes up to that many jitter offsets of 64 / that many pixels of an
 * 8x8 block when the sample count has the power of two in it - a narrower bundle; 1, 2, 4, 8, 16; no pixel depends on it),
 * "refit_rebuild_percent" (0 = default: never; 100 .. 1000000: ft_scene_commit_deformed builds the tree of an edited, device-built mesh again in place once
 * its measured cost x 100 exceeds this x its cost as built - "deforming meshes" below; any other value is refused.  It is read by ft_scene_commit_deformed
 * alone and needs no new ft_scene_commit),
 * "deform_light_space" (0 = default; any other value means 1: ft_scene_commit_deformed refits the light-space shadow trees of the meshes it edits and builds their
 * grids again on the device instead of stripping them - "deforming meshes" below.  It is read by ft_scene_commit_deformed alone and needs no new
 * ft_scene_commit; a host-only context accepts it without effect, because its deformed commit is the full host commit, which builds the structures anyway; with 0
 * every call launches the kernels and gives the bits it gave before the option existed),
 * "light_space_retree" (0 = default; any other value means 1: ft_scene_commit_lights and ft_scene_commit_deformed build the topology of every light-space shadow
 * tree they would refit again on the device from the current projection, instead of keeping the one the last full commit built - "moving lights" below.  It is
 * read by those two calls alone and needs no new ft_scene_commit; a host-only context accepts it without effect, because both calls are the full host commit
 * there; with 0 both calls launch the kernels and write the bytes they wrote before the option existed),
 * "moved_in_place" (0 = default; any other value means 1: ft_scene_commit_moved uploads the new poses over the old ones and brings the light-space shadow
 * structures up to them on the device, instead of committing the whole scene again, whenever nothing but poses changed - "moving rigid objects" below.  It is
 * read by ft_scene_commit_moved alone and needs no new ft_scene_commit; a host-only context accepts it without effect, because its moved commit is the full host
 * commit; with 0 every call launches the kernels and gives the bits it gave before the option existed),
 * "temporal_follow_deformed" (0 = default; any other value means 1: ft_scene_commit_deformed keeps the triangle records of the meshes it refits as the open
 * temporal accumulation last saw them, and the next ft_temporal_accumulate takes every pixel on a changed triangle back to where that point of the triangle was -
 * "history on deforming meshes" below.  It needs no new ft_scene_commit; a host-only or multi-device context accepts it without effect, because the accumulation
 * lives on a single device; with 0 every call launches the kernels and gives the bits it gave before the option existed),
 * "morph_on_device" (1 = default; any other value means 0: ft_scene_commit_deformed blends the vertices of
 * the meshes that ft_sg_set_mesh_weights describes on the device, from a base and deltas resident in HBM, and scans them there - "morph targets" below; with 0
 * the host blends them and the call is the ft_sg_set_mesh_triangles path, the same bits.  It is read by ft_scene_commit_deformed alone and needs no new
 * ft_scene_commit; a host-only context accepts it without effect),
 * "skin_on_device" (1 = default; any other value means 0: ft_scene_commit_deformed poses the meshes that carry a bone palette on the
 * device, from indices, weights and a rest shape resident in HBM - "skinning" below; with 0 the host skins them and the call is the
 * ft_sg_set_mesh_triangles path, the same bits.  It is read by ft_scene_commit_deformed alone and needs no new ft_scene_commit; a
 * host-only context accepts it without effect).  Every option reaches every device of a context.  Scene-affecting
 * options need a new ft_scene_commit.  Any other key is refused (FT_ERR_INVALID, "unknown option"). */
int32_t ft_set_option(ft_context* ctx, const char* key, int64_t value);

/* ---- scene graph builder (Scene.fs:8-53) ------------------------------------------------- */
ft_node ft_sg_primitive(ft_context* ctx, int32_t kind);                       /* Scene.fs:10-17  */
ft_node ft_sg_triangle(ft_context* ctx, const double v[9]);                   /* Scene.fs:18     */
/* BspMesh.bspMesh false depth triangles (BspMesh.fs:88-97); tris = n x 9 doubles (a,b,c). */
ft_node ft_sg_bsp_mesh(ft_context* ctx, int32_t depth, const double* tris, int64_t n_tris); /* Scene.fs:9 */
ft_node ft_sg_transform(ft_context* ctx, const ft_transform* ts, int32_t n, ft_node child); /* Scene.fs:42 */
/* Replaces the transform list of an existing ft_sg_transform node (the child stays; n may differ from the old count): see
 * "moving rigid objects" below. */
int32_t ft_sg_set_transform(ft_context* ctx, ft_node node, const ft_transform* ts, int32_t n);
ft_node ft_sg_material(ft_context* ctx, const ft_material* m, ft_node child);  /* Scene.fs:43     */
ft_node ft_sg_hue_shift(ft_context* ctx, double angle, ft_node child);         /* Scene.fs:45     */
ft_node ft_sg_ignore_light(ft_context* ctx, ft_node child);                    /* Scene.fs:46     */
ft_node ft_sg_group(ft_context* ctx, const ft_node* children, int32_t n);      /* Scene.fs:35     */
ft_node ft_sg_csg(ft_context* ctx, int32_t op, ft_node a, ft_node b);          /* Scene.fs:36-39  */
/* Scene.fs:44,47-53.  uv_ops: n x {kind, a, b}, outermost TextureFunction first: {0, sx, sy} = Scale, {1, radians, 0} =
 * Rotate (Textures/Texture.fs:13-22); at most 5 per texture. */
ft_node ft_sg_texture_grid(ft_context* ctx, const double colour_a[3], const double colour_b[3],
                           const double* uv_ops, int32_t n_uv_ops, ft_node child);
/* Texture.Image (Scene.fs:48; ImageTexture.image, Textures/Image.fs:20-36).  The F# closure owns the decoded pixels;
 * here the caller hands them over: rgb24 = image.SavePixelData() of an Image<Rgb24>, width*height*3 bytes, row 0 first
 * (copied).  Lookup is the reference's nearest texel at index y*(3*width)+3*x with x = floor(u*width), y = floor(v*height)
 * after Texture.repeat; an index past the last texel (where the reference raises) reads the last texel. */
ft_node ft_sg_texture_image(ft_context* ctx, const uint8_t* rgb24, int32_t width, int32_t height,
                            const double* uv_ops, int32_t n_uv_ops, ft_node child);

/* ---- scene (Scene.fs:107-110, Light.fs:19-26) -------------------------------------------- */
int32_t ft_scene_clear(ft_context* ctx);
int32_t ft_scene_set_objects(ft_context* ctx, ft_node root);
int32_t ft_scene_add_directional(ft_context* ctx, const double dir[3], const double colour[3]);
int32_t ft_scene_add_soft_directional(ft_context* ctx, const double dir[3], int32_t samples,
                                      double scatter_rad, const double colour[3]);
int32_t ft_scene_add_positional(ft_context* ctx, const double pos[3], const double falloff[3],
                                const double colour[3]);
/* Flatten the graph, build BSP trees (BspMesh.compile, BspMesh.fs:51-65) and upload to HBM.  The exact BVH that stands in for the
 * linear scan of a `bspMesh 0` (BspMesh.fs:95-97) is built by the host below 4096 triangles and on the device from there on ("bvh_builder" = 2, default).
 * A graph beyond a limit of the device path (CSG nesting, hits per ray in a CSG subtree, lights, soft-light samples, uv
 * functions, LDS) is FT_ERR_UNSUPPORTED with a message that names the limit.  A commit the flattener refuses - for a limit, or for a
 * graph without objects (FT_ERR_STATE) - replaces nothing: the scene committed before it, if any, stays in HBM and stays renderable. */
int32_t ft_scene_commit(ft_context* ctx);
/* Wall time of the last ft_scene_commit in ms: [0] flatten on the host (includes the host's BVH builds with "bvh_builder" = 0),
 * [1] BVH builds on the device, [2] uploads and the rest; [3] is not a time: the height of the tallest device-built tree. */
int32_t ft_get_commit_times(ft_context* ctx, double ms[4]);

/* ---- render (Program.fs:54-64) ----------------------------------------------------------- */
/* res_h x res_v is Image.Resolution (Image.fs:28).  jitter_xy = spp x 2 offsets, the ONE pattern
 * shared by every pixel (Image.fs:105); spp == 0 selects `samples corner` (CornerSampling, Image.fs:125-150:
 * one ray per pixel corner, jitter_xy ignored).  max_depth = the recursion limit (8 in Shading.fs:142).
 * seed keys the counter-based streams of soft lights.  tiles == NULL renders the whole frame;
 * otherwise only pixels inside the n_tiles rects are written.  out_rgb is res_v x res_h x 3
 * doubles, row 0 = top (Image.fs:39).  out_rgb may be NULL: the frame then stays in HBM until
 * ft_fetch_frame copies it out (same layout; only the last render's tile pixels are written). */
int32_t ft_render(ft_context* ctx, const ft_camera* cam, int32_t res_h, int32_t res_v, int32_t spp,
                  const double* jitter_xy, int32_t max_depth, uint64_t seed,
                  const ft_rect* tiles, int32_t n_tiles, double* out_rgb, ft_stats* stats);

int32_t ft_fetch_frame(ft_context* ctx, double* out_rgb);

/* The same frame as Image.write consumes it (Image.fs:35-44): RGBA8, one byte per channel = truncate(clamp01(c) * 255) (Image.fs:36,
 * Math.fs:12-16; NaN -> 0), alpha 255, res_v x res_h x 4 bytes, row 0 = top.  The quantisation runs on the device in the kernel
 * that averages the samples, so 4 instead of 24 bytes per pixel cross the PCIe link; bytes are identical to ft_quantise_rgba8 of
 * ft_render's frame.  After ft_render_rgba8 / ft_render_enqueue_rgba8 the frame in HBM is the RGBA8 one: fetch it with
 * ft_fetch_frame_rgba8 (ft_fetch_frame then returns FT_ERR_STATE, and vice versa). */
int32_t ft_render_rgba8(ft_context* ctx, const ft_camera* cam, int32_t res_h, int32_t res_v, int32_t spp,
                        const double* jitter_xy, int32_t max_depth, uint64_t seed,
                        const ft_rect* tiles, int32_t n_tiles, uint8_t* out_rgba, ft_stats* stats);
int32_t ft_fetch_frame_rgba8(ft_context* ctx, uint8_t* out_rgba);

/* Page-locked host memory (hipHostMalloc) for frames handed to ft_render / ft_fetch_frame*: the copy out of HBM is then one DMA
 * without the runtime's staging through its own pinned buffers.  Optional: any host pointer works. */
void* ft_host_alloc(size_t bytes);
void  ft_host_free(void* p);

/* A queued frame that also leaves the device: the copy into host_out (res_v x res_h x 3 doubles, or x 4 bytes with rgba8 != 0) is queued
 * behind the frame's last kernel and is complete when ft_render_wait returns (or when a later call retires the frame).  host_out should
 * come from ft_host_alloc (one DMA beside the next frame's tracing); one buffer per frame in flight (four at most: a buffer is the host's again once
 * a later call has retired its frame - queuing frame k + 4 retires frame k - or ft_render_wait has returned). */
int32_t ft_render_enqueue_into(ft_context* ctx, const ft_camera* cam, int32_t res_h, int32_t res_v, int32_t spp, const double* jitter_xy,
                               int32_t max_depth, uint64_t seed, const ft_rect* tiles, int32_t n_tiles, int32_t rgba8, void* host_out);

/* Pipelined rendering, for hosts that render frame after frame (an animation, a progressive preview):
 * ft_render_enqueue queues a frame exactly as ft_render(out_rgb = NULL) would and returns without waiting, so the host prepares
 * the next frame while this one runs; at most four frames are in flight (queuing a fifth first waits for the oldest: one or two are traced, the next
 * waits dispatched on another stream, the last is being classified).  On a context
 * over several devices every device queues its bands on its own stream; ft_render_wait waits for all of them and sums their statistics.
 * ft_render_wait blocks until everything queued has finished, reports the statistics of the LAST frame, and leaves in
 * ft_get_kernel_times the stage times and launch counts summed over all frames since the previous wait.  The frame buffer holds
 * the last frame (ft_fetch_frame).  The reference's own flow is synchronous (Program.fs:63-64): ft_render stays that way. */
int32_t ft_render_enqueue(ft_context* ctx, const ft_camera* cam, int32_t res_h, int32_t res_v, int32_t spp, const double* jitter_xy,
                          int32_t max_depth, uint64_t seed, const ft_rect* tiles, int32_t n_tiles);
int32_t ft_render_enqueue_rgba8(ft_context* ctx, const ft_camera* cam, int32_t res_h, int32_t res_v, int32_t spp, const double* jitter_xy,
                                int32_t max_depth, uint64_t seed, const ft_rect* tiles, int32_t n_tiles);
int32_t ft_render_wait(ft_context* ctx, ft_stats* stats);

/* ---- progressive accumulation ------------------------------------------------------------- */
/* A frame refined pass by pass without tracing any sample twice: each pass adds samples to the running per-pixel sums of one fixed
 * request, and pixels whose 8x8 block has settled stop receiving samples.
 *  - Exactness: pixel p holds S, the sum of its samples per channel in the order they were traced (pass order, then sample order within a
 *    pass); a pass's resolve continues that sum from S, and the mean is S / n.  A frame built from passes over pieces of a jitter pattern is
 *    therefore bit-identical to one ft_render over the whole pattern (Image.fs:112-116: Array.average is a sequential sum, then one
 *    division).  A block that k_classify finishes in a pass adds spp zero samples: S unchanged, n += spp, what tracing them gives.
 *  - Seeded streams: soft-light and depth-of-field streams of a pass are keyed as in an ft_render of that pass (sample = pixel_id * spp + s,
 *    with the pass's spp and seed): a pass's samples are those of ft_render(cam, spp, jitter_xy, seed).  Give each pass its own seed.
 *  - Retirement (tolerance > 0): after each pass, per pixel and channel var = max(0, Q/n - (S/n)^2) * n / (n - 1) and se = sqrt(var / n),
 *    with Q the running sum of squares.  A 64-pixel block (an 8x8 tile of the list) retires when n >= min_samples and the largest se of
 *    its 64 pixels and 3 channels is <= tolerance.  Retirement is final: a retired block is never traced again and its S, Q, n stay.
 *    Q adds each sample's square rounded on its own, and every operation of var and se is rounded on its own (nothing is fused): the
 *    device judges a block by exactly the se ft_progressive_fetch reports for it.
 *  - Lifetime: one accumulation per context; a caller's ft_scene_commit or ft_scene_clear ends it (the next pass returns FT_ERR_STATE, as a
 *    pass without a begin does).  The re-commit by which a blocking call grows the CSG hit lists does not: the pass that overflowed leaves no
 *    trace and runs again.  ft_render calls between passes are allowed and change nothing accumulated.  A pass retires queued frames first,
 *    overwrites the frame buffer (ft_fetch_frame / ft_fetch_frame_rgba8 return the means) and forgets which blocks the last ft_render
 *    left as Colour.Zero.
 *  - Multi-device contexts: each device accumulates, retires and copies out the 8-row bands ft_render gives it; fetch and status combine them.
 *  - Host-only contexts: FT_ERR_NO_DEVICE from every ft_progressive_* call.
 * Device memory: 48 bytes per tile pixel (S, two copies), 96 with tolerance > 0 (Q too), and 8 bytes per 64-pixel block. */
/* Start a progressive accumulation (a second begin replaces the first).  Fixes the camera, frame size, recursion limit and tiles (as
 * ft_render's) for every later pass.  tolerance <= 0: plain accumulation, nothing retires.  tolerance > 0: adaptive; min_samples >= 2 is
 * required (else FT_ERR_INVALID) and every clipped tile must have sides that are multiples of 8 (else FT_ERR_UNSUPPORTED). */
int32_t ft_progressive_begin(ft_context* ctx, const ft_camera* cam, int32_t res_h, int32_t res_v, int32_t max_depth,
                             const ft_rect* tiles, int32_t n_tiles, double tolerance, int32_t min_samples);
/* One blocking pass: spp >= 1 new samples (jitter_xy = spp x 2, seed as ft_render's) for every block not yet retired; spp == 0 (corner
 * sampling, whose blend is not a per-pixel average) is FT_ERR_UNSUPPORTED.  Writes the running mean of every tile pixel (retired blocks
 * included) into out, laid out as ft_render's out_rgb, or as ft_render_rgba8's bytes if rgba8 != 0.  out may be NULL: the mean then stays
 * in the frame buffer for ft_fetch_frame / ft_fetch_frame_rgba8.  stats: as ft_render's, for this pass. */
int32_t ft_progressive_pass(ft_context* ctx, int32_t spp, const double* jitter_xy, uint64_t seed, int32_t rgba8, void* out, ft_stats* stats);
/* The accumulated state of the tile pixels; any pointer may be NULL: mean (res_v x res_h x 3; 0 before the first pass), standard error of
 * the mean per channel (same shape; 0 where fewer than 2 samples; adaptive accumulations only, else FT_ERR_STATE), samples per pixel
 * (res_v x res_h). */
int32_t ft_progressive_fetch(ft_context* ctx, double* mean_rgb, double* stderr_rgb, uint32_t* samples);
/* out = passes, min and max samples per pixel, 64-pixel blocks in the accumulation, blocks retired, samples traced in the last pass
 * (the listed samples of the blocks its active list held). */
int32_t ft_progressive_status(ft_context* ctx, int64_t out[6]);
/* End the accumulation and free its buffers (FT_OK when there is none). */
int32_t ft_progressive_end(ft_context* ctx);

/* ---- per-pixel surface buffers (AOVs) ---------------------------------------------------------- */
/* ft_render_aov reports, for every tile pixel, the hit of the geometry ray of sample `sample` that
 * ft_render(cam, res_h, res_v, spp, jitter_xy, max_depth, seed, tiles) would trace for that pixel: rayThroughPixel with jitter offset
 * `sample` (Image.fs:83-89), depth of field with the stream key pixel_id * spp + sample exactly as a frame's sample, then slightOffset
 * (Shading.fs:129-136).  The buffers therefore describe the surface that sample of the frame shades, bit for bit.  printIntersectionAt
 * (Program.fs:33-49) intersects the un-offset ray instead: the two disagree only for surfaces closer than 1e-4 * |d| to the eye.
 * Planes are row-major res_v x res_h, row 0 = top (as ft_render's out_rgb); 3-vectors are 3 doubles per pixel.  Only tile pixels are
 * written.  Per pixel (hit | miss):
 *   t         RayIntersection.t along the offset ray                                                   | +inf
 *   p         the hit point the shaders use                                                            | 0
 *   n         the normal the shaders see (after transforms and flipNormals)                            | 0
 *   colour    the material colour after texture and hueShift (what ft_debug_closest reports)           | 0
 *   material  reflectance, shineyness, roughness                                                       | 0
 *   leaf      index of the placed primitive in the committed scene (a flattened leaf)                  | -1
 *   node      the ft_node of the ft_sg_primitive / ft_sg_triangle / ft_sg_bsp_mesh call that made the leaf (a node placed twice
 *             gives two leaves and one node); under CSG the operand whose surface was hit               | -1
 *   triangle  meshes: index into the tris handed to ft_sg_bsp_mesh (a piece clipped by the BSP build reports the face it was cut
 *             from); ft_sg_triangle: 0; other primitives: -1                                            | -1
 * Device memory: up to 116 bytes per pixel of a window of "chunk_samples" pixels, plus the pixel list. */
typedef struct ft_aov {            /* any pointer may be NULL: that channel is neither computed into HBM nor copied */
    double* t; double* p; double* n; double* colour; double* material;
    int32_t* leaf; int32_t* node; int32_t* triangle;
} ft_aov;
/* Blocking; retires queued frames first.  spp == 0 (corner sampling) is FT_ERR_UNSUPPORTED; sample outside [0, spp) or no channel
 * requested FT_ERR_INVALID; a host-only context FT_ERR_NO_DEVICE.  Hit lists that overflow grow and the call runs again (csg_auto_grow).
 * Multi-device contexts split the frame into ft_render's 8-row bands.  stats: rays_primary, hits_primary, kernel_ms, wall_ms and
 * n_launches; the other fields are 0.  The frame buffer (ft_fetch_frame*), the next ft_render's history and a progressive accumulation
 * are left as they were. */
int32_t ft_render_aov(ft_context* ctx, const ft_camera* cam, int32_t res_h, int32_t res_v, int32_t spp, const double* jitter_xy,
                      int32_t sample, uint64_t seed, const ft_rect* tiles, int32_t n_tiles, const ft_aov* out, ft_stats* stats);

/* ---- denoising the frame in HBM ---------------------------------------------------------------- */
/* ft_denoise filters the FP64 frame that is in HBM (what ft_fetch_frame would return) on the device with an edge-avoiding a-trous
 * wavelet filter (Dammertz et al. 2010), FP64, guided by the surface buffers ft_render_aov defines for the same
 * (cam, res, spp, jitter_xy, sample, seed, tiles).  Per frame pixel x: c(x) the frame; n(x), p(x), a(x) the normal, point and
 * `colour` plane of sample `sample`'s geometry ray; k(x) its class, hit (leaf >= 0) or miss; T the tile pixels of the request (the
 * clipped rects, the whole frame when tiles == NULL); se(x) the per-channel standard error of the mean of a live ADAPTIVE progressive
 * accumulation, as ft_progressive_fetch defines it (use_variance only).
 *   d(x) = per channel max(a(x), albedo_floor) for a hit pixel when `demodulate`, else 1;  u_0 = c / d.
 *   V(x) = variance_floor + (1/3) * sum_ch (se_ch(x) / d_ch(x))^2 when `use_variance`, else 1.
 *   for i = 0 .. iterations-1, s = 2^i, h = [1/16, 1/4, 3/8, 1/4, 1/16], taps q = x + s * (dx, dy), dy = -2 .. 2 outer, dx = -2 .. 2 inner
 *   (the summation order); a tap takes part only if q is in T and k(q) == k(x):
 *     E = |n(x)-n(q)|^2 / sigma_normal^2 + |p(x)-p(q)|^2 / sigma_position^2 + |u_i(x)-u_i(q)|^2 / ((sigma_colour * 2^-i)^2 * V(x))
 *     (a term whose sigma is 0 is left out; for miss pixels n and p are 0, so only the colour term acts),
 *     w = h[dx+2] * h[dy+2] * exp(-E),   u_{i+1}(x) = (sum w * u_i(q)) / (sum w).   The centre tap has E = 0: the denominator is never 0.
 *   Non-finite data never spreads: a tap whose E is NaN or whose u_i(q) has a non-finite channel is skipped, and a pixel whose own
 *   u_i(x) has a non-finite channel is copied through unchanged (the reference's specular term can produce NaN, Shading.fs:85-87).
 *   Result: u_N(x) * d(x) for every x in T; pixels outside T are not written; iterations == 0 returns c bit for bit.
 * The variance is NOT filtered from iteration to iteration (SVGF does; out of scope).  The guides are those of ONE sample: a
 * depth-of-field frame gets sample `sample`'s surfaces and is softened accordingly.
 * Blocking; retires queued frames first.  `out` is laid out as ft_render's out_rgb, or as ft_render_rgba8's bytes when rgba8 != 0
 * (quantised on the device: the bytes of ft_quantise_rgba8 of the FP64 result); whole rows leave as one copy, as ft_fetch_frame's do
 * (one DMA when out came from ft_host_alloc).
 * Errors, checked before anything runs: spp == 0 FT_ERR_UNSUPPORTED; sample outside [0, spp), null params / out, iterations outside
 * 0 .. 6, a negative (or NaN) sigma, a floor <= 0 where it is used FT_ERR_INVALID; then a host-only context FT_ERR_NO_DEVICE; a context
 * over several devices FT_ERR_UNSUPPORTED (the frame lives in bands on different devices and a tap crosses bands); no FP64 frame of
 * res_h x res_v in HBM (nothing rendered, an RGBA8 frame, another size) FT_ERR_STATE; use_variance without a live adaptive accumulation
 * of the same size and tiles FT_ERR_STATE.  Hit lists that overflow in the guide pass grow and the call runs again (csg_auto_grow).
 * The frame buffer, the next ft_render's history and a progressive accumulation are left as they were.
 * stats: rays_primary / hits_primary of the guide pass (0 when iterations == 0: there is none), kernel_ms, wall_ms, n_launches; the
 * rest 0.  Device memory, allocated on first use and kept: 81 bytes per frame pixel of guides, two colour buffers of 24, 4 of RGBA8
 * when asked for, beside ft_render_aov's window (76 bytes per pixel of it: n, p, colour, leaf). */
typedef struct ft_denoise_params { int32_t iterations, demodulate, use_variance, _pad;
    double sigma_colour, sigma_normal, sigma_position, albedo_floor, variance_floor; } ft_denoise_params;
int32_t ft_denoise(ft_context* ctx, const ft_camera* cam, int32_t res_h, int32_t res_v, int32_t spp,
                   const double* jitter_xy, int32_t sample, uint64_t seed, const ft_rect* tiles, int32_t n_tiles,
                   const ft_denoise_params* params, int32_t rgba8, void* out, ft_stats* stats);

/* ---- reprojected frame accumulation for a moving camera ---------------------------------------- */
/* ft_temporal_* accumulates the FP64 frames a host renders along a camera path: each pixel's surface point is projected into the
 * previous call's image, what was accumulated there is fetched, checked for being the same surface and blended with the new frame.
 * The scene is static (leaf ids and points are compared in world space) unless it is moved with ft_scene_commit_moved ("moving rigid
 * objects" below).  State lives in the context, on a single device: two history
 * sets in frame layout (row 0 = top), "previous" and "current", flipped after every call; per frame pixel a set holds the mean M (3
 * doubles), the mean of squares Q (3), the history length N (1), p and n (3 each) and leaf (int32): 108 bytes; and the previous call's
 * image plane cam' (ImagePlane.create of its ft_camera, Image.fs:48-81: o' i' j' k', the top-left pixel centre tlx' tly', the pixel
 * size pw' ph').  ft_temporal_begin sets N = 0 everywhere in both sets.
 * ft_temporal_accumulate takes c(x), the FP64 frame in HBM (what ft_fetch_frame would return); p(x), n(x), leaf(x) as ft_render_aov
 * defines them for the call's (cam, res, spp, jitter_xy, sample, seed, tiles); T, the tile pixels fixed at begin.  For every x in T:
 *  1. Projection, for a hit pixel (leaf(x) >= 0) with a previous call behind it: v = p(x) - o', zc = v.k'; if zc > 0:
 *     fx = ((v.i')/zc - tlx') / pw', fy = (tly' - (v.j')/zc) / ph' (the inverse of rayThroughPixel, Image.fs:83-89, at jitter 0: pixel
 *     centres sit at integer coordinates); x0 = floor(fx), y0 = floor(fy), wx = fx - x0, wy = fy - y0.
 *  2. Taps q = (x0+dx, y0+dy), dy = 0, 1 outer, dx = 0, 1 inner (the summation order), b_q = (dx ? wx : 1-wx) * (dy ? wy : 1-wy).  A tap
 *     is valid iff q is in the frame, N'(q) >= 1, leaf'(q) == leaf(x), n(x).n'(q) >= min_normal_dot,
 *     |p(x)-p'(q)|^2 <= (position_tolerance_px * max(pw', ph') * zc)^2, and M'(q), Q'(q) are finite in every channel.
 *  3. W = sum of b_q over the valid taps; the history is valid iff W >= FT_TEMPORAL_MIN_WEIGHT (which also makes the result continuous
 *     where fx crosses an integer).  Then M_h = (sum b_q M'(q)) / W, Q_h and N_h likewise; N(x) = min(N_h + 1, max_history);
 *     M(x) = M_h + (c(x) - M_h) / N(x); Q(x) = Q_h + (c(x)^2 - Q_h) / N(x) per channel.
 *  3a. The neighbourhood clamp, only while ft_temporal_set_clamp (below) has it on, with its radius r, gamma, floor and clamped_history;
 *     for a pixel whose history is valid by clause 3 (so c(x) is finite).  No product here is fused with a sum.
 *     Taps q = x + (dx, dy), dy = -r .. r outer, dx = -r .. r inner (the summation order); a tap takes part iff q lies in the frame, q is
 *     in T (the frame outside the tiles is not this render's) and c(q) is finite in every channel.  k = the number of taps that took
 *     part; k >= 1, as x itself does.  Per channel: s1 = sum c(q); s2 = sum (c(q) * c(q)); mu = s1 / k; v = s2 / k - mu * mu;
 *     sd = sqrt(v > 0 ? v : 0); h = gamma * sd + floor; lo = mu - h, hi = mu + h.
 *     M_c = M_h < lo ? lo : (M_h > hi ? hi : M_h) per channel; clamped(x) = M_c != M_h in any channel.
 *     Where clamped(x): per channel Vh = Q_h - M_h * M_h and Q_c = M_c * M_c + (Vh > 0 ? Vh : 0) - the history keeps its variance around
 *     the moved mean - and N_h = min(N_h, clamped_history).  Elsewhere Q_c = Q_h and N_h stays.
 *     Clause 3 then continues with M_c, Q_c and that N_h: N(x) = min(N_h + 1, max_history), M(x) = M_c + (c(x) - M_c) / N(x), Q likewise;
 *     clamped_history = 0 therefore restarts a clamped pixel at M = c.  Pixels without valid history take clause 4 or 5 as before; a
 *     miss pixel has no history, so the clamp never touches it.
 *  4. No history (a miss pixel, the first call after begin, zc <= 0, W below the constant): N(x) = 1, M(x) = c(x) bit for bit,
 *     Q(x) = c(x)^2.
 *  5. Non-finite data never spreads: a pixel whose c(x) has a non-finite channel stores N(x) = 0, M(x) = c(x) (and Q(x) = c(x)^2), so
 *     no later tap uses it; clause 2 already rejects non-finite history.
 *  6. M, Q, N, p(x), n(x), leaf(x) go into the current set (p = n = 0 for a miss); pixels outside T are never written and keep N = 0.
 *     The sets are then flipped and cam' = cam.
 *  7. M(x) for x in T goes to `out`, laid out as ft_render's out_rgb, or as ft_render_rgba8's bytes when rgba8 != 0 (quantised on the
 *     device with ft_quantise_rgba8's arithmetic); out may be NULL.  With to_frame != 0, M also replaces the tile pixels of the FP64
 *     frame in HBM, so ft_fetch_frame and ft_denoise see the accumulated frame (and which blocks the last ft_render left as Colour.Zero
 *     is forgotten, as after a progressive pass: a later ft_render is bit-identical all the same).
 * With a static camera this is the running mean of the frames up to max_history, an exponential average after that.
 * Lifetime: one accumulation per context (a second begin replaces the first); a caller's ft_scene_commit or ft_scene_clear ends it,
 * because leaf ids are only comparable within one commit; the re-commit by which a blocking call grows the CSG hit lists does not.
 * Errors of ft_temporal_accumulate, checked before anything runs, in this order: spp == 0 FT_ERR_UNSUPPORTED; then FT_ERR_INVALID
 * for spp < 0 or a null jitter_xy, sample outside [0, spp), null cam or params, max_history < 1, min_normal_dot NaN or outside
 * [-1, 1], position_tolerance_px not > 0; then a host-only context FT_ERR_NO_DEVICE; a context over several devices
 * FT_ERR_UNSUPPORTED (taps cross the bands the frame lives in, as ft_denoise's); then FT_ERR_STATE for no begin, an accumulation
 * ended by a commit, or no FP64 frame of the begin's size in HBM.  ft_temporal_begin: FT_ERR_INVALID for a size below 2 x 2 or
 * tiles != NULL with n_tiles < 1, then FT_ERR_NO_DEVICE and FT_ERR_UNSUPPORTED as above.
 * The call blocks and retires queued frames first.  Hit lists that overflow grow and the call runs again (csg_auto_grow); a call that
 * failed leaves the history as it was.  stats: rays_primary, hits_primary, kernel_ms, wall_ms, n_launches, and trace_kernel_ms = the
 * share of kernel_ms that is the guide pass (k_aov); the rest 0.  The cached pixel list, the level hint, a progressive accumulation
 * and (without to_frame) the frame buffer stay untouched.
 * Device memory: 216 bytes per frame pixel (the two sets), 24 for the FP64 result and 4 for RGBA8 when asked for, beside
 * ft_render_aov's window (52 bytes per pixel of it: p, n, leaf). */
#define FT_TEMPORAL_MIN_WEIGHT 0.0625   /* 1/16 */
typedef struct ft_temporal_params { int32_t max_history, to_frame; double min_normal_dot, position_tolerance_px; } ft_temporal_params;
int32_t ft_temporal_begin(ft_context* ctx, int32_t res_h, int32_t res_v, const ft_rect* tiles, int32_t n_tiles);
int32_t ft_temporal_accumulate(ft_context* ctx, const ft_camera* cam, int32_t spp, const double* jitter_xy, int32_t sample, uint64_t seed,
                               const ft_temporal_params* params, int32_t rgba8, void* out, ft_stats* stats);
/* The accumulated state of the tile pixels (frame-shaped planes; other pixels are not written); any pointer may be NULL: the mean M
 * (res_v x res_h x 3), the standard error of the mean per channel, sqrt(max(0, Q - M*M) / max(N, 1)) with the product unfused and 0
 * where N < 2 (same shape), and the history length N (res_v x res_h).  FT_ERR_STATE without an accumulation. */
int32_t ft_temporal_fetch(ft_context* ctx, double* mean_rgb, double* stderr_rgb, double* length);
/* out = calls since begin, tile pixels, pixels with valid history in the last call, pixels whose N is max_history after it. */
int32_t ft_temporal_status(ft_context* ctx, int64_t out[4]);
/* The neighbourhood clamp of the history (clause 3a above; variance clipping, Salvi 2016): the fetched history mean is moved into the
 * box mu +- (gamma * sd + floor) of the CURRENT frame's (2r+1)^2 neighbourhood before it is blended, and the history is shortened to
 * clamped_history where that moved it.  Without it the history follows surfaces but not their shading: a shadow or a reflection that
 * left a surface whose history is valid lingers for up to max_history calls.  Off after ft_temporal_begin: every kernel launched and
 * every bit produced is then what it is without these functions.
 * ft_temporal_set_clamp may be called any time between ft_temporal_begin and the end of the accumulation; every later
 * ft_temporal_accumulate reads it, nothing already accumulated changes.  params == NULL switches it off.  A second begin replaces the
 * first, clamp included; whatever ends the accumulation drops it.
 *  - floor absorbs rounding where the neighbourhood is flat: there sd = 0, and a history that differs from mu in the last bit would
 *    otherwise count as clamped (and lose its length).
 *  - gamma >= sqrt((2r+1)^2 - 1) can never clamp a history that equals the current frame: no sample of k values lies further than
 *    sqrt(k - 1) standard deviations from their mean (Samuelson's inequality), and the bound is met by one bright tap among equal ones.
 *    That is 2.83 for r = 1, 4.90 for r = 2, 6.93 for r = 3.  gamma near 1 is the aggressive setting for noise-free frames; noisy
 *    1-spp frames want a larger radius and a larger gamma, or the clamp takes the noise of the neighbourhood for a change of light.
 *  - It composes with ft_scene_commit_moved, ft_scene_commit_deformed and "temporal_follow_deformed": those only change which history
 *    is fetched.  ft_temporal_filter is unaffected.  With to_frame the frame is overwritten after the boxes were taken: they see the
 *    rendered colours.
 * Errors, in this order: a null context FT_ERR_INVALID; with non-null params FT_ERR_INVALID for radius outside 1 .. 3,
 * clamped_history < 0, gamma NaN, infinite or negative, floor NaN, infinite or negative; a host-only context FT_ERR_NO_DEVICE; a
 * context over several devices FT_ERR_UNSUPPORTED; no open accumulation FT_ERR_STATE.
 * ft_temporal_clamp_status: out = the radius in force (0 = off), the pixels with clamped(x) in the last accumulate (0 after a call
 * that ran with the clamp off; a failed accumulate leaves the previous value, as it leaves the other counts).  The with_history and
 * at_max counts of ft_temporal_status keep their meaning.  FT_ERR_INVALID for a null context or out, then FT_ERR_NO_DEVICE, then
 * FT_ERR_STATE without an accumulation.
 * stats of an accumulate with the clamp on: the box pass (one kernel per clipped rect, before the first window) counts towards
 * kernel_ms and n_launches, not towards trace_kernel_ms.
 * Device memory, allocated by the first accumulate with the clamp on and freed with the accumulation: 48 bytes per frame pixel for the
 * boxes (lo and hi, three channels) and 1 for the in-T mask.  The accumulation's counters are three words. */
typedef struct ft_temporal_clamp_params { int32_t radius, clamped_history; double gamma, floor; } ft_temporal_clamp_params;  /* 24 bytes */
int32_t ft_temporal_set_clamp(ft_context* ctx, const ft_temporal_clamp_params* params);   /* params == NULL: off */
int32_t ft_temporal_clamp_status(ft_context* ctx, int64_t out[2]);   /* radius in force (0 = off), pixels clamped in the last accumulate */
/* End the accumulation and free its buffers (FT_OK when there is none). */
int32_t ft_temporal_end(ft_context* ctx);

/* ---- variance-guided filter of the temporal history -------------------------------------------- */
/* ft_temporal_filter filters, on the device, the history set the last ft_temporal_accumulate wrote (the "previous" set after the flip)
 * with an edge-avoiding a-trous filter whose colour term is scaled by a per-pixel variance that is filtered from iteration to iteration
 * (Schied et al. 2017), FP64.  The set is read in place.  Per frame pixel x: M(x), N(x), p(x), n(x), leaf(x) of the set; se_ch(x) the
 * per-channel standard error exactly as ft_temporal_fetch defines it (sqrt(max(0, Q - M*M) / max(N, 1)), the product unfused, 0 where
 * N < 2); T the tile pixels fixed at ft_temporal_begin; k(x) the class: hit (leaf >= 0) or miss for x in T, "outside" otherwise, which
 * matches no tap.  max(a, b) below is a > b ? a : b.
 *  1. d(x).  With `demodulate` one guide pass (ft_render_aov's colour a and leaf for cam, the begin's size, spp, jitter_xy, sample, seed:
 *     the arguments of the accumulate call this follows) gives, for a hit pixel whose guide leaf equals the set's leaf, d(x) = per channel
 *     max(a(x), albedo_floor); otherwise, and without `demodulate`, d(x) = 1.  Without `demodulate` cam, spp, jitter_xy, sample and seed
 *     are not read (they may be null / 0), no guide pass runs and no pixel list is uploaded.
 *  2. u_0 = M / d;  vt(x) = (1/3) * sum_ch (se_ch(x) / d_ch(x))^2.
 *  3. Where N(x) < min_history (N compared as the double that is stored), a spatial estimate: taps q = x + (dx, dy), dy = -3 .. 3 outer,
 *     dx = -3 .. 3 inner, taking part iff q is in the frame, k(q) == k(x) and u_0(q) is finite;
 *     g = exp(-(|n(x)-n(q)|^2 / sigma_normal^2 + |p(x)-p(q)|^2 / sigma_position^2)) (a term whose sigma is 0 is left out; a miss pixel has
 *     no geometric term); m1_ch = sum g * u_0(q)_ch / sum g, m2_ch = sum g * (u_0(q)_ch * u_0(q)_ch) / sum g,
 *     vs = (1/3) * sum_ch max(m2_ch - m1_ch * m1_ch, 0) with the product unfused; v_0(x) = max(vs, vt(x)).  Elsewhere v_0(x) = vt(x).
 *  4. For i = 0 .. iterations-1, s = 2^i, h = [1/16, 1/4, 3/8, 1/4, 1/16]:
 *     gv_i(x) = the 3x3 average of v_i with the weights [1/4, 1/2, 1/4] x [1/4, 1/2, 1/4] over the taps at distance 1 (not s) that are
 *     in the frame, have class k(x) and a finite v_i, renormalised by the weights that took part;
 *     taps q = x + s * (dx, dy), dy = -2 .. 2 outer, dx = -2 .. 2 inner (the summation order), taking part iff q is in the frame,
 *     k(q) == k(x), u_i(q) and v_i(q) are finite and E is not NaN, with
 *     E = |n(x)-n(q)|^2 / sigma_normal^2 + |p(x)-p(q)|^2 / sigma_position^2 + |u_i(x)-u_i(q)|^2 / (sigma_colour^2 * (gv_i(x) + variance_floor))
 *     (a term whose sigma is 0 is left out; a miss pixel has no geometric term; there is no 2^-i on sigma_colour: the variance shrinks
 *     by itself), w = h[dx+2] * h[dy+2] * exp(-E),
 *     u_{i+1}(x) = (sum w * u_i(q)) / (sum w),   v_{i+1}(x) = (sum w * w * v_i(q)) / (sum w)^2.
 *     A pixel whose own u_i(x) or v_i(x) is not finite is copied through, u and v: an N = 0 pixel of ft_temporal_accumulate's clause 5
 *     stays where it is and spreads nothing.
 *  5. u_N(x) * d(x) for x in T goes to `out`, laid out as ft_render's out_rgb, or as ft_render_rgba8's bytes when rgba8 != 0 (quantised
 *     on the device with ft_quantise_rgba8's arithmetic); v_N(x) goes to out_variance (res_v x res_h doubles); either may be NULL, not
 *     both.  Pixels outside T are not written.  iterations == 0 returns M bit for bit, and v_0.  With to_frame != 0 the FP64 result also
 *     replaces the tile pixels of the FP64 frame in HBM once the call can no longer fail (and which blocks the last ft_render left as
 *     Colour.Zero is forgotten, exactly as ft_temporal_accumulate's to_frame does).
 * The history sets, cam', the counts of ft_temporal_status, the level hint, the cached pixel list, a progressive accumulation and
 * (without to_frame) the frame buffer are left untouched: an accumulate after a filter call gives bit for bit what it gives without
 * one.  The filtered colour is NOT fed back into the history (SVGF does; it would change what ft_temporal_* means).
 * Errors, checked before anything runs, in this order: null params, or out and out_variance both null, FT_ERR_INVALID; iterations
 * outside 0 .. 6, a negative or NaN sigma, min_history < 1, variance_floor not > 0, demodulate with albedo_floor not > 0 FT_ERR_INVALID;
 * with demodulate, spp == 0 FT_ERR_UNSUPPORTED, then null cam or jitter_xy, spp < 0, sample outside [0, spp) FT_ERR_INVALID; a host-only
 * context FT_ERR_NO_DEVICE; a context over several devices FT_ERR_UNSUPPORTED; no begin, an accumulation ended by a commit, or no
 * accumulate call since begin FT_ERR_STATE; to_frame without an FP64 frame of the begin's size in HBM FT_ERR_STATE.
 * The call blocks and retires queued frames first.  Hit lists that overflow in the guide pass grow and the call runs again
 * (csg_auto_grow).  stats: as ft_temporal_accumulate's; trace_kernel_ms is the guide pass's share of kernel_ms, 0 without demodulate.
 * Device memory, allocated by the first filter call of an accumulation and freed with it (ft_temporal_end, a commit, the context), per
 * frame pixel: d 24 (with demodulate), class 1, two colour buffers of 24, two variance planes of 8, and 4 of RGBA8 when asked for. */
typedef struct ft_temporal_filter_params { int32_t iterations, demodulate, min_history, to_frame;
    double sigma_colour, sigma_normal, sigma_position, albedo_floor, variance_floor; } ft_temporal_filter_params;   /* 56 bytes */
int32_t ft_temporal_filter(ft_context* ctx, const ft_camera* cam, int32_t spp, const double* jitter_xy, int32_t sample, uint64_t seed,
                           const ft_temporal_filter_params* params, int32_t rgba8, void* out, double* out_variance, ft_stats* stats);

/* ---- queued temporal calls ------------------------------------------------------------------- */
/* ft_temporal_enqueue queues one ft_temporal_accumulate and, with filter != NULL, the ft_temporal_filter of its result, and returns;
 * ft_temporal_wait retires what is queued.  A host that renders with ft_render_enqueue keeps its pipeline: neither call waits on the
 * host for the other.
 * Meaning: a queued call produces, bit for bit, what the blocking pair
 *     ft_temporal_accumulate(cam, spp, jitter_xy, sample, seed, params, rgba8, filter ? NULL : host_out, ..), then, with a filter,
 *     ft_temporal_filter(cam, spp, jitter_xy, sample, seed, filter, rgba8, host_out, NULL, ..)
 * produces on a device that has finished everything queued before it: the two history sets and cam', the pose and the snapshots that
 * are dropped, the counts of ft_temporal_status and ft_temporal_clamp_status, the bytes in host_out.  c(x) is the FP64 frame of the last
 * frame queued or rendered before the call, a frame of ft_render_enqueue that has not finished included: the call is ordered behind
 * that frame on the device, and a later ft_render_enqueue* is ordered so that it does not overwrite the frame before the call has read it.
 *  - ft_temporal_set_clamp applies to the calls queued after it.  ft_scene_commit_moved / ft_scene_commit_deformed and
 *    "temporal_follow_deformed" work as with the blocking call; a commit retires queued temporal calls first, as it retires queued frames.
 *  - With filter->demodulate the one guide pass of the call also delivers the material colour the filter's d is made from: there is
 *    no second k_aov (same arguments, same bits).
 *  - host_out (laid out as ft_temporal_accumulate's out; the tile pixels are written) should come from ft_host_alloc, one buffer per call
 *    in flight.  A buffer is the host's again when ft_temporal_wait has returned or when call k + FT_TEMPORAL_QUEUE_DEPTH has been
 *    queued: that call waits for call k on the host, nothing else does.  host_out may be NULL only when filter is NULL.
 *  - Not offered: params->to_frame != 0 and filter->to_frame != 0 (FT_ERR_INVALID; the blocking calls do that) - the queued call never
 *    writes the frame - and the filter's variance plane (a blocking ft_temporal_filter after the wait delivers it).
 * Errors of ft_temporal_enqueue, checked before anything is queued and leaving everything as it was, in this order:
 * ft_temporal_accumulate's argument errors; with a filter, FT_ERR_INVALID for a null host_out, then ft_temporal_filter's argument
 * errors; FT_ERR_INVALID for params->to_frame, then for filter->to_frame; a host-only context FT_ERR_NO_DEVICE; a context over several
 * devices FT_ERR_UNSUPPORTED; FT_ERR_STATE for no open accumulation, or no FP64 frame of the begin's size as the host knows it when the
 * call is made.
 * A hit list that overflows in the guide pass of a queued call cannot be repaired behind the host's back: FT_ERR_OVERFLOW is returned by
 * whichever call retires the temporal call (ft_render_enqueue has the same rule), the lists do not grow, and the accumulation is ended as
 * by ft_temporal_end - later queued calls have read a history written from overflowed rays.  The remedy: one blocking ft_render or
 * ft_temporal_accumulate first, whose grown lists stay, then ft_temporal_begin again.
 * ft_temporal_wait blocks until every queued temporal call has finished, returns the first error among them, and gives the stats of the
 * last one: rays_primary, hits_primary, n_launches (the hand-over kernel behind the call is not counted), wall_ms from the enqueue to
 * its retirement, kernel_ms from one event pair around the call's device work; trace_kernel_ms is 0 (the guide pass is not bracketed
 * apart) and so is the rest.  FT_OK with nothing queued.
 * Queued temporal calls are retired first by every call that retires queued frames first, and by ft_temporal_fetch, _status,
 * _clamp_status, _begin and _end, the blocking ft_temporal_accumulate and ft_temporal_filter, ft_render_aov, ft_denoise, every commit,
 * ft_scene_clear and ft_destroy.  ft_render_enqueue* and ft_render_wait do not. */
#define FT_TEMPORAL_QUEUE_DEPTH 4
int32_t ft_temporal_enqueue(ft_context* ctx, const ft_camera* cam, int32_t spp, const double* jitter_xy, int32_t sample, uint64_t seed,
                            const ft_temporal_params* params, const ft_temporal_filter_params* filter /* NULL: no filter */,
                            int32_t rgba8, void* host_out);
int32_t ft_temporal_wait(ft_context* ctx, ft_stats* stats);

/* ---- moving rigid objects under a temporal accumulation --------------------------------------- */
/* ft_sg_set_transform + ft_scene_commit_moved move objects of a committed scene without ending ft_temporal_*: the history then follows
 * each moved leaf instead of being looked up where the leaf's surface is now.
 * ft_sg_set_transform(node, ts, n) replaces the transform list of an ft_sg_transform node.  FT_ERR_INVALID, with nothing changed, for a
 * null context, an invalid handle, a node that is not a transform node, null ts, n < 1 or a kind that is no ft_transform_kind.  Like
 * every builder call it leaves the scene uncommitted; unlike the others it is not a structural change.
 * ft_scene_commit_moved commits the graph exactly as ft_scene_commit does (the flatten, the BVH builds, the uploads, every device of the
 * context, ft_get_commit_times), so a later ft_render is bit-identical to one from a fresh context built with the new transforms.  It
 * differs in three ways:
 *  - It returns FT_ERR_STATE, and does nothing, unless the context holds a successful commit and no structural change was made since:
 *    structural are the ft_sg_* calls that add a node, ft_scene_set_objects, ft_scene_add_* and ft_scene_clear; ft_sg_set_transform and
 *    ft_set_option are not.  The graph therefore flattens to the same leaves in the same order (one m2w / w2m pair per leaf, composed
 *    over the transform nodes above it).
 *  - It ends a progressive accumulation (its sums belong to the old scene) but NOT the temporal accumulation.
 *  - It advances the context's pose counter.  (The re-commit by which a blocking call grows the CSG hit lists does not.)
 * A successful ft_temporal_accumulate remembers the pose its set was written in: the pose counter and, per leaf l, H_l = m2w(l) and
 * Wh_l = w2m(l) (3x4, rows).  An accumulate that finds the pose counter unchanged runs as defined above.  Otherwise, with m2w_cur and
 * w2m_cur the matrices of the live commit, per leaf:
 *   moved_l = any of the 12 doubles of m2w_cur(l) differs from H_l (bitwise);
 *   D_l = H_l o w2m_cur(l), the 3x4 affine product: D[i][j] = H[i][0] W[0][j] + H[i][1] W[1][j] + H[i][2] W[2][j], + H[i][3] for j = 3,
 *         summed left to right, unfused.  It maps a current world point of the leaf to where that point was;
 *   A_l = m2w_cur(l)_lin . Wh_l_lin, the 3x3 product summed the same way: the inverse of D_l's linear part.
 * and for a hit pixel x with leaf l = leaf(x) and moved_l:
 *   pr = D_l (p(x), 1): pr_i = D[i][0] p_0 + D[i][1] p_1 + D[i][2] p_2 + D[i][3], left to right;
 *   nr = A_l^T n(x): t_j = A[0][j] n_0 + A[1][j] n_1 + A[2][j] n_2, nr = t * (1 / sqrt(t.t)).
 * Clauses 1 to 3 of ft_temporal_accumulate then use pr and nr wherever they use p(x) and n(x): v = pr - o' (and with it zc, fx, fy and
 * the tolerance), nr.n'(q) >= min_normal_dot, |pr - p'(q)|^2 <= tol^2.  A non-finite nr fails every tap by those comparisons.  Clause 6
 * still stores the CURRENT p(x), n(x), leaf(x), and the pose of the live commit becomes the set's.  Miss pixels and pixels whose leaf has
 * moved_l = 0 take the path defined above with p and n untouched: static surfaces beside a moving object get the bits they would get
 * without it.  Several ft_scene_commit_moved calls between two accumulates compose by construction: H is the pose at the last
 * accumulate, not at the last commit.
 * What follows a leaf is its history, not its shading: light that changes on a moving surface (it turns towards a light, a shadow
 * sweeps over it) is averaged as noise is, max_history bounding how long it lingers - unless the neighbourhood clamp is on
 * (ft_temporal_set_clamp, clause 3a of ft_temporal_accumulate), which pulls such history to the colours the current frame shows
 * around the pixel and shortens it.  Lights move through ft_scene_commit_lights ("moving lights" below); meshes deform through
 * ft_scene_commit_deformed (below), whose history follows the triangles with "temporal_follow_deformed" ("history on deforming meshes").
 * ft_temporal_filter with `demodulate` returns FT_ERR_STATE between an ft_scene_commit_moved and the next ft_temporal_accumulate (its
 * guide pass would show another pose than the set); without `demodulate` it runs as before.
 * A host that never calls these functions gets bit-identical results from everything else.
 * Device memory: 192 bytes per leaf while a moved pose is being accumulated.
 * "moved_in_place" 1: the same contract - the FT_ERR_STATE rules, every later call gives what a fresh context built with the new
 * transforms and committed with ft_scene_commit gives, bit for bit (frames, ft_stats counters, ft_render_aov, ft_debug_closest / _blocked
 * / _colour, ft_debug_leaf_matrices), queued frames retired first, the progressive accumulation ended, the temporal one left open, the pose
 * counter advanced - without the commit: no mesh, tree or grid is built on the host and no mesh array is uploaded.  Every mesh is kept in
 * model space, so a pose is one w2m / m2w pair and a flag word per leaf, the cull records of the top-level items and the scene's table of
 * face directions; those are uploaded over the old ones.  Every (mesh leaf, directional light) pair whose frame - derived from the leaf's
 * new w2m and the light's direction - is not bitwise the one its record holds is then treated as ft_scene_commit_lights treats a light that
 * turned ("moving lights" below): record doubles [0..13] a fresh commit's, the tree refit (built anew under "light_space_retree" 1), under
 * "light_space_shadows" 2 the grid built again behind the full commit's arrays, root INT32_MIN for an unusable frame (a singular matrix).  A
 * translation changes no frame: such a call launches no kernel (ft_get_commit_times[1] is exactly 0).  A leaf back at the full commit's pose
 * under that commit's light direction, neither deformed nor retreed since, gets that commit's record and grid back.  As a refit tree decays
 * with the angle turned (the figures under "moving lights" hold for a leaf that turns as for a light that turns) and the library does not
 * decide when a fresh tree is worth a full commit, the default is 0.
 * The call still takes the full commit, and gives its bits, on a host-only context, while a light setter, an ft_sg_set_mesh_triangles or a
 * commit-time option is pending (a full commit has always absorbed those), and when the re-flatten differs from the held scene in more
 * than poses: an item that crosses six face directions (its OP_CULL pair enters or leaves the program), an item that gains or loses its
 * bounds, a scene-wide face-direction table of another length or one that overflows 32.  ft_debug_moved_commits tells which way a call went.
 * ft_get_commit_times of a call in place: [0] the host's work, [1] the light-space kernels with their readbacks, [2] the uploads, [3]
 * unchanged.  Measured on the 69.6 K-face mesh under one directional light (MI355X): a translation 0.04 - 0.05 ms, a turn
 * 1.7 - 2.3 ms (1.1 - 1.4 ms for a step that follows another), against 72 - 95 ms for the full commit; k_primary on the next frame is a
 * fresh commit's after a translation and a 1 degree turn, 1.14 x after 10 degrees, 4.2 - 4.5 x after 45 and 8.3 - 8.9 x after 90 with the
 * refit tree, and 1.03 - 1.09 x at every angle under "light_space_retree" 1. */
int32_t ft_scene_commit_moved(ft_context* ctx);
/* ---- deforming meshes: a refit instead of a rebuild -------------------------------------------- */
/* ft_sg_set_mesh_triangles + ft_scene_commit_deformed change the vertices of `bspMesh 0` meshes of a committed scene without rebuilding
 * a tree and without ending ft_temporal_*.
 * ft_sg_set_mesh_triangles(node, tris, n_tris) replaces the vertices of an existing ft_sg_bsp_mesh node; tris = n x 9 doubles as there,
 * copied.  FT_ERR_INVALID, with nothing changed, for a null context, an invalid handle, a node that is not a bspMesh node, null tris or
 * an n_tris that differs from the node's triangle count.  Like ft_sg_set_transform it leaves the scene uncommitted and is not a structural
 * change; a later plain ft_scene_commit gives what a fresh graph with the new vertices gives.
 * ft_scene_commit_deformed commits a graph in which only mesh vertices changed since the last successful commit:
 *  - FT_ERR_STATE, and nothing done, unless the context holds a successful commit and no structural change was made since (the rule of
 *    ft_scene_commit_moved), or while an ft_sg_set_transform is pending (ft_scene_commit_moved first, then deform) or an ft_set_option
 *    that needs a new ft_scene_commit.
 *  - FT_ERR_UNSUPPORTED when an edited mesh has depth above 0 (its clipped BSP depends on the positions), holds a non-finite coordinate
 *    (|v| < 1e300 fails, the builders' own test) or moves so far that a top-level item gains or loses its bounds.  This is decided on the
 *    host before anything is uploaded: the old commit stays in HBM and is renderable again; ft_scene_commit handles these cases.
 *  - On success every later call - ft_render, ft_render_enqueue, ft_progressive_*, ft_render_aov, ft_denoise, the ft_debug_* ray queries -
 *    gives what it gives on a fresh context whose graph was built with the new vertices and committed with ft_scene_commit, bit for bit.
 *  - It ends a progressive accumulation, retires queued frames first (as every commit does), leaves the temporal accumulation OPEN and
 *    does not advance the pose counter: by default a deformed leaf gets no special treatment, clause 2's leaf, normal and position tests
 *    decide pixel by pixel whether the history still fits ("temporal_follow_deformed" = 1: "history on deforming meshes" below).  On a multi-device context every device refits its own copy.  A host-only context checks
 *    the same rules and then runs the full host commit.
 *  - ft_get_commit_times: [0] host work, [1] the refit kernels, [2] uploads, [3] unchanged.  The first refit after a full commit also
 *    derives the trees' parent links on the device, inside [1].
 * What is kept: the topology of every tree as the last full commit built it, whichever builder did ("bvh_builder" 0, 1, 3) - children,
 * split axes, leaf ranges, tri_orig, tri_src, the 4-wide children, the coarse frontier; meshes that were not edited are not touched.
 * What is written again, per edited mesh: the triangle records (v0, e1 = v1 - v0, e2 = v2 - v0) and their sorted copies, the boxes of
 * the binary nodes (the exact bounds of the vertices as the hit test sees them, inflated by 1e-7 * extent + 1e-300, extent = the largest
 * |coordinate| of the new mesh), the 4-wide slot boxes, the coarse boxes; on the host the mesh bounds and the cull records of the items
 * that hold the mesh.  A tree that holds every triangle once, bounds them with inflated boxes and breaks ties by list index gives the
 * linear scan's hits whatever its shape, hence the bit-identity above.
 * "light_space_shadows" 1 / 2: the light-space trees and grids are built on the host from the vertices and are NOT refit.  Every leaf of
 * an edited mesh loses its pair records (ft_debug_light_space: 0xFFFFFFFF), so its directional shadow rays walk the refit BVH as option 0
 * does - the same bits - until the next full ft_scene_commit brings the structures back.
 * With ft_set_option("deform_light_space", 1) they are refit instead.  After a successful call every pair of an edited mesh that had a
 * tree at the last full commit, and whose leaf no earlier call stripped, still has one, and under option 2 a grid wherever the full
 * commit's rules give one:
 *  - the pair record's doubles [0..13] are what a fresh full commit of the new vertices writes, bit for bit: the frame and k_rel stay, c
 *    is the centre of the new mesh bounds, R the largest L1 distance of a new vertex from c in the full commit's arithmetic,
 *    s_abs = (k_rel + 1e-6) * R + 1e-20.  With R from 2e29 on the pair gets root INT32_MIN and no grid (the rule of
 *    ft_scene_commit_lights; its rays walk the BVH - the same bits) until a later deformation brings R back;
 *  - the tree keeps the full commit's topology; every leaf record becomes the new record of the triangle it copied (k_ls_gather, by a table
 *    the flattener keeps: duplicates that deform apart stay apart) and every box is written again about the new c with pad 1e-7 * R + 1e-30;
 *  - the grid is built again from the refit list-order records by the passes of ft_scene_commit_lights, so its resolution, cells, entry
 *    boxes, records and their order are a fresh commit's; the edge records follow.
 * Every later call gives a fresh context's bits, frames and counters, as above; the temporal accumulation stays open, the pose counter
 * stays, and "refit_rebuild_percent" and "temporal_follow_deformed" compose (neither touches list-order records after the refit).  A leaf
 * stripped by an earlier call with the option at 0 stays stripped until the next full commit.  A deformed pair's grid lies with the
 * moving lights' grids behind the full commit's arrays (ft_scene_commit_lights below): a call that edits a mesh with pairs lays that
 * region out anew and builds every grid in it again, the ones of other meshes whose lights have turned included, and from then on
 * ft_scene_commit_lights never gives such a pair the full commit's record or grid back, not even at that commit's direction - both
 * describe vertices that are gone.  The full commit's own grids of deformed pairs stay in that commit's arrays, unused, and count against
 * the 256 MiB cap until the next full commit.  On a multi-device context the first device takes the decisions that need a readback and
 * every device carries them out.  ft_get_commit_times: [1] includes the gather, tree and grid kernels with their readbacks, [2] the uploads.
 * What it is worth (MI355X, the 69.6 K-face mesh under one directional light, 1920 x 1080 x 16, tools/deform_shadow_rate.py, DESIGN.md
 * 16.3): after 1, 4 and 16 steps of a twist of 0.05 rad per step k_primary takes 1.05, 1.09 and 2.68 times a fresh commit's time and 0.79,
 * 0.83 and 2.22 times what it takes with the option at 0.  The grid is a fresh commit's, but the tree that wide waves fall back to keeps
 * the rest pose's topology and decays: at 6 steps (0.3 rad) the option makes no difference, from 8 steps (0.4 rad) on it costs.  The call
 * itself takes 2.7 ms instead of 0.95 ms; a full commit takes 86 ms.  The library does not decide when to fall back: the default is 0.
 * Tree quality: the refit tree is the OLD vertices' tree around the new ones, so its boxes overlap more the further the mesh moves from
 * the pose it was built in, and the walk slows down while the results stay exact.  The library measures how far that has gone:
 * ft_scene_tree_quality(mesh_node, out) gives the surface-area cost of the mesh's binary tree as it lies in device memory,
 *    cost = ( sum over the inner nodes of A(stored box) + sum over the leaves of n_tris x A(exact bound of the leaf's triangles) ) / A(root's stored box),
 *    A(lo, hi) = dx dy + dy dz + dz dx; 0 when the root's area is 0 or not finite,
 * summed on the device in a fixed order (the same tree gives the same bits on every device and in every run):
 *    out[0] the cost now; out[1] the cost as built - measured when the tree was last built, by a full commit or by a rebuild in place
 *    (recorded by the first ft_scene_commit_deformed after a full commit before it rewrites anything, or by an earlier query);
 *    out[2] 1 if the tree was built on the device and can be rebuilt in place, else 0; out[3] rebuilds in place since the last full commit.
 *    FT_ERR_INVALID for a null context or out, an invalid handle or a node that is not a bspMesh node; FT_ERR_STATE without a held commit
 *    (or for a node that is not part of it); FT_ERR_UNSUPPORTED for a mesh without a BVH (depth above 0, or fewer than 8 triangles);
 *    FT_ERR_NO_DEVICE on a host-only context, in this order.  A node placed under several transforms has one tree and one answer.  The call
 *    blocks and retires queued frames first; a multi-device context answers from its first device.
 * out[0] / out[1] is the ratio a host judges by; which ratio is tolerable is the host's choice (DESIGN.md 16.1 lists the ratios of the
 * test catalogue: a jitter of 1 % stays below 1.25, a permutation of the triangles reaches 5 - 900).  The remedy needs no full commit:
 * with "refit_rebuild_percent" = P > 0, ft_scene_commit_deformed measures every edited, device-built mesh after its refit and, where
 * cost now x 100 > P x cost as built, runs the device builder again for that one mesh into the ranges its tree already occupies, from
 * the records the refit has just written.  Mesh and leaf indices, the tree's root, the 4-wide root and the coarse range do not move,
 * the temporal accumulation stays open, the pose counter stays, other meshes are not touched, and the results are still those of a fresh
 * context, bit for bit (the argument above holds for any tree).  The rebuilt tree's cost becomes the cost as built.  The decision is taken
 * on the first device of a multi-device context and carried out on all of them.  A rebuild the builder refuses (a tree deeper than 40
 * levels) fails the call with FT_ERR_BUILD, the context then holds no commit, and ft_scene_commit recovers.  ft_get_commit_times: [1]
 * includes the cost kernels and the rebuilds, [3] becomes the larger of its old value and the rebuilt trees' heights.  Trees built by the
 * host ("bvh_builder" 0; meshes below 4096 triangles under the default 2) are measured and never rebuilt in place: a host that wants
 * rebuilds for small meshes sets "bvh_builder" to 1 or 3.  tools/refit_rate.py measures the k_primary ratio of a refit tree to a fresh
 * one beside the cost ratio, and what a commit that rebuilds costs.
 * A host that never calls these functions gets bit-identical results from everything else.
 * Device memory: 8 bytes per BspNode, 52 per BspLeaf and 4 per 4-wide node of the scene from the first refit on, plus the vertices of
 * the meshes being refit. */
int32_t ft_sg_set_mesh_triangles(ft_context* ctx, ft_node node, const double* tris, int64_t n_tris);
int32_t ft_scene_commit_deformed(ft_context* ctx);
int32_t ft_scene_tree_quality(ft_context* ctx, ft_node mesh_node, double out[4]);
/* ---- morph targets: vertices blended on the device before the refit --------------------------- */
/* A mesh whose poses are blends of a few key shapes needs no vertices from the host: the key shapes stay in device memory, a frame sets
 * K weights, and ft_scene_commit_deformed makes the vertices where the refit reads them.
 * ft_sg_set_mesh_targets(mesh, targets, n_targets, n_tris): targets = n_targets x n_tris x 9 doubles, each target laid out as
 * ft_sg_bsp_mesh's tris (absolute positions), copied.  The base B is the node's triangles as they stand at the call (from ft_sg_bsp_mesh,
 * the last ft_sg_set_mesh_triangles or the last ft_sg_set_mesh_weights); the library keeps B and per target the deltas D_k = T_k - B, one
 * rounded subtraction per coordinate.  n_targets = 0 removes the targets (targets may then be null).  Not a structural change, and nothing
 * is marked deformed: the vertices stay what they were.  FT_ERR_INVALID, with nothing changed, for a null context, an invalid handle, a
 * node that is not a bspMesh node, an n_tris that differs from the node's count, n_targets outside 0 .. FT_MAX_MORPH_TARGETS, or null
 * targets with n_targets > 0.
 * ft_sg_set_mesh_weights(mesh, weights, n_weights) declares the node's vertices to be V = blend(B, D, w), per coordinate in IEEE double:
 *     acc = B;  for k = 0 .. K-1 in order:  p = w_k * D_k (one rounded product);  acc = acc + p (one rounded sum, never fused);  V = acc
 * with every term evaluated, zero weights included.  It marks the node as ft_sg_set_mesh_triangles does, leaves the scene uncommitted and
 * is not structural.  FT_ERR_INVALID, with nothing changed, for a null context, an invalid handle, a node that is not a bspMesh node or
 * has no targets, an n_weights that differs from the node's target count, null weights or a weight that is not finite.
 * ft_sg_set_mesh_triangles on a node with targets sets explicit vertices for the next commit; base and deltas stay for a later
 * ft_sg_set_mesh_weights.
 * The promise: ft_sg_set_mesh_weights(node, w) followed by any commit gives every bit that ft_sg_set_mesh_triangles(node, V) followed by
 * the same commit gives - frames, ft_stats (times aside), ft_render_aov, the ft_debug_* ray queries, ft_debug_mesh_trees - so everything
 * said under "deforming meshes" above holds unchanged: the refusals, the open temporal accumulation, "temporal_follow_deformed",
 * "refit_rebuild_percent", "deform_light_space", "light_space_retree", several devices.
 * ft_scene_commit_deformed, for every edited mesh that weights describe, on a device context with "morph_on_device" = 1 (the default):
 * uploads base and deltas to every device on first use or after a new ft_sg_set_mesh_targets ((K + 1) x n_tris x 72 bytes per device, kept
 * until the targets change, ft_scene_clear or ft_destroy; inside ft_get_commit_times [2]); blends the vertices on every device into the buffer the
 * refit reads; reduces bounds, extent and finiteness on the context's first device, bit for bit what the host's pass gives (a zero bound
 * has the sign of the first zero in list order) and reads them back, one small copy; under "deform_light_space" reduces each pair's R
 * there as well; then goes on as for ft_sg_set_mesh_triangles, uploading only the vertices of the meshes edited that way in the same call.
 * The blend writes only that buffer, which no frame reads: a refusal (a non-finite result, bounds that change which items have bounds,
 * depth above 0 - the last before any kernel runs) leaves the old commit renderable, as there.  With the option at 0, on a host-only
 * context, and in every other commit (ft_scene_commit, ft_scene_commit_moved with vertices pending) the host blends V by the formula when
 * the vertices are needed.  ft_get_commit_times: [0] host, [1] blend, scan, R and refit kernels with their readbacks, [2] uploads.
 * ft_debug_morph(mesh, counts, scan), for tests and tools: counts[0] = ft_scene_commit_deformed calls since ft_create that blended at
 * least one mesh on the device, counts[1] = meshes blended on the device in the last ft_scene_commit_deformed, counts[2] = meshes whose
 * blend the host made in it, counts[3] = bytes of base and deltas resident per device for `mesh`; scan[0..5] = the bounds that call used
 * for `mesh`, scan[6] the extent, scan[7] = 1.0 where they came from the device, else 0.0 (all 0 when the call did not edit `mesh`).
 * FT_ERR_INVALID for a null context or pointer, an invalid handle or a node that is not a bspMesh node.
 * What it is worth (MI355X, the 69.6 K-face mesh, nothing in flight, tools/morph_rate.py): a pose by weights
 * takes 0.31 / 0.32 / 0.34 ms at K = 1 / 4 / 16 for the whole step (set the weights, ft_scene_commit_deformed), against 1.43 / 2.08 / 4.82 ms for a host that
 * blends the pose in numpy and hands it to ft_sg_set_mesh_triangles; of the commit, [0] goes from 0.54 ms to under 0.01 ms, [2] from 0.14 to 0.03 ms and
 * [1] from 0.23 to 0.29 ms (blend, scan and readback), whatever K.  With "morph_on_device" 0 the library's host blend makes [0] 0.95 / 1.35 / 5.59 ms.
 * The first pose after ft_sg_set_mesh_targets uploads base and deltas: 0.66 / 0.86 / 4.09 ms in [2]. */
#define FT_MAX_MORPH_TARGETS 16
int32_t ft_sg_set_mesh_targets(ft_context* ctx, ft_node mesh, const double* targets, int32_t n_targets, int64_t n_tris);
int32_t ft_sg_set_mesh_weights(ft_context* ctx, ft_node mesh, const double* weights, int32_t n_weights);
int32_t ft_debug_morph(ft_context* ctx, ft_node mesh, int64_t counts[4], double scan[8]);
/* ---- skinning: vertices posed from a bone palette on the device before the refit ------------- */
/* A bspMesh node has a shape U: its explicit vertices (ft_sg_bsp_mesh, ft_sg_set_mesh_triangles) or blend(B, D, w) once
 * ft_sg_set_mesh_weights has been called.  A node may also carry a skin and a palette; its vertices are then V = skin(U, palette), and
 * ft_scene_commit_deformed makes them where the refit reads them.
 * ft_sg_set_mesh_skin(mesh, bone_index, bone_weight, influences, n_tris): bone_index and bone_weight are n_tris x 3 x influences values,
 * corner-major (triangle, corner a / b / c, slot), copied; influences = J in 1 .. FT_MAX_SKIN_INFLUENCES.  The call attaches the skin and
 * removes any palette.  Not a structural change and no edit: the vertices stay U and nothing is marked deformed - unless a palette was in
 * force, which the call removes: the node is then marked deformed.  influences = 0 removes skin and palette (the pointers may be null).
 * FT_ERR_INVALID, with nothing changed, for a null context, an invalid handle, a node that is not a bspMesh node, an n_tris that differs
 * from the node's count, influences outside 0 .. 4, null arrays with influences > 0, an index outside 0 .. FT_MAX_SKIN_BONES - 1 or a
 * weight that is not finite.  Weights are used as given: the library does not normalise them.
 * ft_sg_set_mesh_bones(mesh, matrices, n_bones): matrices = n_bones x 12 doubles, the rows of a 3x4 affine matrix per bone, copied.  The
 * call declares V = skin(U, palette), marks the node as ft_sg_set_mesh_triangles does, leaves the scene uncommitted and is not structural.
 * n_bones = 0 removes the palette (matrices may be null): V is U again and the node is marked deformed.  FT_ERR_INVALID, with nothing
 * changed, for the node checks above, a node without a skin, n_bones outside 0 .. FT_MAX_SKIN_BONES, 0 < n_bones <= the largest index the
 * skin uses, null matrices with n_bones > 0 or an entry that is not finite.
 * The formula, per corner with shape position (x, y, z), in IEEE double, every product and every sum rounded once and never fused:
 *     for j = 0 .. J-1 in order, b = index[corner][j], M = palette[b], wj = weight[corner][j]:
 *         t_i = ((M[i][0]*x + M[i][1]*y) + M[i][2]*z) + M[i][3]     (i = 0, 1, 2; left to right)
 *         q_i = wj * t_i
 *         acc_i = (j == 0) ? q_i : acc_i + q_i
 *     V = acc
 * Every influence is evaluated, zero weights included.  Two corners with bitwise equal shape positions, indices and weights therefore come
 * out bitwise equal: a mesh that is welded in its rest pose stays welded in every pose.
 * The other setters: ft_sg_set_mesh_triangles and ft_sg_set_mesh_weights on a node with a palette change U and the palette stays in force;
 * ft_sg_set_mesh_targets on such a node takes U as its base, not the skinned V (blend the shape, then skin it).  Nodes without a skin
 * behave exactly as before.
 * The promise: ft_sg_set_mesh_bones(node, P) followed by any commit gives every bit that ft_sg_set_mesh_triangles(node, V) gives on a twin
 * node without a skin, followed by the same commit - frames, ft_stats (times aside), ft_render_aov, the ft_debug_* ray queries,
 * ft_debug_mesh_trees - so everything said under "deforming meshes" above holds unchanged: the refusals (depth above 0, a non-finite V,
 * bounds that change which items have bounds), the open temporal accumulation, "temporal_follow_deformed", "refit_rebuild_percent",
 * "deform_light_space", "light_space_retree", several devices.
 * ft_scene_commit_deformed, for every edited mesh with a palette, on a device context with "skin_on_device" = 1 (the default), where U is
 * explicit or blended on the device in the same call ("morph_on_device" 1): keeps per device the index words (4 bytes per corner), the
 * weights (J x 8 bytes per corner) and, where U is explicit, the rest shape (72 bytes per triangle; uploaded on first use and after an
 * ft_sg_set_mesh_triangles), until the skin is removed, ft_scene_clear or ft_destroy; uploads the palette (n_bones x 96 bytes, at most 24 KiB)
 * per pose, inside ft_get_commit_times [2]; runs k_skin (ft_skin.hip) on every device, in place behind the blend or from the rest shape;
 * reduces bounds, extent, finiteness and, under "deform_light_space", each pair's R on the context's first device with the morph
 * kernels, and goes on as for morph targets: a refused call has written only that buffer and leaves the old commit renderable.  With the
 * option at 0, on a host-only context, with a weight-driven U under "morph_on_device" 0, and in every other commit the host makes V by
 * the formula when the vertices are needed.
 * ft_debug_skin(mesh, counts), for tests and tools: counts[0] = ft_scene_commit_deformed calls since ft_create that skinned at least one
 * mesh on the device, counts[1] = meshes skinned on the device in the last ft_scene_commit_deformed, counts[2] = meshes whose skin the
 * host made in it, counts[3] = bytes resident per device for `mesh` (rest shape, indices, weights, palette).  ft_debug_morph's scan[] keeps
 * reporting the bounds the call used, scan[7] = 1 when they came from the device, skinned or not; its counters count morph blends only.
 * FT_ERR_INVALID for a null context or pointer, an invalid handle or a node that is not a bspMesh node.
 * What it is worth (MI355X, the 69.6 K-face mesh, nothing in flight, tools/skin_rate.py): the commit of a pose set by bones takes
 * 0.33 ms ([0] 0.004, [1] 0.28, [2] 0.05 ms) whatever J and the bone count, against 0.98 ms ([0] 0.55, [1] 0.25, [2] 0.18 ms) for the same
 * vertices handed to ft_sg_set_mesh_triangles; k_skin itself runs 7 - 10 microseconds.  The whole step (make the palette, set it, commit) takes
 * 0.35 / 0.56 / 1.22 ms at J = 4 with 4 / 64 / 256 bones - the difference is the tool's own palette loop - against 31.5 / 32.6 / 32.3 ms for a host
 * that skins in numpy and 2.06 / 2.26 / 2.93 ms with "skin_on_device" 0 (the library's host skin in [0]: 0.93 ms at J = 1, 1.6 ms at J = 4).
 * The device route's whole step lies below the numpy host's by more than both spreads at every row measured (J = 1 and 4; 4, 64 and 256
 * bones; under "deform_light_space"; over morph targets), so the default is 1.  The first pose after ft_sg_set_mesh_skin uploads the
 * resident arrays: 0.6 - 2.3 ms in [2]. */
#define FT_MAX_SKIN_BONES 256
#define FT_MAX_SKIN_INFLUENCES 4
int32_t ft_sg_set_mesh_skin(ft_context* ctx, ft_node mesh, const int32_t* bone_index, const double* bone_weight, int32_t influences, int64_t n_tris);
int32_t ft_sg_set_mesh_bones(ft_context* ctx, ft_node mesh, const double* matrices, int32_t n_bones);
int32_t ft_debug_skin(ft_context* ctx, ft_node mesh, int64_t counts[4]);
/* ---- dual-quaternion skinning: a second kind of palette for the same skin ---------------------- */
/* Linear-blend skinning collapses the surface between two bones that twist against each other (the blended matrix is no rotation).  A
 * node that carries a skin (ft_sg_set_mesh_skin, unchanged) may instead be posed by a palette of unit dual quaternions (Kavan et al.
 * 2008), whose normalised blend is always a rigid motion.
 * ft_sg_set_mesh_bones_dq(mesh, dual_quaternions, n_bones): dual_quaternions = n_bones x 8 doubles, copied; per bone the real part
 * (rw, rx, ry, rz), then the dual part (dw, dx, dy, dz).  The rigid motion "rotate by the unit quaternion r, then translate by t" has
 * real part r and dual part 0.5 * (0, t) (x) r (quaternion product).  Scale and shear cannot be expressed.  The call declares
 * V = skin_dq(U, palette), marks the node as ft_sg_set_mesh_triangles does, leaves the scene uncommitted and is not structural.
 * A node holds at most one palette: ft_sg_set_mesh_bones_dq replaces a matrix palette, ft_sg_set_mesh_bones replaces a dual-quaternion
 * one, n_bones = 0 through either call removes whichever palette is in force (the pointer may be null; V is U again and the node is
 * marked deformed), and ft_sg_set_mesh_skin removes either kind.  Nodes that never see this call behave exactly as before.
 * FT_ERR_INVALID, with nothing changed, for the cases of ft_sg_set_mesh_bones: a null context, an invalid handle, a node that is not a
 * bspMesh node, a node without a skin, n_bones outside 0 .. FT_MAX_SKIN_BONES, 0 < n_bones <= the largest index the skin uses, null
 * data with n_bones > 0 or an entry that is not finite.  The library does not normalise the input and does not check unit length; the
 * blend is normalised, as the formula says.
 * The formula, per corner with shape position p = (x, y, z), in IEEE double; every product, sum, difference, square root and division is
 * rounded once and never fused, sums run left to right as written, negation and multiplication by 2 are exact:
 *     R0 = real part of palette[index[corner][0]]
 *     for j = 0 .. J-1 in order, D = palette[index[corner][j]] (8 values), wj = weight[corner][j]:
 *         if j == 0:  ws = wj
 *         else:       g = ((D.rw*R0.rw + D.rx*R0.rx) + D.ry*R0.ry) + D.rz*R0.rz
 *                     ws = (g < 0) ? -wj : wj          (antipodality: D and -D are the same motion; a NaN g does not negate)
 *         q_k = ws * D_k                                (k = 0 .. 7)
 *         a_k = (j == 0) ? q_k : a_k + q_k
 *     n2 = ((a_0*a_0 + a_1*a_1) + a_2*a_2) + a_3*a_3;   n = sqrt(n2);   s = 1.0 / n;   u_k = a_k * s   (k = 0 .. 7)
 *     w = u_0, v = (u_1, u_2, u_3), e = u_4, f = (u_5, u_6, u_7)
 *     cross(a, b)_x = a_y*b_z - a_z*b_y   (two products, one difference; y and z cyclic)
 *     c_i = cross(v, p)_i + w*p_i
 *     h   = cross(v, c)
 *     m_i = (w*f_i - e*v_i) + cross(v, f)_i
 *     V_i = (p_i + 2*h_i) + 2*m_i
 * Every influence is evaluated, zero weights included.  Two corners with bitwise equal shape positions, indices and weights come out
 * bitwise equal: a mesh that is welded in its rest pose stays welded in every pose.  A blend whose real part is zero gives s = inf and a
 * NaN V: ft_scene_commit_deformed then refuses the call ("an edited mesh holds a non-finite coordinate") and leaves the old commit
 * renderable, as for any non-finite vertex.
 * Everything else is as said under "skinning" for matrices, with V = skin_dq(U, palette): the other setters (ft_sg_set_mesh_triangles and
 * ft_sg_set_mesh_weights change U and the palette stays in force; ft_sg_set_mesh_targets takes U as its base - blend the shape, then skin
 * it), the promise (ft_sg_set_mesh_bones_dq(node, P) followed by any commit gives every bit that ft_sg_set_mesh_triangles(node, V) gives
 * on a twin node without a skin followed by the same commit - frames, ft_stats (times aside), ft_render_aov, the ft_debug_* ray queries,
 * ft_debug_mesh_trees - hence the refusals, the open temporal accumulation, "temporal_follow_deformed", "refit_rebuild_percent",
 * "deform_light_space", "light_space_retree", morph targets under the skin, several devices), and the device route of
 * ft_scene_commit_deformed under exactly the same conditions ("skin_on_device" 1, a device context, U explicit or blended on the device in
 * the same call): the index words, the weights and the rest shape stay resident as they are - switching the palette kind uploads none of
 * them again - the palette (n_bones x 64 bytes, at most 16 KiB) is uploaded per pose inside ft_get_commit_times [2], and k_skin_dq
 * (ft_skin.hip) runs where k_skin runs for matrices.  With the option at 0, on a host-only context and in every other commit the host
 * makes V by the formula when the vertices are needed.
 * ft_debug_skin_dq(mesh, counts), for tests and tools: counts[0] = ft_scene_commit_deformed calls since ft_create that posed at least one
 * mesh with k_skin_dq on the device, counts[1] = meshes posed that way in the last ft_scene_commit_deformed, counts[2] = meshes whose
 * dual-quaternion skin the host made in it, counts[3] = the palette kind in force for `mesh` (0 none, 1 matrices, 2 dual quaternions).
 * ft_debug_skin keeps its meaning for matrix palettes - its first three counters count matrix skins alone - and its counts[3] counts
 * n_bones x 64 bytes for a dual-quaternion palette where it counts n_bones x 96 for matrices.  FT_ERR_INVALID for a null context or
 * pointer, an invalid handle or a node that is not a bspMesh node.
 * What it is worth (MI355X, the 69.6 K-face mesh, nothing in flight, tools/skin_rate.py --dq): the commit of a pose set by
 * dual quaternions takes 0.33 ms ([0] 0.004, [1] 0.28, [2] 0.05 ms) whatever J and the bone count, as for matrices; k_skin_dq itself runs
 * 6.5 - 8.8 microseconds, no slower than k_skin (it is bound by memory, and its palette is a third smaller).  The whole step (make the
 * palette, set it, commit) takes 0.40 / 0.45 / 0.56 ms at J = 4 with 4 / 64 / 256 bones, against 32.3 / 32.4 / 32.3 ms for a host that
 * skins in numpy and 5.09 / 5.13 / 5.23 ms with "skin_on_device" 0 (the library's host skin in [0]: 2.4 ms at J = 1, 4.6 ms at J = 4).
 * The device route's whole step lies below the numpy host's by more than both spreads at every row measured (J = 1 and 4; 4, 64 and 256
 * bones), so the default stays 1. */
int32_t ft_sg_set_mesh_bones_dq(ft_context* ctx, ft_node mesh, const double* dual_quaternions, int32_t n_bones);
int32_t ft_debug_skin_dq(ft_context* ctx, ft_node mesh, int64_t counts[4]);
/* ---- moving lights ----------------------------------------------------------------------------- */
/* ft_scene_set_directional / _soft_directional / _positional + ft_scene_commit_lights change the lights of a committed scene without a
 * flatten, without a BVH build and without ending ft_temporal_*.
 * The setters replace the values of the light with index `light` (the order of the ft_scene_add_* calls) with the arithmetic of the
 * ft_scene_add_* of its kind: directions are normalised as there, everything else is copied.  FT_ERR_INVALID, with nothing changed, for
 * a null context or pointer, an index out of range or a light of another kind.  The kind of a light and a soft light's sample count
 * cannot be set: they decide the kernel variant, the shadow rays per hit and the byte packing, and changing them stays a structural
 * change (ft_scene_clear / ft_scene_add_*).  Like ft_sg_set_transform a setter leaves the scene uncommitted and is not a structural
 * change; a later plain ft_scene_commit or ft_scene_commit_moved gives what a fresh graph with the new lights gives.
 * ft_scene_commit_lights commits a graph in which only light values changed since the last successful commit:
 *  - FT_ERR_STATE, and nothing done, unless the context holds a successful commit and no structural change was made since (the rule of
 *    ft_scene_commit_moved), or while an ft_sg_set_transform is pending (ft_scene_commit_moved first), an ft_sg_set_mesh_triangles is
 *    pending (ft_scene_commit_deformed first) or an ft_set_option that needs a new ft_scene_commit.  ft_scene_commit_deformed in turn
 *    returns FT_ERR_STATE while a light setter is pending (ft_scene_commit_lights first).
 *  - On success every later call - ft_render*, the queued forms, ft_progressive_*, ft_render_aov, ft_denoise, ft_temporal_*, the
 *    ft_debug_* ray queries - gives what it gives on a fresh context whose graph was built with the new lights and committed with
 *    ft_scene_commit, bit for bit, frames and counters.
 *  - It ends a progressive accumulation, retires queued frames first (a frame queued before the call shows the old lights), leaves the
 *    temporal accumulation OPEN and does not advance the pose counter.  On a multi-device context every device rewrites its own copy.
 *    A host-only context checks the same rules and then runs the full host commit.
 *  - ft_get_commit_times: [0] host work, [1] the refit and grid kernels with their readbacks, [2] uploads, [3] unchanged.  On a multi-device
 *    context the first device takes the decisions that need a readback (a grid's resolution, "no grid"); all devices carry them out.
 * "light_space_shadows" 1 / 2: for every (mesh leaf, directional light) pair that had a tree at the last full commit and whose direction
 * changed, the pair record (frame, slack) is derived again on the host with the full commit's arithmetic (one rule is stricter: where the
 * full commit tests that the projected bounds are finite, this call requires the mesh's extent about its centre, R, below 2e29, which
 * implies it; a pair with R from 2e29 on gets no tree here and its rays walk the BVH - the same bits), and on the device
 * (ft_lightspace.hip) the tree is refit - its topology and leaf records stay, every box is projected again into the new frame in FP64 and
 * rounded outward - and, with option 2, the grid is built again by the full commit's rules (the same entry boxes, attempt loop, cell
 * function, caps and order within a cell; two builds of the same input are byte-identical).  Any structure that holds every triangle in
 * conservative boxes gives the BVH walk's bits, hence the bit-identity above.  Only a direction that changes touches a pair: colours and the
 * other kinds of light are an upload alone.  A direction that is zero, not finite or ill-conditioned in the leaf's model space gets root
 * INT32_MIN and no grid (its rays walk the BVH) until a later call gives it a usable direction again; a pair that had no tree at the last
 * full commit, and the pairs ft_scene_commit_deformed stripped, stay without one until the next full commit; a light back at the direction
 * of the last full commit gets that commit's record and grid back (unless its mesh has been deformed under "deform_light_space" since).  The grids built since the full commit lie behind that commit's
 * arrays in freshly sized arrays that every call which turns a light lays out anew, so repeated calls do not grow memory; the bytes the
 * cap (256 MiB) counts include the full commit's arrays whole.  Once a call has rewritten anything ft_debug_light_space answers from device
 * memory.
 * Cost: a call in which no direction changes is two uploads.  A call that turns ANY light refits the trees of the pairs that turned and
 * builds the grid of EVERY pair whose direction is not the last full commit's, the ones that did not turn in this call included: the
 * region behind the commit's arrays is laid out anew as a whole, so that no grid is moved.  With several directional lights or mesh
 * leaves the cost therefore grows with the pairs that have turned since the full commit, not with the ones that turn now; the figures
 * below are for one light over one mesh.
 * Tree quality: the refit tree is the OLD direction's tree in the new frame - its leaves hold triangles that were neighbours in the old
 * projection - so its rectangles overlap more the further the light has turned from the direction of the last full commit, and the waves
 * the grid hands to the tree (those that cover more than four cells) slow down while the results stay exact.  Measured on a 69.6 K-face
 * mesh at 1920 x 1080 x 16: k_primary after a turn of 1 degree costs what a full commit's costs, 10 degrees 1.41 x (1.10 x
 * option 0), 45 degrees 6.7 x, 90 degrees 15 x, 180 degrees 1.46 x.  From about 10 degrees of accumulated turn on, a host that
 * renders many frames under the new direction should pay for a full ft_scene_commit (75 - 85 ms there, against 2 ms for this call), which
 * builds a fresh tree; the library does not decide this by itself.
 * What follows a surface is its history, not its shading: light that moves over a surface is averaged by ft_temporal_accumulate as noise
 * is, max_history bounding how long it lingers - unless the neighbourhood clamp is on (ft_temporal_set_clamp), which pulls such history
 * to the colours the current frame shows around the pixel and shortens it.
 * A host that never calls these functions gets bit-identical results from everything else.
 * Device memory: 4 bytes per 4-wide node of the trees that can be refit, the grids built since the full commit, and while a call runs
 * 20 bytes per triangle and 4 per cell of every pair whose grid is built (kept from call to call) and 8 per cell and 4 per entry of the
 * largest grid.
 * "light_space_retree" 1: the cure for that decay short of a full commit.  Every pair whose tree a call would refit - it has a usable
 * frame and R < 2e29, and its direction changed in this call, or (ft_scene_commit_deformed under "deform_light_space") its mesh was edited
 * in this call - gets a NEW topology instead, built on the device from the current projection, and that tree is then boxed by the same
 * refit pass.  The rule: the pair's n triangles are keyed by the Morton code of the centre of their (u, v) rectangle (16 bits per axis over
 * [-R, R], u in the even bits), sorted by it (stable, so equal codes keep the list order), and the leaf records are copied in that order
 * into the run of n records the pair's tree has always had; over the sorted positions stands a tree that depends on n alone - a binary
 * tree cut at the middle position down to leaves of 2 .. 4, two binary levels per 4-wide node as the host builder collapses them, at most
 * 9 wide levels for the 2^20 triangles a pair may have, so the walk holds at most 27 of its 64 pending entries.  The nodes live in a block of
 * N(n) nodes per pair that the first such call lays out behind the full commit's nodes, in pair order, while the 256 MiB cap allows (a
 * pair whose block does not fit is refit as before, for good); the grids lie behind the blocks from then on, and ft_debug_light_space
 * follows the new sizes.  Everything else in the call is unchanged: pair records, grids, edge records, what the call ends and leaves open,
 * and frames and counters are a fresh context's, bit for bit.  A retreed pair stays retreed until the next full commit: turning the option
 * off later refits it over the new topology, and - as for a pair deformed under "deform_light_space" - a light back at the direction of
 * the last full commit does NOT get that commit's record and grid back, because that commit's tree leads to leaf records that have been
 * sorted anew; it gets a derived record and a rebuilt grid.  A pair that is unusable in a call is not retreed in it.  On a multi-device
 * context every device runs the same deterministic passes.  Device memory: 96 bytes per node of the blocks, about 0.3 n nodes for a pair of
 * n triangles, and 12 bytes per triangle of the largest pair plus the sort's scratch while a call runs (kept from call to call).  Measured
 * on the 69.6 K-face mesh above: the call costs what it costs without the option (1.4 ms against 1.4; 2.4 against 2.1 for a deformed
 * commit), and k_primary stays 1.04 - 1.13 x a fresh full commit's at every turn from 1 to 180 degrees and along 16 steps of a twist, where the refit
 * reaches 7.3 x at 45 degrees, 15 x at 90 and 2.6 x after 16 twist steps.  It pays over the refit from about 10 degrees of turn or 4 twist steps on; at
 * 1 degree it is 4 - 5 % slower than the refit, because a median tree over a Morton order is not as good as the full commit's surface-area tree - by
 * the same 4 - 13 % it stays behind a fresh commit, and at 45 degrees it is 8 % slower than "light_space_shadows" 0 on this mesh, which a fresh
 * commit's tree is not.  Hence the default 0: set it where lights swing far or meshes bend far between full commits. */
int32_t ft_scene_set_directional(ft_context* ctx, int32_t light, const double dir[3], const double colour[3]);
int32_t ft_scene_set_soft_directional(ft_context* ctx, int32_t light, const double dir[3], double scatter_rad, const double colour[3]);
int32_t ft_scene_set_positional(ft_context* ctx, int32_t light, const double pos[3], const double falloff[3], const double colour[3]);
int32_t ft_scene_commit_lights(ft_context* ctx);
/* ---- queued pose and light commits ------------------------------------------------------------- */
/* ft_scene_commit_moved_enqueue / ft_scene_commit_lights_enqueue: the two cheap commits without the drain, so that a host that moves an
 * object or a light every frame keeps its frames in flight (ft_render_enqueue*, ft_temporal_enqueue).  No kernel is added: the work is
 * host-side.
 * Each call has exactly the contract of its blocking twin - ft_scene_commit_moved as it behaves under "moved_in_place" 1, whatever that
 * option says, and ft_scene_commit_lights: the FT_ERR_STATE / FT_ERR_INVALID rules in their order, the progressive accumulation ended, the
 * temporal one left open, the pose counter advanced by the moved call only, no kept classification matched afterwards - with two differences:
 *  1. Nothing queued is retired and no stream is drained.  Frames and temporal calls queued BEFORE the call show the old poses or lights,
 *     the copies of ft_render_enqueue_into and the host_out of ft_temporal_enqueue included; everything queued or run AFTER it - ft_render*,
 *     the queued forms, ft_progressive_*, ft_render_aov, ft_denoise, ft_temporal_*, the ft_debug_* ray queries - shows the new ones, and is
 *     bit for bit what a fresh context built with the new values and committed with ft_scene_commit gives: frames, ft_stats counters (times
 *     and the hint-dependent n_launches aside: the level hint restarts as after every commit), ft_render_aov planes, ft_debug_leaf_matrices.
 *  2. A call that cannot be queued takes its blocking twin's path, with the twin's bits and the twin's draining; ft_debug_pose_queue tells
 *     that it did and why.  Nothing is ever approximated.
 * A call is queued when the context has a device; nothing is pending that the twin hands to a full commit (a light setter, an
 * ft_sg_set_mesh_triangles or a commit-time option, for the moved call); the re-flatten differs from the held scene in poses alone (moved
 * call, as under "moved_in_place"); and no light-space pair changes: for the moved call no (mesh leaf, directional light) pair's frame
 * differs from its record, for the lights call no directional light that has such a pair changes direction.  (A changed pair means refit
 * and grid kernels with readbacks that rewrite arrays the frames in flight still read.)  So translations of anything, any move of
 * primitives and CSG items, any move at all under "light_space_shadows" 0, colours, point lights, a soft light's scatter and the
 * directions of lights without pairs are queued; a mesh leaf that turns under a directional light with "light_space_shadows" 1 / 2 is not.
 * Pose sets.  What depends on a pose or a light value - the leaves, their m2w, the items' cull records and float image, the face
 * directions, the lights - exists in up to 9 copies per device (frame slots 4 + FT_TEMPORAL_QUEUE_DEPTH + 1), made on first need: 224
 * bytes per leaf, 232 per top-level item, 40 per face direction and 96 per light each, and as much page-locked host memory for the
 * upload's source.  A queued call writes a copy that no pending frame or temporal call was given, on a stream of its own that waits for
 * nothing, and the streams that launch scene-reading kernels wait for that upload before their next launch.  Every full commit frees all
 * copies but the first.  A host that never calls these functions has one copy, the scene's own arrays, and gets the launches and bytes it
 * got before.  On a multi-device context every device keeps its own copies.
 * ft_get_commit_times after a queued call: [0] the host's work, [1] exactly 0, [2] the host time to queue the uploads, [3] unchanged.
 * A failed upload leaves the context as a failed ft_scene_commit_moved in place does: uncommitted until ft_scene_commit.
 * Measured (MI355X, 1920 x 1080 x 16, a translation, a commit and a queued RGBA8 frame per step): 0.49 ms per step
 * against 0.80 with the blocking call on the 69.6 K-face mesh (0.29 with no commit at all: a new pose still needs its classification),
 * 3.49 against 4.21 on hollow-sphere (3.48 with no commit). */
int32_t ft_scene_commit_moved_enqueue(ft_context* ctx);
int32_t ft_scene_commit_lights_enqueue(ft_context* ctx);
/* ---- queued deform commits ---------------------------------------------------------------------- */
/* ft_scene_commit_deformed_enqueue: ft_scene_commit_deformed without the drain, so that a host that poses a mesh every frame - set bones
 * or weights, commit, ft_render_enqueue_into - keeps its frames in flight.
 * The call is ft_scene_commit_deformed in every respect - the FT_ERR_STATE rules in their order; the FT_ERR_UNSUPPORTED refusals (depth
 * above 0, a non-finite vertex, bounds that change which items have bounds), after each of which the old commit stays renderable; the
 * progressive accumulation ended, the temporal one left open, the pose counter left; no kept classification matched afterwards; the
 * ft_debug_morph / ft_debug_skin / ft_debug_skin_dq counters - with two differences:
 *  1. Nothing queued is retired and no stream that frames run on is waited for.  Frames and temporal calls queued BEFORE the call show the
 *     old vertices, the copies of ft_render_enqueue_into and the host_out of ft_temporal_enqueue included; everything queued or run AFTER
 *     it is bit for bit what a fresh context built with the new vertices and committed with ft_scene_commit gives: frames, ft_stats
 *     counters (times and the hint-dependent n_launches aside), ft_render_aov planes, the ft_debug_* ray queries, ft_debug_mesh_trees.
 *     The host may wait for the call's own small stream - the readback of the bounds of vertices made on the device, a first-use upload
 *     of a mesh's targets or skin - never for a frame.
 *  2. A call that cannot be queued takes the blocking call's path, bits and draining; ft_debug_deform_queue's out[2] says why:
 *       1  a host-only context;
 *       2  a context over several devices;
 *       3  the first refit since a full commit, which derives the refit's tables, records the trees' costs as built and strips the
 *          light-space pairs: it stays blocking, once;
 *       4  "refit_rebuild_percent" above 0: a rebuild rewrites topology behind a cost readback;
 *       5  "deform_light_space" would give an edited mesh a light-space job, whose arrays are rewritten with readbacks;
 *       6  "temporal_follow_deformed" with an open accumulation that has accumulated: its snapshot reads the records about to be replaced.
 * Every kind of edit is queued: ft_sg_set_mesh_triangles, weights, matrix or dual-quaternion palettes alone or over weights, and their
 * host twins under "morph_on_device" 0 / "skin_on_device" 0.
 * Geometry sets.  What a refit rewrites - the scene's tree nodes (64 bytes each), its triangle records and their sorted copies (72 bytes
 * each), its 4-wide nodes (224 bytes each) and the coarse boxes (24 bytes each), whole arrays - exists in up to 9 copies on the device
 * (frame slots 4 + FT_TEMPORAL_QUEUE_DEPTH + 1), each made on first need by one device-to-device copy: for the 69.6 K-face mesh
 * 10 MB of records per copy, and its nodes.  They are kept apart from the pose sets of the queued pose and light commits: neither kind of call changes which
 * copy of the other kind is live.  A queued call refits into a copy that no pending frame or temporal call was given (the live one
 * when nothing holds it), on a stream of its own that waits for nothing a frame does, after k_refit_carry has brought over the ranges
 * of the meshes the call does not edit where that copy is behind the live one; the streams that launch scene-reading kernels wait
 * for the refit before their next launch.  With every copy held and none left to make, the oldest pending frame or temporal call is
 * retired.  The new leaves and cull records travel as a queued pose commit's do.  Every full commit frees all copies but the first.  A
 * host that never calls this function has one copy, the scene's own arrays, and gets the launches and bytes it got before.
 * ft_get_commit_times after a queued call: [0] the host's work, [1] the blend, skin and scan kernels with the host's wait for their
 * readback (exactly 0 when every edit's vertices came from the host), [2] the host time to queue copies, carry and refit, [3] unchanged.
 * A HIP failure once the refit is being queued leaves the context as a failed ft_scene_commit_deformed does: uncommitted until ft_scene_commit.
 * Measured (MI355X, 1920 x 1080 x 16, a 64-bone palette, a commit and a queued RGBA8 frame per step): 0.87 ms per step
 * against 1.08 with the blocking call on the 69.6 K-face mesh (0.34 with no commit at all: the host still waits for the readback of the
 * new bounds, and a new pose needs its classification), 4.93 against 5.65 on hollow-sphere with a skinned tube. */
int32_t ft_scene_commit_deformed_enqueue(ft_context* ctx);
/* ---- history on deforming meshes ("temporal_follow_deformed") ----------------------------------- */
/* Without the option the history of a deformed mesh survives only where its surface stayed within clause 2's position tolerance.  With
 * ft_set_option("temporal_follow_deformed", 1) the history follows the triangles, as it follows moved leaves:
 * The snapshot.  A successful ft_scene_commit_deformed on the device path copies, before it refits a mesh, the mesh's list-order triangle
 * records (v0, e1, e2: 72 bytes per triangle) as they lie in device memory into a buffer of the temporal accumulation - if the option is
 * 1, an accumulation is open with at least one successful ft_temporal_accumulate behind it, and the mesh holds no snapshot yet.  Only the
 * first commit after an accumulate snapshots a mesh: several deformations between two accumulates compose by construction, as H is the
 * pose at the last accumulate.  Meshes that were not edited get none; a commit refused on the host takes none; the rebuild in place
 * ("refit_rebuild_percent") does not touch list-order records.  The copy is part of ft_get_commit_times [2].  Snapshots are dropped at
 * the end of every successful ft_temporal_accumulate, by ft_temporal_begin and ft_temporal_end, by whatever ends the accumulation (a
 * full commit, ft_scene_clear, the context) and when the option is set to 0; a failed accumulate keeps them.
 * The take-back, in an ft_temporal_accumulate with the option 1, a call behind it and at least one snapshot.  A hit pixel x takes it when
 * its leaf l = leaf(x) is a mesh leaf whose mesh m holds a snapshot and tau = triangle(x) (ft_render_aov's plane) satisfies 0 <= tau < n_m,
 * compared unsigned.  With (a, e1, e2) the live record of triangle tau of m, (a', e1', e2') the snapshot's, W = w2m_cur(l), H = H_l and
 * Wh = Wh_l ("moving rigid objects": the live matrices unless an ft_scene_commit_moved intervened), every sum left to right as written:
 *   if the 18 doubles of the two records are bitwise equal, the pixel takes the path it takes without the option (p and n, or D_l);
 *   q_i = W[i][0] p_0 + W[i][1] p_1 + W[i][2] p_2 + W[i][3];  r = q - a;
 *   d11 = e1.e1, d12 = e1.e2, d22 = e2.e2, r1 = r.e1, r2 = r.e2, det = d11 * d22 - d12 * d12;  if !(det > 0), that path too;
 *   beta = (d22 * r1 - d12 * r2) / det, gamma = (d11 * r2 - d12 * r1) / det;  if either is not finite, that path too;
 *   q'_i = a'_i + beta e1'_i + gamma e2'_i;  pr_i = H[i][0] q'_0 + H[i][1] q'_1 + H[i][2] q'_2 + H[i][3];
 *   g = e1 x e2, g' = e1' x e2';  c_j = W[0][j] g_0 + W[1][j] g_1 + W[2][j] g_2;  s = (n(x).c < 0) ? -1 : 1 (the side of the triangle
 *   the shaders' normal is on);  t_j = Wh[0][j] g'_0 + Wh[1][j] g'_1 + Wh[2][j] g'_2;  nr = s * t * (1 / sqrt(t.t)).
 * Clauses 1 to 3 then use pr and nr wherever they use p(x) and n(x), exactly as for a moved leaf; a non-finite nr fails every tap; clause
 * 2's leaf test is unchanged; clause 6 stores the current p, n, leaf.  For such pixels this replaces the D_l route - it already ends in the
 * history's pose - so a mesh that is both moved and deformed between two accumulates is followed through both.  A triangle that did not
 * change, a pixel on another leaf and a miss pixel get the bits they get without the option.
 * As for moving objects, what follows a triangle is its history, not its shading: light that changes on a bending surface is averaged as
 * noise is (ft_temporal_set_clamp is the remedy here too).  ft_temporal_filter with `demodulate` between a deform and the next accumulate behaves as it does without the option.
 * Device memory: 72 bytes per triangle of each snapshotted mesh until the next accumulate, 280 bytes per leaf and 4 more bytes per pixel
 * of ft_render_aov's window (the triangle plane) in a call that follows. */

/* The per-leaf matrices of the scene the context holds (the last successful commit's; they stay readable while the graph is being
 * edited), for tests: *n_leaves, and into each non-null array 12 doubles per leaf, the rows of the 3x4 model->world (m2w) and
 * world->model (w2m) matrix.  Host-only contexts too.  FT_ERR_STATE without a successful commit. */
int32_t ft_debug_leaf_matrices(ft_context* ctx, int64_t* n_leaves, double* m2w, double* w2m);

/* Closest hit of single rays through the device path (Scene.intersectScene, Scene.fs:118, after
 * Shading.slightOffset is NOT applied): for tests.  Outputs per ray: t, p[3], n[3], material index
 * resolved colour[3]; hit[i] = 0 when the ray misses. */
int32_t ft_debug_closest(ft_context* ctx, const double* origins, const double* dirs, int64_t n,
                         int32_t* hit, double* t, double* p, double* nrm, double* colour);
/* lightIsBocked (Scene.fs:119-121) for single rays. */
int32_t ft_debug_blocked(ft_context* ctx, const double* origins, const double* dirs,
                         const double* max_dist, int64_t n, int32_t* blocked);

/* getColourForRay (Shading.fs:131-139) for single rays through the device path: slightOffset, closest hit, shadow queries, the
 * shaders of Program.fs:59 and up to max_depth reflection bounces, exactly as a frame's samples are shaded.  rgb = n x 3. */
int32_t ft_debug_colour(ft_context* ctx, const double* origins, const double* dirs, int64_t n, int32_t max_depth, double* rgb);

/* Host-logic test hooks (no device work): a context that can build, flatten and BSP-compile a scene
 * but whose render/debug calls fail with FT_ERR_NO_DEVICE; flattened-scene sizes
 * (out = leaves, program words, meshes, bsp nodes, bsp leaves, triangles, csg capacity, stack capacity, top-level items,
 * items with a bounding sphere, 1 if some item is unbounded, distinct face directions or -1);
 * and Triangle.slice (Triangle.fs:24-41) as the BSP builder implements it (9 doubles per triangle,
 * at most 2 triangles per side). */
int32_t ft_create_host_only(ft_context** out);
int32_t ft_debug_scene_info(ft_context* ctx, int64_t out[12]);
int32_t ft_debug_slice(const double p0[3], const double n[3], const double tri[9],
                       double above[18], int32_t* n_above, double below[18], int32_t* n_below);
/* The light-space shadow trees and grids of the committed scene (option "light_space_shadows"; layout in ft_flat.h, kLsPairDoubles):
 * sizes = pair records, nodes, triangle records, leaves; each non-null array receives 16 doubles per record, 24 words per node,
 * 9 doubles per triangle and, per leaf, the index of its first pair record (0xFFFFFFFF = none).  Host-only contexts too. */
int32_t ft_debug_light_space(ft_context* ctx, int64_t sizes[4], double* pairs, uint32_t* nodes, double* tris, uint32_t* leaf_pairs);
/* "light_space_retree" at work, for tests: the pairs of the table ft_scene_commit_lights / ft_scene_commit_deformed keep since the last full
 * commit (*n_pairs; 0 before the first such call).  Each non-null array receives per pair: rows = 8 values - pair record, leaf, light,
 * n_tris, the first of the tree's leaf records in ls_tris (-1: none), 1 if the pair has been retreed, the first node of its block (-1: no
 * block, also before the option's first call) and the block's node count N; R = the pair's extent about its centre as the last call left it.
 * FT_ERR_NO_DEVICE on a host-only context. */
int32_t ft_debug_ls_retree(ft_context* ctx, int64_t* n_pairs, int64_t* rows, double* R);
/* The topology "light_space_retree" gives a pair of n triangles whose leaf records start at ls_first and whose block starts at node
 * first_node, as the host generates it (no context, no device): sizes = nodes N, levels.  Each non-null array receives: child = 4 words per
 * node, numbered from first_node breadth first (>= 0 a node, INT32_MIN empty, otherwise ~(first record << 3 | count)); order = the N nodes
 * by level, deepest level first; levels = per level, deepest first, its offset into order and its count.  FT_ERR_INVALID where n < 5 or an
 * index would not fit its word. */
int32_t ft_debug_ls_topology(int64_t n, int64_t ls_first, int64_t first_node, int64_t sizes[2], uint32_t* child, uint32_t* order, uint32_t* levels);
/* The mesh trees of the committed scene as the kernels walk them (layouts in ft_flat.h), for tests.  A device context copies the arrays
 * back from device memory, so the trees ft_bvh.hip built after the upload are seen; a host-only context hands out the flattened arrays.
 * sizes = BspNode records, BspLeaf records, triangle records, tri_orig entries, tri_src entries, 4-wide nodes, coarse boxes, meshes,
 * device build jobs, the per-lane tree stack capacity, 1 if the arrays came from device memory, 0.  Each non-null array receives
 * 64 bytes per node, 2 words per leaf, 9 doubles per triangle, a word per tri_orig / tri_src entry, 28 doubles per wide node, 6 floats
 * per coarse box, 6 words per mesh (root, bvh_root, n_source_tris, root of the 4-wide tree or INT32_MIN, first coarse box, coarse
 * box count) and 9 words per job (mesh, first_global, n, node_base, leaf_base, tri_base, wide_base, coarse_first, coarse_count). */
int32_t ft_debug_mesh_trees(ft_context* ctx, int64_t sizes[12], void* nodes, uint32_t* bsp_leaves, double* tris, uint32_t* tri_orig, uint32_t* tri_src,
                            double* wide, float* coarse_boxes, int32_t* meshes, uint32_t* jobs);
/* The per-block triangle candidate lists of the last frame queued (option "primary_block_lists"), read back from device memory once
 * everything queued has run, for tests.  sizes = active blocks, entries in use, the mesh leaf the lists are for (-1: that frame was not classified or carried none; the
 * other sizes are then 0), the pool's capacity in entries.  Each non-null array receives: plane = tlx, tly, pw, ph of the frame's image plane
 * (pixel (x, y) under jitter offset (ox, oy) looks through jx = tlx + (x + ox) pw, jy = tly - (y - oy) ph); heads = one word per active block,
 * 0xFFFFFFFF (the block walks the tree) or first entry << 7 | count; pos_block = the block of the frame's pixel list behind each active block;
 * entries = 6 words each: the triangle's record, its list index (tri_orig), and its rectangle x0, x1, y0, y1 in (jx, jy) as floats. */
int32_t ft_debug_block_lists(ft_context* ctx, int64_t sizes[4], double plane[4], uint32_t* heads, uint32_t* pos_block, uint32_t* entries);
/* The edge records of option "edge_cull" as they lie in device memory (written whatever the option says), for tests.  sizes[0] = records of the committed
 * scene's shadow grids: one per triangle record ft_debug_light_space hands out, under the same index, or 0 where the scene carries none; sizes[1] = records of
 * the candidate lists ft_debug_block_lists describes: one per entry in use, under the same index.  Each non-null array receives 9 floats per record: three lines
 * (a, b, c) with a x + b y + c <= 0 at every point of the entry's plane - (u, v) of the pair's frame, (jx, jy) of the image plane - from which a ray can hit the
 * triangle; nine zeros: no edges, the entry is never skipped (also under every record that is not a grid entry).  FT_ERR_NO_DEVICE on a host-only context. */
int32_t ft_debug_edge_records(ft_context* ctx, int64_t sizes[2], float* grid_edges, float* list_edges);
/* "classify_reuse" at work, for tests: counts since ft_create, summed over the context's devices - classifications launched, classifications reused, windows
 * launched, windows not launched because the kept active list ends before them.  FT_ERR_NO_DEVICE on a host-only context. */
int32_t ft_debug_classify_reuse(ft_context* ctx, int64_t out[4]);
/* "moved_in_place" at work, for tests: out[0] = ft_scene_commit_moved calls done in place since ft_create, out[1] = calls that took the full commit, out[2] = why
 * the last call did (0: it did not; 1: the option is off or the context host-only; 2: a light setter, an ft_sg_set_mesh_triangles or a commit-time option was
 * pending; 3: the re-flatten differs from the held scene in more than poses), out[3] = light-space pairs the last call in place refit or retreed.
 * FT_ERR_INVALID for null arguments; works on a host-only context. */
int32_t ft_debug_moved_commits(ft_context* ctx, int64_t out[4]);
/* The queued commits at work, for tests: since ft_create, out[0] = ft_scene_commit_moved_enqueue calls queued without retiring anything, out[1] = calls that
 * took the blocking path, out[2] = why the last call did (0: it was queued; 1: host-only context; 2: a light setter, an ft_sg_set_mesh_triangles or a
 * commit-time option was pending; 3: the re-flatten differs in more than poses; 4: a light-space pair's frame or direction changed), out[3 .. 5] = the same
 * for ft_scene_commit_lights_enqueue, out[6] = pose sets the first device holds (1: the scene's own arrays alone; 0 on a host-only context), out[7] = frames
 * plus temporal calls the host still had pending on the first device when the last of the two calls returned.  FT_ERR_INVALID for null arguments;
 * works on a host-only context, where the queued counts stay 0. */
int32_t ft_debug_pose_queue(ft_context* ctx, int64_t out[8]);
/* The queued deform commits at work, for tests: since ft_create, out[0] = ft_scene_commit_deformed_enqueue calls queued without retiring
 * anything, out[1] = calls that took the blocking path, out[2] = why the last call did (0: it was queued; the reasons are listed with the
 * function), out[3] = geometry sets the first device holds (1: the scene's own arrays alone; 0 on a host-only context), out[4] = frames +
 * temporal calls the host still had pending on the first device when the last call returned, out[5] = frames or temporal calls retired
 * because every set was held, out[6] = mesh ranges k_refit_carry copied between sets in the last call, out[7] = 0. */
int32_t ft_debug_deform_queue(ft_context* ctx, int64_t out[8]);
/* "primary_mesh_kernel" at work, for tests: bounce-0 launches since ft_create, summed over the context's devices - out[0] of k_primary, out[1] of
 * k_primary_mesh.  FT_ERR_NO_DEVICE on a host-only context. */
int32_t ft_debug_primary_kernels(ft_context* ctx, int64_t out[2]);
/* HIP-event time per stage over the last ft_render: index 4 primary (bounce 0 fused: generate + closest + shade), 2 the later
 * bounces (one k_bounce per level; one bracket around them all, or with "timing" = 2 one per level), 3 resolve and 0 the rest (the
 * fill, classification) with "timing" = 2; otherwise 0 = everything that is not bracketed and 3 = 0.  Index 1 is unused. */
int32_t ft_get_kernel_times(ft_context* ctx, double ms[5], int32_t launches[5]);

/* The device ordinals behind a context, in the order given to ft_create (at most `capacity` written); returns how many there are. */
int32_t ft_debug_devices(ft_context* ctx, int32_t* ordinals, int32_t capacity);

/* Image.write's toByte (Image.fs:36): clamp to [0,1], *255, truncate; alpha = 255. */
int32_t ft_quantise_rgba8(const double* rgb, int64_t n_pixels, uint8_t* out_rgba);

#ifdef __cplusplus
}
#endif
#endif

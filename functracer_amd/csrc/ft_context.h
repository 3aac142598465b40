// ft_context.h — private to the C ABI's translation units (ft_capi.cpp, ft_frame.cpp, ft_progressive.cpp, ft_passes.cpp, ft_debug.cpp):
// the context behind include/functracer_hip.h and the few functions that cross those files.
// Reference citations are relative to FuncTracer/ of the reference (antonburger/FuncTracer).
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <condition_variable>
#include <mutex>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/functracer_hip.h"
#include "ft_device.h"
#include "ft_scene.h"

struct DeviceBuf {
    void* p = nullptr; size_t bytes = 0;
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};

struct ft_context;
// The event pair of a feature around kernels of its own on the context's stream (the kernel_ms of the guide passes), created by its first use.
struct TimedLaunch {
    hipEvent_t ev[2] = {};
    // Records, runs `launch`, records again; behind(), if given, then queues what is not timed; the stream is drained and the bracket's time added to `ms`.
    template <class Launch, class Behind> int32_t run(ft_context* c, double& ms, Launch&& launch, Behind&& behind);
    template <class Launch> int32_t run(ft_context* c, double& ms, Launch&& launch) { return run(c, ms, launch, [] { return (int32_t)FT_OK; }); }
    void release() { for (hipEvent_t& e : ev) if (e) { (void)hipEventDestroy(e); e = nullptr; } }
};

// Stage indices of ft_get_kernel_times.
enum { kStageOther = 0, kStageClosest = 1, kStageShade = 2, kStageResolve = 3, kStagePrimary = 4, kStages = 5 };
// What a frame copies back when it retires: FrameCounters from `stats` to its end.
static_assert(sizeof(ftk::FrameCounters) % 16 == 0 && offsetof(ftk::RenderCounters, ref_equiv) == 32, "the hand-over at the end of a frame copies words and clears 16 bytes at a time");

// One host thread per extra device of a multi-device context, alive as long as the context: every frame hands each of them its share
// (round 2 created and joined a std::thread per device per frame - the same order of time as a device's share of a 4K frame).
struct DeviceWorker {
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    std::function<void()> job;
    bool has_job = false, done = true, quit = false;
    void start() {
        th = std::thread([this] {
            std::unique_lock<std::mutex> lk(m);
            for (;;) {
                cv.wait(lk, [this] { return has_job || quit; });
                if (quit) return;
                std::function<void()> fn = std::move(job);
                has_job = false;
                lk.unlock();
                fn();
                lk.lock();
                done = true;
                cv.notify_all();
            }
        });
    }
    void post(std::function<void()> fn) { std::lock_guard<std::mutex> lk(m); job = std::move(fn); has_job = true; done = false; cv.notify_all(); }
    void wait() { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [this] { return done; }); }
    void stop() { { std::lock_guard<std::mutex> lk(m); quit = true; cv.notify_all(); } if (th.joinable()) th.join(); }
};

constexpr int64_t kDeviceBvhMinTris = 4096;   // "bvh_builder" = 2: smaller meshes get the host's swept SAH tree (a few ms at most), larger ones the device's binned one

// The frame tunables of ft_set_option (kOptions, include/functracer_hip.h).  Every device of a context holds the same values; flags are 0 / 1.
struct Options {
    int64_t chunk_samples = 16ll << 20;   // measured: 8 Mi costs 10-25 % (more, smaller launches), 32 Mi slows the shading on many-light scenes
    int64_t wave_samples = 0;       // bounce-0 wavefronts take up to this many samples of 64 / as many pixels when the sample count allows; 0: the default, 16
    int64_t coherent_waves = 1;     // diagnostic: 0 routes every wavefront through the incoherent paths
    int64_t timing = 1;             // HIP events: 0 around the frame only, 1 + around every tracing kernel (k_primary, the k_bounce levels), 2 around every stage
    int64_t classify_pixels = 1;    // k_classify: pixel blocks that cannot see any item are finished before any ray is generated
    int64_t follow_below = -1;      // a level of the reflection tree in which the previous frame had no more rays than this gets no launch of
                                    // its own: the last level launched follows them in registers.  -1: two rays per SIMD (2048 on 256 CUs: 8 x n_cu).  Measured at 1080p
                                    // (0 -> 10 000): hollow-sphere x1 0.881 -> 0.863 ms, sample-det x16 1.190 -> 1.164, sample-soft x4 0.905 -> 0.855; following
                                    // levels of 50 000 rays and more loses (hollow-sphere x1 0.976): a lane then drags its wave through every level
    int64_t level_hint = 1;         // launch only as many k_bounce levels as the previous frame of the same signature had (+ 1); 0: always max_depth
    int64_t classify_ahead = 1;     // 0 keeps every kernel on the one stream
    int64_t resolve_aside = 1;      // 0 keeps k_resolve on the main stream
    int64_t zero_fill_skip = 1;     // 0 writes Colour.Zero into every finished block of every frame
    int64_t classify_reuse = 1;     // 0 classifies every classified frame again, whatever its slot still holds (A/B)
    int64_t mains = 2;              // 1 .. 3: main streams in use (measured: 2 is best - the headline 0.263 / 0.231 / 0.249 ms with 1 / 2 / 3, hollow-sphere x1 0.703 / 0.471 / 0.470)
    int64_t bvh_builder = 2;        // who builds the exact BVH of top-level-Leaf meshes: 0 = the host (swept surface-area split: the best tree, 1.2 ms for 980
                                    // triangles but 160 ms for 69.6 K), 1 = the device's linear BVH (ft_bvh.hip: ~1 ms, traces ~9 % slower), 3 = the device's
                                    // binned surface-area tree over the Morton order, 2 = by size: the host's below kDeviceBvhMinTris triangles, 3's from there on
    int64_t csg_auto_grow = 1;      // ft_render: double csg_mesh_capacity and render again when a hit list overflows (read on device 0)
    int64_t primary_block_lists = 1;   // k_block_lists: the primaries of a classified frame over ONE bare mesh test their block's candidate list; 0: the tree walk everywhere
    int64_t refit_rebuild_percent = 0;   // ft_scene_commit_deformed rebuilds a device-built tree in place once cost now x 100 > this x cost as built; 0: never (not a commit-time option)
    int64_t temporal_follow_deformed = 0;   // ft_scene_commit_deformed keeps a mesh's records as the history saw them and ft_temporal_accumulate follows them
    int64_t uniform_surface = 1;    // k_primary: one-leaf batches take leaf and material through scalar loads, dead shader work and empty-list batches are skipped; 0: per lane, everything (A/B)
};

// One buffer in HBM per array of the flattened scene; DevScene points into them (upload_scene).
enum SceneArray { kLeaves, kM2w, kMaterials, kLights, kTextures, kTexPixels, kProgram, kMeshes, kNodes, kBspLeaves, kTris, kCulls, kCullItems,
                  kCullRows, kItemPc, kWide, kMeshWide, kCoarse, kTriOrig, kLsPairs, kLsNodes, kLsTris,
                  kTriSrc, kRunNodes,   // read by k_aov only (ft_render_aov): not part of DevScene
                  kSceneArrays };

// HIP events of one frame on its main stream.  An event between two dependent kernels costs about 6 us of stream time, so by default
// ("timing" = 1) only the kernels that trace rays (k_primary, the k_bounce levels) are bracketed; 2 brackets every stage, 0 only the frame.
// The frame's first event is recorded in front of its first launch on the main stream, behind the waits for other streams' events: on a
// queued frame it doubles as the start of k_primary's bracket (an event record costs ~5 us of stream time; a frame of 0.27 ms had four
// between two k_primary launches, now two).
struct Brackets {
    std::vector<hipEvent_t> events; size_t used = 0;   // created as needed, reused by the slot's later frames
    struct Span { hipEvent_t a, b; int kind; };
    std::vector<Span> spans;
    hipStream_t ms = nullptr;
    int timing = 1;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // the frame's first and last event (ev1: where it is done)
    hipEvent_t boundary = nullptr;
    bool fresh = false;                        // `boundary` was recorded right before the next entry of the main stream
    void begin(hipStream_t s, int t) { used = 0; spans.clear(); ms = s; timing = t; ev0 = ev1 = boundary = nullptr; fresh = false; }
    hipEvent_t next() {
        if (used == events.size()) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return nullptr; events.push_back(e); }
        return events[used++];
    }
    hipEvent_t record(hipStream_t s) { hipEvent_t e = next(); if (e) (void)hipEventRecord(e, s); return e; }
    void open() { if (ev0) return; ev0 = record(ms); boundary = ev0; fresh = true; }
    template <class Fn> void timed(int kind, Fn&& fn) {
        const bool bracket = timing >= 2 || (timing == 1 && (kind == kStageClosest || kind == kStageShade || kind == kStagePrimary));
        open();
        if (bracket && !fresh) boundary = record(ms);
        fn();
        if (!bracket) { fresh = false; return; }
        hipEvent_t b = record(ms);
        if (boundary && b) spans.push_back(Span{boundary, b, kind});
        boundary = b; fresh = true;
    }
    void release() { for (hipEvent_t e : events) (void)hipEventDestroy(e); events.clear(); used = 0; }
};

// What decides every word k_classify and k_block_lists write for a frame (neither reads the sample count, the offsets themselves or the
// wave grouping): the fields are compared, not hashed.
struct ClassifyKey {
    uint64_t commit_serial = 0;
    int32_t res_h = 0, res_v = 0, list_leaf = -1;
    double jitter_extent = 0.0;
    ftk::Camera cam{};
    std::vector<ft_rect> rects;      // the tiles clipped to the frame: they and res_h decide the pixel list
    bool operator==(const ClassifyKey& o) const {
        return commit_serial == o.commit_serial && res_h == o.res_h && res_v == o.res_v && list_leaf == o.list_leaf &&
               std::memcmp(&jitter_extent, &o.jitter_extent, sizeof jitter_extent) == 0 && std::memcmp(&cam, &o.cam, sizeof cam) == 0 &&
               rects.size() == o.rects.size() && (rects.empty() || std::memcmp(rects.data(), o.rects.data(), rects.size() * sizeof(ft_rect)) == 0);
    }
};

struct ft_context {
    static constexpr int kMains = 3;   // main streams at most: consecutive simple frames trace on different ones (option "mains" says how many are in use)
    static constexpr int kAcc = kMains;   // copies of the sample colours: one per frame between its k_primary and its k_resolve
    static constexpr int kSlots = kMains + 1;   // frames in flight: one per main stream + the one being classified ahead
    std::vector<ft_context*> peers;      // multi-device contexts: one more single-device context per extra GPU (scene replicated)
    std::vector<DeviceWorker*> workers;  // ... and one host thread per peer
    bool host_only = false;
    int device = -1;
    int n_cu = 0;
    hipStream_t stream = nullptr;
    hipStream_t more_mains[kMains - 1] = {};   // further main streams: consecutive simple queued frames trace on different ones, so that a frame's kernels are dispatched while its predecessors' drain
    std::string err;
    Options opt;

    fth::SceneGraph graph;
    fth::FlatScene flat;
    std::vector<float> cull_items_and_rows;   // what d_scene[kCullItems] holds (the upload's source)
    bool committed = false;
    // What ft_scene_commit_moved asks for: `flat` is a successful commit's, and no builder call since has added a node, changed the root
    // or the lights, or cleared the graph (ft_sg_set_transform and ft_set_option have not) - the same leaves in the same order.
    bool holds_commit = false, restructured = false;
    // What ft_scene_commit_deformed asks for on top of that: no ft_sg_set_transform and no commit-time option waiting for a full commit
    // (both cleared by every successful full commit).
    bool moved_pending = false, options_pending = false;
    uint64_t pose_serial = 0;       // advanced by ft_scene_commit_moved only (commit_serial also by the hit lists' re-commit, which moves nothing)
    double commit_ms[4] = {0, 0, 0, 0};   // last ft_scene_commit: flatten on the host, device BVH builds, uploads + the rest, BVH height (not a time)

    DeviceBuf d_scene[kSceneArrays];
    hipStream_t side = nullptr;     // the second stream: k_classify of frame N + 1 beside k_primary's tail / k_resolve of frame N (ft_render_enqueue)
    // Kernel variants and resident workgroups per CU for the committed scene (they only change at commit): bit 0 FANCY, 1 SOFT, 2 MESH; the
    // primary's variant may carry bit 3 (the five-workgroup lean build).
    int variant = 0, variant_primary = 0, blocks_primary = 1, blocks_bounce = 1, blocks_resolve = 2, blocks_aov = 1;
    hipEvent_t classified = nullptr;  // behind the latest k_classify on either stream: the next one waits for it (they share the ticket words of d_wave_counts)
    ftk::DevScene dev_scene{};
    // frame buffers in HBM
    DeviceBuf d_rays[2 * kMains], d_acc[kAcc], d_out, d_out8, d_out_index, d_pixels, d_jitter, d_wave_counts, d_dbg_in, d_dbg_out;
    // ft_render_aov's own pixel list, jitter pattern, planes and counters: nothing a frame or a progressive pass keeps is touched
    struct Aov {
        DeviceBuf d_pixels, d_jitter, d_out, d_ctr;
        TimedLaunch timer;          // around each k_aov launch (kernel_ms)
        void release() { for (DeviceBuf* b : {&d_pixels, &d_jitter, &d_out, &d_ctr}) b->release(); timer.release(); }
    } aov;
    // ft_denoise's own buffers, frame-sized, allocated by the first call: the guide records, the two colour buffers the iterations
    // alternate between (the last one's FP64 result lands in one of them) and the RGBA8 result
    struct Denoise {
        DeviceBuf d_guides, d_u[2], d_out8;
        TimedLaunch timer;          // around the scatter kernels and iterations of a call (kernel_ms)
        void release() { for (DeviceBuf* b : {&d_guides, &d_u[0], &d_u[1], &d_out8}) b->release(); timer.release(); }
    } denoise;
    // The sample colours exist twice: a queued frame's k_resolve runs on a stream of its own (`tail`), behind an event, while the next
    // chunk's / frame's k_primary already fills the other copy - the small kernel hides in the big one's ramp instead of standing between
    // two of them.  acc_free[i]: behind the last k_resolve that read copy i (the next k_primary into that copy waits for it).
    int acc_turn = 0;
    hipStream_t tail = nullptr;
    hipEvent_t acc_free[kAcc] = {};
    bool acc_busy[kAcc] = {};
    // Colour.Zero in the blocks k_classify finished: what the last frame written into d_out / d_out8 classified (scene, camera, size, pixel
    // list, jitter extent).  A frame of the same signature finds those pixels zero already and does not write them again.
    uint64_t zero_signature[2] = {0, 0};
    uint32_t classify_epoch = 0;    // tags the entries k_classify's waves publish in d_wave_counts (cleared only when it wraps or the buffer grows)
    int64_t ray_capacity = 0, acc_capacity = 0;
    // Per-frame state.  One slot per frame in flight, so that frames can be queued while earlier ones still run (ft_render_enqueue).
    struct FrameSlot {
        // What k_classify writes and the frame's later kernels read exists once per slot, so that a queued frame's classification can
        // run (on `side`, behind an event) while the frame before it is still tracing: block_pos / pos_block and the frame's counters.
        DeviceBuf d_block_pos, d_pos_block, d_fc;
        DeviceBuf d_list_heads, d_list_pool;    // k_block_lists: a header per active block, the entries (ftk::BlockLists)
        int32_t list_leaf = -1;                 // the mesh leaf this slot's frame carries lists for; -1: none
        ftk::Camera list_cam{};                 // that frame's image plane (ft_debug_block_lists)
        // "classify_reuse": what d_block_pos, d_pos_block, the lists and SlotCounters::kept hold.  `valid` from the retirement, without
        // error, of the frame that classified into them until anything makes that untrue; a frame of the same key then launches neither
        // k_classify nor k_block_lists.  n_active, culled: what that frame's report said (the active list's length; ft_stats'
        // rays_primary_culled is made from the other, which a frame that reuses the buffers does not count again).
        struct Classified { bool valid = false; ClassifyKey key; int64_t n_active = 0; uint64_t culled = 0; } kept;
        bool keeps = false, reuses = false;     // the pending frame fills `kept` when it retires / reads the buffers as they are
        bool fc_clean = false;                  // d_fc's FrameCounters are all zero: the slot's previous frame cleared it behind its report (no fill needed)
        Brackets ev;
        bool simple = false;                    // one chunk, k_resolve aside
        int main_ix = 0;                        // the main stream it traces on
        ftk::FrameReport* h_report = nullptr;   // pinned: the frame's statistic stripes, k_classify's error word and the last chunk's rays per bounce,
        ftk::FrameReport* d_report = nullptr;   // written by the frame's last kernel through this device-side address of the same memory
        uint64_t signature = 0;                 // what the frame rendered (scene, size, samples, depth, threshold): keys the staged-launch hint
        bool pending = false;
        uint64_t rays_primary = 0; int64_t n_pix_total = 0; int32_t spp = 0, n_launches = 0, n_chunks = 0, format = 0; bool classify = false;   // (n_launches, n_chunks: as planned from the request, FramePlan::n_planned)
        std::chrono::steady_clock::time_point wall0;
        void release() {
            d_block_pos.release(); d_pos_block.release(); d_fc.release(); d_list_heads.release(); d_list_pool.release();
            if (h_report) (void)hipHostFree(h_report);
            h_report = nullptr; d_report = nullptr;
            ev.release();
        }
    };
    FrameSlot slots[kSlots];
    // ft_scene_commit_deformed's own tables in HBM (ftk::RefitArrays), made by the first refit after a full commit and kept until the next
    // one (`ready`); d_verts: the new vertices of the meshes being refit.
    struct Refit {
        DeviceBuf d_verts, d_parent_node, d_parent_leaf, d_arrived, d_leaf_boxes, d_wide_node;
        DeviceBuf d_cost;           // k_refit_cost's partials and, behind them, its result
        bool ready = false;
        void release() { for (DeviceBuf* b : {&d_verts, &d_parent_node, &d_parent_leaf, &d_arrived, &d_leaf_boxes, &d_wide_node, &d_cost}) b->release(); ready = false; }
    } refit;
    // ft_scene_tree_quality, per mesh of `flat`, kept on the context's first device: the cost of the tree when it was last
    // built - measured the first time it is needed after a full commit, and again by every rebuild in place - and the rebuilds in place since
    // that commit.  Emptied by every full commit.
    struct TreeQuality { double cost_built = 0.0; bool known = false; uint32_t rebuilds = 0; };
    std::vector<TreeQuality> tree_quality;
    int slot_turn = 0;
    int64_t reuse_counts[4] = {0, 0, 0, 0};   // since ft_create: classifications launched / reused, windows launched / skipped (ft_debug_classify_reuse)
    int last_classified_slot = -1;   // the slot of the last frame queued if that frame was classified, else -1 (ft_debug_block_lists)
    // Levels of the reflection tree worth launching: the host cannot know how deep the rays of a frame go without waiting, and a
    // k_bounce launch that finds no rays still costs a few microseconds.  It launches as many levels as the previous frame of the
    // same signature had rays in, plus one; the last one launched follows whatever it still spawns to the end inside the kernel,
    // so the frame is complete however deep it goes.  -1: no history, launch max_depth levels.
    int staged_hint = -1;
    uint64_t staged_signature = 0;
    int ray_sets = 0;                // main streams whose pair of ray buffers holds ray_capacity records
    uint64_t commit_serial = 0;
    bool accum_open = false;        // kernel times are being summed over pipelined frames (reset by the next enqueue after a wait)
    // pixel list of the last render, cached across calls with the same resolution and tiles
    std::vector<uint32_t> pixels;
    std::vector<double> jitter_on_device;   // what d_jitter holds
    std::vector<ft_rect> pixel_rects;
    bool pixels_corner = false, pixels_tiled = false;   // the list holds corner-sampling pixels / is made of whole 8x8 tiles
    int last_format = 0;            // 0: the last frame is FP64 RGB in d_out, 1: RGBA8 in d_out8
    int64_t last_n_pix = 0;
    int32_t last_res_h = 0, last_res_v = 0;
    double k_ms[kStages] = {0, 0, 0, 0, 0};
    int32_t k_launches[kStages] = {0, 0, 0, 0, 0};
    int64_t last_active_pix = 0;    // pixels in the active list of the last frame retired (all listed ones when it was not classified)
    // A progressive accumulation (ft_progressive_begin .. _end).  Every device holds the request with its share of the frame (its 8-row
    // bands on a multi-device context) and the running state of that share by position in its pixel list; device 0 also the pass count.
    // The state is double-buffered: a pass reads side `cur` and writes side cur ^ 1, and cur flips only once every device's pass has
    // completed without a hit-list overflow, so the pass that runs again after the lists grew starts from the same sums.
    struct Progressive {
        bool open = false;
        ft_camera cam{};
        int32_t res_h = 0, res_v = 0, max_depth = 0, min_samples = 0;
        double tolerance = 0.0;
        std::vector<ft_rect> tiles;  // this device's rects, as the passes request them (clipped by plan_pixels)
        int64_t n_pix = 0, n_blocks = 0, passes = 0, samples = 0, traced = 0;   // samples: the most any pixel can have; traced: the last pass's
        DeviceBuf d_sum[2], d_sq[2], d_blk[2];
        int cur = 0;
        void release() { for (int k = 0; k < 2; ++k) { d_sum[k].release(); d_sq[k].release(); d_blk[k].release(); } *this = Progressive(); }
    } prog;
    // A temporal accumulation (ft_temporal_begin .. _end; single-device contexts only): the two history sets in frame layout
    // (ftk::TemporalSet, kTemporalSetBytes per frame pixel), the previous call's image plane, the call's result buffers and its two counts.
    // A call reads set `prev` and writes the other one; prev flips only once the call has succeeded, so a call that runs again after the
    // hit lists grew, or that failed, finds the history as it was.
    struct Temporal {
        bool open = false;
        int32_t res_h = 0, res_v = 0;
        std::vector<ft_rect> rects;     // the tiles clipped to the frame
        int64_t n_pix = 0, calls = 0, with_history = 0, at_max = 0;
        ftk::Camera cam{};              // the previous call's (calls > 0)
        DeviceBuf d_set[2], d_rgb, d_rgba8, d_ctr;
        TimedLaunch timer;              // around each k_temporal launch (kernel_ms)
        int prev = 0;
        // The pose the history was written in: the context's pose_serial at the last successful accumulate and every
        // leaf's m2w and w2m then (12 doubles each); d_motion: the call's records for k_temporal<true> (ftk::kTemporalMotionDoubles per leaf)
        uint64_t pose = 0;
        std::vector<double> h_m2w, h_w2m;
        DeviceBuf d_motion;
        // "temporal_follow_deformed" (DESIGN.md 16.2): the list-order records (9 doubles per triangle) of every mesh refit since the last
        // accumulate, as they lay in HBM before its first refit - `n` records of mesh `mesh` at record `first` of d_snap (snap_used of them
        // in all); d_deform: the call's records for k_temporal<MOVING, true> (ftk::TemporalDeformLeaf per leaf).  Dropped by every
        // successful accumulate, with the accumulation, and when the option goes back to 0 (ftc::temporal_drop_snapshots).
        struct Snapshot { uint32_t mesh, first, n; };
        std::vector<Snapshot> snaps;
        size_t snap_used = 0;
        DeviceBuf d_snap, d_deform;
        // ft_temporal_filter's planes, frame-sized, allocated by the first filter call of the accumulation: the divisor d,
        // the class, the two colour buffers and the two variance planes the iterations alternate between, and the RGBA8 result
        DeviceBuf d_fd, d_fcls, d_fu[2], d_fv[2], d_f8;
        TimedLaunch ftimer;             // around the kernels of a filter call (kernel_ms)
        // ft_temporal_set_clamp: clamp.radius 0 = off.  d_box: the six lo / hi planes k_temporal_box writes before the
        // first window of an accumulate; d_mask: a byte per frame pixel, 1 in T, filled once (mask_built); both allocated by the first
        // accumulate with the clamp on.  clamped: the pixels the clamp moved in the last accumulate.
        ft_temporal_clamp_params clamp{};
        int64_t clamped = 0;
        DeviceBuf d_box, d_mask;
        bool mask_built = false;
        void release() {
            for (DeviceBuf* b : {&d_set[0], &d_set[1], &d_rgb, &d_rgba8, &d_ctr, &d_motion, &d_snap, &d_deform, &d_fd, &d_fcls, &d_fu[0], &d_fu[1], &d_fv[0], &d_fv[1], &d_f8, &d_box, &d_mask}) b->release();
            timer.release(); ftimer.release(); *this = Temporal();
        }
    } temporal;
};
static_assert(ftk::kTemporalMinWeight == FT_TEMPORAL_MIN_WEIGHT, "the header states the constant k_temporal uses");

#define FT_HIP(ctx, call)                                                                              \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                            \
            return FT_ERR_HIP;                                                                         \
        }                                                                                              \
    } while (0)

template <class Launch, class Behind> int32_t TimedLaunch::run(ft_context* c, double& ms, Launch&& launch, Behind&& behind) {
    for (hipEvent_t& e : ev) if (!e) FT_HIP(c, hipEventCreate(&e));
    FT_HIP(c, hipEventRecord(ev[0], c->stream));
    launch();
    FT_HIP(c, hipGetLastError());
    FT_HIP(c, hipEventRecord(ev[1], c->stream));
    const int32_t rc = behind();
    if (rc != FT_OK) return rc;
    FT_HIP(c, hipStreamSynchronize(c->stream));
    float t = 0.0f;
    if (hipEventElapsedTime(&t, ev[0], ev[1]) == hipSuccess) ms += t;
    return FT_OK;
}

namespace ftc {

inline int32_t ensure(ft_context* c, DeviceBuf& b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.bytes >= bytes) return FT_OK;
    if (b.p) { FT_HIP(c, hipFree(b.p)); b.p = nullptr; b.bytes = 0; }
    FT_HIP(c, hipMalloc(&b.p, bytes));
    b.bytes = bytes;
    return FT_OK;
}
template <class T> int32_t upload(ft_context* c, DeviceBuf& b, const std::vector<T>& v) {
    int32_t rc = ensure(c, b, v.size() * sizeof(T));
    if (rc != FT_OK) return rc;
    if (!v.empty()) FT_HIP(c, hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, c->stream));
    return FT_OK;
}

// One frame as the caller asked for it: what the ft_render family, a progressive pass and the guide passes hand to the frame driver.
struct RenderRequest {
    const ft_camera* cam; int32_t res_h, res_v, spp; const double* jitter_xy; int32_t max_depth; uint64_t seed;
    const ft_rect* tiles; int32_t n_tiles; int format;               // 0: FP64 RGB frame, 1: RGBA8 frame
    bool progressive = false;                                        // a pass of the context's progressive accumulation (ft_progressive_pass)
};
constexpr double kNoJitter[2] = {0.0, 0.0};
inline bool any_pending(const ft_context* c, bool on_second_main = false) { for (const auto& f : c->slots) if (f.pending && (!on_second_main || f.main_ix != 0)) return true; return false; }

// ft_capi.cpp
bool need_device(ft_context* c);
bool need_committed(ft_context* c);
std::vector<ft_context*> devices(ft_context* c);
ftk::Camera make_camera(const ft_camera& cam, int res_h, int res_v);
size_t lds_bytes_for(const fth::FlatScene& f);
int32_t drain_frame_streams(ft_context* c);
int32_t commit_scene(ft_context* c);
int32_t copy_rects_out(ft_context* c, void* out, const void* frame, size_t px, int32_t res_h, const std::vector<ft_rect>& rects, hipStream_t async);
int32_t copy_frame_out(ft_context* c, void* out, int format, hipStream_t async);
int32_t fetch_single(ft_context* c, void* out, int format);
// ft_frame.cpp
ftk::RayBuf ray_view(const DeviceBuf& b, int64_t cap);
int32_t ensure_frame_buffers(ft_context* c, int64_t cap, bool reflective);
int32_t retire_pending(ft_context* c, ft_stats* stats);
std::vector<std::vector<ft_rect>> band_shares(const RenderRequest& q, size_t n_devs);
int32_t check_request(ft_context* c, const RenderRequest& q);
std::vector<ft_rect> clip_rects(const RenderRequest& q);
bool list_pixels(const std::vector<ft_rect>& rects, int32_t res_h, std::vector<uint32_t>& px);
int32_t render_single(ft_context* c, const RenderRequest& q, void* out, ft_stats* stats, bool defer);
int32_t on_every_device(ft_context* c, ft_stats* stats, std::chrono::steady_clock::time_point wall0,
                        const std::function<int32_t(size_t, ft_context*, ft_stats*)>& share);
int32_t with_growing_hit_lists(ft_context* c, const std::function<int32_t()>& run);
// ft_progressive.cpp, ft_passes.cpp
RenderRequest progressive_request(const ft_context::Progressive& P);
void progressive_close(ft_context* c);
void temporal_close(ft_context* c);
void temporal_drop_snapshots(ft_context* c);

} // namespace ftc

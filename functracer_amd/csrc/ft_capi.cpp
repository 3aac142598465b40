// ft_capi.cpp — the C ABI of libfunctracer_hip.so (include/functracer_hip.h): context, scene
// builder, HBM residency of the flattened scene and the per-frame wavefront pipeline driver.
// Reference citations are relative to FuncTracer/ of the reference (antonburger/FuncTracer).
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
    int64_t mains = 2;              // 1 .. 3: main streams in use (measured: 2 is best - the headline 0.263 / 0.231 / 0.249 ms with 1 / 2 / 3, hollow-sphere x1 0.703 / 0.471 / 0.470)
    int64_t bvh_builder = 2;        // who builds the exact BVH of top-level-Leaf meshes: 0 = the host (swept surface-area split: the best tree, 1.2 ms for 980
                                    // triangles but 160 ms for 69.6 K), 1 = the device's linear BVH (ft_bvh.hip: ~1 ms, traces ~9 % slower), 3 = the device's
                                    // binned surface-area tree over the Morton order, 2 = by size: the host's below kDeviceBvhMinTris triangles, 3's from there on
    int64_t csg_auto_grow = 1;      // ft_render: double csg_mesh_capacity and render again when a hit list overflows (read on device 0)
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
    DeviceBuf d_aov_pixels, d_aov_jitter, d_aov_out, d_aov_ctr;
    hipEvent_t aov_ev[2] = {};      // around each k_aov launch (kernel_ms)
    // ft_denoise's own buffers, frame-sized, allocated by the first call: the guide records, the two colour buffers the iterations
    // alternate between (the last one's FP64 result lands in one of them) and the RGBA8 result
    DeviceBuf d_dn_guides, d_dn_u[2], d_dn_out8;
    hipEvent_t dn_ev[2] = {};       // around the scatter kernels and iterations of a call (kernel_ms)
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
        bool fc_clean = false;                  // d_fc is all zero: the slot's previous frame cleared it behind its report (no fill needed)
        Brackets ev;
        bool simple = false;                    // one chunk, k_resolve aside
        int main_ix = 0;                        // the main stream it traces on
        ftk::FrameReport* h_report = nullptr;   // pinned: the frame's statistic stripes, k_classify's error word and the last chunk's rays per bounce,
        ftk::FrameReport* d_report = nullptr;   // written by the frame's last kernel through this device-side address of the same memory
        uint64_t signature = 0;                 // what the frame rendered (scene, size, samples, depth, threshold): keys the staged-launch hint
        bool pending = false;
        uint64_t rays_primary = 0; int64_t n_pix_total = 0; int32_t spp = 0, n_launches = 0, n_chunks = 0, format = 0; bool classify = false;
        std::chrono::steady_clock::time_point wall0;
        void release() {
            d_block_pos.release(); d_pos_block.release(); d_fc.release();
            if (h_report) (void)hipHostFree(h_report);
            h_report = nullptr; d_report = nullptr;
            ev.release();
        }
    };
    FrameSlot slots[kSlots];
    int slot_turn = 0;
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
        int prev = 0;
        void release() { for (DeviceBuf* b : {&d_set[0], &d_set[1], &d_rgb, &d_rgba8, &d_ctr}) b->release(); *this = Temporal(); }
    } temporal;
    hipEvent_t tp_ev[2] = {};       // around each k_temporal launch (kernel_ms)
};
static_assert(ftk::kTemporalMinWeight == FT_TEMPORAL_MIN_WEIGHT, "the header states the constant k_temporal uses");

namespace {

#define FT_HIP(ctx, call)                                                                              \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                            \
            return FT_ERR_HIP;                                                                         \
        }                                                                                              \
    } while (0)

int32_t ensure(ft_context* c, DeviceBuf& b, size_t bytes) {
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

bool need_device(ft_context* c) {
    if (!c) return false;
    if (c->host_only) { c->err = "host-only context: no HIP device bound (there is no CPU fallback for rendering)"; return false; }
    return true;
}

ftk::RayBuf ray_view(const DeviceBuf& b, int64_t cap) {
    double* d = b.as<double>();
    ftk::RayBuf r;
    r.ox = d; r.oy = d + cap; r.oz = d + 2 * cap; r.dx = d + 3 * cap; r.dy = d + 4 * cap; r.dz = d + 5 * cap; r.w = d + 6 * cap;
    r.slot = reinterpret_cast<uint32_t*>(d + 7 * cap);
    return r;
}

// Per-sample accumulators for every frame; the ray wavefront buffers only for scenes with reflective materials (bounce >= 1).
int32_t ensure_frame_buffers(ft_context* c, int64_t cap, bool reflective) {
    int32_t rc;
    if (cap > c->acc_capacity) { for (int k = 0; k < ft_context::kAcc; ++k) if ((rc = ensure(c, c->d_acc[k], (size_t)cap * 24)) != FT_OK) return rc; c->acc_capacity = cap; }
    if (!reflective || (cap <= c->ray_capacity && c->ray_sets >= c->opt.mains)) return FT_OK;
    const int64_t want = std::max(cap, c->ray_capacity);
    for (int i = 0; i < 2 * c->opt.mains; ++i) if ((rc = ensure(c, c->d_rays[i], (size_t)want * (7 * 8 + 4))) != FT_OK) return rc;   // a ping-pong pair per main stream in use
    c->ray_capacity = want; c->ray_sets = (int)c->opt.mains;
    return FT_OK;
}

// ImagePlane.create (Image.fs:48-53, 67-81), evaluated once per frame on the host.
ftk::Camera make_camera(const ft_camera& cam, int res_h, int res_v) {
    auto norm = [](double v[3]) { double l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); if (!(l < 0.0000001)) { double s = 1.0 / l; v[0] = s * v[0]; v[1] = s * v[1]; v[2] = s * v[2]; } };
    ftk::Camera out{};
    double k[3] = {cam.look_at[0] - cam.o[0], cam.look_at[1] - cam.o[1], cam.look_at[2] - cam.o[2]};
    norm(k);
    const double* u = cam.up;
    double i[3] = {u[1] * k[2] - u[2] * k[1], k[0] * u[2] - k[2] * u[0], u[0] * k[1] - u[1] * k[0]};     // up .** k
    norm(i);
    double j[3] = {k[1] * i[2] - k[2] * i[1], i[0] * k[2] - i[2] * k[0], k[0] * i[1] - k[1] * i[0]};     // k .** i
    const double height = std::tan(cam.fov_y / 2.0) * 2.0;
    const double width = height * cam.aspect_ratio;
    const double pixel_height = height / (double)(res_h - 1);      // sic, Image.fs:71: resH
    const double pixel_width = width / (double)(res_v - 1);        // sic, Image.fs:72: resV
    for (int a = 0; a < 3; ++a) { out.o[a] = cam.o[a]; out.k[a] = k[a]; out.i[a] = i[a]; out.j[a] = j[a]; }
    out.pw = pixel_width; out.ph = pixel_height;
    out.tlx = -width / 2.0 + pixel_width / 2.0; out.tly = height / 2.0 - pixel_height / 2.0;
    out.res_h = res_h; out.res_v = res_v;
    out.has_focus = cam.has_focus ? 1 : 0; out.focal_length = cam.focal_length;
    out.tan_half_aperture = std::tan(cam.aperture_angular_size / 2.0);          // Jitter.fs:30
    return out;
}

// LDS per workgroup: the per-lane CSG hit lists (4 words per entry) and tree stacks.  When the lists alone would not fit, lanes are
// folded (ft_kernels.hip, HitList): fold live lanes share the columns of 64 lanes, so a column needs only ceil(capacity / fold) rows.
constexpr size_t kLdsPerWorkgroup = 160 * 1024;
int lane_fold_for(const fth::FlatScene& f) {
    for (int fold = 1; fold <= 16; fold *= 2) {
        const size_t rows = ((size_t)f.csg_capacity + (size_t)fold - 1) / (size_t)fold;
        if ((4 * rows + (size_t)f.stack_capacity) * ftk::kBlock * 4 <= kLdsPerWorkgroup) return fold;
    }
    return 0;
}
// Materials only the FANCY kernel variants shade: Oren-Nayar, textures, and a specular exponent that is not a small whole number
// (ftd::small_whole_exponent: the lean variants do not carry Math.Pow).
bool needs_fancy(const ftd::Material& m) {
    return m.roughness != 0.0 || m.texture >= 0 || (m.shineyness > 0.0 && !ftd::small_whole_exponent(m.shineyness)) || m.shineyness != m.shineyness;
}
// The context's devices: itself, then its peers.
std::vector<ft_context*> devices(ft_context* c) {
    std::vector<ft_context*> devs{c};
    devs.insert(devs.end(), c->peers.begin(), c->peers.end());
    return devs;
}
size_t lds_bytes_for(const fth::FlatScene& f) {
    const int fold = std::max(1, lane_fold_for(f));
    return (4 * (((size_t)f.csg_capacity + (size_t)fold - 1) / (size_t)fold) + (size_t)f.stack_capacity) * ftk::kBlock * 4;
}

} // namespace

extern "C" {

int32_t ft_abi_version(void) { return FT_ABI_VERSION; }

static int32_t create_single(int32_t device_id, int count, ft_context** out) {
    if (device_id < 0 || device_id >= count) return FT_ERR_INVALID;
    ft_context* c = new ft_context();
    c->device = device_id;
    hipDeviceProp_t prop;
    if (hipSetDevice(c->device) != hipSuccess || hipGetDeviceProperties(&prop, c->device) != hipSuccess ||
        hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return FT_ERR_HIP; }
    int pr_low = 0, pr_high = 0;                                   // the side stream's few workgroups go first whenever slots come free
    if (hipDeviceGetStreamPriorityRange(&pr_low, &pr_high) != hipSuccess) pr_high = 0;
    if (hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, pr_high) != hipSuccess || hipStreamCreateWithPriority(&c->tail, hipStreamNonBlocking, pr_high) != hipSuccess) {
        if (c->side) (void)hipStreamDestroy(c->side);
        (void)hipStreamDestroy(c->stream); delete c; return FT_ERR_HIP;
    }
    for (hipStream_t& m : c->more_mains) if (hipStreamCreateWithFlags(&m, hipStreamNonBlocking) != hipSuccess) { m = nullptr; c->opt.mains = 1; }   // (without them every frame takes the one main stream)
    c->n_cu = prop.multiProcessorCount;
    *out = c;
    return FT_OK;
}

int32_t ft_create(const int32_t* device_ids, int32_t n_devices, ft_context** out) {
    if (!out) return FT_ERR_INVALID;
    *out = nullptr;
    if (n_devices < 1 || !device_ids) return FT_ERR_NO_DEVICE;     // no CPU backend exists in this library
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count < 1) return FT_ERR_NO_DEVICE;
    ft_context* c = nullptr;
    int32_t rc = create_single(device_ids[0], count, &c);
    if (rc != FT_OK) return rc;
    // More devices: the scene is replicated and every frame is split into 8-row bands dealt round-robin (no exchange
    // between devices; the bands meet in the caller's host buffer).  The same ordinal may be listed twice.
    for (int32_t k = 1; k < n_devices; ++k) {
        ft_context* p = nullptr;
        rc = create_single(device_ids[k], count, &p);
        if (rc != FT_OK) { ft_destroy(c); return rc; }
        c->peers.push_back(p);
        DeviceWorker* w = new DeviceWorker();
        w->start();
        c->workers.push_back(w);
    }
    *out = c;
    return FT_OK;
}

int32_t ft_create_host_only(ft_context** out) {
    if (!out) return FT_ERR_INVALID;
    ft_context* c = new ft_context();
    c->host_only = true;
    *out = c;
    return FT_OK;
}

void ft_destroy(ft_context* c) {
    if (!c) return;
    for (DeviceWorker* w : c->workers) { w->stop(); delete w; }
    c->workers.clear();
    for (ft_context* p : c->peers) ft_destroy(p);
    c->peers.clear();
    if (!c->host_only) {
        (void)hipSetDevice(c->device);
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        for (hipStream_t m : c->more_mains) if (m) (void)hipStreamSynchronize(m);
        if (c->side) (void)hipStreamSynchronize(c->side);
        if (c->tail) (void)hipStreamSynchronize(c->tail);
        for (DeviceBuf& b : c->d_scene) b.release();
        for (DeviceBuf& b : c->d_rays) b.release();
        for (DeviceBuf& b : c->d_acc) b.release();
        for (DeviceBuf* b : {&c->d_out, &c->d_out8, &c->d_out_index, &c->d_pixels, &c->d_jitter, &c->d_wave_counts, &c->d_dbg_in, &c->d_dbg_out, &c->d_aov_pixels, &c->d_aov_jitter, &c->d_aov_out, &c->d_aov_ctr, &c->d_dn_guides, &c->d_dn_u[0], &c->d_dn_u[1], &c->d_dn_out8}) b->release();
        for (auto& f : c->slots) f.release();
        c->prog.release();
        c->temporal.release();
        for (hipEvent_t& e : c->tp_ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
        if (c->classified) (void)hipEventDestroy(c->classified);
        for (hipEvent_t& e : c->acc_free) if (e) { (void)hipEventDestroy(e); e = nullptr; }
        for (hipEvent_t& e : c->aov_ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
        for (hipEvent_t& e : c->dn_ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
        if (c->side) (void)hipStreamDestroy(c->side);
        if (c->tail) (void)hipStreamDestroy(c->tail);
        for (hipStream_t m : c->more_mains) if (m) (void)hipStreamDestroy(m);
        if (c->stream) (void)hipStreamDestroy(c->stream);
    }
    delete c;
}

const char* ft_last_error(const ft_context* c) { return c ? c->err.c_str() : "null context"; }

// The keys of ft_set_option.  A flag takes any value as 0 / 1; any other value must lie in [lo, hi] (and be 0 or a power of two where
// kPowerOfTwo says so).  It goes into an Options member of every device of the context, or into device 0's scene graph: the peers
// receive the scene flattened on device 0.  kCommit / kLevelHint / kZeroFill: a change invalidates the committed scene, the staged
// level hint, the zero-fill signatures.
enum { kFlag = 1, kPowerOfTwo = 2, kCommit = 4, kLevelHint = 8, kZeroFill = 16 };
struct OptionSpec {
    const char* key;
    int64_t lo, hi;
    int64_t Options::* field;
    void (*to_graph)(fth::SceneGraph&, int64_t);
    int rules;
};
constexpr int64_t kNoLimit = std::numeric_limits<int64_t>::max();
const OptionSpec kOptions[] = {
    {"chunk_samples", 64, kNoLimit, &Options::chunk_samples, nullptr, 0},
    {"wave_samples", 0, 16, &Options::wave_samples, nullptr, kPowerOfTwo},   // 1 .. 16 samples per wavefront (k_resolve's LDS tile holds 16)
    {"coherent_waves", 0, 1, &Options::coherent_waves, nullptr, kFlag},
    {"timing", 0, 2, &Options::timing, nullptr, 0},
    {"classify_pixels", 0, 1, &Options::classify_pixels, nullptr, kFlag},
    {"follow_below", -1, kNoLimit, &Options::follow_below, nullptr, kLevelHint},
    {"level_hint", 0, 1, &Options::level_hint, nullptr, kFlag},
    {"classify_ahead", 0, 1, &Options::classify_ahead, nullptr, kFlag},
    {"resolve_aside", 0, 1, &Options::resolve_aside, nullptr, kFlag},
    {"zero_fill_skip", 0, 1, &Options::zero_fill_skip, nullptr, kFlag | kZeroFill},
    {"mains", 1, ft_context::kMains, &Options::mains, nullptr, 0},
    {"bvh_builder", 0, 3, &Options::bvh_builder, nullptr, kCommit},
    {"csg_auto_grow", 0, 1, &Options::csg_auto_grow, nullptr, kFlag},
    {"csg_mesh_capacity", 1, 255, nullptr, [](fth::SceneGraph& g, int64_t v) { g.csg_mesh_capacity = (int32_t)v; }, kCommit},
    // directional shadow rays of coherent waves: 0 the BVH; 1 light-space trees; 2 (default) light-space grids, the trees for wide waves.
    // It was a flag before the grids: it still takes any value, and any other than 0 / 1 means 2.
    {"light_space_shadows", std::numeric_limits<int64_t>::min(), kNoLimit, nullptr,
     [](fth::SceneGraph& g, int64_t v) { g.light_space_shadows = v == 0 || v == 1 ? (int32_t)v : 2; }, kCommit},
    {"mesh_unclipped_bvh", 0, 1, nullptr, [](fth::SceneGraph& g, int64_t v) { g.mesh_unclipped_bvh = v != 0; }, kFlag | kCommit},
};

int32_t ft_set_option(ft_context* c, const char* key, int64_t value) {
    if (!c || !key) return FT_ERR_INVALID;
    for (const OptionSpec& o : kOptions) {
        if (std::strcmp(key, o.key)) continue;
        if (o.rules & kFlag) value = value != 0;
        else if (value < o.lo || value > o.hi || ((o.rules & kPowerOfTwo) && (value & (value - 1)))) return FT_ERR_INVALID;
        if (o.to_graph) { o.to_graph(c->graph, value); c->committed = false; return FT_OK; }
        for (ft_context* d : devices(c)) {
            d->opt.*o.field = value;
            for (hipStream_t m : d->more_mains) if (!m) d->opt.mains = 1;   // (without them every frame takes the one main stream)
            d->dev_scene.coherent_waves = d->opt.coherent_waves ? 1 : 0;
            if (o.rules & kCommit) d->committed = false;
            if (o.rules & kLevelHint) d->staged_hint = -1;
            if (o.rules & kZeroFill) d->zero_signature[0] = d->zero_signature[1] = 0;
        }
        return FT_OK;
    }
    c->err = std::string("unknown option: ") + key;
    return FT_ERR_INVALID;
}

// ------------------------------------------------------------------------------------------ builder
static ft_node add_node(ft_context* c, fth::GraphNode&& n) { c->graph.nodes.push_back(std::move(n)); c->committed = false; return (ft_node)c->graph.nodes.size() - 1; }

ft_node ft_sg_primitive(ft_context* c, int32_t kind) {
    if (!c || kind < 0 || kind > FT_PRIM_CYLINDER) return FT_ERR_INVALID;
    fth::GraphNode n; n.kind = fth::GraphNode::Prim; n.prim = kind; return add_node(c, std::move(n));
}
ft_node ft_sg_triangle(ft_context* c, const double v[9]) {
    if (!c || !v) return FT_ERR_INVALID;
    fth::GraphNode n; n.kind = fth::GraphNode::TriangleP; std::memcpy(n.tri, v, sizeof n.tri); return add_node(c, std::move(n));
}
ft_node ft_sg_bsp_mesh(ft_context* c, int32_t depth, const double* tris, int64_t n_tris) {
    if (!c || n_tris < 0 || (n_tris > 0 && !tris) || depth < 0) return FT_ERR_INVALID;
    fth::GraphNode n; n.kind = fth::GraphNode::Mesh; n.depth = depth; n.tris.assign(tris, tris + 9 * n_tris); return add_node(c, std::move(n));
}
ft_node ft_sg_transform(ft_context* c, const ft_transform* ts, int32_t n_ts, ft_node child) {
    if (!c || !c->graph.valid(child) || !ts || n_ts < 1) return FT_ERR_INVALID;
    fth::GraphNode n; n.kind = fth::GraphNode::Transform;
    for (int i = 0; i < n_ts; ++i) { if (ts[i].kind < FT_TRANSLATE || ts[i].kind > FT_ROTATE) return FT_ERR_INVALID; n.xf.push_back(ts[i]); }
    n.children = {child};
    return add_node(c, std::move(n));
}
ft_node ft_sg_material(ft_context* c, const ft_material* m, ft_node child) {
    if (!c || !c->graph.valid(child) || !m) return FT_ERR_INVALID;
    fth::GraphNode n; n.kind = fth::GraphNode::MaterialF; n.mat = *m; n.children = {child}; return add_node(c, std::move(n));
}
ft_node ft_sg_hue_shift(ft_context* c, double, ft_node child) {
    if (!c || !c->graph.valid(child)) return FT_ERR_INVALID;
    fth::GraphNode n; n.kind = fth::GraphNode::HueShift; n.children = {child}; return add_node(c, std::move(n));
}
ft_node ft_sg_ignore_light(ft_context* c, ft_node child) {
    if (!c || !c->graph.valid(child)) return FT_ERR_INVALID;
    fth::GraphNode n; n.kind = fth::GraphNode::IgnoreLight; n.children = {child}; return add_node(c, std::move(n));
}
ft_node ft_sg_group(ft_context* c, const ft_node* children, int32_t n_children) {
    if (!c || n_children < 0 || (n_children > 0 && !children)) return FT_ERR_INVALID;
    fth::GraphNode n; n.kind = fth::GraphNode::Group;
    for (int i = 0; i < n_children; ++i) { if (!c->graph.valid(children[i])) return FT_ERR_INVALID; n.children.push_back(children[i]); }
    return add_node(c, std::move(n));
}
ft_node ft_sg_csg(ft_context* c, int32_t op, ft_node a, ft_node b) {
    if (!c || !c->graph.valid(a) || !c->graph.valid(b) || op < FT_CSG_UNION || op > FT_CSG_EXCLUDE) return FT_ERR_INVALID;
    fth::GraphNode n; n.kind = fth::GraphNode::Csg; n.op = op; n.children = {a, b}; return add_node(c, std::move(n));
}
ft_node ft_sg_texture_grid(ft_context* c, const double ca[3], const double cb[3], const double* uv_ops, int32_t n_uv_ops, ft_node child) {
    if (!c || !c->graph.valid(child) || !ca || !cb || n_uv_ops < 0 || (n_uv_ops > 0 && !uv_ops)) return FT_ERR_INVALID;
    fth::GraphNode n; n.kind = fth::GraphNode::Texture;
    std::memcpy(n.ca, ca, sizeof n.ca); std::memcpy(n.cb, cb, sizeof n.cb);
    n.uv_ops.assign(uv_ops, uv_ops + 3 * n_uv_ops); n.children = {child};
    return add_node(c, std::move(n));
}

ft_node ft_sg_texture_image(ft_context* c, const uint8_t* rgb24, int32_t width, int32_t height, const double* uv_ops, int32_t n_uv_ops, ft_node child) {
    if (!c || !c->graph.valid(child) || !rgb24 || width <= 0 || height <= 0 || (int64_t)width * height > (1ll << 28) || n_uv_ops < 0 || (n_uv_ops > 0 && !uv_ops)) return FT_ERR_INVALID;
    fth::GraphNode n; n.kind = fth::GraphNode::Texture;
    n.pixels.assign(rgb24, rgb24 + (size_t)width * height * 3); n.img_w = width; n.img_h = height;
    n.uv_ops.assign(uv_ops, uv_ops + 3 * n_uv_ops); n.children = {child};
    return add_node(c, std::move(n));
}

// Ends the progressive accumulation of a context, on every device (its buffers are freed).
static void progressive_close(ft_context* c) {
    if (!c->prog.open) return;
    for (ft_context* d : devices(c)) { if (!d->host_only) (void)hipSetDevice(d->device); d->prog.release(); }
}

// Ends the temporal accumulation of a context (its buffers are freed): leaf ids are only comparable within one commit.
static void temporal_close(ft_context* c) {
    if (!c->temporal.open) return;
    (void)hipSetDevice(c->device);
    c->temporal.release();
}

int32_t ft_scene_clear(ft_context* c) {
    if (!c) return FT_ERR_INVALID;
    progressive_close(c);
    temporal_close(c);
    c->graph.nodes.clear(); c->graph.lights.clear(); c->graph.root = -1; c->committed = false;
    return FT_OK;
}
int32_t ft_scene_set_objects(ft_context* c, ft_node root) {
    if (!c || !c->graph.valid(root)) return FT_ERR_INVALID;
    c->graph.root = root; c->committed = false;
    return FT_OK;
}
static void norm3(double v[3]) {                                    // Vector.normalise (CommonTypes.fs:63-67)
    double l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (!(l < 0.0000001)) { double s = 1.0 / l; v[0] = s * v[0]; v[1] = s * v[1]; v[2] = s * v[2]; }
}
int32_t ft_scene_add_directional(ft_context* c, const double dir[3], const double colour[3]) {      // Light.directional (Light.fs:19-20)
    if (!c || !dir || !colour) return FT_ERR_INVALID;
    ftd::Light l{}; l.kind = ftd::LT_DIRECTIONAL;
    std::memcpy(l.v, dir, sizeof l.v); norm3(l.v); std::memcpy(l.colour, colour, sizeof l.colour);
    c->graph.lights.push_back(l); c->committed = false;
    return FT_OK;
}
int32_t ft_scene_add_soft_directional(ft_context* c, const double dir[3], int32_t samples, double scatter_rad, const double colour[3]) {  // Light.fs:22-23
    if (!c || !dir || !colour || samples < 1) return FT_ERR_INVALID;
    ftd::Light l{}; l.kind = ftd::LT_SOFT; l.samples = samples; l.scatter = scatter_rad;
    std::memcpy(l.v, dir, sizeof l.v); norm3(l.v); std::memcpy(l.colour, colour, sizeof l.colour);
    c->graph.lights.push_back(l); c->committed = false;            // rejected at commit until the seeded stream lands
    return FT_OK;
}
int32_t ft_scene_add_positional(ft_context* c, const double pos[3], const double falloff[3], const double colour[3]) {  // Light.fs:25-26
    if (!c || !pos || !falloff || !colour) return FT_ERR_INVALID;
    ftd::Light l{}; l.kind = ftd::LT_POINT;
    std::memcpy(l.v, pos, sizeof l.v); std::memcpy(l.falloff, falloff, sizeof l.falloff); std::memcpy(l.colour, colour, sizeof l.colour);
    c->graph.lights.push_back(l); c->committed = false;
    return FT_OK;
}

static int32_t upload_scene(ft_context* c);
static int32_t retire_pending(ft_context* c, ft_stats* stats);
static bool any_pending(const ft_context* c, bool on_second_main = false) { for (const auto& f : c->slots) if (f.pending && (!on_second_main || f.main_ix != 0)) return true; return false; }
static int32_t commit_scene(ft_context* c);

// A caller's commit ends the progressive and the temporal accumulation; the re-commit of with_growing_hit_lists (commit_scene) does not.
int32_t ft_scene_commit(ft_context* c) {
    if (!c) return FT_ERR_INVALID;
    progressive_close(c);
    temporal_close(c);
    return commit_scene(c);
}

static int32_t commit_scene(ft_context* c) {
    using clock = std::chrono::steady_clock;
    auto ms_since = [](clock::time_point t0) { return std::chrono::duration<double, std::milli>(clock::now() - t0).count(); };
    for (double& v : c->commit_ms) v = 0.0;
    // A device context builds the exact BVH of top-level-Leaf meshes on the device ("bvh_builder" = 1; 2, the default: from 4096 triangles on): the flattener
    // reserves the ranges, upload_scene fills them.  A build the device refuses (a tree too deep for the traversal stacks) falls
    // back to the host's builder, once, for the whole scene.
    for (int attempt = 0; attempt < 2; ++attempt) {
        c->graph.device_bvh = !c->host_only && c->opt.bvh_builder >= 1 && attempt == 0;
        c->graph.device_bvh_min_tris = c->opt.bvh_builder == 2 ? kDeviceBvhMinTris : 0;   // 1: the device's linear BVH, 3: its surface-area tree, whatever the size
        auto t0 = clock::now();
        int32_t rc = c->graph.flatten(c->flat, c->err);
        c->commit_ms[0] += ms_since(t0);
        if (rc != FT_OK) return rc;
        if (c->host_only) { c->committed = true; return FT_OK; }
        t0 = clock::now();
        rc = upload_scene(c);
        for (ft_context* p : c->peers) {                            // replicate the flattened scene on every other device
            if (rc != FT_OK) break;
            p->flat = c->flat;
            if ((rc = upload_scene(p)) != FT_OK) c->err = p->err;
            c->commit_ms[1] += p->commit_ms[1];
        }
        c->commit_ms[2] += ms_since(t0) - c->commit_ms[1];
        if (rc == FT_ERR_BUILD && c->graph.device_bvh) continue;    // refused by the device builder: the host builds it
        return rc;
    }
    return FT_ERR_BUILD;
}

int32_t ft_get_commit_times(ft_context* c, double ms[4]) {
    if (!c || !ms) return FT_ERR_INVALID;
    for (int k = 0; k < 4; ++k) ms[k] = c->commit_ms[k];
    return FT_OK;
}

static int32_t upload_scene(ft_context* c) {
    int32_t rc;
    FT_HIP(c, hipSetDevice(c->device));
    // frames still queued trace the scene these uploads replace, and not all of them on the stream the uploads travel on (FrameSlot::main_ix)
    if (any_pending(c)) { if ((rc = retire_pending(c, nullptr)) != FT_OK) return rc; c->accum_open = false; }
    const fth::FlatScene& f = c->flat;
    if (lane_fold_for(f) == 0) { c->err = "scene needs more than 160 KiB of LDS per workgroup for CSG lists / BSP stacks even with 4 live lanes per wave"; return FT_ERR_UNSUPPORTED; }
    ftk::DevScene& S = c->dev_scene;
    rc = FT_OK;
    auto put = [&](SceneArray k, const auto& v, auto*& ptr) {   // array k into its buffer, and the device scene's pointer to it
        if (rc == FT_OK) rc = upload(c, c->d_scene[k], v);
        ptr = static_cast<std::remove_reference_t<decltype(ptr)>>(c->d_scene[k].p);
    };
    put(kLeaves, f.leaves, S.leaves); put(kM2w, f.m2w, S.m2w); put(kMaterials, f.materials, S.materials); put(kLights, f.lights, S.lights);
    put(kTextures, f.textures, S.textures); put(kTexPixels, f.tex_pixels, S.tex_pixels); put(kProgram, f.program, S.program);
    put(kMeshes, f.meshes, S.meshes); put(kNodes, f.nodes, S.nodes); put(kBspLeaves, f.bsp_leaves, S.bsp_leaves); put(kTris, f.tris, S.tris);
    put(kCulls, f.culls, S.culls);
    {   // behind the items' float records: a float image of every parallel-sensitive direction (x, y, z, its length rounded up), which lane k of a
        // coherent wave tests against the bundle's cone before any ray is tested against it exactly (rows_nearly_parallel, ft_kernels.hip)
        std::vector<float>& v = c->cull_items_and_rows;
        v = f.cull_items;
        v.resize(8 * (f.item_pc.size() - 1), 0.0f);
        for (size_t k = 0; k + 2 < f.cull_rows.size(); k += 3) {
            const double len = std::sqrt(f.cull_rows[k] * f.cull_rows[k] + f.cull_rows[k + 1] * f.cull_rows[k + 1] + f.cull_rows[k + 2] * f.cull_rows[k + 2]);
            float lf = (float)len; while ((double)lf < len) lf = std::nextafter(lf, std::numeric_limits<float>::infinity());
            v.push_back((float)f.cull_rows[k]); v.push_back((float)f.cull_rows[k + 1]); v.push_back((float)f.cull_rows[k + 2]); v.push_back(lf);
        }
        put(kCullItems, v, S.cull_items);
    }
    put(kCullRows, f.cull_rows, S.cull_rows); put(kItemPc, f.item_pc, S.item_pc); put(kWide, f.wide, S.wide); put(kMeshWide, f.mesh_wide, S.mesh_wide);
    put(kCoarse, f.coarse_boxes, S.coarse_boxes); put(kTriOrig, f.tri_orig, S.tri_orig);
    put(kLsPairs, f.ls_pairs, S.ls_pairs); put(kLsNodes, f.ls_nodes, S.ls_nodes); put(kLsTris, f.ls_tris, S.ls_tris);
    if (rc == FT_OK) rc = upload(c, c->d_scene[kTriSrc], f.tri_src);
    if (rc == FT_OK) rc = upload(c, c->d_scene[kRunNodes], f.run_nodes);
    if (rc != FT_OK) return rc;
    for (auto& F : c->slots) { if ((rc = ensure(c, F.d_fc, sizeof(ftk::FrameCounters))) != FT_OK) return rc; F.fc_clean = false; }
    c->zero_signature[0] = c->zero_signature[1] = 0;
    FT_HIP(c, hipStreamSynchronize(c->stream));
    {   // the BVHs the flattener left to the device (ft_bvh.hip), straight into the ranges reserved in the arrays just uploaded
        const auto t0 = std::chrono::steady_clock::now();
        uint32_t tallest = 0;
        for (const fth::FlatScene::BvhJob& j : f.bvh_jobs) {
            const DeviceBuf* B = c->d_scene;
            const ftk::LbvhTarget t{B[kTris].as<double>(), j.first_global, j.n, B[kNodes].as<ftd::BspNode>(), j.node_base, B[kBspLeaves].as<ftd::BspLeaf>(), j.leaf_base,
                                    B[kTriOrig].as<uint32_t>(), j.tri_base, B[kWide].as<double>(), j.wide_base, B[kCoarse].as<float>() + 6 * (size_t)j.coarse_first, j.coarse_count,
                                    B[kTriSrc].as<uint32_t>()};
            uint32_t height = 0;
            FT_HIP(c, ftk::build_lbvh(c->stream, t, &height, c->opt.bvh_builder == 1 ? 0 : 1));
            // height 0: a non-finite coordinate; > 40: deeper than the packet walk's 64-entry stack allows (3 entries per 4-wide level)
            if (height == 0 || height > 40) { c->err = "device BVH build refused (non-finite vertex or a tree deeper than 40 levels): the host builder takes over"; return FT_ERR_BUILD; }
            tallest = std::max(tallest, height);
        }
        if (!f.bvh_jobs.empty()) {
            c->commit_ms[1] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            c->commit_ms[3] = tallest;
            if ((int32_t)tallest + 1 > c->flat.stack_capacity) c->flat.stack_capacity = (int32_t)tallest + 1;   // per-lane node stacks of the incoherent walk (LDS)
            if (lane_fold_for(c->flat) == 0) { c->err = "scene needs more than 160 KiB of LDS per workgroup for CSG lists / BSP stacks even with 4 live lanes per wave"; return FT_ERR_UNSUPPORTED; }
        }
    }
    S.coherent_waves = c->opt.coherent_waves ? 1 : 0;
    S.n_simd = c->n_cu * 4;
    S.n_items = (int32_t)f.item_pc.size() - 1; S.n_cull_rows = f.cull_bundle ? (int32_t)(f.cull_rows.size() / 3) : -1;
    S.n_leaves = (int32_t)f.leaves.size(); S.n_lights = (int32_t)f.lights.size();
    S.csg_cap = f.csg_capacity; S.stack_cap = f.stack_capacity;
    S.lane_fold = lane_fold_for(f); S.csg_rows = (f.csg_capacity + S.lane_fold - 1) / S.lane_fold;
    S.shadow_rays_per_hit = 0;
    for (auto& l : f.lights) S.shadow_rays_per_hit += (l.kind == ftd::LT_SOFT) ? l.samples : 1;   // Shading.fs:24-42
    c->variant = 0;
    for (auto& m : f.materials) if (needs_fancy(m)) c->variant |= 1;                               // FANCY
    for (auto& l : f.lights) if (l.kind == ftd::LT_SOFT) c->variant |= 2;                          // SOFT
    if (!f.meshes.empty()) c->variant |= 4;                                                        // MESH
    const size_t lds = lds_bytes_for(c->flat);
    c->variant_primary = c->variant;
    c->blocks_primary = ftk::occupancy_blocks_primary(lds, &c->variant_primary);
    c->blocks_bounce = ftk::occupancy_blocks_bounce(lds, c->variant);
    c->blocks_resolve = ftk::occupancy_blocks_resolve();
    c->blocks_aov = ftk::occupancy_blocks_aov(lds, c->variant);
    c->committed = true;
    ++c->commit_serial; c->staged_hint = -1;
    return FT_OK;
}

// ------------------------------------------------------------------------------------------ frames out of HBM
// The device keeps the last frame in FRAME layout (row 0 = top, Image.fs:39) whatever the tiles were: d_out as FP64 RGB or d_out8 as
// Image.write's RGBA8 bytes (Image.fs:36).  Fetching copies the rendered rects - whole rows as one copy, narrower rects as a 2D copy -
// straight into the caller's frame; nothing is gathered or scattered on the host.
static int32_t copy_frame_out(ft_context* c, void* out, int format, hipStream_t async);
static int32_t fetch_single(ft_context* c, void* out, int format) {
    if (c->last_n_pix <= 0) { c->err = "no frame rendered yet"; return FT_ERR_STATE; }
    if (format != c->last_format) { c->err = format == 1 ? "the last frame was rendered as FP64 RGB (ft_render): no RGBA8 frame to fetch" : "the last frame was rendered as RGBA8 (ft_render_rgba8): no FP64 frame to fetch"; return FT_ERR_STATE; }
    FT_HIP(c, hipSetDevice(c->device));
    FT_HIP(c, hipStreamSynchronize(c->stream));                     // frames queued with ft_render_enqueue may still be running (the streams are non-blocking)
    for (hipStream_t m : c->more_mains) if (m) FT_HIP(c, hipStreamSynchronize(m));
    FT_HIP(c, hipStreamSynchronize(c->tail));                       // ... their k_resolve on its own stream
    return copy_frame_out(c, out, format, nullptr);
}
// The rects of the context's pixel list out of d_out / d_out8 into the caller's frame: blocking copies, or (async != null) queued on that
// stream behind the frame's k_resolve - the caller's memory should then be page-locked (ft_host_alloc), or the runtime stages the copy.
static int32_t copy_rects_out(ft_context* c, void* out, const void* frame, size_t px, int32_t res_h, const std::vector<ft_rect>& rects, hipStream_t async);
static int32_t copy_frame_out(ft_context* c, void* out, int format, hipStream_t async) {
    return copy_rects_out(c, out, format == 1 ? c->d_out8.p : c->d_out.p, format == 1 ? 4 : 24, c->last_res_h, c->pixel_rects, async);
}
// `rects` of a frame-layout buffer in HBM (px bytes per pixel, res_h pixels per row) into the caller's frame of the same layout.
static int32_t copy_rects_out(ft_context* c, void* out, const void* frame, size_t px, int32_t res_h, const std::vector<ft_rect>& rects, hipStream_t async) {
    auto copy1 = [&](void* d, const void* s_, size_t n) { return async ? hipMemcpyAsync(d, s_, n, hipMemcpyDeviceToHost, async) : hipMemcpy(d, s_, n, hipMemcpyDeviceToHost); };
    auto copy2 = [&](void* d, size_t dp, const void* s_, size_t sp, size_t w, size_t h) { return async ? hipMemcpy2DAsync(d, dp, s_, sp, w, h, hipMemcpyDeviceToHost, async) : hipMemcpy2D(d, dp, s_, sp, w, h, hipMemcpyDeviceToHost); };
    const size_t pitch = (size_t)res_h * px;
    const char* src = static_cast<const char*>(frame);
    char* dst = static_cast<char*>(out);
    // A device of a multi-device context holds every N-th 8-row band of the frame: whole rows, equally high, equally spaced.  Those go
    // out as ONE two-dimensional copy whose "rows" are the bands (band = 8 x pitch contiguous bytes, 8 N x pitch apart on both sides) -
    // 34 blocking copies of 737 KB per device at 4K otherwise.  A shorter last band follows on its own.
    size_t k0 = 0;
    {
        const auto& R = rects;
        size_t run = 0;
        if (R.size() >= 3 && R[0].x0 == 0 && R[0].w == res_h) {
            const int step = R[1].y0 - R[0].y0;
            run = 1;
            while (run < R.size() && R[run].x0 == 0 && R[run].w == R[0].w && R[run].h == R[0].h && R[run].y0 == R[0].y0 + (int)run * step) ++run;
            if (step > R[0].h && run >= 3) {
                const size_t off = (size_t)R[0].y0 * pitch;
                FT_HIP(c, copy2(dst + off, (size_t)step * pitch, src + off, (size_t)step * pitch, (size_t)R[0].h * pitch, run));
                k0 = run;
            }
        }
    }
    for (size_t k = k0; k < rects.size();) {
        const ft_rect r = rects[k];
        if (r.x0 == 0 && r.w == res_h) {                    // whole rows; vertically adjacent rects go out as one copy
            int rows = r.h;
            size_t k2 = k + 1;
            while (k2 < rects.size() && rects[k2].x0 == 0 && rects[k2].w == r.w && rects[k2].y0 == r.y0 + rows) { rows += rects[k2].h; ++k2; }
            FT_HIP(c, copy1(dst + (size_t)r.y0 * pitch, src + (size_t)r.y0 * pitch, (size_t)rows * pitch));
            k = k2;
        } else {
            const size_t off = (size_t)r.y0 * pitch + (size_t)r.x0 * px;
            FT_HIP(c, copy2(dst + off, pitch, src + off, pitch, (size_t)r.w * px, (size_t)r.h));
            ++k;
        }
    }
    return FT_OK;
}

// fn(d) for every listed device d of the context: device 0 on the calling thread, the others on their workers, all at once.
static void on_every_device(ft_context* c, const std::vector<bool>& take, const std::function<void(size_t)>& fn) {
    for (size_t d = 1; d < take.size(); ++d) if (take[d]) c->workers[d - 1]->post([&fn, d] { fn(d); });
    if (take[0]) fn(0);
    for (size_t d = 1; d < take.size(); ++d) if (take[d]) c->workers[d - 1]->wait();
}

static int32_t fetch_all(ft_context* c, void* out, int format) {
    if (!c || !out) return FT_ERR_INVALID;
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    const std::vector<ft_context*> devs = devices(c);
    std::vector<ft_context*> with;
    for (ft_context* d : devs) if (d->last_n_pix > 0) with.push_back(d);
    if (with.empty()) { c->err = "no frame rendered yet"; return FT_ERR_STATE; }
    if (with.size() == 1) { const int32_t rc = fetch_single(with[0], out, format); if (rc != FT_OK && with[0] != c) c->err = with[0]->err; return rc; }
    std::vector<int32_t> rcs(devs.size(), FT_OK);                   // every device copies its own bands into the caller's frame, all at once
    std::vector<bool> take(devs.size());
    for (size_t d = 0; d < devs.size(); ++d) take[d] = devs[d]->last_n_pix > 0;
    on_every_device(c, take, [&](size_t d) { rcs[d] = fetch_single(devs[d], out, format); });
    for (size_t d = 0; d < devs.size(); ++d) if (rcs[d] != FT_OK) { if (devs[d] != c) c->err = devs[d]->err; return rcs[d]; }
    return FT_OK;
}
int32_t ft_fetch_frame(ft_context* c, double* out_rgb) { return fetch_all(c, out_rgb, 0); }
int32_t ft_fetch_frame_rgba8(ft_context* c, uint8_t* out_rgba) { return fetch_all(c, out_rgba, 1); }

/* Page-locked host memory for frames (hipHostMalloc): a D2H copy into it is one DMA at link rate, without the runtime's staging. */
void* ft_host_alloc(size_t bytes) { void* p = nullptr; return (bytes && hipHostMalloc(&p, bytes, hipHostMallocDefault) == hipSuccess) ? p : nullptr; }
void ft_host_free(void* p) { if (p) (void)hipHostFree(p); }

// ------------------------------------------------------------------------------------------ render
struct RenderRequest {
    const ft_camera* cam; int32_t res_h, res_v, spp; const double* jitter_xy; int32_t max_depth; uint64_t seed;
    const ft_rect* tiles; int32_t n_tiles; int format;               // 0: FP64 RGB frame, 1: RGBA8 frame
    bool progressive = false;                                        // a pass of the context's progressive accumulation (ft_progressive_pass)
};
static int32_t render_single(ft_context* c, const RenderRequest& q, void* out, ft_stats* stats, bool defer);
static int32_t retire_frame(ft_context* c, ft_context::FrameSlot& f, ft_stats* stats);
static int32_t render_frame(ft_context* c, const RenderRequest& q, void* out, ft_stats* stats, bool defer);

static int32_t with_growing_hit_lists(ft_context* c, const std::function<int32_t()>& run) {
    // Frames still queued by ft_render_enqueue are retired first, so that an overflow of one of THEM is reported as what it is
    // (queued frames are not rendered again) instead of being taken for this call's.
    if (!c->host_only) {
        for (ft_context* d : devices(c)) {
            if (!any_pending(d)) continue;
            if (hipSetDevice(d->device) != hipSuccess) { c->err = "hipSetDevice failed"; return FT_ERR_NO_DEVICE; }
            const int32_t prc = retire_pending(d, nullptr);
            d->accum_open = false;
            if (prc != FT_OK) { if (d != c) c->err = d->err; return prc; }
        }
    }
    int32_t rc = run();
    while (rc == FT_ERR_OVERFLOW && c->opt.csg_auto_grow && c->graph.csg_mesh_capacity < 255) {
        const int32_t before = c->graph.csg_mesh_capacity;
        const std::string why = c->err;
        c->graph.csg_mesh_capacity = std::min(255, before * 2);
        if (commit_scene(c) != FT_OK) {                            // the longer lists do not fit: back to the scene as it was
            c->graph.csg_mesh_capacity = before;
            if (commit_scene(c) == FT_OK) c->err = why;
            return FT_ERR_OVERFLOW;
        }
        rc = run();
    }
    return rc;
}

// The reference's hit lists are unbounded F# lists; the device's are sized at commit time.  A line that crosses a mesh under CSG
// more often than "csg_mesh_capacity" allows is detected (never truncated): the blocking call then doubles the capacity,
// re-commits the scene and renders the frame again, so the caller sees the reference's result without tuning anything.  The
// larger capacity stays for the following frames.  Only when the lists stop fitting is FT_ERR_OVERFLOW handed to the caller.
int32_t ft_render(ft_context* c, const ft_camera* cam, int32_t res_h, int32_t res_v, int32_t spp, const double* jitter_xy,
                  int32_t max_depth, uint64_t seed, const ft_rect* tiles, int32_t n_tiles, double* out_rgb, ft_stats* stats) {
    if (!c) return FT_ERR_INVALID;
    const RenderRequest q{cam, res_h, res_v, spp, jitter_xy, max_depth, seed, tiles, n_tiles, 0};
    return with_growing_hit_lists(c, [&] { return render_frame(c, q, out_rgb, stats, false); });
}
int32_t ft_render_rgba8(ft_context* c, const ft_camera* cam, int32_t res_h, int32_t res_v, int32_t spp, const double* jitter_xy,
                        int32_t max_depth, uint64_t seed, const ft_rect* tiles, int32_t n_tiles, uint8_t* out_rgba, ft_stats* stats) {
    if (!c) return FT_ERR_INVALID;
    const RenderRequest q{cam, res_h, res_v, spp, jitter_xy, max_depth, seed, tiles, n_tiles, 1};
    return with_growing_hit_lists(c, [&] { return render_frame(c, q, out_rgba, stats, false); });
}

static void add_stats(ft_stats* t, const ft_stats& s) {
    t->rays_primary += s.rays_primary; t->rays_shadow += s.rays_shadow; t->rays_reflect += s.rays_reflect; t->rays_traced += s.rays_traced;
    t->rays_reference_equivalent += s.rays_reference_equivalent; t->hits_primary += s.hits_primary; t->csg_overflow += s.csg_overflow;
    t->kernel_ms = std::max(t->kernel_ms, s.kernel_ms); t->trace_kernel_ms = std::max(t->trace_kernel_ms, s.trace_kernel_ms);
    t->algorithmic_bytes += s.algorithmic_bytes; t->hits_total += s.hits_total; t->algorithmic_bytes_closest += s.algorithmic_bytes_closest;
    t->algorithmic_bytes_shade += s.algorithmic_bytes_shade; t->algorithmic_bytes_primary += s.algorithmic_bytes_primary; t->n_launches += s.n_launches; t->n_chunks += s.n_chunks;
    t->rays_tail += s.rays_tail; t->rays_primary_culled += s.rays_primary_culled; t->rays_shadow_primary += s.rays_shadow_primary; t->rays_reflect_primary += s.rays_reflect_primary;
}

// Image-tile partition of a region over the devices of a context: 8-row bands of every requested rect, dealt round-robin.
static std::vector<std::vector<ft_rect>> band_shares(const RenderRequest& q, size_t n_devs) {
    std::vector<std::vector<ft_rect>> share(n_devs);
    const ft_rect whole_frame{0, 0, q.res_h, q.res_v};
    const ft_rect* src = q.tiles ? q.tiles : &whole_frame;
    const int n_src = q.tiles ? q.n_tiles : 1;
    size_t band = 0;
    for (int k = 0; k < n_src; ++k)
        for (int y = src[k].y0; y < src[k].y0 + src[k].h; y += 8, ++band)
            share[band % n_devs].push_back(ft_rect{src[k].x0, y, src[k].w, std::min(8, src[k].y0 + src[k].h - y)});
    return share;
}

static int32_t check_request(ft_context* c, const RenderRequest& q) {
    if (!q.cam || q.res_h < 2 || q.res_v < 2 || q.spp < 0 || (q.spp > 0 && !q.jitter_xy) || q.max_depth < 0 || (q.tiles && q.n_tiles < 1)) { c->err = "bad ft_render argument"; return FT_ERR_INVALID; }
    if (q.max_depth > ftk::kMaxBounce) { c->err = "max_depth above 16"; return FT_ERR_UNSUPPORTED; }
    if ((int64_t)q.res_h * q.res_v > (int64_t)0x7FFFFFFF) { c->err = "resolution too large"; return FT_ERR_INVALID; }
    return FT_OK;
}

static int32_t render_frame(ft_context* c, const RenderRequest& q, void* out, ft_stats* stats, bool defer) {
    const int32_t rc = check_request(c, q);
    if (rc != FT_OK) return rc;
    if (c->peers.empty() || c->host_only) return render_single(c, q, out, stats, defer);
    if (!c->committed) { c->err = "scene not committed (ft_scene_commit)"; return FT_ERR_STATE; }
    const auto wall0 = std::chrono::steady_clock::now();
    const std::vector<ft_context*> devs = devices(c);
    const std::vector<std::vector<ft_rect>> share = band_shares(q, devs.size());
    std::vector<int32_t> rcs(devs.size(), FT_OK);
    std::vector<ft_stats> sts(devs.size());
    // One host thread per device: each queues its bands' frame on its own stream, waits for it and copies its bands straight into the
    // caller's frame (whole rows: one contiguous copy per band).  No device waits for another; the bands meet in `out`.
    on_every_device(c, std::vector<bool>(devs.size(), true), [&](size_t d) {
        std::memset(&sts[d], 0, sizeof(ft_stats));
        if (share[d].empty()) { devs[d]->last_n_pix = 0; return; }
        RenderRequest qd = q;
        qd.tiles = share[d].data(); qd.n_tiles = (int32_t)share[d].size();
        rcs[d] = render_single(devs[d], qd, out, &sts[d], defer);
    });
    for (size_t d = 0; d < devs.size(); ++d) if (rcs[d] != FT_OK) { if (d) c->err = devs[d]->err; return rcs[d]; }
    if (stats && !defer) {
        std::memset(stats, 0, sizeof *stats);
        for (auto& s : sts) add_stats(stats, s);
        stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    }
    return FT_OK;
}

// What a frame is, decided on the host from the request and the context's cached state before anything is queued (plan_pixels,
// plan_chunks); queue_frame then puts it on the device.
struct FramePlan {
    struct Job { uint32_t id_base, n_ids, w, h, out_base, n_out; };   // a chunk: a window of the pixel list, or a corner grid
    std::vector<ft_rect> rects;          // the tiles clipped to the frame
    bool corner = false;                 // CornerSampling.strategy (Image.fs:125-150): one ray per pixel corner
    bool same_list = false;              // the context's pixel list, and d_pixels, already are this frame's
    std::vector<uint32_t> corner_ids;    // corner frames: the ids of the corner rays, what d_pixels must hold
    std::vector<Job> jobs;
    std::vector<double> jitter;          // what d_jitter must hold
    int32_t spp = 0;
    int64_t n_pix_total = 0;
    bool classify = false;
    bool simple = false;                 // a queued frame of one chunk: k_resolve aside, k_primary on the next main stream (queue_frame)
    bool progressive = false;            // a progressive pass: k_resolve_progressive over the accumulation's running sums
    bool mask_only = false;              // ... classified only by the retired blocks (adaptive passes of frames the host does not classify)
    double jitter_extent = 1.0;
    uint64_t signature = 0;              // scene, size, samples, depth, list, chunking: keys the level hint
    uint64_t zsig = 0;                   // what decides which blocks k_classify finishes: keys the zero-fill skip
    int64_t pix_per_chunk = 0, cap = 0;
    int group_log2 = 0, last_bounce = 0;
    ftk::Camera cam{};
};

// Pixel list restricted to the tiles.  The reference enumerates pixels y-major, x (Image.fs:104); samples are
// independent, so the device is free to walk them in any order: rects whose sides are multiples of 8 are
// walked in 8x8 pixel blocks, which makes the 64 lanes of a wavefront a compact bundle of rays.
static std::vector<ft_rect> clip_rects(const RenderRequest& q) {
    std::vector<ft_rect> rects;
    if (!q.tiles) rects.push_back(ft_rect{0, 0, q.res_h, q.res_v});
    else for (int k = 0; k < q.n_tiles; ++k) {
        ft_rect r = q.tiles[k];
        if (r.x0 < 0) { r.w += r.x0; r.x0 = 0; }
        if (r.y0 < 0) { r.h += r.y0; r.y0 = 0; }
        if (r.x0 + r.w > q.res_h) r.w = q.res_h - r.x0;
        if (r.y0 + r.h > q.res_v) r.h = q.res_v - r.y0;
        if (r.w > 0 && r.h > 0) rects.push_back(r);
    }
    return rects;
}
// The pixel list of (non-corner) rects; returns whether it is made of whole 8x8 tiles.
static bool list_pixels(const std::vector<ft_rect>& rects, int32_t res_h, std::vector<uint32_t>& px) {
    px.clear();
    bool tiled = true;
    for (const ft_rect& r : rects) {
        if (r.w % 8 == 0 && r.h % 8 == 0) {
            // inside a block the pixels run in Z order (first its top-left corner, last its bottom-right one, as k_classify expects):
            // the 4 or 16 consecutive pixels a wavefront takes under grouped numbering are a 2x2 or 4x4 square, not a strip
            for (int ty = 0; ty < r.h; ty += 8) for (int tx = 0; tx < r.w; tx += 8)
                for (int k = 0; k < 64; ++k) {
                    const int ix = (k & 1) | ((k >> 1) & 2) | ((k >> 2) & 4), iy = ((k >> 1) & 1) | ((k >> 2) & 2) | ((k >> 3) & 4);
                    px.push_back((uint32_t)((r.y0 + ty + iy) * res_h + r.x0 + tx + ix));
                }
        } else {
            tiled = false;
            for (int y = r.y0; y < r.y0 + r.h; ++y) for (int x = r.x0; x < r.x0 + r.w; ++x) px.push_back((uint32_t)(y * res_h + x));
        }
    }
    return tiled;
}

static void plan_pixels(ft_context* c, const RenderRequest& q, FramePlan& p) {
    const int32_t res_h = q.res_h, res_v = q.res_v;
    p.corner = q.spp == 0;
    p.spp = p.corner ? 1 : q.spp;
    p.progressive = q.progressive;
    p.rects = clip_rects(q);
    const std::vector<ft_rect>& rects = p.rects;
    p.same_list = !p.corner && !c->pixels_corner && c->last_n_pix > 0 && c->last_res_h == res_h && c->last_res_v == res_v &&
                  c->pixel_rects.size() == rects.size() && (rects.empty() || std::memcmp(c->pixel_rects.data(), rects.data(), rects.size() * sizeof(ft_rect)) == 0);
    std::vector<uint32_t>& px = c->pixels;
    if (p.corner) {
        // Each rect (split by rows so that its corner grid fits one chunk) is a job of (w+1) x (h+1) corner rays.
        px.clear();
        const uint32_t cs = (uint32_t)res_h + 1;
        for (const ft_rect& r : rects) {
            int64_t max_rows = c->opt.chunk_samples / (r.w + 1) - 1;
            if (max_rows < 1) max_rows = 1;
            for (int y0 = r.y0; y0 < r.y0 + r.h; y0 += (int)max_rows) {
                const int h = (int)std::min<int64_t>(max_rows, r.y0 + r.h - y0);
                FramePlan::Job j{(uint32_t)p.corner_ids.size(), (uint32_t)((r.w + 1) * (h + 1)), (uint32_t)r.w, (uint32_t)h, (uint32_t)px.size(), (uint32_t)(r.w * h)};
                for (int y = y0; y <= y0 + h; ++y) for (int x = r.x0; x <= r.x0 + r.w; ++x) p.corner_ids.push_back((uint32_t)y * cs + (uint32_t)x);
                for (int y = y0; y < y0 + h; ++y) for (int x = r.x0; x < r.x0 + r.w; ++x) px.push_back((uint32_t)(y * res_h + x));
                p.jobs.push_back(j);
            }
        }
        c->pixel_rects = rects; c->pixels_corner = true; c->pixels_tiled = false; c->last_n_pix = 0;
    } else if (!p.same_list) {
        const bool tiled = list_pixels(rects, res_h, px);
        c->pixel_rects = rects; c->pixels_corner = false; c->pixels_tiled = tiled; c->last_n_pix = 0;
    }
    p.n_pix_total = (int64_t)px.size();
}

// Classification, signatures and chunking of a frame with a non-empty pixel list.
static void plan_chunks(ft_context* c, const RenderRequest& q, bool defer, FramePlan& p) {
    const int64_t n_pix_total = p.n_pix_total, spp = p.spp;
    const int64_t chunk_samples = c->opt.chunk_samples;
    // k_classify bounds every sample of a pixel by a square of +-extent pixels around its centre.  The reference's offsets lie in the
    // unit disc (Jitter.fs:15-21) but the pattern is the caller's: the square follows the pattern, and a pattern with a non-finite
    // or absurd offset turns classification off instead of bounding nothing.
    bool jitter_bounded = true;
    if (!p.corner) for (size_t k = 0; k < 2 * (size_t)spp; ++k) { const double v = q.jitter_xy[k]; if (!(std::fabs(v) <= 64.0)) jitter_bounded = false; else p.jitter_extent = std::max(p.jitter_extent, std::fabs(v)); }
    // k_classify applies to pinhole cameras over pixel lists made of 8x8 tiles and scenes in which every top-level item is bounded (with
    // a ground plane in view an exact plane test does find the sky blocks - 20 % of night-house - but the denser first chunk makes the
    // shading slower than the blocks save).  A classified frame's chunks are windows of its ACTIVE pixel list, usually a fraction
    // of the frame: they are twice as wide (measured at 1080p x 16 in round 1: bunny 0.58 -> 0.55 ms, hollow-sphere 6.1 -> 5.8, sample
    // 1.64 -> 1.50; the unclassified night-house loses 14 % at that width and keeps the narrow one).
    p.classify = c->opt.classify_pixels && jitter_bounded && !p.corner && c->pixels_tiled && !q.cam->has_focus && c->flat.cull_bundle && c->flat.item_pc.size() > 1 && !c->flat.unbounded;
    p.signature = c->commit_serial * 0x9E3779B97F4A7C15ull;
    for (uint64_t v : {(uint64_t)q.res_h, (uint64_t)q.res_v, (uint64_t)spp, (uint64_t)q.max_depth, (uint64_t)n_pix_total, (uint64_t)chunk_samples, (uint64_t)(p.corner ? 1 : 0)})
        p.signature = (p.signature ^ v) * 0x100000001B3ull;
    // (round 3: five times as wide, not twice - 80 Mi listed samples.  A frame of one window is a SIMPLE frame below: its k_resolve goes aside and its
    //  k_primary to the other main stream.  A rank's eighth of 3840x2160x64 - 66 M listed samples, 5 M of them active - was two windows, the
    //  second one empty: 0.458 -> 0.417 ms per frame as one; its half 1.69 -> 1.62, its quarter and the whole frame unchanged, tools/rank_share_ab.py)
    // An unclassified frame without soft lights is worth one chunk of twice the width for the same reason (night-house-det 1080p x 16: two
    // chunks 2.60 ms, one - a simple, pipelined frame - 2.46); with soft lights the narrow chunks still win (night-house: 3.62 against 3.75).
    // The windows of a classified frame are cut from its LISTED pixels (the host does not know the active list's length when it queues
    // them), so a sparse frame is one window of work and a row of launches that find theirs empty (~20 us each: k_primary + k_resolve +
    // the counter fill; 3840x2160x64 of the bunny: 16 windows, 14 empty).  Windows widened by the last frame's active count measured no
    // net gain.
    const int64_t chunk_budget = p.classify ? 5 * chunk_samples : ((c->variant & 2) ? chunk_samples : 2 * chunk_samples);
    // An adaptive progressive pass always runs k_classify: on a frame the host does not classify (unbounded items, a focus camera, the
    // option off, an unbounded pattern) only to leave the retired blocks out of the active list.  Its windows stay as wide as unclassified ones.
    if (p.progressive && c->prog.tolerance > 0.0 && !p.classify) p.classify = p.mask_only = true;
    p.pix_per_chunk = std::max<int64_t>(1, std::min<int64_t>(n_pix_total, chunk_budget / spp));
    if (p.pix_per_chunk > 64) {
        // equal chunks rather than full ones and a remainder: a short last chunk is all latency (measured on night-house at
        // 1080p x 16: 25 M + 8 M samples 5.35 ms, 2 x 16.6 M 4.83 ms); 8x8 blocks (= wavefronts) stay whole
        const int64_t n_chunks = (n_pix_total + p.pix_per_chunk - 1) / p.pix_per_chunk;
        const int64_t even = ((n_pix_total + n_chunks - 1) / n_chunks + 63) / 64 * 64;
        p.pix_per_chunk -= p.pix_per_chunk % 64;
        if (even < p.pix_per_chunk) p.pix_per_chunk = even;
    }
    p.cap = p.pix_per_chunk * spp;
    if (p.corner) { p.cap = 1; for (auto& j : p.jobs) p.cap = std::max<int64_t>(p.cap, j.n_ids); }
    else for (int64_t p0 = 0; p0 < n_pix_total; p0 += p.pix_per_chunk) {
        const uint32_t n = (uint32_t)std::min<int64_t>(p.pix_per_chunk, n_pix_total - p0);
        p.jobs.push_back(FramePlan::Job{(uint32_t)p0, n, 0, 0, (uint32_t)p0, n});
    }
    p.last_bounce = c->flat.any_reflective ? q.max_depth : 0;   // no reflective material ⇒ no reflection rays are ever spawned
    if (p.corner) p.jitter = {-0.5, 0.5};                        // Image.fs:131
    else p.jitter.assign(q.jitter_xy, q.jitter_xy + 2 * (size_t)spp);
    p.cam = make_camera(*q.cam, q.res_h, q.res_v);
    // Samples per bounce-0 wavefront (slot_at, ft_kernels.hip): 2^group_log2 samples of 64 / 2^group_log2 pixels when the sample count
    // has that power of two in it and the list is made of whole 8x8 blocks.  Narrow bundles pay most where a wave walks a BVH
    // (measured at 1080p x 16, 1 -> 16 samples per wave: bunny through BSP leaves 1.46 -> 1.29 ms, night-house 4.63 -> 4.45).
    const int64_t most = c->opt.wave_samples > 0 ? c->opt.wave_samples : 16;
    if (!p.corner && c->pixels_tiled) while ((2ll << p.group_log2) <= most && !((spp >> p.group_log2) & 1)) ++p.group_log2;
    p.zsig = p.signature;
    auto mix = [&](const void* v, size_t n) { const unsigned char* b = static_cast<const unsigned char*>(v); for (size_t k = 0; k < n; ++k) p.zsig = (p.zsig ^ b[k]) * 0x100000001B3ull; };
    mix(&p.cam, sizeof p.cam); mix(&p.jitter_extent, sizeof p.jitter_extent);
    if (!p.rects.empty()) mix(p.rects.data(), p.rects.size() * sizeof(ft_rect));
    p.zsig |= 1ull;                                              // never 0: 0 means "nothing known about the buffer"
    // Queued frames of one chunk put k_resolve on its own stream (blocking frames have nothing to hide it in).  A frame cut into many
    // windows (3840x2160x64: 16, most of them empty behind the classification) pays an event pair per window and gains nothing - the windows'
    // small launches already overlap on one stream (measured: 3.46 -> 3.63 ms with it, profiles/r03_z_overlap_by_scene.json)
    p.simple = defer && c->opt.resolve_aside && !p.corner && c->opt.timing < 2 && p.jobs.size() == 1;
}

// Frame buffers, the output frame and the pixel list / jitter pattern on the device.  `queued`: something this frame's k_classify
// reads is still on its way on the first main stream.
static int32_t upload_frame_inputs(ft_context* c, const RenderRequest& q, const FramePlan& p, bool& queued) {
    int32_t rc;
    if ((rc = ensure_frame_buffers(c, p.cap, p.last_bounce > 0)) != FT_OK) return rc;
    DeviceBuf& ob = q.format == 1 ? c->d_out8 : c->d_out;
    const void* before = ob.p;
    if ((rc = ensure(c, ob, (size_t)q.res_h * (size_t)q.res_v * (q.format == 1 ? 4 : 24))) != FT_OK) return rc;
    if (ob.p != before) c->zero_signature[q.format] = 0;          // a new allocation holds nothing yet
    const bool new_jitter = p.jitter != c->jitter_on_device;      // frames usually reuse the pattern: skip the staged host-to-device copy
    queued = p.corner || !p.same_list || new_jitter;
    // The uploads below travel on the first main stream: a frame still tracing on the second one (FrameSlot::main_ix), or one whose k_resolve is
    // still to run on the tail stream (it reads the pixel list), reads what they replace.
    if (queued && any_pending(c) && (rc = retire_pending(c, nullptr)) != FT_OK) return rc;
    if (p.corner) {
        if ((rc = upload(c, c->d_pixels, p.corner_ids)) != FT_OK) return rc;
        if ((rc = upload(c, c->d_out_index, c->pixels)) != FT_OK) return rc;
    } else if (!p.same_list && (rc = upload(c, c->d_pixels, c->pixels)) != FT_OK) return rc;
    if (new_jitter) {
        c->jitter_on_device = p.jitter;                            // (the copy source outlives this call)
        if ((rc = upload(c, c->d_jitter, c->jitter_on_device)) != FT_OK) return rc;
    }
    return FT_OK;
}

// The whole frame is classified once; the chunks then take consecutive windows of the frame's ACTIVE pixel list, so a sparse
// frame is one chunk of real work and launches that find their window empty return at once.
static int32_t queue_classify(ft_context* c, const RenderRequest& q, const FramePlan& p, ft_context::FrameSlot& F, bool ahead) {
    const ftk::Primary all{p.cam, c->d_pixels.as<uint32_t>(), c->d_jitter.as<double>(), 0u, (uint32_t)p.n_pix_total, p.spp, (uint32_t)q.res_h,
                           (unsigned long long)q.seed, 1.0 / (double)p.n_pix_total, 1.0 / (double)q.res_h, nullptr, nullptr};
    const ftk::ClassifyOut cls{F.d_block_pos.as<int32_t>(), F.d_pos_block.as<uint32_t>(), c->d_wave_counts.as<uint32_t>()};
    const uint32_t* retired = p.progressive ? c->prog.d_blk[c->prog.cur].as<uint32_t>() : nullptr;   // a progressive pass leaves its retired blocks out
    auto* fc = F.d_fc.as<ftk::FrameCounters>();
    const uint32_t epoch = ++c->classify_epoch;
    // A queued frame's classification reads nothing the frames before it write (its slot's buffers were free once the slot's previous
    // frame was retired): it goes to the side stream and the main stream waits for its event, so it runs beside the previous
    // frame's k_primary tail and k_resolve instead of behind them.  A blocking frame, or one whose inputs are still being uploaded on
    // the main stream, classifies in line.  (Started as soon as it is queued, it takes the first workgroup slots of the previous frame's
    // k_primary: 226 -> 242 us, but holding it back for that frame's tracing only moved those 24 us.)
    const hipStream_t cs = ahead ? c->side : F.ev.ms;
    const ftk::Launch Lg{cs, c->n_cu * 8, 0, 0};
    if (!c->classified) FT_HIP(c, hipEventCreateWithFlags(&c->classified, hipEventDisableTiming));
    else FT_HIP(c, hipStreamWaitEvent(cs, c->classified, 0));  // one classification at a time, whichever streams they are on
    if (ahead) {
        ftk::launch_classify(Lg, c->dev_scene, all, cls, p.jitter_extent, epoch, fc, retired, p.mask_only);
        FT_HIP(c, hipEventRecord(c->classified, c->side));
        FT_HIP(c, hipStreamWaitEvent(F.ev.ms, c->classified, 0));
    } else {
        F.ev.timed(kStageOther, [&] { ftk::launch_classify(Lg, c->dev_scene, all, cls, p.jitter_extent, epoch, fc, retired, p.mask_only); });
        FT_HIP(c, hipEventRecord(c->classified, F.ev.ms));
    }
    F.ev.fresh = false;
    return FT_OK;
}

// The frame's chunks on its main stream: k_primary, the k_bounce levels and k_resolve of every window of the pixel list (or corner grid).
static int32_t queue_chunks(ft_context* c, const RenderRequest& q, const FramePlan& p, ft_context::FrameSlot& F, int main_ix, int32_t& n_launches) {
    Brackets& E = F.ev;
    const hipStream_t ms = E.ms;
    auto* fc = F.d_fc.as<ftk::FrameCounters>();
    const size_t lds = lds_bytes_for(c->flat);
    const ftk::Launch Lp{ms, c->n_cu * c->blocks_primary, lds, c->variant_primary};
    const ftk::Launch Lb{ms, c->n_cu * c->blocks_bounce, lds, c->variant};
    const ftk::Launch Lg{ms, c->n_cu * 8, 0, 0};
    const ftk::Launch Lr{ms, c->n_cu * c->blocks_resolve, 0, 0};
    const ftk::RayBuf rb[2] = {ray_view(c->d_rays[2 * main_ix], c->ray_capacity), ray_view(c->d_rays[2 * main_ix + 1], c->ray_capacity)};
    const bool zeros_in_place = p.classify && !p.progressive && c->opt.zero_fill_skip && c->zero_signature[q.format] == p.zsig;
    c->zero_signature[q.format] = p.classify && !p.progressive ? p.zsig : 0;   // (a progressive pass writes means into the finished blocks)
    double* const out_rgb = q.format == 1 ? nullptr : c->d_out.as<double>();
    uint8_t* const out_rgba = q.format == 1 ? c->d_out8.as<uint8_t>() : nullptr;
    const uint32_t stride = (uint32_t)(p.corner ? q.res_h + 1 : q.res_h);
    // Bounces >= 1: one k_bounce per level of the reflection tree, as many as the previous frame of this signature had (+ 1).
    // With "timing" = 1 the whole region is one bracket (kind shade): a bracket per launch costs more than a small level does.
    const bool hinted = c->opt.level_hint && c->staged_hint >= 0 && c->staged_signature == p.signature;
    const int n_levels = hinted ? std::min(p.last_bounce, c->staged_hint + 1) : p.last_bounce;
    for (const FramePlan::Job& job : p.jobs) {
        const bool first = &job == &p.jobs.front(), last = &job == &p.jobs.back();   // the frame's last kernel hands the counters over (FrameReport)
        const uint32_t n_pix = job.n_ids, n_samples = n_pix * (uint32_t)p.spp;
        if (!first) E.timed(kStageOther, [&] { (void)hipMemsetAsync(&fc->cc, 0, sizeof(ftk::ChunkCounters), ms); });
        ftk::Primary gen{p.cam, c->d_pixels.as<uint32_t>(), c->d_jitter.as<double>(), job.id_base, n_pix, p.spp, stride, (unsigned long long)q.seed,
                         1.0 / (double)n_pix, 1.0 / (double)stride, nullptr, nullptr};
        if (p.classify) { gen.counts = &fc->counts; gen.block_map = F.d_pos_block.as<uint32_t>(); }   // pix_base = job.id_base: the window's start in the active list
        gen.group_log2 = (n_pix % 64u == 0u) ? p.group_log2 : 0;
        const int at = c->acc_turn;
        double* const acc = c->d_acc[at].as<double>();
        if (c->acc_busy[at]) { FT_HIP(c, hipStreamWaitEvent(ms, c->acc_free[at], 0)); c->acc_busy[at] = false; E.fresh = false; }   // a k_resolve on `tail` may still be reading this copy
        E.timed(kStagePrimary, [&] { ftk::launch_primary(Lp, c->dev_scene, gen, rb[1], acc, n_samples, q.max_depth, fc); });
        auto bounce = [&](int b) { ftk::launch_bounce(Lb, c->dev_scene, gen, rb[b & 1], rb[(b + 1) & 1], acc, n_samples, b, q.max_depth, b == n_levels && n_levels < p.last_bounce, fc); };
        if (E.timing >= 2) for (int b = 1; b <= n_levels; ++b) E.timed(kStageShade, [&] { bounce(b); });
        else if (n_levels >= 1) E.timed(kStageShade, [&] { for (int b = 1; b <= n_levels; ++b) bounce(b); });
        n_launches += 2 + n_levels;                                 // k_primary, the levels, k_resolve
        if (!p.simple) for (int k = 0; k < ft_context::kAcc; ++k) if (c->acc_busy[k]) {   // a queued frame's k_resolve may still be writing the frame on `tail`: frames reach d_out in order
            FT_HIP(c, hipStreamWaitEvent(ms, c->acc_free[k], 0)); c->acc_busy[k] = false; E.fresh = false;
        }
        if (p.corner) { E.timed(kStageResolve, [&] { ftk::launch_resolve_corner(Lg, acc, n_samples, job.w, job.h, c->d_out_index.as<uint32_t>() + job.out_base, out_rgb, out_rgba); }); continue; }
        const ftk::ResolveArgs ra{acc, n_samples, p.classify ? &fc->counts : nullptr, job.id_base, n_pix, p.spp,
                                  p.classify ? F.d_pos_block.as<uint32_t>() : nullptr, (p.classify && first && !zeros_in_place) ? F.d_block_pos.as<int32_t>() : nullptr,
                                  (uint32_t)(p.n_pix_total / 64), c->d_pixels.as<uint32_t>(), out_rgb, out_rgba, (uint32_t)gen.group_log2, fc, last ? F.d_report : nullptr};
        if (p.progressive) {
            ft_context::Progressive& P = c->prog;
            const int in = P.cur, out = P.cur ^ 1;
            const ftk::ProgressiveArgs pa{P.d_sum[in].as<double>(), P.d_sum[out].as<double>(), P.d_sq[in].as<double>(), P.d_sq[out].as<double>(),
                                          P.d_blk[in].as<uint32_t>(), P.d_blk[out].as<uint32_t>(), (uint32_t)P.n_pix, (uint32_t)P.min_samples, P.tolerance};
            ftk::ResolveArgs rp = ra;
            rp.block_pos = p.classify && first ? F.d_block_pos.as<int32_t>() : nullptr;   // every block the pass does not trace, every pass
            E.timed(kStageResolve, [&] { ftk::launch_resolve_progressive(Lr, rp, pa); });
        } else if (p.simple) {
            // behind the frame's tracing kernels, on its own stream: the main stream goes straight on with the next frame.  Where the
            // tracing ends: the event that closed its last bracket, if that is still the stream's last entry.
            hipEvent_t traced = E.fresh ? E.boundary : nullptr;
            if (!traced) { if (!(traced = E.next())) { c->err = "hipEventCreate failed"; return FT_ERR_HIP; } FT_HIP(c, hipEventRecord(traced, ms)); }
            FT_HIP(c, hipStreamWaitEvent(c->tail, traced, 0));
            ftk::Launch La = Lr; La.stream = c->tail;
            ftk::launch_resolve(La, ra);
            if (!c->acc_free[at]) FT_HIP(c, hipEventCreateWithFlags(&c->acc_free[at], hipEventDisableTiming));
            FT_HIP(c, hipEventRecord(c->acc_free[at], c->tail));
            c->acc_busy[at] = true;
            c->acc_turn = (c->acc_turn + 1) % ft_context::kAcc;
            E.fresh = false;
        } else E.timed(kStageResolve, [&] { ftk::launch_resolve(Lr, ra); });
        if (last) F.fc_clean = true;
    }
    if (!F.fc_clean) { ftk::launch_report(Lg, fc, F.d_report); F.fc_clean = true; }   // corner frames end in k_resolve_corner: the hand-over is a launch of its own
    return FT_OK;
}

// Queue a planned frame: its inputs, its slot and main stream, the classification and the chunks.  A blocking frame is then retired
// (and fetched into `out`); a queued one is retired by a later call.
static int32_t queue_frame(ft_context* c, const RenderRequest& q, const FramePlan& p, void* out, ft_stats* stats, bool defer,
                           std::chrono::steady_clock::time_point wall0) {
    int32_t rc;
    bool uploads_queued = false;
    if ((rc = upload_frame_inputs(c, q, p, uploads_queued)) != FT_OK) return rc;
    // A blocking call retires whatever is in flight first; a deferred one only the frame whose slot (host state, counters, classification
    // buffers) it is about to reuse.
    if (!defer && (rc = retire_pending(c, nullptr)) != FT_OK) return rc;
    const int turn = c->slot_turn;
    ft_context::FrameSlot& F = c->slots[turn];
    if (F.pending && (rc = retire_frame(c, F, nullptr)) != FT_OK) return rc;
    if (!defer || !c->accum_open) { for (int k = 0; k < kStages; ++k) { c->k_ms[k] = 0; c->k_launches[k] = 0; } c->accum_open = defer; }   // queued frames sum their kernel times until a wait
    if (p.classify) {
        const size_t n_blocks = (size_t)p.n_pix_total / 64, n_waves = (n_blocks + 255) / 256;   // one word per k_classify workgroup
        if ((rc = ensure(c, F.d_block_pos, n_blocks * 4)) != FT_OK) return rc;
        if ((rc = ensure(c, F.d_pos_block, n_blocks * 4)) != FT_OK) return rc;
        if (c->d_wave_counts.bytes < n_waves * 4 || c->classify_epoch >= 0x3FFFFEu) {   // entries are tagged with the frame's epoch and never cleared in between
            if ((rc = ensure(c, c->d_wave_counts, std::max<size_t>(n_waves * 4, 4096) + 4096 * 4 + 2048 * 64)) != FT_OK) return rc;   // (+ room for the diagnostic build's stamps)
            FT_HIP(c, hipStreamSynchronize(c->side));              // (a classification of the other slot may still be publishing into the old words)
            FT_HIP(c, hipMemsetAsync(c->d_wave_counts.p, 0, c->d_wave_counts.bytes, c->stream));
            c->classify_epoch = 0;
            uploads_queued = true;
        }
    }
    // Which main stream.  Two consecutive k_primary launches on ONE stream are an in-order pair: the second is dispatched when the first has
    // drained, and a persistent grid drains slowly (its last batches run on a machine that is mostly idle).  A simple frame - one chunk,
    // k_resolve aside - shares nothing with its predecessor that events do not already order (sample colours: acc_free; counters and
    // classification: per slot; the frame buffer: the tail stream; ray buffers: a pair per main stream), so every other one goes to the second main stream and its
    // workgroups take the CUs as the predecessor's leave them.
    const ft_context::FrameSlot& prev = c->slots[(turn + ft_context::kSlots - 1) % ft_context::kSlots];
    if (!p.simple && any_pending(c, true) && (rc = retire_pending(c, nullptr)) != FT_OK) return rc;   // anything else keeps the one-stream order
    const int main_ix = (p.simple && c->opt.mains > 1 && !uploads_queued && prev.pending && prev.simple) ? (prev.main_ix + 1) % (int)c->opt.mains : 0;   // the next stream after its predecessor's
    const hipStream_t ms = main_ix ? c->more_mains[main_ix - 1] : c->stream;
    // chunk counters, statistic stripes, list length, tickets: cleared by the slot's previous frame's last kernel, or by a fill when there was none
    if (!F.fc_clean) { FT_HIP(c, hipMemsetAsync(F.d_fc.p, 0, sizeof(ftk::FrameCounters), ms)); uploads_queued = true; }
    F.fc_clean = false;                                            // until this frame's own hand-over is queued
    F.ev.begin(ms, (int)c->opt.timing);
    if (p.classify && (rc = queue_classify(c, q, p, F, defer && c->opt.classify_ahead && !uploads_queued)) != FT_OK) return rc;
    if (!F.h_report) {
        FT_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&F.h_report), sizeof(ftk::FrameReport), hipHostMallocDefault));
        FT_HIP(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&F.d_report), F.h_report, 0));
    }
    int32_t n_launches = p.classify ? 1 : 0;
    if ((rc = queue_chunks(c, q, p, F, main_ix, n_launches)) != FT_OK) return rc;
    c->last_n_pix = p.n_pix_total; c->last_res_h = q.res_h; c->last_res_v = q.res_v; c->last_format = q.format;
    if (defer && out) {                                            // ft_render_enqueue_into: the frame's way out is queued behind its last kernel
        if ((rc = copy_frame_out(c, out, q.format, p.simple ? c->tail : ms)) != FT_OK) return rc;
        F.ev.fresh = false;
    }
    F.ev.open();
    if (p.simple) F.ev.ev1 = F.ev.record(c->tail);                // the frame ends where its last k_resolve (and copy) does
    else F.ev.ev1 = F.ev.fresh ? F.ev.boundary : F.ev.record(ms);
    FT_HIP(c, hipGetLastError());
    F.signature = p.signature; F.simple = p.simple; F.main_ix = main_ix;
    F.pending = true; F.wall0 = wall0;
    F.rays_primary = 0; for (auto& j : p.jobs) F.rays_primary += (uint64_t)j.n_ids * (uint64_t)p.spp;
    F.n_pix_total = p.n_pix_total; F.spp = p.spp; F.n_launches = n_launches; F.n_chunks = (int32_t)p.jobs.size(); F.classify = p.classify; F.format = q.format;
    c->slot_turn = (c->slot_turn + 1) % ft_context::kSlots;
    if (defer) return FT_OK;                                       // ft_render_enqueue: the frame is retired by a later call
    if ((rc = retire_frame(c, F, stats)) != FT_OK) return rc;
    if (out && (rc = fetch_single(c, out, q.format)) != FT_OK) return rc;   // out == NULL: the frame stays in HBM
    if (stats) stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    return FT_OK;
}

static int32_t render_single(ft_context* c, const RenderRequest& q, void* out, ft_stats* stats, bool defer) {
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    if (!c->committed) { c->err = "scene not committed (ft_scene_commit)"; return FT_ERR_STATE; }
    const auto wall0 = std::chrono::steady_clock::now();
    FT_HIP(c, hipSetDevice(c->device));
    FramePlan p;
    plan_pixels(c, q, p);
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (p.n_pix_total == 0) return FT_OK;
    if (q.progressive && p.n_pix_total != c->prog.n_pix) { c->err = "progressive pass: the pixel list differs from the accumulation's"; return FT_ERR_STATE; }
    plan_chunks(c, q, defer, p);
    if (p.cap > 0x7FFFFFFFll) { c->err = "chunk too large"; return FT_ERR_INVALID; }
    if (p.classify && p.progressive && p.jobs.size() > 1 && p.pix_per_chunk % 64) { c->err = "progressive pass: too many samples per pass for whole-block windows"; return FT_ERR_UNSUPPORTED; }
    return queue_frame(c, q, p, out, stats, defer, wall0);
}

// Wait for a queued frame, add its stage times to the context's sums and fill its statistics.
static int32_t retire_frame(ft_context* c, ft_context::FrameSlot& F, ft_stats* stats) {
    if (!F.pending) return FT_OK;
    F.pending = false;
    if (F.ev.ev1) FT_HIP(c, hipEventSynchronize(F.ev.ev1)); else FT_HIP(c, hipStreamSynchronize(c->stream));
    const ftk::RenderCounters hrc = F.h_report->total;              // the stripes, summed by the frame's last kernel
    const bool classify_failed = F.h_report->classify_error != 0;
    // How deep this frame's rays went in numbers worth a launch (more than "follow_below" rays; levels followed in registers count
    // theirs too): the next frame of the same signature launches that many levels + 1, and that last one follows what is left.
    int deepest = 0;
    const int64_t few = c->opt.follow_below >= 0 ? c->opt.follow_below : 8ll * c->n_cu;   // -1: two rays per SIMD
    while (deepest + 1 <= ftk::kMaxBounce && (int64_t)F.h_report->n_rays[deepest + 1] > few) ++deepest;
    c->staged_hint = deepest; c->staged_signature = F.signature;
    const int timing = F.ev.timing; const int32_t spp = F.spp; const int64_t n_pix_total = F.n_pix_total; const bool classify = F.classify;
    c->last_active_pix = classify ? (int64_t)F.h_report->n_pix_active : n_pix_total;
    hipEvent_t ev0 = F.ev.ev0, ev1 = F.ev.ev1;
    double bracketed = 0.0, traced = 0.0;
    for (auto& s : F.ev.spans) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, s.a, s.b) != hipSuccess) continue;
        c->k_ms[s.kind] += ms; c->k_launches[s.kind]++; bracketed += ms;
        if (s.kind == kStageClosest || s.kind == kStageShade || s.kind == kStagePrimary) traced += ms;
    }
    float total = 0;
    if (ev0 && ev1) (void)hipEventElapsedTime(&total, ev0, ev1);
    if (timing < 2) c->k_ms[kStageOther] += std::max(0.0, (double)total - bracketed);   // everything that was not bracketed: the fill, k_classify, k_resolve
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        stats->rays_primary = F.rays_primary;
        stats->rays_shadow = hrc.rays_shadow; stats->rays_reflect = hrc.rays_reflect;
        // rays the device really traced: primaries of pixel blocks k_classify finished (Colour.Zero for the whole block, no ray generated)
        // are part of rays_primary and of the reference-equivalent count, not of rays_traced
        stats->rays_primary_culled = (uint64_t)hrc.pixels_culled * (uint64_t)spp;
        stats->rays_traced = stats->rays_primary - std::min<uint64_t>(stats->rays_primary, stats->rays_primary_culled) + stats->rays_shadow + stats->rays_reflect;
        stats->rays_reference_equivalent = (double)stats->rays_primary + hrc.ref_equiv;
        stats->hits_primary = hrc.hits_primary; stats->csg_overflow = hrc.csg_overflow;
        stats->rays_shadow_primary = hrc.rays_shadow_primary; stats->rays_reflect_primary = hrc.rays_reflect_primary;
        stats->kernel_ms = total; stats->trace_kernel_ms = traced;
        {   // Bytes the pipeline has to move by construction of its data layout (ft_device.h).  P generated primaries, Rp / R
            // reflection rays spawned by k_primary / in all, Hb hits shaded by the k_bounce levels.
            const uint64_t P = stats->rays_primary - std::min<uint64_t>(stats->rays_primary, stats->rays_primary_culled);
            const uint64_t RR = hrc.rays_reflect, Rp = hrc.rays_reflect_primary;
            const uint64_t Hb = hrc.hits_total - std::min(hrc.hits_total, hrc.hits_primary);     // hits shaded by k_bounce
            stats->hits_total = hrc.hits_total;
            stats->rays_tail = 0;
            stats->algorithmic_bytes_primary = P * (ftk::kPixelIdBytes + ftk::kAccBytes) + Rp * ftk::kRayRecBytes;
            stats->algorithmic_bytes_closest = 0;
            stats->algorithmic_bytes_shade = RR * ftk::kRayRecBytes + Hb * 2 * ftk::kAccBytes + (RR - std::min(RR, Rp)) * ftk::kRayRecBytes;   // k_bounce: rays in, colours read-modify-written, rays out
            const uint64_t out_px = F.format == 1 ? 4 : 24, blocks = (uint64_t)n_pix_total / 64;
            stats->algorithmic_bytes = stats->algorithmic_bytes_primary + stats->algorithmic_bytes_shade +
                                       P * ftk::kAccBytes + out_px * (uint64_t)n_pix_total + 4 * (uint64_t)n_pix_total +  // + k_resolve: samples in, pixels out, pixel ids
                                       (classify ? blocks * 16 : 0ull);                                                 // + k_classify: two ids in, two words out per block
        }
        stats->n_launches = F.n_launches; stats->n_chunks = F.n_chunks;
        stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - F.wall0).count();
    }
    if (classify_failed) { c->err = "k_classify: a bounded wait ran out (device error)"; return FT_ERR_HIP; }
    if (hrc.csg_overflow) {
        c->err = "CSG hit list overflow on " + std::to_string(hrc.csg_overflow) + " rays: raise csg_mesh_capacity (ft_set_option)";
        return FT_ERR_OVERFLOW;
    }
    return FT_OK;
}

// Retire every queued frame, oldest first; `stats` receives the newest one's.
static int32_t retire_pending(ft_context* c, ft_stats* stats) {
    int32_t rc = FT_OK;
    int last = -1;
    for (int k = 0; k < ft_context::kSlots; ++k) if (c->slots[(c->slot_turn + k) % ft_context::kSlots].pending) last = k;
    for (int k = 0; k < ft_context::kSlots; ++k) {                  // oldest first; the statistics asked for are the newest frame's
        ft_context::FrameSlot& f = c->slots[(c->slot_turn + k) % ft_context::kSlots];
        if (f.pending) { int32_t r = retire_frame(c, f, k == last ? stats : nullptr); if (r != FT_OK) rc = r; }
    }
    return rc;
}

/* Pipelined rendering: queue the frame and return; see functracer_hip.h.  On a context over several devices every device queues
 * its bands of the frame on its own stream. */
static int32_t enqueue(ft_context* c, const RenderRequest& q) {
    if (!c) return FT_ERR_INVALID;
    return render_frame(c, q, nullptr, nullptr, true);
}
int32_t ft_render_enqueue(ft_context* c, const ft_camera* cam, int32_t res_h, int32_t res_v, int32_t spp, const double* jitter_xy,
                          int32_t max_depth, uint64_t seed, const ft_rect* tiles, int32_t n_tiles) {
    return enqueue(c, RenderRequest{cam, res_h, res_v, spp, jitter_xy, max_depth, seed, tiles, n_tiles, 0});
}
int32_t ft_render_enqueue_rgba8(ft_context* c, const ft_camera* cam, int32_t res_h, int32_t res_v, int32_t spp, const double* jitter_xy,
                                int32_t max_depth, uint64_t seed, const ft_rect* tiles, int32_t n_tiles) {
    return enqueue(c, RenderRequest{cam, res_h, res_v, spp, jitter_xy, max_depth, seed, tiles, n_tiles, 1});
}
/* A queued frame that also leaves the device: the copy into host_out (res_v x res_h x 3 doubles, or x 4 bytes with rgba8 != 0) is queued
 * behind the frame's last kernel and is complete when ft_render_wait returns (or when a later call retires the frame).  host_out should
 * come from ft_host_alloc: the copy is then one DMA beside the next frame's tracing - a stream of RGBA8 frames reaches the host at the
 * rate the device renders them. */
int32_t ft_render_enqueue_into(ft_context* c, const ft_camera* cam, int32_t res_h, int32_t res_v, int32_t spp, const double* jitter_xy,
                               int32_t max_depth, uint64_t seed, const ft_rect* tiles, int32_t n_tiles, int32_t rgba8, void* host_out) {
    if (!c || !host_out) return FT_ERR_INVALID;
    return render_frame(c, RenderRequest{cam, res_h, res_v, spp, jitter_xy, max_depth, seed, tiles, n_tiles, rgba8 ? 1 : 0}, host_out, nullptr, true);
}
int32_t ft_render_wait(ft_context* c, ft_stats* stats) {
    if (!c) return FT_ERR_INVALID;
    if (c->host_only) return FT_ERR_NO_DEVICE;
    if (stats) std::memset(stats, 0, sizeof *stats);
    int32_t rc = FT_OK;
    for (ft_context* d : devices(c)) {
        FT_HIP(c, hipSetDevice(d->device));
        ft_stats sd;
        std::memset(&sd, 0, sizeof sd);
        const int32_t r = retire_pending(d, &sd);
        d->accum_open = false;
        if (r != FT_OK && rc == FT_OK) { rc = r; if (d != c) c->err = d->err; }
        if (stats) { const double wall = std::max(stats->wall_ms, sd.wall_ms); add_stats(stats, sd); stats->wall_ms = wall; }
    }
    return rc;
}

// ------------------------------------------------------------------------------------------ progressive accumulation
// A progressive render is a run of blocking frames over one fixed request whose k_resolve goes on from each pixel's running sum
// (k_resolve_progressive): the sum of a pixel's samples in pass order, then sample order, is the sum one ft_render over the concatenated
// pattern forms, so the mean S / n is that frame bit for bit.  See functracer_hip.h.
static const double kNoJitter[2] = {0.0, 0.0};
static RenderRequest progressive_request(const ft_context::Progressive& P) {
    return RenderRequest{&P.cam, P.res_h, P.res_v, 1, kNoJitter, P.max_depth, 0, P.tiles.data(), (int32_t)P.tiles.size(), 0, true};
}

int32_t ft_progressive_begin(ft_context* c, const ft_camera* cam, int32_t res_h, int32_t res_v, int32_t max_depth, const ft_rect* tiles, int32_t n_tiles,
                             double tolerance, int32_t min_samples) {
    if (!c) return FT_ERR_INVALID;
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    const RenderRequest q{cam, res_h, res_v, 1, kNoJitter, max_depth, 0, tiles, n_tiles, 0};
    int32_t rc = check_request(c, q);
    if (rc != FT_OK) return rc;
    if (tolerance != tolerance) { c->err = "progressive tolerance is NaN"; return FT_ERR_INVALID; }
    const bool adaptive = tolerance > 0.0;
    if (adaptive && min_samples < 2) { c->err = "an adaptive progressive render needs min_samples >= 2 (a standard error needs two samples)"; return FT_ERR_INVALID; }
    if (adaptive) for (const ft_rect& r : clip_rects(q))
        if (r.w % 8 || r.h % 8) { c->err = "adaptive progressive rendering retires 8x8 blocks: every clipped tile needs sides that are multiples of 8"; return FT_ERR_UNSUPPORTED; }
    if (!c->committed) { c->err = "scene not committed (ft_scene_commit)"; return FT_ERR_STATE; }
    progressive_close(c);                                           // a second begin replaces the first
    const std::vector<ft_context*> devs = devices(c);
    const std::vector<std::vector<ft_rect>> share = devs.size() > 1 ? band_shares(q, devs.size()) : std::vector<std::vector<ft_rect>>{clip_rects(q)};
    for (size_t d = 0; d < devs.size(); ++d) {
        ft_context* D = devs[d];
        ft_context::Progressive& P = D->prog;
        P.open = true;
        P.cam = *cam; P.res_h = res_h; P.res_v = res_v; P.max_depth = max_depth; P.tolerance = adaptive ? tolerance : 0.0; P.min_samples = adaptive ? min_samples : 0;
        P.tiles = share[d];
        P.n_pix = 0;
        if (!P.tiles.empty()) for (const ft_rect& r : clip_rects(progressive_request(P))) P.n_pix += (int64_t)r.w * r.h;
        P.n_blocks = (P.n_pix + 63) / 64;
        if (P.n_pix == 0) continue;
        const size_t plane_bytes = (size_t)P.n_pix * 24;
        rc = hipSetDevice(D->device) == hipSuccess ? FT_OK : FT_ERR_HIP;
        for (int k = 0; k < 2 && rc == FT_OK; ++k)
            if ((rc = ensure(D, P.d_sum[k], plane_bytes)) != FT_OK || (adaptive && (rc = ensure(D, P.d_sq[k], plane_bytes)) != FT_OK) ||
                (rc = ensure(D, P.d_blk[k], (size_t)P.n_blocks * 4)) != FT_OK) break;
        if (rc == FT_OK && (hipMemsetAsync(P.d_sum[0].p, 0, plane_bytes, D->stream) != hipSuccess || (adaptive && hipMemsetAsync(P.d_sq[0].p, 0, plane_bytes, D->stream) != hipSuccess) ||
                            hipMemsetAsync(P.d_blk[0].p, 0, (size_t)P.n_blocks * 4, D->stream) != hipSuccess || hipStreamSynchronize(D->stream) != hipSuccess)) {
            D->err = "progressive accumulation: clearing the running sums failed"; rc = FT_ERR_HIP;
        }
        if (rc != FT_OK) { if (D != c) c->err = D->err; progressive_close(c); return rc; }
    }
    return FT_OK;
}

int32_t ft_progressive_pass(ft_context* c, int32_t spp, const double* jitter_xy, uint64_t seed, int32_t rgba8, void* out, ft_stats* stats) {
    if (!c) return FT_ERR_INVALID;
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    if (!c->prog.open) { c->err = "no progressive accumulation (ft_progressive_begin; a caller's ft_scene_commit or ft_scene_clear ends it)"; return FT_ERR_STATE; }
    if (spp == 0) { c->err = "a progressive pass needs spp >= 1: corner sampling's blend is not a per-pixel average"; return FT_ERR_UNSUPPORTED; }
    if (spp < 0 || !jitter_xy) { c->err = "bad ft_progressive_pass argument"; return FT_ERR_INVALID; }
    if (c->prog.samples + spp > 0x7FFFFFFFll) { c->err = "more than 2^31 - 1 samples per pixel"; return FT_ERR_INVALID; }
    const auto wall0 = std::chrono::steady_clock::now();
    const std::vector<ft_context*> devs = devices(c);
    std::vector<ft_stats> sts(devs.size());
    // One host thread per device, as render_frame: every device traces its share and copies its bands of the means into `out`.  A hit-list
    // overflow anywhere re-commits and runs the pass again on every device, from the same side of the running sums.
    const int32_t rc = with_growing_hit_lists(c, [&] {
        std::vector<int32_t> rcs(devs.size(), FT_OK);
        on_every_device(c, std::vector<bool>(devs.size(), true), [&](size_t d) {
            ft_context* D = devs[d];
            std::memset(&sts[d], 0, sizeof(ft_stats));
            if (D->prog.n_pix == 0) { D->last_n_pix = 0; return; }
            RenderRequest q = progressive_request(D->prog);
            q.spp = spp; q.jitter_xy = jitter_xy; q.seed = seed; q.format = rgba8 ? 1 : 0;
            rcs[d] = render_single(D, q, out, &sts[d], false);
        });
        for (size_t d = 0; d < devs.size(); ++d) if (rcs[d] != FT_OK) { if (d) c->err = devs[d]->err; return rcs[d]; }
        return (int32_t)FT_OK;
    });
    if (rc != FT_OK) return rc;
    c->prog.passes += 1; c->prog.samples += spp; c->prog.traced = 0;
    for (ft_context* D : devs) if (D->prog.n_pix > 0) { D->prog.cur ^= 1; c->prog.traced += D->last_active_pix * spp; }
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        for (auto& s : sts) add_stats(stats, s);
        stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    }
    return FT_OK;
}

// fn(device, its list's pixel ids, running sums, sums of squares (adaptive only, when `squares`), block words) for every device with pixels.
static int32_t progressive_read(ft_context* c, bool squares, const std::function<void(const ft_context::Progressive&, const std::vector<uint32_t>&,
                                const std::vector<double>&, const std::vector<double>&, const std::vector<uint32_t>&)>& fn) {
    for (ft_context* D : devices(c)) {
        const ft_context::Progressive& P = D->prog;
        if (P.n_pix == 0) continue;
        const size_t n = (size_t)P.n_pix;
        std::vector<double> sum(3 * n), sq(squares ? 3 * n : 0);
        std::vector<uint32_t> blk((size_t)P.n_blocks), px;
        FT_HIP(c, hipSetDevice(D->device));
        FT_HIP(c, hipStreamSynchronize(D->stream));
        FT_HIP(c, hipMemcpy(sum.data(), P.d_sum[P.cur].p, 3 * n * 8, hipMemcpyDeviceToHost));
        if (squares) FT_HIP(c, hipMemcpy(sq.data(), P.d_sq[P.cur].p, 3 * n * 8, hipMemcpyDeviceToHost));
        FT_HIP(c, hipMemcpy(blk.data(), P.d_blk[P.cur].p, blk.size() * 4, hipMemcpyDeviceToHost));
        list_pixels(clip_rects(progressive_request(P)), P.res_h, px);
        fn(P, px, sum, sq, blk);
    }
    return FT_OK;
}

int32_t ft_progressive_fetch(ft_context* c, double* mean_rgb, double* stderr_rgb, uint32_t* samples) {
    if (!c) return FT_ERR_INVALID;
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    if (!c->prog.open) { c->err = "no progressive accumulation (ft_progressive_begin)"; return FT_ERR_STATE; }
    if (stderr_rgb && !(c->prog.tolerance > 0.0)) { c->err = "standard errors are kept by adaptive accumulations only (tolerance > 0)"; return FT_ERR_STATE; }
    return progressive_read(c, stderr_rgb != nullptr, [&](const ft_context::Progressive& P, const std::vector<uint32_t>& px, const std::vector<double>& sum,
                                                         const std::vector<double>& sq, const std::vector<uint32_t>& blk) {
        const size_t n = (size_t)P.n_pix;
        for (size_t i = 0; i < n; ++i) {
            const uint32_t cnt = blk[i >> 6] & ~ftk::kRetired;
            const double dn = (double)cnt;
            const size_t o = px[i];
            for (int ch = 0; ch < 3; ++ch) {
                const double S = sum[(size_t)ch * n + i];
                if (mean_rgb) mean_rgb[3 * o + ch] = cnt ? S / dn : 0.0;
                if (stderr_rgb) {                                   // as k_resolve_progressive judges it
                    double se = 0.0;
                    if (cnt >= 2) { const double m = S / dn, v0 = sq[(size_t)ch * n + i] / dn - m * m, v = (v0 < 0.0 ? 0.0 : v0) * dn / (dn - 1.0); se = std::sqrt(v / dn); }
                    stderr_rgb[3 * o + ch] = se;
                }
            }
            if (samples) samples[o] = cnt;
        }
    });
}

int32_t ft_progressive_status(ft_context* c, int64_t out[6]) {
    if (!c || !out) return FT_ERR_INVALID;
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    if (!c->prog.open) { c->err = "no progressive accumulation (ft_progressive_begin)"; return FT_ERR_STATE; }
    int64_t lo = std::numeric_limits<int64_t>::max(), hi = 0, blocks = 0, retired = 0;
    const int32_t rc = progressive_read(c, false, [&](const ft_context::Progressive& P, const std::vector<uint32_t>&, const std::vector<double>&,
                                                      const std::vector<double>&, const std::vector<uint32_t>& blk) {
        for (uint32_t w : blk) { const int64_t cnt = w & ~ftk::kRetired; lo = std::min(lo, cnt); hi = std::max(hi, cnt); retired += (w & ftk::kRetired) ? 1 : 0; }
        blocks += P.n_blocks;
    });
    if (rc != FT_OK) return rc;
    out[0] = c->prog.passes; out[1] = blocks ? lo : 0; out[2] = hi; out[3] = blocks; out[4] = retired; out[5] = c->prog.traced;
    return FT_OK;
}

int32_t ft_progressive_end(ft_context* c) {
    if (!c) return FT_ERR_INVALID;
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    progressive_close(c);
    return FT_OK;
}

int32_t ft_get_kernel_times(ft_context* c, double ms[5], int32_t launches[5]) {
    if (!c || !ms || !launches) return FT_ERR_INVALID;
    for (int k = 0; k < kStages; ++k) { ms[k] = c->k_ms[k]; launches[k] = c->k_launches[k]; }
    for (ft_context* p : c->peers) for (int k = 0; k < kStages; ++k) { ms[k] = std::max(ms[k], p->k_ms[k]); launches[k] = std::max(launches[k], p->k_launches[k]); }   // the slowest device's
    return FT_OK;
}

// ------------------------------------------------------------------------------------------ per-pixel surface buffers
// ft_render_aov: the hit of one sample's geometry ray per tile pixel (functracer_hip.h).  The call keeps to buffers of its own - pixel
// list, jitter pattern, planes, counters - so the frame buffer, the cached pixel list, the zero-fill and level-hint history and a
// progressive accumulation stay as they were.  The list is ft_render's (8x8 blocks in Z order where the rects allow), cut into windows
// of "chunk_samples" entries; per window one k_aov writes the requested planes by list position and the host scatters them into the
// caller's frame-shaped planes.
namespace {
struct AovPlanes { int64_t off[8]; int width[8]; size_t bytes_per_entry; };   // t, p, n, colour, material, leaf, node, triangle
AovPlanes aov_planes(const bool (&want)[8], int64_t per) {
    AovPlanes a{};
    const int width[8] = {1, 3, 3, 3, 3, 1, 1, 1};
    int64_t at = 0;                                                 // bytes; doubles first, then the 32-bit planes
    for (int k = 0; k < 8; ++k) {
        a.off[k] = -1; a.width[k] = width[k];
        if (!want[k]) continue;
        a.off[k] = at;
        at += per * width[k] * (k < 5 ? 8 : 4);
        a.bytes_per_entry += (size_t)width[k] * (k < 5 ? 8 : 4);
    }
    return a;
}
struct AovRun { int64_t n_pix = 0; unsigned long long hits = 0; double kernel_ms = 0.0; int32_t n_launches = 0; };
} // namespace

// The device half of an AOV pass, shared by ft_render_aov and ft_denoise: the pixel list `px` and the pattern go up, and per window of
// "chunk_samples" entries one k_aov writes the wanted planes into d_aov_out by position in the window.  consume(p0, n, planes, dev) then
// sees the window [p0, p0 + n) with its planes still in HBM, behind the kernel on the context's stream - it copies them out, or queues a
// kernel that reads them.  The stream is drained after every window (the next one overwrites the planes' buffer and the event pair).
static int32_t aov_windows(ft_context* c, const RenderRequest& q, int32_t sample, const bool (&want)[8], const std::vector<uint32_t>& px, AovRun& run,
                           const std::function<int32_t(int64_t, uint32_t, const AovPlanes&, char*)>& consume) {
    int32_t rc;
    const int64_t n_pix = (int64_t)px.size();
    run = AovRun{};
    run.n_pix = n_pix;
    if (n_pix == 0) return FT_OK;
    int64_t per = std::max<int64_t>(1, std::min<int64_t>(n_pix, c->opt.chunk_samples));
    if (per > 64) per -= per % 64;                                  // windows of whole 8x8 blocks
    const AovPlanes pl = aov_planes(want, per);
    if ((rc = upload(c, c->d_aov_pixels, px)) != FT_OK) return rc;
    if ((rc = upload(c, c->d_aov_jitter, std::vector<double>(q.jitter_xy, q.jitter_xy + 2 * (size_t)q.spp))) != FT_OK) return rc;
    if ((rc = ensure(c, c->d_aov_out, (size_t)per * pl.bytes_per_entry)) != FT_OK) return rc;
    if ((rc = ensure(c, c->d_aov_ctr, 2 * sizeof(unsigned long long))) != FT_OK) return rc;
    FT_HIP(c, hipMemsetAsync(c->d_aov_ctr.p, 0, 2 * sizeof(unsigned long long), c->stream));
    const ftk::Camera cam = make_camera(*q.cam, q.res_h, q.res_v);
    const size_t lds = lds_bytes_for(c->flat);
    const ftk::Launch L{c->stream, c->n_cu * c->blocks_aov, lds, c->variant};
    const ftk::AovSource src{c->d_scene[kTriSrc].as<uint32_t>(), c->d_scene[kRunNodes].as<int32_t>()};
    char* const dev = c->d_aov_out.as<char>();
    hipEvent_t* const ev = c->aov_ev;
    for (int k = 0; k < 2; ++k) if (!ev[k]) FT_HIP(c, hipEventCreate(&ev[k]));
    for (int64_t p0 = 0; p0 < n_pix; p0 += per) {
        const uint32_t n = (uint32_t)std::min<int64_t>(per, n_pix - p0);
        ftk::Primary gen{cam, c->d_aov_pixels.as<uint32_t>(), c->d_aov_jitter.as<double>(), (uint32_t)p0, n, q.spp, (uint32_t)q.res_h, (unsigned long long)q.seed,
                         1.0 / (double)n, 1.0 / (double)q.res_h, nullptr, nullptr};
        gen.group_log2 = 0;
        auto plane = [&](int k) -> void* { return pl.off[k] < 0 ? nullptr : dev + pl.off[k]; };
        const ftk::AovOut out{static_cast<double*>(plane(0)), static_cast<double*>(plane(1)), static_cast<double*>(plane(2)), static_cast<double*>(plane(3)),
                              static_cast<double*>(plane(4)), static_cast<int32_t*>(plane(5)), static_cast<int32_t*>(plane(6)), static_cast<int32_t*>(plane(7)), n};
        FT_HIP(c, hipEventRecord(ev[0], c->stream));
        ftk::launch_aov(L, c->dev_scene, gen, (uint32_t)sample, src, out, c->d_aov_ctr.as<unsigned long long>());
        FT_HIP(c, hipGetLastError());
        FT_HIP(c, hipEventRecord(ev[1], c->stream));
        ++run.n_launches;
        if ((rc = consume(p0, n, pl, dev)) != FT_OK) return rc;
        FT_HIP(c, hipStreamSynchronize(c->stream));
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) run.kernel_ms += ms;
    }
    unsigned long long ctr[2] = {0, 0};
    FT_HIP(c, hipMemcpy(ctr, c->d_aov_ctr.p, sizeof ctr, hipMemcpyDeviceToHost));
    if (ctr[1]) { c->err = "CSG hit list overflow"; return FT_ERR_OVERFLOW; }
    run.hits = ctr[0];
    return FT_OK;
}

static int32_t aov_single(ft_context* c, const RenderRequest& q, int32_t sample, const ft_aov& o, ft_stats* stats) {
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    if (!c->committed) { c->err = "scene not committed (ft_scene_commit)"; return FT_ERR_STATE; }
    const auto wall0 = std::chrono::steady_clock::now();
    FT_HIP(c, hipSetDevice(c->device));
    int32_t rc;
    if (any_pending(c) && (rc = retire_pending(c, nullptr)) != FT_OK) return rc;
    if (stats) std::memset(stats, 0, sizeof *stats);
    std::vector<uint32_t> px;
    (void)list_pixels(clip_rects(q), q.res_h, px);
    if (px.empty()) return FT_OK;
    void* const dst[8] = {o.t, o.p, o.n, o.colour, o.material, o.leaf, o.node, o.triangle};
    bool want[8];
    for (int k = 0; k < 8; ++k) want[k] = dst[k] != nullptr;
    std::vector<char> host;
    AovRun run;
    rc = aov_windows(c, q, sample, want, px, run, [&](int64_t p0, uint32_t n, const AovPlanes& pl, char* dev) -> int32_t {
        size_t need = 0;                                            // the planes keep the offsets of a full window
        for (int k = 0; k < 8; ++k) if (pl.off[k] >= 0) need = std::max(need, (size_t)pl.off[k] + (size_t)n * pl.width[k] * (k < 5 ? 8 : 4));
        if (host.size() < need) host.resize(need);
        for (int k = 0; k < 8; ++k) if (pl.off[k] >= 0) {          // a channel's planes lie back to back: n entries apart within the window
            const size_t esz = k < 5 ? 8 : 4;
            FT_HIP(c, hipMemcpyAsync(host.data() + pl.off[k], dev + pl.off[k], (size_t)n * pl.width[k] * esz, hipMemcpyDeviceToHost, c->stream));
        }
        FT_HIP(c, hipStreamSynchronize(c->stream));
        for (int k = 0; k < 8; ++k) if (pl.off[k] >= 0) {          // into the caller's planes: frame layout, row 0 = top, w components per pixel
            const int w = pl.width[k];
            const char* src_k = host.data() + pl.off[k];
            if (k < 5) {
                const double* s = reinterpret_cast<const double*>(src_k);
                double* d = static_cast<double*>(dst[k]);
                for (uint32_t i = 0; i < n; ++i) { const size_t id = px[(size_t)p0 + i]; for (int a = 0; a < w; ++a) d[id * w + a] = s[(size_t)a * n + i]; }
            } else {
                const int32_t* s = reinterpret_cast<const int32_t*>(src_k);
                int32_t* d = static_cast<int32_t*>(dst[k]);
                for (uint32_t i = 0; i < n; ++i) d[px[(size_t)p0 + i]] = s[i];
            }
        }
        return FT_OK;
    });
    if (rc != FT_OK) return rc;
    if (stats) {
        stats->rays_primary = (uint64_t)run.n_pix; stats->hits_primary = run.hits;
        stats->kernel_ms = run.kernel_ms; stats->n_launches = run.n_launches;
        stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    }
    return FT_OK;
}

static int32_t aov_frame(ft_context* c, const RenderRequest& q, int32_t sample, const ft_aov& o, ft_stats* stats) {
    if (c->peers.empty()) return aov_single(c, q, sample, o, stats);
    if (!c->committed) { c->err = "scene not committed (ft_scene_commit)"; return FT_ERR_STATE; }
    const auto wall0 = std::chrono::steady_clock::now();
    const std::vector<ft_context*> devs = devices(c);
    const std::vector<std::vector<ft_rect>> share = band_shares(q, devs.size());   // ft_render's 8-row bands: each device writes its rows
    std::vector<int32_t> rcs(devs.size(), FT_OK);
    std::vector<ft_stats> sts(devs.size());
    on_every_device(c, std::vector<bool>(devs.size(), true), [&](size_t d) {
        std::memset(&sts[d], 0, sizeof(ft_stats));
        if (share[d].empty()) return;
        RenderRequest qd = q;
        qd.tiles = share[d].data(); qd.n_tiles = (int32_t)share[d].size();
        rcs[d] = aov_single(devs[d], qd, sample, o, &sts[d]);
    });
    for (size_t d = 0; d < devs.size(); ++d) if (rcs[d] != FT_OK) { if (d) c->err = devs[d]->err; return rcs[d]; }
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        for (auto& s : sts) add_stats(stats, s);
        stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    }
    return FT_OK;
}

int32_t ft_render_aov(ft_context* c, const ft_camera* cam, int32_t res_h, int32_t res_v, int32_t spp, const double* jitter_xy,
                      int32_t sample, uint64_t seed, const ft_rect* tiles, int32_t n_tiles, const ft_aov* out, ft_stats* stats) {
    if (!c) return FT_ERR_INVALID;
    const RenderRequest q{cam, res_h, res_v, spp, jitter_xy, 0, seed, tiles, n_tiles, 0};
    int32_t rc = check_request(c, q);
    if (rc != FT_OK) return rc;
    if (spp == 0) { c->err = "ft_render_aov: corner sampling (spp == 0) has no per-sample geometry ray"; return FT_ERR_UNSUPPORTED; }
    if (sample < 0 || sample >= spp) { c->err = "ft_render_aov: sample outside [0, spp)"; return FT_ERR_INVALID; }
    if (!out || !(out->t || out->p || out->n || out->colour || out->material || out->leaf || out->node || out->triangle)) { c->err = "ft_render_aov: no channel requested"; return FT_ERR_INVALID; }
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    return with_growing_hit_lists(c, [&] { return aov_frame(c, q, sample, *out, stats); });
}

// ------------------------------------------------------------------------------------------ denoising the frame in HBM
// ft_denoise (functracer_hip.h).  The guide pass is ft_render_aov's (aov_windows: n, p, colour, leaf), but its windows
// never leave the device: k_denoise_scatter turns each into frame-layout guide records and u_0 = c / d.  Then one k_denoise per
// iteration alternates between two colour buffers; the last one multiplies d back.  Only buffers of the call's own are written: d_out is
// read, the cached pixel list, signatures, level hint and a progressive accumulation are not touched.
static int32_t denoise_single(ft_context* c, const RenderRequest& q, int32_t sample, const ft_denoise_params& P, bool rgba8, void* out, ft_stats* stats) {
    const auto wall0 = std::chrono::steady_clock::now();
    FT_HIP(c, hipSetDevice(c->device));
    int32_t rc;
    if (any_pending(c) && (rc = retire_pending(c, nullptr)) != FT_OK) return rc;
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (c->last_n_pix <= 0 || c->last_format != 0 || c->last_res_h != q.res_h || c->last_res_v != q.res_v) {
        c->err = c->last_n_pix <= 0 ? "ft_denoise: no frame rendered yet" : c->last_format != 0 ? "ft_denoise: the frame in HBM is RGBA8 (ft_render_rgba8); the filter needs the FP64 frame"
                                                                                                   : "ft_denoise: the frame in HBM has another size";
        return FT_ERR_STATE;
    }
    const std::vector<ft_rect> rects = clip_rects(q);
    const ft_context::Progressive& G = c->prog;
    if (P.use_variance) {
        const bool live = G.open && G.tolerance > 0.0 && G.passes > 0 && G.res_h == q.res_h && G.res_v == q.res_v;
        const std::vector<ft_rect> mine = live ? clip_rects(progressive_request(G)) : std::vector<ft_rect>();
        if (!live || mine.size() != rects.size() || (!rects.empty() && std::memcmp(mine.data(), rects.data(), rects.size() * sizeof(ft_rect)) != 0)) {
            c->err = "ft_denoise: use_variance needs a live adaptive progressive accumulation (tolerance > 0, at least one pass) of the same size and tiles";
            return FT_ERR_STATE;
        }
    }
    std::vector<uint32_t> px;
    (void)list_pixels(rects, q.res_h, px);
    if (px.empty()) return FT_OK;
    if (!c->committed) { c->err = "scene not committed (ft_scene_commit)"; return FT_ERR_STATE; }
    FT_HIP(c, hipStreamSynchronize(c->stream));                     // the frame may have been written on another stream (fetch_single)
    for (hipStream_t m : c->more_mains) if (m) FT_HIP(c, hipStreamSynchronize(m));
    FT_HIP(c, hipStreamSynchronize(c->tail));
    const size_t n_px = (size_t)q.res_h * (size_t)q.res_v;
    const double* frame = c->d_out.as<double>();
    const void* result = frame;                                     // zero iterations: the frame itself
    double kernel_ms = 0.0;
    int32_t n_launches = 0;
    AovRun run;
    hipEvent_t* const ev = c->dn_ev;
    for (int k = 0; k < 2; ++k) if (!ev[k]) FT_HIP(c, hipEventCreate(&ev[k]));
    auto elapsed = [&]() -> int32_t {
        FT_HIP(c, hipStreamSynchronize(c->stream));
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) kernel_ms += ms;
        return FT_OK;
    };
    if (rgba8 && (rc = ensure(c, c->d_dn_out8, n_px * 4)) != FT_OK) return rc;
    if (P.iterations > 0) {
        if ((rc = ensure(c, c->d_dn_guides, n_px * ftk::kDenoiseGuideBytes)) != FT_OK) return rc;
        for (int k = 0; k < 2; ++k) if ((rc = ensure(c, c->d_dn_u[k], n_px * 24)) != FT_OK) return rc;
        ftk::DenoiseGuides g{};
        double* plane = c->d_dn_guides.as<double>();
        for (int k = 0; k < 3; ++k) { g.n[k] = plane + (size_t)k * n_px; g.p[k] = plane + (size_t)(3 + k) * n_px; g.d[k] = plane + (size_t)(6 + k) * n_px; }
        g.v = plane + 9 * n_px;
        g.cls = reinterpret_cast<uint8_t*>(plane + 10 * n_px);
        FT_HIP(c, hipMemsetAsync(g.cls, ftk::kDenoiseOutside, n_px, c->stream));
        const bool want[8] = {false, true, true, true, false, true, false, false};   // p, n, colour, leaf
        rc = aov_windows(c, q, sample, want, px, run, [&](int64_t p0, uint32_t n, const AovPlanes& pl, char* dev) -> int32_t {
            ftk::DenoiseScatterArgs a{};
            a.pixel_ids = c->d_aov_pixels.as<uint32_t>(); a.first = (uint32_t)p0; a.n = n;
            a.p_plane = reinterpret_cast<const double*>(dev + pl.off[1]); a.n_plane = reinterpret_cast<const double*>(dev + pl.off[2]);
            a.colour = reinterpret_cast<const double*>(dev + pl.off[3]); a.leaf = reinterpret_cast<const int32_t*>(dev + pl.off[5]); a.stride = n;
            a.frame = frame; a.u0 = c->d_dn_u[0].as<double>(); a.g = g;
            a.demodulate = P.demodulate ? 1 : 0; a.albedo_floor = P.albedo_floor;
            if (P.use_variance) {
                a.sum = G.d_sum[G.cur].as<double>(); a.sq = G.d_sq[G.cur].as<double>(); a.blk = G.d_blk[G.cur].as<uint32_t>();
                a.n_list = (uint32_t)G.n_pix; a.variance_floor = P.variance_floor;
            }
            FT_HIP(c, hipEventRecord(ev[0], c->stream));
            ftk::launch_denoise_scatter(c->stream, a);
            FT_HIP(c, hipGetLastError());
            FT_HIP(c, hipEventRecord(ev[1], c->stream));
            ++n_launches;
            return elapsed();
        });
        if (rc != FT_OK) return rc;
        auto inv_sq = [](double sigma) { return sigma > 0.0 ? 1.0 / (sigma * sigma) : 0.0; };
        FT_HIP(c, hipEventRecord(ev[0], c->stream));
        for (int i = 0; i < P.iterations; ++i) {
            const bool last = i + 1 == P.iterations;
            ftk::DenoiseArgs a{};
            a.u_in = c->d_dn_u[i & 1].as<double>(); a.u_out = c->d_dn_u[(i + 1) & 1].as<double>();
            a.out8 = last && rgba8 ? c->d_dn_out8.as<uint8_t>() : nullptr;
            a.g = g; a.res_h = q.res_h; a.res_v = q.res_v; a.step = 1 << i;
            a.inv_sn2 = inv_sq(P.sigma_normal); a.inv_sp2 = inv_sq(P.sigma_position); a.inv_sc2 = inv_sq(P.sigma_colour * std::ldexp(1.0, -i));
            ftk::launch_denoise(c->stream, a, last);
            ++n_launches;
            if (last) result = rgba8 ? (const void*)a.out8 : (const void*)a.u_out;
        }
        FT_HIP(c, hipGetLastError());
        FT_HIP(c, hipEventRecord(ev[1], c->stream));
        if ((rc = elapsed()) != FT_OK) return rc;
    } else if (rgba8) {
        FT_HIP(c, hipEventRecord(ev[0], c->stream));
        ftk::launch_denoise_quantise(c->stream, frame, c->d_dn_out8.as<uint8_t>(), (uint32_t)n_px);
        FT_HIP(c, hipGetLastError());
        FT_HIP(c, hipEventRecord(ev[1], c->stream));
        ++n_launches;
        if ((rc = elapsed()) != FT_OK) return rc;
        result = c->d_dn_out8.p;
    }
    if ((rc = copy_rects_out(c, out, result, rgba8 ? 4 : 24, q.res_h, rects, nullptr)) != FT_OK) return rc;
    if (stats) {
        stats->rays_primary = (uint64_t)run.n_pix; stats->hits_primary = run.hits;
        stats->kernel_ms = run.kernel_ms + kernel_ms; stats->n_launches = run.n_launches + n_launches;
        stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    }
    return FT_OK;
}

int32_t ft_denoise(ft_context* c, const ft_camera* cam, int32_t res_h, int32_t res_v, int32_t spp, const double* jitter_xy, int32_t sample, uint64_t seed,
                   const ft_rect* tiles, int32_t n_tiles, const ft_denoise_params* params, int32_t rgba8, void* out, ft_stats* stats) {
    if (!c) return FT_ERR_INVALID;
    const RenderRequest q{cam, res_h, res_v, spp, jitter_xy, 0, seed, tiles, n_tiles, 0};
    int32_t rc = check_request(c, q);
    if (rc != FT_OK) return rc;
    if (spp == 0) { c->err = "ft_denoise: corner sampling (spp == 0) has no per-sample geometry ray to take the guides from"; return FT_ERR_UNSUPPORTED; }
    if (sample < 0 || sample >= spp) { c->err = "ft_denoise: sample outside [0, spp)"; return FT_ERR_INVALID; }
    if (!params || !out) { c->err = "ft_denoise: null params or out"; return FT_ERR_INVALID; }
    const ft_denoise_params& P = *params;
    if (P.iterations < 0 || P.iterations > 6) { c->err = "ft_denoise: iterations outside 0 .. 6"; return FT_ERR_INVALID; }
    if (!(P.sigma_colour >= 0.0) || !(P.sigma_normal >= 0.0) || !(P.sigma_position >= 0.0)) { c->err = "ft_denoise: a sigma is negative or NaN (0 switches a term off)"; return FT_ERR_INVALID; }
    if (P.demodulate && !(P.albedo_floor > 0.0)) { c->err = "ft_denoise: demodulate needs albedo_floor > 0"; return FT_ERR_INVALID; }
    if (P.use_variance && !(P.variance_floor > 0.0)) { c->err = "ft_denoise: use_variance needs variance_floor > 0"; return FT_ERR_INVALID; }
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    if (!c->peers.empty()) {
        c->err = "ft_denoise: a context over several devices keeps the frame in 8-row bands on different devices and a tap crosses bands; gathering them is not supported";
        return FT_ERR_UNSUPPORTED;
    }
    return with_growing_hit_lists(c, [&] { return denoise_single(c, q, sample, P, rgba8 != 0, out, stats); });
}

// ------------------------------------------------------------------------------------------ reprojected frame accumulation
// ft_temporal_* (functracer_hip.h).  The guide pass is ft_render_aov's again (aov_windows: p, n, leaf), its windows stay
// on the device, and one k_temporal per window blends the frame's colours with the previous history set and writes the other one.
static ftk::TemporalSet temporal_set(const DeviceBuf& b, size_t n_px) {
    ftk::TemporalSet s{};
    double* plane = b.as<double>();                                 // M, Q and N first: ft_temporal_fetch reads them as one run
    for (int k = 0; k < 3; ++k) { s.m[k] = plane + (size_t)k * n_px; s.q[k] = plane + (size_t)(3 + k) * n_px; s.p[k] = plane + (size_t)(7 + k) * n_px; s.n[k] = plane + (size_t)(10 + k) * n_px; }
    s.len = plane + 6 * n_px;
    s.leaf = reinterpret_cast<int32_t*>(plane + 13 * n_px);
    return s;
}

int32_t ft_temporal_begin(ft_context* c, int32_t res_h, int32_t res_v, const ft_rect* tiles, int32_t n_tiles) {
    if (!c) return FT_ERR_INVALID;
    if (res_h < 2 || res_v < 2 || (tiles && n_tiles < 1) || (int64_t)res_h * res_v > (int64_t)0x7FFFFFFF) { c->err = "bad ft_temporal_begin argument"; return FT_ERR_INVALID; }
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    if (!c->peers.empty()) {
        c->err = "ft_temporal_begin: a context over several devices keeps the frame in 8-row bands on different devices and a tap crosses bands; gathering them is not supported";
        return FT_ERR_UNSUPPORTED;
    }
    temporal_close(c);                                              // a second begin replaces the first
    ft_context::Temporal& T = c->temporal;
    const int32_t rc = [&]() -> int32_t {
        FT_HIP(c, hipSetDevice(c->device));
        const size_t set_bytes = (size_t)res_h * (size_t)res_v * ftk::kTemporalSetBytes;
        int32_t r;
        for (DeviceBuf& b : T.d_set) {                              // N = 0 everywhere: no tap finds history (the rest is cleared with it)
            if ((r = ensure(c, b, set_bytes)) != FT_OK) return r;
            FT_HIP(c, hipMemsetAsync(b.p, 0, set_bytes, c->stream));
        }
        if ((r = ensure(c, T.d_ctr, 2 * sizeof(unsigned long long))) != FT_OK) return r;
        FT_HIP(c, hipStreamSynchronize(c->stream));
        return FT_OK;
    }();
    if (rc != FT_OK) { T.release(); return rc; }
    T.open = true; T.res_h = res_h; T.res_v = res_v;
    T.rects = clip_rects(RenderRequest{nullptr, res_h, res_v, 1, kNoJitter, 0, 0, tiles, n_tiles, 0});
    for (const ft_rect& r : T.rects) T.n_pix += (int64_t)r.w * r.h;
    return FT_OK;
}

static int32_t temporal_single(ft_context* c, const RenderRequest& q, int32_t sample, const ft_temporal_params& P, bool rgba8, void* out, ft_stats* stats) {
    const auto wall0 = std::chrono::steady_clock::now();
    FT_HIP(c, hipSetDevice(c->device));
    int32_t rc;
    if (any_pending(c) && (rc = retire_pending(c, nullptr)) != FT_OK) return rc;
    if (stats) std::memset(stats, 0, sizeof *stats);
    ft_context::Temporal& T = c->temporal;
    if (c->last_n_pix <= 0 || c->last_format != 0 || c->last_res_h != T.res_h || c->last_res_v != T.res_v) {
        c->err = c->last_n_pix <= 0 ? "ft_temporal_accumulate: no frame rendered yet" : c->last_format != 0 ? "ft_temporal_accumulate: the frame in HBM is RGBA8 (ft_render_rgba8); the accumulation needs the FP64 frame"
                                                                                                               : "ft_temporal_accumulate: the frame in HBM has another size than ft_temporal_begin fixed";
        return FT_ERR_STATE;
    }
    std::vector<uint32_t> px;
    (void)list_pixels(T.rects, T.res_h, px);
    if (!c->committed) { c->err = "scene not committed (ft_scene_commit)"; return FT_ERR_STATE; }
    FT_HIP(c, hipStreamSynchronize(c->stream));                     // the frame may have been written on another stream (fetch_single)
    for (hipStream_t m : c->more_mains) if (m) FT_HIP(c, hipStreamSynchronize(m));
    FT_HIP(c, hipStreamSynchronize(c->tail));
    const size_t n_px = (size_t)T.res_h * (size_t)T.res_v;
    const bool want_rgb = P.to_frame || (out && !rgba8), want_rgba8 = out && rgba8;
    if (want_rgb && (rc = ensure(c, T.d_rgb, n_px * 24)) != FT_OK) return rc;
    if (want_rgba8 && (rc = ensure(c, T.d_rgba8, n_px * 4)) != FT_OK) return rc;
    FT_HIP(c, hipMemsetAsync(T.d_ctr.p, 0, 2 * sizeof(unsigned long long), c->stream));
    const ftk::Camera cam = make_camera(*q.cam, T.res_h, T.res_v);
    double kernel_ms = 0.0;
    int32_t n_launches = 0;
    AovRun run;
    hipEvent_t* const ev = c->tp_ev;
    for (int k = 0; k < 2; ++k) if (!ev[k]) FT_HIP(c, hipEventCreate(&ev[k]));
    const bool want[8] = {false, true, true, false, false, true, false, false};   // p, n, leaf
    rc = aov_windows(c, q, sample, want, px, run, [&](int64_t p0, uint32_t n, const AovPlanes& pl, char* dev) -> int32_t {
        ftk::TemporalArgs a{};
        a.pixel_ids = c->d_aov_pixels.as<uint32_t>(); a.first = (uint32_t)p0; a.n = n;
        a.p_plane = reinterpret_cast<const double*>(dev + pl.off[1]); a.n_plane = reinterpret_cast<const double*>(dev + pl.off[2]);
        a.leaf = reinterpret_cast<const int32_t*>(dev + pl.off[5]); a.stride = n;
        a.frame = c->d_out.as<double>();
        a.prev = temporal_set(T.d_set[T.prev], n_px); a.cur = temporal_set(T.d_set[T.prev ^ 1], n_px);
        for (int k = 0; k < 3; ++k) { a.o[k] = T.cam.o[k]; a.i[k] = T.cam.i[k]; a.j[k] = T.cam.j[k]; a.k[k] = T.cam.k[k]; }
        a.tlx = T.cam.tlx; a.tly = T.cam.tly; a.pw = T.cam.pw; a.ph = T.cam.ph;
        a.res_h = T.res_h; a.res_v = T.res_v; a.has_prev = T.calls > 0 ? 1 : 0;
        a.max_history = (double)P.max_history; a.min_normal_dot = P.min_normal_dot;
        a.tol_scale = P.position_tolerance_px * std::max(T.cam.pw, T.cam.ph);
        a.out_rgb = want_rgb ? T.d_rgb.as<double>() : nullptr; a.out8 = want_rgba8 ? T.d_rgba8.as<uint8_t>() : nullptr;
        a.counters = T.d_ctr.as<unsigned long long>();
        FT_HIP(c, hipEventRecord(ev[0], c->stream));
        ftk::launch_temporal(c->stream, a);
        FT_HIP(c, hipGetLastError());
        FT_HIP(c, hipEventRecord(ev[1], c->stream));
        ++n_launches;
        FT_HIP(c, hipStreamSynchronize(c->stream));
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) kernel_ms += ms;
        return FT_OK;
    });
    if (rc != FT_OK) return rc;                                     // nothing was flipped: the history is as it was
    unsigned long long ctr[2] = {0, 0};
    if (!px.empty()) FT_HIP(c, hipMemcpy(ctr, T.d_ctr.p, sizeof ctr, hipMemcpyDeviceToHost));
    if (out && (rc = copy_rects_out(c, out, rgba8 ? T.d_rgba8.p : T.d_rgb.p, rgba8 ? 4 : 24, T.res_h, T.rects, nullptr)) != FT_OK) return rc;
    if (P.to_frame && !px.empty()) {                                // the means replace the tile pixels of the frame, once the call can no longer fail
        const size_t pitch = (size_t)T.res_h * 24;
        for (const ft_rect& r : T.rects) {
            const size_t off = (size_t)r.y0 * pitch + (size_t)r.x0 * 24;
            FT_HIP(c, hipMemcpy2DAsync(c->d_out.as<char>() + off, pitch, T.d_rgb.as<char>() + off, pitch, (size_t)r.w * 24, (size_t)r.h, hipMemcpyDeviceToDevice, c->stream));
        }
        FT_HIP(c, hipStreamSynchronize(c->stream));
        c->zero_signature[0] = 0;                                   // (as a progressive pass: the blocks the last ft_render left as Colour.Zero hold means now)
    }
    T.prev ^= 1; T.cam = cam; T.calls += 1;
    T.with_history = (int64_t)ctr[0]; T.at_max = (int64_t)ctr[1];
    if (stats) {
        stats->rays_primary = (uint64_t)run.n_pix; stats->hits_primary = run.hits;
        stats->kernel_ms = run.kernel_ms + kernel_ms; stats->trace_kernel_ms = run.kernel_ms; stats->n_launches = run.n_launches + n_launches;
        stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    }
    return FT_OK;
}

int32_t ft_temporal_accumulate(ft_context* c, const ft_camera* cam, int32_t spp, const double* jitter_xy, int32_t sample, uint64_t seed,
                               const ft_temporal_params* params, int32_t rgba8, void* out, ft_stats* stats) {
    if (!c) return FT_ERR_INVALID;
    if (spp == 0) { c->err = "ft_temporal_accumulate: corner sampling (spp == 0) has no per-sample geometry ray to take the surfaces from"; return FT_ERR_UNSUPPORTED; }
    if (spp < 0 || !jitter_xy) { c->err = "bad ft_temporal_accumulate argument"; return FT_ERR_INVALID; }
    if (sample < 0 || sample >= spp) { c->err = "ft_temporal_accumulate: sample outside [0, spp)"; return FT_ERR_INVALID; }
    if (!cam || !params) { c->err = "ft_temporal_accumulate: null cam or params"; return FT_ERR_INVALID; }
    const ft_temporal_params& P = *params;
    if (P.max_history < 1) { c->err = "ft_temporal_accumulate: max_history below 1"; return FT_ERR_INVALID; }
    if (!(P.min_normal_dot >= -1.0 && P.min_normal_dot <= 1.0)) { c->err = "ft_temporal_accumulate: min_normal_dot is NaN or outside [-1, 1]"; return FT_ERR_INVALID; }
    if (!(P.position_tolerance_px > 0.0)) { c->err = "ft_temporal_accumulate: position_tolerance_px is not > 0"; return FT_ERR_INVALID; }
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    if (!c->peers.empty()) {
        c->err = "ft_temporal_accumulate: a context over several devices keeps the frame in 8-row bands on different devices and a tap crosses bands; gathering them is not supported";
        return FT_ERR_UNSUPPORTED;
    }
    if (!c->temporal.open) { c->err = "no temporal accumulation (ft_temporal_begin; a caller's ft_scene_commit or ft_scene_clear ends it)"; return FT_ERR_STATE; }
    const RenderRequest q{cam, c->temporal.res_h, c->temporal.res_v, spp, jitter_xy, 0, seed, nullptr, 0, 0};   // (the pixel list is made from the begin's rects)
    return with_growing_hit_lists(c, [&] { return temporal_single(c, q, sample, P, rgba8 != 0, out, stats); });
}

int32_t ft_temporal_fetch(ft_context* c, double* mean_rgb, double* stderr_rgb, double* length) {
    if (!c) return FT_ERR_INVALID;
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    const ft_context::Temporal& T = c->temporal;
    if (!T.open) { c->err = "no temporal accumulation (ft_temporal_begin)"; return FT_ERR_STATE; }
    const size_t n_px = (size_t)T.res_h * (size_t)T.res_v;
    std::vector<double> h(7 * n_px);                                // M, Q, N of the set the last call wrote
    FT_HIP(c, hipSetDevice(c->device));
    FT_HIP(c, hipStreamSynchronize(c->stream));
    FT_HIP(c, hipMemcpy(h.data(), T.d_set[T.prev].p, h.size() * 8, hipMemcpyDeviceToHost));
    for (const ft_rect& r : T.rects)
        for (int y = r.y0; y < r.y0 + r.h; ++y) for (int x = r.x0; x < r.x0 + r.w; ++x) {
            const size_t id = (size_t)y * (size_t)T.res_h + (size_t)x;
            const double N = h[6 * n_px + id];
            for (int ch = 0; ch < 3; ++ch) {
                const double M = h[(size_t)ch * n_px + id];
                if (mean_rgb) mean_rgb[3 * id + ch] = M;
                if (stderr_rgb) {
                    double se = 0.0;
                    if (N >= 2.0) { const double mm = M * M, v = h[(size_t)(3 + ch) * n_px + id] - mm; se = std::sqrt((v > 0.0 ? v : 0.0) / N); }
                    stderr_rgb[3 * id + ch] = se;
                }
            }
            if (length) length[id] = N;
        }
    return FT_OK;
}

int32_t ft_temporal_status(ft_context* c, int64_t out[4]) {
    if (!c || !out) return FT_ERR_INVALID;
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    const ft_context::Temporal& T = c->temporal;
    if (!T.open) { c->err = "no temporal accumulation (ft_temporal_begin)"; return FT_ERR_STATE; }
    out[0] = T.calls; out[1] = T.n_pix; out[2] = T.with_history; out[3] = T.at_max;
    return FT_OK;
}

int32_t ft_temporal_end(ft_context* c) {
    if (!c) return FT_ERR_INVALID;
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    temporal_close(c);
    return FT_OK;
}

// ------------------------------------------------------------------------------------------ debug / tests
// The start of a ray query (ft_debug_closest / ft_debug_blocked): the checks, the device, the rays into d_dbg_in (origins, directions and,
// when `max_dist` is given, the lengths), room for `out_bytes` per ray in d_dbg_out, and the overflow count cleared (in slot 0's counters).
static int32_t debug_rays_in(ft_context* c, const double* origins, const double* dirs, const double* max_dist, int64_t n, size_t out_bytes) {
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    if (!c->committed) { c->err = "scene not committed"; return FT_ERR_STATE; }
    if (n == 0) return FT_OK;
    FT_HIP(c, hipSetDevice(c->device));
    int32_t rc;
    const size_t N = (size_t)n;
    if ((rc = ensure(c, c->d_dbg_in, N * (max_dist ? 56 : 48))) != FT_OK) return rc;
    if ((rc = ensure(c, c->d_dbg_out, N * out_bytes)) != FT_OK) return rc;
    double* din = c->d_dbg_in.as<double>();
    FT_HIP(c, hipMemcpyAsync(din, origins, N * 24, hipMemcpyHostToDevice, c->stream));
    FT_HIP(c, hipMemcpyAsync(din + 3 * N, dirs, N * 24, hipMemcpyHostToDevice, c->stream));
    if (max_dist) FT_HIP(c, hipMemcpyAsync(din + 6 * N, max_dist, N * 8, hipMemcpyHostToDevice, c->stream));
    c->slots[0].fc_clean = false;
    FT_HIP(c, hipMemsetAsync(c->slots[0].d_fc.p, 0, sizeof(unsigned long long), c->stream));   // the overflow count of this query
    return FT_OK;
}
// ... and its end, behind the copies of the results: the overflow count read back, the stream synchronised.
static int32_t debug_rays_done(ft_context* c) {
    unsigned long long n_overflow = 0;
    FT_HIP(c, hipMemcpyAsync(&n_overflow, c->slots[0].d_fc.p, sizeof n_overflow, hipMemcpyDeviceToHost, c->stream));
    FT_HIP(c, hipStreamSynchronize(c->stream));
    if (n_overflow) { c->err = "CSG hit list overflow"; return FT_ERR_OVERFLOW; }
    return FT_OK;
}

static int32_t debug_closest(ft_context* c, const double* origins, const double* dirs, int64_t n, int32_t* hit, double* t, double* p, double* nrm, double* colour);
int32_t ft_debug_closest(ft_context* c, const double* origins, const double* dirs, int64_t n, int32_t* hit, double* t, double* p, double* nrm, double* colour) {
    if (!c) return FT_ERR_INVALID;
    return with_growing_hit_lists(c, [&] { return debug_closest(c, origins, dirs, n, hit, t, p, nrm, colour); });
}
static int32_t debug_closest(ft_context* c, const double* origins, const double* dirs, int64_t n, int32_t* hit, double* t, double* p, double* nrm, double* colour) {
    if (!c || !origins || !dirs || n < 0 || !hit || !t || !p || !nrm || !colour) return FT_ERR_INVALID;
    int32_t rc = debug_rays_in(c, origins, dirs, nullptr, n, 4 + 8 + 72);
    if (rc != FT_OK || n == 0) return rc;
    const size_t N = (size_t)n;
    double* din = c->d_dbg_in.as<double>();
    double* dt = c->d_dbg_out.as<double>();
    double* dp = dt + N; double* dn = dp + 3 * N; double* dc = dn + 3 * N;
    int32_t* dh = reinterpret_cast<int32_t*>(dc + 3 * N);
    ftk::Launch L{c->stream, c->n_cu * 4, lds_bytes_for(c->flat), 0};
    ftk::launch_debug_closest(L, c->dev_scene, din, din + 3 * N, (uint32_t)n, dh, dt, dp, dn, dc, c->slots[0].d_fc.as<unsigned long long>());
    FT_HIP(c, hipGetLastError());
    FT_HIP(c, hipMemcpyAsync(t, dt, N * 8, hipMemcpyDeviceToHost, c->stream));
    FT_HIP(c, hipMemcpyAsync(p, dp, N * 24, hipMemcpyDeviceToHost, c->stream));
    FT_HIP(c, hipMemcpyAsync(nrm, dn, N * 24, hipMemcpyDeviceToHost, c->stream));
    FT_HIP(c, hipMemcpyAsync(colour, dc, N * 24, hipMemcpyDeviceToHost, c->stream));
    FT_HIP(c, hipMemcpyAsync(hit, dh, N * 4, hipMemcpyDeviceToHost, c->stream));
    return debug_rays_done(c);
}

static int32_t debug_blocked(ft_context* c, const double* origins, const double* dirs, const double* max_dist, int64_t n, int32_t* blocked);
int32_t ft_debug_blocked(ft_context* c, const double* origins, const double* dirs, const double* max_dist, int64_t n, int32_t* blocked) {
    if (!c) return FT_ERR_INVALID;
    return with_growing_hit_lists(c, [&] { return debug_blocked(c, origins, dirs, max_dist, n, blocked); });
}
static int32_t debug_blocked(ft_context* c, const double* origins, const double* dirs, const double* max_dist, int64_t n, int32_t* blocked) {
    if (!c || !origins || !dirs || !max_dist || n < 0 || !blocked) return FT_ERR_INVALID;
    int32_t rc = debug_rays_in(c, origins, dirs, max_dist, n, 4);
    if (rc != FT_OK || n == 0) return rc;
    const size_t N = (size_t)n;
    double* din = c->d_dbg_in.as<double>();
    ftk::Launch L{c->stream, c->n_cu * 4, lds_bytes_for(c->flat), 0};
    ftk::launch_debug_blocked(L, c->dev_scene, din, din + 3 * N, din + 6 * N, (uint32_t)n, c->d_dbg_out.as<int32_t>(), c->slots[0].d_fc.as<unsigned long long>());
    FT_HIP(c, hipGetLastError());
    FT_HIP(c, hipMemcpyAsync(blocked, c->d_dbg_out.p, N * 4, hipMemcpyDeviceToHost, c->stream));
    return debug_rays_done(c);
}

// getColourForRay (Shading.fs:131-139) for explicit rays through the device path: the rays enter k_bounce as level 0 with weight 1
// and are followed to their end, so closest hit, shadow queries, shaders and up to max_depth reflection bounces run exactly as they
// do for a frame's samples.  Streams of soft lights are keyed with seed 0 and sample = ray index.
static int32_t debug_colour(ft_context* c, const double* origins, const double* dirs, int64_t n, int32_t max_depth, double* rgb);
int32_t ft_debug_colour(ft_context* c, const double* origins, const double* dirs, int64_t n, int32_t max_depth, double* rgb) {
    if (!c) return FT_ERR_INVALID;
    return with_growing_hit_lists(c, [&] { return debug_colour(c, origins, dirs, n, max_depth, rgb); });
}
static int32_t debug_colour(ft_context* c, const double* origins, const double* dirs, int64_t n, int32_t max_depth, double* rgb) {
    if (!c || !origins || !dirs || n < 0 || !rgb || max_depth < 0) return FT_ERR_INVALID;
    if (max_depth > ftk::kMaxBounce) { c->err = "max_depth above 16"; return FT_ERR_UNSUPPORTED; }
    if (n >= (1ll << 30)) return FT_ERR_INVALID;
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    if (!c->committed) { c->err = "scene not committed"; return FT_ERR_STATE; }
    if (n == 0) return FT_OK;
    FT_HIP(c, hipSetDevice(c->device));
    int32_t rc;
    if ((rc = ensure_frame_buffers(c, n, true)) != FT_OK) return rc;
    const size_t N = (size_t)n, cap = (size_t)c->ray_capacity;
    std::vector<double> soa(7 * N);
    std::vector<uint32_t> slot(N);
    for (size_t i = 0; i < N; ++i) {
        for (int k = 0; k < 3; ++k) { soa[(size_t)k * N + i] = origins[3 * i + k]; soa[(size_t)(3 + k) * N + i] = dirs[3 * i + k]; }
        soa[6 * N + i] = 1.0; slot[i] = (uint32_t)i;
    }
    auto* fc = c->slots[0].d_fc.as<ftk::FrameCounters>();
    c->slots[0].fc_clean = false;
    FT_HIP(c, hipMemsetAsync(fc, 0, sizeof(ftk::FrameCounters), c->stream));
    const ftk::RayBuf rb0 = ray_view(c->d_rays[0], c->ray_capacity), rb1 = ray_view(c->d_rays[1], c->ray_capacity);
    for (int k = 0; k < 7; ++k) FT_HIP(c, hipMemcpyAsync(c->d_rays[0].as<double>() + (size_t)k * cap, soa.data() + (size_t)k * N, N * 8, hipMemcpyHostToDevice, c->stream));
    FT_HIP(c, hipMemcpyAsync(rb0.slot, slot.data(), N * 4, hipMemcpyHostToDevice, c->stream));
    const uint32_t n_rays = (uint32_t)n;
    FT_HIP(c, hipMemcpyAsync(&fc->cc.n_rays[0], &n_rays, 4, hipMemcpyHostToDevice, c->stream));
    FT_HIP(c, hipMemsetAsync(c->d_acc[0].p, 0, 3 * N * 8, c->stream));
    const size_t lds = lds_bytes_for(c->flat);
    ftk::Launch Lt{c->stream, c->n_cu * c->blocks_bounce, lds, c->variant};
    ftk::Primary gen{};
    gen.pixel_ids = nullptr; gen.pix_base = 0; gen.n_pix = n_rays; gen.spp = 1; gen.inv_n_pix = 1.0 / (double)n_rays; gen.seed = 0ull; gen.counts = nullptr; gen.block_map = nullptr;
    ftk::launch_bounce(Lt, c->dev_scene, gen, rb0, rb1, c->d_acc[0].as<double>(), n_rays, 0, max_depth, true, fc);   // level 0, followed to the end
    FT_HIP(c, hipGetLastError());
    std::vector<double> planes(3 * N);
    FT_HIP(c, hipMemcpyAsync(planes.data(), c->d_acc[0].p, 3 * N * 8, hipMemcpyDeviceToHost, c->stream));
    struct { ftk::RenderCounters stats[ftk::kStatStripes]; } tail;
    FT_HIP(c, hipMemcpyAsync(&tail, &fc->stats[0], sizeof tail, hipMemcpyDeviceToHost, c->stream));
    FT_HIP(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < N; ++i) { rgb[3 * i] = planes[i]; rgb[3 * i + 1] = planes[N + i]; rgb[3 * i + 2] = planes[2 * N + i]; }
    unsigned long long ovf = 0;
    for (int k = 0; k < ftk::kStatStripes; ++k) ovf += tail.stats[k].csg_overflow;
    if (ovf) { c->err = "CSG hit list overflow"; return FT_ERR_OVERFLOW; }
    return FT_OK;
}

/* Diagnostic builds (-DFT_STAMPS): the s_memrealtime stamps k_classify's workgroups left behind (8 per workgroup). */
int32_t ft_debug_classify_stamps(ft_context* c, unsigned long long* out, int32_t n_groups) {
    if (!c || !out || n_groups < 1 || n_groups > 2048 || !c->d_wave_counts.p) return FT_ERR_INVALID;
    if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) return FT_ERR_HIP;
    return hipMemcpy(out, c->d_wave_counts.as<uint32_t>() + 4096, (size_t)n_groups * 64, hipMemcpyDeviceToHost) == hipSuccess ? FT_OK : FT_ERR_HIP;
}

int32_t ft_debug_scene_info(ft_context* c, int64_t out[12]) {
    if (!c || !out) return FT_ERR_INVALID;
    if (!c->committed) { c->err = "scene not committed"; return FT_ERR_STATE; }
    const fth::FlatScene& f = c->flat;
    out[0] = (int64_t)f.leaves.size(); out[1] = (int64_t)f.program.size(); out[2] = (int64_t)f.meshes.size(); out[3] = (int64_t)f.nodes.size() - f.bvh_nodes;
    out[4] = (int64_t)f.bsp_leaves.size() - f.bvh_leaves; out[5] = (int64_t)(f.tris.size() / 9) - f.bvh_tris; out[6] = f.csg_capacity; out[7] = f.bsp_stack_capacity;   // BSP-only: excludes the device-side BVH
    int64_t bounded = 0; for (size_t k = 0; k + 1 < f.item_pc.size(); ++k) if (f.cull_items[8 * k + 3] < 1e30f) ++bounded;
    out[8] = (int64_t)f.item_pc.size() - 1; out[9] = bounded; out[10] = f.unbounded ? 1 : 0; out[11] = f.cull_bundle ? (int64_t)(f.cull_rows.size() / 3) : -1;
    return FT_OK;
}

int32_t ft_debug_light_space(ft_context* c, int64_t sizes[4], double* pairs, uint32_t* nodes, double* tris, uint32_t* leaf_pairs) {
    if (!c || !sizes) return FT_ERR_INVALID;
    if (!c->committed) { c->err = "scene not committed"; return FT_ERR_STATE; }
    const fth::FlatScene& f = c->flat;
    sizes[0] = (int64_t)(f.ls_pairs.size() / ftd::kLsPairDoubles); sizes[1] = (int64_t)(f.ls_nodes.size() / ftd::kLsNodeWords);
    sizes[2] = (int64_t)(f.ls_tris.size() / 9); sizes[3] = (int64_t)f.leaves.size();
    if (pairs) std::memcpy(pairs, f.ls_pairs.data(), f.ls_pairs.size() * sizeof(double));
    if (nodes) std::memcpy(nodes, f.ls_nodes.data(), f.ls_nodes.size() * sizeof(uint32_t));
    if (tris) std::memcpy(tris, f.ls_tris.data(), f.ls_tris.size() * sizeof(double));
    if (leaf_pairs) for (size_t k = 0; k < f.leaves.size(); ++k) leaf_pairs[k] = f.leaves[k].ls_pairs;
    return FT_OK;
}

int32_t ft_debug_slice(const double p0[3], const double n[3], const double tri[9], double above[18], int32_t* n_above, double below[18], int32_t* n_below) {
    if (!p0 || !n || !tri || !above || !below || !n_above || !n_below) return FT_ERR_INVALID;
    std::vector<double> a, b; std::string err;
    int32_t rc = fth::slice_triangle(p0, n, tri, a, b, err);
    if (rc != FT_OK) return rc;
    *n_above = (int32_t)(a.size() / 9); *n_below = (int32_t)(b.size() / 9);
    if (!a.empty()) std::memcpy(above, a.data(), a.size() * 8);
    if (!b.empty()) std::memcpy(below, b.data(), b.size() * 8);
    return FT_OK;
}

int32_t ft_debug_devices(ft_context* c, int32_t* ordinals, int32_t capacity) {   // the device ordinals behind a context, in order; returns how many
    if (!c || capacity < 0 || (capacity > 0 && !ordinals)) return FT_ERR_INVALID;
    if (c->host_only) return 0;
    int32_t n = 0;
    if (n < capacity) ordinals[n] = c->device;
    ++n;
    for (ft_context* p : c->peers) { if (n < capacity) ordinals[n] = p->device; ++n; }
    return n;
}

int32_t ft_quantise_rgba8(const double* rgb, int64_t n_pixels, uint8_t* out) {   // Image.fs:36, Math.fs:12-16
    if (!rgb || !out || n_pixels < 0) return FT_ERR_INVALID;
    for (int64_t i = 0; i < n_pixels; ++i) {
        for (int k = 0; k < 3; ++k) {
            double x = rgb[3 * i + k];
            if (x > 1.0) x = 1.0; else if (x < 0.0) x = 0.0;                     // NaN passes through the clamp unchanged
            x = x * 255.0;
            out[4 * i + k] = (x != x) ? 0 : (uint8_t)x;                          // truncation, not rounding
        }
        out[4 * i + 3] = 255;
    }
    return FT_OK;
}

} // extern "C"

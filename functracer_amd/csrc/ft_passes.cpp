// ft_passes.cpp — the passes over the surface buffers: ft_render_aov, and ft_denoise, ft_temporal_* and ft_temporal_filter which take
// their guides from it.
#include "ft_context.h"

namespace ftc {

// Ends the temporal accumulation of a context (its buffers are freed): leaf ids are only comparable within one commit and the
// ft_scene_commit_moved calls that follow it.
void temporal_close(ft_context* c) {
    if (!c->temporal.open) return;
    (void)hipSetDevice(c->device);
    (void)retire_temporal(c, nullptr);                              // queued calls still use the buffers (an overflow among them has closed it already)
    if (c->temporal.open) c->temporal.release();
}

// The snapshots of "temporal_follow_deformed" and their device memory let go: the history has caught up with the meshes (a successful
// accumulate), or nothing will follow them (the option back at 0).
void temporal_drop_snapshots(ft_context* c) {
    ft_context::Temporal& T = c->temporal;
    if (T.snaps.empty() && !T.d_snap.p && !T.d_deform.p) return;
    (void)hipSetDevice(c->device);
    T.snaps.clear(); T.snap_used = 0;
    T.d_snap.release(); T.d_deform.release();
}

} // namespace ftc
using namespace ftc;

extern "C" {

// ------------------------------------------------------------------------------------------ per-pixel surface buffers
// ft_render_aov: the hit of one sample's geometry ray per tile pixel (functracer_hip.h).  The call keeps to buffers of its own - pixel
// list, jitter pattern, planes, counters - so the frame buffer, the cached pixel list, the zero-fill and level-hint history and a
// progressive accumulation stay as they were.  The list is ft_render's (8x8 blocks in Z order where the rects allow), cut into windows
// of "chunk_samples" entries; per window one k_aov writes the requested planes by list position and the host scatters them into the
// caller's frame-shaped planes.
namespace {
struct AovPlanes { int64_t off[8]; int width[8], esz[8]; size_t bytes_per_entry; };   // t, p, n, colour, material, leaf, node, triangle; esz: bytes of an element
void* aov_plane(const AovPlanes& pl, char* dev, int k) { return pl.off[k] < 0 ? nullptr : dev + pl.off[k]; }   // plane k of the window at `dev`; null: not wanted
AovPlanes aov_planes(const bool (&want)[8], int64_t per) {
    AovPlanes a{};
    const int width[8] = {1, 3, 3, 3, 3, 1, 1, 1};
    int64_t at = 0;                                                 // bytes; doubles first, then the 32-bit planes
    for (int k = 0; k < 8; ++k) {
        a.off[k] = -1; a.width[k] = width[k]; a.esz[k] = k < 5 ? 8 : 4;
        if (!want[k]) continue;
        a.off[k] = at;
        at += per * width[k] * a.esz[k];
        a.bytes_per_entry += (size_t)width[k] * a.esz[k];
    }
    return a;
}
struct AovRun { int64_t n_pix = 0; unsigned long long hits = 0; double kernel_ms = 0.0; int32_t n_launches = 0; };
} // namespace

// What the passes below share.  The parameters of the a-trous filters: the iteration count and the sigmas, then (the passes check their
// own in between) the albedo floor.
static int32_t check_filter_params(ft_context* c, const std::string& api, int32_t iterations, double sigma_colour, double sigma_normal, double sigma_position) {
    if (iterations < 0 || iterations > 6) { c->err = api + ": iterations outside 0 .. 6"; return FT_ERR_INVALID; }
    if (!(sigma_colour >= 0.0) || !(sigma_normal >= 0.0) || !(sigma_position >= 0.0)) { c->err = api + ": a sigma is negative or NaN (0 switches a term off)"; return FT_ERR_INVALID; }
    return FT_OK;
}
static int32_t check_albedo_floor(ft_context* c, const std::string& api, int32_t demodulate, double albedo_floor) {
    if (demodulate && !(albedo_floor > 0.0)) { c->err = api + ": demodulate needs albedo_floor > 0"; return FT_ERR_INVALID; }
    return FT_OK;
}
static double inv_sq(double sigma) { return sigma > 0.0 ? 1.0 / (sigma * sigma) : 0.0; }   // 1 / sigma^2 as the kernels take it; 0 switches the term off
// The window [p0, p0 + n) of aov_windows as a kernel reads it: the planes the pass asked k_aov for, the others null.
static ftk::GuideWindow guide_window(const uint32_t* pixel_ids, int64_t p0, uint32_t n, const AovPlanes& pl, char* dev) {
    return ftk::GuideWindow{static_cast<const int32_t*>(aov_plane(pl, dev, 7)), pixel_ids, (uint32_t)p0, n, static_cast<const double*>(aov_plane(pl, dev, 1)),
                            static_cast<const double*>(aov_plane(pl, dev, 2)), static_cast<const double*>(aov_plane(pl, dev, 3)), static_cast<const int32_t*>(aov_plane(pl, dev, 5)), n};
}
static int32_t read_counters(ft_context* c, const DeviceBuf& buf, unsigned long long* ctr, size_t n = 2) {   // the n counts a pass's kernels kept in `buf`
    FT_HIP(c, hipMemcpy(ctr, buf.p, n * sizeof *ctr, hipMemcpyDeviceToHost)); return FT_OK;
}

// The device half of an AOV pass, shared by ft_render_aov and ft_denoise: the pixel list `px` and the pattern go up, and per window of
// "chunk_samples" entries one k_aov writes the wanted planes into d_aov_out by position in the window.  consume(p0, n, planes, dev) then
// sees the window [p0, p0 + n) with its planes still in HBM, behind the kernel on the context's stream - it copies them out, or queues a
// kernel that reads them.  The stream is drained after every window (the next one overwrites the planes' buffer and the event pair).
// The windows of a guide pass over n_pix list entries: `per` entries each, whole 8x8 blocks.
static int64_t guide_window_size(const ft_context* c, int64_t n_pix) {
    int64_t per = std::max<int64_t>(1, std::min<int64_t>(n_pix, c->opt.chunk_samples));
    if (per > 64) per -= per % 64;
    return per;
}
// One k_aov over the window [p0, p0 + n) of the list `pixels` (on the device, as `jitter`), its planes into `dev` by position in the window.
static void launch_guide_window(ft_context* c, const RenderRequest& q, int32_t sample, const ftk::Camera& cam, const uint32_t* pixels, const double* jitter,
                                int64_t p0, uint32_t n, const AovPlanes& pl, char* dev) {
    const ftk::Launch L{c->stream, c->n_cu * c->blocks_aov, lds_bytes_for(c->flat), c->variant};
    const ftk::AovSource src{c->d_scene[kTriSrc].as<uint32_t>(), c->d_scene[kRunNodes].as<int32_t>()};
    ftk::Primary gen{cam, pixels, jitter, (uint32_t)p0, n, q.spp, (uint32_t)q.res_h, (unsigned long long)q.seed, 1.0 / (double)n, 1.0 / (double)q.res_h, nullptr, nullptr};
    gen.group_log2 = 0;
    const ftk::AovOut out{static_cast<double*>(aov_plane(pl, dev, 0)), static_cast<double*>(aov_plane(pl, dev, 1)), static_cast<double*>(aov_plane(pl, dev, 2)), static_cast<double*>(aov_plane(pl, dev, 3)),
                          static_cast<double*>(aov_plane(pl, dev, 4)), static_cast<int32_t*>(aov_plane(pl, dev, 5)), static_cast<int32_t*>(aov_plane(pl, dev, 6)), static_cast<int32_t*>(aov_plane(pl, dev, 7)), n};
    ftk::launch_aov(L, c->dev_scene, gen, (uint32_t)sample, src, out, c->aov.d_ctr.as<unsigned long long>());
}
static int32_t aov_windows(ft_context* c, const RenderRequest& q, int32_t sample, const bool (&want)[8], const std::vector<uint32_t>& px, AovRun& run,
                           const std::function<int32_t(int64_t, uint32_t, const AovPlanes&, char*)>& consume) {
    int32_t rc;
    const int64_t n_pix = (int64_t)px.size();
    run = AovRun{};
    run.n_pix = n_pix;
    if (n_pix == 0) return FT_OK;
    const int64_t per = guide_window_size(c, n_pix);
    const AovPlanes pl = aov_planes(want, per);
    if ((rc = upload(c, c->aov.d_pixels, px)) != FT_OK) return rc;
    if ((rc = upload(c, c->aov.d_jitter, std::vector<double>(q.jitter_xy, q.jitter_xy + 2 * (size_t)q.spp))) != FT_OK) return rc;
    if ((rc = ensure(c, c->aov.d_out, (size_t)per * pl.bytes_per_entry)) != FT_OK) return rc;
    if ((rc = ensure(c, c->aov.d_ctr, 2 * sizeof(unsigned long long))) != FT_OK) return rc;
    FT_HIP(c, hipMemsetAsync(c->aov.d_ctr.p, 0, 2 * sizeof(unsigned long long), c->stream));
    c->aov.ctr_clean = false;
    const ftk::Camera cam = make_camera(*q.cam, q.res_h, q.res_v);
    char* const dev = c->aov.d_out.as<char>();
    for (int64_t p0 = 0; p0 < n_pix; p0 += per) {
        const uint32_t n = (uint32_t)std::min<int64_t>(per, n_pix - p0);
        rc = c->aov.timer.run(c, run.kernel_ms, [&] { launch_guide_window(c, q, sample, cam, c->aov.d_pixels.as<uint32_t>(), c->aov.d_jitter.as<double>(), p0, n, pl, dev); },
                              [&] { ++run.n_launches; return consume(p0, n, pl, dev); });
        if (rc != FT_OK) return rc;
    }
    unsigned long long ctr[2] = {0, 0};
    if ((rc = read_counters(c, c->aov.d_ctr, ctr)) != FT_OK) return rc;
    if (ctr[1]) { c->err = "CSG hit list overflow"; return FT_ERR_OVERFLOW; }
    run.hits = ctr[0];
    return FT_OK;
}

// This device is about to run a guide pass: the frames and temporal calls still queued on it are retired first, and the caller's stats start from zero.
static int32_t begin_pass(ft_context* c, ft_stats* stats) {
    FT_HIP(c, hipSetDevice(c->device));
    int32_t rc;
    if (any_queued(c) && (rc = retire_queued(c)) != FT_OK) return rc;
    if (stats) std::memset(stats, 0, sizeof *stats);
    return FT_OK;
}
// ... and has run it: the k_aov launches of `run` and the `own_launches` kernels of the pass itself, own_ms on the device, behind them.
static void end_pass(ft_stats* stats, const AovRun& run, double own_ms, int32_t own_launches, std::chrono::steady_clock::time_point wall0) {
    if (!stats) return;
    stats->rays_primary = (uint64_t)run.n_pix; stats->hits_primary = run.hits;
    stats->kernel_ms = run.kernel_ms + own_ms; stats->n_launches = run.n_launches + own_launches;
    stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
}
// What `api` reads must be the FP64 frame of this size in HBM; `reader` and `size_tail` word the refusal.
static int32_t need_fp64_frame(ft_context* c, const std::string& api, int32_t res_h, int32_t res_v, const char* reader, const char* size_tail) {
    if (c->last_n_pix > 0 && c->last_format == 0 && c->last_res_h == res_h && c->last_res_v == res_v) return FT_OK;
    c->err = api + (c->last_n_pix <= 0 ? ": no frame rendered yet" : c->last_format != 0 ? std::string(": the frame in HBM is RGBA8 (ft_render_rgba8); the ") + reader + " needs the FP64 frame"
                                                                                       : std::string(": the frame in HBM has another size") + size_tail);
    return FT_ERR_STATE;
}
// The passes that read the whole frame in HBM refuse a context over several devices.
static int32_t need_one_device(ft_context* c, const std::string& api) {
    if (c->peers.empty()) return FT_OK;
    c->err = api + ": a context over several devices keeps the frame in 8-row bands on different devices and a tap crosses bands; gathering them is not supported";
    return FT_ERR_UNSUPPORTED;
}
// The sample a guide pass takes its geometry ray from; `corner_tail` ends the sentence about corner sampling.  (Behind check_request
// the second test cannot fail: ft_temporal_accumulate, which has no request to check, relies on it.)
static int32_t check_guide_sample(ft_context* c, const std::string& api, int32_t spp, const double* jitter_xy, int32_t sample, const char* corner_tail) {
    if (spp == 0) { c->err = api + ": corner sampling (spp == 0) has no per-sample geometry ray" + corner_tail; return FT_ERR_UNSUPPORTED; }
    if (spp < 0 || !jitter_xy) { c->err = "bad " + api + " argument"; return FT_ERR_INVALID; }
    if (sample < 0 || sample >= spp) { c->err = api + ": sample outside [0, spp)"; return FT_ERR_INVALID; }
    return FT_OK;
}

static int32_t aov_single(ft_context* c, const RenderRequest& q, int32_t sample, const ft_aov& o, ft_stats* stats) {
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    if (!need_committed(c)) return FT_ERR_STATE;
    const auto wall0 = std::chrono::steady_clock::now();
    int32_t rc;
    if ((rc = begin_pass(c, stats)) != FT_OK) return rc;
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
        for (int k = 0; k < 8; ++k) if (pl.off[k] >= 0) need = std::max(need, (size_t)pl.off[k] + (size_t)n * pl.width[k] * pl.esz[k]);
        if (host.size() < need) host.resize(need);
        for (int k = 0; k < 8; ++k) if (pl.off[k] >= 0) {          // a channel's planes lie back to back: n entries apart within the window
            FT_HIP(c, hipMemcpyAsync(host.data() + pl.off[k], dev + pl.off[k], (size_t)n * pl.width[k] * pl.esz[k], hipMemcpyDeviceToHost, c->stream));
        }
        FT_HIP(c, hipStreamSynchronize(c->stream));
        for (int k = 0; k < 8; ++k) if (pl.off[k] >= 0) {          // into the caller's planes: frame layout, row 0 = top, w components per pixel
            const int w = pl.width[k];
            const char* src_k = host.data() + pl.off[k];
            if (pl.esz[k] == 8) {
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
    end_pass(stats, run, 0.0, 0, wall0);
    return FT_OK;
}

static int32_t aov_frame(ft_context* c, const RenderRequest& q, int32_t sample, const ft_aov& o, ft_stats* stats) {
    if (c->peers.empty()) return aov_single(c, q, sample, o, stats);
    if (!need_committed(c)) return FT_ERR_STATE;
    const auto wall0 = std::chrono::steady_clock::now();
    const std::vector<std::vector<ft_rect>> share = band_shares(q, 1 + c->peers.size());   // ft_render's 8-row bands: each device writes its rows
    return on_every_device(c, stats, wall0, [&](size_t d, ft_context* D, ft_stats* sd) -> int32_t {
        if (share[d].empty()) return FT_OK;
        RenderRequest qd = q;
        qd.tiles = share[d].data(); qd.n_tiles = (int32_t)share[d].size();
        return aov_single(D, qd, sample, o, sd);
    });
}

int32_t ft_render_aov(ft_context* c, const ft_camera* cam, int32_t res_h, int32_t res_v, int32_t spp, const double* jitter_xy,
                      int32_t sample, uint64_t seed, const ft_rect* tiles, int32_t n_tiles, const ft_aov* out, ft_stats* stats) {
    if (!c) return FT_ERR_INVALID;
    const RenderRequest q{cam, res_h, res_v, spp, jitter_xy, 0, seed, tiles, n_tiles, 0};
    int32_t rc = check_request(c, q);
    if (rc != FT_OK) return rc;
    if ((rc = check_guide_sample(c, "ft_render_aov", spp, jitter_xy, sample, "")) != FT_OK) return rc;
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
    int32_t rc;
    if ((rc = begin_pass(c, stats)) != FT_OK) return rc;
    if ((rc = need_fp64_frame(c, "ft_denoise", q.res_h, q.res_v, "filter", "")) != FT_OK) return rc;
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
    if (!need_committed(c)) return FT_ERR_STATE;
    if ((rc = drain_frame_streams(c)) != FT_OK) return rc;          // the frame may have been written on another stream (fetch_single)
    const size_t n_px = (size_t)q.res_h * (size_t)q.res_v;
    const double* frame = c->d_out.as<double>();
    const void* result = frame;                                     // zero iterations: the frame itself
    double kernel_ms = 0.0;
    int32_t n_launches = 0;
    AovRun run;
    TimedLaunch& timer = c->denoise.timer;
    if (rgba8 && (rc = ensure(c, c->denoise.d_out8, n_px * 4)) != FT_OK) return rc;
    if (P.iterations > 0) {
        if ((rc = ensure(c, c->denoise.d_guides, n_px * ftk::kDenoiseGuideBytes)) != FT_OK) return rc;
        for (int k = 0; k < 2; ++k) if ((rc = ensure(c, c->denoise.d_u[k], n_px * 24)) != FT_OK) return rc;
        ftk::DenoiseGuides g{};
        double* plane = c->denoise.d_guides.as<double>();
        for (int k = 0; k < 3; ++k) { g.n[k] = plane + (size_t)k * n_px; g.p[k] = plane + (size_t)(3 + k) * n_px; g.d[k] = plane + (size_t)(6 + k) * n_px; }
        g.v = plane + 9 * n_px;
        g.cls = reinterpret_cast<uint8_t*>(plane + 10 * n_px);
        FT_HIP(c, hipMemsetAsync(g.cls, ftk::kDenoiseOutside, n_px, c->stream));
        const bool want[8] = {false, true, true, true, false, true, false, false};   // p, n, colour, leaf
        rc = aov_windows(c, q, sample, want, px, run, [&](int64_t p0, uint32_t n, const AovPlanes& pl, char* dev) -> int32_t {
            ftk::DenoiseScatterArgs a{};
            a.win = guide_window(c->aov.d_pixels.as<uint32_t>(), p0, n, pl, dev);
            a.frame = frame; a.u0 = c->denoise.d_u[0].as<double>(); a.g = g;
            a.demodulate = P.demodulate ? 1 : 0; a.albedo_floor = P.albedo_floor;
            if (P.use_variance) {
                a.sum = G.d_sum[G.cur].as<double>(); a.sq = G.d_sq[G.cur].as<double>(); a.blk = G.d_blk[G.cur].as<uint32_t>();
                a.n_list = (uint32_t)G.n_pix; a.variance_floor = P.variance_floor;
            }
            ++n_launches;
            return timer.run(c, kernel_ms, [&] { ftk::launch_denoise_scatter(c->stream, a); });
        });
        if (rc != FT_OK) return rc;
        rc = timer.run(c, kernel_ms, [&] { for (int i = 0; i < P.iterations; ++i) {   // one bracket around all iterations
            const bool last = i + 1 == P.iterations;
            ftk::DenoiseArgs a{};
            a.u_in = c->denoise.d_u[i & 1].as<double>(); a.u_out = c->denoise.d_u[(i + 1) & 1].as<double>();
            a.out8 = last && rgba8 ? c->denoise.d_out8.as<uint8_t>() : nullptr;
            a.g = g; a.res_h = q.res_h; a.res_v = q.res_v; a.step = 1 << i;
            a.inv_sn2 = inv_sq(P.sigma_normal); a.inv_sp2 = inv_sq(P.sigma_position); a.inv_sc2 = inv_sq(P.sigma_colour * std::ldexp(1.0, -i));
            ftk::launch_denoise(c->stream, a, last);
            ++n_launches;
            if (last) result = rgba8 ? (const void*)a.out8 : (const void*)a.u_out;
        } });
        if (rc != FT_OK) return rc;
    } else if (rgba8) {
        ++n_launches;
        if ((rc = timer.run(c, kernel_ms, [&] { ftk::launch_denoise_quantise(c->stream, frame, c->denoise.d_out8.as<uint8_t>(), (uint32_t)n_px); })) != FT_OK) return rc;
        result = c->denoise.d_out8.p;
    }
    if ((rc = copy_rects_out(c, out, result, rgba8 ? 4 : 24, q.res_h, rects, nullptr)) != FT_OK) return rc;
    end_pass(stats, run, kernel_ms, n_launches, wall0);
    return FT_OK;
}

int32_t ft_denoise(ft_context* c, const ft_camera* cam, int32_t res_h, int32_t res_v, int32_t spp, const double* jitter_xy, int32_t sample, uint64_t seed,
                   const ft_rect* tiles, int32_t n_tiles, const ft_denoise_params* params, int32_t rgba8, void* out, ft_stats* stats) {
    if (!c) return FT_ERR_INVALID;
    const RenderRequest q{cam, res_h, res_v, spp, jitter_xy, 0, seed, tiles, n_tiles, 0};
    int32_t rc = check_request(c, q);
    if (rc != FT_OK) return rc;
    if ((rc = check_guide_sample(c, "ft_denoise", spp, jitter_xy, sample, " to take the guides from")) != FT_OK) return rc;
    if (!params || !out) { c->err = "ft_denoise: null params or out"; return FT_ERR_INVALID; }
    const ft_denoise_params& P = *params;
    if ((rc = check_filter_params(c, "ft_denoise", P.iterations, P.sigma_colour, P.sigma_normal, P.sigma_position)) != FT_OK) return rc;
    if ((rc = check_albedo_floor(c, "ft_denoise", P.demodulate, P.albedo_floor)) != FT_OK) return rc;
    if (P.use_variance && !(P.variance_floor > 0.0)) { c->err = "ft_denoise: use_variance needs variance_floor > 0"; return FT_ERR_INVALID; }
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    if ((rc = need_one_device(c, "ft_denoise")) != FT_OK) return rc;
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
// `to_frame`: the tile pixels of the frame in HBM become those of `rgb` (frame layout, 3 doubles per pixel).
static int32_t temporal_to_frame(ft_context* c, const void* rgb) {
    const ft_context::Temporal& T = c->temporal;
    const size_t pitch = (size_t)T.res_h * 24;
    for (const ft_rect& r : T.rects) {
        const size_t off = (size_t)r.y0 * pitch + (size_t)r.x0 * 24;
        FT_HIP(c, hipMemcpy2DAsync(c->d_out.as<char>() + off, pitch, static_cast<const char*>(rgb) + off, pitch, (size_t)r.w * 24, (size_t)r.h, hipMemcpyDeviceToDevice, c->stream));
    }
    FT_HIP(c, hipStreamSynchronize(c->stream));
    c->zero_signature[0] = 0;                                       // (as a progressive pass: the blocks the last ft_render left as Colour.Zero hold means now)
    return FT_OK;
}
// The refusals of the calls that need an open accumulation.
static const char kNoTemporal[] = "no temporal accumulation (ft_temporal_begin)";
static const char kNoTemporalEnded[] = "no temporal accumulation (ft_temporal_begin; a caller's ft_scene_commit or ft_scene_clear ends it)";

// The records of k_temporal<true> (ftk::kTemporalMotionDoubles per leaf, ft_device.h) for a scene whose leaves stand at (m2w, w2m) now
// and whose history was written when they stood at (H, Wh).  Per leaf: D = H o w2m, a 3x4 affine product that takes a current world
// point of the leaf to where it was; A = m2w_lin * Wh_lin, the inverse of D's linear part; moved: any of the 12 m2w doubles differs.
static std::vector<double> temporal_motion(const fth::FlatScene& f, const std::vector<double>& H, const std::vector<double>& Wh) {
    const size_t n = f.leaves.size();
    std::vector<double> rec(n * ftk::kTemporalMotionDoubles, 0.0);
    for (size_t l = 0; l < n; ++l) {
        const double* M = &f.m2w[12 * l];
        const double* Wc = f.leaves[l].w2m;
        const double* Hl = &H[12 * l];
        const double* Wl = &Wh[12 * l];
        double* r = &rec[l * ftk::kTemporalMotionDoubles];
        for (int i = 0; i < 3; ++i) {
            for (int j = 0; j < 4; ++j) {
                double d = Hl[4 * i] * Wc[j] + Hl[4 * i + 1] * Wc[4 + j] + Hl[4 * i + 2] * Wc[8 + j];
                if (j == 3) d += Hl[4 * i + 3];
                r[4 * i + j] = d;
            }
            for (int j = 0; j < 3; ++j) r[12 + 3 * i + j] = M[4 * i] * Wl[j] + M[4 * i + 1] * Wl[4 + j] + M[4 * i + 2] * Wl[8 + j];
        }
        r[21] = std::memcmp(M, Hl, 12 * sizeof(double)) != 0 ? 1.0 : 0.0;   // bitwise: any double differs (a NaN matrix counts as moved)
    }
    return rec;
}

// The records of k_temporal<MOVING, true> (ftk::TemporalDeformLeaf per leaf, ft_device.h): every mesh leaf whose mesh holds a snapshot gets
// its live w2m, the m2w and the linear part of the w2m the history was written under, and where its live and its kept records start;
// every other leaf n = 0.  A snapshot whose mesh no longer has the range it was taken from is left out (n = 0).
static std::vector<ftk::TemporalDeformLeaf> temporal_deform(const fth::FlatScene& f, const ft_context::Temporal& T) {
    std::vector<ftk::TemporalDeformLeaf> rec(f.leaves.size(), ftk::TemporalDeformLeaf{});
    for (size_t l = 0; l < f.leaves.size(); ++l) {
        const ftd::Leaf& L = f.leaves[l];
        if (L.kind != ftd::LK_MESH || L.mesh >= f.meshes.size() || f.meshes[L.mesh].root >= 0 || (size_t)~f.meshes[L.mesh].root >= f.bsp_leaves.size()) continue;
        const ftd::BspLeaf& list = f.bsp_leaves[(size_t)~f.meshes[L.mesh].root];
        for (const ft_context::Temporal::Snapshot& s : T.snaps) {
            if (s.mesh != L.mesh || s.n != list.n_tris || (size_t)list.first_tri + s.n > f.tris.size() / 9 || (size_t)s.first + s.n > T.snap_used) continue;
            ftk::TemporalDeformLeaf& r = rec[l];
            std::memcpy(r.W, L.w2m, sizeof r.W);
            std::memcpy(r.H, &T.h_m2w[12 * l], sizeof r.H);
            for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) r.Wh[3 * i + j] = T.h_w2m[12 * l + 4 * i + j];
            r.first_live = list.first_tri; r.snap_first = s.first; r.n = s.n;
        }
    }
    return rec;
}

int32_t ft_temporal_begin(ft_context* c, int32_t res_h, int32_t res_v, const ft_rect* tiles, int32_t n_tiles) {
    if (!c) return FT_ERR_INVALID;
    if (res_h < 2 || res_v < 2 || (tiles && n_tiles < 1) || (int64_t)res_h * res_v > (int64_t)0x7FFFFFFF) { c->err = "bad ft_temporal_begin argument"; return FT_ERR_INVALID; }
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    int32_t rc;
    if ((rc = need_one_device(c, "ft_temporal_begin")) != FT_OK) return rc;
    if ((rc = retire_temporal(c, nullptr)) != FT_OK) return rc;     // an error among the queued calls of the accumulation this one replaces
    temporal_close(c);                                              // a second begin replaces the first
    ft_context::Temporal& T = c->temporal;
    rc = [&]() -> int32_t {
        FT_HIP(c, hipSetDevice(c->device));
        const size_t set_bytes = (size_t)res_h * (size_t)res_v * ftk::kTemporalSetBytes;
        int32_t r;
        for (DeviceBuf& b : T.d_set) {                              // N = 0 everywhere: no tap finds history (the rest is cleared with it)
            if ((r = ensure(c, b, set_bytes)) != FT_OK) return r;
            FT_HIP(c, hipMemsetAsync(b.p, 0, set_bytes, c->stream));
        }
        if ((r = ensure(c, T.d_ctr, 3 * sizeof(unsigned long long))) != FT_OK) return r;
        FT_HIP(c, hipStreamSynchronize(c->stream));
        return FT_OK;
    }();
    if (rc != FT_OK) { T.release(); return rc; }
    T.open = true; T.res_h = res_h; T.res_v = res_v;
    T.rects = clip_rects(RenderRequest{nullptr, res_h, res_v, 1, kNoJitter, 0, 0, tiles, n_tiles, 0});
    for (const ft_rect& r : T.rects) T.n_pix += (int64_t)r.w * r.h;
    return FT_OK;
}

// The steps ft_temporal_accumulate and ft_temporal_enqueue share; what differs between them is what stands between the launches.
// The clamp's planes: allocated by the first call with the clamp on, the mask filled once per accumulation (the rects are the begin's,
// as ft_temporal_filter fills its class plane); `box` then points into them.
static int32_t temporal_box_planes(ft_context* c, ftk::TemporalBox& box) {
    ft_context::Temporal& T = c->temporal;
    const size_t n_px = (size_t)T.res_h * (size_t)T.res_v;
    int32_t rc;
    if ((rc = ensure(c, T.d_box, n_px * ftk::kTemporalBoxBytes)) != FT_OK || (rc = ensure(c, T.d_mask, n_px)) != FT_OK) return rc;
    uint8_t* const mask = T.d_mask.as<uint8_t>();
    if (!T.mask_built) {
        FT_HIP(c, hipMemsetAsync(mask, 0, n_px, c->stream));
        for (const ft_rect& r : T.rects)
            FT_HIP(c, hipMemset2DAsync(mask + (size_t)r.y0 * (size_t)T.res_h + (size_t)r.x0, (size_t)T.res_h, 1, (size_t)r.w, (size_t)r.h, c->stream));
        T.mask_built = true;
    }
    for (int k = 0; k < 3; ++k) { box.lo[k] = T.d_box.as<double>() + (size_t)k * n_px; box.hi[k] = T.d_box.as<double>() + (size_t)(3 + k) * n_px; }
    return FT_OK;
}
// One k_temporal_box per rect: the boxes of the frame's neighbourhoods.
static void launch_temporal_boxes(ft_context* c, const ftk::TemporalBox& box, int32_t& n_launches) {
    const ft_context::Temporal& T = c->temporal;
    for (const ft_rect& r : T.rects) {
        ftk::launch_temporal_box(c->stream, ftk::TemporalBoxArgs{c->d_out.as<double>(), T.d_mask.as<uint8_t>(), box, T.res_h, T.res_v, r.x0, r.y0, r.w, r.h, T.clamp.radius, T.clamp.gamma, T.clamp.floor});
        ++n_launches;
    }
}
// The records a window's k_temporal reads beside the sets: null where the call does not move / follow.
struct TemporalRecords { const double* motion = nullptr; const ftk::TemporalDeformLeaf* deform = nullptr; const double* snap = nullptr; };
// k_temporal's arguments for the window `win`, from the accumulation as it stands before the call's flip.
static ftk::TemporalArgs temporal_args(ft_context* c, const ftk::GuideWindow& win, const ft_temporal_params& P, bool want_rgb, bool want_rgba8, const TemporalRecords& rec,
                                       const ftk::TemporalBox& box) {
    const ft_context::Temporal& T = c->temporal;
    const size_t n_px = (size_t)T.res_h * (size_t)T.res_v;
    ftk::TemporalArgs a{};
    a.win = win;
    a.frame = c->d_out.as<double>();
    a.prev = temporal_set(T.d_set[T.prev], n_px); a.cur = temporal_set(T.d_set[T.prev ^ 1], n_px);
    for (int k = 0; k < 3; ++k) { a.o[k] = T.cam.o[k]; a.i[k] = T.cam.i[k]; a.j[k] = T.cam.j[k]; a.k[k] = T.cam.k[k]; }
    a.tlx = T.cam.tlx; a.tly = T.cam.tly; a.pw = T.cam.pw; a.ph = T.cam.ph;
    a.res_h = T.res_h; a.res_v = T.res_v; a.has_prev = T.calls > 0 ? 1 : 0;
    a.max_history = (double)P.max_history; a.min_normal_dot = P.min_normal_dot;
    a.tol_scale = P.position_tolerance_px * std::max(T.cam.pw, T.cam.ph);
    a.out_rgb = want_rgb ? T.d_rgb.as<double>() : nullptr; a.out8 = want_rgba8 ? T.d_rgba8.as<uint8_t>() : nullptr;
    a.counters = T.d_ctr.as<unsigned long long>();
    a.motion = rec.motion; a.n_leaves = (uint32_t)c->flat.leaves.size();
    if (rec.deform) { a.deform = rec.deform; a.tris = geo_array(c, kTris).as<double>(); a.snap = rec.snap; }
    a.box = box; a.clamped_history = (double)T.clamp.clamped_history;
    return a;
}
// The host's half of a successful accumulate, blocking or queued: the pose the set just written belongs to, the snapshots it has caught
// up with, the flip, cam' and the call count.
static void temporal_advance(ft_context* c, const ftk::Camera& cam, bool moving) {
    ft_context::Temporal& T = c->temporal;
    const size_t n_leaves = c->flat.leaves.size();
    if (T.calls == 0 || moving) {
        T.h_m2w = c->flat.m2w;
        T.h_w2m.resize(12 * n_leaves);
        for (size_t l = 0; l < n_leaves; ++l) std::memcpy(&T.h_w2m[12 * l], c->flat.leaves[l].w2m, 12 * sizeof(double));
        T.pose = c->pose_serial;
    }
    temporal_drop_snapshots(c);                                     // the set just written saw the meshes as they are
    T.prev ^= 1; T.cam = cam; T.calls += 1;
}

static int32_t temporal_single(ft_context* c, const RenderRequest& q, int32_t sample, const ft_temporal_params& P, bool rgba8, void* out, ft_stats* stats) {
    const auto wall0 = std::chrono::steady_clock::now();
    int32_t rc;
    if ((rc = begin_pass(c, stats)) != FT_OK) return rc;
    ft_context::Temporal& T = c->temporal;
    if ((rc = need_fp64_frame(c, "ft_temporal_accumulate", T.res_h, T.res_v, "accumulation", " than ft_temporal_begin fixed")) != FT_OK) return rc;
    std::vector<uint32_t> px;
    (void)list_pixels(T.rects, T.res_h, px);
    if (!need_committed(c)) return FT_ERR_STATE;
    if ((rc = drain_frame_streams(c)) != FT_OK) return rc;          // the frame may have been written on another stream (fetch_single)
    const size_t n_px = (size_t)T.res_h * (size_t)T.res_v;
    const bool want_rgb = P.to_frame || (out && !rgba8), want_rgba8 = out && rgba8;
    if (want_rgb && (rc = ensure(c, T.d_rgb, n_px * 24)) != FT_OK) return rc;
    if (want_rgba8 && (rc = ensure(c, T.d_rgba8, n_px * 4)) != FT_OK) return rc;
    FT_HIP(c, hipMemsetAsync(T.d_ctr.p, 0, 3 * sizeof(unsigned long long), c->stream));
    T.ctr_clean = false;
    const ftk::Camera cam = make_camera(*q.cam, T.res_h, T.res_v);
    // The scene was committed in another pose since the history was written (ft_scene_commit_moved, perhaps several times: H is the
    // pose of the last accumulate, so they compose): every leaf's way back to that pose goes up and k_temporal<true> runs.
    const size_t n_leaves = c->flat.leaves.size();
    const bool moving = T.calls > 0 && T.pose != c->pose_serial;
    // "temporal_follow_deformed": meshes were refit since the history was written and their records of then are kept: k_temporal<true, true>
    // runs, with the triangle plane in its windows
    const bool following = c->opt.temporal_follow_deformed && T.calls > 0 && !T.snaps.empty();
    if (moving || following) {
        if (T.h_m2w.size() != 12 * n_leaves || T.h_w2m.size() != 12 * n_leaves) { c->err = "ft_temporal_accumulate: the scene has other leaves than the history"; return FT_ERR_STATE; }
        if (moving && (rc = upload(c, T.d_motion, temporal_motion(c->flat, T.h_m2w, T.h_w2m))) != FT_OK) return rc;
        if (following && (rc = upload(c, T.d_deform, temporal_deform(c->flat, T))) != FT_OK) return rc;
        FT_HIP(c, hipStreamSynchronize(c->stream));                 // (the records are a temporary)
    }
    double kernel_ms = 0.0;
    int32_t n_launches = 0;
    // The clamp is on (ft_temporal_set_clamp): the boxes of the frame's neighbourhoods, one k_temporal_box per rect in front of the first
    // window.  They depend on the frame alone, so a call that runs again for longer hit lists writes the same boxes again.
    ftk::TemporalBox box{};
    if (T.clamp.radius > 0 && !px.empty()) {
        if ((rc = temporal_box_planes(c, box)) != FT_OK) return rc;
        if ((rc = T.timer.run(c, kernel_ms, [&] { launch_temporal_boxes(c, box, n_launches); })) != FT_OK) return rc;
    }
    AovRun run;
    const bool want[8] = {false, true, true, false, false, true, false, following};   // p, n, leaf; the triangle only in a call that follows
    TemporalRecords rec;
    if (moving) rec.motion = T.d_motion.as<double>();
    if (following) { rec.deform = T.d_deform.as<ftk::TemporalDeformLeaf>(); rec.snap = T.d_snap.as<double>(); }
    rc = aov_windows(c, q, sample, want, px, run, [&](int64_t p0, uint32_t n, const AovPlanes& pl, char* dev) -> int32_t {
        const ftk::TemporalArgs a = temporal_args(c, guide_window(c->aov.d_pixels.as<uint32_t>(), p0, n, pl, dev), P, want_rgb, want_rgba8, rec, box);
        ++n_launches;
        return T.timer.run(c, kernel_ms, [&] { ftk::launch_temporal(c->stream, a); });
    });
    if (rc != FT_OK) return rc;                                     // nothing was flipped: the history is as it was
    unsigned long long ctr[3] = {0, 0, 0};
    if (!px.empty() && (rc = read_counters(c, T.d_ctr, ctr, 3)) != FT_OK) return rc;
    if (out && (rc = copy_rects_out(c, out, rgba8 ? T.d_rgba8.p : T.d_rgb.p, rgba8 ? 4 : 24, T.res_h, T.rects, nullptr)) != FT_OK) return rc;
    if (P.to_frame && !px.empty() && (rc = temporal_to_frame(c, T.d_rgb.p)) != FT_OK) return rc;   // the means replace the tile pixels of the frame, once the call can no longer fail
    temporal_advance(c, cam, moving);
    T.with_history = (int64_t)ctr[0]; T.at_max = (int64_t)ctr[1]; T.clamped = (int64_t)ctr[2];
    end_pass(stats, run, kernel_ms, n_launches, wall0);
    if (stats) stats->trace_kernel_ms = run.kernel_ms;
    return FT_OK;
}

// The argument checks of ft_temporal_accumulate, which ft_temporal_enqueue makes in the same order under its own name.
static int32_t check_accumulate_args(ft_context* c, const std::string& api, const ft_camera* cam, int32_t spp, const double* jitter_xy, int32_t sample, const ft_temporal_params* params) {
    int32_t rc;
    if ((rc = check_guide_sample(c, api, spp, jitter_xy, sample, " to take the surfaces from")) != FT_OK) return rc;
    if (!cam || !params) { c->err = api + ": null cam or params"; return FT_ERR_INVALID; }
    const ft_temporal_params& P = *params;
    if (P.max_history < 1) { c->err = api + ": max_history below 1"; return FT_ERR_INVALID; }
    if (!(P.min_normal_dot >= -1.0 && P.min_normal_dot <= 1.0)) { c->err = api + ": min_normal_dot is NaN or outside [-1, 1]"; return FT_ERR_INVALID; }
    if (!(P.position_tolerance_px > 0.0)) { c->err = api + ": position_tolerance_px is not > 0"; return FT_ERR_INVALID; }
    return FT_OK;
}

int32_t ft_temporal_accumulate(ft_context* c, const ft_camera* cam, int32_t spp, const double* jitter_xy, int32_t sample, uint64_t seed,
                               const ft_temporal_params* params, int32_t rgba8, void* out, ft_stats* stats) {
    if (!c) return FT_ERR_INVALID;
    int32_t rc;
    if ((rc = check_accumulate_args(c, "ft_temporal_accumulate", cam, spp, jitter_xy, sample, params)) != FT_OK) return rc;
    const ft_temporal_params& P = *params;
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    if ((rc = need_one_device(c, "ft_temporal_accumulate")) != FT_OK) return rc;
    if (!c->temporal.open) { c->err = kNoTemporalEnded; return FT_ERR_STATE; }
    const RenderRequest q{cam, c->temporal.res_h, c->temporal.res_v, spp, jitter_xy, 0, seed, nullptr, 0, 0};   // (the pixel list is made from the begin's rects)
    return with_growing_hit_lists(c, [&] { return temporal_single(c, q, sample, P, rgba8 != 0, out, stats); });
}

// ft_temporal_filter (functracer_hip.h): the set the last accumulate wrote, filtered in place.  Only the filter's own
// planes are written until the call can no longer fail; the sets, cam', the counts, the cached pixel list and the level hint are not
// touched.  Without `demodulate` there is no guide pass, no pixel list and no upload: the class plane is filled per rect and the
// kernels run over rects and the frame.
// The steps ft_temporal_filter and ft_temporal_enqueue share.  The filter's planes: allocated by the first filter of the accumulation; the
// class plane is filled here - outside everywhere, then "in the tiles" per rect: k_tfilter_prepare makes that hit or miss.
static int32_t tfilter_planes(ft_context* c, bool demodulate, bool want8, ftk::TFilterPlanes& g) {
    ft_context::Temporal& T = c->temporal;
    const size_t n_px = (size_t)T.res_h * (size_t)T.res_v;
    int32_t rc;
    if (demodulate && (rc = ensure(c, T.d_fd, n_px * 24)) != FT_OK) return rc;
    if ((rc = ensure(c, T.d_fcls, n_px)) != FT_OK) return rc;
    for (int k = 0; k < 2; ++k) {
        if ((rc = ensure(c, T.d_fu[k], n_px * 24)) != FT_OK) return rc;
        if ((rc = ensure(c, T.d_fv[k], n_px * 8)) != FT_OK) return rc;
    }
    if (want8 && (rc = ensure(c, T.d_f8, n_px * 4)) != FT_OK) return rc;
    if (demodulate) for (int k = 0; k < 3; ++k) g.d[k] = T.d_fd.as<double>() + (size_t)k * n_px;
    g.cls = T.d_fcls.as<uint8_t>();
    FT_HIP(c, hipMemsetAsync(g.cls, ftk::kDenoiseOutside, n_px, c->stream));
    for (const ft_rect& r : T.rects)
        FT_HIP(c, hipMemset2DAsync(g.cls + (size_t)r.y0 * (size_t)T.res_h + (size_t)r.x0, (size_t)T.res_h, ftk::kDenoiseMiss, (size_t)r.w, (size_t)r.h, c->stream));
    return FT_OK;
}
// k_tfilter_prepare per rect and the iterations; result / variance: where the last one left them (prepare's planes without iterations).
static void launch_tfilter_passes(ft_context* c, const ft_temporal_filter_params& P, const ftk::TemporalSet& set, const ftk::TFilterPlanes& g, bool want8, bool want_rgb,
                                  int32_t& n_launches, const void*& result, const double*& variance) {
    const ft_context::Temporal& T = c->temporal;
    for (const ft_rect& r : T.rects) {
        ftk::TFilterPrepareArgs a{};
        a.set = set; a.g = g; a.u0 = T.d_fu[0].as<double>(); a.v0 = T.d_fv[0].as<double>();
        a.raw = P.iterations == 0 ? 1 : 0; a.out8 = a.raw && want8 ? T.d_f8.as<uint8_t>() : nullptr;
        a.res_h = T.res_h; a.res_v = T.res_v; a.x0 = r.x0; a.y0 = r.y0; a.w = r.w; a.h = r.h;
        a.min_history = (double)P.min_history; a.inv_sn2 = inv_sq(P.sigma_normal); a.inv_sp2 = inv_sq(P.sigma_position);
        ftk::launch_tfilter_prepare(c->stream, a);
        ++n_launches;
    }
    for (int i = 0; i < P.iterations; ++i) {
        const bool last = i + 1 == P.iterations;
        ftk::TFilterArgs a{};
        a.u_in = T.d_fu[i & 1].as<double>(); a.v_in = T.d_fv[i & 1].as<double>();
        a.u_out = !last || want_rgb ? T.d_fu[(i + 1) & 1].as<double>() : nullptr; a.v_out = T.d_fv[(i + 1) & 1].as<double>();
        a.out8 = last && want8 ? T.d_f8.as<uint8_t>() : nullptr;
        a.set = set; a.g = g; a.res_h = T.res_h; a.res_v = T.res_v; a.step = 1 << i;
        a.inv_sn2 = inv_sq(P.sigma_normal); a.inv_sp2 = inv_sq(P.sigma_position); a.inv_sc2 = inv_sq(P.sigma_colour); a.variance_floor = P.variance_floor;
        ftk::launch_tfilter(c->stream, a, last);
        ++n_launches;
        if (last) { result = a.u_out; variance = a.v_out; }
    }
}

static int32_t temporal_filter_single(ft_context* c, const RenderRequest& q, int32_t sample, const ft_temporal_filter_params& P, bool rgba8, void* out,
                                      double* out_variance, ft_stats* stats) {
    const auto wall0 = std::chrono::steady_clock::now();
    int32_t rc;
    if ((rc = begin_pass(c, stats)) != FT_OK) return rc;
    ft_context::Temporal& T = c->temporal;
    if (P.to_frame && (rc = need_fp64_frame(c, "ft_temporal_filter", T.res_h, T.res_v, "filter's to_frame", " than ft_temporal_begin fixed")) != FT_OK) return rc;
    AovRun run;
    if (T.n_pix == 0) { end_pass(stats, run, 0.0, 0, wall0); return FT_OK; }
    if (P.demodulate && !need_committed(c)) return FT_ERR_STATE;
    if ((rc = drain_frame_streams(c)) != FT_OK) return rc;          // the frame may have been written on another stream (fetch_single)
    const size_t n_px = (size_t)T.res_h * (size_t)T.res_v;
    const bool want8 = out && rgba8, want_rgb = P.to_frame || (out && !rgba8);
    const ftk::TemporalSet set = temporal_set(T.d_set[T.prev], n_px);
    ftk::TFilterPlanes g{};
    if ((rc = tfilter_planes(c, P.demodulate != 0, want8, g)) != FT_OK) return rc;
    double kernel_ms = 0.0;
    int32_t n_launches = 0;
    TimedLaunch& timer = T.ftimer;
    if (P.demodulate) {
        std::vector<uint32_t> px;
        (void)list_pixels(T.rects, T.res_h, px);
        const bool want[8] = {false, false, false, true, false, true, false, false};   // colour, leaf
        rc = aov_windows(c, q, sample, want, px, run, [&](int64_t p0, uint32_t n, const AovPlanes& pl, char* dev) -> int32_t {
            ftk::TFilterScatterArgs a{};
            a.win = guide_window(c->aov.d_pixels.as<uint32_t>(), p0, n, pl, dev);
            a.set_leaf = set.leaf; a.albedo_floor = P.albedo_floor;
            for (int k = 0; k < 3; ++k) a.d[k] = T.d_fd.as<double>() + (size_t)k * n_px;
            ++n_launches;
            return timer.run(c, kernel_ms, [&] { ftk::launch_tfilter_scatter(c->stream, a); });
        });
        if (rc != FT_OK) return rc;
    }
    const void* result = T.d_fu[0].p;                               // no iterations: prepare's M
    const double* variance = T.d_fv[0].as<double>();
    // one bracket around prepare and all iterations
    if ((rc = timer.run(c, kernel_ms, [&] { launch_tfilter_passes(c, P, set, g, want8, want_rgb, n_launches, result, variance); })) != FT_OK) return rc;
    if (out && (rc = copy_rects_out(c, out, rgba8 ? T.d_f8.p : result, rgba8 ? 4 : 24, T.res_h, T.rects, nullptr)) != FT_OK) return rc;
    if (out_variance && (rc = copy_rects_out(c, out_variance, variance, 8, T.res_h, T.rects, nullptr)) != FT_OK) return rc;
    if (P.to_frame && (rc = temporal_to_frame(c, result)) != FT_OK) return rc;   // the result replaces them, once the call can no longer fail
    end_pass(stats, run, kernel_ms, n_launches, wall0);
    if (stats) stats->trace_kernel_ms = run.kernel_ms;
    return FT_OK;
}

// The argument checks of ft_temporal_filter behind its null tests, which ft_temporal_enqueue makes in the same order under its own name.
static int32_t check_tfilter_args(ft_context* c, const std::string& api, const ft_camera* cam, int32_t spp, const double* jitter_xy, int32_t sample, const ft_temporal_filter_params& P) {
    int32_t rc;
    if ((rc = check_filter_params(c, api, P.iterations, P.sigma_colour, P.sigma_normal, P.sigma_position)) != FT_OK) return rc;
    if (P.min_history < 1) { c->err = api + ": min_history below 1"; return FT_ERR_INVALID; }
    if (!(P.variance_floor > 0.0)) { c->err = api + ": variance_floor is not > 0"; return FT_ERR_INVALID; }
    if ((rc = check_albedo_floor(c, api, P.demodulate, P.albedo_floor)) != FT_OK) return rc;
    if (P.demodulate) {
        if ((rc = check_guide_sample(c, api, spp, jitter_xy, sample, " to take the material colour from")) != FT_OK) return rc;
        if (!cam) { c->err = api + ": demodulate needs the camera of the accumulate call"; return FT_ERR_INVALID; }
    }
    return FT_OK;
}

int32_t ft_temporal_filter(ft_context* c, const ft_camera* cam, int32_t spp, const double* jitter_xy, int32_t sample, uint64_t seed,
                           const ft_temporal_filter_params* params, int32_t rgba8, void* out, double* out_variance, ft_stats* stats) {
    if (!c) return FT_ERR_INVALID;
    if (!params || (!out && !out_variance)) { c->err = "ft_temporal_filter: null params, or neither out nor out_variance"; return FT_ERR_INVALID; }
    const ft_temporal_filter_params& P = *params;
    int32_t rc;
    if ((rc = check_tfilter_args(c, "ft_temporal_filter", cam, spp, jitter_xy, sample, P)) != FT_OK) return rc;
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    if ((rc = need_one_device(c, "ft_temporal_filter")) != FT_OK) return rc;
    if (!c->temporal.open) { c->err = kNoTemporalEnded; return FT_ERR_STATE; }
    if (c->temporal.calls == 0) { c->err = "ft_temporal_filter: no ft_temporal_accumulate since ft_temporal_begin"; return FT_ERR_STATE; }
    if (P.demodulate && c->temporal.pose != c->pose_serial) {
        c->err = "ft_temporal_filter: demodulate after ft_scene_commit_moved needs an ft_temporal_accumulate first (the guide pass would show another pose than the set)";
        return FT_ERR_STATE;
    }
    const RenderRequest q{cam, c->temporal.res_h, c->temporal.res_v, spp, jitter_xy, 0, seed, nullptr, 0, 0};   // (read with demodulate only)
    return with_growing_hit_lists(c, [&] { return temporal_filter_single(c, q, sample, P, rgba8 != 0, out, out_variance, stats); });
}

// ------------------------------------------------------------------------------------------ queued temporal calls
// ft_temporal_enqueue / ft_temporal_wait (functracer_hip.h).  The call is the blocking pair's kernels, launched as they
// are, in the pair's order on the context's first main stream with nothing between them but stream order: no host wait between windows,
// one event pair around the lot, and k_temporal_report as the last kernel, which hands the counts to the slot's pinned record.  What the
// blocking calls do on the host once the device has finished - the flip, cam', the pose, the snapshot drop - happens when the call is
// queued; the counts arrive when it retires.  DESIGN.md 12.2 lists every buffer the call shares with a frame or another call and what
// orders the two.
} // extern "C"

// A buffer that queued calls may still be using is not freed under them: everything they queue is on the context's first main stream.
static int32_t ensure_quiet(ft_context* c, DeviceBuf& b, size_t bytes) {
    if (b.p && b.bytes < std::max<size_t>(bytes, 16) && c->temporal.q_pending > 0) FT_HIP(c, hipStreamSynchronize(c->stream));
    return ensure(c, b, bytes);
}
template <class T> static int32_t upload_quiet(ft_context* c, DeviceBuf& b, const std::vector<T>& v) {
    const int32_t rc = ensure_quiet(c, b, v.size() * sizeof(T));
    return rc != FT_OK ? rc : upload(c, b, v);
}

// Waits for the call in slot S and takes its counts; `stats`, when given, receives the call's.
static int32_t retire_temporal_slot(ft_context* c, ft_context::Temporal::QueueSlot& S, ft_stats* stats) {
    ft_context::Temporal& T = c->temporal;
    FT_HIP(c, hipEventSynchronize(S.ev[1]));
    const ftk::TemporalReport r = *S.h_report;
    S.d_snap.release();                                             // the snapshots the call followed
    T.with_history = (int64_t)r.with_history; T.at_max = (int64_t)r.at_max; T.clamped = (int64_t)r.clamped;
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        stats->rays_primary = (uint64_t)S.n_pix; stats->hits_primary = r.hits;
        stats->n_launches = S.n_launches;
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, S.ev[0], S.ev[1]) == hipSuccess) stats->kernel_ms = ms;
        stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - S.wall0).count();
    }
    if (r.overflow) {
        c->err = "ft_temporal_enqueue: CSG hit list overflow in the guide pass of a queued call; the accumulation is ended (one blocking ft_render or "
                 "ft_temporal_accumulate grows the lists, which stay: then ft_temporal_begin again)";
        return FT_ERR_OVERFLOW;
    }
    return FT_OK;
}

namespace ftc {
int32_t retire_temporal(ft_context* c, ft_stats* stats) {
    ft_context::Temporal& T = c->temporal;
    if (T.q_pending == 0) return FT_OK;
    FT_HIP(c, hipSetDevice(c->device));
    int32_t rc = FT_OK;
    std::string why;
    while (T.q_pending > 0) {                                       // oldest first; the statistics asked for are the newest call's
        ft_context::Temporal::QueueSlot& S = T.queue[(T.q_turn + ft_context::Temporal::kQueue - T.q_pending) % ft_context::Temporal::kQueue];
        const int32_t r = retire_temporal_slot(c, S, T.q_pending == 1 ? stats : nullptr);
        --T.q_pending;
        if (r != FT_OK && rc == FT_OK) { rc = r; why = c->err; }
    }
    T.fork_owed = false;                                            // the event behind the last reader of the frame has passed
    if (rc == FT_ERR_OVERFLOW) T.release();                         // later calls read a history written from overflowed rays: as ft_temporal_end
    if (rc != FT_OK) c->err = why;
    return rc;
}
int32_t retire_oldest_temporal(ft_context* c) {
    ft_context::Temporal& T = c->temporal;
    if (T.q_pending == 0) return FT_OK;
    FT_HIP(c, hipSetDevice(c->device));
    const int32_t rc = retire_temporal_slot(c, T.queue[(T.q_turn + ft_context::Temporal::kQueue - T.q_pending) % ft_context::Temporal::kQueue], nullptr);
    --T.q_pending;
    if (T.q_pending == 0) T.fork_owed = false;
    if (rc == FT_ERR_OVERFLOW) { const std::string why = c->err; (void)retire_temporal(c, nullptr); T.release(); c->err = why; }   // as retire_temporal ends it
    return rc;
}
} // namespace ftc

static int32_t temporal_enqueue_single(ft_context* c, const RenderRequest& q, int32_t sample, const ft_temporal_params& P, const ft_temporal_filter_params* F, bool rgba8, void* host_out) {
    using Temporal = ft_context::Temporal;
    const auto wall0 = std::chrono::steady_clock::now();
    int32_t rc;
    FT_HIP(c, hipSetDevice(c->device));
    Temporal& T = c->temporal;
    if ((rc = need_fp64_frame(c, "ft_temporal_enqueue", T.res_h, T.res_v, "accumulation", " than ft_temporal_begin fixed")) != FT_OK) return rc;
    if (!need_committed(c)) return FT_ERR_STATE;
    const size_t n_leaves = c->flat.leaves.size();
    const bool moving = T.calls > 0 && T.pose != c->pose_serial;
    const bool following = c->opt.temporal_follow_deformed && T.calls > 0 && !T.snaps.empty();
    if ((moving || following) && (T.h_m2w.size() != 12 * n_leaves || T.h_w2m.size() != 12 * n_leaves)) { c->err = "ft_temporal_enqueue: the scene has other leaves than the history"; return FT_ERR_STATE; }
    // The slot: call k + FT_TEMPORAL_QUEUE_DEPTH waits for call k here, on the host.  An error of that call is this call's answer (and
    // ends the wait for the others: their host buffers are the host's again).
    if (T.q_pending == Temporal::kQueue) {
        rc = retire_temporal_slot(c, T.queue[T.q_turn], nullptr);
        --T.q_pending;
        if (rc != FT_OK) {
            const std::string why = c->err;
            (void)retire_temporal(c, nullptr);
            if (rc == FT_ERR_OVERFLOW && T.open) T.release();
            c->err = why;
            return rc;
        }
    }
    Temporal::QueueSlot& S = T.queue[T.q_turn];
    if (!S.h_report) {
        FT_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&S.h_report), sizeof(ftk::TemporalReport), hipHostMallocDefault));
        FT_HIP(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&S.d_report), S.h_report, 0));
    }
    for (hipEvent_t& e : S.ev) if (!e) FT_HIP(c, hipEventCreate(&e));
    if (!T.fork) FT_HIP(c, hipEventCreateWithFlags(&T.fork, hipEventDisableTiming));
    const size_t n_px = (size_t)T.res_h * (size_t)T.res_v;
    const int64_t n_pix = T.n_pix;
    const bool filtering = F && n_pix > 0;                           // (the blocking filter returns at once over no pixels)
    const bool want_rgb = !F && host_out && !rgba8, want_rgba8 = !F && host_out && rgba8;   // the accumulate's own results: only when they leave
    if (want_rgb && (rc = ensure_quiet(c, T.d_rgb, n_px * 24)) != FT_OK) return rc;
    if (want_rgba8 && (rc = ensure_quiet(c, T.d_rgba8, n_px * 4)) != FT_OK) return rc;
    // Everything below is queued on the one stream, in the blocking pair's order.  First what the accumulation keeps for its queued calls.
    if (n_pix > 0 && T.q_pixels.empty()) {
        (void)list_pixels(T.rects, T.res_h, T.q_pixels);
        if ((rc = upload_quiet(c, T.d_qpixels, T.q_pixels)) != FT_OK) return rc;
    }
    {
        std::vector<double> jitter(q.jitter_xy, q.jitter_xy + 2 * (size_t)q.spp);
        if (jitter != T.q_jitter || !T.d_qjitter.p) {
            S.jitter = jitter;                                      // (the copy's source lives as long as the call)
            if ((rc = upload_quiet(c, T.d_qjitter, S.jitter)) != FT_OK) return rc;
            T.q_jitter.swap(jitter);
        }
    }
    if ((rc = ensure_quiet(c, c->aov.d_ctr, 2 * sizeof(unsigned long long))) != FT_OK) return rc;
    if (!T.ctr_clean) FT_HIP(c, hipMemsetAsync(T.d_ctr.p, 0, 3 * sizeof(unsigned long long), c->stream));
    if (!c->aov.ctr_clean) FT_HIP(c, hipMemsetAsync(c->aov.d_ctr.p, 0, 2 * sizeof(unsigned long long), c->stream));
    TemporalRecords rec;
    if (moving) {
        S.motion = temporal_motion(c->flat, T.h_m2w, T.h_w2m);
        if ((rc = upload_quiet(c, S.d_motion, S.motion)) != FT_OK) return rc;
        rec.motion = S.d_motion.as<double>();
    }
    if (following) {
        S.deform = temporal_deform(c->flat, T);
        if ((rc = upload_quiet(c, S.d_deform, S.deform)) != FT_OK) return rc;
        rec.deform = S.d_deform.as<ftk::TemporalDeformLeaf>(); rec.snap = T.d_snap.as<double>();
    }
    const int64_t per = guide_window_size(c, n_pix);
    const bool want[8] = {false, true, true, filtering && F->demodulate, false, true, false, following};   // p, n, leaf; the colour for the filter's d; the triangle in a call that follows
    const AovPlanes pl = aov_planes(want, per);
    if (n_pix > 0 && (rc = ensure_quiet(c, c->aov.d_out, (size_t)per * pl.bytes_per_entry)) != FT_OK) return rc;
    ftk::TemporalBox box{};
    const bool clamping = T.clamp.radius > 0 && n_pix > 0;
    if (clamping && (rc = temporal_box_planes(c, box)) != FT_OK) return rc;
    ftk::TFilterPlanes g{};
    // Join: the frame this call reads may still be on its way on the frame driver's other streams - k_resolve on `tail`, the tracing of
    // simple frames on the further mains (the first main is this call's own stream).  Waits on the device only.
    if (n_pix > 0 && any_pending(c)) {
        bool on[ft_context::kMains] = {};
        for (const ft_context::FrameSlot& f : c->slots) if (f.pending) { on[0] = on[0] || f.simple; if (f.main_ix > 0) on[f.main_ix] = true; }
        for (int k = 0; k < ft_context::kMains; ++k) {
            if (!on[k]) continue;
            if (!T.join[k]) FT_HIP(c, hipEventCreateWithFlags(&T.join[k], hipEventDisableTiming));
            FT_HIP(c, hipEventRecord(T.join[k], k == 0 ? c->tail : c->more_mains[k - 1]));
            FT_HIP(c, hipStreamWaitEvent(c->stream, T.join[k], 0));
        }
    }
    FT_HIP(c, hipEventRecord(S.ev[0], c->stream));
    int32_t n_launches = 0;
    if (clamping) launch_temporal_boxes(c, box, n_launches);
    const ftk::TemporalSet written = temporal_set(T.d_set[T.prev ^ 1], n_px);   // the set this call writes: the filter's input
    if (filtering) {
        const bool want8 = rgba8;
        if ((rc = tfilter_planes(c, F->demodulate != 0, want8, g)) != FT_OK) return rc;
    }
    const ftk::Camera cam = make_camera(*q.cam, T.res_h, T.res_v);
    char* const dev = c->aov.d_out.as<char>();
    for (int64_t p0 = 0; p0 < n_pix; p0 += per) {
        const uint32_t n = (uint32_t)std::min<int64_t>(per, n_pix - p0);
        launch_guide_window(c, q, sample, cam, T.d_qpixels.as<uint32_t>(), T.d_qjitter.as<double>(), p0, n, pl, dev);
        const ftk::GuideWindow win = guide_window(T.d_qpixels.as<uint32_t>(), p0, n, pl, dev);
        ftk::launch_temporal(c->stream, temporal_args(c, win, P, want_rgb, want_rgba8, rec, box));
        n_launches += 2;
        // Fork: behind the last kernel that reads the frame.  The next frame's writers of d_out wait for this event (queue_frame).
        if (p0 + per >= n_pix) { FT_HIP(c, hipEventRecord(T.fork, c->stream)); T.fork_owed = true; }
        if (filtering && F->demodulate) {                            // the filter's d from this window's colours: there is no second guide pass
            ftk::TFilterScatterArgs a{};
            a.win = win; a.set_leaf = written.leaf; a.albedo_floor = F->albedo_floor;
            for (int k = 0; k < 3; ++k) a.d[k] = T.d_fd.as<double>() + (size_t)k * n_px;
            ftk::launch_tfilter_scatter(c->stream, a);
            ++n_launches;
        }
    }
    if (!F && host_out && (rc = copy_rects_out(c, host_out, rgba8 ? T.d_rgba8.p : T.d_rgb.p, rgba8 ? 4 : 24, T.res_h, T.rects, c->stream)) != FT_OK) return rc;
    if (filtering) {
        const void* result = T.d_fu[0].p;
        const double* variance = T.d_fv[0].as<double>();
        launch_tfilter_passes(c, *F, written, g, rgba8, !rgba8, n_launches, result, variance);
        if ((rc = copy_rects_out(c, host_out, rgba8 ? T.d_f8.p : result, rgba8 ? 4 : 24, T.res_h, T.rects, c->stream)) != FT_OK) return rc;
    }
    ftk::launch_temporal_report(c->stream, T.d_ctr.as<unsigned long long>(), c->aov.d_ctr.as<unsigned long long>(), S.d_report);
    T.ctr_clean = c->aov.ctr_clean = true;
    FT_HIP(c, hipEventRecord(S.ev[1], c->stream));
    FT_HIP(c, hipGetLastError());
    // The host's half, now: the snapshots this call follows stay alive in its slot, everything else as the blocking call leaves it.
    S.d_snap.release();
    if (following) { S.d_snap = T.d_snap; T.d_snap = DeviceBuf{}; }
    temporal_advance(c, cam, moving);
    S.n_pix = n_pix; S.n_launches = n_launches; S.wall0 = wall0;
    S.pose_set = c->pose.live;                                      // the guide passes above were given dev_scene as it points now
    S.geo_set = c->geo.live;
    T.q_turn = (T.q_turn + 1) % Temporal::kQueue; ++T.q_pending;
    return FT_OK;
}

extern "C" {

int32_t ft_temporal_enqueue(ft_context* c, const ft_camera* cam, int32_t spp, const double* jitter_xy, int32_t sample, uint64_t seed,
                            const ft_temporal_params* params, const ft_temporal_filter_params* filter, int32_t rgba8, void* host_out) {
    if (!c) return FT_ERR_INVALID;
    static const std::string api = "ft_temporal_enqueue";
    int32_t rc;
    if ((rc = check_accumulate_args(c, api, cam, spp, jitter_xy, sample, params)) != FT_OK) return rc;
    if (filter) {
        if (!host_out) { c->err = api + ": a filter needs host_out (the filtered frame has nowhere else to go)"; return FT_ERR_INVALID; }
        if ((rc = check_tfilter_args(c, api, cam, spp, jitter_xy, sample, *filter)) != FT_OK) return rc;
    }
    if (params->to_frame) { c->err = api + ": to_frame is not offered in the queued call (it would write the frame a queued frame may be writing): use the blocking ft_temporal_accumulate"; return FT_ERR_INVALID; }
    if (filter && filter->to_frame) { c->err = api + ": the filter's to_frame is not offered in the queued call: use the blocking ft_temporal_filter"; return FT_ERR_INVALID; }
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    if ((rc = need_one_device(c, api)) != FT_OK) return rc;
    if (!c->temporal.open) { c->err = kNoTemporalEnded; return FT_ERR_STATE; }
    const RenderRequest q{cam, c->temporal.res_h, c->temporal.res_v, spp, jitter_xy, 0, seed, nullptr, 0, 0};
    return temporal_enqueue_single(c, q, sample, *params, filter, rgba8 != 0, host_out);
}

int32_t ft_temporal_wait(ft_context* c, ft_stats* stats) {
    if (!c) return FT_ERR_INVALID;
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    if (stats) std::memset(stats, 0, sizeof *stats);
    return retire_temporal(c, stats);
}

// The calls below answer from the host's copy of the accumulation's state: queued calls are retired first.
int32_t ft_temporal_fetch(ft_context* c, double* mean_rgb, double* stderr_rgb, double* length) {
    if (!c) return FT_ERR_INVALID;
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    int32_t qrc;
    if ((qrc = retire_temporal(c, nullptr)) != FT_OK) return qrc;
    const ft_context::Temporal& T = c->temporal;
    if (!T.open) { c->err = kNoTemporal; return FT_ERR_STATE; }
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
    int32_t qrc;
    if ((qrc = retire_temporal(c, nullptr)) != FT_OK) return qrc;
    const ft_context::Temporal& T = c->temporal;
    if (!T.open) { c->err = kNoTemporal; return FT_ERR_STATE; }
    out[0] = T.calls; out[1] = T.n_pix; out[2] = T.with_history; out[3] = T.at_max;
    return FT_OK;
}

int32_t ft_temporal_set_clamp(ft_context* c, const ft_temporal_clamp_params* params) {
    if (!c) return FT_ERR_INVALID;
    if (params) {
        const ft_temporal_clamp_params& P = *params;
        if (P.radius < 1 || P.radius > ftk::kTemporalClampMaxRadius) { c->err = "ft_temporal_set_clamp: radius outside 1 .. 3"; return FT_ERR_INVALID; }
        if (P.clamped_history < 0) { c->err = "ft_temporal_set_clamp: clamped_history below 0"; return FT_ERR_INVALID; }
        if (!(P.gamma >= 0.0) || !std::isfinite(P.gamma)) { c->err = "ft_temporal_set_clamp: gamma is negative or not finite"; return FT_ERR_INVALID; }
        if (!(P.floor >= 0.0) || !std::isfinite(P.floor)) { c->err = "ft_temporal_set_clamp: floor is negative or not finite"; return FT_ERR_INVALID; }
    }
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    int32_t rc;
    if ((rc = need_one_device(c, "ft_temporal_set_clamp")) != FT_OK) return rc;
    ft_context::Temporal& T = c->temporal;
    if (!T.open) { c->err = kNoTemporalEnded; return FT_ERR_STATE; }
    T.clamp = params ? *params : ft_temporal_clamp_params{};       // (radius 0: off; what is accumulated stays as it is)
    return FT_OK;
}

int32_t ft_temporal_clamp_status(ft_context* c, int64_t out[2]) {
    if (!c || !out) return FT_ERR_INVALID;
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    int32_t qrc;
    if ((qrc = retire_temporal(c, nullptr)) != FT_OK) return qrc;
    const ft_context::Temporal& T = c->temporal;
    if (!T.open) { c->err = kNoTemporal; return FT_ERR_STATE; }
    out[0] = T.clamp.radius; out[1] = T.clamped;
    return FT_OK;
}

int32_t ft_temporal_end(ft_context* c) {
    if (!c) return FT_ERR_INVALID;
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    const int32_t qrc = retire_temporal(c, nullptr);                // an error among the queued calls is reported; the accumulation ends either way
    temporal_close(c);
    return qrc;
}

} // extern "C"

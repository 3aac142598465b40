// ft_frame.cpp — the frame driver behind the ft_render family: a frame is planned on the host, queued on the device's streams and retired;
// on a context over several devices every device takes its bands of it.
#include "ft_context.h"

namespace ftc {

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


// Image-tile partition of a region over the devices of a context: 8-row bands of every requested rect, dealt round-robin.
std::vector<std::vector<ft_rect>> band_shares(const RenderRequest& q, size_t n_devs) {
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

int32_t check_request(ft_context* c, const RenderRequest& q) {
    if (!q.cam || q.res_h < 2 || q.res_v < 2 || q.spp < 0 || (q.spp > 0 && !q.jitter_xy) || q.max_depth < 0 || (q.tiles && q.n_tiles < 1)) { c->err = "bad ft_render argument"; return FT_ERR_INVALID; }
    if (q.max_depth > ftk::kMaxBounce) { c->err = "max_depth above 16"; return FT_ERR_UNSUPPORTED; }
    if ((int64_t)q.res_h * q.res_v > (int64_t)0x7FFFFFFF) { c->err = "resolution too large"; return FT_ERR_INVALID; }
    return FT_OK;
}

// Wait for a queued frame, add its stage times to the context's sums and fill its statistics.
static int32_t retire_frame(ft_context* c, ft_context::FrameSlot& F, ft_stats* stats) {
    if (!F.pending) return FT_OK;
    F.pending = false;
    // "classify_reuse": a frame that classified leaves its slot's buffers described by `kept` once it has ended without error; one that
    // read them as they were leaves them so.  Any error drops the record.
    const bool keeps = F.keeps, reuses = F.reuses;
    const bool held = F.kept.valid;                                 // (a change of option may have dropped the record under a queued frame)
    F.keeps = F.reuses = false;
    F.kept.valid = false;
    if (F.ev.ev1) FT_HIP(c, hipEventSynchronize(F.ev.ev1)); else FT_HIP(c, hipStreamSynchronize(c->stream));
    ftk::RenderCounters hrc = F.h_report->total;                    // the stripes, summed by the frame's last kernel
    const bool classify_failed = F.h_report->classify_error != 0;
    if (reuses) hrc.pixels_culled = F.kept.culled;                  // counted by the frame that classified; this one's stripes hold 0
    if ((keeps || (reuses && held)) && !classify_failed && !hrc.csg_overflow) {
        F.kept.valid = true;
        if (keeps) { F.kept.n_active = (int64_t)F.h_report->n_pix_active; F.kept.culled = hrc.pixels_culled; }
    }
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
int32_t retire_pending(ft_context* c, ft_stats* stats) {
    int32_t rc = FT_OK;
    int last = -1;
    for (int k = 0; k < ft_context::kSlots; ++k) if (c->slots[(c->slot_turn + k) % ft_context::kSlots].pending) last = k;
    for (int k = 0; k < ft_context::kSlots; ++k) {                  // oldest first; the statistics asked for are the newest frame's
        ft_context::FrameSlot& f = c->slots[(c->slot_turn + k) % ft_context::kSlots];
        if (f.pending) { int32_t r = retire_frame(c, f, k == last ? stats : nullptr); if (r != FT_OK) rc = r; }
    }
    return rc;
}

int32_t retire_oldest_frame(ft_context* c) {
    for (int k = 0; k < ft_context::kSlots; ++k) {
        ft_context::FrameSlot& f = c->slots[(c->slot_turn + k) % ft_context::kSlots];
        if (f.pending) return retire_frame(c, f, nullptr);
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
    int32_t list_leaf = -1;              // >= 0: the frame carries per-block candidate lists for this bare mesh leaf (k_block_lists)
    ftk::Camera cam{};
    // "classify_reuse": the key of what this frame's classification writes (keepable: a plain classified frame; a progressive pass's
    // depends on its retired blocks), whether the frame's slot already holds exactly that, and the windows a frame that classifies is
    // cut into - what ft_stats reports whichever way the frame runs.
    bool keepable = false, reuse = false;
    ClassifyKey key;
    int32_t n_planned = 0;
};

// Pixel list restricted to the tiles.  The reference enumerates pixels y-major, x (Image.fs:104); samples are
// independent, so the device is free to walk them in any order: rects whose sides are multiples of 8 are
// walked in 8x8 pixel blocks, which makes the 64 lanes of a wavefront a compact bundle of rays.
std::vector<ft_rect> clip_rects(const RenderRequest& q) {
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
bool list_pixels(const std::vector<ft_rect>& rects, int32_t res_h, std::vector<uint32_t>& px) {
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
    // net gain.  A frame that finds its classification in its slot ("classify_reuse", below) does know the length.
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
    // Candidate lists: classified frames in grouped numbering over a scene with exactly ONE bare mesh leaf that has a 4-wide BVH.  Scenes
    // with several such leaves and progressive passes keep the tree walk.
    if (c->opt.primary_block_lists && p.classify && !p.mask_only && !p.progressive && p.group_log2 > 0 && (c->variant & 4)) {
        int32_t leaf = -1, n_bare = 0;
        for (size_t k = 0; k + 1 < c->flat.item_pc.size(); ++k) {
            uint32_t w[3]; std::memcpy(w, &c->flat.cull_items[8 * k + 5], sizeof w);   // first coarse box, count, leaf
            if (w[1] != 0u) { ++n_bare; leaf = (int32_t)w[2]; }
        }
        if (n_bare == 1) {
            const uint32_t mesh = c->flat.leaves[leaf].mesh;
            if (c->flat.meshes[mesh].bvh_root != INT32_MIN && c->flat.mesh_wide[mesh] != INT32_MIN) p.list_leaf = leaf;
        }
    }
    p.zsig = p.signature;
    auto mix = [&](const void* v, size_t n) { const unsigned char* b = static_cast<const unsigned char*>(v); for (size_t k = 0; k < n; ++k) p.zsig = (p.zsig ^ b[k]) * 0x100000001B3ull; };
    mix(&p.cam, sizeof p.cam); mix(&p.jitter_extent, sizeof p.jitter_extent);
    if (!p.rects.empty()) mix(p.rects.data(), p.rects.size() * sizeof(ft_rect));
    p.zsig |= 1ull;                                              // never 0: 0 means "nothing known about the buffer"
    // Queued frames of one chunk put k_resolve on its own stream (blocking frames have nothing to hide it in).  A frame cut into many
    // windows (3840x2160x64: 16, most of them empty behind the classification) pays an event pair per window and gains nothing - the windows'
    // small launches already overlap on one stream (measured: 3.46 -> 3.63 ms with it, profiles/r03_z_overlap_by_scene.json)
    p.n_planned = (int32_t)p.jobs.size();
    // The slot this frame takes (its previous frame has been retired: render_single) may still hold this very classification.
    const ft_context::FrameSlot& F = c->slots[c->slot_turn];
    p.keepable = p.classify && !p.progressive && !p.mask_only;
    if (p.keepable) {
        p.key.commit_serial = c->commit_serial; p.key.res_h = q.res_h; p.key.res_v = q.res_v; p.key.list_leaf = p.list_leaf;
        p.key.jitter_extent = p.jitter_extent; p.key.cam = p.cam; p.key.rects = p.rects;
        p.reuse = c->opt.classify_reuse && !F.pending && F.kept.valid && F.kept.key == p.key;
    }
    // Such a frame knows its active list's length before anything is queued: its windows are cut from that list by the rule above, no
    // wider than the frame's own (p.cap and the buffers stay what a frame that classifies needs), and those past its end are not launched.
    // A frame without an active pixel still launches one: its k_resolve writes the finished blocks and hands the counters over.
    if (p.reuse) {
        const int64_t n_active = std::max<int64_t>(F.kept.n_active, std::min<int64_t>(64, n_pix_total));
        int64_t per = p.pix_per_chunk;
        if (per > 64) {
            const int64_t n_chunks = (n_active + per - 1) / per;
            per = std::min(per, ((n_active + n_chunks - 1) / n_chunks + 63) / 64 * 64);
        }
        p.jobs.clear();
        for (int64_t p0 = 0; p0 < n_active; p0 += per) {
            const uint32_t n = (uint32_t)std::min<int64_t>(per, n_active - p0);
            p.jobs.push_back(FramePlan::Job{(uint32_t)p0, n, 0, 0, (uint32_t)p0, n});
        }
    }
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
    ftk::PixCount* const kept = &F.d_fc.as<ftk::SlotCounters>()->kept;
    const ftk::ClassifyOut cls{F.d_block_pos.as<int32_t>(), F.d_pos_block.as<uint32_t>(), c->d_wave_counts.as<uint32_t>(), kept};
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
    // the block lists right behind the classification, on its stream and inside its event: they ride beside the predecessors' tracing too
    const ftk::BlockLists lists{F.d_list_heads.as<uint32_t>(), F.d_list_pool.as<uint32_t>(), (uint32_t)(F.d_list_pool.bytes / (ftk::kListEntryWords * 4)), p.list_leaf,
                                F.d_list_edges.bytes / (ftk::kEdgeFloats * 4) >= F.d_list_pool.bytes / (ftk::kListEntryWords * 4) ? F.d_list_edges.as<float>() : nullptr};   // (written whatever "edge_cull" says: a later frame may reuse the lists with it on)
    auto queue_lists = [&] { if (p.list_leaf >= 0) ftk::launch_block_lists(Lg, c->dev_scene, all, cls.pos_block, lists, p.jitter_extent, fc, kept); };
    if (ahead) {
        ftk::launch_classify(Lg, c->dev_scene, all, cls, p.jitter_extent, epoch, fc, retired, p.mask_only);
        queue_lists();
        FT_HIP(c, hipEventRecord(c->classified, c->side));
        FT_HIP(c, hipStreamWaitEvent(F.ev.ms, c->classified, 0));
    } else {
        F.ev.timed(kStageOther, [&] { ftk::launch_classify(Lg, c->dev_scene, all, cls, p.jitter_extent, epoch, fc, retired, p.mask_only); queue_lists(); });
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
    const ftk::PixCount* const kept = &F.d_fc.as<ftk::SlotCounters>()->kept;   // the active list's length: this frame's k_classify wrote it, or the one this frame reuses
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
        if (p.classify) { gen.counts = kept; gen.block_map = F.d_pos_block.as<uint32_t>(); }   // pix_base = job.id_base: the window's start in the active list
        if (p.list_leaf >= 0) { gen.list_heads = F.d_list_heads.as<uint32_t>(); gen.list_pool = F.d_list_pool.as<uint32_t>(); gen.list_leaf = p.list_leaf;
                                 // (the edge pool is sized with the entry pool and written by the k_block_lists that wrote that one)
                                 gen.list_edges = c->opt.edge_cull && F.d_list_edges.bytes / (ftk::kEdgeFloats * 4) >= F.d_list_pool.bytes / (ftk::kListEntryWords * 4) ? F.d_list_edges.as<float>() : nullptr; }
        gen.group_log2 = (n_pix % 64u == 0u) ? p.group_log2 : 0;
        const int at = c->acc_turn;
        double* const acc = c->d_acc[at].as<double>();
        if (c->acc_busy[at]) { FT_HIP(c, hipStreamWaitEvent(ms, c->acc_free[at], 0)); c->acc_busy[at] = false; E.fresh = false; }   // a k_resolve on `tail` may still be reading this copy
        // k_primary_mesh (option "primary_mesh_kernel") for the scene it is written for, in a plain frame of whole wavefronts: grouped numbering,
        // coherent waves, the one-leaf path on, no focus.  Anything else - progressive passes, corner sampling among it - takes k_primary.
        const bool mesh_kernel = c->opt.primary_mesh_kernel && c->mesh_kernel_scene && c->opt.coherent_waves && c->opt.uniform_surface && !p.progressive && !p.corner &&
                                 gen.group_log2 > 0 && !p.cam.has_focus;
        ftk::Launch Lj = Lp;
        if (mesh_kernel) { Lj.grid = c->n_cu * c->blocks_primary_mesh; Lj.lds_bytes = 0; Lj.variant |= ftk::kVariantMeshKernel; }
        ++c->primary_launches[mesh_kernel ? 1 : 0];
        E.timed(kStagePrimary, [&] { ftk::launch_primary(Lj, c->dev_scene, gen, rb[1], acc, n_samples, q.max_depth, fc); });
        auto bounce = [&](int b) { ftk::launch_bounce(Lb, c->dev_scene, gen, rb[b & 1], rb[(b + 1) & 1], acc, n_samples, b, q.max_depth, b == n_levels && n_levels < p.last_bounce, fc); };
        if (E.timing >= 2) for (int b = 1; b <= n_levels; ++b) E.timed(kStageShade, [&] { bounce(b); });
        else if (n_levels >= 1) E.timed(kStageShade, [&] { for (int b = 1; b <= n_levels; ++b) bounce(b); });
        n_launches += 2 + n_levels;                                 // k_primary, the levels, k_resolve
        if (!p.simple) for (int k = 0; k < ft_context::kAcc; ++k) if (c->acc_busy[k]) {   // a queued frame's k_resolve may still be writing the frame on `tail`: frames reach d_out in order
            FT_HIP(c, hipStreamWaitEvent(ms, c->acc_free[k], 0)); c->acc_busy[k] = false; E.fresh = false;
        }
        if (p.corner) { E.timed(kStageResolve, [&] { ftk::launch_resolve_corner(Lg, acc, n_samples, job.w, job.h, c->d_out_index.as<uint32_t>() + job.out_base, out_rgb, out_rgba); }); continue; }
        const ftk::ResolveArgs ra{acc, n_samples, p.classify ? kept : nullptr, job.id_base, n_pix, p.spp,
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
    n_launches += (p.n_planned - (int32_t)p.jobs.size()) * (2 + n_levels);   // ft_stats counts the windows not launched as well
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
    ft_context::FrameSlot& F = c->slots[turn];                     // (its previous frame was retired before this one was planned)
    if (!defer || !c->accum_open) { for (int k = 0; k < kStages; ++k) { c->k_ms[k] = 0; c->k_launches[k] = 0; } c->accum_open = defer; }   // queued frames sum their kernel times until a wait
    // What the slot keeps of its last classification stays true only through a frame that reads it as it is; a frame that classifies makes it
    // unknown until it retires, any other frame is not followed (it leaves the buffers alone but last_classified_slot moves on).
    F.keeps = p.keepable && !p.reuse; F.reuses = p.reuse;
    if (!p.reuse) F.kept.valid = false;
    if (F.keeps) F.kept.key = p.key;
    c->reuse_counts[p.reuse ? 1 : 0] += p.classify ? 1 : 0;
    c->reuse_counts[2] += (int64_t)p.jobs.size(); c->reuse_counts[3] += p.n_planned - (int64_t)p.jobs.size();
    if (p.reuse) {                                                 // the buffers are large enough: they hold this frame's classification
        F.list_leaf = p.list_leaf; F.list_cam = p.cam;
        c->last_classified_slot = turn;
    } else if (p.classify) {
        const size_t n_blocks = (size_t)p.n_pix_total / 64, n_waves = (n_blocks + 255) / 256;   // one word per k_classify workgroup
        if ((rc = ensure(c, F.d_block_pos, n_blocks * 4)) != FT_OK) return rc;
        if ((rc = ensure(c, F.d_pos_block, n_blocks * 4)) != FT_OK) return rc;
        if (p.list_leaf >= 0) {
            // a header per block; the pool is sized from the block count, 16 entries a block (a list holds 64 at most, the bunny's blocks
            // average under ten): blocks that find it full walk the tree
            if ((rc = ensure(c, F.d_list_heads, n_blocks * 4)) != FT_OK) return rc;
            if ((rc = ensure(c, F.d_list_pool, (16 * n_blocks + 4096) * ftk::kListEntryWords * 4)) != FT_OK) return rc;
            if ((rc = ensure(c, F.d_list_edges, F.d_list_pool.bytes / (ftk::kListEntryWords * 4) * ftk::kEdgeFloats * 4)) != FT_OK) return rc;
        }
        F.list_leaf = p.list_leaf; F.list_cam = p.cam;
        c->last_classified_slot = turn;
        if (c->d_wave_counts.bytes < n_waves * 4 || c->classify_epoch >= 0x3FFFFEu) {   // entries are tagged with the frame's epoch and never cleared in between
            if ((rc = ensure(c, c->d_wave_counts, std::max<size_t>(n_waves * 4, 4096) + 4096 * 4 + 2048 * 64)) != FT_OK) return rc;   // (+ room for the diagnostic build's stamps)
            FT_HIP(c, hipStreamSynchronize(c->side));              // (a classification of the other slot may still be publishing into the old words)
            FT_HIP(c, hipMemsetAsync(c->d_wave_counts.p, 0, c->d_wave_counts.bytes, c->stream));
            c->classify_epoch = 0;
            uploads_queued = true;
        }
    } else {
        F.list_leaf = -1;                                          // the slot's lists, if any, were its previous frame's
        c->last_classified_slot = -1;                              // (ft_debug_block_lists describes the LAST frame queued: not an older frame's lists, still in another slot)
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
    // A queued temporal call (ft_temporal_enqueue) may still be reading the FP64 frame this one overwrites: the stream this frame's
    // k_resolve / k_resolve_corner (and, inside k_resolve, the fill of the finished blocks) runs on waits for the event behind that
    // call's last reader.  The tracing kernels do not wait.  Taken only by the first FP64 frame queued after such a call.
    if (c->temporal.fork_owed && q.format == 0) {
        FT_HIP(c, hipStreamWaitEvent(p.simple ? c->tail : ms, c->temporal.fork, 0));
        c->temporal.fork_owed = false;
    }
    // chunk counters, statistic stripes, list length, tickets: cleared by the slot's previous frame's last kernel, or by a fill when there was none
    if (!F.fc_clean) { FT_HIP(c, hipMemsetAsync(F.d_fc.p, 0, sizeof(ftk::FrameCounters), ms)); uploads_queued = true; }
    F.fc_clean = false;                                            // until this frame's own hand-over is queued
    F.ev.begin(ms, (int)c->opt.timing);
    if (p.classify && !p.reuse && (rc = queue_classify(c, q, p, F, defer && c->opt.classify_ahead && !uploads_queued)) != FT_OK) return rc;
    if (!F.h_report) {
        FT_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&F.h_report), sizeof(ftk::FrameReport), hipHostMallocDefault));
        FT_HIP(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&F.d_report), F.h_report, 0));
    }
    int32_t n_launches = p.classify ? 1 : 0;                       // k_classify; k_block_lists rides behind it and is not counted (functracer_hip.h)
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
    F.pose_set = c->pose.live;                                     // every launch above was given dev_scene as it points now
    F.geo_set = c->geo.live;
    F.rays_primary = 0;
    if (p.corner) for (auto& j : p.jobs) F.rays_primary += (uint64_t)j.n_ids * (uint64_t)p.spp;
    else F.rays_primary = (uint64_t)p.n_pix_total * (uint64_t)p.spp;   // the windows of a pixel list cover it, launched or not
    F.n_pix_total = p.n_pix_total; F.spp = p.spp; F.n_launches = n_launches; F.n_chunks = p.n_planned; F.classify = p.classify; F.format = q.format;
    c->slot_turn = (c->slot_turn + 1) % ft_context::kSlots;
    if (defer) return FT_OK;                                       // ft_render_enqueue: the frame is retired by a later call
    if ((rc = retire_frame(c, F, stats)) != FT_OK) return rc;
    if (out && (rc = fetch_single(c, out, q.format)) != FT_OK) return rc;   // out == NULL: the frame stays in HBM
    if (stats) stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    return FT_OK;
}

int32_t render_single(ft_context* c, const RenderRequest& q, void* out, ft_stats* stats, bool defer) {
    if (!need_device(c)) return FT_ERR_NO_DEVICE;
    if (!c->committed) { c->err = "scene not committed (ft_scene_commit)"; return FT_ERR_STATE; }
    const auto wall0 = std::chrono::steady_clock::now();
    FT_HIP(c, hipSetDevice(c->device));
    FramePlan p;
    plan_pixels(c, q, p);
    if (stats) std::memset(stats, 0, sizeof *stats);
    if (p.n_pix_total == 0) return FT_OK;
    if (q.progressive && p.n_pix_total != c->prog.n_pix) { c->err = "progressive pass: the pixel list differs from the accumulation's"; return FT_ERR_STATE; }
    // The slot the frame takes is free before it is planned: the plan looks at what the slot's last classification left in it.
    if (c->slots[c->slot_turn].pending) { const int32_t rc = retire_frame(c, c->slots[c->slot_turn], nullptr); if (rc != FT_OK) return rc; }
    plan_chunks(c, q, defer, p);
    if (p.cap > 0x7FFFFFFFll) { c->err = "chunk too large"; return FT_ERR_INVALID; }
    if (p.classify && p.progressive && p.jobs.size() > 1 && p.pix_per_chunk % 64) { c->err = "progressive pass: too many samples per pass for whole-block windows"; return FT_ERR_UNSUPPORTED; }
    return queue_frame(c, q, p, out, stats, defer, wall0);
}

static void add_stats(ft_stats* t, const ft_stats& s) {
    t->rays_primary += s.rays_primary; t->rays_shadow += s.rays_shadow; t->rays_reflect += s.rays_reflect; t->rays_traced += s.rays_traced;
    t->rays_reference_equivalent += s.rays_reference_equivalent; t->hits_primary += s.hits_primary; t->csg_overflow += s.csg_overflow;
    t->kernel_ms = std::max(t->kernel_ms, s.kernel_ms); t->trace_kernel_ms = std::max(t->trace_kernel_ms, s.trace_kernel_ms);
    t->algorithmic_bytes += s.algorithmic_bytes; t->hits_total += s.hits_total; t->algorithmic_bytes_closest += s.algorithmic_bytes_closest;
    t->algorithmic_bytes_shade += s.algorithmic_bytes_shade; t->algorithmic_bytes_primary += s.algorithmic_bytes_primary; t->n_launches += s.n_launches; t->n_chunks += s.n_chunks;
    t->rays_tail += s.rays_tail; t->rays_primary_culled += s.rays_primary_culled; t->rays_shadow_primary += s.rays_shadow_primary; t->rays_reflect_primary += s.rays_reflect_primary;
}
// One host thread per device: share(d, device d, its stats) for every device of the context at once, device 0 on the calling thread, the
// others on their workers, each with zeroed stats of its own.  No device waits for another.  The first failure in device order is
// returned with that device's error text; otherwise `stats`, when given, receives the sum and the wall time since wall0.
int32_t on_every_device(ft_context* c, ft_stats* stats, std::chrono::steady_clock::time_point wall0,
                               const std::function<int32_t(size_t, ft_context*, ft_stats*)>& share) {
    const std::vector<ft_context*> devs = devices(c);
    std::vector<int32_t> rcs(devs.size(), FT_OK);
    std::vector<ft_stats> sts(devs.size());
    auto run = [&](size_t d) { std::memset(&sts[d], 0, sizeof(ft_stats)); rcs[d] = share(d, devs[d], &sts[d]); };
    for (size_t d = 1; d < devs.size(); ++d) c->workers[d - 1]->post([&run, d] { run(d); });
    run(0);
    for (size_t d = 1; d < devs.size(); ++d) c->workers[d - 1]->wait();
    for (size_t d = 0; d < devs.size(); ++d) if (rcs[d] != FT_OK) { if (d) c->err = devs[d]->err; return rcs[d]; }
    if (stats) {
        std::memset(stats, 0, sizeof *stats);
        for (auto& s : sts) add_stats(stats, s);
        stats->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    }
    return FT_OK;
}

static int32_t render_frame(ft_context* c, const RenderRequest& q, void* out, ft_stats* stats, bool defer) {
    const int32_t rc = check_request(c, q);
    if (rc != FT_OK) return rc;
    if (c->peers.empty() || c->host_only) return render_single(c, q, out, stats, defer);
    if (!need_committed(c)) return FT_ERR_STATE;
    const auto wall0 = std::chrono::steady_clock::now();
    const std::vector<std::vector<ft_rect>> share = band_shares(q, 1 + c->peers.size());
    // Each device queues its bands' frame on its own stream, waits for it and copies its bands straight into the caller's frame (whole
    // rows: one contiguous copy per band); the bands meet in `out`.
    return on_every_device(c, defer ? nullptr : stats, wall0, [&](size_t d, ft_context* D, ft_stats* sd) -> int32_t {
        if (share[d].empty()) { D->last_n_pix = 0; return FT_OK; }
        RenderRequest qd = q;
        qd.tiles = share[d].data(); qd.n_tiles = (int32_t)share[d].size();
        return render_single(D, qd, out, sd, defer);
    });
}

int32_t with_growing_hit_lists(ft_context* c, const std::function<int32_t()>& run) {
    // Frames still queued by ft_render_enqueue, and the temporal calls queued behind them (ft_temporal_enqueue), are retired first, so that
    // an overflow of one of THEM is reported as what it is (neither is run again) instead of being taken for this call's.
    if (!c->host_only) {
        for (ft_context* d : devices(c)) {
            if (!any_queued(d)) continue;
            if (hipSetDevice(d->device) != hipSuccess) { c->err = "hipSetDevice failed"; return FT_ERR_NO_DEVICE; }
            const int32_t prc = retire_queued(d);
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

} // namespace ftc
using namespace ftc;

extern "C" {

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

int32_t ft_get_kernel_times(ft_context* c, double ms[5], int32_t launches[5]) {
    if (!c || !ms || !launches) return FT_ERR_INVALID;
    for (int k = 0; k < kStages; ++k) { ms[k] = c->k_ms[k]; launches[k] = c->k_launches[k]; }
    for (ft_context* p : c->peers) for (int k = 0; k < kStages; ++k) { ms[k] = std::max(ms[k], p->k_ms[k]); launches[k] = std::max(launches[k], p->k_launches[k]); }   // the slowest device's
    return FT_OK;
}

} // extern "C"

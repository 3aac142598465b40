// ft_progressive.cpp — ft_progressive_*: sample accumulation over passes of the frame driver (ft_frame.cpp).
#include "ft_context.h"

// A progressive render is a run of blocking frames over one fixed request whose k_resolve goes on from each pixel's running sum
// (k_resolve_progressive): the sum of a pixel's samples in pass order, then sample order, is the sum one ft_render over the concatenated
// pattern forms, so the mean S / n is that frame bit for bit.  See functracer_hip.h.
namespace ftc {

RenderRequest progressive_request(const ft_context::Progressive& P) {
    return RenderRequest{&P.cam, P.res_h, P.res_v, 1, kNoJitter, P.max_depth, 0, P.tiles.data(), (int32_t)P.tiles.size(), 0, true};
}

// Ends the progressive accumulation of a context, on every device (its buffers are freed).
void progressive_close(ft_context* c) {
    if (!c->prog.open) return;
    for (ft_context* d : devices(c)) { if (!d->host_only) (void)hipSetDevice(d->device); d->prog.release(); }
}

} // namespace ftc
using namespace ftc;

extern "C" {

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
    if (!need_committed(c)) return FT_ERR_STATE;
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
    // As render_frame: every device traces its share and copies its bands of the means into `out`.  A hit-list overflow anywhere
    // re-commits and runs the pass again on every device, from the same side of the running sums.
    const int32_t rc = with_growing_hit_lists(c, [&] {
        return on_every_device(c, stats, wall0, [&](size_t, ft_context* D, ft_stats* sd) -> int32_t {
            if (D->prog.n_pix == 0) { D->last_n_pix = 0; return FT_OK; }
            RenderRequest q = progressive_request(D->prog);
            q.spp = spp; q.jitter_xy = jitter_xy; q.seed = seed; q.format = rgba8 ? 1 : 0;
            return render_single(D, q, out, sd, false);
        });
    });
    if (rc != FT_OK) return rc;
    c->prog.passes += 1; c->prog.samples += spp; c->prog.traced = 0;
    for (ft_context* D : devices(c)) if (D->prog.n_pix > 0) { D->prog.cur ^= 1; c->prog.traced += D->last_active_pix * spp; }
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

} // extern "C"

// ft_denoise.hip — the kernels of ft_denoise (include/functracer_hip.h): an edge-avoiding a-trous wavelet filter
// (Dammertz et al. 2010) over the FP64 frame in HBM, guided by the surfaces k_aov reports.  A translation unit of its own: nothing
// here is inlined into, or shares registers or LDS with, the tracing kernels of ft_kernels.hip.
//
// The kernels are bandwidth-shaped.  Guides and colours live in FRAME layout (row 0 = top), the guides as one plane per component, so
// the 64 lanes of a wavefront - 64 consecutive pixels of one row (the workgroup is a 64 x 4 pixel tile) - read one contiguous 512-byte
// run per plane and tap (1536 bytes of the interleaved colours), whatever the step 2^i is.  Every tap after the first of a pixel is a
// re-read of something a neighbouring lane, wave or workgroup also reads: those are served by the L2, the kernel stages nothing.
#include <hip/hip_runtime.h>

#include "ft_device.h"
#include "ft_filter.h"

namespace ftk {
namespace {

// One lane per entry of a window of the pixel list: k_aov's planes of the window (by position) become the pixel's guide record in
// frame layout, and u_0 = c / d.  The class plane was filled with kDenoiseOutside before the first window, so what no window writes
// is a pixel outside the tiles.
__global__ __launch_bounds__(kBlock) void k_denoise_scatter(DenoiseScatterArgs a) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.win.n) return;
    const uint32_t pos = a.win.first + i;                           // position in the pixel list
    const size_t id = a.win.pixel_ids[pos];                         // y * res_h + x
    const bool hit = a.win.leaf[i] >= 0;
    const size_t S = a.win.stride;
    double d[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        a.g.n[ch][id] = hit ? a.win.n_plane[ch * S + i] : 0.0;
        a.g.p[ch][id] = hit ? a.win.p_plane[ch * S + i] : 0.0;
        const double alb = a.win.colour[ch * S + i];
        d[ch] = (hit && a.demodulate) ? demodulation_divisor(alb, a.albedo_floor) : 1.0;
        a.g.d[ch][id] = d[ch];
        a.u0[3 * id + ch] = a.frame[3 * id + ch] / d[ch];
    }
    double V = 1.0;
    if (a.sum) {                                                    // the standard error of the mean exactly as ft_progressive_fetch reports it
        const uint32_t cnt = a.blk[pos >> 6] & ~kRetired;
        const double dn = (double)cnt;
        const size_t L = a.n_list;
        double acc = 0.0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            double se = 0.0;
            if (cnt >= 2u) {
                const double m = a.sum[ch * L + pos] / dn;
                const double mm = m * m;                            // a statement of its own: the host's subtraction is not fused either
                const double v0 = a.sq[ch * L + pos] / dn - mm;
                const double v = (v0 < 0.0 ? 0.0 : v0) * dn / (dn - 1.0);
                se = sqrt(v / dn);
            }
            const double r = se / d[ch];
            acc += r * r;
        }
        V = a.variance_floor + (1.0 / 3.0) * acc;
    }
    a.g.v[id] = V;
    a.g.cls[id] = hit ? kDenoiseHit : kDenoiseMiss;
}

// One a-trous iteration, one lane per frame pixel, a workgroup per 64 x 4 pixel tile: atrous_taps (ft_filter.h) over the guide records, no variance.
// LAST: the iteration multiplies d back and writes FP64 or, with out8, RGBA8 bytes.
template <bool LAST>
__global__ __launch_bounds__(kBlock) void k_denoise(DenoiseArgs a) {
    const int x = (int)(blockIdx.x * 64u + threadIdx.x), y = (int)(blockIdx.y * 4u + threadIdx.y);
    if (x >= a.res_h || y >= a.res_v) return;
    const size_t id = (size_t)y * (size_t)a.res_h + (size_t)x;
    const uint8_t kx = a.g.cls[id];
    if (kx == kDenoiseOutside) return;
    const double ux0 = a.u_in[3 * id], ux1 = a.u_in[3 * id + 1], ux2 = a.u_in[3 * id + 2];
    double o0 = ux0, o1 = ux1, o2 = ux2;
    if (finite3(ux0, ux1, ux2)) {                                   // a pixel with a non-finite channel is copied through
        const FrameTaps<DenoiseGuides> taps{a.g, a.g.cls, a.u_in, nullptr, a.res_h};
        const bool use_c = a.inv_sc2 > 0.0;
        const double kc = use_c ? a.inv_sc2 / a.g.v[id] : 0.0;
        const EdgeCentre centre = edge_centre(taps, id, kx == kDenoiseHit, a.inv_sn2, a.inv_sp2, use_c, kc, ux0, ux1, ux2);   // (a miss: the colour term alone)
        double ov = 0.0;                                            // (no variance rides along)
        atrous_taps<false>(taps, centre, kx, x, y, a.step, a.res_h, a.res_v, o0, o1, o2, ov);
    }
    if (LAST) {
        o0 *= a.g.d[0][id]; o1 *= a.g.d[1][id]; o2 *= a.g.d[2][id];
        if (a.out8) { store_rgba8(a.out8, id, o0, o1, o2); return; }
    }
    a.u_out[3 * id] = o0; a.u_out[3 * id + 1] = o1; a.u_out[3 * id + 2] = o2;
}

// Zero iterations with RGBA8 output: the frame's bytes, nothing filtered.
__global__ __launch_bounds__(kBlock) void k_denoise_quantise(const double* rgb, uint8_t* out8, uint32_t n_px) {
    const uint32_t id = blockIdx.x * kBlock + threadIdx.x;
    if (id < n_px) store_rgba8(out8, id, rgb[3 * (size_t)id], rgb[3 * (size_t)id + 1], rgb[3 * (size_t)id + 2]);
}

} // namespace

void launch_denoise_scatter(hipStream_t stream, const DenoiseScatterArgs& a) {
    if (a.win.n == 0) return;
    hipLaunchKernelGGL(k_denoise_scatter, dim3((a.win.n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a);
}

void launch_denoise(hipStream_t stream, const DenoiseArgs& a, bool last) {
    if (last) hipLaunchKernelGGL(k_denoise<true>, tile_grid(a.res_h, a.res_v), tile_block(), 0, stream, a);
    else hipLaunchKernelGGL(k_denoise<false>, tile_grid(a.res_h, a.res_v), tile_block(), 0, stream, a);
}

void launch_denoise_quantise(hipStream_t stream, const double* rgb, uint8_t* out8, uint32_t n_px) {
    hipLaunchKernelGGL(k_denoise_quantise, dim3((n_px + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, rgb, out8, n_px);
}

} // namespace ftk

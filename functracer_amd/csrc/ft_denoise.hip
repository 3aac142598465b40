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

namespace ftk {
namespace {

__device__ __forceinline__ bool finite3(double a, double b, double c) { return isfinite(a) && isfinite(b) && isfinite(c); }

// Image.write's toByte (Image.fs:36, Math.fs:12-16), as ft_quantise_rgba8: clamp to [0, 1] (a NaN passes the clamp), * 255, truncate.
__device__ __forceinline__ uint32_t to_byte(double x) {
    if (x > 1.0) x = 1.0; else if (x < 0.0) x = 0.0;
    x = x * 255.0;
    return (x != x) ? 0u : (uint32_t)x;
}
__device__ __forceinline__ void store_rgba8(uint8_t* out8, size_t id, double r, double g, double b) {
    reinterpret_cast<uint32_t*>(out8)[id] = to_byte(r) | (to_byte(g) << 8) | (to_byte(b) << 16) | 0xFF000000u;
}

// One lane per entry of a window of the pixel list: k_aov's planes of the window (by position) become the pixel's guide record in
// frame layout, and u_0 = c / d.  The class plane was filled with kDenoiseOutside before the first window, so what no window writes
// is a pixel outside the tiles.
__global__ __launch_bounds__(kBlock) void k_denoise_scatter(DenoiseScatterArgs a) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t pos = a.first + i;                               // position in the pixel list
    const size_t id = a.pixel_ids[pos];                             // y * res_h + x
    const bool hit = a.leaf[i] >= 0;
    const size_t S = a.stride;
    double d[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        a.g.n[ch][id] = hit ? a.n_plane[ch * S + i] : 0.0;
        a.g.p[ch][id] = hit ? a.p_plane[ch * S + i] : 0.0;
        const double alb = a.colour[ch * S + i];
        d[ch] = (hit && a.demodulate) ? (alb > a.albedo_floor ? alb : a.albedo_floor) : 1.0;   // max(a, floor); a NaN albedo gives the floor
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

// One a-trous iteration, one lane per frame pixel, a workgroup per 64 x 4 pixel tile.  Taps in the order dy = -2 .. 2 outer, dx = -2 .. 2
// inner; a tap takes part when it lies in the frame, has the centre's class (outside-the-tiles never matches), its colour is finite
// and its E is not NaN.  LAST: the iteration multiplies d back and writes FP64 or, with out8, RGBA8 bytes.
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
        const bool geo = kx == kDenoiseHit;                         // a miss has n = p = 0 on both sides: only the colour term acts
        const bool use_n = geo && a.inv_sn2 > 0.0, use_p = geo && a.inv_sp2 > 0.0, use_c = a.inv_sc2 > 0.0;
        double nx0 = 0.0, nx1 = 0.0, nx2 = 0.0, px0 = 0.0, px1 = 0.0, px2 = 0.0;
        if (use_n) { nx0 = a.g.n[0][id]; nx1 = a.g.n[1][id]; nx2 = a.g.n[2][id]; }
        if (use_p) { px0 = a.g.p[0][id]; px1 = a.g.p[1][id]; px2 = a.g.p[2][id]; }
        const double kc = use_c ? a.inv_sc2 / a.g.v[id] : 0.0;
        const double h[5] = {1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, sw = 0.0;
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
            const int qy = y + a.step * dy;
            if (qy < 0 || qy >= a.res_v) continue;
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const int qx = x + a.step * dx;
                if (qx < 0 || qx >= a.res_h) continue;
                const size_t q = (size_t)qy * (size_t)a.res_h + (size_t)qx;
                if (a.g.cls[q] != kx) continue;
                const double u0 = a.u_in[3 * q], u1 = a.u_in[3 * q + 1], u2 = a.u_in[3 * q + 2];
                if (!finite3(u0, u1, u2)) continue;
                double E = 0.0;
                if (use_n) { const double e0 = nx0 - a.g.n[0][q], e1 = nx1 - a.g.n[1][q], e2 = nx2 - a.g.n[2][q]; E += (e0 * e0 + e1 * e1 + e2 * e2) * a.inv_sn2; }
                if (use_p) { const double e0 = px0 - a.g.p[0][q], e1 = px1 - a.g.p[1][q], e2 = px2 - a.g.p[2][q]; E += (e0 * e0 + e1 * e1 + e2 * e2) * a.inv_sp2; }
                if (use_c) { const double e0 = ux0 - u0, e1 = ux1 - u1, e2 = ux2 - u2; E += (e0 * e0 + e1 * e1 + e2 * e2) * kc; }
                if (E != E) continue;
                const double w = (h[dx + 2] * h[dy + 2]) * exp(-E);
                s0 += w * u0; s1 += w * u1; s2 += w * u2; sw += w;
            }
        }
        o0 = s0 / sw; o1 = s1 / sw; o2 = s2 / sw;                   // the centre tap has w = 9 / 64: sw > 0
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
    if (a.n == 0) return;
    hipLaunchKernelGGL(k_denoise_scatter, dim3((a.n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a);
}

void launch_denoise(hipStream_t stream, const DenoiseArgs& a, bool last) {
    const dim3 grid((uint32_t)(a.res_h + 63) / 64u, (uint32_t)(a.res_v + 3) / 4u), block(64, 4);
    if (last) hipLaunchKernelGGL(k_denoise<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(k_denoise<false>, grid, block, 0, stream, a);
}

void launch_denoise_quantise(hipStream_t stream, const double* rgb, uint8_t* out8, uint32_t n_px) {
    hipLaunchKernelGGL(k_denoise_quantise, dim3((n_px + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, rgb, out8, n_px);
}

} // namespace ftk

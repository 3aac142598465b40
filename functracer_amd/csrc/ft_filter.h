// ft_filter.h — what the post-processing passes (ft_denoise.hip, ft_temporal.hip, ft_temporal_filter.hip) state
// once: the image writer's byte rule (write_pixel of ft_kernels.hip takes it too), the demodulation divisor, the edge-stopping distance,
// the 25-tap a-trous loop and the 64 x 4 tile grid.  For the .hip files only; all forceinline, as if written out in each kernel.
#ifndef FT_FILTER_H
#define FT_FILTER_H
#include <hip/hip_runtime.h>

#include "ft_device.h"

namespace ftk {

static __device__ __forceinline__ bool finite3(double a, double b, double c) { return isfinite(a) && isfinite(b) && isfinite(c); }
// Image.write's toByte (Image.fs:36; Math.fs:12-16), as ft_quantise_rgba8: clamp to [0, 1] (a NaN passes the clamp), * 255, truncate.
static __device__ __forceinline__ uint32_t to_byte(double x) {
    if (x > 1.0) x = 1.0; else if (x < 0.0) x = 0.0;
    x = x * 255.0;
    return (x != x) ? 0u : (uint32_t)x;
}
static __device__ __forceinline__ void store_rgba8(uint8_t* out8, size_t id, double r, double g, double b) {
    reinterpret_cast<uint32_t*>(out8)[id] = to_byte(r) | (to_byte(g) << 8) | (to_byte(b) << 16) | 0xFF000000u;   // R, G, B, A = 255 in memory order
}
// The demodulation divisor d = max(albedo, floor); a NaN albedo gives the floor.
static __device__ __forceinline__ double demodulation_divisor(double albedo, double floor) { return albedo > floor ? albedo : floor; }

// The frame-shaped kernels: one lane per pixel, a workgroup per 64 x 4 pixel tile of a w x h region.
static inline dim3 tile_block() { return dim3(64, 4); }
static inline dim3 tile_grid(int w, int h) { return dim3((uint32_t)(w + 63) / 64u, (uint32_t)(h + 3) / 4u); }

// Where a tap is read when nothing is staged: planes in frame layout, by pixel id; g (DenoiseGuides, TemporalSet) holds the n and p
// planes, the colours are interleaved.  A user fills in what it reads.  (Copies of the kernel's arguments, not a reference to them:
// through a reference the compiler recomputes a row's qy * res_h for every tap.)
template <class G> struct FrameTaps {
    G g; const uint8_t* classes; const double *u_in, *v_in; int res_h;
    __device__ __forceinline__ size_t at(int qx, int qy) const { return (size_t)qy * (size_t)res_h + (size_t)qx; }
    __device__ __forceinline__ uint8_t cls(size_t q) const { return classes[q]; }
    __device__ __forceinline__ double u(size_t q, int ch) const { return u_in[3 * q + ch]; }
    __device__ __forceinline__ double v(size_t q) const { return v_in[q]; }
    __device__ __forceinline__ double n(size_t q, int ch) const { return g.n[ch][q]; }
    __device__ __forceinline__ double p(size_t q, int ch) const { return g.p[ch][q]; }
};
// The centre of a footprint as the edge-stopping distance sees it: which terms are on, the centre's normal, point and colour (each
// read only where its term is on) and the three factors 1 / sigma_n^2, 1 / sigma_p^2 and the colour term's 1 / (sigma_c^2 V).
struct EdgeCentre { bool use_n, use_p, use_c; double n[3], p[3], u[3], inv_sn2, inv_sp2, kc; };
// Taps: n(q, ch) and p(q, ch) of the entry q.  `geo`: the centre is a hit (a miss has no geometric term).  Without use_c .. u2: no colour term.
template <class Taps> static __device__ __forceinline__ EdgeCentre edge_centre(const Taps& t, size_t c, bool geo, double inv_sn2, double inv_sp2, bool use_c = false, double kc = 0.0,
                                                                               double u0 = 0.0, double u1 = 0.0, double u2 = 0.0) {
    EdgeCentre e{geo && inv_sn2 > 0.0, geo && inv_sp2 > 0.0, use_c, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {u0, u1, u2}, inv_sn2, inv_sp2, kc};
    if (e.use_n) { e.n[0] = t.n(c, 0); e.n[1] = t.n(c, 1); e.n[2] = t.n(c, 2); }
    if (e.use_p) { e.p[0] = t.p(c, 0); e.p[1] = t.p(c, 1); e.p[2] = t.p(c, 2); }
    return e;
}
// E of the tap q with the colour (u0, u1, u2): |dn|^2 / sigma_n^2 + |dp|^2 / sigma_p^2 + |du|^2 / (sigma_c^2 V), the terms that are
// on, in this order.  A NaN E is the caller's to reject.
template <class Taps> static __device__ __forceinline__ double edge_distance(const EdgeCentre& c, const Taps& t, size_t q, double u0 = 0.0, double u1 = 0.0, double u2 = 0.0) {
    double E = 0.0;
    if (c.use_n) { const double e0 = c.n[0] - t.n(q, 0), e1 = c.n[1] - t.n(q, 1), e2 = c.n[2] - t.n(q, 2); E += (e0 * e0 + e1 * e1 + e2 * e2) * c.inv_sn2; }
    if (c.use_p) { const double e0 = c.p[0] - t.p(q, 0), e1 = c.p[1] - t.p(q, 1), e2 = c.p[2] - t.p(q, 2); E += (e0 * e0 + e1 * e1 + e2 * e2) * c.inv_sp2; }
    if (c.use_c) { const double e0 = c.u[0] - u0, e1 = c.u[1] - u1, e2 = c.u[2] - u2; E += (e0 * e0 + e1 * e1 + e2 * e2) * c.kc; }
    return E;
}

// The 25 taps of one a-trous iteration around the pixel (x, y) of class kx, `step` pixels apart, in the order dy = -2 .. 2 outer,
// dx = -2 .. 2 inner.  A tap takes part when it lies in the frame, has the centre's class (outside-the-tiles never matches), its colour
// (VAR: and its variance) is finite and its E is not NaN; its weight is w = h h exp(-E).  o = sum w u / sum w and, with VAR,
// ov = sum w^2 v / (sum w)^2.  Taps says where a tap is read: at(qx, qy) is its entry, cls, u, v, n, p what the entry holds.
template <bool VAR, class Taps> static __device__ __forceinline__ void atrous_taps(const Taps& t, const EdgeCentre& c, uint8_t kx, int x, int y, int step,
                                                                                   int res_h, int res_v, double& o0, double& o1, double& o2, double& ov) {
    const double h[5] = {1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, sw = 0.0, sv = 0.0;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int qy = y + step * dy;
        if (qy < 0 || qy >= res_v) continue;
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + step * dx;
            if (qx < 0 || qx >= res_h) continue;
            const size_t q = t.at(qx, qy);
            if (t.cls(q) != kx) continue;
            double u0 = t.u(q, 0), u1 = t.u(q, 1), u2 = t.u(q, 2), vq = 0.0;
            if constexpr (VAR) vq = t.v(q);
            if (!finite3(u0, u1, u2) || (VAR && !isfinite(vq))) continue;
            const double E = edge_distance(c, t, q, u0, u1, u2);
            if (E != E) continue;
            const double w = (h[dx + 2] * h[dy + 2]) * exp(-E);
            s0 += w * u0; s1 += w * u1; s2 += w * u2; sw += w;
            if (VAR) sv += (w * w) * vq;
        }
    }
    o0 = s0 / sw; o1 = s1 / sw; o2 = s2 / sw;                       // the centre tap has w = 9 / 64: sw > 0
    if (VAR) ov = sv / (sw * sw);
}

} // namespace ftk
#endif

// ft_temporal_filter.hip — the kernels of ft_temporal_filter (include/functracer_hip.h): a variance-guided, edge-avoiding
// a-trous filter (Dammertz et al. 2010 with the variance of Schied et al. 2017) over the history set ft_temporal_accumulate just wrote.
// A translation unit of its own, as ft_denoise.hip and ft_temporal.hip: nothing here is inlined into, or shares registers or LDS with,
// the tracing kernels of ft_kernels.hip.
//
// The set is read in place: M, Q, N for the colour and its variance once (k_tfilter_prepare), n, p and the class by every tap of every
// iteration, straight from the TemporalSet planes.  All planes are in FRAME layout, one plane per component, so the 64 lanes of a
// wavefront - 64 consecutive pixels of one row - read one contiguous 512-byte run per plane and tap, whatever the step is.  The
// iterations with steps 1 and 2 stage their tile and its halo in the LDS; from step 4 on the halo outgrows the tile and the re-reads
// among the 25 + 9 taps are left to the L2 (DESIGN.md 13 has the measurement of both ways at steps 1 and 2).
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

// One lane per entry of a window of the pixel list: d of the pixel, by pixel id.  The guide's colour belongs to the surface the set
// holds only where the two leaves agree (they do wherever the guide pass repeats the accumulate call's arguments).
__global__ __launch_bounds__(kBlock) void k_tfilter_scatter(TFilterScatterArgs a) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    const size_t id = a.pixel_ids[a.first + i];                     // y * res_h + x
    const int32_t leaf = a.set_leaf[id];
    const bool match = leaf >= 0 && a.leaf[i] == leaf;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double alb = a.colour[(size_t)ch * a.stride + i];
        a.d[ch][id] = match ? (alb > a.albedo_floor ? alb : a.albedo_floor) : 1.0;   // max(a, floor); a NaN albedo gives the floor
    }
}

// The per-channel standard error of the mean exactly as ft_temporal_fetch reports it, over d, squared and averaged: vt.
__device__ __forceinline__ double temporal_variance(const double (&M)[3], const double (&Q)[3], double N, const double (&d)[3]) {
    double acc = 0.0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        double se = 0.0;
        if (N >= 2.0) {
            const double mm = M[ch] * M[ch];                        // a statement of its own: the host's subtraction is not fused either
            const double v = Q[ch] - mm;
            se = sqrt((v > 0.0 ? v : 0.0) / N);
        }
        const double r = se / d[ch];
        acc += r * r;
    }
    return (1.0 / 3.0) * acc;
}

// One lane per pixel of a clipped rect, a workgroup per 64 x 4 pixels of it.  The 7 x 7 spatial estimate recomputes its taps' class and
// u_0 from the set (and d), never from what other lanes of this launch write, and only wavefronts that hold a short history enter it.
__global__ __launch_bounds__(kBlock) void k_tfilter_prepare(TFilterPrepareArgs a) {
    const int lx = (int)(blockIdx.x * 64u + threadIdx.x), ly = (int)(blockIdx.y * 4u + threadIdx.y);
    const bool active = lx < a.w && ly < a.h;
    const int x = a.x0 + lx, y = a.y0 + ly;
    const size_t id = active ? (size_t)y * (size_t)a.res_h + (size_t)x : 0;
    const bool demod = a.g.d[0] != nullptr;
    double M[3] = {0.0, 0.0, 0.0}, Q[3] = {0.0, 0.0, 0.0}, d[3] = {1.0, 1.0, 1.0}, u[3] = {0.0, 0.0, 0.0}, N = 0.0, vt = 0.0;
    bool hit = false;
    if (active) {
        hit = a.set.leaf[id] >= 0;
        N = a.set.len[id];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            M[ch] = a.set.m[ch][id]; Q[ch] = a.set.q[ch][id];
            if (demod) d[ch] = a.g.d[ch][id];
            u[ch] = M[ch] / d[ch];
        }
        vt = temporal_variance(M, Q, N, d);
    }
    double v0 = vt;
    const bool is_short = active && N < a.min_history;
    if (__any(is_short)) {                                          // the whole wavefront skips the 49 taps where every history is long enough
        if (is_short) {
            const bool use_n = hit && a.inv_sn2 > 0.0, use_p = hit && a.inv_sp2 > 0.0;
            double nx[3] = {0.0, 0.0, 0.0}, px[3] = {0.0, 0.0, 0.0};
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) { if (use_n) nx[ch] = a.set.n[ch][id]; if (use_p) px[ch] = a.set.p[ch][id]; }
            double sg = 0.0, s1[3] = {0.0, 0.0, 0.0}, s2[3] = {0.0, 0.0, 0.0};
            for (int dy = -3; dy <= 3; ++dy) {
                const int qy = y + dy;
                if (qy < 0 || qy >= a.res_v) continue;
                for (int dx = -3; dx <= 3; ++dx) {
                    const int qx = x + dx;
                    if (qx < 0 || qx >= a.res_h) continue;
                    const size_t q = (size_t)qy * (size_t)a.res_h + (size_t)qx;
                    if (a.g.cls[q] == kDenoiseOutside || (a.set.leaf[q] >= 0) != hit) continue;
                    double uq[3];
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) uq[ch] = a.set.m[ch][q] / (demod ? a.g.d[ch][q] : 1.0);
                    if (!finite3(uq[0], uq[1], uq[2])) continue;
                    double E = 0.0;
                    if (use_n) { const double e0 = nx[0] - a.set.n[0][q], e1 = nx[1] - a.set.n[1][q], e2 = nx[2] - a.set.n[2][q]; E += (e0 * e0 + e1 * e1 + e2 * e2) * a.inv_sn2; }
                    if (use_p) { const double e0 = px[0] - a.set.p[0][q], e1 = px[1] - a.set.p[1][q], e2 = px[2] - a.set.p[2][q]; E += (e0 * e0 + e1 * e1 + e2 * e2) * a.inv_sp2; }
                    const double g = exp(-E);
                    sg += g;
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) { s1[ch] += g * uq[ch]; s2[ch] += g * (uq[ch] * uq[ch]); }
                }
            }
            double acc = 0.0;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const double m1 = s1[ch] / sg, m2 = s2[ch] / sg;
                const double mm = m1 * m1;                          // unfused, as the definition says
                const double v = m2 - mm;
                acc += v > 0.0 ? v : 0.0;                           // (no tap at all: 0 / 0, and a NaN is not > 0)
            }
            const double vs = (1.0 / 3.0) * acc;
            if (vs > vt) v0 = vs;
        }
    }
    if (!active) return;
    a.g.cls[id] = hit ? kDenoiseHit : kDenoiseMiss;
    a.v0[id] = v0;
    if (a.raw) {                                                    // no iterations: M bit for bit
        a.u0[3 * id] = M[0]; a.u0[3 * id + 1] = M[1]; a.u0[3 * id + 2] = M[2];
        if (a.out8) store_rgba8(a.out8, id, M[0], M[1], M[2]);
    } else {
        a.u0[3 * id] = u[0]; a.u0[3 * id + 1] = u[1]; a.u0[3 * id + 2] = u[2];
    }
}

// One a-trous iteration, one lane per frame pixel, a workgroup per 64 x 4 pixel tile (k_denoise's shape).  First the 3 x 3 prefilter of
// the variance around the pixel (taps at distance 1 whatever the step), then the 25 taps in the order dy = -2 .. 2 outer, dx = -2 .. 2
// inner; a tap takes part when it lies in the frame, has the centre's class (outside-the-tiles never matches), its colour and variance
// are finite and its E is not NaN.  LAST: the iteration multiplies d back and writes FP64 and / or RGBA8 bytes.
// LDS: the tile and its halo of 2 * step pixels (class, u, v, and n, p where their term is on) are staged in the LDS as planes of
// (64 + 4 step) x (4 + 4 step) entries and every tap reads from there; what lies outside the frame is staged as class "outside".
extern __shared__ double tf_lds[];
template <bool LAST, bool LDS>
__global__ __launch_bounds__(kBlock) void k_tfilter(TFilterArgs a) {
    const int tx0 = (int)(blockIdx.x * 64u), ty0 = (int)(blockIdx.y * 4u);
    const int x = tx0 + (int)threadIdx.x, y = ty0 + (int)threadIdx.y;
    const int halo = 2 * a.step, TW = 64 + 2 * halo, NT = TW * (4 + 2 * halo);
    double* const Lu = tf_lds; double* const Lv = Lu + 3 * NT; double* const Ln = Lv + NT; double* const Lp = Ln + 3 * NT;
    uint8_t* const Lc = reinterpret_cast<uint8_t*>(Lp + 3 * NT);
    if (LDS) {
        const bool st_n = a.inv_sn2 > 0.0, st_p = a.inv_sp2 > 0.0;
        for (int t = (int)(threadIdx.y * 64u + threadIdx.x); t < NT; t += kBlock) {
            const int ty = t / TW, tx = t - ty * TW;
            const int gx = tx0 - halo + tx, gy = ty0 - halo + ty;
            uint8_t k = kDenoiseOutside;
            if (gx >= 0 && gx < a.res_h && gy >= 0 && gy < a.res_v) {
                const size_t q = (size_t)gy * (size_t)a.res_h + (size_t)gx;
                k = a.g.cls[q];
                if (k != kDenoiseOutside) {
                    Lu[t] = a.u_in[3 * q]; Lu[NT + t] = a.u_in[3 * q + 1]; Lu[2 * NT + t] = a.u_in[3 * q + 2]; Lv[t] = a.v_in[q];
                    if (k == kDenoiseHit) {
                        if (st_n) { Ln[t] = a.set.n[0][q]; Ln[NT + t] = a.set.n[1][q]; Ln[2 * NT + t] = a.set.n[2][q]; }
                        if (st_p) { Lp[t] = a.set.p[0][q]; Lp[NT + t] = a.set.p[1][q]; Lp[2 * NT + t] = a.set.p[2][q]; }
                    }
                }
            }
            Lc[t] = k;
        }
        __syncthreads();
    }
    if (x >= a.res_h || y >= a.res_v) return;
    const size_t id = (size_t)y * (size_t)a.res_h + (size_t)x;
    // where a tap is read: its index in the staged planes (stride NT between components) or in the frame (components interleaved for u)
    auto at = [&](int qx, int qy) -> size_t { return LDS ? (size_t)((qy - ty0 + halo) * TW + (qx - tx0 + halo)) : (size_t)qy * (size_t)a.res_h + (size_t)qx; };
    auto cls_at = [&](size_t q) -> uint8_t { return LDS ? Lc[q] : a.g.cls[q]; };
    auto v_at = [&](size_t q) -> double { return LDS ? Lv[q] : a.v_in[q]; };
    auto u_at = [&](size_t q, int ch) -> double { return LDS ? Lu[ch * NT + q] : a.u_in[3 * q + ch]; };
    auto n_at = [&](size_t q, int ch) -> double { return LDS ? Ln[ch * NT + q] : a.set.n[ch][q]; };
    auto p_at = [&](size_t q, int ch) -> double { return LDS ? Lp[ch * NT + q] : a.set.p[ch][q]; };
    const size_t c = at(x, y);
    const uint8_t kx = cls_at(c);
    if (kx == kDenoiseOutside) return;
    const double ux0 = u_at(c, 0), ux1 = u_at(c, 1), ux2 = u_at(c, 2), vx = v_at(c);
    double o0 = ux0, o1 = ux1, o2 = ux2, ov = vx;
    if (finite3(ux0, ux1, ux2) && isfinite(vx)) {                   // a pixel with a non-finite colour or variance is copied through
        const double h3[3] = {1.0 / 4.0, 1.0 / 2.0, 1.0 / 4.0};
        double gs = 0.0, gw = 0.0;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int qy = y + dy;
            if (qy < 0 || qy >= a.res_v) continue;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int qx = x + dx;
                if (qx < 0 || qx >= a.res_h) continue;
                const size_t q = at(qx, qy);
                if (cls_at(q) != kx) continue;
                const double vq = v_at(q);
                if (!isfinite(vq)) continue;
                const double w = h3[dx + 1] * h3[dy + 1];
                gs += w * vq; gw += w;
            }
        }
        const double gv = gs / gw;                                  // the centre takes part: gw >= 1 / 4
        const bool geo = kx == kDenoiseHit;                         // a miss has no geometric term
        const bool use_n = geo && a.inv_sn2 > 0.0, use_p = geo && a.inv_sp2 > 0.0, use_c = a.inv_sc2 > 0.0;
        double nx0 = 0.0, nx1 = 0.0, nx2 = 0.0, px0 = 0.0, px1 = 0.0, px2 = 0.0;
        if (use_n) { nx0 = n_at(c, 0); nx1 = n_at(c, 1); nx2 = n_at(c, 2); }
        if (use_p) { px0 = p_at(c, 0); px1 = p_at(c, 1); px2 = p_at(c, 2); }
        const double kc = use_c ? a.inv_sc2 / (gv + a.variance_floor) : 0.0;
        const double h[5] = {1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0};
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, sw = 0.0, sv = 0.0;
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
            const int qy = y + a.step * dy;
            if (qy < 0 || qy >= a.res_v) continue;
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const int qx = x + a.step * dx;
                if (qx < 0 || qx >= a.res_h) continue;
                const size_t q = at(qx, qy);
                if (cls_at(q) != kx) continue;
                const double u0 = u_at(q, 0), u1 = u_at(q, 1), u2 = u_at(q, 2), vq = v_at(q);
                if (!finite3(u0, u1, u2) || !isfinite(vq)) continue;
                double E = 0.0;
                if (use_n) { const double e0 = nx0 - n_at(q, 0), e1 = nx1 - n_at(q, 1), e2 = nx2 - n_at(q, 2); E += (e0 * e0 + e1 * e1 + e2 * e2) * a.inv_sn2; }
                if (use_p) { const double e0 = px0 - p_at(q, 0), e1 = px1 - p_at(q, 1), e2 = px2 - p_at(q, 2); E += (e0 * e0 + e1 * e1 + e2 * e2) * a.inv_sp2; }
                if (use_c) { const double e0 = ux0 - u0, e1 = ux1 - u1, e2 = ux2 - u2; E += (e0 * e0 + e1 * e1 + e2 * e2) * kc; }
                if (E != E) continue;
                const double w = (h[dx + 2] * h[dy + 2]) * exp(-E);
                s0 += w * u0; s1 += w * u1; s2 += w * u2; sw += w; sv += (w * w) * vq;
            }
        }
        o0 = s0 / sw; o1 = s1 / sw; o2 = s2 / sw; ov = sv / (sw * sw);   // the centre tap has w = 9 / 64: sw > 0
    }
    a.v_out[id] = ov;
    if (LAST) {
        if (a.g.d[0]) { o0 *= a.g.d[0][id]; o1 *= a.g.d[1][id]; o2 *= a.g.d[2][id]; }
        if (a.out8) store_rgba8(a.out8, id, o0, o1, o2);
        if (!a.u_out) return;
    }
    a.u_out[3 * id] = o0; a.u_out[3 * id + 1] = o1; a.u_out[3 * id + 2] = o2;
}

} // namespace

void launch_tfilter_scatter(hipStream_t stream, const TFilterScatterArgs& a) {
    if (a.n == 0) return;
    hipLaunchKernelGGL(k_tfilter_scatter, dim3((a.n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a);
}

void launch_tfilter_prepare(hipStream_t stream, const TFilterPrepareArgs& a) {
    if (a.w <= 0 || a.h <= 0) return;
    hipLaunchKernelGGL(k_tfilter_prepare, dim3((uint32_t)(a.w + 63) / 64u, (uint32_t)(a.h + 3) / 4u), dim3(64, 4), 0, stream, a);
}

template <bool LAST, bool LDS> static void launch_tfilter_as(hipStream_t stream, const TFilterArgs& a) {
    const dim3 grid((uint32_t)(a.res_h + 63) / 64u, (uint32_t)(a.res_v + 3) / 4u), block(64, 4);
    size_t lds = 0;
    if (LDS) {                                                      // ten planes of doubles and the classes; beyond 64 KB a kernel has to ask
        const size_t nt = (size_t)(64 + 4 * a.step) * (size_t)(4 + 4 * a.step);
        lds = (nt * 81 + 7) & ~(size_t)7;                           // 44 064 bytes at step 1, 69 984 at step 2
        if (lds > 65536) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_tfilter<LAST, LDS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    }
    hipLaunchKernelGGL((k_tfilter<LAST, LDS>), grid, block, lds, stream, a);
}

void launch_tfilter(hipStream_t stream, const TFilterArgs& a, bool last) {
    const bool lds = a.step <= 2;                                   // measured: 0.19 against 0.50 ms at step 1, 0.30 against 0.52 ms at step 2 (1080p)
    if (last) { if (lds) launch_tfilter_as<true, true>(stream, a); else launch_tfilter_as<true, false>(stream, a); }
    else { if (lds) launch_tfilter_as<false, true>(stream, a); else launch_tfilter_as<false, false>(stream, a); }
}

} // namespace ftk

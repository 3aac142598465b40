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
#include "ft_filter.h"

namespace ftk {
namespace {

// One lane per entry of a window of the pixel list: d of the pixel, by pixel id.  The guide's colour belongs to the surface the set
// holds only where the two leaves agree (they do wherever the guide pass repeats the accumulate call's arguments).
__global__ __launch_bounds__(kBlock) void k_tfilter_scatter(TFilterScatterArgs a) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.win.n) return;
    const size_t id = a.win.pixel_ids[a.win.first + i];             // y * res_h + x
    const int32_t leaf = a.set_leaf[id];
    const bool match = leaf >= 0 && a.win.leaf[i] == leaf;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double alb = a.win.colour[(size_t)ch * a.win.stride + i];
        a.d[ch][id] = match ? demodulation_divisor(alb, a.albedo_floor) : 1.0;
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
            const FrameTaps<TemporalSet> taps{a.set};   // (n and p alone are read)
            const EdgeCentre centre = edge_centre(taps, id, hit, a.inv_sn2, a.inv_sp2);   // no colour term
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
                    const double g = exp(-edge_distance(centre, taps, q));
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

// Where k_tfilter's taps are read.  An entry is an index in the staged planes (stride NT between components) or in the frame
// (components interleaved for u; n and p from the set's planes).
template <bool LDS> struct TFilterTaps {
    FrameTaps<TemporalSet> f;
    const double *Lu, *Lv, *Ln, *Lp; const uint8_t* Lc; int tx0, ty0, halo, TW, NT;
    __device__ __forceinline__ size_t at(int qx, int qy) const { return LDS ? (size_t)((qy - ty0 + halo) * TW + (qx - tx0 + halo)) : f.at(qx, qy); }
    __device__ __forceinline__ uint8_t cls(size_t q) const { return LDS ? Lc[q] : f.cls(q); }
    __device__ __forceinline__ double v(size_t q) const { return LDS ? Lv[q] : f.v(q); }
    __device__ __forceinline__ double u(size_t q, int ch) const { return LDS ? Lu[ch * NT + q] : f.u(q, ch); }
    __device__ __forceinline__ double n(size_t q, int ch) const { return LDS ? Ln[ch * NT + q] : f.n(q, ch); }
    __device__ __forceinline__ double p(size_t q, int ch) const { return LDS ? Lp[ch * NT + q] : f.p(q, ch); }
};

// One a-trous iteration, one lane per frame pixel, a workgroup per 64 x 4 pixel tile.  First the 3 x 3 prefilter of the variance around
// the pixel (taps at distance 1 whatever the step), then atrous_taps (ft_filter.h) with the variance riding along.  LAST: the iteration
// multiplies d back and writes FP64 and / or RGBA8 bytes.
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
    const TFilterTaps<LDS> taps{{a.set, a.g.cls, a.u_in, a.v_in, a.res_h}, Lu, Lv, Ln, Lp, Lc, tx0, ty0, halo, TW, NT};
    const size_t c = taps.at(x, y);
    const uint8_t kx = taps.cls(c);
    if (kx == kDenoiseOutside) return;
    const double ux0 = taps.u(c, 0), ux1 = taps.u(c, 1), ux2 = taps.u(c, 2), vx = taps.v(c);
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
                const size_t q = taps.at(qx, qy);
                if (taps.cls(q) != kx) continue;
                const double vq = taps.v(q);
                if (!isfinite(vq)) continue;
                const double w = h3[dx + 1] * h3[dy + 1];
                gs += w * vq; gw += w;
            }
        }
        const double gv = gs / gw;                                  // the centre takes part: gw >= 1 / 4
        const bool use_c = a.inv_sc2 > 0.0;
        const double kc = use_c ? a.inv_sc2 / (gv + a.variance_floor) : 0.0;
        const EdgeCentre centre = edge_centre(taps, c, kx == kDenoiseHit, a.inv_sn2, a.inv_sp2, use_c, kc, ux0, ux1, ux2);
        atrous_taps<true>(taps, centre, kx, x, y, a.step, a.res_h, a.res_v, o0, o1, o2, ov);
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
    if (a.win.n == 0) return;
    hipLaunchKernelGGL(k_tfilter_scatter, dim3((a.win.n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, a);
}

void launch_tfilter_prepare(hipStream_t stream, const TFilterPrepareArgs& a) {
    if (a.w <= 0 || a.h <= 0) return;
    hipLaunchKernelGGL(k_tfilter_prepare, tile_grid(a.w, a.h), tile_block(), 0, stream, a);
}

template <bool LAST, bool LDS> static void launch_tfilter_as(hipStream_t stream, const TFilterArgs& a) {
    size_t lds = 0;
    if (LDS) {                                                      // ten planes of doubles and the classes; beyond 64 KB a kernel has to ask
        const size_t nt = (size_t)(64 + 4 * a.step) * (size_t)(4 + 4 * a.step);
        lds = (nt * 81 + 7) & ~(size_t)7;                           // 44 064 bytes at step 1, 69 984 at step 2
        if (lds > 65536) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&k_tfilter<LAST, LDS>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    }
    hipLaunchKernelGGL((k_tfilter<LAST, LDS>), tile_grid(a.res_h, a.res_v), tile_block(), lds, stream, a);
}

void launch_tfilter(hipStream_t stream, const TFilterArgs& a, bool last) {
    const bool lds = a.step <= 2;                                   // measured: 0.19 against 0.50 ms at step 1, 0.30 against 0.52 ms at step 2 (1080p)
    if (last) { if (lds) launch_tfilter_as<true, true>(stream, a); else launch_tfilter_as<true, false>(stream, a); }
    else { if (lds) launch_tfilter_as<false, true>(stream, a); else launch_tfilter_as<false, false>(stream, a); }
}

} // namespace ftk

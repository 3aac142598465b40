// ft_temporal.hip — the kernel of ft_temporal_accumulate (include/functracer_hip.h): the FP64 frame in HBM blended with
// the history of the surface point each pixel shows, fetched where that point lay in the previous call's image.  A translation unit of
// its own, as ft_denoise.hip: nothing here is inlined into, or shares registers or LDS with, the tracing kernels of ft_kernels.hip.
//
// One lane per entry of a window of the pixel list, queued behind the window's k_aov.  The list runs in 8x8 blocks (Z order inside a
// block), so a wavefront holds one block: what it reads by pixel id and what it writes are 8 runs of 64 bytes per plane (192 of the
// interleaved colours), and its 4 x 64 taps fall into a region of about 9x9 pixels of the previous set, 8-byte planes again: the four
// taps of a lane and those of its neighbours are the same cache lines, served by the L2; the kernel stages nothing.  A tap is tested
// in the order of what it costs: leaf and N (12 bytes), n (24), p (24), and only one that takes part reads M and Q (48).
//
// k_temporal<true> runs when the scene's pose differs from the one the history was written in (ft_scene_commit_moved): a hit
// lane whose leaf moved takes its point and normal back to that pose through the leaf's motion record (kTemporalMotionDoubles) before
// the projection and the tap tests; every other lane, and k_temporal<false>, runs the statements below on p and n themselves.  The
// lanes of a wavefront mostly share a leaf, so the record's 176 bytes are one or two cache lines read by every lane at the same address.
//
// k_temporal<MOVING, true> runs when "temporal_follow_deformed" is set and a mesh was snapshotted before its refit (ft_scene_commit_deformed,
// DESIGN.md 16.2): a hit lane whose triangle changed solves for its barycentric coordinates in the live record and takes the same
// coordinates in the snapshot's record back through H.  It reads its leaf's TemporalDeformLeaf (280 bytes at one address for the lanes
// that share the leaf) and two records of 72 bytes; the lanes of an 8x8 block lie on a few neighbouring triangles, so those are a
// few cache lines per wavefront, read once each: staging them in LDS would add a barrier and save no fetch.  The leaf index and the
// triangle index come from planes and are range-checked before they address anything.
//
// k_temporal<.., .., true> runs while ft_temporal_set_clamp is on: behind the division by W a lane reads the six
// doubles of its pixel's colour box by pixel id - 8 runs of 64 bytes per plane, as everything else it reads by pixel id - and moves the
// fetched mean into it.  The boxes come from k_temporal_box, once per call and clipped rect before the first window: 64 x 4 pixels per
// workgroup, the frame's colours and a halo staged in the LDS (at most 70 x 10 pixels x 25 bytes).  The instantiations without CLAMP
// are, instruction for instruction, what they were before the clamp existed (the new arguments lie behind the old ones).
#include <hip/hip_runtime.h>

#include "ft_device.h"
#include "ft_filter.h"

namespace ftk {
namespace {

// Clause 3a's two per-channel steps.  The products are statements of their own, as the definition has them.
__device__ __forceinline__ double clamp_to(double m, double lo, double hi) { return m < lo ? lo : (m > hi ? hi : m); }
__device__ __forceinline__ double moved_square(double q, double m, double k) {
    const double mm = m * m;
    const double vh = q - mm;
    const double kk = k * k;
    return kk + (vh > 0.0 ? vh : 0.0);
}

template <bool MOVING, bool DEFORMING = false, bool CLAMP = false> __global__ __launch_bounds__(kBlock) void k_temporal(TemporalArgs a) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.win.n) return;
    const size_t id = a.win.pixel_ids[a.win.first + i];             // y * res_h + x
    const size_t S = a.win.stride;
    const int32_t leaf = a.win.leaf[i];
    const bool hit = leaf >= 0;
    const double c0 = a.frame[3 * id], c1 = a.frame[3 * id + 1], c2 = a.frame[3 * id + 2];
    double p0 = 0.0, p1 = 0.0, p2 = 0.0, n0 = 0.0, n1 = 0.0, n2 = 0.0;
    if (hit) {
        p0 = a.win.p_plane[i]; p1 = a.win.p_plane[S + i]; p2 = a.win.p_plane[2 * S + i];
        n0 = a.win.n_plane[i]; n1 = a.win.n_plane[S + i]; n2 = a.win.n_plane[2 * S + i];
    }
    // the point and the normal the history is asked about: p and n, or where they were in the pose the history was written in
    double r0 = p0, r1 = p1, r2 = p2, u0 = n0, u1 = n1, u2 = n2;
    bool followed = false;                                          // through the snapshot: the way back already ends in the history's pose
    if (DEFORMING && hit && a.has_prev && (uint32_t)leaf < a.n_leaves) {
        const TemporalDeformLeaf* L = a.deform + (size_t)leaf;
        const uint32_t tau = (uint32_t)a.win.triangle[i], n_m = L->n;   // n_m = 0: the leaf's mesh holds no snapshot
        if (tau < n_m) {
            const double* live = a.tris + 9ull * ((size_t)L->first_live + tau);
            const double* old = a.snap + 9ull * ((size_t)L->snap_first + tau);
            double T[9], O[9];
            bool same = true;
#pragma unroll
            for (int k = 0; k < 9; ++k) { T[k] = live[k]; O[k] = old[k]; same = same && __double_as_longlong(T[k]) == __double_as_longlong(O[k]); }
            if (!same) {
                const double* Wm = L->W;
                const double q0 = Wm[0] * p0 + Wm[1] * p1 + Wm[2] * p2 + Wm[3];     // the hit point in model space
                const double q1 = Wm[4] * p0 + Wm[5] * p1 + Wm[6] * p2 + Wm[7];
                const double q2 = Wm[8] * p0 + Wm[9] * p1 + Wm[10] * p2 + Wm[11];
                const double d0 = q0 - T[0], d1 = q1 - T[1], d2 = q2 - T[2];
                const double d11 = T[3] * T[3] + T[4] * T[4] + T[5] * T[5], d12 = T[3] * T[6] + T[4] * T[7] + T[5] * T[8];
                const double d22 = T[6] * T[6] + T[7] * T[7] + T[8] * T[8];
                const double h1 = d0 * T[3] + d1 * T[4] + d2 * T[5], h2 = d0 * T[6] + d1 * T[7] + d2 * T[8];
                const double det = d11 * d22 - d12 * d12;
                if (det > 0.0) {                                    // (a collapsed triangle, or a NaN, keeps the existing path)
                    const double beta = (d22 * h1 - d12 * h2) / det, gamma = (d11 * h2 - d12 * h1) / det;
                    if (isfinite(beta) && isfinite(gamma)) {
                        followed = true;
                        const double w0 = O[0] + beta * O[3] + gamma * O[6], w1 = O[1] + beta * O[4] + gamma * O[7], w2 = O[2] + beta * O[5] + gamma * O[8];
                        const double* Hm = L->H;
                        r0 = Hm[0] * w0 + Hm[1] * w1 + Hm[2] * w2 + Hm[3];
                        r1 = Hm[4] * w0 + Hm[5] * w1 + Hm[6] * w2 + Hm[7];
                        r2 = Hm[8] * w0 + Hm[9] * w1 + Hm[10] * w2 + Hm[11];
                        const double g0 = T[4] * T[8] - T[5] * T[7], g1 = T[5] * T[6] - T[3] * T[8], g2 = T[3] * T[7] - T[4] * T[6];       // e1 x e2
                        const double f0 = O[4] * O[8] - O[5] * O[7], f1 = O[5] * O[6] - O[3] * O[8], f2 = O[3] * O[7] - O[4] * O[6];
                        const double c0n = Wm[0] * g0 + Wm[4] * g1 + Wm[8] * g2, c1n = Wm[1] * g0 + Wm[5] * g1 + Wm[9] * g2, c2n = Wm[2] * g0 + Wm[6] * g1 + Wm[10] * g2;
                        const double side = (n0 * c0n + n1 * c1n + n2 * c2n < 0.0) ? -1.0 : 1.0;   // the side of the triangle the shaders' normal is on
                        const double* Wh = L->Wh;
                        const double t0 = Wh[0] * f0 + Wh[3] * f1 + Wh[6] * f2, t1 = Wh[1] * f0 + Wh[4] * f1 + Wh[7] * f2, t2 = Wh[2] * f0 + Wh[5] * f1 + Wh[8] * f2;
                        const double s = 1.0 / sqrt(t0 * t0 + t1 * t1 + t2 * t2);   // (a non-finite result fails every tap's normal test)
                        u0 = side * t0 * s; u1 = side * t1 * s; u2 = side * t2 * s;
                    }
                }
            }
        }
    }
    if (MOVING && !(DEFORMING && (followed || !a.motion)) && hit && a.has_prev && (uint32_t)leaf < a.n_leaves) {
        const double* rec = a.motion + (size_t)leaf * kTemporalMotionDoubles;
        if (rec[21] != 0.0) {
            r0 = rec[0] * p0 + rec[1] * p1 + rec[2] * p2 + rec[3];      // D (p, 1), rows left to right
            r1 = rec[4] * p0 + rec[5] * p1 + rec[6] * p2 + rec[7];
            r2 = rec[8] * p0 + rec[9] * p1 + rec[10] * p2 + rec[11];
            const double t0 = rec[12] * n0 + rec[15] * n1 + rec[18] * n2;   // A^T n
            const double t1 = rec[13] * n0 + rec[16] * n1 + rec[19] * n2;
            const double t2 = rec[14] * n0 + rec[17] * n1 + rec[20] * n2;
            const double s = 1.0 / sqrt(t0 * t0 + t1 * t1 + t2 * t2);       // (a non-finite result fails every tap's normal test)
            u0 = t0 * s; u1 = t1 * s; u2 = t2 * s;
        }
    }
    double W = 0.0, m0 = 0.0, m1 = 0.0, m2 = 0.0, q0 = 0.0, q1 = 0.0, q2 = 0.0, len = 0.0;
    if (hit && a.has_prev) {
        const double v0 = r0 - a.o[0], v1 = r1 - a.o[1], v2 = r2 - a.o[2];
        const double zc = v0 * a.k[0] + v1 * a.k[1] + v2 * a.k[2];
        if (zc > 0.0) {                                             // the inverse of rayThroughPixel (Image.fs:83-89) at jitter 0
            const double fx = ((v0 * a.i[0] + v1 * a.i[1] + v2 * a.i[2]) / zc - a.tlx) / a.pw;
            const double fy = (a.tly - (v0 * a.j[0] + v1 * a.j[1] + v2 * a.j[2]) / zc) / a.ph;
            // outside [-1, res): none of the four taps lies in the frame (a NaN fails every comparison)
            if (fx >= -1.0 && fx < (double)a.res_h && fy >= -1.0 && fy < (double)a.res_v) {
                const double fx0 = floor(fx), fy0 = floor(fy);
                const int x0 = (int)fx0, y0 = (int)fy0;
                const double wx = fx - fx0, wy = fy - fy0;
                const double tol = a.tol_scale * zc;
                const double tol2 = tol * tol;
#pragma unroll
                for (int dy = 0; dy < 2; ++dy) {
                    const int qy = y0 + dy;
                    if (qy < 0 || qy >= a.res_v) continue;
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx) {
                        const int qx = x0 + dx;
                        if (qx < 0 || qx >= a.res_h) continue;
                        const size_t q = (size_t)qy * (size_t)a.res_h + (size_t)qx;
                        const double lq = a.prev.len[q];
                        if (!(lq >= 1.0) || a.prev.leaf[q] != leaf) continue;
                        if (!(u0 * a.prev.n[0][q] + u1 * a.prev.n[1][q] + u2 * a.prev.n[2][q] >= a.min_normal_dot)) continue;
                        const double e0 = r0 - a.prev.p[0][q], e1 = r1 - a.prev.p[1][q], e2 = r2 - a.prev.p[2][q];
                        if (!(e0 * e0 + e1 * e1 + e2 * e2 <= tol2)) continue;
                        const double hm0 = a.prev.m[0][q], hm1 = a.prev.m[1][q], hm2 = a.prev.m[2][q];
                        const double hq0 = a.prev.q[0][q], hq1 = a.prev.q[1][q], hq2 = a.prev.q[2][q];
                        if (!finite3(hm0, hm1, hm2) || !finite3(hq0, hq1, hq2)) continue;
                        const double b = (dx ? wx : 1.0 - wx) * (dy ? wy : 1.0 - wy);
                        W += b; len += b * lq;
                        m0 += b * hm0; m1 += b * hm1; m2 += b * hm2;
                        q0 += b * hq0; q1 += b * hq1; q2 += b * hq2;
                    }
                }
            }
        }
    }
    const double s0 = c0 * c0, s1 = c1 * c1, s2 = c2 * c2;          // statements of their own: not fused into the differences below
    const bool finite = finite3(c0, c1, c2);
    const bool history = finite && W >= kTemporalMinWeight;
    double N = finite ? 1.0 : 0.0, M0 = c0, M1 = c1, M2 = c2, Q0 = s0, Q1 = s1, Q2 = s2;
    bool clamped = false;
    if (history) {
        m0 /= W; m1 /= W; m2 /= W; q0 /= W; q1 /= W; q2 /= W;
        double nh = len / W;
        if (CLAMP) {                                                // clause 3a: the fetched mean into the box of the frame's neighbourhood
            const double k0 = clamp_to(m0, a.box.lo[0][id], a.box.hi[0][id]), k1 = clamp_to(m1, a.box.lo[1][id], a.box.hi[1][id]);
            const double k2 = clamp_to(m2, a.box.lo[2][id], a.box.hi[2][id]);
            clamped = k0 != m0 || k1 != m1 || k2 != m2;
            if (clamped) {                                          // the history keeps its variance around the moved mean, and is shortened
                q0 = moved_square(q0, m0, k0); q1 = moved_square(q1, m1, k1); q2 = moved_square(q2, m2, k2);
                m0 = k0; m1 = k1; m2 = k2;
                if (nh > a.clamped_history) nh = a.clamped_history;
            }
        }
        N = nh + 1.0;
        if (N > a.max_history) N = a.max_history;
        M0 = m0 + (c0 - m0) / N; M1 = m1 + (c1 - m1) / N; M2 = m2 + (c2 - m2) / N;
        Q0 = q0 + (s0 - q0) / N; Q1 = q1 + (s1 - q1) / N; Q2 = q2 + (s2 - q2) / N;
    }
    a.cur.m[0][id] = M0; a.cur.m[1][id] = M1; a.cur.m[2][id] = M2;
    a.cur.q[0][id] = Q0; a.cur.q[1][id] = Q1; a.cur.q[2][id] = Q2;
    a.cur.len[id] = N;
    a.cur.p[0][id] = p0; a.cur.p[1][id] = p1; a.cur.p[2][id] = p2;
    a.cur.n[0][id] = n0; a.cur.n[1][id] = n1; a.cur.n[2][id] = n2;
    a.cur.leaf[id] = leaf;
    if (a.out_rgb) { a.out_rgb[3 * id] = M0; a.out_rgb[3 * id + 1] = M1; a.out_rgb[3 * id + 2] = M2; }
    if (a.out8) store_rgba8(a.out8, id, M0, M1, M2);
    // the call's counts: one atomic per wavefront and count (the lanes past the window's end left above; lane 0 never does alone)
    const unsigned long long with_history = __ballot(history), at_max = __ballot(finite && N == a.max_history);
    const unsigned long long moved = CLAMP ? __ballot(clamped) : 0ull;
    if ((threadIdx.x & 63u) == 0u) {
        if (with_history) atomicAdd(&a.counters[0], (unsigned long long)__popcll(with_history));
        if (at_max) atomicAdd(&a.counters[1], (unsigned long long)__popcll(at_max));
        if (CLAMP && moved) atomicAdd(&a.counters[2], (unsigned long long)__popcll(moved));
    }
}

// The box of a pixel's neighbourhood in the frame (clause 3a).  One lane per pixel of a clipped rect, a workgroup per 64 x 4 pixels of
// it, as k_tfilter_prepare; the tile and its halo of R pixels are staged in the LDS - the colours interleaved as the frame holds them,
// and a byte per staged pixel: it takes part iff it lies in the frame, is in T (the mask) and is finite.  A lane then sums its
// (2R + 1)^2 taps from the LDS in the defined order.  Products are statements of their own: nothing here is fused.
template <int R> __global__ __launch_bounds__(kBlock) void k_temporal_box(TemporalBoxArgs a) {
    constexpr int TW = 64 + 2 * R, NT = TW * (4 + 2 * R);
    __shared__ double Lc[3 * NT];
    __shared__ uint8_t Lk[NT];
    const int tx0 = a.x0 + (int)(blockIdx.x * 64u), ty0 = a.y0 + (int)(blockIdx.y * 4u);
    for (int t = (int)(threadIdx.y * 64u + threadIdx.x); t < NT; t += kBlock) {
        const int ty = t / TW, tx = t - ty * TW;
        const int gx = tx0 - R + tx, gy = ty0 - R + ty;
        uint8_t k = 0;
        if (gx >= 0 && gx < a.res_h && gy >= 0 && gy < a.res_v) {
            const size_t q = (size_t)gy * (size_t)a.res_h + (size_t)gx;
            if (a.mask[q]) {
                const double c0 = a.frame[3 * q], c1 = a.frame[3 * q + 1], c2 = a.frame[3 * q + 2];
                if (finite3(c0, c1, c2)) { k = 1; Lc[3 * t] = c0; Lc[3 * t + 1] = c1; Lc[3 * t + 2] = c2; }
            }
        }
        Lk[t] = k;
    }
    __syncthreads();
    const int lx = (int)(blockIdx.x * 64u + threadIdx.x), ly = (int)(blockIdx.y * 4u + threadIdx.y);
    if (lx >= a.w || ly >= a.h) return;
    const size_t id = (size_t)(a.y0 + ly) * (size_t)a.res_h + (size_t)(a.x0 + lx);
    double n = 0.0, s1[3] = {0.0, 0.0, 0.0}, s2[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int dy = 0; dy <= 2 * R; ++dy) {
#pragma unroll
        for (int dx = 0; dx <= 2 * R; ++dx) {
            const int t = ((int)threadIdx.y + dy) * TW + (int)threadIdx.x + dx;
            if (!Lk[t]) continue;
            n += 1.0;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const double c = Lc[3 * t + ch];
                const double cc = c * c;
                s1[ch] += c; s2[ch] += cc;
            }
        }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {                                // (a pixel that is not finite itself may have no tap: NaN, and clause 3a never reads it)
        const double mu = s1[ch] / n, m2 = s2[ch] / n;
        const double mm = mu * mu;
        const double v = m2 - mm;
        const double sd = sqrt(v > 0.0 ? v : 0.0);
        const double gs = a.gamma * sd;
        const double h = gs + a.floor;
        a.box.lo[ch][id] = mu - h; a.box.hi[ch][id] = mu + h;
    }
}

// The end of a queued call.  What it hands over was written by kernels that ended before this one began (their atomics were performed
// at the L2), so the loads need no fence; the record lies in pinned host memory and the stores are plain vector stores: they are
// visible to the host when the kernel has ended, and the host reads the record only behind an event recorded after this launch (the
// frame driver's hand_over_frame relies on the same).  The loads return before the cells are cleared: each lane clears what it read.
__global__ __launch_bounds__(64) void k_temporal_report(unsigned long long* temporal_counters, unsigned long long* guide_counters, TemporalReport* report) {
    const uint32_t t = threadIdx.x;
    if (t >= 8) return;
    unsigned long long* const cell = t < 3 ? temporal_counters + t : (t < 5 ? guide_counters + (t - 3) : nullptr);
    const unsigned long long v = cell ? *cell : 0ull;
    reinterpret_cast<unsigned long long*>(report)[t] = v;
    if (cell) *cell = 0ull;
}

} // namespace

void launch_temporal_report(hipStream_t stream, unsigned long long* temporal_counters, unsigned long long* guide_counters, TemporalReport* report) {
    hipLaunchKernelGGL(k_temporal_report, dim3(1), dim3(64), 0, stream, temporal_counters, guide_counters, report);
}

void launch_temporal(hipStream_t stream, const TemporalArgs& a) {
    if (a.win.n == 0) return;
    const dim3 grid((a.win.n + kBlock - 1) / kBlock), block(kBlock);
    if (a.box.lo[0]) {                                              // the clamp is on: the same three, reading the boxes
        if (a.deform) hipLaunchKernelGGL((k_temporal<true, true, true>), grid, block, 0, stream, a);
        else if (a.motion) hipLaunchKernelGGL((k_temporal<true, false, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((k_temporal<false, false, true>), grid, block, 0, stream, a);
        return;
    }
    if (a.deform) hipLaunchKernelGGL((k_temporal<true, true>), grid, block, 0, stream, a);   // (a null motion table: no leaf moved)
    else if (a.motion) hipLaunchKernelGGL(k_temporal<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(k_temporal<false>, grid, block, 0, stream, a);
}

void launch_temporal_box(hipStream_t stream, const TemporalBoxArgs& a) {
    if (a.w <= 0 || a.h <= 0) return;
    const dim3 grid = tile_grid(a.w, a.h), block = tile_block();
    if (a.radius == 1) hipLaunchKernelGGL(k_temporal_box<1>, grid, block, 0, stream, a);
    else if (a.radius == 2) hipLaunchKernelGGL(k_temporal_box<2>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(k_temporal_box<kTemporalClampMaxRadius>, grid, block, 0, stream, a);
}

} // namespace ftk

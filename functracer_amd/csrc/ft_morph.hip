// ft_morph.hip — morph targets ON THE DEVICE (ft_sg_set_mesh_weights + ft_scene_commit_deformed): the vertices of a mesh
// blended from a base and K deltas resident in HBM, straight into the buffer the refit reads (ft_refit.hip, `verts`), and the host's
// pass over them (fth::scan_mesh, fth::ls_pair_extent) as reductions of fixed shape.
//
//   k_morph_blend    per coordinate acc = B; acc = acc + w_k * D_k for k = 0 .. K-1 in order, product and sum rounded apart (__dmul_rn,
//                    __dadd_rn: -ffp-contract=on fuses within one source expression only, and these are two).  Pure streaming, two doubles
//                    (16 bytes) per lane and array; the weights are kernel arguments, hence scalar loads.
//   k_morph_scan     one triangle per lane: scan_mesh's bounds, extent and finiteness.  A bound travels with the list position of the
//                    value it came from (3 x triangle + corner) and equal values keep the smaller position, which is what the host's strict
//                    `v < bound` over the list does: -0.0 == +0.0, so a zero bound carries the sign of the FIRST zero in list order.  With
//                    the position as tie-break the combination is commutative and associative: no order of lanes, waves or blocks shows.
//   k_morph_fold     one block: the blocks' partials, the same combination.
//   k_morph_extent   fth::ls_pair_extent(vertices = true) about a given centre: a maximum of non-negative finite values; k_morph_extent_fold.
// Lane shuffles over the 64 lanes, the four waves of a block through LDS, one partial per block in a fixed slot, a second small launch:
// no floating-point atomics.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "ft_device.h"

namespace ftk {
namespace {

constexpr uint32_t kNoPos = 0xFFFFFFFFu;

// What one lane, wave or block knows of the scan: lo / hi bounds with the list positions they came from, extent, finiteness.
struct Scan {
    double b[6]; uint32_t at[6]; double extent; uint32_t finite;
};
__device__ __forceinline__ Scan scan_identity() {
    Scan s;
    for (int a = 0; a < 3; ++a) { s.b[a] = INFINITY; s.b[3 + a] = -INFINITY; s.at[a] = s.at[3 + a] = kNoPos; }
    s.extent = 0.0; s.finite = 1u;
    return s;
}
// (v, at) joins bound k of s: the smaller (k < 3) or larger value wins, of equal values the one that comes first in the list.  A NaN
// never wins (both comparisons are false) and is never in s.
__device__ __forceinline__ void join_bound(Scan& s, int k, double v, uint32_t at) {
    const bool better = k < 3 ? v < s.b[k] : v > s.b[k];
    if (better || (v == s.b[k] && at < s.at[k])) { s.b[k] = v; s.at[k] = at; }
}
__device__ __forceinline__ void join(Scan& s, const Scan& o) {
    for (int k = 0; k < 6; ++k) join_bound(s, k, o.b[k], o.at[k]);
    if (o.extent > s.extent) s.extent = o.extent;
    s.finite &= o.finite;
}
__device__ __forceinline__ Scan shuffled_down(const Scan& s, int delta) {
    Scan o;
    for (int k = 0; k < 6; ++k) { o.b[k] = __shfl_down(s.b[k], delta, 64); o.at[k] = __shfl_down(s.at[k], delta, 64); }
    o.extent = __shfl_down(s.extent, delta, 64); o.finite = __shfl_down(s.finite, delta, 64);
    return o;
}
// The block's scan in thread 0 (blocks of 256 threads: four waves).
__device__ __forceinline__ Scan block_scan(Scan s, Scan* lds) {
    for (int delta = 32; delta > 0; delta >>= 1) { const Scan o = shuffled_down(s, delta); join(s, o); }
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    if (lane == 0) lds[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) for (uint32_t w = 1; w < 4; ++w) join(s, lds[w]);
    return s;
}

__global__ __launch_bounds__(256) void k_morph_blend(MorphBlend a) {
    const uint64_t i = 2ull * (blockIdx.x * 256ull + threadIdx.x);
    if (i >= a.count) return;
    if (i + 1 < a.count) {                                          // (base, stride and out keep every pair 16-byte aligned)
        double2 acc = *reinterpret_cast<const double2*>(a.resident + i);
        for (int32_t k = 0; k < a.n_targets; ++k) {
            const double2 d = *reinterpret_cast<const double2*>(a.resident + (uint64_t)(k + 1) * a.stride + i);
            const double w = a.w[k];
            const double px = __dmul_rn(w, d.x), py = __dmul_rn(w, d.y);
            acc.x = __dadd_rn(acc.x, px);
            acc.y = __dadd_rn(acc.y, py);
        }
        *reinterpret_cast<double2*>(a.out + i) = acc;
    } else {                                                        // the last coordinate of an odd count
        double acc = a.resident[i];
        for (int32_t k = 0; k < a.n_targets; ++k) {
            const double p = __dmul_rn(a.w[k], a.resident[(uint64_t)(k + 1) * a.stride + i]);
            acc = __dadd_rn(acc, p);
        }
        a.out[i] = acc;
    }
}

__global__ __launch_bounds__(256) void k_morph_scan(const double* __restrict__ verts, uint32_t n, MorphPartial* __restrict__ partials) {
    __shared__ Scan lds[4];
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    Scan s = scan_identity();
    if (t < n) {
        const double* T = verts + 9ull * t;
        double v[9];
        for (int k = 0; k < 9; ++k) v[k] = T[k];
        for (int k = 0; k < 3; ++k) for (int a = 0; a < 3; ++a) { join_bound(s, a, v[3 * k + a], 3u * t + k); join_bound(s, 3 + a, v[3 * k + a], 3u * t + k); }
        for (int a = 0; a < 3; ++a) {                               // as the hit test sees them: v0, v0 + e1, v0 + e2; then the corners as given
            const double e1 = v[3 + a] - v[a], e2 = v[6 + a] - v[a];
            const double f[3] = {fabs(v[a]), fabs(v[a] + e1), fabs(v[a] + e2)};
            for (int q = 0; q < 3; ++q) { if (!(f[q] < 1e300)) s.finite = 0u; if (f[q] > s.extent) s.extent = f[q]; }
            if (!(fabs(v[3 + a]) < 1e300) || !(fabs(v[6 + a]) < 1e300)) s.finite = 0u;
        }
    }
    s = block_scan(s, lds);
    if (threadIdx.x == 0) {
        MorphPartial& P = partials[blockIdx.x];
        for (int k = 0; k < 6; ++k) { P.b[k] = s.b[k]; P.at[k] = s.at[k]; }
        P.extent = s.extent; P.finite = s.finite; P.pad = 0u;
    }
}

__global__ __launch_bounds__(256) void k_morph_fold(const MorphPartial* __restrict__ partials, uint32_t blocks, MorphScanOut* __restrict__ out) {
    __shared__ Scan lds[4];
    Scan s = scan_identity();
    for (uint32_t j = threadIdx.x; j < blocks; j += 256u) {
        const MorphPartial& P = partials[j];
        Scan o;
        for (int k = 0; k < 6; ++k) { o.b[k] = P.b[k]; o.at[k] = P.at[k]; }
        o.extent = P.extent; o.finite = P.finite;
        join(s, o);
    }
    s = block_scan(s, lds);
    if (threadIdx.x == 0) {
        for (int k = 0; k < 6; ++k) out->bounds[k] = s.b[k];
        out->extent = s.extent; out->finite = s.finite ? 1.0 : 0.0;
    }
}

// The block's maximum in thread 0.
__device__ __forceinline__ double block_max(double r, double* lds) {
    for (int delta = 32; delta > 0; delta >>= 1) { const double o = __shfl_down(r, delta, 64); if (r < o) r = o; }
    if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x == 0) for (uint32_t w = 1; w < 4; ++w) if (r < lds[w]) r = lds[w];
    return r;
}

__global__ __launch_bounds__(256) void k_morph_extent(const double* __restrict__ verts, uint32_t n, MorphCentre c, double* __restrict__ partials) {
    __shared__ double lds[4];
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    double R = 0.0;
    if (t < n) {
        const double* T = verts + 9ull * t;
        for (int v = 0; v < 3; ++v) {
            double p[3];
            for (int q = 0; q < 3; ++q) {
                const double e = v == 0 ? 0.0 : T[3 * v + q] - T[q];
                p[q] = (T[q] - c.c[q]) + e;
            }
            const double l1 = fabs(p[0]) + fabs(p[1]) + fabs(p[2]);
            if (R < l1) R = l1;
        }
    }
    R = block_max(R, lds);
    if (threadIdx.x == 0) partials[blockIdx.x] = R;
}

__global__ __launch_bounds__(256) void k_morph_extent_fold(const double* __restrict__ partials, uint32_t blocks, double* __restrict__ out) {
    __shared__ double lds[4];
    double R = 0.0;
    for (uint32_t j = threadIdx.x; j < blocks; j += 256u) if (R < partials[j]) R = partials[j];
    R = block_max(R, lds);
    if (threadIdx.x == 0) *out = R;
}

} // namespace

void morph_blend(hipStream_t stream, const MorphBlend& a) {
    if (a.count == 0) return;
    const uint64_t pairs = (a.count + 1) / 2;
    hipLaunchKernelGGL(k_morph_blend, dim3((uint32_t)((pairs + 255) / 256)), dim3(256), 0, stream, a);
}

void morph_scan(hipStream_t stream, const double* verts, uint32_t n, MorphPartial* partials, MorphScanOut* out) {
    const uint32_t blocks = morph_blocks(n);
    if (n) hipLaunchKernelGGL(k_morph_scan, dim3(blocks), dim3(256), 0, stream, verts, n, partials);
    hipLaunchKernelGGL(k_morph_fold, dim3(1), dim3(256), 0, stream, partials, n ? blocks : 0u, out);
}

void morph_extent(hipStream_t stream, const double* verts, uint32_t n, const double c[3], double* partials, double* out) {
    const uint32_t blocks = morph_blocks(n);
    MorphCentre C{{c[0], c[1], c[2]}};
    if (n) hipLaunchKernelGGL(k_morph_extent, dim3(blocks), dim3(256), 0, stream, verts, n, C, partials);
    hipLaunchKernelGGL(k_morph_extent_fold, dim3(1), dim3(256), 0, stream, partials, n ? blocks : 0u, out);
}

} // namespace ftk

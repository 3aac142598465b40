// ft_skin.hip — linear-blend skinning ON THE DEVICE (ft_sg_set_mesh_bones + ft_scene_commit_deformed): the corners of a mesh
// posed by a palette of 3x4 bone matrices, straight into the buffer the refit reads (ft_refit.hip, `verts`).  The bounds, extent and
// finiteness of the result, and the light-space R, are ft_morph.hip's reductions over that buffer, as they are.
//
//   k_skin<J, LDS>   one corner per lane, blocks of 256.  The block stages the palette into LDS (n_bones x 96 bytes, at most 24 KiB; 16 bytes
//                    per lane and step), a lane loads its three coordinates, its J bone indices as one 32-bit word (a byte per slot) and its J
//                    weights from slot-major arrays (weight[j][corner]: a wave's loads are contiguous), and evaluates per influence, in slot order,
//                        t_i = ((M[i][0] * x + M[i][1] * y) + M[i][2] * z) + M[i][3];  q_i = w_j * t_i;  acc_i = j == 0 ? q_i : acc_i + q_i
//                    with every product and sum a statement of its own (__dmul_rn, __dadd_rn: -ffp-contract=on fuses within one source
//                    expression only): fth::skin_blend's bits.  Every influence is evaluated, zero weights included.  J is a template
//                    parameter: straight-line code.  src == out is the morph-then-skin route: a lane reads only its own corner before it
//                    writes it.  Corners are independent, so the last block's tail is a bounds test and nothing else.
//   LDS = false      gathers the matrices from global memory instead (FT_SKIN_PALETTE_GLOBAL builds, for the A/B of DESIGN.md 16.5).
//
// Dual-quaternion skinning (ft_sg_set_mesh_bones_dq): the same lanes, blocks, index words and slot-major weights.
//
//   k_skin_dq<J, LDS>  The block stages the palette into LDS as double2 (4 per bone: n_bones x 64 bytes, at most 16 KiB).  A lane reads the
//                    real part of slot 0's bone once more as R0, and per influence, in slot order, the bone's eight values D:
//                        g = ((D0*R0_0 + D1*R0_1) + D2*R0_2) + D3*R0_3;  ws = (j > 0 && g < 0) ? -w_j : w_j;  a_k = j == 0 ? ws*D_k : a_k + ws*D_k
//                    The sign is a select on ws, not a branch: lanes of a wave whose bones lie on opposite hemispheres run the same
//                    instructions.  Then n = sqrt(((a0*a0 + a1*a1) + a2*a2) + a3*a3), s = 1 / n, u = a * s and, with w = u0, v = u1..3,
//                    e = u4, f = u5..7:  c = cross(v, p) + w*p;  h = cross(v, c);  m = (w*f - e*v) + cross(v, f);  V = (p + 2h) + 2m.
//                    Every operation is an intrinsic call of its own (__dmul_rn, __dadd_rn, __dsub_rn, __dsqrt_rn, __ddiv_rn - the last two
//                    correctly rounded): fth::skin_blend_dq's bits.  It shares no device function with k_skin.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "ft_device.h"

#ifndef FT_SKIN_PALETTE_GLOBAL
#define FT_SKIN_PALETTE_GLOBAL 0
#endif

namespace ftk {
namespace {

// One row of a bone matrix applied to (x, y, z): left to right, one rounding per operation.
__device__ __forceinline__ double skin_row(const double* R, double x, double y, double z) {
    const double px = __dmul_rn(R[0], x);
    const double py = __dmul_rn(R[1], y);
    const double pz = __dmul_rn(R[2], z);
    double t = __dadd_rn(px, py);
    t = __dadd_rn(t, pz);
    t = __dadd_rn(t, R[3]);
    return t;
}

template <int J, bool LDS>
__global__ __launch_bounds__(256) void k_skin(SkinPose a) {
    extern __shared__ double2 staged[];                             // LDS: 6 x n_bones of them
    const double* palette = a.palette;
    if constexpr (LDS) {
        const double2* g = reinterpret_cast<const double2*>(a.palette);
        const uint32_t n2 = 6u * (uint32_t)a.n_bones;
        for (uint32_t i = threadIdx.x; i < n2; i += 256u) staged[i] = g[i];
        __syncthreads();
        palette = reinterpret_cast<const double*>(staged);
    }
    const uint64_t c = blockIdx.x * 256ull + threadIdx.x;
    if (c >= a.corners) return;
    const double x = a.src[3 * c], y = a.src[3 * c + 1], z = a.src[3 * c + 2];
    const uint32_t word = a.index[c];
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const double* M = palette + 12u * ((word >> (8 * j)) & 255u);
        const double w = a.weight[(uint64_t)j * a.wstride + c];
        const double t0 = skin_row(M, x, y, z);
        const double t1 = skin_row(M + 4, x, y, z);
        const double t2 = skin_row(M + 8, x, y, z);
        const double q0 = __dmul_rn(w, t0);
        const double q1 = __dmul_rn(w, t1);
        const double q2 = __dmul_rn(w, t2);
        if (j == 0) { acc0 = q0; acc1 = q1; acc2 = q2; }
        else { acc0 = __dadd_rn(acc0, q0); acc1 = __dadd_rn(acc1, q1); acc2 = __dadd_rn(acc2, q2); }
    }
    a.out[3 * c] = acc0; a.out[3 * c + 1] = acc1; a.out[3 * c + 2] = acc2;
}

// cross(a, b)_i: two products and one difference, each rounded once.
__device__ __forceinline__ double dq_cross(double a1, double a2, double b1, double b2) {
    const double l = __dmul_rn(a1, b2);
    const double r = __dmul_rn(a2, b1);
    return __dsub_rn(l, r);
}

template <int J, bool LDS>
__global__ __launch_bounds__(256) void k_skin_dq(SkinPose a) {
    extern __shared__ double2 staged[];                             // LDS: 4 x n_bones of them
    const double2* palette = reinterpret_cast<const double2*>(a.palette);
    if constexpr (LDS) {
        const uint32_t n2 = 4u * (uint32_t)a.n_bones;
        for (uint32_t i = threadIdx.x; i < n2; i += 256u) staged[i] = palette[i];
        __syncthreads();
        palette = staged;
    }
    const uint64_t c = blockIdx.x * 256ull + threadIdx.x;
    if (c >= a.corners) return;
    const double x = a.src[3 * c], y = a.src[3 * c + 1], z = a.src[3 * c + 2];
    const uint32_t word = a.index[c];
    double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0;                  // R0: the real part of slot 0's bone
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0, a5 = 0.0, a6 = 0.0, a7 = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const double2* D = palette + 4u * ((word >> (8 * j)) & 255u);
        const double2 d01 = D[0], d23 = D[1], d45 = D[2], d67 = D[3];
        const double wj = a.weight[(uint64_t)j * a.wstride + c];
        double ws = wj;
        if (j == 0) { r0 = d01.x; r1 = d01.y; r2 = d23.x; r3 = d23.y; }
        else {
            const double g0 = __dmul_rn(d01.x, r0);
            const double g1 = __dmul_rn(d01.y, r1);
            const double g2 = __dmul_rn(d23.x, r2);
            const double g3 = __dmul_rn(d23.y, r3);
            double g = __dadd_rn(g0, g1);
            g = __dadd_rn(g, g2);
            g = __dadd_rn(g, g3);
            ws = g < 0.0 ? -wj : wj;                                // a select; a NaN g does not negate
        }
        const double q0 = __dmul_rn(ws, d01.x), q1 = __dmul_rn(ws, d01.y), q2 = __dmul_rn(ws, d23.x), q3 = __dmul_rn(ws, d23.y);
        const double q4 = __dmul_rn(ws, d45.x), q5 = __dmul_rn(ws, d45.y), q6 = __dmul_rn(ws, d67.x), q7 = __dmul_rn(ws, d67.y);
        if (j == 0) { a0 = q0; a1 = q1; a2 = q2; a3 = q3; a4 = q4; a5 = q5; a6 = q6; a7 = q7; }
        else {
            a0 = __dadd_rn(a0, q0); a1 = __dadd_rn(a1, q1); a2 = __dadd_rn(a2, q2); a3 = __dadd_rn(a3, q3);
            a4 = __dadd_rn(a4, q4); a5 = __dadd_rn(a5, q5); a6 = __dadd_rn(a6, q6); a7 = __dadd_rn(a7, q7);
        }
    }
    const double s0 = __dmul_rn(a0, a0), s1 = __dmul_rn(a1, a1), s2 = __dmul_rn(a2, a2), s3 = __dmul_rn(a3, a3);
    double n2 = __dadd_rn(s0, s1);
    n2 = __dadd_rn(n2, s2);
    n2 = __dadd_rn(n2, s3);
    const double n = __dsqrt_rn(n2);
    const double s = __ddiv_rn(1.0, n);
    const double w = __dmul_rn(a0, s), v0 = __dmul_rn(a1, s), v1 = __dmul_rn(a2, s), v2 = __dmul_rn(a3, s);
    const double e = __dmul_rn(a4, s), f0 = __dmul_rn(a5, s), f1 = __dmul_rn(a6, s), f2 = __dmul_rn(a7, s);
    // c = cross(v, p) + w * p
    const double c0 = __dadd_rn(dq_cross(v1, v2, y, z), __dmul_rn(w, x));
    const double c1 = __dadd_rn(dq_cross(v2, v0, z, x), __dmul_rn(w, y));
    const double c2 = __dadd_rn(dq_cross(v0, v1, x, y), __dmul_rn(w, z));
    // h = cross(v, c)
    const double h0 = dq_cross(v1, v2, c1, c2);
    const double h1 = dq_cross(v2, v0, c2, c0);
    const double h2 = dq_cross(v0, v1, c0, c1);
    // m = (w * f - e * v) + cross(v, f)
    const double m0 = __dadd_rn(__dsub_rn(__dmul_rn(w, f0), __dmul_rn(e, v0)), dq_cross(v1, v2, f1, f2));
    const double m1 = __dadd_rn(__dsub_rn(__dmul_rn(w, f1), __dmul_rn(e, v1)), dq_cross(v2, v0, f2, f0));
    const double m2 = __dadd_rn(__dsub_rn(__dmul_rn(w, f2), __dmul_rn(e, v2)), dq_cross(v0, v1, f0, f1));
    // V = (p + 2 h) + 2 m
    a.out[3 * c] = __dadd_rn(__dadd_rn(x, __dmul_rn(2.0, h0)), __dmul_rn(2.0, m0));
    a.out[3 * c + 1] = __dadd_rn(__dadd_rn(y, __dmul_rn(2.0, h1)), __dmul_rn(2.0, m1));
    a.out[3 * c + 2] = __dadd_rn(__dadd_rn(z, __dmul_rn(2.0, h2)), __dmul_rn(2.0, m2));
}

template <int J>
void launch(hipStream_t stream, const SkinPose& a) {
    constexpr bool lds = !FT_SKIN_PALETTE_GLOBAL;
    const uint32_t blocks = (uint32_t)((a.corners + 255) / 256);
    hipLaunchKernelGGL((k_skin<J, lds>), dim3(blocks), dim3(256), lds ? (size_t)a.n_bones * 96 : 0, stream, a);
}

template <int J>
void launch_dq(hipStream_t stream, const SkinPose& a) {
    constexpr bool lds = !FT_SKIN_PALETTE_GLOBAL;
    const uint32_t blocks = (uint32_t)((a.corners + 255) / 256);
    hipLaunchKernelGGL((k_skin_dq<J, lds>), dim3(blocks), dim3(256), lds ? (size_t)a.n_bones * 64 : 0, stream, a);
}

} // namespace

void skin(hipStream_t stream, const SkinPose& a) {
    if (a.corners == 0 || a.n_bones < 1 || a.n_bones > kMaxSkinBones) return;
    switch (a.influences) {
        case 1: launch<1>(stream, a); break;
        case 2: launch<2>(stream, a); break;
        case 3: launch<3>(stream, a); break;
        case 4: launch<4>(stream, a); break;
        default: break;
    }
}

void skin_dq(hipStream_t stream, const SkinPose& a) {
    if (a.corners == 0 || a.n_bones < 1 || a.n_bones > kMaxSkinBones) return;
    switch (a.influences) {
        case 1: launch_dq<1>(stream, a); break;
        case 2: launch_dq<2>(stream, a); break;
        case 3: launch_dq<3>(stream, a); break;
        case 4: launch_dq<4>(stream, a); break;
        default: break;
    }
}

} // namespace ftk

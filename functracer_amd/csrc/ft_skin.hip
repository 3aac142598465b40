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

template <int J>
void launch(hipStream_t stream, const SkinPose& a) {
    constexpr bool lds = !FT_SKIN_PALETTE_GLOBAL;
    const uint32_t blocks = (uint32_t)((a.corners + 255) / 256);
    hipLaunchKernelGGL((k_skin<J, lds>), dim3(blocks), dim3(256), lds ? (size_t)a.n_bones * 96 : 0, stream, a);
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

} // namespace ftk

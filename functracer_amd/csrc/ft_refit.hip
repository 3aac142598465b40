// ft_refit.hip — the BVH of a top-level-Leaf mesh refit ON THE DEVICE after its vertices changed (ft_scene_commit_deformed).
// The tree any builder left in the scene's arrays - the host's swept surface-area split (ft_scene.cpp, BspBuilder::bvh_build) or one of
// ft_bvh.hip's - keeps its topology: left / right / axis, the leaf ranges, tri_orig, tri_src, the 4-wide children, the coarse frontier.
// What depends on the positions is written again, so that the tree still (a) holds every triangle once, (b) bounds them with inflated
// boxes and (c) breaks ties by list index: the three properties that make it give the linear scan's hits bit for bit (ft_flat.h).
//
// Stages (all on the context's stream; n = triangles of the mesh):
//   k_refit_parents  once per full commit: the parent of every node and leaf of the tree, read off the emitted left / right
//   k_refit_records  per list-order triangle v0, e1 = v1 - v0, e2 = v2 - v0 (the flattener's subtraction); per sorted copy the same
//                    arithmetic on its tri_orig's vertices, hence a bitwise copy of that record
//   k_refit_fit      per leaf its box from (v0, v0 + e1, v0 + e2) - what the hit test reads, as k_bvh_prepare - inflated; then leaves to
//                    root as k_bvh_fit: the second child to arrive unites the boxes.  Inflating commutes with min / max (x - pad is
//                    monotone in x), so a node's stored box is the exact bound of its triangles, inflated: what every builder stores
//   k_refit_wide     per 4-wide node the inflated boxes of what its slots point to; empty slots stay all-NaN
//   k_refit_coarse   one thread: the level of the tree with at most 64 nodes (the rule both builders use), as float boxes rounded outward
// k_refit_carry copies ranges of these arrays from one geometry set to another (ft_scene_commit_deformed_enqueue): what
// a queued refit does not write of a set that is behind the live one.
// Beside them k_refit_cost / k_refit_cost_sum measure the surface-area cost of a tree as it lies in HBM (ft_scene_tree_quality, the
// "refit_rebuild_percent" decision): one thread per node slot, a sum of fixed shape, no floating-point atomics.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdint.h>

#include "ft_device.h"
#include "ft_refit_cost.h"

using namespace ftd;

namespace ftk {
namespace {

using namespace refit;                                             // node_in, leaf_in, real_node, leaf_bound, the cost arithmetic (ft_refit_cost.h)

__global__ __launch_bounds__(256) void k_refit_parents(RefitArrays A, RefitMesh m) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= m.node_count) return;
    const uint32_t r = m.node_first + i;
    if (!real_node(A, m, r)) return;
    const int32_t ch[2] = {A.nodes[r].left, A.nodes[r].right};
    for (int c = 0; c < 2; ++c) {
        if (node_in(m, ch[c])) A.parent_node[ch[c]] = (int32_t)r;
        else if (leaf_in(m, ch[c])) A.parent_leaf[~ch[c]] = (int32_t)r;
    }
}

__global__ __launch_bounds__(256) void k_refit_records(RefitArrays A, RefitMesh m, const double* __restrict__ verts) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= m.n + m.tri_count) return;
    uint32_t dst = m.first_global + t, src = t;
    if (t >= m.n) {                                                 // a sorted copy: its list-order triangle's vertices
        dst = m.tri_first + (t - m.n);
        src = A.tri_orig[dst] - m.first_global;
        if (src >= m.n) return;
    }
    const double* V = verts + 9ull * src;
    double* O = A.tris + 9ull * dst;
    for (int a = 0; a < 3; ++a) { O[a] = V[a]; O[3 + a] = V[3 + a] - V[a]; O[6 + a] = V[6 + a] - V[a]; }
}

// The inflated box of leaf `l` (an index into the scene's BspLeaf array), or false when it is no leaf of the tree's size.
__device__ __forceinline__ bool leaf_box(const RefitArrays& A, const RefitMesh& m, uint32_t l, double box[6]) {
    if (!leaf_bound(A, m, l, box)) return false;
    for (int a = 0; a < 3; ++a) { box[a] = box[a] - m.pad; box[3 + a] = box[3 + a] + m.pad; }
    return true;
}

__global__ __launch_bounds__(256) void k_refit_fit(RefitArrays A, RefitMesh m) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= m.leaf_count) return;
    const uint32_t l = m.leaf_first + j;
    double box[6];
    if (!leaf_box(A, m, l, box)) return;
    for (int k = 0; k < 6; ++k) A.leaf_boxes[6ull * l + k] = box[k];
    if (m.device_built && j < m.node_count) {                       // a build node standing as a leaf: its BspNode record holds the same box
        BspNode* nd = A.nodes + (m.node_first + j);
        for (int a = 0; a < 3; ++a) { nd->bmin[a] = box[a]; nd->bmax[a] = box[3 + a]; }
    }
    int32_t node = A.parent_leaf[l];
    while (node_in(m, node)) {
        __threadfence();                                            // this thread's box of the child below is visible before the counter moves
        if (atomicAdd(&A.arrived[node], 1u) == 0u) return;          // the sibling subtree is not done yet: its thread carries on from here
        __threadfence();
        double lo[3], hi[3];
        const int32_t ch[2] = {A.nodes[node].left, A.nodes[node].right};
        for (int c = 0; c < 2; ++c) {
            if (!(node_in(m, ch[c]) || leaf_in(m, ch[c]))) return;
            const volatile double* b = ch[c] >= 0 ? A.nodes[ch[c]].bmin : A.leaf_boxes + 6ull * (uint32_t)~ch[c];   // (bmin, bmax: six doubles in a row)
            for (int a = 0; a < 3; ++a) { const double lw = b[a], up = b[3 + a]; lo[a] = c == 0 ? lw : fmin(lo[a], lw); hi[a] = c == 0 ? up : fmax(hi[a], up); }
        }
        for (int a = 0; a < 3; ++a) { A.nodes[node].bmin[a] = lo[a]; A.nodes[node].bmax[a] = hi[a]; }
        node = A.parent_node[node];
    }
}

// The inflated box of what a reference of the tree points to: a node's record, a leaf's entry of leaf_boxes.
__device__ __forceinline__ bool ref_box(const RefitArrays& A, const RefitMesh& m, int32_t ref, double* out) {
    const double* b;
    if (node_in(m, ref)) b = A.nodes[ref].bmin;
    else if (leaf_in(m, ref)) b = A.leaf_boxes + 6ull * (uint32_t)~ref;
    else return false;
    for (int k = 0; k < 6; ++k) out[k] = b[k];
    return true;
}

__global__ __launch_bounds__(256) void k_refit_wide(RefitArrays A, RefitMesh m) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= m.wide_count) return;
    const uint32_t w = m.wide_first + i;
    const int32_t b = A.wide_node[w];
    if (!node_in(m, b) || !real_node(A, m, (uint32_t)b)) return;
    double* W = A.wide + (unsigned long long)kWideNodeDoubles * w;
    const int32_t halves[2] = {A.nodes[b].left, A.nodes[b].right};
    for (int h = 0; h < 2; ++h) {                                   // the slots as widen / k_bvh_emit fill them: a leaf takes one slot of its half
        const int32_t c = halves[h];
        if (c < 0) { ref_box(A, m, c, W + 6 * (2 * h)); continue; }
        if (!node_in(m, c)) continue;
        const int32_t gk[2] = {A.nodes[c].left, A.nodes[c].right};
        for (int k = 0; k < 2; ++k) ref_box(A, m, gk[k], W + 6 * (2 * h + k));
    }
}

__device__ __forceinline__ float round_down(double v) { float f = (float)v; if ((double)f > v) f = __uint_as_float(f > 0.0f ? __float_as_uint(f) - 1u : (f < 0.0f ? __float_as_uint(f) + 1u : 0x80000001u)); return f; }
__device__ __forceinline__ float round_up(double v) { return -round_down(-v); }
// The frontier both builders take (build_bsp, k_bvh_coarse): levels of the tree as long as the next one has at most 64 entries; the
// same `count` boxes, the last one repeated where the frontier is shorter; k_bvh_coarse's outward rounding, here of the inflated boxes.
__global__ void k_refit_coarse(RefitArrays A, RefitMesh m) {
    __shared__ int32_t frontier[2][64];
    if (threadIdx.x != 0 || m.coarse_count == 0u || !(node_in(m, m.bvh_root) || leaf_in(m, m.bvh_root))) return;
    int cur = 0; uint32_t nf = 1;
    frontier[0][0] = m.bvh_root;
    for (;;) {
        uint32_t nn = 0; bool any_inner = false, fits = true;
        for (uint32_t k = 0; k < nf; ++k) {
            const int32_t c = frontier[cur][k];
            const bool inner = node_in(m, c);
            if (nn + (inner ? 2u : 1u) > 64u) { fits = false; break; }
            if (!inner) { frontier[cur ^ 1][nn++] = c; continue; }
            any_inner = true;
            frontier[cur ^ 1][nn++] = A.nodes[c].left; frontier[cur ^ 1][nn++] = A.nodes[c].right;
        }
        if (!any_inner || !fits) break;
        cur ^= 1; nf = nn;
    }
    for (uint32_t k = 0; k < m.coarse_count; ++k) {
        double b[6];
        if (!ref_box(A, m, frontier[cur][k < nf ? k : nf - 1u], b)) continue;
        float* out = A.coarse + 6ull * (m.coarse_first + k);
        for (int x = 0; x < 3; ++x) {
            const double lo = b[x], hi = b[3 + x];
            const double pad = 1e-5 * (fabs(lo) + fabs(hi) + (hi - lo)) + 1e-30;
            out[x] = round_down(lo - pad); out[3 + x] = round_up(hi + pad);
        }
    }
}

// One thread per node slot of the mesh's range (cost_term, ft_refit_cost.h).  The block's sum has a fixed shape: xor shuffles within the
// wave64, the four waves in order through LDS, one partial per block.
__global__ __launch_bounds__(256) void k_refit_cost(RefitArrays A, RefitMesh m, double* __restrict__ partials) {
    __shared__ double wave_sum[4];
    double term = cost_term(A, m, blockIdx.x * 256u + threadIdx.x);
    for (int off = 32; off > 0; off >>= 1) term += __shfl_xor(term, off);
    if ((threadIdx.x & 63u) == 0u) wave_sum[threadIdx.x >> 6] = term;
    __syncthreads();
    if (threadIdx.x == 0u) partials[blockIdx.x] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}
// One thread: the partials in index order, over the area of the root's stored box.
__global__ void k_refit_cost_sum(RefitArrays A, RefitMesh m, const double* __restrict__ partials, uint32_t n_partials, double* __restrict__ cost) {
    if (blockIdx.x != 0u || threadIdx.x != 0u) return;
    double sum = 0.0;
    for (uint32_t k = 0; k < n_partials; ++k) sum += partials[k];
    *cost = cost_of_sum(A, m, sum);
}

// Range blockIdx.y of the table, the launch's blocks along x striding over its 16-byte lanes; the first thread also copies the 8-byte
// element in front of the first whole lane and the one behind the last, where the range starts or ends between two lanes.
__global__ __launch_bounds__(256) void k_refit_carry(CarryTable t) {
    if (blockIdx.y >= t.n) return;
    const CarryRange r = t.r[blockIdx.y];
    const unsigned long long head = (16ull - ((unsigned long long)(uintptr_t)r.src & 15ull)) & 15ull;   // 0 or 8
    if (r.bytes < head + 16ull) {                                   // no whole lane: at most two elements
        if (blockIdx.x == 0u && threadIdx.x < r.bytes / 8ull) reinterpret_cast<double*>(r.dst)[threadIdx.x] = reinterpret_cast<const double*>(r.src)[threadIdx.x];
        return;
    }
    const unsigned long long lanes = (r.bytes - head) / 16ull, tail = head + 16ull * lanes;
    const double2* __restrict__ src = reinterpret_cast<const double2*>(r.src + head);
    double2* __restrict__ dst = reinterpret_cast<double2*>(r.dst + head);
    for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i < lanes; i += gridDim.x * 256ull) dst[i] = src[i];
    if (blockIdx.x == 0u && threadIdx.x == 0u) {
        if (head) *reinterpret_cast<double*>(r.dst) = *reinterpret_cast<const double*>(r.src);
        if (tail < r.bytes) *reinterpret_cast<double*>(r.dst + tail) = *reinterpret_cast<const double*>(r.src + tail);
    }
}

} // namespace

void refit_carry(hipStream_t stream, const CarryTable& t) {
    if (t.n == 0u) return;
    uint64_t most = 0;
    for (uint32_t k = 0; k < t.n; ++k) most = most > t.r[k].bytes ? most : t.r[k].bytes;
    const uint64_t blocks = (most / 16u + 255u) / 256u;             // the longest range's lanes, 256 blocks per range at most: the rest is strided
    hipLaunchKernelGGL(k_refit_carry, dim3((uint32_t)(blocks < 1u ? 1u : (blocks > 256u ? 256u : blocks)), t.n), dim3(256), 0, stream, t);
}

void refit_cost(hipStream_t stream, const RefitArrays& A, const RefitMesh& m, double* partials, double* cost) {
    const uint32_t blocks = refit_cost_blocks(m);
    if (blocks) hipLaunchKernelGGL(k_refit_cost, dim3(blocks), dim3(256), 0, stream, A, m, partials);
    hipLaunchKernelGGL(k_refit_cost_sum, dim3(1), dim3(64), 0, stream, A, m, partials, blocks, cost);
}

void refit_parents(hipStream_t stream, const RefitArrays& A, const RefitMesh& m) {
    if (m.node_count == 0u) return;
    hipLaunchKernelGGL(k_refit_parents, dim3((m.node_count + 255u) / 256u), dim3(256), 0, stream, A, m);
}

void refit_mesh(hipStream_t stream, const RefitArrays& A, const RefitMesh& m, const double* verts) {
    if (m.n == 0u) return;
    hipLaunchKernelGGL(k_refit_records, dim3((m.n + m.tri_count + 255u) / 256u), dim3(256), 0, stream, A, m, verts);
    if (m.bvh_root == INT32_MIN || m.leaf_count == 0u) return;
    hipLaunchKernelGGL(k_refit_fit, dim3((m.leaf_count + 255u) / 256u), dim3(256), 0, stream, A, m);
    if (m.wide_count) hipLaunchKernelGGL(k_refit_wide, dim3((m.wide_count + 255u) / 256u), dim3(256), 0, stream, A, m);
    if (m.coarse_count) hipLaunchKernelGGL(k_refit_coarse, dim3(1), dim3(64), 0, stream, A, m);
}

} // namespace ftk

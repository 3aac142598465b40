// ft_lightspace.hip — the light-space shadow tree of a (mesh leaf, directional light) pair refit ON THE DEVICE after the light turned
// (ft_scene_commit_lights).  The tree the host built at the last full commit (ft_scene.cpp, build_light_space) keeps its
// topology - the child words of every 4-wide node and the leaf records in ls_tris, bitwise copies of the mesh's own records - and only the
// projection changes: every child box is written again in the pair's new frame (U, V, D) about the same centre c.  A tree that holds every
// triangle in conservative boxes gives the BVH walk's bits whatever its shape (ft_flat.h), so no tracing kernel changes.
//
// k_ls_refit: one lane per 4-wide node, one launch per level of the tree, deepest level first (the host derives the order once per full
// commit).  A leaf child ~(first << 3 | count) projects the three vertices of its records into the new frame in FP64, with the host
// builder's own unfused arithmetic, and rounds outward to float through the device twins of f_down / f_up; a node child takes the union of
// that node's four child boxes, which the level before wrote (a union of floats is exact, and f_down / f_up are monotone, so the result is
// what the host's widen computes from the union in double).  Empty slots keep their NaN boxes.
//
// The same passes serve a mesh whose vertices changed (ft_scene_commit_deformed under "deform_light_space"): there the
// frame stays and the centre, the pad and the leaf records change, so k_ls_gather first copies the refit list-order records into the
// tree's leaves, and k_ls_refit and the grid passes then run as for a turned light.
//
// Under "light_space_retree"  the topology is built again as well: k_ls_keys gives every list-order triangle of the pair
// the Morton code of its projected centre, a radix sort orders the triangles by it, k_ls_gather copies the records in that order, and
// k_ls_refit boxes the tree the host generated over the sorted positions (ft_ls_topology.h) - a function of the triangle count alone.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <math.h>
#include <stdint.h>

#include "ft_device.h"
#include "ft_edges.h"

using namespace ftd;

namespace ftk {
namespace {

// LsBuilder::f_down / f_up (ft_scene.cpp): the float at or below / above a double.
__device__ __forceinline__ float f_down(double v) { float f = (float)v; if ((double)f > v) f = __uint_as_float(f > 0.0f ? __float_as_uint(f) - 1u : (f < 0.0f ? __float_as_uint(f) + 1u : 0x80000001u)); return f; }
__device__ __forceinline__ float f_up(double v) { return -f_down(-v); }
// a . b summed left to right, unfused: the host builder's `p[0] * U[0] + p[1] * U[1] + p[2] * U[2]` under -ffp-contract=off
__device__ __forceinline__ double dot_lr(const double p[3], const double a[3]) { return __dadd_rn(__dadd_rn(__dmul_rn(p[0], a[0]), __dmul_rn(p[1], a[1])), __dmul_rn(p[2], a[2])); }

// The (u, v) rectangle and the largest w of a running set grown by one triangle record (v0, e1, e2), as build_light_space projects it.
__device__ __forceinline__ void grow_by_tri(const double* __restrict__ T, const LsFrame& F, double lo[2], double hi[2], double& wmax) {
    for (int v = 0; v < 3; ++v) {
        double p[3];
        for (int q = 0; q < 3; ++q) p[q] = __dadd_rn(__dsub_rn(T[q], F.c[q]), v == 1 ? T[3 + q] : v == 2 ? T[6 + q] : 0.0);
        const double pu = dot_lr(p, F.U), pv = dot_lr(p, F.V), pw = dot_lr(p, F.D);
        lo[0] = fmin(lo[0], pu); hi[0] = fmax(hi[0], pu);
        lo[1] = fmin(lo[1], pv); hi[1] = fmax(hi[1], pv);
        wmax = fmax(wmax, pw);
    }
}
__device__ __forceinline__ void round_box(const double lo[2], const double hi[2], double wmax, double pad, float box[5]) {
    box[0] = f_down(lo[0] - pad); box[1] = f_up(hi[0] + pad);
    box[2] = f_down(lo[1] - pad); box[3] = f_up(hi[1] + pad);
    box[4] = f_up(wmax + pad);
}

__global__ __launch_bounds__(256) void k_ls_refit(uint32_t* __restrict__ nodes, uint32_t n_nodes, const double* __restrict__ tris, uint32_t n_tris,
                                                  const uint32_t* __restrict__ order, uint32_t count, LsFrame F) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const uint32_t n = order[i];
    if (n >= n_nodes) return;
    uint32_t* N = nodes + (size_t)kLsNodeWords * n;
    for (int c = 0; c < 4; ++c) {
        const int32_t child = (int32_t)N[20 + c];
        if (child == INT32_MIN) continue;                           // an empty slot: its all-NaN box stays
        float box[5];
        if (child >= 0) {
            if ((uint32_t)child >= n_nodes) continue;
            const float* B = reinterpret_cast<const float*>(nodes + (size_t)kLsNodeWords * (uint32_t)child);
            box[0] = box[2] = INFINITY; box[1] = box[3] = box[4] = -INFINITY;
            for (int k = 0; k < 4; ++k) {                           // fminf / fmaxf pass over the NaN of an empty slot
                box[0] = fminf(box[0], B[5 * k]); box[1] = fmaxf(box[1], B[5 * k + 1]);
                box[2] = fminf(box[2], B[5 * k + 2]); box[3] = fmaxf(box[3], B[5 * k + 3]);
                box[4] = fmaxf(box[4], B[5 * k + 4]);
            }
        } else {
            const uint32_t first = (uint32_t)~child >> 3, cnt = (uint32_t)~child & 7u;
            if ((uint64_t)first + cnt > n_tris) continue;
            double lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY}, wmax = -INFINITY;
            for (uint32_t t = 0; t < cnt; ++t) grow_by_tri(tris + 9ull * (first + t), F, lo, hi, wmax);
            round_box(lo, hi, wmax, F.pad, box);
        }
        for (int k = 0; k < 5; ++k) N[5 * c + k] = __float_as_uint(box[k]);
    }
}

// ---- the leaf records of a pair's tree after its mesh was refit (ft_scene_commit_deformed under "deform_light_space") ----
// One lane per leaf record of the tree: ls_tris[ls_first + i] becomes the bitwise copy of tris[src[i]] again, the list-order record
// k_refit_records has just written for the triangle that record copied at the full commit (fth::FlatScene::ls_src).  An index outside the
// mesh's list-order range [mesh_first, mesh_first + mesh_n), outside tris (n_tris records) or outside ls_tris (n_ls records) writes nothing.
__global__ __launch_bounds__(256) void k_ls_gather(const double* __restrict__ tris, uint32_t n_tris, uint32_t mesh_first, uint32_t mesh_n, const uint32_t* __restrict__ src,
                                                   uint32_t count, double* __restrict__ ls_tris, uint32_t n_ls, uint32_t ls_first) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const uint32_t s = src[i];
    const uint64_t d = (uint64_t)ls_first + i;
    if (s < mesh_first || s - mesh_first >= mesh_n || s >= n_tris || d >= n_ls) return;
    const double* T = tris + 9ull * s;
    double* O = ls_tris + 9ull * d;
    for (int q = 0; q < 9; ++q) O[q] = T[q];
}

// ---- the order of a pair's leaf records under "light_space_retree"  ------------------------------------------------------
// x in the even bits, y in the odd bits
__device__ __forceinline__ uint32_t spread16(uint32_t v) {
    v &= 0xFFFFu;
    v = (v | v << 8) & 0x00FF00FFu; v = (v | v << 4) & 0x0F0F0F0Fu; v = (v | v << 2) & 0x33333333u; v = (v | v << 1) & 0x55555555u;
    return v;
}
// A centre coordinate in [-R, R] on 65536 steps, clamped; a NaN gives 0 (fmax and fmin return their other operand).
__device__ __forceinline__ uint32_t morton_axis(double c, double R, double g) { return (uint32_t)fmin(65535.0, fmax(0.0, floor(__dmul_rn(__dadd_rn(c, R), g)))); }

// One lane per list-order triangle k of the pair (record first_tri + k of tris, n_tris records in all): the (u, v) rectangle exactly as
// grow_by_tri computes it, its centre, and the Morton code of the centre as the key; the record's index as the value.  g = 32768 / R.
__global__ __launch_bounds__(256) void k_ls_keys(const double* __restrict__ tris, uint32_t n_tris, uint32_t first_tri, uint32_t n, LsFrame F, double R, double g,
                                                 uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    const uint64_t t = (uint64_t)first_tri + k;
    uint32_t key = 0u;
    if (t < n_tris) {
        double lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY}, wmax = -INFINITY;
        grow_by_tri(tris + 9ull * t, F, lo, hi, wmax);
        const double cu = __dmul_rn(0.5, __dadd_rn(lo[0], hi[0])), cv = __dmul_rn(0.5, __dadd_rn(lo[1], hi[1]));
        key = spread16(morton_axis(cu, R, g)) | spread16(morton_axis(cv, R, g)) << 1;
    }
    keys[k] = key; vals[k] = (uint32_t)t;                           // (an index outside tris: k_ls_gather writes nothing for it)
}

// ---- the grid of a pair, built again (ft_scene.cpp, build_grid, with its host loops as passes) ----------------------------------------
// The cell of a float coordinate along an axis of n cells: the float operations of the host's ls_cell and of the tracing kernels'.
__device__ __forceinline__ uint32_t ls_cell(float x, float s, uint32_t n) {
    const float f = __builtin_floorf(__builtin_fmaf(x, s, 0.5f * (float)n));
    return (uint32_t)fminf(fmaxf(f, 0.0f), (float)(n - 1));
}

// One lane per list-order triangle of the mesh: its five-float entry box; ruv (when given): the largest |u| and |v| bound over all
// entries, as the bits of non-negative floats (an integer maximum orders them as the floats).
__global__ __launch_bounds__(256) void k_ls_entries(const double* __restrict__ tris, uint32_t n, LsFrame F, float* __restrict__ ebox, uint32_t* __restrict__ ruv) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    double lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY}, wmax = -INFINITY;
    grow_by_tri(tris + 9ull * k, F, lo, hi, wmax);
    float box[5];
    round_box(lo, hi, wmax, F.pad, box);
    for (int q = 0; q < 5; ++q) ebox[5ull * k + q] = box[q];
    if (!ruv) return;
    atomicMax(&ruv[0], __float_as_uint(fmaxf(fabsf(box[0]), fabsf(box[1]))));
    atomicMax(&ruv[1], __float_as_uint(fmaxf(fabsf(box[2]), fabsf(box[3]))));
}

// The cells every triangle's rectangle covers under each candidate of the host's attempt loop, summed into one counter per candidate.
__global__ __launch_bounds__(256) void k_ls_count(const float* __restrict__ ebox, uint32_t n, LsGridCandidates C, unsigned long long* __restrict__ sums) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    const float* e = ebox + 5ull * k;
    for (int a = 0; a < C.n; ++a) {
        const float s = C.s[a]; const uint32_t nu = C.nu[a], nv = C.nv[a];
        const unsigned long long cells = (unsigned long long)(ls_cell(e[1], s, nu) - ls_cell(e[0], s, nu) + 1u) * (ls_cell(e[3], s, nv) - ls_cell(e[2], s, nv) + 1u);
        atomicAdd(&sums[a], cells);
    }
}

// Entries per cell under the chosen candidate, FILL = false; FILL = true: the triangle's index into the range `first` gives each cell it
// covers, at a place an atomic cursor hands out (k_ls_emit sorts the range, so the order of arrival does not show).
template <bool FILL>
__global__ __launch_bounds__(256) void k_ls_cells(const float* __restrict__ ebox, uint32_t n, float s, uint32_t nu, uint32_t nv, uint32_t* __restrict__ counts,
                                                  const uint32_t* __restrict__ first, uint32_t* __restrict__ idx, uint32_t n_idx) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    const float* e = ebox + 5ull * k;
    const uint32_t i0 = ls_cell(e[0], s, nu), i1 = ls_cell(e[1], s, nu), j0 = ls_cell(e[2], s, nv), j1 = ls_cell(e[3], s, nv);
    for (uint32_t j = j0; j <= j1 && j < nv; ++j)
        for (uint32_t i = i0; i <= i1 && i < nu; ++i) {
            const uint32_t cell = j * nu + i;
            const uint32_t at = atomicAdd(&counts[cell], 1u);
            if (FILL) { const uint32_t p = first[cell] + at; if (p < n_idx) idx[p] = k; }
        }
}

__global__ __launch_bounds__(256) void k_ls_max(const uint32_t* __restrict__ counts, uint32_t n_cells, uint32_t* __restrict__ out) {
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c < n_cells && counts[c] > 0u) atomicMax(out, counts[c]);
}

// One wave per cell: its at most kLsGridMaxCell indices ranked by (w_max descending, list index ascending) - the host's stable sort of
// an ascending list - then the cell word {first, box, count, 0}, the five floats per entry and the bitwise copies of the records.
__global__ __launch_bounds__(256) void k_ls_emit(const float* __restrict__ ebox, const double* __restrict__ tris, uint32_t n, const uint32_t* __restrict__ idx,
                                                 const uint32_t* __restrict__ counts, const uint32_t* __restrict__ first, uint32_t n_cells, uint32_t n_entries,
                                                 uint32_t* __restrict__ ls_nodes, uint32_t at, double* __restrict__ ls_tris, uint32_t tri_at) {
    __shared__ uint32_t s_idx[4][kLsGridMaxCell];
    __shared__ float s_w[4][kLsGridMaxCell];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t cell = blockIdx.x * 4u + wave;
    const bool live = cell < n_cells;                               // (every wave reaches the barrier)
    const uint32_t f0 = live ? first[cell] : 0u;
    uint32_t cnt = live ? counts[cell] : 0u;
    if (cnt > kLsGridMaxCell) cnt = kLsGridMaxCell;                 // (the host has refused such a grid already)
    if ((uint64_t)f0 + cnt > n_entries) cnt = 0u;
    const uint32_t box0 = at + 4u * n_cells;
    if (live && lane == 0u) { uint32_t* W = ls_nodes + at + 4ull * cell; W[0] = tri_at + f0; W[1] = box0 + 5u * f0; W[2] = cnt; W[3] = 0u; }
    for (uint32_t k = lane; k < cnt; k += 64u) {
        uint32_t t = idx[f0 + k];
        if (t >= n) t = 0u;
        s_idx[wave][k] = t; s_w[wave][k] = ebox[5ull * t + 4];
    }
    __syncthreads();
    for (uint32_t k = lane; k < cnt; k += 64u) {
        const uint32_t t = s_idx[wave][k]; const float w = s_w[wave][k];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < cnt; ++j) { const float wj = s_w[wave][j]; rank += (wj > w || (wj == w && s_idx[wave][j] < t)) ? 1u : 0u; }
        const uint32_t e = f0 + rank;
        for (int q = 0; q < 5; ++q) ls_nodes[box0 + 5ull * e + q] = __float_as_uint(ebox[5ull * t + q]);
        for (int q = 0; q < 9; ++q) ls_tris[9ull * (tri_at + e) + q] = tris[9ull * t + q];
    }
}

// ---- the edge records of a pair's grid (ft_edges.h; option "edge_cull") --------------------------------------------------------------
// One wave per cell, one lane per entry: the entry's record in ls_tris projected as grow_by_tri projects it, and the record of its three
// edges in (u, v).  E, the inflation the entry's rectangle carries: how far the five-float box the builder wrote beside the entry lies
// outside the projected vertices - the builder's pad and its outward rounding, read off the box itself, so it is the grid's own whoever
// built it (build_grid on the host, k_ls_emit here).  Every index is checked against the arrays' sizes: a cell table that says otherwise
// writes nothing.
__global__ __launch_bounds__(256) void k_ls_edges(const double* __restrict__ pair, const uint32_t* __restrict__ nodes, uint32_t node_words,
                                                  const double* __restrict__ tris, uint32_t n_recs, uint32_t n_cells, float* __restrict__ edges) {
    const uint32_t cell = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (cell >= n_cells) return;
    const uint32_t cells = reinterpret_cast<const uint32_t*>(pair + 14)[1];
    if ((uint64_t)cells + 4ull * cell + 4ull > node_words) return;
    const uint32_t* W = nodes + cells + 4ull * cell;
    const uint32_t first = W[0], box = W[1];
    uint32_t cnt = W[2];
    if (cnt > kLsGridMaxCell) cnt = kLsGridMaxCell;
    if ((uint64_t)first + cnt > n_recs || (uint64_t)box + 5ull * cnt > node_words) return;
    LsFrame F;
    for (int q = 0; q < 3; ++q) { F.U[q] = pair[q]; F.V[q] = pair[3 + q]; F.D[q] = pair[6 + q]; F.c[q] = pair[9 + q]; }
    F.pad = 0.0;
    for (uint32_t e = lane; e < cnt; e += 64u) {
        const double* T = tris + 9ull * (first + e);
        double x[3], y[3];
        for (int v = 0; v < 3; ++v) {
            double p[3];
            for (int q = 0; q < 3; ++q) p[q] = __dadd_rn(__dsub_rn(T[q], F.c[q]), v == 1 ? T[3 + q] : v == 2 ? T[6 + q] : 0.0);
            x[v] = dot_lr(p, F.U); y[v] = dot_lr(p, F.V);
        }
        const float* B = reinterpret_cast<const float*>(nodes + box + 5ull * e);
        const double xl = fmin(x[0], fmin(x[1], x[2])), xh = fmax(x[0], fmax(x[1], x[2])), yl = fmin(y[0], fmin(y[1], y[2])), yh = fmax(y[0], fmax(y[1], y[2]));
        const double E = fmax(fmax(xl - (double)B[0], (double)B[1] - xh), fmax(yl - (double)B[2], (double)B[3] - yh));
        const bool bounded = fabs((double)B[0]) + fabs((double)B[1]) + fabs((double)B[2]) + fabs((double)B[3]) < 3e38;
        float rec[kEdgeFloats];
        edge_record(x, y, E, bounded, rec);
        for (uint32_t q = 0; q < kEdgeFloats; ++q) edges[(size_t)kEdgeFloats * (first + e) + q] = rec[q];
    }
}

} // namespace

void ls_edge_records(hipStream_t stream, const double* pair, const uint32_t* ls_nodes, uint32_t node_words, const double* ls_tris, uint32_t n_recs, uint32_t n_cells, float* edges) {
    if (n_cells == 0u) return;
    hipLaunchKernelGGL(k_ls_edges, dim3((n_cells + 3u) / 4u), dim3(256), 0, stream, pair, ls_nodes, node_words, ls_tris, n_recs, n_cells, edges);
}

void ls_grid_entries(hipStream_t stream, const double* tris, uint32_t n, const LsFrame& F, float* ebox, uint32_t* ruv) {
    hipLaunchKernelGGL(k_ls_entries, dim3((n + 255u) / 256u), dim3(256), 0, stream, tris, n, F, ebox, ruv);
}
void ls_grid_count(hipStream_t stream, const float* ebox, uint32_t n, const LsGridCandidates& C, unsigned long long* sums) {
    hipLaunchKernelGGL(k_ls_count, dim3((n + 255u) / 256u), dim3(256), 0, stream, ebox, n, C, sums);
}
void ls_grid_cell_counts(hipStream_t stream, const float* ebox, uint32_t n, float s, uint32_t nu, uint32_t nv, uint32_t* counts, uint32_t* max_count) {
    hipLaunchKernelGGL(k_ls_cells<false>, dim3((n + 255u) / 256u), dim3(256), 0, stream, ebox, n, s, nu, nv, counts, (const uint32_t*)nullptr, (uint32_t*)nullptr, 0u);
    if (max_count) hipLaunchKernelGGL(k_ls_max, dim3((nu * nv + 255u) / 256u), dim3(256), 0, stream, counts, nu * nv, max_count);
}
hipError_t ls_grid_scan(hipStream_t stream, const uint32_t* counts, uint32_t* first, uint32_t n_cells, void* tmp, size_t* tmp_bytes) {
    return rocprim::exclusive_scan(tmp, *tmp_bytes, counts, first, 0u, (size_t)n_cells, rocprim::plus<uint32_t>(), stream);
}
void ls_grid_emit(hipStream_t stream, const float* ebox, const double* tris, uint32_t n, float s, uint32_t nu, uint32_t nv, const uint32_t* counts, const uint32_t* first,
                  uint32_t* cursor, uint32_t* idx, uint32_t n_entries, uint32_t* ls_nodes, uint32_t at, double* ls_tris, uint32_t tri_at) {
    hipLaunchKernelGGL(k_ls_cells<true>, dim3((n + 255u) / 256u), dim3(256), 0, stream, ebox, n, s, nu, nv, cursor, first, idx, n_entries);
    hipLaunchKernelGGL(k_ls_emit, dim3((nu * nv + 3u) / 4u), dim3(256), 0, stream, ebox, tris, n, idx, counts, first, nu * nv, n_entries, ls_nodes, at, ls_tris, tri_at);
}

void ls_morton_keys(hipStream_t stream, const double* tris, uint32_t n_tris, uint32_t first_tri, uint32_t n, const LsFrame& F, double R, uint32_t* keys, uint32_t* vals) {
    if (n == 0u) return;
    hipLaunchKernelGGL(k_ls_keys, dim3((n + 255u) / 256u), dim3(256), 0, stream, tris, n_tris, first_tri, n, F, R, 32768.0 / R, keys, vals);
}
hipError_t ls_sort_pairs(hipStream_t stream, const uint32_t* keys_in, uint32_t* keys_out, const uint32_t* vals_in, uint32_t* vals_out, uint32_t n, void* tmp, size_t* tmp_bytes) {
    return rocprim::radix_sort_pairs(tmp, *tmp_bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0u, 32u, stream);
}

void ls_gather(hipStream_t stream, const double* tris, uint32_t n_tris, uint32_t mesh_first, uint32_t mesh_n, const uint32_t* src, uint32_t count, double* ls_tris, uint32_t n_ls,
               uint32_t ls_first) {
    if (count == 0u) return;
    hipLaunchKernelGGL(k_ls_gather, dim3((count + 255u) / 256u), dim3(256), 0, stream, tris, n_tris, mesh_first, mesh_n, src, count, ls_tris, n_ls, ls_first);
}

void ls_refit_level(hipStream_t stream, uint32_t* nodes, uint32_t n_nodes, const double* tris, uint32_t n_tris, const uint32_t* order, uint32_t count, const LsFrame& F) {
    if (count == 0u) return;
    hipLaunchKernelGGL(k_ls_refit, dim3((count + 255u) / 256u), dim3(256), 0, stream, nodes, n_nodes, tris, n_tris, order, count, F);
}

} // namespace ftk

// ft_ls_topology.h — the topology of a light-space shadow tree rebuilt on the device (option "light_space_retree"), and
// where such trees lie behind the full commit's arrays.  Host code, header only: ft_capi.cpp lays the blocks out and uploads the child
// words, ft_debug.cpp hands the generator to the tests, tools/retree_host_check.cpp runs it under the sanitizers.
//
// The device sorts a pair's n triangles along a Morton curve of their projected centres (ft_lightspace.hip, k_ls_keys); the tree over the
// sorted positions is then a function of n alone: a binary tree over [lo, hi), a leaf where hi - lo <= 4, cut at mid = (lo + hi) / 2
// otherwise, two binary levels per 4-wide node exactly as LsBuilder::widen collapses them (ft_scene.cpp) - slots 0 and 1 the left half's
// children, 2 and 3 the right half's; a half that is a leaf takes the first slot of its half, the other stays INT32_MIN under an all-NaN
// box.  A leaf child is ~((ls_first + lo) << 3 | (hi - lo)).  Nodes are numbered breadth first, left to right, from first_node on.
//
// N(n), the number of 4-wide nodes.  The cuts give the binary node at depth d sizes floor(n / 2^d) or that plus one, n mod 2^d of them
// the larger; a 4-wide node stands at every even depth where the binary node holds more than 4 positions.  So, with q = n >> d and
// r = n & (2^d - 1),  N(n) = sum over even d of (q > 4 ? 2^d : q == 4 ? r : 0)  for n >= 5.
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

namespace fth {

constexpr uint32_t kLsTopoNodeWords = 24;                           // ftd::kLsNodeWords: 4 x 5 box floats, 4 child words
constexpr uint32_t kLsTopoLeaf = 4;                                 // LsBuilder::kLeafTris
constexpr uint32_t kLsTopoNaN = 0x7FC00000u;                        // the quiet NaN the host builder gives an empty slot's box

inline uint64_t ls_retree_node_count(uint64_t n) {
    if (n <= kLsTopoLeaf) return 0;
    uint64_t total = 0;
    for (unsigned d = 0; d < 64 && (n >> d) >= kLsTopoLeaf; d += 2) {
        const uint64_t q = n >> d, r = n & ((1ull << d) - 1);
        total += q > kLsTopoLeaf ? 1ull << d : r;
    }
    return total;
}

struct LsTopology {
    std::vector<uint32_t> nodes;                                    // N x 24 words: NaN boxes (k_ls_refit writes those of the slots in use), the child words
    std::vector<uint32_t> order;                                    // the nodes by level, deepest level first
    std::vector<std::pair<uint32_t, uint32_t>> levels;              // per level, deepest first: offset into `order` and count
};

// False (and nothing generated) where n < 5 - the root would be a leaf - or a leaf word or a node index would not fit its 28 / 31 bits.
inline bool ls_retree_topology(uint32_t n, uint32_t ls_first, uint32_t first_node, LsTopology& out) {
    out.nodes.clear(); out.order.clear(); out.levels.clear();
    const uint64_t N = ls_retree_node_count(n);
    if (n <= kLsTopoLeaf || (uint64_t)ls_first + n >= (1ull << 28) || (uint64_t)first_node + N >= (1ull << 31)) return false;
    struct Range { uint32_t lo, hi, level; };
    std::vector<Range> q;                                           // the 4-wide nodes in breadth-first order: node first_node + k covers q[k]
    q.reserve((size_t)N);
    q.push_back({0u, n, 0u});
    out.nodes.assign((size_t)N * kLsTopoNodeWords, kLsTopoNaN);
    for (size_t k = 0; k < q.size(); ++k) {
        const Range r = q[k];
        uint32_t* child = &out.nodes[k * kLsTopoNodeWords + 20];
        for (int c = 0; c < 4; ++c) child[c] = 0x80000000u;         // INT32_MIN: an empty slot
        const uint32_t mid = r.lo + (r.hi - r.lo) / 2;
        const uint32_t half[2][2] = {{r.lo, mid}, {mid, r.hi}};
        for (int h = 0; h < 2; ++h) {
            const uint32_t lo = half[h][0], hi = half[h][1];
            uint32_t kid[2][2] = {{lo, hi}, {0u, 0u}};
            int kids = 1;
            if (hi - lo > kLsTopoLeaf) { const uint32_t m = lo + (hi - lo) / 2; kid[0][1] = m; kid[1][0] = m; kid[1][1] = hi; kids = 2; }
            for (int s = 0; s < kids; ++s) {
                const uint32_t a = kid[s][0], b = kid[s][1];
                if (b - a <= kLsTopoLeaf) { child[2 * h + s] = ~((ls_first + a) << 3 | (b - a)); continue; }
                child[2 * h + s] = first_node + (uint32_t)q.size();
                q.push_back({a, b, r.level + 1u});
            }
        }
    }
    // breadth first: a level is a run of q; the runs laid out deepest first
    const uint32_t depth = q.back().level + 1u;
    std::vector<std::pair<uint32_t, uint32_t>> run(depth, {0u, 0u});   // first position in q, count
    for (size_t k = 0; k < q.size(); ++k) { if (run[q[k].level].second++ == 0u) run[q[k].level].first = (uint32_t)k; }
    for (uint32_t d = depth; d-- > 0;) {
        out.levels.push_back({(uint32_t)out.order.size(), run[d].second});
        for (uint32_t k = 0; k < run[d].second; ++k) out.order.push_back(first_node + run[d].first + k);
    }
    return q.size() == N;
}

// Where the blocks lie: one of N(n_tris) nodes per pair, in table order, from node `first_node` on, while the bytes stay within `cap`
// (`bytes`: what the arrays hold already).  block[k] = the first node of pair k's block, or ~0u where it does not fit (or the pair has no
// run of leaf records to sort: n = 0).  Returns the nodes the blocks take together.
inline uint64_t ls_retree_layout(const std::vector<uint32_t>& n_tris, uint64_t first_node, uint64_t bytes, uint64_t cap, std::vector<uint32_t>& block) {
    block.assign(n_tris.size(), ~0u);
    uint64_t at = first_node;
    for (size_t k = 0; k < n_tris.size(); ++k) {
        const uint64_t N = ls_retree_node_count(n_tris[k]);
        if (N == 0 || bytes + N * kLsTopoNodeWords * 4 > cap || at + N >= (1ull << 31)) continue;
        block[k] = (uint32_t)at;
        at += N; bytes += N * kLsTopoNodeWords * 4;
    }
    return at - first_node;
}

} // namespace fth

// retree_host_check.cpp — the host half of "light_space_retree" (functracer_amd/csrc/ft_ls_topology.h) under
// AddressSanitizer + UBSan, as a stand-alone program (CPU only, no device object).  For n = 5 .. 4100 and n = 2^20 it generates the
// topology and checks that
//   - every sorted position lies in exactly one leaf, and every leaf holds 2 .. 4 of them;
//   - slot 0 of a node is never empty, an empty slot comes second in its half, and every child node lies inside the block;
//   - the levels partition the nodes, every child node lies in a deeper level than its parent (so an earlier launch of the refit), there are at most 9 of
//     them and the walk never holds more than 27 pending entries;
//   - N(n) is the closed form the header documents, and n < 5 is refused;
// and, since no test can afford to fill 256 MiB on the device, the layout arithmetic under a lowered cap: blocks are given out in table order while the bytes
// fit, a pair whose block does not fit gets none while a later, smaller one still may, blocks never overlap, and the total is what the grids are laid behind.
// Build and run from the repository root:
//   g++ -fsanitize=address,undefined -fno-omit-frame-pointer -g -O1 -std=c++17 -ffp-contract=off tools/retree_host_check.cpp \
//       -o build/retree_host_check && build/retree_host_check
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../functracer_amd/csrc/ft_ls_topology.h"

#define CHECK(x) do { if (!(x)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #x); std::exit(1); } } while (0)

// N(n) by the definition itself: the 4-wide nodes of the collapsed binary tree over [lo, hi).
static uint64_t count_by_recursion(uint64_t lo, uint64_t hi) {
    if (hi - lo <= 4) return 0;
    const uint64_t mid = lo + (hi - lo) / 2;
    uint64_t total = 1;
    const uint64_t half[2][2] = {{lo, mid}, {mid, hi}};
    for (const auto& h : half) {
        if (h[1] - h[0] <= 4) continue;
        const uint64_t m = h[0] + (h[1] - h[0]) / 2;
        total += count_by_recursion(h[0], m) + count_by_recursion(m, h[1]);
    }
    return total;
}

static void check_topology(uint32_t n, uint32_t ls_first, uint32_t first_node) {
    fth::LsTopology t;
    CHECK(fth::ls_retree_topology(n, ls_first, first_node, t));
    const size_t N = t.nodes.size() / fth::kLsTopoNodeWords;
    CHECK(N == fth::ls_retree_node_count(n) && N == count_by_recursion(0, n));
    std::vector<uint8_t> covered(n, 0);
    std::vector<int32_t> level_of(N, -1);
    CHECK(t.order.size() == N && !t.levels.empty() && t.levels.size() <= 9);
    size_t at = 0;
    for (size_t l = 0; l < t.levels.size(); ++l) {                  // deepest first: level index counts up towards the root
        CHECK(t.levels[l].first == at && t.levels[l].second > 0);
        for (uint32_t k = 0; k < t.levels[l].second; ++k, ++at) {
            const uint32_t node = t.order[at];
            CHECK(node >= first_node && node - first_node < N && level_of[node - first_node] < 0);
            level_of[node - first_node] = (int32_t)l;
        }
    }
    CHECK(at == N && t.order[N - 1] == first_node);                 // the root is the block's first node and is boxed last
    for (size_t k = 0; k < N; ++k) {
        const uint32_t* w = &t.nodes[k * fth::kLsTopoNodeWords];
        for (int q = 0; q < 20; ++q) CHECK(w[q] == fth::kLsTopoNaN);
        CHECK((int32_t)w[20] != INT32_MIN && (int32_t)w[22] != INT32_MIN);   // the first slot of each half
        for (int c = 0; c < 4; ++c) {
            const int32_t ch = (int32_t)w[20 + c];
            if (ch == INT32_MIN) continue;
            if (ch >= 0) {
                CHECK((uint32_t)ch > first_node + k && (uint32_t)ch - first_node < N);
                CHECK(level_of[(uint32_t)ch - first_node] < level_of[k]);
                continue;
            }
            const uint32_t first = (uint32_t)~ch >> 3, cnt = (uint32_t)~ch & 7u;
            CHECK(cnt >= 2 && cnt <= 4 && first >= ls_first && first - ls_first + cnt <= n);
            for (uint32_t i = 0; i < cnt; ++i) { CHECK(!covered[first - ls_first + i]); covered[first - ls_first + i] = 1; }
        }
    }
    CHECK(std::count(covered.begin(), covered.end(), 1) == (long)n);
    // ls_tree_walk: slots 3, 2, 1 pushed where in use, slot 0 taken directly
    size_t worst = 0;
    std::vector<std::pair<uint32_t, size_t>> todo{{first_node, 0}};
    while (!todo.empty()) {
        const auto [node, sp] = todo.back();
        todo.pop_back();
        const uint32_t* w = &t.nodes[(size_t)(node - first_node) * fth::kLsTopoNodeWords + 20];
        int32_t pushed[3]; size_t np = 0;
        for (int c = 3; c >= 1; --c) if ((int32_t)w[c] != INT32_MIN) pushed[np++] = (int32_t)w[c];
        worst = std::max(worst, sp + np);
        if ((int32_t)w[0] >= 0) todo.push_back({w[0], sp + np});
        for (size_t k = 0; k < np; ++k) if (pushed[np - 1 - k] >= 0) todo.push_back({(uint32_t)pushed[np - 1 - k], sp + np - 1 - k});
    }
    CHECK(worst <= 27);
}

int main() {
    fth::LsTopology t;
    for (uint32_t n = 0; n < 5; ++n) { CHECK(!fth::ls_retree_topology(n, 0, 0, t) && fth::ls_retree_node_count(n) == 0); }
    CHECK(!fth::ls_retree_topology(8, (1u << 28) - 4, 0, t));       // a leaf word that would not fit
    CHECK(!fth::ls_retree_topology(8, 0, 0x7FFFFFFFu, t));          // a node index that would not fit
    for (uint32_t n = 5; n <= 4100; ++n) check_topology(n, n % 3 ? 17u * n : 0u, n % 2 ? 1000u + n : 0u);
    check_topology(1u << 20, 12345u, 678u);
    check_topology((1u << 20) - 1, 0u, 0u);

    // the layout: blocks in table order against a cap
    const uint64_t node_bytes = fth::kLsTopoNodeWords * 4;
    std::vector<uint32_t> n_tris{980, 0, 65, 4097, 8, 257};
    std::vector<uint32_t> block;
    uint64_t all = 0;
    for (uint32_t n : n_tris) all += fth::ls_retree_node_count(n);
    // no cap in the way: consecutive blocks in table order, none for the pair without a run of records
    CHECK(fth::ls_retree_layout(n_tris, 100, 5000, ~0ull, block) == all && block.size() == n_tris.size());
    uint64_t at = 100;
    for (size_t k = 0; k < n_tris.size(); ++k) {
        if (n_tris[k] == 0) { CHECK(block[k] == ~0u); continue; }
        CHECK(block[k] == at);
        at += fth::ls_retree_node_count(n_tris[k]);
    }
    // a cap that the fourth pair's block passes: it gets none, for good; the smaller ones behind it still fit, right behind the third's
    const uint64_t three = fth::ls_retree_node_count(980) + fth::ls_retree_node_count(65);
    const uint64_t small = fth::ls_retree_node_count(8) + fth::ls_retree_node_count(257);
    const uint64_t cap = 5000 + (three + small) * node_bytes + node_bytes / 2;
    CHECK(fth::ls_retree_node_count(4097) > small + 1);
    CHECK(fth::ls_retree_layout(n_tris, 100, 5000, cap, block) == three + small);
    CHECK(block[0] == 100 && block[1] == ~0u && block[2] == 100 + fth::ls_retree_node_count(980) && block[3] == ~0u);
    CHECK(block[4] == 100 + three && block[5] == block[4] + fth::ls_retree_node_count(8));
    // exactly at the cap fits, one byte less does not; nothing fits: nothing laid out
    CHECK(fth::ls_retree_layout({980}, 0, 0, fth::ls_retree_node_count(980) * node_bytes, block) == fth::ls_retree_node_count(980) && block[0] == 0);
    CHECK(fth::ls_retree_layout({980}, 0, 1, fth::ls_retree_node_count(980) * node_bytes, block) == 0 && block[0] == ~0u);
    CHECK(fth::ls_retree_layout(n_tris, 100, 5000, 5000, block) == 0);
    for (uint32_t b : block) CHECK(b == ~0u);
    std::printf("retree_host_check: ok (n = 5 .. 4100, 2^20 - 1, 2^20; N(980) = %llu, N(2^20) = %llu)\n", (unsigned long long)fth::ls_retree_node_count(980),
                (unsigned long long)fth::ls_retree_node_count(1u << 20));
    return 0;
}

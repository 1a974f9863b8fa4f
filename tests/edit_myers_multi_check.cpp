// edit_myers_multi_check.cpp -- csrc/edit_myers_multi.hpp held to the plain two-row DP on the CPU: a stand-alone program that
// tests/test_edit_long_cpu.py compiles with the host compiler under -fsanitize=address,undefined and runs.
//
// Random pairs over alphabets of 1 to 5 tokens that differ only above bit 32 (a 32-bit compare sees one token); half of the lengths
// come from the word edges {1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 448, 511, 512}; a third of the equal-length pairs are
// identical.  Every W that csrc/edit_long.hip instantiates (1, 2, 3, 4, 6, 8) runs, each pair through the smallest that fits -- and,
// as the kernel may, through every larger one too, whose words above the query's last one hold all-zero masks.
// Prints "pairs=N bad=B"; exit status 1 where B > 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "edit_myers_multi.hpp"

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd() {                                      // xorshift64*
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}
static int below(int n) { return (int)(rnd() % (uint64_t)n); }

static int two_row(const std::vector<int64_t>& a, const std::vector<int64_t>& b) {
    const size_t m = a.size(), n = b.size();
    std::vector<int> prev(m + 1), cur(m + 1);
    for (size_t i = 0; i <= m; ++i) prev[i] = (int)i;
    for (size_t t = 1; t <= n; ++t) {
        cur[0] = (int)t;
        for (size_t i = 1; i <= m; ++i) cur[i] = std::min(std::min(prev[i] + 1, cur[i - 1] + 1), prev[i - 1] + (a[i - 1] == b[t - 1] ? 0 : 1));
        prev.swap(cur);
    }
    return prev[m];
}

template <int W>
static int multi(const std::vector<int64_t>& q, const std::vector<int64_t>& r) {
    const int m = (int)q.size();
    const int lw = (m - 1) >> 6;
    const uint64_t top = (uint64_t)1 << ((m - 1) & 63);
    slnlp::MyersMultiState<W> s;
    slnlp::myers_multi_begin(s, m);
    for (size_t t = 0; t < r.size(); ++t) {
        uint64_t Eq[W];
        for (int w = 0; w < W; ++w) Eq[w] = 0;
        for (int j = 0; j < m; ++j) {
            if (q[j] == r[t]) Eq[j >> 6] |= (uint64_t)1 << (j & 63);
        }
        slnlp::myers_multi_step(s, Eq, lw, top);
    }
    return s.score;
}

// through the smallest instantiated W that fits (first) and every larger one: the number of wrong answers
static int wrong(const std::vector<int64_t>& q, const std::vector<int64_t>& r, int want) {
    const int words = (((int)q.size() - 1) >> 6) + 1;
    int bad = 0;
    if (words <= 1) bad += multi<1>(q, r) != want;
    if (words <= 2) bad += multi<2>(q, r) != want;
    if (words <= 3) bad += multi<3>(q, r) != want;
    if (words <= 4) bad += multi<4>(q, r) != want;
    if (words <= 6) bad += multi<6>(q, r) != want;
    bad += multi<8>(q, r) != want;
    return bad;
}

int main(int argc, char** argv) {
    const int pairs = argc > 1 ? atoi(argv[1]) : 3000;
    static const int edges[] = {1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 448, 511, 512};
    const int n_edges = (int)(sizeof(edges) / sizeof(edges[0]));
    auto length = [&]() { return below(2) ? edges[below(n_edges)] : 1 + below(512); };
    int bad = 0, same = 0;
    for (int p = 0; p < pairs; ++p) {
        const int alphabet = 1 + below(5);
        auto token = [&]() { return ((int64_t)(1 + below(alphabet)) << 33) | 7; };
        int m = length(), n = p % 4 == 0 ? m : length();
        if (p % 8 == 1) n = below(3);                        // short and empty references
        std::vector<int64_t> q(m), r(n);
        for (auto& c : q) c = token();
        for (auto& c : r) c = token();
        if (m == n && below(3) == 0) { r = q; ++same; }
        const int want = two_row(q, r);
        const int b = wrong(q, r, want);
        if (b && bad < 5) fprintf(stderr, "pair %d: m=%d n=%d alphabet=%d: the DP says %d, %d instantiations disagree\n", p, m, n, alphabet, want, b);
        bad += b ? 1 : 0;
    }
    printf("pairs=%d identical=%d bad=%d\n", pairs, same, bad);
    return bad ? 1 : 0;
}

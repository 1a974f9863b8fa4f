// A CPU build of csrc/edit_myers.hpp held to the plain two-row dynamic program (tests/test_edit_knn_cpu.py compiles and runs it):
// random pairs over small alphabets whose tokens differ only above bit 32, a quarter of the lengths at 63 or 64 -- the top bit of the
// word -- and a third of the equal-length pairs identical.  Prints "<pairs> pairs, <bad> bad"; exit status 1 when any differs.
#include "../sign-language-nlp_amd/csrc/edit_myers.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

using slnlp::MyersState;

static int plain(const std::vector<int64_t>& a, const std::vector<int64_t>& b) {
    std::vector<int> prev(b.size() + 1), cur(b.size() + 1);
    for (size_t j = 0; j <= b.size(); ++j) prev[j] = (int)j;
    for (size_t i = 1; i <= a.size(); ++i) {
        cur[0] = (int)i;
        for (size_t j = 1; j <= b.size(); ++j) cur[j] = std::min({prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1] ? 1 : 0)});
        std::swap(prev, cur);
    }
    return prev[b.size()];
}

static int myers(const std::vector<int64_t>& q, const std::vector<int64_t>& r) {
    const int m = (int)q.size();
    if (m == 0) return (int)r.size();
    MyersState s = slnlp::myers_begin(m);
    const uint64_t top = (uint64_t)1 << (m - 1);
    for (int64_t c : r) {
        uint64_t Eq = 0;
        for (int j = 0; j < m; ++j) Eq |= (uint64_t)(q[j] == c ? 1 : 0) << j;
        slnlp::myers_step(s, Eq, top);
    }
    return s.score;
}

int main(int argc, char** argv) {
    const long pairs = argc > 1 ? atol(argv[1]) : 20000;
    srand(1);
    long bad = 0;
    for (long it = 0; it < pairs; ++it) {
        const int A = 1 + rand() % 5;
        const int m = rand() % 4 == 0 ? 64 - rand() % 2 : rand() % 65, l = rand() % 4 == 0 ? 64 - rand() % 2 : rand() % 65;
        std::vector<int64_t> q(m), r(l);
        for (auto& x : q) x = ((int64_t)(1 + rand() % A) << 33) + 7;
        for (auto& x : r) x = ((int64_t)(1 + rand() % A) << 33) + 7;
        if (m == l && rand() % 3 == 0) r = q;
        const int want = plain(q, r), got = myers(q, r);
        if (want != got) {
            if (bad < 5) printf("m=%d l=%d: %d, the plain program gives %d\n", m, l, got, want);
            ++bad;
        }
    }
    printf("%ld pairs, %ld bad\n", pairs, bad);
    return bad != 0;
}

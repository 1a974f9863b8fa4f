// A CPU build of the WEIGHTED column step of csrc/field_edit.hpp -- field_weigh over the zero-padded code vectors, a token outside
// the table at W, the gap in 1..W -- held to the plain two-row dynamic program (tests/test_field_weights_cpu.py compiles and runs
// it, once plain and once with -fsanitize=address,undefined): random pairs with a quarter of the lengths at 63 or 64, F in
// {1, 4, 5, 6, 13, 16}, weights that include zeros and, in a third of the cases, a single 16 on one field; code tables over two
// values per field and tokens outside the table as in field_edit_check.cpp.  Prints "<pairs> pairs, <bad> bad"; exit status 1
// when any differs.
#include "../sign-language-nlp_amd/csrc/field_edit.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct Table {
    int F, Vt, W;
    std::vector<int> codes;                 // [Vt, F]
    std::vector<int> w;                     // [F]
};

static int sub(const Table& T, int64_t a, int64_t b) {
    if (a == b) return 0;
    if (a < 0 || a >= T.Vt || b < 0 || b >= T.Vt) return T.W;
    int n = 0;
    for (int f = 0; f < T.F; ++f) n += T.codes[a * T.F + f] != T.codes[b * T.F + f] ? T.w[f] : 0;
    return n;
}

static int plain(const Table& T, int gap, const std::vector<int64_t>& a, const std::vector<int64_t>& b) {
    std::vector<int> prev(b.size() + 1), cur(b.size() + 1);
    for (size_t j = 0; j <= b.size(); ++j) prev[j] = (int)j * gap;
    for (size_t i = 1; i <= a.size(); ++i) {
        cur[0] = (int)i * gap;
        for (size_t j = 1; j <= b.size(); ++j) cur[j] = std::min({prev[j] + gap, cur[j - 1] + gap, prev[j - 1] + sub(T, a[i - 1], b[j - 1])});
        std::swap(prev, cur);
    }
    return prev[b.size()];
}

struct Column {
    unsigned w[slnlp::FIELD_WORDS];
    unsigned load(int p) const { return w[p]; }
    void store(int p, unsigned v) { w[p] = v; }
};

// as the weighted kernel: the query's tokens, flags and zero-padded code vectors first, the weights padded with zeros to 16,
// then one column step per reference token
static int header(const Table& T, int gap, const std::vector<int64_t>& q, const std::vector<int64_t>& r) {
    const int m = (int)q.size(), words = (m + 1) >> 1, groups = (T.F + 3) >> 2;
    slnlp::FieldWeights fw = {};
    for (int f = 0; f < T.F; ++f) fw.w[f] = T.w[f];
    int64_t qtok[64] = {0};
    int qout[64], qcode[64][slnlp::FIELD_MAX] = {{0}};
    for (int j = 0; j < 64; ++j) {
        const int64_t c = j < m ? q[j] : 0;
        qtok[j] = c;
        qout[j] = (c >= 0 && c < T.Vt) ? 0 : 1;
        if (j < m && !qout[j])
            for (int f = 0; f < T.F; ++f) qcode[j][f] = T.codes[c * T.F + f];
    }
    Column col;
    slnlp::field_column_begin(col, words, gap);
    int t = 0;
    for (int64_t c : r) {
        const bool inside = c >= 0 && c < T.Vt;
        int rc[slnlp::FIELD_MAX] = {0};
        if (inside)
            for (int f = 0; f < T.F; ++f) rc[f] = T.codes[c * T.F + f];
        slnlp::field_column_step(col, words, ++t, gap, [&](int p) {
            return slnlp::field_sub(qtok[p] == c, (qout[p] != 0) | !inside, slnlp::field_weigh(qcode[p], rc, fw, groups), T.W);
        });
    }
    return slnlp::field_column_score(col, m, (int)r.size(), gap);
}

int main(int argc, char** argv) {
    const long pairs = argc > 1 ? atol(argv[1]) : 20000;
    srand(2);
    long bad = 0, zeros = 0, sixteens = 0, long_rows = 0;
    const int Fs[6] = {1, 4, 5, 6, 13, 16};
    for (long it = 0; it < pairs; ++it) {
        Table T;
        T.F = Fs[rand() % 6];
        T.Vt = 2 + rand() % 7;
        T.codes.resize((size_t)T.Vt * T.F);
        const bool wide = rand() % 2 == 0;                       // codes[v] = v-like tables, or two values per field
        for (int v = 0; v < T.Vt; ++v)
            for (int f = 0; f < T.F; ++f) T.codes[v * T.F + f] = wide ? v - 3 : rand() % 2;
        T.w.assign(T.F, 0);
        if (rand() % 3 == 0) {                                   // a single 16, every other field at 0
            T.w[rand() % T.F] = 16;
            ++sixteens;
        } else {                                                 // W units dealt to random fields: zeros wherever none lands
            const int W = 1 + rand() % 16;
            for (int u = 0; u < W; ++u) ++T.w[rand() % T.F];
        }
        T.W = 0;
        for (int f = 0; f < T.F; ++f) {
            T.W += T.w[f];
            zeros += T.w[f] == 0 ? 1 : 0;
        }
        const int gap = rand() % 3 == 0 ? 1 : (rand() % 2 == 0 ? T.W : 1 + rand() % T.W);
        const int m = rand() % 4 == 0 ? 64 - rand() % 2 : rand() % 65, l = rand() % 4 == 0 ? 64 - rand() % 2 : rand() % 65;
        long_rows += (m >= 63 ? 1 : 0) + (l >= 63 ? 1 : 0);
        auto token = [&]() -> int64_t {
            const int kind = rand() % 8;
            if (kind == 0) return -(int64_t)(1 + rand() % 3);                       // negative: outside the table
            if (kind == 1) return ((int64_t)(1 + rand() % 3) << 33) + 7;            // equal in their low 32 bits, outside too
            return rand() % T.Vt;
        };
        std::vector<int64_t> q(m), r(l);
        for (auto& x : q) x = token();
        for (auto& x : r) x = token();
        if (m == l && rand() % 3 == 0) r = q;
        const int want = plain(T, gap, q, r), got = header(T, gap, q, r);
        if (want != got) {
            if (bad < 5) printf("F=%d W=%d gap=%d m=%d l=%d: %d, the plain program gives %d\n", T.F, T.W, gap, m, l, got, want);
            ++bad;
        }
    }
    if (zeros == 0 || sixteens == 0 || long_rows * 8 < pairs * 2 * 2) {          // what the cases were to hold: about a quarter long
        printf("the cases hold %ld zero weights, %ld single sixteens, %ld long rows\n", zeros, sixteens, long_rows);
        return 2;
    }
    printf("%ld pairs, %ld bad\n", pairs, bad);
    return bad != 0;
}

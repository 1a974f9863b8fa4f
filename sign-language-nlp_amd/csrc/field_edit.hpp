// field_edit.hpp -- the cost function and one column step of the phonology-weighted edit distance (include/slnlp.h states the
// definitions), host and device: field_knn.hip runs it per reference token, and a CPU build can hold the kernel's own arithmetic to
// the plain two-row program (tests/field_edit_check.cpp).
//
// A token is a composition of F fields (1..16); substituting one frame for another costs the number of fields in which their code
// vectors differ, inserting or deleting a frame costs gap (1..F).  The query (m <= 64 frames) runs down a column, a reference token
// is one column step:   cell[j] = min(old[j] + gap, cell[j - 1] + gap, old[j - 1] + sub(query[j - 1], token)),   cell[0] = t gap.
//
// THE COLUMN holds the positions 1 .. 64 as 32 words of two uint16 values -- word p: position 2p + 1 in the low half, 2p + 2 in the
// high half -- behind load(p) / store(p, w), so the kernel keeps it transposed in LDS ([word][thread]) and a host program in a plain
// array.  A step touches the (m + 1) / 2 words that hold a position <= m; with m odd the high half of the last word is a cell of
// position m + 1 that nothing reads (a cell depends on the positions j - 1 and j only).  Every value is at most 16 * 65 < 2^16.
//
// CODE VECTORS are padded with zeros to 16 entries on both sides, so they compare in whole groups of four: groups = (F + 3) / 4.
#pragma once
#include <stdint.h>

#ifndef SLNLP_HD
#if defined(__HIPCC__)
#define SLNLP_HD __host__ __device__ __forceinline__
#else
#define SLNLP_HD static inline
#endif
#endif

namespace slnlp {

constexpr int FIELD_MAX = 16;                // SLNLP_FIELD_MAX_FIELDS
constexpr int FIELD_WORDS = 32;              // of a column: the positions 1 .. 64, two a word

// the number of entries in which two padded code vectors differ, over the first G groups of four: G a compile-time constant (the
// kernel is built once per G, so a cell is straight-line code), or a run-time one
template <int G, class A, class B>
SLNLP_HD int field_differ_groups(const A& a, const B& b) {
    int n = 0;
#pragma unroll
    for (int e = 0; e < 4 * G; ++e) n += a[e] != b[e] ? 1 : 0;
    return n;
}
template <class A, class B>
SLNLP_HD int field_differ(const A& a, const B& b, int groups) {
    switch (groups) {
        case 1: return field_differ_groups<1>(a, b);
        case 2: return field_differ_groups<2>(a, b);
        case 3: return field_differ_groups<3>(a, b);
        default: return field_differ_groups<4>(a, b);
    }
}

// sub(a, b): 0 for the same int64 token; F when either lies outside the table; else the fields in which their codes differ (may be 0)
SLNLP_HD int field_sub(bool same, bool outside, int differ, int F) { return same ? 0 : (outside ? F : differ); }

// ------------------------------------------------------------------------------------------------ per-field weights ----
// The weighted metric (slnlp_field_distances_w): field f counts w[f] (0..16, their sum W in 1..16) instead of 1, a token outside
// the table costs W, gap lies in 1..W.  Sixteen ints, zeros behind F as the code vectors: the kernel takes the struct BY VALUE among
// its arguments, so the weights are uniform values in scalar registers and no table is read for them.
struct FieldWeights {
    int w[FIELD_MAX];
};

// the sum of w[e] over the entries in which two padded code vectors differ, over the first G groups of four
template <int G, class A, class B>
SLNLP_HD int field_weigh_groups(const A& a, const B& b, const FieldWeights& fw) {
    int n = 0;
#pragma unroll
    for (int e = 0; e < 4 * G; ++e) n += a[e] != b[e] ? fw.w[e] : 0;
    return n;
}
template <class A, class B>
SLNLP_HD int field_weigh(const A& a, const B& b, const FieldWeights& fw, int groups) {
    switch (groups) {
        case 1: return field_weigh_groups<1>(a, b, fw);
        case 2: return field_weigh_groups<2>(a, b, fw);
        case 3: return field_weigh_groups<3>(a, b, fw);
        default: return field_weigh_groups<4>(a, b, fw);
    }
}

SLNLP_HD int field_cell(int up, int left, int diag, int sub, int gap) {
    const int a = (up < left ? up : left) + gap, b = diag + sub;
    return a < b ? a : b;
}

// the column in front of the first reference token: position j holds j gap
template <class Col>
SLNLP_HD void field_column_begin(Col& col, int words, int gap) {
    for (int p = 0; p < words; ++p) col.store(p, (unsigned)((2 * p + 1) * gap) | ((unsigned)((2 * p + 2) * gap) << 16));
}

// reference token number t (1-based) against the query: sub(j) is its cost against the query's position j (0-based; asked for
// j <= 2 words - 1 <= 63)
template <class Col, class Sub>
SLNLP_HD void field_column_step(Col& col, int words, int t, int gap, Sub&& sub) {
    int diag = (t - 1) * gap, left = t * gap;
    for (int p = 0; p < words; ++p) {
        const unsigned w = col.load(p);
        const int o1 = (int)(w & 0xffffu), o2 = (int)(w >> 16);
        const int n1 = field_cell(o1, left, diag, sub(2 * p), gap);
        const int n2 = field_cell(o2, n1, o1, sub(2 * p + 1), gap);
        col.store(p, (unsigned)n1 | ((unsigned)n2 << 16));
        diag = o2;
        left = n2;
    }
}

// d(query of m frames, the n reference tokens stepped so far)
template <class Col>
SLNLP_HD int field_column_score(Col& col, int m, int n, int gap) {
    if (m == 0) return n * gap;
    return (int)((col.load((m - 1) >> 1) >> (((m - 1) & 1) * 16)) & 0xffffu);
}

}  // namespace slnlp

// spans.hpp -- the argument checks the entry points share (host only): a named byte range, whether two of them overlap, the
// "no output aliases an input or another output" loop, and the checks of a float32 [N, ld] matrix of which V columns are used.
// The messages are part of the interface (the tests assert them): every entry point passes its own name.
#pragma once
#include <limits.h>

#include "common.hpp"

namespace slnlp {

struct Span {
    const void* p;      // null: an optional argument that is absent -- it overlaps nothing
    size_t bytes;
    const char* name;
};
static inline bool spans_overlap(const Span& a, const Span& b) {
    const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
    return a.p && b.p && a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

// every output against every input, and against the outputs before it.  An entry point that words its refusals differently
// loops over its Spans itself.
template <int NO, int NI>
static inline int check_no_overlap(const char* what, const Span (&out)[NO], const Span (&in)[NI]) {
    for (int o = 0; o < NO; ++o) {
        for (int i = 0; i < NI; ++i)
            SLNLP_CHECK_ARG(!spans_overlap(out[o], in[i]), "%s: output %s overlaps input %s", what, out[o].name, in[i].name);
        for (int q = 0; q < o; ++q)
            SLNLP_CHECK_ARG(!spans_overlap(out[o], out[q]), "%s: outputs %s and %s overlap", what, out[q].name, out[o].name);
    }
    return 0;
}

// the bytes from the first to the last used element of a [N, ld] matrix of 4-byte elements with V columns used
static inline size_t matrix_bytes(int64_t N, int64_t ld, int64_t V) { return ((size_t)(N - 1) * (size_t)ld + (size_t)V) * 4; }

// the log-prob matrix argument: N in 1..n_max, V in 1..v_max, ld >= V, ld N addressable; *span = its bytes, named "logp"
static inline int check_logp_matrix(const char* what, const float* logp, int64_t N, int64_t n_max, int64_t V, int64_t v_max, int64_t ld,
                                    Span* span) {
    SLNLP_CHECK_ARG(N >= 1 && N <= n_max, "%s: N=%ld outside 1..%ld", what, (long)N, (long)n_max);
    SLNLP_CHECK_ARG(V >= 1 && V <= v_max, "%s: V=%ld outside 1..%ld", what, (long)V, (long)v_max);
    SLNLP_CHECK_ARG(ld >= V, "%s: ld=%ld is less than V=%ld", what, (long)ld, (long)V);
    SLNLP_CHECK_ARG(ld <= INT64_MAX / 8 / N, "%s: ld=%ld times N=%ld is no addressable matrix", what, (long)ld, (long)N);
    *span = Span{logp, matrix_bytes(N, ld, V), "logp"};
    return 0;
}

}  // namespace slnlp

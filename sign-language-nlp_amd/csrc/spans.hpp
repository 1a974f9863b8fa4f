// spans.hpp -- the argument checks the entry points share (host only): a named byte range, whether two of them overlap, the
// "no output aliases an input or another output" loop, the checks of a float32 [N, ld] matrix of which V columns are used -- as
// an input, as an output, as an output that may be the input itself -- and the check of a fit's scratch buffer.
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

// N in 1..n_max, V in 1..v_max
static inline int check_logp_dims(const char* what, int64_t N, int64_t n_max, int64_t V, int64_t v_max) {
    SLNLP_CHECK_ARG(N >= 1 && N <= n_max, "%s: N=%ld outside 1..%ld", what, (long)N, (long)n_max);
    SLNLP_CHECK_ARG(V >= 1 && V <= v_max, "%s: V=%ld outside 1..%ld", what, (long)V, (long)v_max);
    return 0;
}

// the log-prob matrix argument: its dimensions, ld >= V, ld N addressable; *span = its bytes, named "logp"
static inline int check_logp_matrix(const char* what, const float* logp, int64_t N, int64_t n_max, int64_t V, int64_t v_max, int64_t ld,
                                    Span* span) {
    SLNLP_TRY(check_logp_dims(what, N, n_max, V, v_max));
    SLNLP_CHECK_ARG(ld >= V, "%s: ld=%ld is less than V=%ld", what, (long)ld, (long)V);
    SLNLP_CHECK_ARG(ld <= INT64_MAX / 8 / N, "%s: ld=%ld times N=%ld is no addressable matrix", what, (long)ld, (long)N);
    *span = Span{logp, matrix_bytes(N, ld, V), "logp"};
    return 0;
}

// the log-prob matrix an entry point writes, [N, ld_out] with V columns used (N >= 1, called n_name in the message): ld_out >= V,
// ld_out N addressable; *span = its bytes, named "out"
static inline int check_out_matrix(const char* what, const float* out, int64_t N, const char* n_name, int64_t V, int64_t ld_out, Span* span) {
    SLNLP_CHECK_ARG(ld_out >= V, "%s: ld_out=%ld is less than V=%ld", what, (long)ld_out, (long)V);
    SLNLP_CHECK_ARG(ld_out <= INT64_MAX / 8 / N, "%s: ld_out=%ld times %s=%ld is no addressable matrix", what, (long)ld_out, n_name, (long)N);
    *span = Span{out, matrix_bytes(N, ld_out, V), "out"};
    return 0;
}

// out may be logp itself -- the same pointer and the same row stride (the kernels' rows re-read a column right before they store
// it: calibration.hip) -- and overlap it in no other way
static inline int check_in_place(const char* what, const Span& out, int64_t ld_out, const Span& logp, int64_t ld) {
    SLNLP_CHECK_ARG((out.p == logp.p && ld_out == ld) || !spans_overlap(out, logp),
                    "%s: out overlaps logp without being logp itself (in place means the same pointer and the same row stride)", what);
    return 0;
}

// a fit's scratch: `need` bytes for N rows of V classes (V = 0: the size depends on the rows alone), aligned to `align` bytes
// (0: the entry point checks that with its other pointers)
static inline int check_scratch(const char* what, const void* scratch, int64_t bytes, size_t need, int64_t N, int64_t V, unsigned align) {
    const bool fits = bytes >= 0 && (size_t)bytes >= need;
    if (V == 0) SLNLP_CHECK_ARG(fits, "%s: scratch of %ld bytes is too small, %ld rows need %ld", what, (long)bytes, (long)N, (long)need);
    SLNLP_CHECK_ARG(fits, "%s: scratch of %ld bytes is too small, %ld rows of %ld classes need %ld", what, (long)bytes, (long)N, (long)V, (long)need);
    SLNLP_CHECK_ARG(align == 0 || ((uintptr_t)scratch & (align - 1)) == 0, "%s: scratch is not %u-byte aligned", what, align);
    return 0;
}

}  // namespace slnlp

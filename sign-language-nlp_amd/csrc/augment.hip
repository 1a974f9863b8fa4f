// augment.hip -- a train epoch's input augmentation, drawn on the device (iterator_train__augment).
//
// Two regularisers of token sequences, per epoch, on the fit's own train rows: FRAME DROPPING deletes random timesteps (the rest
// closes up, the row gets shorter), TOKEN MASKING replaces random tokens by <unk>.  The result goes into the two buffers every
// consumer of the train split already reads, so nothing downstream -- gather, step, captured graph, lockstep group -- changes.
//
// The draw (tests/augment_ref.py is its numpy restatement; include/slnlp.h states it for callers): X int64 [n, S], L int64 [n],
// row i has len = clamp(L[i], 0, S).  Position t < len makes ONE Threefry-4x32 call (the dropout masks' rounds) under key
// (seed_lo, seed_hi, 0, 0) at counter (i, epoch, t, 0) (common.hpp: seed_words); of its words only X0 is used:
//   drop  iff (X0 & 0xFFFF) < thr16(p_drop)          thr16: the dropout threshold rule (common.hpp: dropout_threshold)
//   mask  iff (X0 >> 16)    < thr16(p_mask)
// A row whose every position drew drop drops NONE: a row never loses all of its frames.  The kept positions, in ascending t, go
// to X_out[i, 0 .. len'): <unk> where the position drew mask, X[i, t] otherwise; X_out[i, len' .. S) = pad; L_out[i] = len'.
// Positions >= len of the input are never read.  A pure function of the arguments: nothing depends on the grid or on timing.
//
// One wave per row, four rows per block, rows over a grid-stride loop (wave_rows, common.hpp: gather_id_rows' shape).  Lanes stride the
// positions 64 at a time; within a chunk a kept position's slot is the running base plus the number of kept lanes below it (the
// wave's keep ballot through v_mbcnt), and the base carries over the chunks.  The "everything dropped" rule needs the row's
// total before any store, so a first pass over the chunks only counts ballots and the second draws the same words again and
// stores: a word is ~100 integer instructions, a row of 48 positions one chunk -- cheaper than parking words anywhere.  Integer
// arithmetic only, no atomics, no LDS.
#include <limits.h>

#include "common.hpp"
#include "launch.hpp"
#include "spans.hpp"

namespace slnlp {

__device__ __forceinline__ void augment_rows_body(const int64_t* __restrict__ X, const int64_t* __restrict__ L, int n, int S, int64_t pad,
                                                  int64_t unk, unsigned thr_drop, unsigned thr_mask, unsigned long long seed,
                                                  unsigned epoch, int64_t* __restrict__ X_out, int64_t* __restrict__ L_out) {
    const SeedKey K = seed_key(seed, epoch);
    wave_rows<int>(n, [&](int r, int lane) {             // r, len: the same in every lane, so are the loops' trip counts
        const int64_t l64 = L[r];
        const int len = l64 < 0 ? 0 : (l64 > S ? S : (int)l64);
        const int64_t* src = X + (long)r * S;
        int64_t* dst = X_out + (long)r * S;
        int kept = 0;
        for (int t0 = 0; t0 < len; t0 += 64) {
            const int t = t0 + lane;
            const bool keep = t < len && (seed_words((unsigned)r, (unsigned)t, K).x & 0xFFFFu) >= thr_drop;
            kept += __popcll(__ballot(keep));
        }
        const bool keep_all = kept == 0;                 // every position drew drop (or len == 0): none is dropped
        int base = 0;
        for (int t0 = 0; t0 < len; t0 += 64) {
            const int t = t0 + lane;
            const unsigned w = t < len ? seed_words((unsigned)r, (unsigned)t, K).x : 0u;
            const bool keep = t < len && (keep_all || (w & 0xFFFFu) >= thr_drop);
            const unsigned long long ballot = __ballot(keep);
            if (keep) dst[base + lanes_below(ballot)] = (w >> 16) < thr_mask ? unk : src[t];     // slot <= t < S
            base += __popcll(ballot);
        }
        for (int c = base + lane; c < S; c += 64) dst[c] = pad;
        if (lane == 0) L_out[r] = base;
    });
}
SLNLP_ZKERNEL(augment_rows_kernel, 256, augment_rows_body)

int augment_rows(const int64_t* X, const int64_t* L, int64_t n, int64_t S, int64_t pad, int64_t unk, float p_drop, float p_mask,
                 uint64_t seed, int64_t epoch, int64_t* X_out, int64_t* L_out, hipStream_t st) {
    SLNLP_CHECK_ARG(X && L && X_out && L_out, "augment_rows: null pointer");
    SLNLP_CHECK_ARG(n >= 1 && n <= INT_MAX, "augment_rows: n=%ld outside 1..%d", (long)n, INT_MAX);
    SLNLP_CHECK_ARG(S >= 1 && S <= INT_MAX, "augment_rows: S=%ld outside 1..%d", (long)S, INT_MAX);
    SLNLP_CHECK_ARG(S <= INT64_MAX / 8 / n, "augment_rows: n=%ld times S=%ld is no addressable matrix", (long)n, (long)S);
    SLNLP_CHECK_ARG(epoch >= 0 && epoch <= 0xffffffffLL, "augment_rows: epoch %ld outside [0, 2^32)", (long)epoch);
    SLNLP_CHECK_ARG(p_drop >= 0.0f && p_drop < 1.0f, "augment_rows: p_drop=%g outside [0, 1)", (double)p_drop);      // (a NaN fails both)
    SLNLP_CHECK_ARG(p_mask >= 0.0f && p_mask < 1.0f, "augment_rows: p_mask=%g outside [0, 1)", (double)p_mask);
    const size_t x_bytes = (size_t)n * (size_t)S * 8, l_bytes = (size_t)n * 8;
    // not in-place: a row's stores would run ahead of another chunk's loads, and L is read while L_out is written
    const Span x = {X, x_bytes, "X"}, l = {L, l_bytes, "L"}, xo = {X_out, x_bytes, "X_out"}, lo = {L_out, l_bytes, "L_out"};
    SLNLP_CHECK_ARG(!spans_overlap(xo, x), "augment_rows: X_out overlaps X (the kernel is not in-place)");
    SLNLP_CHECK_ARG(!spans_overlap(lo, l), "augment_rows: L_out overlaps L (the kernel is not in-place)");
    SLNLP_CHECK_ARG(!spans_overlap(xo, l) && !spans_overlap(lo, x) && !spans_overlap(xo, lo), "augment_rows: the id and length buffers overlap");
    return zlaunch(augment_rows_kernel, dim3(wave_rows_grid(n)), 256, 0, st, "augment_rows", X, L, (int)n, (int)S, pad, unk, dropout_threshold(p_drop),
                   dropout_threshold(p_mask), (unsigned long long)seed, (unsigned)epoch, X_out, L_out);
}

}  // namespace slnlp

extern "C" int slnlp_augment_rows(const int64_t* X, const int64_t* L, int64_t n, int64_t S, int64_t pad, int64_t unk, float p_drop,
                                  float p_mask, uint64_t seed, int64_t epoch, int64_t* X_out, int64_t* L_out, void* stream) {
    return slnlp::augment_rows(X, L, n, S, pad, unk, p_drop, p_mask, seed, epoch, X_out, L_out, (hipStream_t)stream);
}

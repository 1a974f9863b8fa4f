// edit_myers.hpp -- one column step of the single-word bit-vector Levenshtein recurrence (Myers 1999 in Hyyro's 2001 form for the
// GLOBAL distance: the horizontal delta of row 0 is +1, the `| 1` below), host and device: edit_knn.hip runs it per reference token,
// and a CPU build can hold it to the plain two-row DP.
//
// The pattern (a query of m tokens, 1 <= m <= 64) lives in the bits 0 .. m - 1 of one 64-bit word; bit j of Pv / Mv says that
// D[j + 1][t] - D[j][t] is +1 / -1 in the current column t.  THE TOP BIT: nothing here forms `1 << m` or a mask of m ones, which
// are what goes wrong at m = 64.  Pv starts as ALL 64 ones whatever m is -- carries of the addition and the shifts only travel
// upwards, so the bits at and above m never reach the bits below it -- and the score is read off bit m - 1 alone
// (top = 1 << (m - 1): 1 << 63 at m = 64 is an ordinary shift).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SLNLP_HD __host__ __device__ __forceinline__
#else
#define SLNLP_HD static inline
#endif

namespace slnlp {

struct MyersState {
    uint64_t Pv, Mv;
    int score;              // D[m][t]
};

SLNLP_HD MyersState myers_begin(int m) { return MyersState{~(uint64_t)0, 0, m}; }

// one text token whose match mask over the pattern positions is Eq (bit j: pattern[j] == token); top = 1 << (m - 1)
SLNLP_HD void myers_step(MyersState& s, uint64_t Eq, uint64_t top) {
    const uint64_t Xv = Eq | s.Mv;
    const uint64_t Xh = (((Eq & s.Pv) + s.Pv) ^ s.Pv) | Eq;
    uint64_t Ph = s.Mv | ~(Xh | s.Pv);
    uint64_t Mh = s.Pv & Xh;
    s.score += (Ph & top) ? 1 : 0;
    s.score -= (Mh & top) ? 1 : 0;
    Ph = (Ph << 1) | 1;
    Mh <<= 1;
    s.Pv = Mh | ~(Xv | Ph);
    s.Mv = Ph & Xv;
}

}  // namespace slnlp

// edit_myers_multi.hpp -- one column step of the MULTI-WORD bit-vector Levenshtein recurrence (Myers 1999 in Hyyro's 2001 form for
// the GLOBAL distance, as edit_myers.hpp; the words chained as in Hyyro's block formulation), host and device: edit_long.hip runs it
// per reference token, and a CPU build holds it to the plain two-row DP (tests/edit_myers_multi_check.cpp).
//
// The pattern (a query of m tokens, 1 <= m <= 64 W) lives in the words 0 .. lw, lw = (m - 1) >> 6: bit j & 63 of word j >> 6 is
// position j.  One text token steps the words in ascending order and hands three bits from a word to the next: the carry of the
// 64-bit addition, and the bits that the shifts of Ph and Mh push out of bit 63 (into word 0 go carry 0, ph 1 -- the horizontal delta
// of row 0 is +1, edit_myers.hpp's `| 1` -- and mh 0).  THE TOP BIT: nothing here forms `1 << m` or a mask of m ones.  Pv starts as
// ALL ones in every word whatever m is -- carries and shifts only travel upwards, so the bits above m - 1 in the last word (and the
// words above lw, which a W larger than needed steps too) never reach the bits below -- and the score is read off bit (m - 1) & 63
// of word lw alone.
//
// W is a template argument and every word loop has constant bounds, so that a compiler unrolls them and Pv[] / Mv[] / Eq[] are
// registers: an array indexed by a run-time value would go to scratch memory.
#pragma once
#include <stdint.h>

#include "edit_myers.hpp"

namespace slnlp {

template <int W>
struct MyersMultiState {
    uint64_t Pv[W], Mv[W];
    int score;              // D[m][t]
};

template <int W>
SLNLP_HD void myers_multi_begin(MyersMultiState<W>& s, int m) {
#pragma unroll
    for (int w = 0; w < W; ++w) {
        s.Pv[w] = ~(uint64_t)0;
        s.Mv[w] = 0;
    }
    s.score = m;
}

// one text token whose match mask over the pattern positions is Eq[0 .. W - 1] (bit j & 63 of word j >> 6: pattern[j] == token; zero
// above lw); lw = (m - 1) >> 6 < W, top = 1 << ((m - 1) & 63)
template <int W>
SLNLP_HD void myers_multi_step(MyersMultiState<W>& s, const uint64_t (&Eq)[W], int lw, uint64_t top) {
    uint64_t carry = 0, ph_in = 1, mh_in = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const uint64_t Pv = s.Pv[w], Mv = s.Mv[w], E = Eq[w];
        const uint64_t Xv = E | Mv;
        const uint64_t a = E & Pv;
        const uint64_t part = a + Pv;                        // the 65-bit sum a + Pv + carry: two adds, at most one of them wraps
        const uint64_t sum = part + carry;
        carry = (uint64_t)(part < a) | (uint64_t)(sum < part);
        const uint64_t Xh = (sum ^ Pv) | E;
        uint64_t Ph = Mv | ~(Xh | Pv);
        uint64_t Mh = Pv & Xh;
        if (w == lw) {
            s.score += (Ph & top) ? 1 : 0;
            s.score -= (Mh & top) ? 1 : 0;
        }
        const uint64_t ph_out = Ph >> 63, mh_out = Mh >> 63;
        Ph = (Ph << 1) | ph_in;
        Mh = (Mh << 1) | mh_in;
        ph_in = ph_out;
        mh_in = mh_out;
        s.Pv[w] = Mh | ~(Xv | Ph);
        s.Mv[w] = Ph & Xv;
    }
}

}  // namespace slnlp

// edit_dist.hpp -- the distance body of the two unit-cost searches, written once: all-pairs Levenshtein distances by Myers'
// bit-vector recurrence (edit_myers_multi.hpp; at one word it is edit_myers.hpp's recurrence, the carry dead and the bits handed into
// word 0 constants).  edit_knn.hip instantiates it for queries of up to 64 frames over a uint8 matrix, edit_long.hip for up to 512
// frames over a uint16 matrix; DESIGN.md section 4.
//
// A block of 256 threads per query (queries over a grid-stride loop; with few queries the references in tiles over grid.y:
// edit_dist_grid).  The query's tokens go to LDS; thread t forms the match masks of the positions t, t + 256, ... -- WORDS words
// each, zero above the query's last word -- and the first occurrence of a token claims a slot of an open hash of SLOTS = 2 MAXLEN
// entries (an integer compare-and-swap on LDS; which slot it lands in is a race, what a lookup finds is not; at most MAXLEN slots
// are taken, so a probe always ends).  Thread t then runs the recurrence over the references t, t + 256, ...: per reference token one
// hash lookup and W word steps.  THE NUMBER OF WORDS lw + 1 = ceil(m / 64) is the same in every thread of a block, which branches once
// per query to the loop built for the smallest W >= lw + 1 of 1, 2, 3, 4, 6, 8 that MAXLEN allows (5 words run the 6-word loop, 7 the
// 8-word one: the words above lw hold all-zero masks and nothing travels downwards).  W is a template argument and the word loops
// unroll, so Pv[] / Mv[] are registers (no scratch memory).
//
// Everything is derived from MAXLEN, the matrix element T and its entry NONE for a pair with an unusable row:
//   MAXLEN  WORDS  SLOTS  hash shift  LDS: tokens + masks + owners          loops
//     64      1     128      57       512 +   512 +  512 =  1536 bytes      W = 1
//    512      8    1024      54      4096 + 32768 + 4096 = 40960 bytes      W = 1, 2, 3, 4, 6, 8
// THE TOP BIT: nothing here forms `1 << m` or a mask of m ones (edit_myers.hpp has the note); a mask bit is 1 << b with b <= 63 and
// the score is read off bit (m - 1) & 63 of word lw.  Tokens are compared as full int64 values.  A query outside its bound writes
// NONE across its tile and reads nothing more; a query of no tokens gives the reference's length.
#pragma once
#include <stdint.h>

#include "common.hpp"
#include "edit_myers_multi.hpp"

namespace slnlp {

template <int MAXLEN>
struct EditDistShape {
    static constexpr int WORDS = MAXLEN / 64, SLOTS = 2 * MAXLEN;
    static constexpr int log2_of(int n) { return n <= 1 ? 0 : 1 + log2_of(n / 2); }
    static constexpr int SHIFT = 64 - log2_of(SLOTS);
    static_assert(WORDS * 64 == MAXLEN && (SLOTS & (SLOTS - 1)) == 0 && WORDS >= 1 && WORDS <= 8, "MAXLEN: 64 times a power of two, at most 512");
    // the top log2(SLOTS) bits of one multiplier: the larger table's index extends the smaller's
    static __device__ __forceinline__ unsigned hash(int64_t c) { return (unsigned)(((uint64_t)c * 0x9E3779B97F4A7C15ull) >> SHIFT); }
};

// the references j_begin + tid, + 256, ... < j_end against the block's query of m >= 1 tokens in W >= lw + 1 words
template <int MAXLEN, int W, class T, int NONE>
__device__ __forceinline__ void edit_dist_refs(const int64_t* __restrict__ Xr, long ldr, const int64_t* __restrict__ Lr, int max_r, int j_begin,
                                               int j_end, int m, const int64_t* pat, const uint64_t* eqm, const int* owner, T* __restrict__ out) {
    using Shape = EditDistShape<MAXLEN>;
    const int lw = Shape::WORDS == 1 ? 0 : (m - 1) >> 6;    // lw < WORDS: a 64-frame query leaves the compiler no branch on it
    const uint64_t top = (uint64_t)1 << ((m - 1) & 63);
    for (int j = j_begin + (int)threadIdx.x; j < j_end; j += 256) {
        const int64_t lr = Lr[j];
        int d = NONE;
        if (lr >= 0 && lr <= max_r) {
            MyersMultiState<W> s;
            myers_multi_begin(s, m);
            const int64_t* row = Xr + (long)j * ldr;
            const int n = (int)lr;
            for (int t = 0; t < n; ++t) {
                const int64_t c = row[t];
                unsigned h = Shape::hash(c);
                int o;
                for (;;) {
                    o = owner[h];
                    if (o < 0 || pat[o] == c) break;
                    h = (h + 1) & (Shape::SLOTS - 1);
                }
                uint64_t Eq[W];
#pragma unroll
                for (int w = 0; w < W; ++w) Eq[w] = o >= 0 ? eqm[o * Shape::WORDS + w] : 0;
                myers_multi_step(s, Eq, lw, top);
            }
            d = s.score;
        }
        out[j] = (T)d;
    }
}

template <int MAXLEN, class T, int NONE>
__device__ __forceinline__ void edit_dist_generic(const int64_t* __restrict__ Xq, long ldq, const int64_t* __restrict__ Lq, int nq,
                                                  const int64_t* __restrict__ Xr, long ldr, const int64_t* __restrict__ Lr, int nr, int max_q,
                                                  int max_r, int tile, T* __restrict__ dist) {
    using Shape = EditDistShape<MAXLEN>;
    constexpr int WORDS = Shape::WORDS, SLOTS = Shape::SLOTS;
    __shared__ int64_t pat[MAXLEN];
    __shared__ uint64_t eqm[MAXLEN * WORDS];
    __shared__ int owner[SLOTS];
    const int tid = threadIdx.x;
    // block (x, y) takes the references [y tile, (y + 1) tile) of the queries x, x + gridDim.x, ...: few queries still fill the device
    const long j_first = (long)blockIdx.y * tile;
    const int j_begin = (int)j_first;
    const int j_end = (int)(j_first + tile < nr ? j_first + tile : nr);
    for (int q = blockIdx.x; q < nq; q += gridDim.x) {       // q, lq, m: the same in every thread, so is every branch on them
        const int64_t lq = Lq[q];
        T* out = dist + (long)q * nr;
        if (lq < 0 || lq > max_q) {                          // reads nothing more
            for (int j = j_begin + tid; j < j_end; j += 256) out[j] = (T)NONE;
            continue;
        }
        const int m = (int)lq;
        if (m == 0) {                                        // the reference's length
            for (int j = j_begin + tid; j < j_end; j += 256) {
                const int64_t lr = Lr[j];
                out[j] = (T)((lr < 0 || lr > max_r) ? NONE : (int)lr);
            }
            continue;
        }
        const int words = ((m - 1) >> 6) + 1;
        __syncthreads();                                     // the lookups of the block's previous query are over
        for (int i = tid; i < SLOTS; i += 256) owner[i] = -1;
        for (int p = tid; p < m; p += 256) pat[p] = Xq[(long)q * ldq + p];
        __syncthreads();
        for (int p = tid; p < m; p += 256) {                 // two positions a thread where m > 256
            const int64_t c = pat[p];
            bool first = true;
#pragma unroll
            for (int w = 0; w < WORDS; ++w) {
                uint64_t mask = 0;
                if (w < words) {
                    const int stop = m - 64 * w < 64 ? m - 64 * w : 64;
                    for (int b = 0; b < stop; ++b) {
                        if (pat[64 * w + b] == c) {
                            mask |= (uint64_t)1 << b;        // b <= 63
                            first = first && 64 * w + b >= p;
                        }
                    }
                }
                eqm[p * WORDS + w] = mask;
            }
            if (first) {                                     // one claim per distinct token
                unsigned h = Shape::hash(c);
                while (atomicCAS(&owner[h], -1, p) != -1) h = (h + 1) & (SLOTS - 1);
            }
        }
        __syncthreads();
#define SLNLP_EDIT_REFS(W) edit_dist_refs<MAXLEN, W, T, NONE>(Xr, ldr, Lr, max_r, j_begin, j_end, m, pat, eqm, owner, out)
        if constexpr (WORDS == 1) {
            SLNLP_EDIT_REFS(1);
        } else {
#ifdef SLNLP_EDIT_LONG_ONLY_W                                // one loop alone, for its register count (tools/time_edit_long.py --registers)
            static_assert(SLNLP_EDIT_LONG_ONLY_W >= 1 && SLNLP_EDIT_LONG_ONLY_W <= WORDS, "SLNLP_EDIT_LONG_ONLY_W outside 1..8");
            if (words <= SLNLP_EDIT_LONG_ONLY_W) SLNLP_EDIT_REFS(SLNLP_EDIT_LONG_ONLY_W);
#else
            static_assert(WORDS == 8, "the loops below: 1, 2, 3, 4, 6, 8 words");
            if (words <= 1) SLNLP_EDIT_REFS(1);
            else if (words <= 2) SLNLP_EDIT_REFS(2);
            else if (words <= 3) SLNLP_EDIT_REFS(3);
            else if (words <= 4) SLNLP_EDIT_REFS(4);
            else if (words <= 6) SLNLP_EDIT_REFS(6);
            else SLNLP_EDIT_REFS(8);
#endif
        }
#undef SLNLP_EDIT_REFS
    }
}

}  // namespace slnlp

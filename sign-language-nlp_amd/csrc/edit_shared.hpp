// edit_shared.hpp -- what the three neighbour searches share: edit_knn.hip (unit-cost Levenshtein over rows of up to 64 frames, a
// uint8 matrix), edit_long.hip (the same distance over rows of up to 512 frames, a uint16 matrix) and field_knn.hip (the
// phonology-weighted distance, a uint16 matrix, the distances 0 .. 64 F).  Device side: the selection body, generic over the matrix
// element, its "none" value and the number of bins.  Host side: the checks of a side, of the pairs and of the scratch size, the grid
// of a distance launch (and the launch itself of the two unit-cost ones), and THE SHELL of the two kinds of call --
// edit_search_distances and edit_search_rows hold every check behind the sides and the order of the launches; a search states its
// names, its element width and its distance bound (EditSearch) and hands in the callables that launch its own kernels.  The head and
// the votes live in edit_knn.hip and take the distance bound and the unit as arguments.  include/slnlp.h states the definitions.
#pragma once
#include <limits.h>

#include "common.hpp"
#include "launch.hpp"
#include "spans.hpp"

namespace slnlp {

enum { EDIT_HEAD_QUERIES = 0, EDIT_HEAD_REFERENCES = 1, EDIT_HEAD_BAD_LABELS = 2 };
constexpr int EDIT_BINS = SLNLP_EDIT_MAX_LEN + 1;        // the distances 0 .. 64
constexpr int EDIT_NONE = 255;                           // the matrix entry of a pair with an unusable row
constexpr int EDIT_MAX_BLOCKS = 65536;

// a wave's LDS stores and atomics, done and visible to its other lanes' loads behind this point
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// ------------------------------------------------------------------------------------------------------- selection ----
// T: the matrix element; NONE: its entry for a pair with an unusable row; CAP: the most bins (LDS: four waves of CAP ints).  The
// distances are 0 .. bins - 1 with bins <= CAP a launch argument -- or, with FIXED, CAP itself at compile time (the uint8 search:
// the code it always had).
template <class T, int NONE, int CAP, bool FIXED>
__device__ __forceinline__ void edit_select_generic(const T* __restrict__ dist, const int64_t* __restrict__ Lq, const int64_t* __restrict__ exclude,
                                                    int nq, int nr, int max_q, int k, int radius, int bins, int* __restrict__ rows,
                                                    int* __restrict__ nbr) {
    __shared__ int hist[4][CAP];
    __shared__ int cand_d[4][64];
    __shared__ int cand_i[4][64];
    const int nb = FIXED ? CAP : bins;
    const int w = threadIdx.x >> 6;
    wave_rows<int>(nq, [&](int q, int lane) {                // q, code, ex and every count below: the same in every lane
        const int64_t lq = Lq[q];
        int code = (lq < 0 || lq > max_q) ? SLNLP_EDIT_CODE_QUERY : 0;
        int ex = -1;
        if (exclude) {
            const int64_t e = exclude[q];
            if (e >= 0 && e < nr) ex = (int)e;
            else if (e != -1) code |= SLNLP_EDIT_CODE_EXCLUDE;
        }
        const bool usable = !(code & SLNLP_EDIT_CODE_QUERY);
        const T* row = dist + (long)q * nr;
        for (int b = lane; b < nb; b += 64) hist[w][b] = 0;
        wave_lds_sync();
        if (usable) {
            for (int j0 = 0; j0 < nr; j0 += 64) {
                const int j = j0 + lane;
                if (j < nr && j != ex) {
                    const int d = row[j];
                    if (d < nb) atomicAdd(&hist[w][d], 1);
                }
            }
        }
        wave_lds_sync();
        int total = 0, cut = nb, below = 0, within = 0, nearest = -1;
        for (int b = 0; b < nb; ++b) {
            const int c = hist[w][b];
            if (c > 0 && nearest < 0) nearest = b;
            if (cut == nb && total + c >= k) { cut = b; below = total; }
            total += c;
            if (b <= radius) within = total;
        }
        const int found = total < k ? total : k;
        const int need = cut < nb ? k - below : 0;           // rows AT the cut-off distance still wanted (cut == bins: every row is below)
        int base = 0, ties = 0;
        for (int j0 = 0; j0 < nr && base < found; j0 += 64) {
            const int j = j0 + lane;
            int d = NONE;
            if (j < nr && j != ex) d = row[j];
            const bool tie = d == cut;
            const unsigned long long tie_ballot = __ballot(tie);
            const bool take = d < cut && d < nb ? true : (tie && ties + lanes_below(tie_ballot) < need);
            const unsigned long long take_ballot = __ballot(take);
            const int slot = base + lanes_below(take_ballot);
            if (take && slot < 64) { cand_d[w][slot] = d; cand_i[w][slot] = j; }
            base += __popcll(take_ballot);
            ties += __popcll(tie_ballot);
        }
        wave_lds_sync();
        const bool mine = lane < found;
        const int my_d = mine ? cand_d[w][lane] : INT_MAX, my_i = mine ? cand_i[w][lane] : INT_MAX;
        int pos = 0;                                         // the pairs in front of mine in (distance, index) order: indices are distinct
        for (int t = 0; t < found; ++t) {
            const int od = cand_d[w][t], oi = cand_i[w][t];
            pos += (od < my_d || (od == my_d && oi < my_i)) ? 1 : 0;
        }
        int* out = nbr + (long)q * k * 2;
        if (mine) { out[2 * pos] = my_d; out[2 * pos + 1] = my_i; }
        else if (lane < k) { out[2 * lane] = -1; out[2 * lane + 1] = -1; }
        if (lane == 0) {
            int* r = rows + 4 * (long)q;
            r[0] = found; r[1] = within; r[2] = nearest; r[3] = code;
        }
        wave_lds_sync();                                     // the wave's next query rewrites hist and cand
    });
}

// ------------------------------------------------------------------------------------------------------- host side ----
struct EditSide {
    const int64_t *X, *L;
    int64_t ld, n;
    Span x, l;
    int max_len;
};
// one side's rows: n in 1..INT_MAX, ld >= 1 and addressable, alignment; a usable row has at most min(bound, ld) tokens, and only
// they are read: the bytes that may be
static inline int edit_check_side(const char* what, const char* side, const int64_t* X, int64_t ld, const int64_t* L, int64_t n, int64_t bound,
                                  EditSide* out) {
    SLNLP_CHECK_ARG(X && L, "%s: null pointer (%s rows)", what, side);
    SLNLP_CHECK_ARG(n >= 1 && n <= SLNLP_EDIT_MAX_ROWS, "%s: %s rows n=%ld outside 1..%d", what, side, (long)n, SLNLP_EDIT_MAX_ROWS);
    SLNLP_CHECK_ARG(ld >= 1 && ld <= INT64_MAX / 8 / n, "%s: %s row stride %ld times %ld rows is no addressable matrix", what, side, (long)ld, (long)n);
    SLNLP_CHECK_ARG((((uintptr_t)X | (uintptr_t)L) & 7) == 0, "%s: misaligned pointer (%s rows: 8 bytes)", what, side);
    const int max_len = (int)(ld < bound ? ld : bound);
    *out = EditSide{X, L, ld, n, Span{X, ((size_t)(n - 1) * (size_t)ld + (size_t)max_len) * 8, side}, Span{L, (size_t)n * 8, side}, max_len};
    return 0;
}
// width: the bytes of a matrix element, 1 or 2
static inline int edit_check_pairs(const char* what, int64_t nq, int64_t nr, int width) {
    SLNLP_CHECK_ARG(nq <= SLNLP_EDIT_MAX_PAIRS / nr, "%s: %ld x %ld pairs, at most %ld (%s each) are formed per call", what, (long)nq, (long)nr,
                    (long)SLNLP_EDIT_MAX_PAIRS, width == 1 ? "one byte" : "two bytes");
    return 0;
}
// the body of the three slnlp_*_knn_scratch_bytes
static inline int64_t edit_scratch_bytes(const char* what, int64_t nq, int64_t nr, int width) {
    if (nq < 1 || nq > SLNLP_EDIT_MAX_ROWS || nr < 1 || nr > SLNLP_EDIT_MAX_ROWS || nq > SLNLP_EDIT_MAX_PAIRS / nr) {
        set_error("%s: %ld x %ld pairs: both counts lie in 1..%d and at most %ld pairs are formed per call", what, (long)nq, (long)nr,
                  SLNLP_EDIT_MAX_ROWS, (long)SLNLP_EDIT_MAX_PAIRS);
        return -1;
    }
    return nq * nr * width;
}
static inline int edit_blocks(int64_t n) { return (int)(n < EDIT_MAX_BLOCKS ? n : EDIT_MAX_BLOCKS); }
// the grid of a distance launch: a block per query, and with fewer than EDIT_FILL queries the references in y tiles (a multiple of
// 256, as many tiles as bring the launch to about EDIT_FILL blocks, every tile with work)
constexpr int EDIT_FILL = 8192;
static inline dim3 edit_dist_grid(int64_t nq, int64_t nr, int* tile_out) {
    int64_t tiles = (EDIT_FILL + nq - 1) / nq;
    const int64_t most = (nr + 255) / 256;
    tiles = tiles < 1 ? 1 : (tiles > most ? most : tiles);
    const int64_t tile = ((nr + tiles - 1) / tiles + 255) / 256 * 256;
    tiles = (nr + tile - 1) / tile;                          // <= EDIT_FILL
    *tile_out = (int)tile;
    return dim3(edit_blocks(nq), (unsigned)tiles);
}

// the distance launch of the two unit-cost searches (edit_dist.hpp's body over T); each tile's block forms the query's hash again
template <class Kernel, class T>
static inline int edit_launch_dist(Kernel kernel, const char* what, const EditSide& Q, const EditSide& R, T* dist, hipStream_t st) {
    int tile;
    const dim3 grid = edit_dist_grid(Q.n, R.n, &tile);
    return zlaunch(kernel, grid, 256, 0, st, what, Q.X, (long)Q.ld, Q.L, (int)Q.n, R.X, (long)R.ld, R.L, (int)R.n, Q.max_len, R.max_len, tile, dist);
}

// ----------------------------------------------------------------------------------------------------------- shell ----
int edit_launch_head(const char* what, const int64_t* Lq, int64_t nq, int max_q, const int64_t* Lr, int64_t nr, int max_r, int64_t* head, hipStream_t st);

// what a search states about itself: its name in every refusal and the names of its three launches, the bytes of a matrix element
// (1 or 2), its largest distance and how the radius refusal words it, and one more input span (the code table; {}: none)
struct EditSearch {
    const char *what, *what_dist, *what_select, *what_head;
    int width;
    int64_t bound;
    const char* bound_says;
    Span extra;
};

// *_distances behind the sides (and the table): dist, the pairs, the overlaps; then launch(what, dist) fills the matrix
template <class Launch>
static inline int edit_search_distances(const EditSearch& s, const EditSide& Q, const EditSide& R, void* dist, Launch launch) {
    const char* what = s.what;
    SLNLP_CHECK_ARG(dist, "%s: null pointer (dist)", what);
    SLNLP_CHECK_ARG(((uintptr_t)dist & (uintptr_t)(s.width - 1)) == 0, "%s: misaligned pointer (dist: %d bytes)", what, s.width);
    SLNLP_TRY(edit_check_pairs(what, Q.n, R.n, s.width));
    const Span in[5] = {Q.x, Q.l, R.x, R.l, s.extra};
    const Span out[1] = {{dist, (size_t)Q.n * (size_t)R.n * s.width, "dist"}};
    SLNLP_TRY(check_no_overlap(what, out, in));
    return launch(what, dist);
}

// *_knn_rows behind the sides (and the table): null pointers, pairs, k, radius, scratch, alignment, overlaps; then
// distances(what_dist, matrix) into the scratch, select(what_select, matrix) and the head
template <class Distances, class Select>
static inline int edit_search_rows(const EditSearch& s, const EditSide& Q, const EditSide& R, const int64_t* exclude, int64_t k, int64_t radius,
                                   void* scratch, int64_t scratch_bytes, int64_t* head, int32_t* rows, int32_t* nbr, hipStream_t st,
                                   Distances distances, Select select) {
    const char* what = s.what;
    SLNLP_CHECK_ARG(scratch && head && rows && nbr, "%s: null pointer (scratch, head, rows or nbr)", what);
    SLNLP_TRY(edit_check_pairs(what, Q.n, R.n, s.width));
    SLNLP_CHECK_ARG(k >= 1 && k <= SLNLP_EDIT_MAX_K, "%s: k=%ld outside 1..%d", what, (long)k, SLNLP_EDIT_MAX_K);
    SLNLP_CHECK_ARG(radius >= 0 && radius <= s.bound, "%s: radius=%ld outside 0..%s", what, (long)radius, s.bound_says);
    const size_t bytes = (size_t)Q.n * (size_t)R.n * s.width;
    SLNLP_TRY(check_scratch(what, scratch, scratch_bytes, bytes, Q.n, 0, s.width));
    SLNLP_CHECK_ARG((((uintptr_t)head | (uintptr_t)exclude) & 7) == 0 && (((uintptr_t)rows | (uintptr_t)nbr) & 3) == 0,
                    "%s: misaligned pointer (head, exclude: 8 bytes; rows, nbr: 4 bytes)", what);
    const Span in[6] = {Q.x, Q.l, R.x, R.l, {exclude, (size_t)Q.n * 8, "exclude"}, s.extra};
    const Span out[4] = {{scratch, bytes, "scratch"}, {head, SLNLP_EDIT_HEAD_BYTES, "head"}, {rows, (size_t)Q.n * 16, "rows"},
                         {nbr, (size_t)Q.n * (size_t)k * 8, "nbr"}};
    SLNLP_TRY(check_no_overlap(what, out, in));
    SLNLP_TRY(distances(s.what_dist, scratch));
    SLNLP_TRY(select(s.what_select, scratch));
    return edit_launch_head(s.what_head, Q.L, Q.n, Q.max_len, R.L, R.n, R.max_len, head, st);
}

// edit_knn.hip: the head of a search, and the votes with their head, for distances 0 .. bound in units of `unit` fields (the
// unit-cost search: 64 and 1).  `what` names the entry point in every message, what_head the second launch.
int edit_launch_logp(const char* what, const char* what_head, int bound, int unit, const int32_t* nbr, const int32_t* rows, const int64_t* Lq,
                     const int64_t* Lr, const int64_t* yr, int64_t nq, int64_t nr, int64_t k, int64_t V, int weights, double tau, int normalize,
                     double lam, const double* prior, float* logp, int64_t ld, int64_t* head, hipStream_t st);

}  // namespace slnlp

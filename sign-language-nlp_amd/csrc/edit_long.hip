// edit_long.hip -- edit_knn.hip's search for rows of up to 512 frames (slnlp.EditKNN(max_len=...), slnlp.split_audit(max_len=...);
// DESIGN.md section 4): all-pairs unit-cost Levenshtein distances by Myers' bit-vector recurrence in its MULTI-WORD form
// (edit_myers_multi.hpp), the query in 1 .. 8 64-bit words.  include/slnlp.h states the definitions and the buffers;
// tests/edit_long_ref.py restates them in numpy.
//
// Rows and buffers are those of edit_knn.hip, but a row is USABLE when its length lies in 0 .. min(max_len, its row stride), max_len
// (1 .. SLNLP_EDIT_LONG_MAX_LEN = 512) a launch argument: only the first L tokens of a usable row are read, nothing of an unusable one
// is -- a row longer than max_len is refused, never truncated -- and tokens are compared as full int64 values.  EVERYTHING IS INTEGER
// until the votes and there are no atomics on global memory: each result is a pure function of the arguments, whatever the grid, the
// stream or the kernels beside it.
//
//   edit_long_dist    a block of 256 threads per query (queries over a grid-stride loop; with few queries the references in tiles
//                     over grid.y: edit_dist_grid, as edit_dist).  The query's tokens go to LDS; thread t forms the match masks of
//                     the positions t and t + 256 -- 8 words each, zero above the query's last word -- and the first occurrence of a
//                     token claims a slot of a 1024-slot open hash (an integer compare-and-swap on LDS; which slot it lands in is a
//                     race, what a lookup finds is not; at most 512 slots are taken, so a probe always ends).  LDS: 4 KiB of tokens,
//                     32 KiB of masks, 4 KiB of owners = 40960 bytes a block, so four blocks share a CU's 160 KiB.  Thread t then
//                     runs the recurrence over references t, t + 256, ...: per reference token one hash lookup and W word steps.
//                     THE NUMBER OF WORDS lw + 1 = ceil(m / 64) is the same in every thread of a block, which branches once per
//                     query to the loop built for the smallest W >= lw + 1 of 1, 2, 3, 4, 6, 8 (5 words run the 6-word loop, 7 the
//                     8-word one: the words above lw hold all-zero masks and nothing travels downwards).  W is a template argument
//                     and the word loops unroll, so Pv[] / Mv[] are registers (no scratch memory: profiles/edit_long_timing.json
//                     lists the register counts).  uint16 [nq, nr]; 65535 where either row is unusable.
//   edit_long_select  edit_shared.hpp's selection body over the uint16 matrix with max_len + 1 <= 513 bins.
//   the head and the votes are edit_knn.hip's kernels with the bound max_len and the unit 1.
#include <limits.h>

#include "common.hpp"
#include "edit_myers_multi.hpp"
#include "edit_shared.hpp"
#include "launch.hpp"
#include "spans.hpp"

namespace slnlp {

constexpr int LONG_NONE = 65535;                             // the matrix entry of a pair with an unusable row
constexpr int LONG_WORDS = SLNLP_EDIT_LONG_MAX_LEN / 64;     // 8
constexpr int LONG_BINS_CAP = SLNLP_EDIT_LONG_MAX_LEN + 1;   // the distances 0 .. 512
constexpr int LONG_SLOTS = 1024;                             // of the query's token hash: at most 512 are taken, a probe always ends
static_assert(LONG_WORDS * 64 == SLNLP_EDIT_LONG_MAX_LEN && LONG_SLOTS >= 2 * SLNLP_EDIT_LONG_MAX_LEN, "edit_long.hip and slnlp.h disagree");

// the top 10 bits of edit_knn.hip's multiplier
__device__ __forceinline__ unsigned edit_long_hash(int64_t c) { return (unsigned)(((uint64_t)c * 0x9E3779B97F4A7C15ull) >> 54); }

// ------------------------------------------------------------------------------------------------------- distances ----
// the references j_begin + tid, + 256, ... < j_end against the block's query of m >= 1 tokens in W >= lw + 1 words
template <int W>
__device__ __forceinline__ void edit_long_refs(const int64_t* __restrict__ Xr, long ldr, const int64_t* __restrict__ Lr, int max_r, int j_begin,
                                               int j_end, int m, const int64_t* pat, const uint64_t* eqm, const int* owner,
                                               unsigned short* __restrict__ out) {
    const int lw = (m - 1) >> 6;
    const uint64_t top = (uint64_t)1 << ((m - 1) & 63);
    for (int j = j_begin + (int)threadIdx.x; j < j_end; j += 256) {
        const int64_t lr = Lr[j];
        int d = LONG_NONE;
        if (lr >= 0 && lr <= max_r) {
            MyersMultiState<W> s;
            myers_multi_begin(s, m);
            const int64_t* row = Xr + (long)j * ldr;
            const int n = (int)lr;
            for (int t = 0; t < n; ++t) {
                const int64_t c = row[t];
                unsigned h = edit_long_hash(c);
                int o;
                for (;;) {
                    o = owner[h];
                    if (o < 0 || pat[o] == c) break;
                    h = (h + 1) & (LONG_SLOTS - 1);
                }
                uint64_t Eq[W];
#pragma unroll
                for (int w = 0; w < W; ++w) Eq[w] = o >= 0 ? eqm[o * LONG_WORDS + w] : 0;
                myers_multi_step(s, Eq, lw, top);
            }
            d = s.score;
        }
        out[j] = (unsigned short)d;
    }
}

__device__ __forceinline__ void edit_long_dist_body(const int64_t* __restrict__ Xq, long ldq, const int64_t* __restrict__ Lq, int nq,
                                                    const int64_t* __restrict__ Xr, long ldr, const int64_t* __restrict__ Lr, int nr, int max_q,
                                                    int max_r, int tile, unsigned short* __restrict__ dist) {
    __shared__ int64_t pat[SLNLP_EDIT_LONG_MAX_LEN];
    __shared__ uint64_t eqm[SLNLP_EDIT_LONG_MAX_LEN * LONG_WORDS];
    __shared__ int owner[LONG_SLOTS];
    const int tid = threadIdx.x;
    // block (x, y) takes the references [y tile, (y + 1) tile) of the queries x, x + gridDim.x, ...: few queries still fill the device
    const long j_first = (long)blockIdx.y * tile;
    const int j_begin = (int)j_first;
    const int j_end = (int)(j_first + tile < nr ? j_first + tile : nr);
    for (int q = blockIdx.x; q < nq; q += gridDim.x) {       // q, lq, m: the same in every thread, so is every branch on them
        const int64_t lq = Lq[q];
        unsigned short* out = dist + (long)q * nr;
        if (lq < 0 || lq > max_q) {                          // reads nothing more
            for (int j = j_begin + tid; j < j_end; j += 256) out[j] = (unsigned short)LONG_NONE;
            continue;
        }
        const int m = (int)lq;
        if (m == 0) {                                        // the reference's length
            for (int j = j_begin + tid; j < j_end; j += 256) {
                const int64_t lr = Lr[j];
                out[j] = (unsigned short)((lr < 0 || lr > max_r) ? LONG_NONE : (int)lr);
            }
            continue;
        }
        const int words = ((m - 1) >> 6) + 1;
        __syncthreads();                                     // the lookups of the block's previous query are over
        for (int i = tid; i < LONG_SLOTS; i += 256) owner[i] = -1;
        for (int p = tid; p < m; p += 256) pat[p] = Xq[(long)q * ldq + p];
        __syncthreads();
        for (int p = tid; p < m; p += 256) {                 // two positions a thread where m > 256
            const int64_t c = pat[p];
            bool first = true;
#pragma unroll
            for (int w = 0; w < LONG_WORDS; ++w) {
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
                eqm[p * LONG_WORDS + w] = mask;
            }
            if (first) {                                     // one claim per distinct token
                unsigned h = edit_long_hash(c);
                while (atomicCAS(&owner[h], -1, p) != -1) h = (h + 1) & (LONG_SLOTS - 1);
            }
        }
        __syncthreads();
#ifdef SLNLP_EDIT_LONG_ONLY_W                                // one loop alone, for its register count (tools/time_edit_long.py --registers)
        static_assert(SLNLP_EDIT_LONG_ONLY_W >= 1 && SLNLP_EDIT_LONG_ONLY_W <= LONG_WORDS, "SLNLP_EDIT_LONG_ONLY_W outside 1..8");
        if (words <= SLNLP_EDIT_LONG_ONLY_W) edit_long_refs<SLNLP_EDIT_LONG_ONLY_W>(Xr, ldr, Lr, max_r, j_begin, j_end, m, pat, eqm, owner, out);
        continue;
#endif
        if (words <= 1) edit_long_refs<1>(Xr, ldr, Lr, max_r, j_begin, j_end, m, pat, eqm, owner, out);
        else if (words <= 2) edit_long_refs<2>(Xr, ldr, Lr, max_r, j_begin, j_end, m, pat, eqm, owner, out);
        else if (words <= 3) edit_long_refs<3>(Xr, ldr, Lr, max_r, j_begin, j_end, m, pat, eqm, owner, out);
        else if (words <= 4) edit_long_refs<4>(Xr, ldr, Lr, max_r, j_begin, j_end, m, pat, eqm, owner, out);
        else if (words <= 6) edit_long_refs<6>(Xr, ldr, Lr, max_r, j_begin, j_end, m, pat, eqm, owner, out);
        else edit_long_refs<8>(Xr, ldr, Lr, max_r, j_begin, j_end, m, pat, eqm, owner, out);
    }
}
SLNLP_ZKERNEL(edit_long_dist_kernel, 256, edit_long_dist_body)

// ------------------------------------------------------------------------------------------------------- selection ----
__device__ __forceinline__ void edit_long_select_body(const unsigned short* __restrict__ dist, const int64_t* __restrict__ Lq,
                                                      const int64_t* __restrict__ exclude, int nq, int nr, int max_q, int k, int radius, int bins,
                                                      int* __restrict__ rows, int* __restrict__ nbr) {
    edit_select_generic<unsigned short, LONG_NONE, LONG_BINS_CAP, false>(dist, Lq, exclude, nq, nr, max_q, k, radius, bins, rows, nbr);
}
SLNLP_ZKERNEL(edit_long_select_kernel, 256, edit_long_select_body)

// ------------------------------------------------------------------------------------------------------- host side ----
static int edit_long_check_max_len(const char* what, int64_t max_len) {
    SLNLP_CHECK_ARG(max_len >= 1 && max_len <= SLNLP_EDIT_LONG_MAX_LEN, "%s: max_len=%ld outside 1..%d", what, (long)max_len, SLNLP_EDIT_LONG_MAX_LEN);
    return 0;
}
// edit_check_side with the bound max_len where it has 64: a usable row has at most min(max_len, ld) tokens, and only they are read
static int edit_long_check_side(const char* what, const char* side, const int64_t* X, int64_t ld, const int64_t* L, int64_t n, int64_t max_len,
                                EditSide* out) {
    SLNLP_TRY(edit_check_side(what, side, X, ld, L, n, out));
    out->max_len = (int)(ld < max_len ? ld : max_len);
    out->x = Span{X, ((size_t)(n - 1) * (size_t)ld + (size_t)out->max_len) * 8, side};
    return 0;
}
static int edit_long_check_pairs(const char* what, int64_t nq, int64_t nr) {
    SLNLP_CHECK_ARG(nq <= SLNLP_EDIT_MAX_PAIRS / nr, "%s: %ld x %ld pairs, at most %ld (two bytes each) are formed per call", what, (long)nq, (long)nr,
                    (long)SLNLP_EDIT_MAX_PAIRS);
    return 0;
}
static int launch_edit_long_dist(const char* what, const int64_t* Xq, int64_t ldq, const int64_t* Lq, int64_t nq, int max_q, const int64_t* Xr,
                                 int64_t ldr, const int64_t* Lr, int64_t nr, int max_r, unsigned short* dist, hipStream_t st) {
    int tile;
    const dim3 grid = edit_dist_grid(nq, nr, &tile);
    return zlaunch(edit_long_dist_kernel, grid, 256, 0, st, what, Xq, (long)ldq, Lq, (int)nq, Xr, (long)ldr, Lr, (int)nr, max_q, max_r, tile, dist);
}

int edit_long_distances(const int64_t* Xq, int64_t ldq, const int64_t* Lq, int64_t nq, const int64_t* Xr, int64_t ldr, const int64_t* Lr, int64_t nr,
                        int64_t max_len, uint16_t* dist, hipStream_t st) {
    const char* what = "edit_long_distances";
    EditSide Q, R;
    SLNLP_TRY(edit_long_check_max_len(what, max_len));
    SLNLP_TRY(edit_long_check_side(what, "query", Xq, ldq, Lq, nq, max_len, &Q));
    SLNLP_TRY(edit_long_check_side(what, "reference", Xr, ldr, Lr, nr, max_len, &R));
    SLNLP_CHECK_ARG(dist, "%s: null pointer (dist)", what);
    SLNLP_CHECK_ARG(((uintptr_t)dist & 1) == 0, "%s: misaligned pointer (dist: 2 bytes)", what);
    SLNLP_TRY(edit_long_check_pairs(what, nq, nr));
    const Span in[4] = {Q.x, Q.l, R.x, R.l};
    const Span out[1] = {{dist, (size_t)nq * (size_t)nr * 2, "dist"}};
    SLNLP_TRY(check_no_overlap(what, out, in));
    return launch_edit_long_dist(what, Xq, ldq, Lq, nq, Q.max_len, Xr, ldr, Lr, nr, R.max_len, (unsigned short*)dist, st);
}

int edit_long_knn_rows(const int64_t* Xq, int64_t ldq, const int64_t* Lq, int64_t nq, const int64_t* Xr, int64_t ldr, const int64_t* Lr, int64_t nr,
                       int64_t max_len, const int64_t* exclude, int64_t k, int64_t radius, void* scratch, int64_t scratch_bytes, int64_t* head,
                       int32_t* rows, int32_t* nbr, hipStream_t st) {
    const char* what = "edit_long_knn_rows";
    EditSide Q, R;
    SLNLP_TRY(edit_long_check_max_len(what, max_len));
    SLNLP_TRY(edit_long_check_side(what, "query", Xq, ldq, Lq, nq, max_len, &Q));
    SLNLP_TRY(edit_long_check_side(what, "reference", Xr, ldr, Lr, nr, max_len, &R));
    SLNLP_CHECK_ARG(scratch && head && rows && nbr, "%s: null pointer (scratch, head, rows or nbr)", what);
    SLNLP_TRY(edit_long_check_pairs(what, nq, nr));
    SLNLP_CHECK_ARG(k >= 1 && k <= SLNLP_EDIT_MAX_K, "%s: k=%ld outside 1..%d", what, (long)k, SLNLP_EDIT_MAX_K);
    SLNLP_CHECK_ARG(radius >= 0 && radius <= max_len, "%s: radius=%ld outside 0..max_len=%ld", what, (long)radius, (long)max_len);
    const size_t pairs = (size_t)nq * (size_t)nr;
    SLNLP_TRY(check_scratch(what, scratch, scratch_bytes, pairs * 2, nq, 0, 2));
    SLNLP_CHECK_ARG((((uintptr_t)head | (uintptr_t)exclude) & 7) == 0 && (((uintptr_t)rows | (uintptr_t)nbr) & 3) == 0,
                    "%s: misaligned pointer (head, exclude: 8 bytes; rows, nbr: 4 bytes)", what);
    const Span in[5] = {Q.x, Q.l, R.x, R.l, {exclude, (size_t)nq * 8, "exclude"}};
    const Span out[4] = {{scratch, pairs * 2, "scratch"}, {head, SLNLP_EDIT_HEAD_BYTES, "head"}, {rows, (size_t)nq * 16, "rows"},
                         {nbr, (size_t)nq * (size_t)k * 8, "nbr"}};
    SLNLP_TRY(check_no_overlap(what, out, in));
    unsigned short* dist = (unsigned short*)scratch;
    SLNLP_TRY(launch_edit_long_dist("edit_long_knn_distances", Xq, ldq, Lq, nq, Q.max_len, Xr, ldr, Lr, nr, R.max_len, dist, st));
    SLNLP_TRY(zlaunch(edit_long_select_kernel, dim3(wave_rows_grid(nq)), 256, 0, st, "edit_long_knn_select", (const unsigned short*)dist, Lq, exclude,
                      (int)nq, (int)nr, Q.max_len, (int)k, (int)radius, (int)max_len + 1, (int*)rows, (int*)nbr));
    return edit_launch_head("edit_long_knn_head", Lq, nq, Q.max_len, Lr, nr, R.max_len, head, st);
}

int edit_long_knn_logp(const int32_t* nbr, const int32_t* rows, const int64_t* Lq, const int64_t* Lr, const int64_t* yr, int64_t nq, int64_t nr,
                       int64_t k, int64_t V, int64_t max_len, int weights, double tau, int normalize, double lam, const double* prior, float* logp,
                       int64_t ld, int64_t* head, hipStream_t st) {
    const char* what = "edit_long_knn_logp";
    SLNLP_TRY(edit_long_check_max_len(what, max_len));
    return edit_launch_logp(what, "edit_long_knn_logp_head", (int)max_len, 1, nbr, rows, Lq, Lr, yr, nq, nr, k, V, weights, tau, normalize, lam, prior, logp,
                            ld, head, st);
}

}  // namespace slnlp

extern "C" int slnlp_edit_long_distances(const int64_t* Xq, int64_t ldq, const int64_t* Lq, int64_t nq, const int64_t* Xr, int64_t ldr, const int64_t* Lr,
                                         int64_t nr, int64_t max_len, uint16_t* dist, void* stream) {
    return slnlp::edit_long_distances(Xq, ldq, Lq, nq, Xr, ldr, Lr, nr, max_len, dist, (hipStream_t)stream);
}
extern "C" int64_t slnlp_edit_long_knn_scratch_bytes(int64_t nq, int64_t nr) {
    if (nq < 1 || nq > SLNLP_EDIT_MAX_ROWS || nr < 1 || nr > SLNLP_EDIT_MAX_ROWS || nq > SLNLP_EDIT_MAX_PAIRS / nr) {
        slnlp::set_error("edit_long_knn_scratch_bytes: %ld x %ld pairs: both counts lie in 1..%d and at most %ld pairs are formed per call", (long)nq,
                         (long)nr, SLNLP_EDIT_MAX_ROWS, (long)SLNLP_EDIT_MAX_PAIRS);
        return -1;
    }
    return nq * nr * 2;
}
extern "C" int slnlp_edit_long_knn_rows(const int64_t* Xq, int64_t ldq, const int64_t* Lq, int64_t nq, const int64_t* Xr, int64_t ldr, const int64_t* Lr,
                                        int64_t nr, int64_t max_len, const int64_t* exclude, int64_t k, int64_t radius, void* scratch,
                                        int64_t scratch_bytes, int64_t* head, int32_t* rows, int32_t* nbr, void* stream) {
    return slnlp::edit_long_knn_rows(Xq, ldq, Lq, nq, Xr, ldr, Lr, nr, max_len, exclude, k, radius, scratch, scratch_bytes, head, rows, nbr,
                                     (hipStream_t)stream);
}
extern "C" int slnlp_edit_long_knn_logp(const int32_t* nbr, const int32_t* rows, const int64_t* Lq, const int64_t* Lr, const int64_t* yr, int64_t nq,
                                        int64_t nr, int64_t k, int64_t V, int64_t max_len, int weights, double tau, int normalize, double lam,
                                        const double* prior, float* logp, int64_t ld, int64_t* head, void* stream) {
    return slnlp::edit_long_knn_logp(nbr, rows, Lq, Lr, yr, nq, nr, k, V, max_len, weights, tau, normalize, lam, prior, logp, ld, head,
                                     (hipStream_t)stream);
}

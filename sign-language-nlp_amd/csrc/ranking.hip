// ranking.hip -- what one-vs-rest ROC AUC and average precision of a set of log-probs are functions of, on the device (DESIGN.md
// section 4; slnlp/metrics.py's auc_macro / auc_weighted / ap_macro / ap_weighted, NeuralNetClassifier.ranking).
//
// z float32 log-probs [N, ld] (V columns used), y int64 [N].  For class c the rows with y = c are its positives (P of them), every
// other row with a label in [0, V) a negative (Q); the score of row j for class c is z[j, c] as stored: ties are ties of the float32
// values, -0.0 == +0.0, -inf is an ordinary value.  Per row i, with c = y_i and x = z[i, c], three exact integers:
//   gt_neg = #{negatives j: z[j, c] > x}     eq_neg = #{negatives j: z[j, c] == x}     ge_pos = #{positives j: z[j, c] >= x} (i included)
// rows[i] = (gt_neg, eq_neg, ge_pos, code): code 0; -1 for a label outside [0, V) (never used as an index; such a row is neither
// positive nor negative for any class; the counts are 0); -2 when column c holds a NaN in a row with a valid label (the class is
// undefined; the counts are 0).  table [V + 1, 4]: row c = (P_c, the NaN entries of column c over the valid rows,
// sum_{i in c} (2 (Q - gt_neg) - eq_neg), sum_{i in c} ge_pos / (ge_pos + gt_neg + eq_neg)) -- the two sums are 0 for a class with
// a NaN -- and row V = (valid rows, rows with a bad label, 0, 0).  AUC_c = table[c][2] / (2 P Q) (Mann-Whitney, half credit for
// ties), AP_c = table[c][3] / P (the step-wise average precision).  tests/ranking_ref.py restates all of it.
//
// HOW IT RUNS.  One launch, V blocks of 256 threads, block c takes class c; no global atomics, nothing that depends on the grid.
// The chunk_* steps are rank_chunk.hpp's, block_tree is block_reduce.hpp's.
//   1. chunk_ordinal: the block scans y in tiles of 256 rows and compacts its positives -- row index and rank_key of the value, an
//      order-preserving uint32 -- into LDS in ascending row order, so which positives form a chunk (RANK_CHUNK of them) does not
//      depend on timing; the valid rows are counted in the same round.  chunk_pad_and_clear: padding, zeroed histograms;
//   2. chunk_bitonic_sort: the chunk by key (equal keys give equal counts and equal terms: their order is immaterial);
//   3. the block streams the N values of column c: per valid row chunk_lower_bound (lb) and chunk_upper_bound (ub) and integer
//      LDS atomics on three histograms: a negative adds 1 at lo[lb] and at up[ub], a positive at pos[ub].  Integer adds commute;
//   4. chunk_suffix / chunk_step: strict suffix sums S give the counts of the positive at sorted position p: gt_neg = S_lo[p],
//      eq_neg = S_up[p] - S_lo[p], ge_pos = S_pos[p]; they go to rows by original row index;
//   5. the two table sums: a thread adds its 8 sorted positions in ascending order, block_tree adds the 256 threads, thread 0
//      adds the chunks in ascending order.  The third column is an exact integer (2 N^2 < 2^53 is checked).
// A class with more than RANK_CHUNK positives repeats 1-5 per chunk (the column is streamed once per chunk: correct, not fast; the
// data set has about 20 positives per class).  NaNs are counted per column and take part in no search.  The column reads are
// strided (ld x 4 bytes apart); 32 neighbouring classes share each line out of L2.
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "block_reduce.hpp"
#include "common.hpp"
#include "launch.hpp"
#include "rank_chunk.hpp"
#include "spans.hpp"

namespace slnlp {

constexpr int RANK_CHUNK = SLNLP_RANK_CHUNK;    // positives per LDS chunk: a power of two, 8 per thread
constexpr int RANK_PER_THREAD = RANK_CHUNK / 256;
static_assert(RANK_PER_THREAD * 256 == RANK_CHUNK && (RANK_CHUNK & (RANK_CHUNK - 1)) == 0, "RANK_CHUNK: a power of two, a multiple of 256");
constexpr unsigned RANK_KEY_NAN = 0xFFFFFFFEu;  // a positive whose own value is a NaN: behind every real key (+inf is 0xFF800000)
constexpr unsigned RANK_KEY_PAD = 0xFFFFFFFFu;  // the sort's padding

__device__ __forceinline__ void ranking_rows_body(const float* __restrict__ logp, long ld, const int64_t* __restrict__ y, int N, int V,
                                                  int* __restrict__ rows, double* __restrict__ table) {
    __shared__ unsigned keys[RANK_CHUNK];
    __shared__ int idx[RANK_CHUNK];
    __shared__ int hist[3][RANK_CHUNK + 1];              // lo[lb], up[ub] of the negatives, pos[ub] of the positives
    __shared__ int part[3][256];
    __shared__ double red[2][256];
    __shared__ int wtot[2][4];
    const int tid = threadIdx.x;
    const int c = blockIdx.x;                            // < V
    const float* col = logp + c;
    double sum_u = 0.0, sum_ap = 0.0;                    // thread 0: the table's two sums over the chunks so far
    int P = 0, nvalid = 0, nan_c = 0;
    int first = 0;                                       // the ordinal of the chunk's first positive
    do {
        // 1. the positives of this chunk, in ascending row order
        int pos_base = 0, valid_base = 0;
        for (long r0 = 0; r0 < N; r0 += 256) {           // every thread makes every round: ballots and barriers inside
            const long r = r0 + tid;
            int64_t label = -1;
            if (r < N) label = y[r];
            const bool valid = label >= 0 && label < V;  // a label outside the columns is never used as an index
            const bool mine = valid && label == c;
            const bool flags[2] = {mine, valid};
            int all[2];                                  // the tile's positives, its valid rows
            const int ord = pos_base + chunk_ordinal(flags, wtot, tid, all);
            if (mine && ord >= first && ord - first < RANK_CHUNK) {
                const float x = col[r * ld];
                keys[ord - first] = x != x ? RANK_KEY_NAN : rank_key(x);
                idx[ord - first] = (int)r;
            }
            if (first == 0 && c == 0 && rows && r < N && !valid) *(int4*)(rows + 4 * r) = int4{0, 0, 0, -1};
            pos_base += all[0];
            valid_base += all[1];
        }
        P = pos_base;
        nvalid = valid_base;
        const int n = min(P - first, RANK_CHUNK);        // 0 only when P == 0
        const int m = chunk_pad_and_clear(keys, idx, hist, n, RANK_KEY_PAD, tid);
        // 2. the chunk by key
        chunk_bitonic_sort(keys, idx, m, tid);
        // 3. the column against the sorted keys
        int nans = 0;
        for (long r = tid; r < N; r += 256) {
            const int64_t label = y[r];
            if (label < 0 || label >= V) continue;
            const float x = col[r * ld];
            if (x != x) { ++nans; continue; }
            const unsigned key = rank_key(x);
            const int lb = chunk_lower_bound(keys, n, key);
            const int ub = chunk_upper_bound(keys, n, key, lb);
            if (label == c) {
                atomicAdd(&hist[2][ub], 1);
            } else {
                atomicAdd(&hist[0][lb], 1);
                atomicAdd(&hist[1][ub], 1);
            }
        }
        part[0][tid] = nans;
        block_tree<1>(part, tid, TreeSum{});
        nan_c = part[0][0];
        __syncthreads();                                 // part is rewritten below; the histograms are complete
        // 4. strict suffix sums; the thread's positions from the last to the first, the terms kept to be added in ascending order
        int run[3];
        chunk_suffix(hist, part, tid, run);
        const int p0 = tid * RANK_PER_THREAD;
        const double Q = (double)(nvalid - P);
        double tu[RANK_PER_THREAD], ta[RANK_PER_THREAD];
#pragma unroll
        for (int q = RANK_PER_THREAD - 1; q >= 0; --q) {
            const int p = p0 + q;
            tu[q] = 0.0; ta[q] = 0.0;
            if (p < n) {
                const int gt = run[0], eq = run[1] - run[0], ge = run[2];
                if (nan_c == 0) {
                    tu[q] = 2.0 * (Q - (double)gt) - (double)eq;
                    ta[q] = (double)ge / ((double)ge + (double)gt + (double)eq);
                }
                if (rows) *(int4*)(rows + 4 * (long)idx[p]) = nan_c == 0 ? int4{gt, eq, ge, 0} : int4{0, 0, 0, -2};
            }
            chunk_step(run, hist, p);
        }
        // 5. the chunk's two sums
        double su = 0.0, sa = 0.0;
#pragma unroll
        for (int q = 0; q < RANK_PER_THREAD; ++q) { su += tu[q]; sa += ta[q]; }
        red[0][tid] = su; red[1][tid] = sa;
        block_tree<2>(red, tid, TreeSum{});
        if (tid == 0) { sum_u += red[0][0]; sum_ap += red[1][0]; }
        __syncthreads();                                 // the next chunk rewrites everything
        first += RANK_CHUNK;
    } while (first < P);
    if (tid == 0) {
        *(double4*)(table + 4 * (long)c) = double4{(double)P, (double)nan_c, sum_u, sum_ap};
        if (c == 0) *(double4*)(table + 4 * (long)V) = double4{(double)nvalid, (double)(N - nvalid), 0.0, 0.0};
    }
}
SLNLP_ZKERNEL(ranking_rows_kernel, 256, ranking_rows_body)

int ranking_rows(const float* logp, int64_t ld, const int64_t* y, int64_t N, int64_t V, int32_t* rows, double* table, hipStream_t st) {
    SLNLP_CHECK_ARG(logp && y && table, "ranking_rows: null pointer");
    Span z;
    SLNLP_TRY(check_logp_matrix("ranking_rows", logp, N, SLNLP_RANK_MAX_ROWS, V, INT_MAX - 1, ld, &z));
    SLNLP_CHECK_ARG(((uintptr_t)logp & 3) == 0 && ((uintptr_t)y & 7) == 0, "ranking_rows: misaligned pointer");
    SLNLP_CHECK_ARG(((uintptr_t)rows & 15) == 0, "ranking_rows: rows is not 16-byte aligned");
    SLNLP_CHECK_ARG(((uintptr_t)table & 31) == 0, "ranking_rows: table is not 32-byte aligned");
    const size_t n = (size_t)N;
    const Span in[2] = {z, {y, n * 8, "y"}};
    const Span out[2] = {{rows, n * 16, "rows"}, {table, ((size_t)V + 1) * 32, "table"}};
    SLNLP_TRY(check_no_overlap("ranking_rows", out, in));
    return zlaunch(ranking_rows_kernel, dim3((unsigned)V), 256, 0, st, "ranking_rows", logp, (long)ld, y, (int)N, (int)V, (int*)rows, table);
}

}  // namespace slnlp

extern "C" int slnlp_ranking_rows(const float* logp, int64_t ld, const int64_t* y, int64_t N, int64_t V, int32_t* rows, double* table,
                                  void* stream) {
    return slnlp::ranking_rows(logp, ld, y, N, V, rows, table, (hipStream_t)stream);
}

// score.hip -- an epoch's log-probs reduced to what the scoring metrics need, on the device (slnlp/metrics.py).
//
// Accuracy, log-loss, the precision / recall / F1 family (weighted or macro), balanced accuracy and top-k accuracy are all
// functions of three values per sample and three counts per class.  One pass over logp [N, ld] (V columns used) and y [N]:
//
//   pred[i]    the index of the row's first maximum (np.argmax: a NaN is larger than everything, the first NaN wins)
//   picked[i]  v = logp[i, y[i]], bit for bit
//   rank[i]    #{j : logp[i, j] > v} + #{j > y[i] : logp[i, j] == v} -- the position of the true class in a stable ascending
//              argsort read backwards (sklearn's top_k_accuracy_score: among equal scores the higher index comes first);
//              V -- never a hit -- when the row holds a NaN
//   counts     true_sum [V] | pred_sum [V] | tp_sum [V] | n_bad: the per-class sums of a confusion matrix's row, column and
//              diagonal, and the number of labels outside [0, V)
//
// A label outside [0, V) is never used as an index: its row gets picked = NaN and rank = V, counts as one n_bad and enters
// pred_sum only.  tests/score_ref.py is the numpy restatement.
//
// One wave per row, four rows per block, rows over a grid-stride loop (wave_rows, common.hpp): lanes stride the columns (coalesced), v is read first,
// so the maximum, its index and the two rank counts come out of the same pass.  The wave-level combines are DPP exchanges and
// v_readlane over all 64 lanes (common.hpp); the arg-max rule -- larger value wins, equal values: lower index, NaN beats all -- is
// a total order on (value, index), so every lane of a pair computes the same winner.  The class counts are integer atomics, one
// lane per row: sums of integers, the same whatever the order of arrival.  Both kernels take the argument-pack form of launch.hpp.
#include <limits.h>
#include <math.h>

#include <algorithm>

#include "block_reduce.hpp"
#include "common.hpp"
#include "launch.hpp"
#include "spans.hpp"

namespace slnlp {

constexpr int SCORE_ZERO_MAX_BLOCKS = 2048;  // x 256 entries: more counts wrap score_zero's stride loop

// (the arg-max order score_beats, its wave reduction wave_best and wave_sum_i: common.hpp)

__device__ __forceinline__ void score_zero_body(int* __restrict__ counts, int n) {
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += gridDim.x * 256L) counts[i] = 0;
}
SLNLP_ZKERNEL(score_zero_kernel, 256, score_zero_body)

__device__ __forceinline__ void score_rows_body(const float* __restrict__ logp, long ld, const int64_t* __restrict__ y, int N, int V,
                                                int* __restrict__ pred, float* __restrict__ picked, int* __restrict__ rank,
                                                int* __restrict__ counts) {
    const float qnan = __builtin_bit_cast(float, 0x7fc00000);
    wave_rows(N, [&](long r, int lane) {
        const float* row = logp + r * ld;
        const int64_t label = y[r];
        const bool ok = label >= 0 && label < V;
        const float v = ok ? row[label] : qnan;
        float bv = -INFINITY;                            // (any column beats this start: -inf at column j ties and j < INT_MAX)
        int bi = INT_MAX, gt = 0, eq = 0, nans = 0;
        for (int j = lane; j < V; j += 64) {
            const float x = row[j];
            if (score_beats(x, j, bv, bi)) { bv = x; bi = j; }
            gt += x > v ? 1 : 0;
            eq += (x == v && j > label) ? 1 : 0;
            nans += x != x ? 1 : 0;
        }
        wave_best(bv, bi);                               // bi in [0, V): V >= 1, lane 0 read column 0
        gt = wave_sum_i(gt);
        eq = wave_sum_i(eq);
        nans = wave_sum_i(nans);
        if (lane == 0) {
            pred[r] = bi;
            picked[r] = v;
            rank[r] = (ok && nans == 0) ? gt + eq : V;
            atomicAdd(&counts[(long)V + bi], 1);
            if (ok) {
                atomicAdd(&counts[label], 1);
                if (bi == label) atomicAdd(&counts[2L * V + label], 1);
            } else {
                atomicAdd(&counts[3L * V], 1);
            }
        }
    });
}
SLNLP_ZKERNEL(score_rows_kernel, 256, score_rows_body)

int score_rows(const float* logp, int64_t ld, const int64_t* y, int64_t N, int V, int32_t* pred, float* picked, int32_t* rank,
               int32_t* counts, hipStream_t st) {
    SLNLP_CHECK_ARG(logp && y && pred && picked && rank && counts, "score_rows: null pointer");
    Span z;                                              // counts holds 3 V + 1 int32 entries and is indexed with int32 class ids
    SLNLP_TRY(check_logp_matrix("score_rows", logp, N, INT_MAX, V, (INT_MAX - 1) / 3, ld, &z));
    SLNLP_CHECK_ARG((((uintptr_t)logp | (uintptr_t)pred | (uintptr_t)picked | (uintptr_t)rank | (uintptr_t)counts) & 3) == 0 &&
                        ((uintptr_t)y & 7) == 0,
                    "score_rows: misaligned pointer");
    const size_t n = (size_t)N, n_counts = 3 * (size_t)V + 1;
    const Span in[2] = {z, {y, n * 8, "y"}};
    const Span out[4] = {{pred, n * 4, "pred"}, {picked, n * 4, "picked"}, {rank, n * 4, "rank"}, {counts, n_counts * 4, "counts"}};
    SLNLP_TRY(check_no_overlap("score_rows", out, in));
    const int zero_blocks = (int)std::min<size_t>((n_counts + 255) / 256, SCORE_ZERO_MAX_BLOCKS);
    SLNLP_TRY(zlaunch(score_zero_kernel, dim3(zero_blocks), 256, 0, st, "score_zero", counts, (int)n_counts));
    return zlaunch(score_rows_kernel, dim3(wave_rows_grid(N)), 256, 0, st, "score_rows", logp, (long)ld, y, (int)N, V, pred, picked, rank, counts);
}

// ---------------------------------------------------------------------------------------------- leave-one-out objective ----
// What a search over candidate metrics ranks by (slnlp.fit_field_weights): the rows whose arg-max is the label and the fp64 sum
// of -logp[i, y_i], into slot `slot` of a device table of 32-byte slots -- int64 right | fp64 sum | int64 NaN rows | int64 labels
// outside 0..V-1 -- so the candidates of a step fill one table and the host downloads it once.  ONE block: thread t takes the rows
// t, t + 256, ... in increasing order (a row's columns in order, the first maximum wins: the lowest index on a tie, as
// score_rows), then block_tree adds the 256 threads -- an order that depends on N alone, so the sum's bits are a function of the
// log-probs.  A row that holds a NaN is wrong, adds nothing and is counted; so is a row whose label lies outside the classes.
__device__ __forceinline__ void loo_objective_body(const float* __restrict__ logp, long ld, const int64_t* __restrict__ y, int N, int V,
                                                   int64_t* __restrict__ slot) {
    __shared__ double sum[256];
    __shared__ int cnt[3][256];
    const int tid = threadIdx.x;
    double acc = 0.0;
    int right = 0, nans = 0, bad = 0;
    for (long r = tid; r < N; r += 256) {
        const float* row = logp + r * ld;
        float bv = row[0];
        int bi = 0;
        bool nan = bv != bv;
        for (int j = 1; j < V; ++j) {
            const float x = row[j];
            nan |= x != x;
            if (x > bv) { bv = x; bi = j; }
        }
        const int64_t label = y[r];
        if (nan) {
            ++nans;
        } else if (label < 0 || label >= V) {
            ++bad;
        } else {
            right += bi == label ? 1 : 0;
            acc += -(double)row[label];
        }
    }
    sum[tid] = acc;
    cnt[0][tid] = right;
    cnt[1][tid] = nans;
    cnt[2][tid] = bad;
    block_tree<1>(&sum, tid, TreeSum{});
    block_tree<3>(cnt, tid, TreeSum{});
    if (tid == 0) {
        slot[0] = cnt[0][0];
        slot[1] = __builtin_bit_cast(int64_t, sum[0]);
        slot[2] = cnt[1][0];
        slot[3] = cnt[2][0];
    }
}
SLNLP_ZKERNEL(loo_objective_kernel, 256, loo_objective_body)

int loo_objective(const float* logp, int64_t ld, const int64_t* y, int64_t N, int64_t V, void* table, int64_t C, int64_t slot, hipStream_t st) {
    const char* what = "loo_objective";
    SLNLP_CHECK_ARG(logp && y && table, "%s: null pointer", what);
    Span z;
    SLNLP_TRY(check_logp_matrix(what, logp, N, INT_MAX, V, INT_MAX, ld, &z));
    SLNLP_CHECK_ARG(C >= 1 && C <= SLNLP_LOO_MAX_SLOTS, "%s: C=%ld slots outside 1..%d", what, (long)C, SLNLP_LOO_MAX_SLOTS);
    SLNLP_CHECK_ARG(slot >= 0 && slot < C, "%s: slot=%ld outside 0..C-1=%ld", what, (long)slot, (long)(C - 1));
    SLNLP_CHECK_ARG(((uintptr_t)logp & 3) == 0 && (((uintptr_t)y | (uintptr_t)table) & 7) == 0, "%s: misaligned pointer (logp: 4 bytes; y, table: 8 bytes)",
                    what);
    const Span in[2] = {z, {y, (size_t)N * 8, "y"}};
    const Span out[1] = {{table, (size_t)C * SLNLP_LOO_SLOT_BYTES, "table"}};
    SLNLP_TRY(check_no_overlap(what, out, in));
    return zlaunch(loo_objective_kernel, dim3(1), 256, 0, st, what, logp, (long)ld, y, (int)N, (int)V,
                   (int64_t*)((char*)table + slot * SLNLP_LOO_SLOT_BYTES));
}

}  // namespace slnlp

extern "C" int slnlp_loo_objective(const float* logp, int64_t ld, const int64_t* y, int64_t N, int64_t V, void* table, int64_t C, int64_t slot,
                                   void* stream) {
    return slnlp::loo_objective(logp, ld, y, N, V, table, C, slot, (hipStream_t)stream);
}
extern "C" int slnlp_score_rows(const float* logp, int64_t ld, const int64_t* y, int64_t N, int V, int32_t* pred, float* picked,
                                int32_t* rank, int32_t* counts, void* stream) {
    return slnlp::score_rows(logp, ld, y, N, V, pred, picked, rank, counts, (hipStream_t)stream);
}
